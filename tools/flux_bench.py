"""Reaction-flux pass against the batched RHS sweep, alternated in one process (DESIGN 3.1c quotes the result).
Each shape: kin_flux_batched_dev (flux only) and kin_rhs_batched_dev on the same buffers, HIP events, after a 1 s
spin-up and a warm-up of the shape, ALT alternations of REPS launches each; medians and spread of the per-launch times.
Usage: python tools/flux_bench.py [--out profiles/flux_sweep_ab.txt] [--shapes c3,c2,c3_shared,c3_T,c3_rates,c5]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import synthetic_crn

ALT, REPS, PEAK = 6, 5, 8.0e12


def timed(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(REPS):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / REPS


def stats(x):
    x = np.sort(np.asarray(x))
    return float(np.median(x)), float(x[0]), float(x[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_sweep_ab.txt"))
    ap.add_argument("--shapes", default="c3,c2,c3_shared,c3_T,c3_rates,c5")
    args = ap.parse_args()
    want = args.shapes.split(",")
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    # spin-up: the clocks settle under load
    x = torch.rand((4096, 4096), device=dev)
    t0 = time.time()
    while time.time() - t0 < 1.0:
        x = x @ x * 1e-4
        torch.cuda.synchronize()
    lines = [f"# tools/flux_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations x {REPS} launches, per-launch seconds "
             f"(median [min, max]); GB/s = algorithmic bytes / median; share of {PEAK / 1e12:.0f} TB/s"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    nets = {}

    def net_of(N, R):
        if (N, R) not in nets:
            net, Ea, A = synthetic_crn(N, R)
            h = capi.HipNetwork.from_flat(net)
            h.set_arrhenius(Ea, A, k_max=1e12)
            h.rates_at(1000.0)
            nets[(N, R)] = h
        return nets[(N, R)]

    cases = [("c3", 10000, 50000, 4096, "k"), ("c2", 1000, 5000, 4096, "k"), ("c3_shared", 10000, 50000, 4096, "shared"),
             ("c3_T", 10000, 50000, 4096, "T"), ("c3_rates", 10000, 50000, 4096, "k+rates"), ("c5", 50000, 250000, 1024, "k")]
    for name, N, R, B, form in cases:
        if name not in want:
            continue
        h = net_of(N, R)
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        u = torch.pow(10.0, torch.rand((B, N), dtype=torch.float64, device=dev, generator=g) * 12 - 12)
        k = torch.rand((B, R), dtype=torch.float64, device=dev, generator=g) + 0.5
        T = torch.linspace(600.0, 1200.0, B, dtype=torch.float64, device=dev)
        w = torch.rand((B,), dtype=torch.float64, device=dev, generator=g)
        du = torch.empty_like(u)
        flux = torch.empty((R,), dtype=torch.float64, device=dev)
        rates = torch.empty((B, R), dtype=torch.float64, device=dev) if form == "k+rates" else None
        torch.cuda.synchronize()
        s = st.cuda_stream
        if form in ("k", "k+rates"):
            f = lambda: h.flux_batched_dev(B, u.data_ptr(), d_k=k.data_ptr(), d_w=w.data_ptr(), d_flux=flux.data_ptr(),
                                           d_rates=rates.data_ptr() if rates is not None else 0, stream=s)
            alg_f = B * (8 * R + 8 * N) + 8 * R + (8 * B * R if rates is not None else 0)
        elif form == "shared":
            f = lambda: h.flux_batched_dev(B, u.data_ptr(), d_w=w.data_ptr(), d_flux=flux.data_ptr(), stream=s)
            alg_f = B * 8 * N + 24 * R
        else:
            f = lambda: h.flux_batched_dev(B, u.data_ptr(), d_T=T.data_ptr(), d_w=w.data_ptr(), d_flux=flux.data_ptr(), stream=s)
            alg_f = B * 8 * N + 24 * R
        # the yardstick: the sweep at the same shape with the same kind of rate constants (per-state k, or the handle's)
        r = lambda: h.rhs_batched_dev(B, u.data_ptr(), k.data_ptr() if form in ("k", "k+rates") else 0, du.data_ptr(), s)
        alg_r = B * ((8 * R if form in ("k", "k+rates") else 0) + 16 * N) + 20 * R
        for _ in range(3):
            f(); r()
        torch.cuda.synchronize()
        tf, tr = [], []
        for _ in range(ALT):
            tf.append(timed(f, st))
            tr.append(timed(r, st))
        mf, lf, hf = stats(tf)
        mr, lr, hr = stats(tr)
        bound = {"T": " (VALU bound: no HBM share claimed)", "shared": ""}.get(form, "")
        if name == "c5":
            bound = " (gather path, L2 bound: no HBM share claimed)"
        emit(f"{name:10s} N={N} R={R} B={B} form={form}")
        emit(f"  flux   {mf * 1e3:8.3f} ms [{lf * 1e3:.3f}, {hf * 1e3:.3f}]  {alg_f / mf / 1e9:7.0f} GB/s  {100 * alg_f / mf / PEAK:5.1f} %{bound}")
        emit(f"  sweep  {mr * 1e3:8.3f} ms [{lr * 1e3:.3f}, {hr * 1e3:.3f}]  {alg_r / mr / 1e9:7.0f} GB/s  {100 * alg_r / mr / PEAK:5.1f} %")
        emit(f"  flux / sweep = {mf / mr:.3f}")
        del u, k, du, rates
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    for h in nets.values():
        h.close()


if __name__ == "__main__":
    main()
