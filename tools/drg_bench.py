"""Directed-relation-graph pass against the flux pass that is its first stage, alternated in one process (DESIGN 3.1e quotes
the result). Each shape: kin_drg_batched_dev (pairing on and off) and kin_flux_batched_dev with the per-state rates wanted, on
the same states with the handle's rate constants, HIP events, after a 1 s spin-up and a warm-up of the shape, ALT alternations
of REPS calls each; medians and spread of the per-call times.
Usage: python tools/drg_bench.py [--out profiles/drg_ab.txt] [--shapes c3,ens300]"""
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

ALT, REPS = 5, 3


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drg_ab.txt"))
    ap.add_argument("--shapes", default="c3,ens300")
    args = ap.parse_args()
    want = args.shapes.split(",")
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    x = torch.rand((4096, 4096), device=dev)      # spin-up: the clocks settle under load
    t0 = time.time()
    while time.time() - t0 < 1.0:
        x = x @ x * 1e-4
        torch.cuda.synchronize()
    lines = [f"# tools/drg_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations x {REPS} calls, per-call seconds "
             f"(median [min, max]); states 10^U(-12, 0), the handle's rate constants (Arrhenius at 1000 K, k_max 1e12)"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    # name, species, reactions, states (ens300: K = 1 024 members x 101 rows of a stored ensemble, as one batch)
    cases = [("c3", 10000, 50000, 4096), ("ens300", 300, 1500, 1024 * 101)]
    for name, N, R, B in cases:
        if name not in want:
            continue
        net, Ea, A = synthetic_crn(N, R)
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        h.rates_at(1000.0)
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        u = torch.pow(10.0, torch.rand((B, N), dtype=torch.float64, device=dev, generator=g) * 12 - 12)
        rates = torch.empty((B, R), dtype=torch.float64, device=dev)
        s = st.cuda_stream
        info = {p: capi.drg_pattern_host(net, p)[2] for p in (1, 0)}
        coef = {p: torch.empty((max(info[p]["edges"], 1),), dtype=torch.float64, device=dev) for p in (1, 0)}
        torch.cuda.synchronize()
        fns = {"drg pairing": lambda: h.drg_batched_dev(B, u.data_ptr(), coef[1].data_ptr(), pairing=True, stream=s),
               "drg single": lambda: h.drg_batched_dev(B, u.data_ptr(), coef[0].data_ptr(), pairing=False, stream=s),
               "flux+rates": lambda: h.flux_batched_dev(B, u.data_ptr(), d_rates=rates.data_ptr(), stream=s)}
        for f in fns.values():
            f(); f()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(ALT):
            for k, f in fns.items():
                ts[k].append(timed(f, st))
        emit(f"{name:8s} N={N} R={R} B={B}  edges {info[1]['edges']}, contributions den / edge: pairing {info[1]['den_contributions']} / "
             f"{info[1]['edge_contributions']}, single {info[0]['den_contributions']} / {info[0]['edge_contributions']}")
        base = stats(ts["flux+rates"])[0]
        for k in fns:
            m, lo, hi = stats(ts[k])
            emit(f"  {k:12s} {m * 1e3:9.3f} ms [{lo * 1e3:.3f}, {hi * 1e3:.3f}]  {m / base:6.2f} x flux+rates")
        h.close()
        del u, rates
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
