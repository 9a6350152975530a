"""PFA pass, stage by stage, against the DRG pass, alternated in one process (DESIGN 3.1h quotes the result). Each shape:
kin_pfa_batched_dev ended after stage 1 (the flux sweep), after the split stage (den, rp and rc) and complete
(KIN_PFA_STAGES=1, 2, unset), the complete pass with every row given to a workgroup and with every row given to a single
wavefront (KIN_PFA_WG_COST=0 and 10^12), and kin_drg_batched_dev, pairing on, on the same states with the handle's rate
constants, HIP events, after a 1 s spin-up and a warm-up of the shape, ALT alternations of REPS calls each; medians and spread
of the per-call times, the stages as differences of the medians, and the second-generation stage's products per second.
Usage: python tools/pfa_bench.py [--out profiles/pfa_ab.txt] [--shapes 300,1000,10k]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfa_ab.txt"))
    ap.add_argument("--shapes", default="300,1000,10k")
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
    lines = [f"# tools/pfa_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations x {REPS} calls, per-call times "
             f"(median [min, max]); states 10^U(-12, 0), the handle's rate constants (Arrhenius at 1000 K, k_max 1e12), pairing on"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    cases = [("300", 300, 1500, 4096), ("1000", 1000, 5000, 1024), ("10k", 10000, 50000, 64)]
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
        s = st.cuda_stream
        info = capi.pfa_pattern_host(net, 1)[2]
        coef = torch.empty((max(info["edges"], 1),), dtype=torch.float64, device=dev)
        coef2 = torch.empty((max(info["pairs"], 1),), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def pfa(upto, wg_cost=None):
            def run():
                if upto:
                    os.environ["KIN_PFA_STAGES"] = str(upto)
                if wg_cost is not None:
                    os.environ["KIN_PFA_WG_COST"] = str(wg_cost)
                h.pfa_batched_dev(B, u.data_ptr(), coef2.data_ptr(), pairing=True, stream=s)
                os.environ.pop("KIN_PFA_STAGES", None)
                os.environ.pop("KIN_PFA_WG_COST", None)
            return run

        fns = {"stage 1": pfa(1), "stages 1-2": pfa(2), "pfa": pfa(0), "pfa, all wg": pfa(0, 0), "pfa, all wave": pfa(0, 10 ** 12),
               "drg": lambda: h.drg_batched_dev(B, u.data_ptr(), coef.data_ptr(), pairing=True, stream=s)}
        for f in fns.values():
            f(); f()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(ALT):
            for k, f in fns.items():
                ts[k].append(timed(f, st))
        emit(f"{name:4s} N={N} R={R} B={B}  edges {info['edges']}, pairs {info['pairs']}, products per state {info['products']}, "
             f"largest row of E {info['max_row']}")
        med = {k: stats(v)[0] for k, v in ts.items()}
        for k in fns:
            m, lo, hi = stats(ts[k])
            emit(f"  {k:14s} {m * 1e3:9.3f} ms [{lo * 1e3:.3f}, {hi * 1e3:.3f}]  {m / med['stage 1']:7.2f} x stage 1")
        second = med["pfa"] - med["stages 1-2"]
        emit(f"  by difference: split stage {1e3 * (med['stages 1-2'] - med['stage 1']):.3f} ms, second-generation stage "
             f"{1e3 * second:.3f} ms ({B * info['products'] / second * 1e-9:.1f} G products/s, all wg "
             f"{1e3 * (med['pfa, all wg'] - med['stages 1-2']):.3f} ms, all wave {1e3 * (med['pfa, all wave'] - med['stages 1-2']):.3f} ms); "
             f"drg's stage 2 {1e3 * (med['drg'] - med['stage 1']):.3f} ms; pfa / drg = {med['pfa'] / med['drg']:.2f}")
        h.close()
        del u
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
