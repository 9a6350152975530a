"""DRGEP pass, stage by stage, against the DRG pass, alternated in one process (DESIGN 3.1f quotes the result). Each shape:
kin_drgep_batched_dev ended after stage 1 (the flux sweep), after stage 2 (den and r) and complete (KIN_DRGEP_STAGES=1, 2,
unset), and kin_drg_batched_dev, pairing on, 3 targets, on the same states with the handle's rate constants, HIP events, after
a 1 s spin-up and a warm-up of the shape, ALT alternations of REPS calls each; medians and spread of the per-call times, and
the stages as differences of the medians. The rounds per state come from the host entry (kin_drgep_batched with rounds_out)
on the first ROUND_STATES states.
Usage: python tools/drgep_bench.py [--out profiles/drgep_ab.txt] [--shapes 10k,50k]"""
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

ALT, REPS, ROUND_STATES = 5, 3, 64
TARGETS = np.array([0, 1, 2], np.int64)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drgep_ab.txt"))
    ap.add_argument("--shapes", default="10k,50k")
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
    lines = [f"# tools/drgep_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations x {REPS} calls, per-call times "
             f"(median [min, max]); 1024 states 10^U(-12, 0), the handle's rate constants (Arrhenius at 1000 K, k_max 1e12), "
             f"pairing on, targets 0, 1, 2; rounds per state over the first {ROUND_STATES} states"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    cases = [("10k", 10000, 50000, 1024), ("50k", 50000, 250000, 1024)]
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
        info = capi.drg_pattern_host(net, 1)[2]
        coef = torch.empty((max(info["edges"], 1),), dtype=torch.float64, device=dev)
        imp = torch.empty((N,), dtype=torch.float64, device=dev)
        tg = torch.tensor(TARGETS, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        def drgep(upto):
            def run():
                if upto:
                    os.environ["KIN_DRGEP_STAGES"] = str(upto)
                else:
                    os.environ.pop("KIN_DRGEP_STAGES", None)
                h.drgep_batched_dev(B, u.data_ptr(), tg.data_ptr(), len(TARGETS), imp.data_ptr(), pairing=True, stream=s)
                os.environ.pop("KIN_DRGEP_STAGES", None)
            return run

        fns = {"stage 1": drgep(1), "stages 1-2": drgep(2), "drgep": drgep(0),
               "drg": lambda: h.drg_batched_dev(B, u.data_ptr(), coef.data_ptr(), pairing=True, stream=s)}
        for f in fns.values():
            f(); f()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(ALT):
            for k, f in fns.items():
                ts[k].append(timed(f, st))
        nr = min(ROUND_STATES, B)
        imp_h, _, _, rounds = h.drgep_batched(u[:nr].cpu().numpy(), TARGETS, pairing=True, stages=True)
        emit(f"{name:4s} N={N} R={R} B={B}  edges {info['edges']}, contributions den / edge {info['den_contributions']} / "
             f"{info['edge_contributions']}; search in {'LDS' if N <= 4080 else 'global memory'}")
        med = {k: stats(v)[0] for k, v in ts.items()}
        for k in fns:
            m, lo, hi = stats(ts[k])
            emit(f"  {k:10s} {m * 1e3:9.3f} ms [{lo * 1e3:.3f}, {hi * 1e3:.3f}]  {m / med['stage 1']:6.2f} x stage 1")
        emit(f"  by difference: stage 2 {1e3 * (med['stages 1-2'] - med['stage 1']):.3f} ms, path stage "
             f"{1e3 * (med['drgep'] - med['stages 1-2']):.3f} ms; drg's stage 2 {1e3 * (med['drg'] - med['stage 1']):.3f} ms; "
             f"drgep / drg = {med['drgep'] / med['drg']:.2f}")
        emit(f"  rounds per state (min / median / max): {int(rounds.min())} / {int(np.median(rounds))} / {int(rounds.max())}; importance: "
             f"median {np.median(imp_h):.2e}, 90th percentile {np.percentile(imp_h, 90):.2e}")
        h.close()
        del u
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
