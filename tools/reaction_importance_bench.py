"""Reaction-importance pass against the DRG pass, alternated in one process (DESIGN 3.1i quotes the result). Each shape:
kin_reaction_importance_batched_dev (every species selected, and a third of them through the device mask), kin_drg_batched_dev
and, for scale, stage 1 alone (kin_drgep_batched_dev ended after the flux sweep, KIN_DRGEP_STAGES=1) on the same
device-resident states with the handle's rate constants, pairing on, HIP events, after a 1 s spin-up and a warm-up of the
shape, ALT alternations of REPS calls each; medians and spread of the per-call times.
Usage: python tools/reaction_importance_bench.py [--out profiles/reaction_importance_ab.txt] [--shapes 300,1k,10k]"""
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

ALT, REPS = 7, 5


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reaction_importance_ab.txt"))
    ap.add_argument("--shapes", default="300,1k,10k")
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
    lines = [f"# tools/reaction_importance_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations x {REPS} calls, per-call "
             f"times (median [min, max]); states 10^U(-12, 0), the handle's rate constants (Arrhenius at 1000 K, k_max 1e12), "
             f"pairing on; 'third': a random third of the species selected through the device mask"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    cases = [("300", 300, 1500, 4096), ("1k", 1000, 5000, 1024), ("10k", 10000, 50000, 1024)]
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
        plan = capi.reaction_importance_plan_host(net, 1)[3]
        coef = torch.empty((max(info["edges"], 1),), dtype=torch.float64, device=dev)
        imp = torch.empty((R,), dtype=torch.float64, device=dev)
        imp3 = torch.empty((R,), dtype=torch.float64, device=dev)
        spn = torch.empty((N,), dtype=torch.float64, device=dev)
        third = np.sort(np.random.default_rng(3).choice(N, N // 3, replace=False)).astype(np.int64)
        d_third = torch.tensor(third, dtype=torch.int64, device=dev)
        tg = torch.tensor([0], dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def stage1():
            os.environ["KIN_DRGEP_STAGES"] = "1"
            h.drgep_batched_dev(B, u.data_ptr(), tg.data_ptr(), 1, spn.data_ptr(), pairing=True, stream=s)
            os.environ.pop("KIN_DRGEP_STAGES", None)

        fns = {"stage 1": stage1,
               "importance": lambda: h.reaction_importance_batched_dev(B, u.data_ptr(), imp.data_ptr(), pairing=True, stream=s),
               "drg": lambda: h.drg_batched_dev(B, u.data_ptr(), coef.data_ptr(), pairing=True, stream=s),
               "third": lambda: h.reaction_importance_batched_dev(B, u.data_ptr(), imp3.data_ptr(), d_species=d_third.data_ptr(),
                                                                  n_sel=len(third), pairing=True, stream=s)}
        for f in fns.values():
            f(); f()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(ALT):
            for k, f in fns.items():
                ts[k].append(timed(f, st))
        imp_h, imp3_h = imp.cpu().numpy(), imp3.cpu().numpy()
        assert np.all(imp_h >= 0) and np.all(imp_h <= 1) and np.all(imp3_h <= imp_h)
        emit(f"{name:4s} N={N} R={R} B={B}  records {plan['records']}, den contributions {info['den_contributions']}, edges {info['edges']}, "
             f"edge contributions {info['edge_contributions']}")
        med = {k: stats(v)[0] for k, v in ts.items()}
        for k in fns:
            m, lo, hi = stats(ts[k])
            emit(f"  {k:10s} {m * 1e3:9.3f} ms [{lo * 1e3:.3f}, {hi * 1e3:.3f}]  {m / med['drg']:6.2f} x drg")
        emit(f"  by difference: importance's stages 2-3 {1e3 * (med['importance'] - med['stage 1']):.3f} ms, drg's stage 2 "
             f"{1e3 * (med['drg'] - med['stage 1']):.3f} ms; importance >= 0.02: {int(np.sum(imp_h >= 0.02))} of {R} reactions, "
             f"judged by the third: {int(np.sum(imp3_h >= 0.02))}")
        h.close()
        del u
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
