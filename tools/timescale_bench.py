"""Timescale pass against the directed-relation-graph pass, alternated in one process per shape (DESIGN 3.1g quotes the result).
Each shape: kin_drg_batched_dev (pairing on), kin_timescale_batched_dev (summary + norm) and kin_jac_batched_dev on the same
states with the handle's rate constants, HIP events, after a 1 s spin-up and a warm-up of the shape, ALT alternations of REPS
calls each; medians and spread of the per-call times, next to the algorithmic bytes per state of the two new passes. Every
shape is a leg: a child process of its own under its own time limit; a leg that fails or runs out of time ends the run.
Usage: python tools/timescale_bench.py [--out profiles/timescale_ab.txt] [--shapes 10k,300] [--limit 240]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALT, REPS = 5, 3
# name: species, reactions, states
SHAPES = {"10k": (10000, 50000, 1024), "300": (300, 1500, 4096)}


def algorithmic_bytes(net, nnz):
    """(timescale, jac) bytes per state that the passes cannot avoid: stage 1 reads u and writes rates and dr (the rate constants
    are one shared row); the entry gather reads one dr per contribution and writes the entries; the row pass reads the entries and
    one rate per (species, reaction) term and writes g; the norm reads g. jac: stage 1 without the rates, and the entry gather."""
    N, R = net.n_species, net.n_reactions
    contrib = terms = 0
    for r in range(R):
        reac, prod = net.reaction(r)
        nu = {}
        for s, c in reac:
            nu[int(s)] = nu.get(int(s), 0) - int(c)
        for s, c in prod:
            nu[int(s)] = nu.get(int(s), 0) + int(c)
        rows = sum(1 for v in nu.values() if v != 0)
        cols = 2 if len(reac) == 2 else 1
        terms += rows
        contrib += rows * cols
    stage1 = 8 * (N + 2 * R)
    entries = 8 * (contrib + nnz)
    return stage1 + 8 * R + entries + 8 * (nnz + terms + N) + 8 * N, stage1 + entries, contrib, terms


def leg(name):
    import numpy as np
    import torch
    from kinetica_jl_amd import capi
    from kinetica_jl_amd.synth import synthetic_crn

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

    N, R, B = SHAPES[name]
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    x = torch.rand((4096, 4096), device=dev)      # spin-up: the clocks settle under load
    t0 = time.time()
    while time.time() - t0 < 1.0:
        x = x @ x * 1e-4
        torch.cuda.synchronize()
    net, Ea, A = synthetic_crn(N, R)
    plan = capi.timescale_plan_host(net)
    nnz = plan["nnz"]
    b_ts, b_jac, contrib, terms = algorithmic_bytes(net, nnz)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    h.rates_at(1000.0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    u = torch.pow(10.0, torch.rand((B, N), dtype=torch.float64, device=dev, generator=g) * 12 - 12)
    edges = capi.drg_pattern_host(net, 1)[2]["edges"]
    coef = torch.empty((max(edges, 1),), dtype=torch.float64, device=dev)
    summary = torch.empty((3, N), dtype=torch.float64, device=dev)
    norm = torch.empty((B,), dtype=torch.float64, device=dev)
    vals = torch.empty((B, nnz), dtype=torch.float64, device=dev)
    s = st.cuda_stream
    torch.cuda.synchronize()
    timescale = lambda: h.timescale_batched_dev(B, u.data_ptr(), d_summary=summary.data_ptr(), d_norm=norm.data_ptr(), stream=s)

    def staged(n):      # the timescale call ended after stage n of every block (KIN_TS_STAGES: read per call, a knob for timing)
        def fn():
            os.environ["KIN_TS_STAGES"] = str(n)
            try:
                timescale()
            finally:
                del os.environ["KIN_TS_STAGES"]
        return fn

    fns = {"drg pairing": lambda: h.drg_batched_dev(B, u.data_ptr(), coef.data_ptr(), pairing=True, stream=s),
           "timescale": timescale, "ts stage 1": staged(1), "ts stages 1-2": staged(2),
           "jac": lambda: h.jac_batched_dev(B, u.data_ptr(), vals.data_ptr(), stream=s)}
    for f in fns.values():
        f(); f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(ALT):
        for k, f in fns.items():
            ts[k].append(timed(f, st))
    print(f"{name:5s} N={N} R={R} B={B}  nnz {nnz}, contributions {contrib}, RHS terms {terms}, rows short / medium / long "
          f"{plan['rows_short']} / {plan['rows_medium']} / {plan['rows_long']}; DRG edges {edges}; {torch.cuda.get_device_name(0)}")
    base = stats(ts["drg pairing"])[0]
    per_state = {"timescale": b_ts, "jac": b_jac}
    for k in fns:
        m, lo, hi = stats(ts[k])
        by = per_state.get(k)
        tail = "" if by is None else f"  {by} B/state algorithmic, {by * B / m * 1e-9:.1f} GB/s of them"
        print(f"  {k:12s} {m * 1e3:9.3f} ms [{lo * 1e3:.3f}, {hi * 1e3:.3f}]  {m / base:6.2f} x drg{tail}")
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timescale_ab.txt"))
    ap.add_argument("--shapes", default="10k,300")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a leg may take")
    ap.add_argument("--leg", default=None, help="(internal) run one shape in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg)
        return 0
    lines = [f"# tools/timescale_bench.py: {ALT} alternations x {REPS} calls, per-call times (median [min, max]); states 10^U(-12, 0), "
             f"the handle's rate constants (Arrhenius at 1000 K, k_max 1e12); timescale = summary + norm, drg = pairing on"]
    rc = 0
    for name in args.shapes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: no result within {args.limit:.0f} s; nothing was started after it")
            rc = 1
            break
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            lines.append(f"{name}: the leg ended with status {p.returncode}; nothing was started after it")
            rc = 1
            break
        lines += p.stdout.rstrip("\n").split("\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
