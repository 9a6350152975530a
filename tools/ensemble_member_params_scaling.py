"""What per-member Arrhenius parameters cost in an ensemble call (kin_solve_ensemble_continuous_params / _discrete_params).
Workloads: DESIGN 3.5b's (continuous: member m ramps from 900 K to 1000 + 300 m / (K - 1) K over the 2 ms span) and 3.5c's
(discrete: member m ramps from 900 K to 1 100 K at 1e5 + 4e5 m / (K - 1) K/s, ts_update = 2e-5 s: 21-101 stops), the
300-species synthetic CRN, K = 256 and 1 024, 1 ms chunks. Forms:
  existing  (a) the existing entry (the handle's parameters for all members);
  copies    (b) the _params entry given K copies of the handle's parameters - the arithmetic of (a): (b) against (a) isolates
                what the per-member pointers and the upload of the [K][R] blocks cost. (a) and (b) run alternately, REPS times
                each; walls are medians, spread_a = (max - min) / median of (a)'s walls;
  distinct  (c) the _params entry with parameters of every member's own (barriers off by up to 3 kJ/mol, prefactors by up to
                e): another problem per member, so its wall is reported with the members' steps, not as a ratio to judge;
  parent    (a) again with another build of the library (--parent-lib: the parent commit's libkinetica_hip.so), REPS times
                in a child process of the same session: has the existing entry moved?
Usage: python tools/ensemble_member_params_scaling.py [out.jsonl] [--K 256,1024] [--kinds continuous,discrete] [--reps 5] [--parent-lib PATH]
       [--append]
(default profiles/ensemble_member_params.jsonl; --append: a repeated run's rows behind those already there)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kinetica_jl_amd import capi  # noqa: E402
from kinetica_jl_amd.conditions import create_savepoints  # noqa: E402
from kinetica_jl_amd.synth import synthetic_crn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "ensemble_member_params.jsonl"))
ap.add_argument("--K", default="256,1024")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kinds", default="continuous,discrete")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--append", action="store_true", help="add the rows to the file (a repeated run) instead of replacing it")
ap.add_argument("--existing-only", action="store_true", help="time form (a) alone and print one JSON line per row (the child of --parent-lib)")
args = ap.parse_args()
N_SPECIES, T1_SPAN, TS_UPDATE = 300, 2e-3, 2e-5
Ks = [int(x) for x in args.K.split(",")]
p = capi.KinParams(tspan0=0.0, tspan1=T1_SPAN, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1, ban_negatives=0,
                   solve_chunkstep=1e-3, maxiters=100000, save_interval=-1.0, dtmin=0.0)


def inputs(kind, K):
    if kind == "continuous":
        T1 = 1000.0 + 300.0 * np.arange(K) / max(K - 1, 1)
        return [(np.array([0.0, T1_SPAN]), np.array([900.0, T1[m]])) for m in range(K)]
    out = []
    for m in range(K):
        rate = 1e5 + 4e5 * m / max(K - 1, 1)
        ts = create_savepoints(0.0, 200.0 / rate, TS_UPDATE)
        out.append((ts, np.minimum(900.0 + rate * ts, 1100.0)))
    return out


def timed(fn):
    t0 = time.perf_counter(); r = fn(); return time.perf_counter() - t0, r


def summary(walls, K, res):
    steps = [s["n_steps"] for s in res[4]]
    w = float(np.median(walls))
    return {"wall_s": w, "walls_s": walls, "solves_per_s": K / w, "ok": int((np.asarray(res[3]) == 0).sum()),
            "steps_mean": float(np.mean(steps)), "steps_max": int(max(steps))}


net, Ea, A = synthetic_crn(N_SPECIES, 5 * N_SPECIES)
h = capi.HipNetwork.from_flat(net)
h.set_arrhenius(Ea, A, k_max=1e12)
rows = []
for kind in args.kinds.split(","):
    solve = h.solve_ensemble_continuous if kind == "continuous" else h.solve_ensemble_discrete
    for K in Ks:
        U0 = np.zeros((K, N_SPECIES)); U0[:, 0] = 1.0
        pairs = inputs(kind, K)
        run_a = lambda: solve(p, U0, pairs)
        run_a()                                                            # warm-up (symbolic analysis, workspaces)
        if args.existing_only:
            wa = []
            for _ in range(args.reps):
                w, ra = timed(run_a); wa.append(w)
            print(json.dumps({"kind": kind, "K": K, "existing": summary(wa, K, ra)}), flush=True)
            continue
        EaC, AC = np.tile(Ea, (K, 1)), np.tile(A, (K, 1))
        rng = np.random.default_rng(11)
        EaD, AD = Ea[None, :] + rng.uniform(-3e3, 3e3, (K, len(Ea))), A[None, :] * np.exp(rng.uniform(-1.0, 1.0, (K, len(A))))
        run_b = lambda: solve(p, U0, pairs, Ea=EaC, A=AC)
        run_c = lambda: solve(p, U0, pairs, Ea=EaD, A=AD)
        run_b()
        wa, wb = [], []
        for _ in range(args.reps):                                         # (a) and (b) alternated
            w, ra = timed(run_a); wa.append(w)
            w, rb = timed(run_b); wb.append(w)
        run_c()
        wc, rc = timed(run_c)
        a, b = summary(wa, K, ra), summary(wb, K, rb)
        rows.append({"species": N_SPECIES, "kind": kind, "K": K, "reps": args.reps, "bytes_member_params": 16 * K * len(Ea),
                     "existing": a, "copies": b, "distinct": summary([wc], K, rc),
                     "copies_bit_identical_to_existing": bool(np.array_equal(ra[1], rb[1])),
                     "spread_existing": (max(wa) - min(wa)) / a["wall_s"],
                     "ratio_wall_copies_over_existing": b["wall_s"] / a["wall_s"]})
h.close()
if not args.existing_only:
    parent = {}
    if args.parent_lib:
        # the parent's library in a fresh process (one library per process), this binding, the same session
        env = dict(os.environ, KIN_LIB_PATH=os.path.abspath(args.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only", "--K", args.K, "--reps", str(args.reps), "--kinds",
                              args.kinds],
                             env=env, capture_output=True, text=True, check=True).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                parent[(r["kind"], r["K"])] = r["existing"]
    with open(args.out, "a" if args.append else "w") as f:
        for r in rows:
            q = parent.get((r["kind"], r["K"]))
            if q is not None:
                r["parent_existing"] = q
                r["spread_parent"] = (max(q["walls_s"]) - min(q["walls_s"])) / q["wall_s"]
                r["ratio_wall_existing_over_parent"] = r["existing"]["wall_s"] / q["wall_s"]
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")
