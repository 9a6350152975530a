"""Scaling of kin_solve_ensemble_discrete (one stop schedule per member) against the ways to get the same answers without it.
Networks: the 300- and 1 000-species synthetic CRNs, K = 1, 64, 256, 1 024; 2 ms span, 1 ms chunks. Member m ramps from 900 K
to 1 100 K at its own rate, 1e5 + 4e5 m / (K - 1) K/s, under discrete updates every ts_update = 2e-5 s: its stops are
create_savepoints(0, t_end, ts_update) with its own t_end = 200 K / rate (member 0: 2 ms, 101 stops; member K - 1: 0.4 ms, 21),
the temperatures the ramp's at them - what discrete_stop_temperatures gives for a LinearGradientProfile with ts_update.
Forms:
  per_member   (a)  kin_solve_ensemble_discrete with every member's own schedule;
  same_sched   (a') kin_solve_ensemble_discrete with member 0's schedule for every member;
  shared       (b)  kin_solve_ensemble with member 0's schedule shared - the same arithmetic as (a'): (a') against (b) isolates
                    what the per-member stop pointers cost. (a') and (b) run alternately, REPS times each; walls are medians;
  sequential   (c)  min(K, 16) kin_solve calls with the members' own schedules, extrapolated per solve.
us_per_member_step = wall / the accepted steps of all members together (the members of (a) take different step counts, and a
resident launch lasts as long as its slowest member). route: resident_ensemble_route's rule (resident.cpp): the one-launch form
unless N > 700 and K < 32, where the members are kin_solve calls on host threads.
Usage: python tools/ensemble_discrete_scaling.py [out.jsonl] [--species 300,1000] [--K 1,64,256,1024]
(default profiles/r07_ensemble_discrete.jsonl; --species / --K: a subset of the rows)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kinetica_jl_amd import capi  # noqa: E402
from kinetica_jl_amd.conditions import create_savepoints  # noqa: E402
from kinetica_jl_amd.synth import synthetic_crn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                      "r07_ensemble_discrete.jsonl"))
ap.add_argument("--species", default="300,1000")
ap.add_argument("--K", default="1,64,256,1024")
args = ap.parse_args()
out_path = args.out
T1_SPAN, TS_UPDATE, REPS = 2e-3, 2e-5, 3
p = capi.KinParams(tspan0=0.0, tspan1=T1_SPAN, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1, ban_negatives=0,
                   solve_chunkstep=1e-3, maxiters=100000, save_interval=-1.0, dtmin=0.0)


def schedules(K):
    out = []
    for m in range(K):
        rate = 1e5 + 4e5 * m / max(K - 1, 1)
        ts = create_savepoints(0.0, 200.0 / rate, TS_UPDATE)
        out.append((ts, np.minimum(900.0 + rate * ts, 1100.0)))
    return out


def form(w, K, rcs, sts):
    steps = [s["n_steps"] for s in sts]
    return {"wall_s": w, "solves_per_s": K / w, "ok": int((np.asarray(rcs) == 0).sum()), "steps_mean": float(np.mean(steps)),
            "steps_max": int(max(steps)), "restarts_mean": float(np.mean([s["n_restarts"] for s in sts])),
            "restarts_max": int(max(s["n_restarts"] for s in sts)), "us_per_member_step": 1e6 * w / float(np.sum(steps))}


def timed(fn):
    t0 = time.perf_counter(); r = fn(); return time.perf_counter() - t0, r


with open(out_path, "w") as f:
    for n in [int(x) for x in args.species.split(",")]:
        net, Ea, A = synthetic_crn(n, 5 * n)
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        for K in [int(x) for x in args.K.split(",")]:
            U0 = np.zeros((K, n)); U0[:, 0] = 1.0
            st = schedules(K)
            s0 = [st[0]] * K
            run_a = lambda: h.solve_ensemble_discrete(p, U0, st)
            run_a1 = lambda: h.solve_ensemble_discrete(p, U0, s0)
            run_b = lambda: h.solve_ensemble(p, U0, tstops=st[0][0], T_stops=st[0][1])
            run_a()                                                        # warm-up (symbolic analysis, workspaces)
            wa, ra = timed(run_a)
            run_a1(); run_b()
            wa1, wb = [], []
            for _ in range(REPS):                                          # (a') and (b) alternated
                w, ra1 = timed(run_a1); wa1.append(w)
                w, rb = timed(run_b); wb.append(w)
            same = bool(np.array_equal(ra1[1], rb[1]))
            Kq = min(K, 16)
            h.solve(p, U0[0], tstops=st[0][0], T_stops=st[0][1])
            t0 = time.perf_counter()
            q_sts, q_rcs = [], []
            for m in range(Kq):
                _, _, rc, sq, _ = h.solve(p, U0[m], tstops=st[m][0], T_stops=st[m][1])
                q_sts.append(sq); q_rcs.append(rc)
            wq = (time.perf_counter() - t0) / Kq
            r = {"species": n, "K": K, "route": "threads" if (n > 700 and K < 32) else "resident", "lu_slots": ra[4][0]["lu_slots"],
                 "ts_update": TS_UPDATE, "stops_min": min(len(s[0]) for s in st), "stops_max": max(len(s[0]) for s in st),
                 "per_member": form(wa, K, ra[3], ra[4]),
                 "same_sched": dict(form(float(np.median(wa1)), K, ra1[3], ra1[4]), walls_s=wa1),
                 "shared": dict(form(float(np.median(wb)), K, rb[3], rb[4]), walls_s=wb),
                 "same_sched_bit_identical_to_shared": same,
                 "sequential_kin_solve": dict(form(wq * Kq, Kq, q_rcs, q_sts), members_run=Kq, wall_per_solve_s=wq),
                 "ratio_wall_same_sched_over_shared": float(np.median(wa1) / np.median(wb)),
                 "speedup_over_sequential": (K / wa) * wq}
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")
        h.close()
