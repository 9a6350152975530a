"""Scaling of kin_solve_ensemble_continuous (one temperature profile per member, resident route) against the two ways to get
the same answers without it: K sequential kin_solve_continuous calls (run for min(K, 16) members, extrapolated per solve) and the
static per-member-T ensemble at the same K (kin_solve_ensemble, each member at its ramp's mean temperature).
Networks: the 300- and 1 000-species synthetic CRNs; member m ramps linearly from 900 K to 1000 + 300 m / (K - 1) K over the
2 ms span (1 ms chunks). launch_us_per_step = wall / mean accepted steps of a member: what one step of the whole launch costs
(all K members advance together), comparable between the continuous and the static form whatever their step counts;
us_per_member_step = wall / the steps of all members together. The two forms' ratio is the same in either measure.
route: resident_ensemble_route's rule (resident.cpp) for these networks, both of which fit the resident kernel - the one-launch
form unless N > 700 and K < 32, where the members are kin_solve_continuous calls on host threads; lu_slots (at most 64 on the
resident route, more on the host-driven integrator) is recorded as the members' own evidence of it.
Usage: python tools/ensemble_continuous_scaling.py [out.jsonl]   (default profiles/r06_ensemble_continuous.jsonl)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kinetica_jl_amd import capi  # noqa: E402
from kinetica_jl_amd.synth import synthetic_crn  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                              "r06_ensemble_continuous.jsonl")
T1_SPAN = 2e-3
p = capi.KinParams(tspan0=0.0, tspan1=T1_SPAN, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1, ban_negatives=0,
                   solve_chunkstep=1e-3, maxiters=100000, save_interval=-1.0, dtmin=0.0)
recs = []
with open(out_path, "w") as f:
    for n in (300, 1000):
        net, Ea, A = synthetic_crn(n, 5 * n)
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        for K in (1, 64, 256, 1024):
            U0 = np.zeros((K, n)); U0[:, 0] = 1.0
            T1 = 1000.0 + 300.0 * np.arange(K) / max(K - 1, 1)
            nodes = [(np.array([0.0, T1_SPAN]), np.array([900.0, T1[m]])) for m in range(K)]
            Tstat = 0.5 * (900.0 + T1)
            h.solve_ensemble_continuous(p, U0, nodes)                      # warm-up (symbolic analysis, workspaces)
            t0 = time.perf_counter(); _, _, _, rcs, sts = h.solve_ensemble_continuous(p, U0, nodes); w = time.perf_counter() - t0
            h.solve_ensemble(p, U0, T=Tstat)
            t0 = time.perf_counter(); _, _, _, rcs_s, sts_s = h.solve_ensemble(p, U0, T=Tstat); ws = time.perf_counter() - t0
            Kq = min(K, 16)
            h.solve_continuous(p, U0[0], *nodes[0])
            t0 = time.perf_counter()
            q_steps = []
            for m in range(Kq):
                _, _, rc, st, _ = h.solve_continuous(p, U0[m], *nodes[m])
                q_steps.append(st["n_steps"])
            wq = (time.perf_counter() - t0) / Kq
            steps = float(np.mean([s["n_steps"] for s in sts])); steps_s = float(np.mean([s["n_steps"] for s in sts_s]))
            r = {"species": n, "K": K, "route": "threads" if (n > 700 and K < 32) else "resident", "lu_slots": sts[0]["lu_slots"],
                 "continuous": {"wall_s": w, "solves_per_s": K / w, "ok": int((rcs == 0).sum()), "steps_mean": steps,
                                "steps_max": int(max(s["n_steps"] for s in sts)), "launch_us_per_step": 1e6 * w / steps,
                                "us_per_member_step": 1e6 * w / (K * steps)},
                 "static_T": {"wall_s": ws, "solves_per_s": K / ws, "ok": int((rcs_s == 0).sum()), "steps_mean": steps_s,
                              "launch_us_per_step": 1e6 * ws / steps_s, "us_per_member_step": 1e6 * ws / (K * steps_s)},
                 "sequential_kin_solve_continuous": {"members_run": Kq, "wall_per_solve_s": wq, "solves_per_s": 1.0 / wq,
                                                     "steps_mean": float(np.mean(q_steps))},
                 "ratio_per_step_cont_over_static": (w / steps) / (ws / steps_s),
                 "speedup_over_sequential": (K / w) * wq}
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")
        h.close()
