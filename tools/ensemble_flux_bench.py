"""Per-member reaction fluxes of an ensemble, three ways, alternated in one process (DESIGN 3.1d quotes the result).
Each case solves an ensemble of K members with a 101-row save grid, then times
  1  ensemble_flux   kin_ensemble_flux on the stored ensemble: keys and weights up, ONE segmented launch, flux[K][R] down
                     (host clock around the call, which ends in a stream synchronisation);
  1d segmented_dev   the same launch alone, kin_flux_segmented_dev over a copy of the states in a buffer of the tool's
                     (device events): the kernel to set against 2;
  2  batched_dev     ONE kin_flux_batched_dev over the same K x rows states with the same per-state T: the same bytes, no
                     per-member result (one flux[R]), no reuse of rate constants between states (device events);
  3  today           what a caller did before: download out_u, then K kin_flux_batched calls, one per member (host clock;
                     the download is timed as a device-to-host copy of an array of out_u's size).
1d and 2 are timed over enough repetitions to fill about a second, 1 over a quarter of that, 3 once per alternation; ALT
alternations; medians and [min, max] of the per-call times. Bytes are algorithmic: what the form has to move, from the shapes.
Cases: static (one T per member, 300 / 1 500 and 1 000 / 5 000), discrete (300 / 1 500, 21-101 stops per member as in
profiles/r07_ensemble_discrete.jsonl).
Usage: python tools/ensemble_flux_bench.py [--out profiles/ensemble_flux_ab.txt] [--cases static300,discrete300,static1000] [--K 1024]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.conditions import create_savepoints
from kinetica_jl_amd.synth import synthetic_crn

ALT, WINDOW = 5, 1.0
T_SPAN, SAVE = 2e-3, 2e-5


def schedules(K):
    """tools/ensemble_discrete_scaling.py's members: a ramp from 900 K to 1 100 K at the member's own rate, updated every 2e-5 s"""
    out = []
    for m in range(K):
        rate = 1e5 + 4e5 * m / max(K - 1, 1)
        ts = create_savepoints(0.0, 200.0 / rate, 2e-5)
        out.append((ts, np.minimum(900.0 + rate * ts, 1100.0)))
    return out


def ev_timed(fn, reps, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def wall_timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def reps_for(t_one, window):
    return int(min(max(np.ceil(window / max(t_one, 1e-7)), 3), 20000))


def fmt(x):
    x = np.sort(np.asarray(x))
    return f"{np.median(x) * 1e3:9.3f} ms [{x[0] * 1e3:.3f}, {x[-1] * 1e3:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_flux_ab.txt"))
    ap.add_argument("--cases", default="static300,discrete300,static1000")
    ap.add_argument("--K", type=int, default=1024)
    args = ap.parse_args()
    if capi.device_count() == 0:
        raise RuntimeError("ensemble_flux_bench needs a HIP device")
    K = args.K
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    x = torch.rand((4096, 4096), device=dev)          # spin-up: the clocks settle under load
    t0 = time.time()
    while time.time() - t0 < 1.0:
        x = x @ x * 1e-4
        torch.cuda.synchronize()
    del x
    lines = [f"# tools/ensemble_flux_bench.py on {torch.cuda.get_device_name(0)}: K = {K} members, {ALT} alternations, per-call times "
             f"(median [min, max]); windows of ~{WINDOW:.0f} s (1d, 2), ~{WINDOW / 4:.2f} s (1), one pass (3); MB = algorithmic bytes"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    p = capi.KinParams(tspan0=0.0, tspan1=T_SPAN, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1,
                       ban_negatives=0, solve_chunkstep=1e-3, maxiters=100000, save_interval=SAVE, dtmin=0.0)
    shapes = {"static300": (300, "static"), "discrete300": (300, "discrete_members"), "static1000": (1000, "static")}
    for name in args.cases.split(","):
        N, kind = shapes[name]
        R = 5 * N
        net, Ea, A = synthetic_crn(N, R)
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        U0 = np.zeros((K, N)); U0[:, 0] = 1.0
        t_solve = time.perf_counter()
        if kind == "static":
            Tm = np.linspace(900.0, 1100.0, K)
            t, u, ns, rcs, _ = h.solve_ensemble(p, U0, T=Tm)
            src = S.ensemble_flux_sources("static", t, ns, T=Tm)
        else:
            stops = schedules(K)
            t, u, ns, rcs, _ = h.solve_ensemble_discrete(p, U0, stops)
            src = S.ensemble_flux_sources("discrete_members", t, ns, stops=stops)
        t_solve = time.perf_counter() - t_solve
        rows = len(t)
        B = K * rows
        w, Trows = src["w"], src["T_rows"]
        keys_per_member = np.mean([1 + np.count_nonzero(np.diff(Trows[m, :ns[m]])) for m in range(K) if ns[m] > 0])
        d_u = torch.tensor(u.reshape(B, N), dtype=torch.float64, device=dev)
        d_T = torch.tensor(Trows.reshape(B), dtype=torch.float64, device=dev)
        d_w = torch.tensor(w.reshape(B), dtype=torch.float64, device=dev)
        d_ns = torch.tensor(ns, dtype=torch.int64, device=dev)
        d_fs = torch.empty((K, R), dtype=torch.float64, device=dev)
        d_f1 = torch.empty((R,), dtype=torch.float64, device=dev)
        pin = torch.empty((B, N), dtype=torch.float64).pin_memory()
        torch.cuda.synchronize()
        s = st.cuda_stream
        v1 = lambda: h.ensemble_flux(w=w, T_rows=Trows)
        v1d = lambda: h.flux_segmented_dev(K, rows, d_u.data_ptr(), d_fs.data_ptr(), d_seg_n=d_ns.data_ptr(), d_T=d_T.data_ptr(),
                                          d_w=d_w.data_ptr(), stream=s)
        v2 = lambda: h.flux_batched_dev(B, d_u.data_ptr(), d_T=d_T.data_ptr(), d_w=d_w.data_ptr(), d_flux=d_f1.data_ptr(), stream=s)

        def v3():
            pin.copy_(d_u, non_blocking=True)               # the download of out_u (a pinned target: the copy at its best)
            torch.cuda.synchronize()
            um = pin.numpy().reshape(K, rows, N)
            return np.stack([h.flux_batched(um[m, :ns[m]], T=Trows[m, :ns[m]], w=w[m, :ns[m]]) for m in range(K)])

        # the same numbers from every form (1 and 1d bit for bit; 3 a different summation order: the flux bound, twice)
        f1 = v1(); v1d(); torch.cuda.synchronize()
        f3 = v3()
        same_bits = bool(np.array_equal(f1, d_fs.cpu().numpy()))
        rel3 = float(np.max(np.abs(f1 - f3) / (np.abs(f3) + 1e-300)))
        v2(); torch.cuda.synchronize()
        relsum = float(np.max(np.abs(f1.sum(axis=0) - d_f1.cpu().numpy()) / (np.abs(d_f1.cpu().numpy()) + 1e-300)))
        n1 = reps_for(wall_timed(v1, 3), WINDOW / 4)
        n1d = reps_for(ev_timed(v1d, 3, st), WINDOW)
        n2 = reps_for(ev_timed(v2, 3, st), WINDOW)
        t1, t1d, t2, t3 = [], [], [], []
        for _ in range(ALT):
            t1.append(wall_timed(v1, n1))
            t1d.append(ev_timed(v1d, n1d, st))
            t2.append(ev_timed(v2, n2, st))
            t3.append(wall_timed(v3, 1))
        states = int(ns.sum())
        mb_seg = (states * (8 * N + 16) + K * 24 * R + 8 * K) / 1e6
        mb_host = mb_seg + (16 * B + 8 * K) / 1e6 + 8 * K * R / 1e6         # + keys and weights up, flux[K][R] down (PCIe)
        mb_bat = (B * (8 * N + 16) + 24 * R) / 1e6
        mb_today = (8 * B * N + states * (8 * N + 16) + K * 8 * R) / 1e6 + mb_seg      # out_u down, members up again, K results down, K passes
        emit(f"{name:12s} N={N} R={R} K={K} rows={rows} states={states} kind={kind} keys/member={keys_per_member:.1f} "
             f"(solve {t_solve:.2f} s, {int((rcs == 0).sum())} ok)")
        emit(f"  1  ensemble_flux  {fmt(t1)}  x{n1:<6d} {mb_host:9.1f} MB")
        emit(f"  1d segmented_dev  {fmt(t1d)}  x{n1d:<6d} {mb_seg:9.1f} MB")
        emit(f"  2  batched_dev    {fmt(t2)}  x{n2:<6d} {mb_bat:9.1f} MB")
        emit(f"  3  today          {fmt(t3)}  x1      {mb_today:9.1f} MB")
        emit(f"  1d / 2 = {np.median(t1d) / np.median(t2):.3f}   spread of 2: {(max(t2) - min(t2)) / np.median(t2) * 100:.1f} %, of 1d: "
             f"{(max(t1d) - min(t1d)) / np.median(t1d) * 100:.1f} %   3 / 1 = {np.median(t3) / np.median(t1):.1f}")
        emit(f"  checks: 1 == 1d bit for bit: {same_bits}; max rel |1 - 3|: {rel3:.2e}; max rel |sum_m 1 - 2|: {relsum:.2e}")
        h.close()
        del d_u, d_T, d_w, d_fs, pin, u
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
