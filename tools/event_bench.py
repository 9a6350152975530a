"""Event times of stored trajectories next to the one-read maximum pass, alternated in one process (DESIGN 3.1l quotes the
result). Each ensemble case solves K members with a 101-row save grid, then times on the stored ensemble
  max      kin_ensemble_max: the parent's one-read pass over the same states, the yardstick (host entry: one [K][N] down);
  abs      kin_ensemble_events, absolute level from the beginning, t_cross alone: one read (host entry: one [K][N] down, as max);
  of_peak  kin_ensemble_events, level 0.5 x the peak, falling from the peak, t_cross alone: the second walk (host entry);
  abs_all  the first with u_peak, t_peak and t_cross wanted: the same launch, three [K][N] down;
  abs_dev / of_peak_dev   the same two launches alone, kin_events_segmented_dev over a copy of the states (device events);
  numpy    what a caller did before: download out_u, then the same answer in vectorised NumPy (host clock; the download is
           timed as a device-to-host copy into a pinned array of out_u's size).
The single-trajectory case does the same with kin_solution_max / kin_solution_events over the stored states of one kin_solve
(10 000 species, 2 801 saved rows). Host entries are timed by the host clock around calls that end in a stream synchronisation,
over enough repetitions to fill a quarter of a second; device entries by device events over about half a second; ALT
alternations; medians and [min, max] of the per-call times. MB = the states' bytes (one read).
Usage: python tools/event_bench.py [--out profiles/event_times_ab.txt] [--cases ens300,ens1000,single10k] [--K 1024]"""
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

ALT, WINDOW = 5, 0.5


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


def numpy_events(u, t, level, kind, direction, start):
    """The definitions of include/kinetica_hip.h in vectorised NumPy for full segments u[S][L][N], shared t[L]."""
    S, L, N = u.shape
    jp = np.argmax(u, axis=1)                                   # the first row that holds the maximum
    peak = np.take_along_axis(u, jp[:, None, :], axis=1)[:, 0]
    l = np.broadcast_to(level, (S, N)) * (peak if kind == "of_peak" else 1.0)
    met = (u >= l[:, None, :]) if direction == "rise" else (u <= l[:, None, :])
    j0 = jp if start == "peak" else np.zeros_like(jp)
    met &= np.arange(L)[None, :, None] >= j0[:, None, :]
    jc = np.argmax(met, axis=1)
    some = np.take_along_axis(met, jc[:, None, :], axis=1)[:, 0]
    ja = np.maximum(jc - 1, 0)
    a = np.take_along_axis(u, ja[:, None, :], axis=1)[:, 0]
    b = np.take_along_axis(u, jc[:, None, :], axis=1)[:, 0]
    with np.errstate(all="ignore"):
        chord = t[ja] + ((l - a) / (b - a)) * (t[jc] - t[ja])
    return dict(u_peak=peak, t_peak=t[jp], t_cross=np.where(some, np.where(jc == j0, t[j0], chord), np.nan))


def same(a, b):
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_times_ab.txt"))
    ap.add_argument("--cases", default="ens300,ens1000,single10k")
    ap.add_argument("--K", type=int, default=1024)
    args = ap.parse_args()
    if capi.device_count() == 0:
        raise RuntimeError("event_bench needs a HIP device")
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
    lines = [f"# tools/event_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations, per-call times (median [min, max]); host "
             f"entries over ~{WINDOW / 2:.2f} s, device entries over ~{WINDOW:.1f} s, numpy once; MB = bytes of the states (one read)"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    REQ = dict(abs=dict(kind="abs", direction="rise", start="begin"), of_peak=dict(kind="of_peak", direction="fall", start="peak"))
    shapes = {"ens300": (300, K, 2e-3, 1e-3, 2e-5), "ens1000": (1000, K, 2e-3, 1e-3, 2e-5), "single10k": (10000, 1, 2.8e-3, 4e-4, 1e-6)}
    for name in args.cases.split(","):
        N, S, t_end, chunk, save = shapes[name]
        net, Ea, A = synthetic_crn(N, 5 * N)
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        p = capi.KinParams(tspan0=0.0, tspan1=t_end, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1,
                           ban_negatives=0, solve_chunkstep=chunk, maxiters=100000, save_interval=save, dtmin=0.0)
        t_solve = time.perf_counter()
        if S > 1:
            U0 = np.zeros((S, N)); U0[:, 0] = 1.0
            t, u, ns, rcs, _ = h.solve_ensemble(p, U0, T=np.linspace(900.0, 1100.0, S))
            ok = int((rcs == 0).sum())
            run_max = h.ensemble_max
            run_ev = lambda level, **kw: h.ensemble_events(t, level=level, **kw)
        else:
            h.rates_at(1000.0)
            u0 = np.zeros(N); u0[0] = 1.0
            t, u, rc, _, _ = h.solve(p, u0)
            u, ns, ok = u[None], np.array([len(t)]), int(rc == 0)
            run_max = h.solution_max
            run_ev = lambda level, **kw: h.solution_events(level=level, **kw)
        t_solve = time.perf_counter() - t_solve
        rows = len(t)
        assert np.all(ns == rows), "the vectorised NumPy form takes full segments"
        # levels: the absolute one a tenth of every species' largest value anywhere, the relative one half of the peak
        levels = dict(abs=0.1 * u.max(axis=(0, 1)), of_peak=np.full(N, 0.5))
        d_u = torch.tensor(u.reshape(S * rows, N), dtype=torch.float64, device=dev)
        d_t = torch.tensor(t, dtype=torch.float64, device=dev)
        d_l = {q: torch.tensor(v, dtype=torch.float64, device=dev) for q, v in levels.items()}
        d_o = [torch.empty((S, N), dtype=torch.float64, device=dev) for _ in range(3)]
        pin = torch.empty((S * rows, N), dtype=torch.float64).pin_memory()
        torch.cuda.synchronize()
        s = st.cuda_stream
        host = {q: (lambda q=q: run_ev(levels[q], want=("t_cross",), **REQ[q])) for q in REQ}
        host["abs_all"] = lambda: run_ev(levels["abs"], **REQ["abs"])
        devf = {q: (lambda q=q: h.events_segmented_dev(S, rows, d_u.data_ptr(), d_t.data_ptr(), d_level=d_l[q].data_ptr(), d_u_peak=d_o[0].data_ptr(),
                                                       d_t_peak=d_o[1].data_ptr(), d_t_cross=d_o[2].data_ptr(), stream=s, **REQ[q])) for q in REQ}

        def numpy_way(q):
            pin.copy_(d_u, non_blocking=True)               # the download of out_u (a pinned target: the copy at its best)
            torch.cuda.synchronize()
            return numpy_events(pin.numpy().reshape(S, rows, N), t, levels[q], **REQ[q])

        checks = []
        for q in REQ:
            a, b = run_ev(levels[q], **REQ[q]), numpy_way(q)
            devf[q](); torch.cuda.synchronize()
            a = {w: v.reshape(S, N) for w, v in a.items()}
            checks.append(f"{q}: host == numpy {all(same(a[w], b[w]) for w in a)}, host == dev "
                          f"{all(same(a[w], d_o[i].cpu().numpy()) for i, w in enumerate(('u_peak', 't_peak', 't_cross')))}, "
                          f"crossings found {int((~np.isnan(a['t_cross'])).sum())} of {S * N}")
        checks.append(f"u_peak == max {same(np.asarray(run_max()).reshape(S, N), a['u_peak'])}")
        n_max = reps_for(wall_timed(run_max, 3), WINDOW / 2)
        n_host = {q: reps_for(wall_timed(host[q], 3), WINDOW / 2) for q in host}
        n_dev = {q: reps_for(ev_timed(devf[q], 3, st), WINDOW) for q in REQ}
        T = {q: [] for q in ("max", "abs", "of_peak", "abs_all", "abs_dev", "of_peak_dev", "numpy_abs", "numpy_of_peak")}
        for _ in range(ALT):
            T["max"].append(wall_timed(run_max, n_max))
            T["abs_all"].append(wall_timed(host["abs_all"], n_host["abs_all"]))
            for q in REQ:
                T[q].append(wall_timed(host[q], n_host[q]))
                T[q + "_dev"].append(ev_timed(devf[q], n_dev[q], st))
                T["numpy_" + q].append(wall_timed(lambda: numpy_way(q), 1))
        mb = 8.0 * S * rows * N / 1e6
        med = {q: float(np.median(v)) for q, v in T.items()}
        emit(f"{name:10s} N={N} segments={S} rows={rows} (solve {t_solve:.2f} s, {ok} ok)  {mb:.1f} MB")
        for q in T:
            emit(f"  {q:14s} {fmt(T[q])}  {mb / 1e3 / med[q]:8.1f} GB/s")
        emit(f"  abs / max = {med['abs'] / med['max']:.3f}   of_peak / max = {med['of_peak'] / med['max']:.3f}   of_peak_dev / abs_dev = "
             f"{med['of_peak_dev'] / med['abs_dev']:.3f}   numpy_abs / abs = {med['numpy_abs'] / med['abs']:.1f}   numpy_of_peak / of_peak = "
             f"{med['numpy_of_peak'] / med['of_peak']:.1f}")
        emit(f"  spread: max {(max(T['max']) - min(T['max'])) / med['max'] * 100:.1f} %, abs {(max(T['abs']) - min(T['abs'])) / med['abs'] * 100:.1f} %, "
             f"abs_dev {(max(T['abs_dev']) - min(T['abs_dev'])) / med['abs_dev'] * 100:.1f} %")
        emit("  checks: " + "; ".join(checks))
        h.close()
        del d_u, pin, u
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
