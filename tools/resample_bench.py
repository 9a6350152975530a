"""Resampling a stored ensemble onto a common axis next to the one-read maximum pass and to what a caller did before,
alternated in one process (DESIGN 3.1m quotes the result). Each case solves K members with a 101-row save grid and gives every
member an axis of its own, a ramp from 900 K at its own heating rate that holds at 1300 K; the queries are Q = n_rows points per
member spread over the member's own range, so that every query is inside, every member keeps all Q rows and a stored result has
the shape of the record it replaces. Timed on the stored ensemble:
  resample   kin_ensemble_resample(store=1, out=NULL): the axes checked and uploaded, the launch, the record replaced (host entry;
             each call resamples the record the call before left - same shape, same axes, the two handle buffers in turn);
  max        kin_ensemble_max over the same record: the parent's one-read pass over the same states, the yardstick (host entry:
             one [K][N] down);
  resample_dev   the launch alone, kin_resample_segmented_dev over a copy of the solve's states (device events);
  numpy      what the parent commit offers: download out_u (timed as a device-to-host copy into a pinned array of out_u's
             size), then np.interp per member and species (host clock).
Host entries are timed by the host clock around calls that end in a stream synchronisation, over enough repetitions to fill a
quarter of a second; the device entry by device events over about half a second; ALT alternations; medians and [min, max] of
the per-call times. The traffic of the pass is what the algorithm needs: every distinct row that closes or opens a bracket read
once, every query's row written, the axes and queries read - computed here from the brackets (kin_resample_bracket_host).
Usage: python tools/resample_bench.py [--out profiles/resample_ab.txt] [--cases ens300,ens1000]"""
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


def traffic_bytes(jc, w, N, x, xq):
    """The bytes the pass needs: the distinct rows of a member that some bracket reads, once each; every query's row written; the
    axes and the queries."""
    S, Q = jc.shape
    L = x.shape[-1]
    rows = 0
    for s in range(S):
        hit = np.zeros(L + 1, bool)
        inside = jc[s] >= 0
        hit[jc[s][inside]] = True
        hit[jc[s][inside & (w[s] != 0.0)] - 1] = True
        rows += int(hit[:L].sum())
    return 8 * (rows * N + S * Q * N + x.size + xq.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_ab.txt"))
    ap.add_argument("--cases", default="ens300,ens1000")
    args = ap.parse_args()
    if capi.device_count() == 0:
        raise RuntimeError("resample_bench needs a HIP device")
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    z = torch.rand((4096, 4096), device=dev)          # spin-up: the clocks settle under load
    t0 = time.time()
    while time.time() - t0 < 1.0:
        z = z @ z * 1e-4
        torch.cuda.synchronize()
    del z
    lines = [f"# tools/resample_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations, per-call times (median [min, max]); host "
             f"entries over ~{WINDOW / 2:.2f} s, the device entry over ~{WINDOW:.1f} s, numpy once; GB/s = the pass's algorithmic "
             "traffic (resample legs) or the states' bytes (max, numpy) over the time"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    shapes = {"ens300": (300, 1024), "ens1000": (1000, 256)}
    for name in args.cases.split(","):
        N, K = shapes[name]
        net, Ea, A = synthetic_crn(N, 5 * N)
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        p = capi.KinParams(tspan0=0.0, tspan1=2e-3, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1,
                           ban_negatives=0, solve_chunkstep=1e-3, maxiters=100000, save_interval=2e-5, dtmin=0.0)
        t_solve = time.perf_counter()
        U0 = np.zeros((K, N)); U0[:, 0] = 1.0
        t, u, ns, rcs, _ = h.solve_ensemble(p, U0, T=np.linspace(900.0, 1100.0, K))
        t_solve = time.perf_counter() - t_solve
        rows = len(t)
        assert np.all(ns == rows), "the NumPy leg takes full segments"
        Q = rows
        rates = np.linspace(1e5, 4e5, K)
        x = np.minimum(900.0 + rates[:, None] * t[None, :], 1300.0)               # [K][rows]: a ramp that holds
        xq = np.stack([np.linspace(x[m, 0], x[m, -1], Q) for m in range(K)])      # [K][Q]: every query inside
        jc, w = capi.resample_brackets(x, xq)
        assert np.all(jc >= 0)
        traffic = traffic_bytes(jc, w, N, x, xq)
        d_u = torch.tensor(u.reshape(K * rows, N), dtype=torch.float64, device=dev)
        d_x = torch.tensor(x, dtype=torch.float64, device=dev)
        d_q = torch.tensor(xq, dtype=torch.float64, device=dev)
        d_o = torch.empty((K * Q, N), dtype=torch.float64, device=dev)
        pin = torch.empty((K * rows, N), dtype=torch.float64).pin_memory()
        torch.cuda.synchronize()
        s = st.cuda_stream
        run_store = lambda: h.ensemble_resample(x, xq, store=True, download=False)
        run_max = h.ensemble_max
        run_dev = lambda: h.resample_segmented_dev(K, rows, d_u.data_ptr(), d_x.data_ptr(), Q, d_q.data_ptr(), d_o.data_ptr(),
                                                   x_per_segment=True, xq_per_segment=True, stream=s)

        def numpy_way():
            pin.copy_(d_u, non_blocking=True)               # the download of out_u (a pinned target: the copy at its best)
            torch.cuda.synchronize()
            uu = pin.numpy().reshape(K, rows, N)
            out = np.empty((K, Q, N))
            for m in range(K):
                for i in range(N):
                    out[m, :, i] = np.interp(xq[m], x[m], uu[m, :, i])
            return out

        # what the legs compute: the stored entry, the device entry and np.interp on the solve's states
        first = h.ensemble_resample(x, xq)
        run_dev(); torch.cuda.synchronize()
        ref = numpy_way()
        scale = np.abs(u).max()
        # (where the query is the value of a plateau the definition takes the first row that holds it, np.interp the last)
        on_plateau = (w == 0.0) & (np.take_along_axis(x, np.minimum(jc + 1, rows - 1), axis=1) == xq) & (jc + 1 < rows)
        checks = [f"host == dev {first.tobytes() == d_o.cpu().numpy().reshape(K, Q, N).tobytes()}",
                  f"max |host - np.interp| / max |u| = {np.abs(first - ref)[~on_plateau].max() / scale:.2e} over the "
                  f"{int((~on_plateau).sum())} queries off a plateau's value",
                  f"copies {int((w == 0.0).sum())} and chords {int((w != 0.0).sum())} of {K * Q} queries",
                  f"distinct rows read {(traffic // 8 - K * Q * N - x.size - xq.size) // N} of {K * rows}"]
        run_store()
        assert h.ensemble_size()[1] == Q and np.all(h.ensemble_size()[3] == Q)
        n_store = reps_for(wall_timed(run_store, 3), WINDOW / 2)
        n_max = reps_for(wall_timed(run_max, 3), WINDOW / 2)
        n_dev = reps_for(ev_timed(run_dev, 3, st), WINDOW)
        T = {q: [] for q in ("resample", "max", "resample_dev", "numpy")}
        for _ in range(ALT):
            T["resample"].append(wall_timed(run_store, n_store))
            T["max"].append(wall_timed(run_max, n_max))
            T["resample_dev"].append(ev_timed(run_dev, n_dev, st))
            T["numpy"].append(wall_timed(numpy_way, 1))
        mb = 8.0 * K * rows * N / 1e6
        med = {q: float(np.median(v)) for q, v in T.items()}
        emit(f"{name:8s} N={N} R={5 * N} K={K} rows={rows} Q={Q} (solve {t_solve:.2f} s, {int((rcs == 0).sum())} ok)  states {mb:.1f} MB, "
             f"resample traffic {traffic / 1e6:.1f} MB")
        for q in T:
            nbytes = traffic if q.startswith("resample") else 8.0 * K * rows * N
            emit(f"  {q:14s} {fmt(T[q])}  {nbytes / 1e9 / med[q]:8.1f} GB/s")
        emit(f"  resample / max = {med['resample'] / med['max']:.3f}   resample_dev / max = {med['resample_dev'] / med['max']:.3f}   "
             f"numpy / resample = {med['numpy'] / med['resample']:.1f}")
        emit("  spread: " + ", ".join(f"{q} {(max(T[q]) - min(T[q])) / med[q] * 100:.1f} %" for q in T))
        emit("  checks: " + "; ".join(checks))
        h.close()
        del d_u, d_o, pin, u
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
