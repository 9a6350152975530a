"""The observables pass next to the one-read maximum pass, to the eight kin_ensemble_dot calls it replaces and to download plus
NumPy, alternated in one process (DESIGN 3.1n quotes the result). Each case solves an ensemble and times, on the stored record,
two specs: `forms8`, eight forms over all N species (G = 8), and `molefrac`, the mole fractions of all species (H = N + 1, G = N).
  compact    kin_ensemble_observables(store=0) at pitch G with the result downloaded: what replaces the dot calls (forms8 only:
             the mole fractions' compact block is as large as the states, its download is the numpy leg's);
  store      kin_ensemble_observables(store=1, out=NULL) at pitch N: the launch, the record replaced, nothing downloaded (each call
             takes the record the call before left - same shape, the two handle buffers in turn);
  dev        the launch alone, kin_observables_segmented_dev over a copy of the solve's states at pitch G (device events);
  max        kin_ensemble_max over the same record: the one-read pass over the same states, the yardstick (one [K][N] down);
  dot8       eight kin_ensemble_dot calls, one per form, each with its [K][n_rows] downloaded (forms8 only);
  numpy      the download of the states (a device-to-host copy into a pinned array), then u @ W.T or u / u.sum (host clock).
Host entries are timed by the host clock around calls that end in a stream synchronisation, over enough repetitions to fill a
quarter of a second; the device entry by device events over about half a second; ALT alternations; medians and [min, max] of the
per-call times. The checks run on the solve's own record; in the timed loop the store leg leaves a record of observables, which
the stored legs after it read - the same shape and bytes, no longer the solve's values (the times do not depend on them); the
solve is repeated after each spec. GB/s: the states' bytes read once plus the output's bytes written, over the time (max, dot8: the states' bytes).
Usage: python tools/observables_bench.py [--out profiles/observables_ab.txt] [--cases ens300,big10k]"""
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


def forms8(N):
    """Eight forms over all N species, weights of both signs, each species order its own rotation."""
    rng = np.random.default_rng(8)
    idx = np.concatenate([np.roll(np.arange(N), 37 * f) for f in range(8)])
    return S.ObservableSpec(tuple(f"class{f}" for f in range(8)), N, np.arange(9, dtype=np.int64) * N, idx.astype(np.int64),
                            rng.uniform(-1.0, 2.0, 8 * N), np.arange(8, dtype=np.int64), np.full(8, -1, np.int64))


# name -> (species, members, save interval over a span of 2e-3 s, member temperatures)
SHAPES = {"ens300": (300, 1024, 2e-5, (900.0, 1100.0)), "big10k": (10000, 64, 2e-3 / 63, (900.0, 1000.0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "observables_ab.txt"))
    ap.add_argument("--cases", default="ens300,big10k")
    args = ap.parse_args()
    if capi.device_count() == 0:
        raise RuntimeError("observables_bench needs a HIP device")
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    z = torch.rand((4096, 4096), device=dev)          # spin-up: the clocks settle under load
    t0 = time.time()
    while time.time() - t0 < 1.0:
        z = z @ z * 1e-4
        torch.cuda.synchronize()
    del z
    lines = [f"# tools/observables_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations, per-call times (median [min, max]); "
             f"host entries over ~{WINDOW / 2:.2f} s, the device entry over ~{WINDOW:.1f} s, numpy once; GB/s = the states read once plus "
             "the output written (observables legs, numpy) or the states' bytes (max, dot8) over the time"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for name in args.cases.split(","):
        N, K, save, (Ta, Tb) = SHAPES[name]
        net, Ea, A = synthetic_crn(N, 5 * N)
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        p = capi.KinParams(tspan0=0.0, tspan1=2e-3, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1,
                           ban_negatives=0, solve_chunkstep=1e-3, maxiters=100000, save_interval=save, dtmin=0.0)
        U0 = np.zeros((K, N)); U0[:, 0] = 1.0

        def solve():
            return h.solve_ensemble(p, U0, T=np.linspace(Ta, Tb, K))

        t_solve = time.perf_counter()
        t, u, ns, rcs, _ = solve()
        t_solve = time.perf_counter() - t_solve
        rows = len(t)
        assert np.all(ns == rows), "the NumPy leg takes full segments"
        B = K * rows
        states = 8.0 * B * N
        d_u = torch.tensor(u.reshape(B, N), dtype=torch.float64, device=dev)
        pin = torch.empty((B, N), dtype=torch.float64).pin_memory()
        torch.cuda.synchronize()
        s = st.cuda_stream
        emit(f"{name:8s} N={N} R={5 * N} K={K} rows={rows} states={B} (solve {t_solve:.2f} s, {int((rcs == 0).sum())} ok)  states {states / 1e6:.1f} MB")
        for label, spec in (("forms8", forms8(N)), ("molefrac", S.mole_fractions(N))):
            G, arrays = spec.G, spec.arrays()
            d_o = torch.empty((B, G), dtype=torch.float64, device=dev)
            W = None
            if label == "forms8":
                W = np.zeros((G, N))
                for f in range(8):
                    np.add.at(W[f], spec.form_idx[f * N:(f + 1) * N], spec.form_w[f * N:(f + 1) * N])
            run_compact = lambda: h.ensemble_observables(*arrays)
            run_store = lambda: h.ensemble_observables(*arrays, store=True, download=False)
            run_dev = lambda: h.observables_segmented_dev(K, rows, d_u.data_ptr(), *arrays, G, d_o.data_ptr(), stream=s)
            run_max = h.ensemble_max
            run_dot8 = lambda: [h.ensemble_dot(W[f]) for f in range(8)]

            def numpy_way():
                pin.copy_(d_u, non_blocking=True)               # the download of out_u (a pinned target: the copy at its best)
                torch.cuda.synchronize()
                uu = pin.numpy()
                return uu @ W.T if label == "forms8" else uu / uu.sum(axis=1, keepdims=True)

            # what the legs compute, on the solve's own record: the stored entry, the device entry, NumPy and the dot calls
            first = h.ensemble_observables(*arrays).reshape(B, G)
            run_dev(); torch.cuda.synchronize()
            ref = numpy_way()
            with np.errstate(all="ignore"):
                checks = [f"host == dev {first.tobytes() == d_o.cpu().numpy().tobytes()}",
                          f"max |host - numpy| / max |numpy| = {np.nanmax(np.abs(first - ref)) / np.nanmax(np.abs(ref)):.2e}"]
            if label == "forms8":
                dots = np.stack([d.ravel() for d in run_dot8()], axis=1)
                checks.append(f"max |host - dot| / max |dot| = {np.abs(first - dots).max() / np.abs(dots).max():.2e}")
            legs = dict(store=(run_store, "wall"), dev=(run_dev, "ev"), max=(run_max, "wall"), numpy=(numpy_way, "once"))
            if label == "forms8":
                legs = dict(compact=(run_compact, "wall"), **legs, dot8=(run_dot8, "wall"))
            reps = {}
            for q, (fn, how) in legs.items():
                reps[q] = 1 if how == "once" else reps_for(wall_timed(fn, 3), WINDOW / 2) if how == "wall" else reps_for(ev_timed(fn, 3, st), WINDOW)
            T = {q: [] for q in legs}
            for _ in range(ALT):
                for q, (fn, how) in legs.items():
                    T[q].append(ev_timed(fn, reps[q], st) if how == "ev" else wall_timed(fn, reps[q]))
            med = {q: float(np.median(v)) for q, v in T.items()}
            traffic = dict(compact=states + 8.0 * B * G, dev=states + 8.0 * B * G, store=2 * states, numpy=states + 8.0 * B * G, max=states,
                           dot8=8 * states)
            emit(f" {label}: H={spec.H} G={G} entries={len(spec.form_idx)}")
            for q in T:
                emit(f"  {q:8s} {fmt(T[q])}  {traffic[q] / 1e9 / med[q]:8.1f} GB/s")
            ratios = [f"dev / max = {med['dev'] / med['max']:.3f}", f"store / max = {med['store'] / med['max']:.3f}",
                      f"numpy / store = {med['numpy'] / med['store']:.1f}"]
            if label == "forms8":
                ratios += [f"compact / dot8 = {med['compact'] / med['dot8']:.3f}", f"dev / dot8 = {med['dev'] / med['dot8']:.3f}"]
            emit("  " + "   ".join(ratios))
            emit("  spread: " + ", ".join(f"{q} {(max(T[q]) - min(T[q])) / med[q] * 100:.1f} %" for q in T))
            emit("  checks: " + "; ".join(checks))
            solve()                                             # the stored legs left a record of observables: the states again
            del d_o
        h.close()
        del d_u, pin, u
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
