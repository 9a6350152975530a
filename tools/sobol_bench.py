"""The Sobol pass on the device against its yardstick and against the moments pass, alternated in one process (DESIGN 3.1k quotes
the result). Each shape holds a Saltelli block u[M (P + 2)][L][N] on the device, as a stored ensemble does. The pass - S1, ST,
mean and variance of all species at every row - is timed through its device entry (kin_members_sobol_dev: the call and the
wait for the stream, so the host's share - participants and weights - counts) against the device-to-host download of the same
states plus the NumPy form of the estimators on the host, and next to kin_members_moments_dev over the same block in the same
alternation. Bytes per second count what each pass actually reads: the moments read the block twice, the Sobol pass A and B
twice per chunk of inputs and every AB_p once - (P + 4 ceil(P / chunk)) / (P + 2) times the block - plus the outputs.
Wall-clock times per call (a call is tens of microseconds: the launch and the wait are part of it, for both passes alike)
after a 1 s spin-up and a warm-up of the shape, ALT alternations of REPS calls; medians and spread.
Usage: python tools/sobol_bench.py [--out profiles/sobol_ab.txt] [--shapes 300-p6,300-p30,1500-p6,1500-p30,300-p20]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from kinetica_jl_amd import capi

ALT, REPS = 5, 200
CHUNK = 8      # member_stats.hpp: SB_CHUNK
HBM_PEAK = 8.0e12


def wall(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def stats(x):
    x = np.sort(np.asarray(x))
    return float(np.median(x)), float(x[0]), float(x[-1])


def chain(N):
    ptr = np.arange(N, dtype=np.int64)
    one = np.ones(N - 1, dtype=np.int64)
    return N, ptr, np.arange(N - 1, dtype=np.int64), one, ptr, np.arange(1, N, dtype=np.int64), one


def numpy_sobol(a, M, P):
    """The estimators of include/kinetica_hip.h in plain NumPy over u[K][L][N]."""
    x = a.reshape(P + 2, M, *a.shape[1:])
    A, B, C = x[0], x[1], x[2:]
    mu = 0.5 * (A.mean(axis=0) + B.mean(axis=0))
    V = 0.5 * (((A - mu) ** 2).mean(axis=0) + ((B - mu) ** 2).mean(axis=0))
    with np.errstate(all="ignore"):
        S1 = np.where(V > 0, ((B - mu) * (C - A)).mean(axis=1) / V, 0.0)
        ST = np.where(V > 0, 0.5 * ((A - C) ** 2).mean(axis=1) / V, 0.0)
    return np.moveaxis(S1, 0, -1), np.moveaxis(ST, 0, -1), mu, V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sobol_ab.txt"))
    ap.add_argument("--shapes", default="300-p6,300-p30,1500-p6,1500-p30,300-p20")
    args = ap.parse_args()
    want = args.shapes.split(",")
    dev = torch.device("cuda")
    x = torch.rand((4096, 4096), device=dev)      # spin-up: the clocks settle under load
    t0 = time.time()
    while time.time() - t0 < 1.0:
        x = x @ x * 1e-4
        torch.cuda.synchronize()
    lines = [f"# tools/sobol_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations (device passes: {REPS} calls each, "
             f"yardstick: 1), wall-clock per call (median [min, max]); states 1 + U(0, 1) of a linear model of the design's inputs, "
             f"every sample takes part, all species; yardstick = download of u + the NumPy estimators on the host; "
             f"TB/s of the bytes each pass reads and writes (HBM peak {HBM_PEAK / 1e12:.0f} TB/s)"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    # (name, species, base samples, inputs, rows): K = 1024-class designs at 300 / 1 500 species, one P above two chunks
    cases = [("300-p6", 300, 128, 6, 21), ("300-p30", 300, 32, 30, 21), ("1500-p6", 1500, 128, 6, 21), ("1500-p30", 1500, 32, 30, 21),
             ("300-p20", 300, 48, 20, 21)]
    for name, N, M, P, L in cases:
        if name not in want:
            continue
        K = M * (P + 2)
        h = capi.HipNetwork(*chain(N))          # (the statistics never look at the reactions)
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        Ab = torch.rand((2, M, P), dtype=torch.float64, device=dev, generator=g)
        Xd = Ab[0].repeat(P + 2, 1, 1)
        Xd[1] = Ab[1]
        for p in range(P):
            Xd[2 + p, :, p] = Ab[1, :, p]
        coef = torch.rand((P, L * N), dtype=torch.float64, device=dev, generator=g)
        u = (1.0 + (Xd.reshape(K, P) @ coef) / P).reshape(K, L, N).contiguous()
        d_o = [torch.empty((L, N, P), dtype=torch.float64, device=dev) for _ in range(2)] + \
              [torch.empty((L, N), dtype=torch.float64, device=dev) for _ in range(2)]
        d_m = [torch.empty((L, N), dtype=torch.float64, device=dev) for _ in range(4)]
        torch.cuda.synchronize()
        host = {}

        def f_sobol():
            h.members_sobol_dev(M, P, L, u.data_ptr(), d_first=d_o[0].data_ptr(), d_total=d_o[1].data_ptr(), d_mean=d_o[2].data_ptr(),
                                d_var=d_o[3].data_ptr())
            torch.cuda.synchronize()

        def f_moments():
            h.members_moments_dev(K, L, u.data_ptr(), d_mean=d_m[0].data_ptr(), d_var=d_m[1].data_ptr(), d_min=d_m[2].data_ptr(),
                                  d_max=d_m[3].data_ptr())
            torch.cuda.synchronize()

        def f_host():
            host["r"] = numpy_sobol(u.cpu().numpy(), M, P)

        block = K * L * N * 8
        emit(f"{name:9s} N={N} M={M} P={P} K={K} rows={L}  states {block / 1e6:.0f} MB, columns {L * N}")
        for f in (f_sobol, f_moments):
            f(); f()
        ts, tm, th = [], [], []
        for _ in range(ALT):
            f_sobol()                               # (the host yardstick leaves the device idle: one untimed call first)
            ts.append(wall(f_sobol, REPS))
            tm.append(wall(f_moments, REPS))
            th.append(wall(f_host))
        for got, ref in zip(d_o, host["r"]):
            assert np.allclose(got.cpu().numpy(), ref, rtol=1e-9, atol=1e-9)
        ms, mm, mh = stats(ts), stats(tm), stats(th)
        chunks = -(-P // CHUNK)
        b_s = (P + 4 * chunks) * M * L * N * 8 + (2 * P + 2) * L * N * 8
        b_m = 2 * block + 4 * L * N * 8
        bw_s, bw_m = b_s / ms[0], b_m / mm[0]
        emit(f"  sobol    device {ms[0] * 1e3:9.3f} ms [{ms[1] * 1e3:.3f}, {ms[2] * 1e3:.3f}]   download + host {mh[0] * 1e3:9.1f} ms "
             f"[{mh[1] * 1e3:.1f}, {mh[2] * 1e3:.1f}]   {mh[0] / ms[0]:.0f} x faster than its yardstick")
        emit(f"  sobol    reads {b_s / block:.3f} x the block: {bw_s / 1e12:.3f} TB/s;   moments {mm[0] * 1e3:9.3f} ms "
             f"[{mm[1] * 1e3:.3f}, {mm[2] * 1e3:.3f}], reads 2 x the block: {bw_m / 1e12:.3f} TB/s;   ratio sobol / moments {bw_s / bw_m:.2f}")
        h.close()
        del u, d_o, d_m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
