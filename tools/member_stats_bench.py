"""Cross-member statistics on the device against their yardstick, alternated in one process (DESIGN 3.1j quotes the result).
Each shape holds a block of states u[K][L][N] on the device, as a stored ensemble does. Each pass - moments, quantiles
(5 / 50 / 95 %), Spearman and Pearson correlation with P = 8 inputs, all species - is timed through its device entry
(kin_members_*_dev: the call and the wait for the stream, so the host's share - participants, the normalised inputs - counts)
against the device-to-host download of the same states plus NumPy / SciPy doing the same job on the host. Wall-clock times
after a 1 s spin-up and a warm-up of the shape, ALT alternations; medians and spread. The moments' fraction of the HBM peak
(8 TB/s) is from their algorithmic bytes: one read of the states and the four outputs (the kernel reads the states twice; the
second read is served by the caches where they hold it).
Usage: python tools/member_stats_bench.py [--out profiles/member_stats_ab.txt] [--shapes 300,1k]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.stats
import torch
from kinetica_jl_amd import capi

ALT, REPS = 5, 3
QS = np.array([0.05, 0.5, 0.95])
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


def normalise(a):
    d = a - a.mean(axis=0)
    s = np.sqrt((d * d).sum(axis=0))
    return np.divide(d, s, out=np.zeros_like(d), where=s > 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "member_stats_ab.txt"))
    ap.add_argument("--shapes", default="300,1k")
    args = ap.parse_args()
    want = args.shapes.split(",")
    dev = torch.device("cuda")
    x = torch.rand((4096, 4096), device=dev)      # spin-up: the clocks settle under load
    t0 = time.time()
    while time.time() - t0 < 1.0:
        x = x @ x * 1e-4
        torch.cuda.synchronize()
    lines = [f"# tools/member_stats_bench.py on {torch.cuda.get_device_name(0)}: {ALT} alternations (device pass: {REPS} calls each, "
             f"yardstick: 1), wall-clock per call (median [min, max]); states 10^U(-12, 0) with 30 % zeros, every member takes part, "
             f"all species; yardstick = download of u + NumPy / SciPy on the host"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    cases = [("300", 300, 1024, 101), ("1k", 1000, 1024, 21)]
    for name, N, K, L in cases:
        if name not in want:
            continue
        h = capi.HipNetwork(*chain(N))          # (the statistics never look at the reactions)
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        u = torch.pow(10.0, torch.rand((K, L, N), dtype=torch.float64, device=dev, generator=g) * 12 - 12)
        u *= (torch.rand((K, L, N), device=dev, generator=g) >= 0.3)
        X = np.random.default_rng(2).standard_normal((K, 8))
        P = X.shape[1]
        d_m = [torch.empty((L, N), dtype=torch.float64, device=dev) for _ in range(4)]
        d_q = torch.empty((3, L, N), dtype=torch.float64, device=dev)
        d_r = torch.empty((L, N, P), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        host = {}

        def np_moments():
            a = u.cpu().numpy()
            host["mean"], host["var"], host["min"], host["max"] = a.mean(axis=0), a.var(axis=0, ddof=1), a.min(axis=0), a.max(axis=0)

        def np_quantiles():
            host["q"] = np.quantile(u.cpu().numpy(), QS, axis=0, method="linear")

        def np_spearman():
            a = u.cpu().numpy().reshape(K, L * N)
            host["rs"] = (normalise(scipy.stats.rankdata(a, axis=0)).T @ normalise(scipy.stats.rankdata(X, axis=0))).reshape(L, N, P)

        def np_pearson():
            a = u.cpu().numpy().reshape(K, L * N)
            host["rp"] = (normalise(a).T @ normalise(X)).reshape(L, N, P)

        passes = {
            "moments": (lambda: h.members_moments_dev(K, L, u.data_ptr(), d_mean=d_m[0].data_ptr(), d_var=d_m[1].data_ptr(),
                                                      d_min=d_m[2].data_ptr(), d_max=d_m[3].data_ptr()), np_moments),
            "quantiles": (lambda: h.members_quantiles_dev(K, L, u.data_ptr(), QS, d_q.data_ptr()), np_quantiles),
            "spearman": (lambda: h.members_correlate_dev(K, L, u.data_ptr(), X, d_r.data_ptr(), rank=True), np_spearman),
            "pearson": (lambda: h.members_correlate_dev(K, L, u.data_ptr(), X, d_r.data_ptr(), rank=False), np_pearson),
        }
        download = lambda: u.cpu()
        emit(f"{name:4s} N={N} K={K} rows={L}  states {u.numel() * 8 / 1e6:.0f} MB, columns {L * N}, inputs {P}")
        wall(download)
        dl = stats([wall(download) for _ in range(ALT)])
        emit(f"  download alone      {dl[0] * 1e3:9.2f} ms [{dl[1] * 1e3:.2f}, {dl[2] * 1e3:.2f}]")
        for pname, (fdev, fhost) in passes.items():
            fdev(); fdev()
            torch.cuda.synchronize()
            td, th = [], []
            for _ in range(ALT):
                td.append(wall(fdev, REPS))
                th.append(wall(fhost))
            md, mh = stats(td), stats(th)
            note = ""
            if pname == "moments":
                byts = (K + 4) * L * N * 8
                note = f"  {byts / md[0] / 1e12:.2f} TB/s of algorithmic bytes = {100 * byts / md[0] / HBM_PEAK:.0f} % of the HBM peak"
                assert np.allclose(d_m[0].cpu().numpy(), host["mean"], rtol=1e-12, atol=0) and np.array_equal(d_m[3].cpu().numpy(), host["max"])
            elif pname == "quantiles":
                assert np.allclose(d_q.cpu().numpy(), host["q"], rtol=1e-12, atol=0)
            else:
                assert np.allclose(d_r.cpu().numpy(), host["rs" if pname == "spearman" else "rp"], rtol=0, atol=1e-9)
            verdict = "slower than" if md[0] > mh[0] else f"{mh[0] / md[0]:.0f} x faster than"
            emit(f"  {pname:10s} device {md[0] * 1e3:9.3f} ms [{md[1] * 1e3:.3f}, {md[2] * 1e3:.3f}]   download + host "
                 f"{mh[0] * 1e3:9.1f} ms [{mh[1] * 1e3:.1f}, {mh[2] * 1e3:.1f}]   {verdict} its yardstick{note}")
        h.close()
        del u, d_m, d_q, d_r
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
