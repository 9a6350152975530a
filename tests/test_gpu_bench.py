"""bench.py's plain run (the headline sweep only) and its --dump-outputs files, at a small size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
N, R, B = 1000, 5000, 8192          # du = 65.5 MB: more than the dump keeps whole, so the seeded sample of states is written


def _bench(*extra):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--species", str(N), "--reactions", str(R), "--batch", str(B),
                        "--spinup-seconds", "0", *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_bench_options_full_and_dump_outputs_exist():
    p = subprocess.run([sys.executable, BENCH, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_timed_sweep(tmp_path):
    """A plain run times exactly --steps sweeps, carries no leg of --full, and writes a seeded sample of the last sweep's du
    (float64, at most 64 MB); a second run with the same arguments sweeps the same inputs and returns the same du, and the
    sampled rows are the RHS of the bench's own states and rate constants (rebuilt here from the same seeds) per the oracle."""
    import torch
    from kinetica_jl_amd.synth import synthetic_crn
    from oracle import oracle as orc

    rec = _bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / "a"))
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["n_gpus"] == 1
    assert rec["unit"] == "RHS evals/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(B * 1e3 / rec["ms_per_step"], rel=1e-9)
    for leg in ("solve_network", "solve_network_summary", "tiled_sweep", "post_cutoff_sweep", "cpu_baseline",
                "single_state_rhs_us_host_roundtrip"):
        assert leg not in rec, leg
    assert rec["roofline"]["traffic"] is None and rec["roofline"]["sustained_launch_ms"] is None
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20

    du = np.load(tmp_path / "a" / "rhs_du.npy")
    rows = np.load(tmp_path / "a" / "rhs_du_rows.npy")
    assert du.dtype == np.float64 and rows.dtype == np.float64 and np.isfinite(du).all()
    assert du.shape == (len(rows), N) and 0 < len(rows) < B
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < B and np.array_equal(rows, np.round(rows))

    _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "b" / "rhs_du_rows.npy"), rows)
    du2 = np.load(tmp_path / "b" / "rhs_du.npy")
    assert np.all(np.abs(du2 - du) <= 1e-12 * np.abs(du).max(axis=1, keepdims=True))

    # the bench's inputs, drawn the way bench.py draws them (rank 0)
    net, Ea, A = synthetic_crn(N, R)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(12345)
    d_u = torch.pow(10.0, torch.rand((B, N), dtype=torch.float64, device=dev, generator=g) * 12.0 - 12.0)
    T = torch.linspace(500.0, 1200.0, B, dtype=torch.float64, device=dev)
    kr = torch.tensor(A, dtype=torch.float64, device=dev)[None, :] * \
        torch.exp(-torch.tensor(Ea, dtype=torch.float64, device=dev)[None, :] / (8.314462618 * T[:, None])) * 6.02214076e23
    d_k = 1.0 / ((1.0 / 1e12) + (1.0 / kr))
    on = orc.OracleNetwork.from_flat(net)
    for i in (0, len(rows) // 2, len(rows) - 1):
        b = int(rows[i])
        u, k = d_u[b].cpu().numpy(), d_k[b].cpu().numpy()
        err = np.abs(du[i] - on.rhs(k, u)) / (on.abs_rhs(k, u) + 1e-300)
        assert err.max() < 1e-13, f"state {b}: du deviates from the oracle by {err.max():.3g}"
