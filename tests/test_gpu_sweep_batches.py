"""The batch plan of the LDS sweeps (kernels.hip: sweep_reg_kernel, sweep_gen_kernel) at the sizes where it changes path.

Both kernels read their record arrays without bounds tests: the host pads them with all-dummy records (network.cpp) and a
batch of rows that reaches past the last record reads the padding as it stands. sweep_reg_kernel keeps the first TR = 8, 4
or 0 rows of BS records in registers and streams the remaining S rows in batches of 4 and 5 rows (sweep_stream_plan); the
workgroup size BS follows the number of species (256 up to N = 2560, 512 up to 5120, else 1024). Each case below is the
smallest network that takes one of these paths; every state has rate constants of its own, and the batch is large enough
for the state loop of a workgroup to come round again where the issue's B allows it (BS = 512, B = 600: it does not - 3
workgroups fit a CU there, 768 states run in the first trip).

Reference: OracleNetwork.rhs on the first state, the last state (a later trip of the state loop) and one in between;
bound: test_gpu_parity's TOL relative to abs_rhs - FP64 on both sides, only the order of the sums differs."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import synthetic_crn
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-13


def _block_order(net, k):
    """the same reactions presented as (p, P + p): all forward reactions, then their reverses in the same order"""
    order = np.concatenate([np.arange(0, net.n_reactions, 2), np.arange(1, net.n_reactions, 2)])
    return net.subset(order), k[order]


def _thinned(net, k, seed):
    """minus a seeded 30 % of the reactions: pairs lose their partners, the network leaves both regular layouts"""
    keep = np.sort(np.random.default_rng(seed).permutation(net.n_reactions)[: int(0.7 * net.n_reactions)])
    return net.subset(keep), k[keep]


def _check(net, k, B, seed=0):
    h = capi.HipNetwork.from_flat(net)
    try:
        on = orc.OracleNetwork.from_flat(net)
        rng = np.random.default_rng(seed)
        U = 10.0 ** rng.uniform(-12, 0, (B, net.n_species))
        K = k[None, :] * rng.uniform(0.5, 2.0, (B, 1))
        DU = h.rhs_batched(U, K)
        assert DU.shape == U.shape and np.isfinite(DU).all()
        for b in (0, B // 2, B - 1):
            err = np.abs(DU[b] - on.rhs(K[b], U[b])) / (on.abs_rhs(K[b], U[b]) + 1e-300)
            assert err.max() < TOL, f"state {b}: {err.max():.3e}"
    finally:
        h.close()


def _crn(n, r):
    net, Ea, A = synthetic_crn(n, r)
    return net, orc.arrhenius(Ea, A, 1000.0, k_max=1e12)


# P = R / 2 records; rows = ceil(P / BS); the first TR rows are register-resident, S = rows - TR are streamed
BS256 = [
    (2000, "TR0_all_streamed_no_prefetch"),          # P = 1000: no full batch of register rows, 4 streamed rows
    (4098, "one_streamed_record_in_lane_0"),         # P = 8 * 256 + 1
    (6144, "one_full_streamed_batch_no_padding"),    # P = 12 * 256
    (6658, "full_batch_plus_ragged_remainder"),      # P = 13 * 256 + 1: S = 6 = 4 + 2 (+ 2 rows of padding)
    (6500, "one_wide_batch"),                        # P = 3250: S = 5, one batch of 5 rows
    (8392, "batch_of_4_then_batch_of_5"),            # P = 4196: S = 9 = 4 + 5
]


@pytest.mark.parametrize("R", [r for r, _ in BS256], ids=[i for _, i in BS256])
def test_bs256_path(R):
    net, k = _crn(300, R)
    _check(net, k, 2100)      # 8 workgroups on each of 256 CUs = 2048 states per trip


BS1024 = [
    (16386, "one_record_past_the_register_rows"),    # P = 8 * 1024 + 1
    (26626, "ragged_remainder_of_2_rows"),           # P = 13 * 1024 + 1: S = 6
    (25576, "one_wide_batch"),                       # P = 12788: S = 5
]


@pytest.mark.parametrize("R", [r for r, _ in BS1024], ids=[i for _, i in BS1024])
def test_bs1024_path(R):
    net, k = _crn(5200, R)
    _check(net, k, 300)       # one workgroup per CU: 256 states per trip


def test_bs512_path():
    net, k = _crn(3000, 2 * (8 * 512 + 4 * 512 + 513))    # S = 6 rows, the last one a single record
    _check(net, k, 600)


def test_block_layout():
    net, k = _crn(300, 6658)
    _check(*_block_order(net, k), 2100)


@pytest.mark.parametrize("n,R,B", [(300, 6658, 2100), (5200, 26626, 300)], ids=["bs256", "bs1024"])
def test_general_sweep_after_a_cutoff(n, R, B):
    net, k = _crn(n, R)
    _check(*_thinned(net, k, seed=R), B)


def test_doubling_k_doubles_du_exactly():
    """A padding record that reached a real species, or real rate constants that reached a real accumulator through one,
    would add a term that the oracle comparison may miss under its tolerance. The accumulators are LDS atomics, so the order
    of a species' sum changes from launch to launch; the inputs are therefore chosen so that NO sum rounds: u in
    {1/2, 1, 2}, k an integer in 1 .. 8 - every term is a multiple of 1/4 below 2^6, every partial sum far below 2^53 / 4.
    Then du is the same in any order, du(2 K) == 2 du(K) bit for bit, and du equals the oracle's exactly."""
    net, _ = _crn(300, 6658)
    h = capi.HipNetwork.from_flat(net)
    try:
        on = orc.OracleNetwork.from_flat(net)
        rng = np.random.default_rng(7)
        B = 2100
        U = 2.0 ** rng.integers(-1, 2, (B, net.n_species)).astype(np.float64)
        K = rng.integers(1, 9, (B, net.n_reactions)).astype(np.float64)
        DU = h.rhs_batched(U, K)
        DU2 = h.rhs_batched(U, 2.0 * K)
        assert np.array_equal(DU2, 2.0 * DU)
        assert np.abs(DU).max() > 0
        for b in (0, B // 2, B - 1):
            assert np.array_equal(DU[b], on.rhs(K[b], U[b]))
    finally:
        h.close()
