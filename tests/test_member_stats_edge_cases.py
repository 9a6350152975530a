"""The edge cases of member_stats_edge_cases.py and the order replays of member_stats_order.py, proved on the CPU (no device):
the replays agree with the exact-sum references within the gates the GPU tests already use - and differ from them in the last
bit often enough to be the sharper statement -, the exact columns give their integer expectation, and every case reaches the
kernel path it was made for. The kernels' loop bounds and tile rule are restated here in comments and small functions."""
import numpy as np
import pytest

import member_stats_cases as mc
import member_stats_edge_cases as ec
import member_stats_order as mo
from kinetica_jl_amd import capi

EPS = mc.EPS


def moments_place(n, q):
    """(wave, in the unrolled loop?) of participant q in ms_moments_kernel: wave w = q mod 8 starts at q0 = w and takes
    q0, q0 + 8, q0 + 16, q0 + 24 per trip of the unrolled loop while q0 + 24 < n, q0 += 32; the tail loop takes the rest."""
    w = q % mo.MOM_WAVES
    q0 = w
    while q0 + 3 * mo.MOM_WAVES < n:
        q0 += 4 * mo.MOM_WAVES
    return w, q < q0


def test_fma_rounds_once():
    assert mo.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60      # (the product alone would lose 2^-60)
    assert (1.0 + 2.0 ** -30) * (1.0 + 2.0 ** -30) - 1.0 == 2.0 ** -29
    assert mo.fma(3.0, 5e-324, 0.0) == 1.5e-323 and mo.fma(0.5, 5e-324, 0.0) == 0.0          # subnormal results, ties to even
    assert mo.fma(0.1, 10.0, -1.0) == 2.0 ** -54


def test_masks():
    for n in ec.SMALL_NS + ec.SORTED_NS:
        use = ec.mask(n)
        idx = mc.participants(n + 5, use)
        assert len(use) == n + 5 and len(idx) == n and np.all(np.diff(idx) > 0)
        if n % 2:
            assert use[0] == 0 and use[-1] == 0
        elif n >= 2:
            assert use[0] != 0 and use[-1] != 0
    assert any(np.any(np.diff(mc.participants(n + 5, ec.mask(n))) > 1) for n in ec.SMALL_NS)      # irregular lists


@pytest.mark.parametrize("n", ec.SMALL_NS)
def test_replayed_moments_against_the_exact_sums(n):
    u, use = ec.mixed_block(n), ec.mask(n)
    assert np.all(np.isfinite(u))
    mean, var = ec.expected_moments(n)
    ref = mc.ref_moments(u, use)
    delta = (n + 8) * EPS * ref["abs_mean"]
    assert np.all(np.abs(mean - ref["mean"]) <= delta)
    if n == 1:
        assert np.all(var == 0.0)
    else:
        assert np.all(np.abs(var - ref["var"]) <= (2 * n + 16) * EPS * ref["S"] / (n - 1) + n * delta ** 2 / (n - 1))
    # the exact column: the replay is the integer expectation
    em, ev = ec.exact_moments(n)
    assert np.array_equal(mean[:, ec.SP_EXACT], em) and np.array_equal(var[:, ec.SP_EXACT], ev)


def test_the_order_is_a_sharper_statement_than_the_gate():
    """Over the random columns of the cases with n >= 24 the mean in the documented order differs from the mean of the exact
    sum in at least a fifth of the columns (it does in 374 of 816; always within the gate, as the test above shows): a kernel
    that summed in another order would pass the gate and fail the replay."""
    differ = total = 0
    for n in (24, 25, 32, 33, 40, 65, 257):
        mean, _ = ec.expected_moments(n)
        ref = mc.ref_moments(ec.mixed_block(n), ec.mask(n))
        differ += int((mean[:, ec.SP_FIRST_RANDOM:] != ref["mean"][:, ec.SP_FIRST_RANDOM:]).sum())
        total += mean[:, ec.SP_FIRST_RANDOM:].size
    assert differ * 5 >= total, (differ, total)


@pytest.mark.parametrize("rank", [True, False])
@pytest.mark.parametrize("n", ec.SMALL_NS)
def test_replayed_correlations_against_the_exact_sums(n, rank):
    r, ok, ref, gate = ec.expected_correlation(n, rank)
    assert np.all(ok)
    ruled = np.isinf(gate)
    assert mc.same_bits_or_zero(r[ruled], ref[ruled]), mc.mismatches(r[ruled], ref[ruled])
    assert np.all(np.abs(r[~ruled] - ref[~ruled]) <= gate[~ruled])
    if not rank and n >= 2:
        # the offset columns: every gate stays below 1e-9, up to where its derivation holds, and the column of row 0 (c / s = 1e3)
        # has a factor of at least 1e3 in every gated entry
        assert np.all(gate[~ruled] < 1e-9)
        sp = ec.correlation_species(n, rank) or list(range(5))
        s = sp.index(ec.SP_OFFSET)
        factor = gate[0, s] / (mc.CORR_C * (n + 16) * EPS)
        assert np.any(np.isfinite(factor)) and np.all(factor[np.isfinite(factor)] >= 1e3), factor


def test_every_input_count_and_tile_edge_is_used():
    assert {ec.shape(n)[2] for n in ec.SMALL_NS} == set(ec.INPUT_PS)
    assert {ec.shape(n)[0] for n in ec.SMALL_NS} == {5, 70} and {ec.shape(n)[1] for n in ec.SMALL_NS + ec.SORTED_NS} == {1, 2, 3}
    for n in ec.SMALL_NS:
        X = ec.inputs(n, ec.shape(n)[2])
        assert X.shape == (n + 5, ec.shape(n)[2]) and (X.shape[1] == 1 or np.all(X[:, -1] == 2.5))


def test_special_values_meet_every_wave_and_both_loops():
    met = set()
    for n in ec.SMALL_NS:
        u, idx = ec.special_block(n), mc.participants(n + 5, ec.mask(n))
        for sp, kind, pos in ec.special_columns():
            q = ec.special_position(n, pos)
            col = u[idx, 0, sp]
            if q is None or (kind == "both" and n < 2):
                assert np.all(np.isfinite(col))
                continue
            bad = np.flatnonzero(~np.isfinite(col))
            if kind == "both":
                assert sorted(bad) == sorted({q, (q + 1) % n}) and col[q] == np.inf and col[(q + 1) % n] == -np.inf
            else:
                assert list(bad) == [q] and (np.isnan(col[q]) if kind == "nan" else col[q] == float(kind + ""))
            met.add((kind,) + moments_place(n, q))
        others = np.ones(70, bool); others[[sp for sp, _, _ in ec.special_columns()]] = False
        assert np.all(np.isfinite(u[:, :, others]))
    for kind in ec.KINDS:
        for w in range(mo.MOM_WAVES):
            # (the last participant is the unrolled loop's fourth load of wave n - 1 - 24 at n = 25 .. 32, the tail loop's otherwise)
            assert (kind, w, False) in met and (kind, w, True) in met, (kind, w)


def test_constant_columns_need_the_flat_rule():
    for n, value in ec.CONSTANT_CASES:
        y = ec.columns_of(ec.constant_block(n, value), ec.mask(n))[:, 1:2]
        assert np.all(y == value)
        yhat, S = mo.replay_values(y, flat_rule=False, want_S=True)
        assert S[0] > 0.0 and np.all(np.abs(yhat) >= 0.4)      # the mean rounds: every deviation is one and the same ulp
        assert np.all(mo.replay_values(y) == 0.0)


def test_sorted_sizes_reach_every_padded_size_and_both_tiles():
    want = {511: (512, 8), 512: (512, 8), 513: (1024, 8), 1024: (1024, 8), 1025: (2048, 8), 2047: (2048, 8), 2048: (2048, 8),
            2049: (4096, 4), 4095: (4096, 4), 4096: (4096, 4)}
    assert {n: ec.sorted_layout(n) for n in ec.SORTED_NS} == want
    assert {ec.sorted_layout(n)[0] for n in ec.SMALL_NS} == {2, 4, 8, 16, 32, 64, 128, 256, 512}
    assert all(ec.sorted_layout(n)[1] == 8 for n in ec.SMALL_NS)
    assert 8 * (2048 + 2) * 8 == 131200 <= 132 * 1024 < 8 * (4096 + 2) * 8      # the largest 8-column image
    for n in ec.SORTED_NS:
        N, L, _ = ec.shape(n)
        T = ec.sorted_layout(n)[1]
        assert (N, L) == (5, 2) and N % T != 0 and (L * N) % T != 0      # a tile crosses the row boundary, the last is ragged
        u, idx = ec.sorted_block(n), mc.participants(n + 5, ec.mask(n))
        assert np.isnan(u[idx, 1, 2]).sum() == 1 and set(u[idx, 0, 3][np.isinf(u[idx, 0, 3])]) == {np.inf, -np.inf}
        assert np.all(np.isfinite(u[idx][:, :, [0, 1, 4]]))
    assert capi.MEMBERS_MAX_SORTED == 4096


def test_probability_vectors():
    for n in ec.SMALL_NS + ec.SORTED_NS:
        vs = ec.probability_vectors(n)
        assert [len(v) for v in vs] == [1, 1] + list(ec.QS)
        for v in vs[3:]:
            assert 0.0 in v and 1.0 in v and np.all((v >= 0.0) & (v <= 1.0))
            h = (n - 1) * v
            inner = (v > 0.0) & (v < 1.0)
            assert n < 3 or np.any(inner & (h == np.floor(h))), n      # (n - 1) p rounds onto an integer
            assert n < 3 or np.any(h != np.floor(h))
    assert 3 * ec.probabilities(4, 1)[0] == 1.0      # 1/3 at n = 4
    # the quantile write-out takes one entry per thread and trip, 256 threads over (columns of the tile) x Q entries: a second
    # trip needs 8 Q > 256, a third 8 Q > 512
    assert 8 * 32 == 256 and 8 * 33 > 256 and 8 * 70 > 512 and 5 * 70 > 256
