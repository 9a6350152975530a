"""GPU tests of the cross-member statistics by their documented sum order and at every edge of the four kernels of
member_stats_kernels.hip (cases: member_stats_edge_cases.py, proved on the CPU by test_member_stats_edge_cases.py; orders:
member_stats_order.py). test_gpu_member_stats.py asserts the accuracy of the algorithms through derived gates; this file asserts
the ORDER the header promises, which a gate cannot see, and the paths the gates' cases never reach.

What is asserted, n the participants (K = n + 5 members, a seeded mask; odd n: without the first and the last member):
  moments        count, min, max exact; mean and variance bit for bit replay_moments on every finite column, n = 1 .. 40, 63 .. 65,
                 255 .. 257; the exact-integer column bit for bit an expectation formed in Python integers; a NaN, a +Inf, a -Inf
                 and both infinities at participant positions 0, 1, 7, 8 and n - 1 against IEEE arithmetic on the header's rules
  quantiles      bit for bit ref_quantiles at the same n and at n = 511 .. 4 096 (every padded size, the 8- and the 4-column
                 tile), Q = 1, 32, 33, 70, with a species list and under KIN_MEMBERS_BLOCK_COLUMNS = 1 and 3 at n = 2 049 and 4 096
  correlations   bit for bit replay_corr(Xhat, replay_ranks / replay_values) on every finite column (Xhat from
                 capi.members_inputs, the host function the library calls), P = 1, 15, 16, 17, 33, AND within the derived gate of
                 member_stats_cases.ref_correlate; Pearson on offset columns 1 + z / 1 000 (gate factor >= 1e3, gate < 1e-9);
                 constant columns 0.1 and 0.7, whose mean rounds, correlate as exactly 0.0
  _dev entries   on a stream of the caller's, byte for byte the host entries
Zeros are compared by value, NaN equals NaN. The replays take FP64 division and square root on the device as correctly
rounded. On an MI355X they are (the build has no fast-math flag): every quotient and root of this file - the mean, the variance,
both Yhat - is bit for bit NumPy's, so no result needed the propagated 2 EPS gate; mutants p, q and s below (a reciprocal and a
product in place of the quotient) show the tests would have seen a last-bit difference. Largest error over the derived gate of
the gated correlation entries: 0.020 (Pearson), 0.006 (Spearman).

Mutation check (one change of member_stats_kernels.hip at a time in a scratch build selected through KIN_LIB_PATH, nothing of it
committed; every mutation keeps all index ranges and barriers; one pytest process per mutant and test set, on an MI355X). "new"
is this file (254 tests), "previous" test_gpu_member_stats.py and test_gpu_ensemble_statistics.py (128 tests). Tests named
without their prefix test_; m_order = moments_in_the_documented_order, special = special_values_at_every_participant_position,
spearman / pearson = *_in_the_documented_order, constant = constant_columns_whose_mean_rounds_correlate_as_zero.
  mutant                                                             new                                          previous
  a moments: no NaN-flag merge for waves k >= 1                      45 fail: special (every n > 1)               all pass
  b moments: x[3] added before x[2] in the unrolled loop             29 fail: m_order 13, special 16              all pass
  c moments: d * d + S for __fma_rn in the second pass               64 fail: m_order 26, special 38              all pass
  d values: no `flat` rule                                           3 fail: constant (0.1 at n = 3, 6; 0.7)      all pass
  e values: the 32 partials added in the order l = 31 .. 0           43 fail: pearson                             all pass
  f product: Xs loaded without pb                                    41 fail: spearman 19, pearson 19, constant 3 all pass
  g sorted: the quantile write-out's `for` an `if`                   57 fail: quantiles 56, device_entries        all pass
  h sorted: e & 7 for e & (T - 1) in the gather (*)                  6 fail: quantiles, spearman at n > 2 048     1 fails (the participant limit)
  i sorted: padded with 0.0 for +Inf                                 131 fail                                     64 fail
  j sorted: < for <= in the second binary search                     103 fail                                     38 fail
  k values: d * d + S for __fma_rn                                   6 fail: pearson                              all pass
  l product: x * y + acc for __fma_rn                                97 fail: spearman 53, pearson 44             all pass
  m moments: first pass's wave partials added in the order 7 .. 0    85 fail: m_order 42, special 43              all pass
  n moments: second pass's wave partials added in the order 7 .. 0   87 fail: m_order 43, special 44              all pass
  o sorted: a.c0 dropped from the tile's column offsets              4 fail: quantiles, spearman under blocking   2 fail (blocking)
  p values: d * (1 / root) for d / root                              44 fail: pearson                             all pass
  q sorted: d * (1 / sqrt(S)) for d / sqrt(S)                        52 fail: spearman                            all pass
  s moments: t * (1 / n) for t / n                                   69 fail: m_order 32, special 37              all pass
(*) with the LDS store kept inside the tile's image (`if (t < T)`): the literal change would store past it at T = 4, and at
T = 8 it changes nothing. No mutant survives the new file; a to g, k to n and p to s pass everything there was before; h, i, j
and o are controls the previous files catch as well.

Wall time of this file on one MI355X: 254 tests in 6.9 s (the slowest, 1.7 s, is the first: it creates the handle)."""
import numpy as np
import pytest

import member_stats_cases as mc
import member_stats_edge_cases as ec
import member_stats_order as mo
from kinetica_jl_amd import capi

pytestmark = pytest.mark.gpu
P7 = np.array([0.0, 0.05, 0.25, 0.5, 0.77, 0.95, 1.0])
LISTED = {2049: (4, 0, 2), 4096: (4, 0, 2)}      # sorted sizes that also run with a species list under two blockings

_handles = {}
worst = {"spearman": 0.0, "pearson": 0.0}       # largest error over gate seen (printed by the tests for the record)


def handle(N):
    if N not in _handles:
        _handles[N] = capi.HipNetwork(*mc.chain_network(N))
    return _handles[N]


def same(got, want, what):
    assert mc.same_bits_or_zero(got, want), (what, mc.mismatches(got, want))


@pytest.mark.parametrize("n", ec.SMALL_NS)
def test_moments_in_the_documented_order(n):
    u, use = ec.mixed_block(n), ec.mask(n)
    got, ref = handle(u.shape[2]).members_moments(u, use=use), mc.ref_moments(u, use)
    assert got["count"] == n
    same(got["min"], ref["min"], "min"); same(got["max"], ref["max"], "max")
    mean, var = ec.expected_moments(n)
    same(got["mean"], mean, "mean"); same(got["var"], var, "var")
    em, ev = ec.exact_moments(n)      # independent of the replay
    same(got["mean"][:, ec.SP_EXACT], em, "exact mean"); same(got["var"][:, ec.SP_EXACT], ev, "exact var")


@pytest.mark.parametrize("n", ec.SMALL_NS)
def test_special_values_at_every_participant_position(n):
    """A NaN / +Inf / -Inf / both infinities at positions 0, 1, 7, 8, n - 1: every wave of the moments and both of its loops
    carry one (the CPU file shows which). NaN: all four NaN. One infinity: that mean and extreme, NaN variance. Both: NaN mean
    and variance, infinite extremes. The sorted and the value pass see the same columns."""
    u, use = ec.special_block(n), ec.mask(n)
    h = handle(70)
    got, ref = h.members_moments(u, use=use), mc.ref_moments(u, use)
    assert got["count"] == n
    special = ~np.isfinite(ref["abs_mean"])
    for q in ("mean", "var", "min", "max"):
        same(got[q][special], ref[q][special], q)      # (NumPy's IEEE arithmetic on the same rules; spelled out below)
    same(got["min"], ref["min"], "min"); same(got["max"], ref["max"], "max")
    for sp, kind, pos in ec.special_columns():
        if ec.special_position(n, pos) is None or (kind == "both" and n < 2):
            continue
        m, v, lo, hi = (got[q][0, sp] for q in ("mean", "var", "min", "max"))
        if kind == "nan":
            assert np.isnan([m, v, lo, hi]).all(), (sp, kind, pos)
        elif kind == "both":
            assert np.isnan(m) and np.isnan(v) and lo == -np.inf and hi == np.inf, (sp, kind, pos)
        else:
            s = float(kind)
            assert m == s and np.isnan(v) and (hi if s > 0 else lo) == s and (n == 1 or np.isfinite(lo if s > 0 else hi)), (sp, kind, pos)
    fin = np.isfinite(ref["abs_mean"])[0]
    mean, var = mo.replay_moments(ec.columns_of(u, use)[:, fin])
    same(got["mean"][0, fin], mean, "finite mean"); same(got["var"][0, fin], var, "finite var")
    # the column passes over the special columns and four finite ones
    sp = [s for s, _, _ in ec.special_columns()] + [20, 63, 64, 69]
    same(h.members_quantiles(u, P7, species=sp, use=use), mc.ref_quantiles(u, P7, sp, use), "quantiles")
    X = mc.inputs(n + 5)
    for rank in (True, False):
        check_gate(h.members_correlate(u, X, species=sp, rank=rank, use=use), *mc.ref_correlate(u, X, sp, rank, use), None)


def check_gate(got, ref, gate, key):
    ruled = np.isinf(gate)                                  # 0.0 or NaN by rule: compared exactly
    same(got[ruled], ref[ruled], "entries set by rule")
    err = np.abs(got[~ruled] - ref[~ruled])
    ratio = float(np.max(err / gate[~ruled], initial=0.0))
    assert np.all(np.isfinite(got[~ruled])) and np.all(err <= gate[~ruled]), ratio
    if key:
        worst[key] = max(worst[key], ratio)
        print(f"{key}: error over gate {ratio:.4f} (largest so far {worst[key]:.4f})")


def quantile_block(n):
    return ec.sorted_block(n) if n in ec.SORTED_NS else ec.mixed_block(n)


@pytest.mark.parametrize("n", ec.SMALL_NS + ec.SORTED_NS)
def test_quantiles(n, monkeypatch):
    u, use = quantile_block(n), ec.mask(n)
    h = handle(u.shape[2])
    lists = [None] + ([list(ec.WIDE_SPECIES)] if u.shape[2] == 70 else [])
    for sp in lists:
        for p in ec.probability_vectors(n):
            same(h.members_quantiles(u, p, species=sp, use=use), mc.ref_quantiles(u, p, sp, use), (sp, len(p)))
    if n in LISTED:
        sp = list(LISTED[n])
        for cols in ("1", "3"):
            monkeypatch.setenv("KIN_MEMBERS_BLOCK_COLUMNS", cols)
            for p in ec.probability_vectors(n)[2:]:
                same(h.members_quantiles(u, p, species=sp, use=use), mc.ref_quantiles(u, p, sp, use), (sp, cols, len(p)))


def correlation(n, rank, block, species=None):
    u, use = (ec.sorted_block if block == "sorted" else ec.mixed_block)(n), ec.mask(n)
    N, _, P = ec.shape(n)
    sp = ec.correlation_species(n, rank) if species is None else list(species)
    got = handle(N).members_correlate(u, ec.inputs(n, P), species=sp, rank=rank, use=use)
    r, ok, ref, gate = ec.expected_correlation(n, rank, block, species)
    same(got[ok], r[ok], "order")
    check_gate(got, ref, gate, "spearman" if rank else "pearson")
    return got


@pytest.mark.parametrize("n", ec.SMALL_NS + ec.SORTED_NS)
def test_spearman_in_the_documented_order(n, monkeypatch):
    correlation(n, True, "sorted" if n in ec.SORTED_NS else "mixed")
    if n in LISTED:
        for cols in ("1", "3"):
            monkeypatch.setenv("KIN_MEMBERS_BLOCK_COLUMNS", cols)
            correlation(n, True, "sorted", LISTED[n])


@pytest.mark.parametrize("n", ec.SMALL_NS)
def test_pearson_in_the_documented_order(n):
    correlation(n, False, "mixed")


@pytest.mark.parametrize("n,value", ec.CONSTANT_CASES)
def test_constant_columns_whose_mean_rounds_correlate_as_zero(n, value):
    u, use, X = ec.constant_block(n, value), ec.mask(n), ec.inputs(n, 17)
    for rank in (False, True):
        got = handle(5).members_correlate(u, X, rank=rank, use=use)
        assert np.all(got[0, 1] == 0.0), (rank, got[0, 1])
        check_gate(got, *mc.ref_correlate(u, X, None, rank, use), None)


def test_device_entries_on_a_stream_of_the_callers():
    import torch
    n = 65
    u, use = ec.mixed_block(n), ec.mask(n)
    K, L, N = u.shape
    h, X, sp, p = handle(N), ec.inputs(n, 17), [4, 63, 2, 0], ec.probabilities(n, 33)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_u = torch.tensor(u, dtype=torch.float64, device="cuda:0")
        new = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda:0")
        d_m = [new(L, N) for _ in range(4)]
        d_q, d_r, d_p = new(len(p), L, len(sp)), new(L, N, 17), new(L, len(sp), 17)
        s = stream.cuda_stream
        assert s != 0
        cnt = h.members_moments_dev(K, L, d_u.data_ptr(), use=use, d_mean=d_m[0].data_ptr(), d_var=d_m[1].data_ptr(),
                                    d_min=d_m[2].data_ptr(), d_max=d_m[3].data_ptr(), stream=s)
        h.members_quantiles_dev(K, L, d_u.data_ptr(), p, d_q.data_ptr(), species=sp, use=use, stream=s)
        h.members_correlate_dev(K, L, d_u.data_ptr(), X, d_r.data_ptr(), rank=True, use=use, stream=s)
        h.members_correlate_dev(K, L, d_u.data_ptr(), X, d_p.data_ptr(), species=sp, rank=False, use=use, stream=s)
        stream.synchronize()
        out = [t.cpu().numpy() for t in d_m + [d_q, d_r, d_p]]
    m = h.members_moments(u, use=use)
    assert cnt == m["count"] == n
    want = [m[q] for q in ("mean", "var", "min", "max")] + [h.members_quantiles(u, p, species=sp, use=use),
                                                            h.members_correlate(u, X, rank=True, use=use),
                                                            h.members_correlate(u, X, species=sp, rank=False, use=use)]
    for i, (a, b) in enumerate(zip(out, want)):
        assert a.tobytes() == b.tobytes(), i
