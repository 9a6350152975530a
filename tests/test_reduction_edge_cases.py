"""The cases of tests/reduction_edge_cases.py are what they claim (no GPU): the intended rows sit in the intended classes of the
gather plans with the intended lengths, the exact inputs are exact - every sum the same in forward order, in reverse order
and through math.fsum - and every listed degree, row length and in-degree occurs. The GPU tests built on these cases
(test_gpu_reduction_edges.py, test_gpu_reduction_trips.py) then cannot pass by missing their target."""
import numpy as np
import pytest

import drgep_cases as ec
import reduction_edge_cases as rx
from kinetica_jl_amd import capi
from tests import jac_cases as jc
from tests import timescale_cases as tc
from tests.linalg_cases import hub_net

T_CASE = "paired_small"       # the gather case that also runs in the temperature form


def rows_of(g, hub, pairing):
    """the four hub rows: (contribution table, first column of (kf, kr), begin, end) of den A, den B, edge (A, B), edge (B, A)"""
    A, B = hub["A"], hub["B"]
    eAB, eBA = rx.edge_of(g, A, B), rx.edge_of(g, B, A)
    return [(g.den, 1, g.den_ptr[A], g.den_ptr[A + 1]), (g.den, 1, g.den_ptr[B], g.den_ptr[B + 1]),
            (g.num, 2, g.edge_ptr[eAB], g.edge_ptr[eAB + 1]), (g.num, 2, g.edge_ptr[eBA], g.edge_ptr[eBA + 1])]


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(rx.GATHER))
def test_hub_rows_have_the_intended_length_and_class(name, pairing):
    c = rx.gather_case(name)
    g = c.drg(pairing)
    info = capi.drg_pattern_host(c.net, pairing)[2]
    assert info == g.info()                                # the library's plans count the rows by class as the reference does
    assert capi.reaction_importance_plan_host(c.net, pairing)[3] == c.ri(pairing).info()
    f = c.factor(pairing)
    want = {"den": {k: 0 for k in ("short", "medium", "long")}, "edge": {k: 0 for k in ("short", "medium", "long")}}
    for hub in c.hubs:
        n = hub["n"]
        (tab, col, a0, a1), (_, _, b0, b1), (num, ncol, e0, e1), (_, _, f0, f1) = rows_of(g, hub, pairing)
        assert a1 - a0 == f * n + rx.SIDE and b1 - b0 == f * n and e1 - e0 == f * n and f1 - f0 == f * n
        kr_A = tab[a0:a1, col + 1]
        paired = c.family == "paired" and pairing
        assert np.sum(kr_A < 0) == (rx.SIDE if paired else f * n + rx.SIDE)     # the side records never pair
        for t, cc, lo, hi in rows_of(g, hub, pairing)[1:]:
            assert np.all((t[lo:hi, cc + 1] >= 0) == paired)                   # b >= 0 throughout with pairing, b < 0 without
        want["den"][rx.row_class(f * n + rx.SIDE)] += 1; want["den"][rx.row_class(f * n)] += 1
        want["edge"][rx.row_class(f * n)] += 2
    # the hub rows are the only rows of their classes but for the shared colliders' (at most len(hubs) records each: medium)
    for plan in ("den", "edge"):
        assert info[f"{plan}_long"] == want[plan]["long"]
        assert info[f"{plan}_medium"] >= want[plan]["medium"]


def test_every_length_and_class_edge_is_met():
    for name, lengths in (("collider", rx.LENGTHS), ("paired", rx.LENGTHS)):
        c = rx.gather_case(name)
        assert tuple(h["n"] for h in c.hubs) == lengths == (1, 8, 9, 64, 65, 256, 257, 1024, 1025, 2049)
    # at the class limits the edge row and the denominator row of A are in different classes (and passes of a long row)
    assert rx.SHORT_MAX in rx.LENGTHS and rx.row_class(rx.SHORT_MAX) != rx.row_class(rx.SHORT_MAX + rx.SIDE)
    assert rx.SEG_LEN in rx.LENGTHS and rx.row_class(rx.SEG_LEN) != rx.row_class(rx.SEG_LEN + rx.SIDE)
    assert rx.LONG_PASS in rx.LENGTHS and rx.passes(rx.LONG_PASS) == 1 and rx.passes(rx.LONG_PASS + rx.SIDE) == 2
    assert rx.passes(2049) == 3 and rx.passes(2 * 2049) == 5
    # PFA's gather cases cover the lengths as far as E2 allows: the colliders all of them, the pairs up to 257 and 1025
    assert rx.gather_case("paired_small").lengths == rx.LENGTHS[:7] and rx.gather_case("paired_1025").lengths == (1025,)
    for name in rx.PFA_GATHER:
        pairs = capi.pfa_pattern_host(rx.gather_case(name).net, 1)[2]["pairs"]
        assert pairs < 5_000_000, (name, pairs)              # (the largest: about 4 n^2 at n = 1025)
    # the trips tests' lengths are hubs of every gather family
    assert set(rx.TRIP_LENGTHS) <= set(rx.LENGTHS)
    # the paired rows checked by name in the issue: with pairing n contributions, without 2 n
    for n in (9, 257, 1025):
        for name in ("paired", "paired_1025" if n == 1025 else "paired_small"):
            c = rx.gather_case(name)
            hub = next(h for h in c.hubs if h["n"] == n)
            for pairing in (1, 0):
                g = c.drg(pairing)
                lens = [hi - lo for _, _, lo, hi in rows_of(g, hub, pairing)]
                assert lens == [(1 if pairing else 2) * n + (rx.SIDE if i == 0 else 0) for i in range(4)]


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", ["collider", "paired", "paired_1025"])
def test_exact_inputs_sum_the_same_in_any_order(name, pairing):
    c = rx.gather_case(name)
    g, s = c.drg(pairing), c.drgep(pairing)
    assert np.all(c.rates * 4 == np.round(c.rates * 4)) and c.rates.max() <= 32.0 and c.rates.min() >= 0.0
    assert len({c.U[b].tobytes() for b in range(c.B)}) == c.B          # the states differ
    if c.B > rx.ZERO_STATE:
        assert np.all(c.rates[rx.ZERO_STATE] == 0.0)
    z = np.zeros(c.net.n_reactions)
    for b in range(c.B):
        q = c.rates[b]
        for hub in c.hubs:
            for tab, col, lo, hi in rows_of(g, hub, pairing):
                stab = s.den if tab is g.den else s.num            # (the same lists, the last column signed)
                t = g._terms(tab[lo:hi], col, q, z)[0]
                sg = s._terms(stab[lo:hi], col, q, z)[0]
                for terms in (t, sg, np.maximum(sg, 0.0), np.maximum(-sg, 0.0)):
                    fwd, rev, exact = rx.order_sums(terms.tolist())
                    assert fwd == rev == exact and exact * 4 == round(exact * 4)


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(rx.GATHER))
def test_hub_coefficients_are_neither_zero_nor_one(name, pairing):
    """unsigned: 0 < r_AB < 1 in some state; signed: P_A and C_A both non-zero in some state and |s_AB| < den_A there"""
    c = rx.gather_case(name)
    g, s = c.drg(pairing), c.drgep(pairing)
    r = c.ref("drg", pairing)[1]
    r_signed = c.ref("drgep", pairing)
    rp, rcn = c.ref("pfa", pairing)
    z = np.zeros(c.net.n_reactions)
    for hub in c.hubs:
        e = rx.edge_of(g, hub["A"], hub["B"])
        assert np.any((r[:, e] > 0.0) & (r[:, e] < 1.0)), hub
        both = []
        for b in range(c.B):
            lo, hi = s.den_ptr[hub["A"]], s.den_ptr[hub["A"] + 1]
            t = s._terms(s.den[lo:hi], 1, c.rates[b], z)[0]
            both.append(np.maximum(t, 0.0).sum() > 0 and np.maximum(-t, 0.0).sum() > 0)
        both = np.array(both)
        assert np.any(both & (r_signed[:, e] < 1.0) & (r_signed[:, e] > 0.0)), hub
        assert np.any(both & (rp[:, e] + rcn[:, e] > 0.0)), hub
    if c.B > rx.ZERO_STATE:
        assert np.all(r[rx.ZERO_STATE] == 0.0) and np.all(r_signed[rx.ZERO_STATE] == 0.0)


@pytest.mark.parametrize("pairing", [1, 0])
def test_temperature_form_bounds_are_tight(pairing):
    """the condition of drg_cases / drgep_cases / pfa_cases / reaction_importance_cases on the inputs chosen here: at most
    1 % of the compared entries have a bound above 1e-9"""
    c = rx.gather_case(T_CASE)
    bounds = [c.t_ref("drg", pairing)[2], c.t_ref("drgep", pairing)[1], c.t_ref("pfa", pairing)[2], c.t_ref("pfa", pairing)[3],
              c.t_ref("ri", pairing)[2]]
    for b in bounds:
        assert float(np.mean(b > 1e-9)) <= 0.01


# ---- the PFA families ------------------------------------------------------------------------------------------------------
def test_pfa_families_reach_every_listed_size():
    out, m_deg, e2, rem = set(), set(), set(), set()
    for name in rx.PFA_PARTS:
        c = rx.pfa_case(name)
        g = c.g
        rowptr, colidx, info = capi.pfa_pattern_host(c.net, 1)
        assert np.array_equal(rowptr, g.rowptr2) and np.array_equal(colidx, g.colidx2) and info == g.info()
        assert capi.pfa_pattern_host(c.net, 0)[2] == info          # no reaction has a reverse: one pattern for both pairings
        assert g.n <= capi.PFA_MAX_SPECIES and g.E2 < 300000
        row2 = np.diff(g.rowptr2)
        for kind, p, q, A, M in c.where:
            out.add(int(g.deg[A])); m_deg.add(int(g.deg[M])); e2.add(int(row2[A]))
            if kind == "ds":
                assert g.deg[A] == p and g.deg[M] == q and row2[A] == p + q - 1
                leaves = [s for s in g.cols[g.rowptr[A]:g.rowptr[A + 1]] if s != M]
                assert all(g.deg[s] == 1 for s in leaves)
            else:
                assert g.deg[A] == p and g.deg[M] == q + 1 and row2[A] == p * (q + 1)
        for d in g.deg:                                            # the staged chunks of every row
            rem.update(min(capi.PFA_CHUNK, int(d) - c0) % capi.PFA_AHEAD for c0 in range(0, int(d), capi.PFA_CHUNK))
    assert set(rx.OUT_DEGREES) <= out and set(rx.M_DEGREES) <= m_deg and set(rx.E2_ROWS) <= e2
    assert rem == {0, 1, 2, 3}
    # the lists sit on the kernel's limits
    assert {capi.PFA_CHUNK - 1, capi.PFA_CHUNK, capi.PFA_CHUNK + 1, 2 * capi.PFA_CHUNK, 2 * capi.PFA_CHUNK + 1} <= set(rx.OUT_DEGREES)
    assert {64, 65, 256, 257} == set(rx.M_DEGREES)
    assert {capi.PFA_KEEP * 64, capi.PFA_KEEP * 64 + 1, capi.PFA_KEEP * 256, capi.PFA_KEEP * 256 + 1} <= set(rx.E2_ROWS)


@pytest.mark.parametrize("d,m", rx.DS_SIZES)
def test_double_star_sizes(d, m):
    net, where = rx.union([("ds", d, m)])
    rowptr, colidx, info = capi.drg_pattern_host(net, 1)
    rowptr2, _, info2 = capi.pfa_pattern_host(net, 1)
    _, _, _, A, M = where[0]
    assert rowptr[A + 1] - rowptr[A] == d and rowptr[M + 1] - rowptr[M] == m
    assert rowptr2[A + 1] - rowptr2[A] == d + m - 1
    for leaf in colidx[rowptr[A]:rowptr[A + 1]]:
        if leaf != M:
            assert rowptr[leaf + 1] - rowptr[leaf] == 1 and colidx[rowptr[leaf]] == A
    assert info2["pairs"] == (d - 1) * d + (m - 1) * m + 2 * (d + m - 1)
    if (d, m) in ((129, 1408), (3, 1535)):              # the register columns of a workgroup, and one more
        assert d + m - 1 == capi.PFA_KEEP * 256 + (1 if d == 3 else 0)


@pytest.mark.parametrize("name", sorted(rx.PFA_PARTS))
def test_pfa_second_stage_inputs_are_exact(name):
    c = rx.pfa_case(name)
    g, ref = c.g, c.r()
    assert set(np.unique(c.rp)) | set(np.unique(c.rc)) == {0.0, 0.25, 0.5, 1.0}
    assert len({c.rp[b].tobytes() + c.rc[b].tobytes() for b in range(len(c.rp))}) == len(c.rp)
    assert np.all(ref[rx.ZERO_STATE] == 0.0) and np.all(ref * 16 == np.round(ref * 16))
    z = np.concatenate([g.z1, g.z1, g.z2, g.z2])
    for b in range(len(c.rp)):
        rp, rcn = c.rp[b], c.rc[b]
        v = np.concatenate([rp, rcn, rp[g.e1] * rp[g.e2], rcn[g.e1] * rcn[g.e2]])
        fwd, rev = np.zeros(g.E2), np.zeros(g.E2)
        np.add.at(fwd, z, v)                                       # (unbuffered: one addition after the other)
        np.add.at(rev, z[::-1], v[::-1])
        assert np.array_equal(fwd, ref[b]) and np.array_equal(rev, ref[b])
    # every row A holds values of more than one state, some of them above 1 (r is not clipped)
    for _, _, _, A, _ in c.where:
        row = ref[:, g.rowptr2[A]:g.rowptr2[A + 1]]
        assert np.sum(np.any(row > 0.0, axis=1)) >= 2
    assert ref.max() > 1.0


# ---- the path family -------------------------------------------------------------------------------------------------------
def test_path_family_reaches_every_in_degree_class_edge():
    c = rx.path_case()
    assert (capi.DRGEP_IN_SHORT_MAX, capi.DRGEP_IN_WAVE_MAX) == (32, 256)
    assert rx.IN_DEGREES == (capi.DRGEP_IN_SHORT_MAX, capi.DRGEP_IN_SHORT_MAX + 1, capi.DRGEP_IN_WAVE_MAX, capi.DRGEP_IN_WAVE_MAX + 1,
                             2 * 256, 2 * 256 + 1)                 # (256: the workgroup's stride over a long species' edges)
    for kind, d, m, A, M in c.where:
        assert c.in_deg[A] == d and c.in_deg[M] == m
    assert set(rx.IN_DEGREES) <= {int(c.in_deg[A]) for _, _, _, A, _ in c.where}
    assert any(c.in_deg[A] > capi.DRGEP_IN_WAVE_MAX and c.in_deg[M] > capi.DRGEP_IN_WAVE_MAX for _, _, _, A, M in c.where)
    cls = ec.in_degree_classes(c.g.cols, c.g.n, capi.DRGEP_IN_SHORT_MAX, capi.DRGEP_IN_WAVE_MAX)
    assert cls[1] == 2 and cls[2] == 5                             # 33 and 256 by a wavefront; 257, 512, 513, 513 and the M of 257 by the workgroup
    # the planted winner: every centre is reached at 0.5 over its last incoming edge, from a leaf
    imp, R, rounds = c.g.importance(c.planted, c.leaves)
    assert np.all(imp[c.centres] == 0.5)
    for s in c.centres:
        e_in = np.flatnonzero(c.g.cols == s)
        assert c.planted[0, e_in[-1]] == 0.5 and np.all(c.planted[0, e_in[:-1]] == 0.25) and c.g.rows[e_in[-1]] in c.leaves


# ---- timescale: the hub and fan-in cases of the trips tests ----------------------------------------------------------------
@pytest.mark.parametrize("L", rx.TRIP_LENGTHS)
def test_timescale_cases_of_the_trips_tests(L):
    assert int(jc.Reference(hub_net(L)).L_jac.max()) == L
    info = capi.timescale_plan_host(tc.fan_in_net(L - 1))
    cls = "rows_short" if L <= capi.TIMESCALE_SHORT_MAX else "rows_medium" if L <= capi.TIMESCALE_WAVE_MAX else "rows_long"
    assert info[cls] >= 1 and (cls == "rows_short" or info[cls] == 1)
