"""CPU checks of tests/cache_cases.py, the references tests/test_gpu_lu_cache.py judges the LU cache with: the drift reference
against rationals on the exact cases, the derived bound on a plain float64 evaluation of the formula, the conditions the cases
promise (spike placement, slot counts, every special value, thresholds away from the bound), the slot-rule table's edges - and
the same cases through the three statements of the rules that need no device: the templates of bdf_rules.hpp with
HostBackend::drift_check (tests/native/resident_host.cpp) and oracle/bdf.py."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import bdf as obdf
from tests import cache_cases as cc
from tests import res_host
from tests.jac_cases import Reference

HOST = cc.host_cases()
RES = cc.resident_cases()
ROWS = cc.slot_rule_rows()
ALL = [c for _, cs in HOST + RES for c in cs] + cc.special_net_cases(cc.special_net().n_species)


def test_reference_is_exact_on_the_exact_cases():
    n = 0
    for case in ALL:
        if not case.exact:
            continue
        for s in range(case.ns):
            assert Fraction(float(case.ref[s])) == cc.drift_exact(case.c[s], case.jd_old[s], case.jd_now)
            n += 1
        # ... and so is plain float64: nothing rounds
        assert np.array_equal(cc.drift_float64(case.c, case.valid, case.jd_old, case.jd_now), case.ref)
    assert n >= 5 * (len(cc.HOST_N) + len(cc.RES_N))
    both = [c for c in ALL if c.exact and c.ns == 4][0]
    assert list(both.ref[:2]) == [1.0, 1.0] and not both.dropped[:2].any()             # M_old / M_new = 2 and 1 / 2: kept at 1.0
    ulp = [c for c in ALL if c.exact and c.ns == 1][0]
    assert ulp.jd_old[0, 0] == -(3.0 + 2.0 ** -50) and ulp.ref[0] == 1.0 + 2.0 ** -51 and ulp.dropped[0]


def test_bound_holds_for_float64_numpy():
    worst = 0.0
    for case in ALL:
        got = cc.drift_float64(case.c, case.valid, case.jd_old, case.jd_now)
        fin = np.isfinite(case.ref)
        assert np.all(np.abs(got[fin] - case.ref[fin]) <= case.bound[fin]), case.name
        assert np.all(got[~fin] >= cc.UNBOUNDED), case.name
        assert np.array_equal(cc.decisions(got, case.valid, case.max_drift), case.dropped), case.name
        nz = fin & (case.bound > 0)
        if nz.any():
            worst = max(worst, float(np.max(np.abs(got[nz] - case.ref[nz]) / case.bound[nz])))
    assert 0.0 < worst <= 1.0
    print(f"float64 NumPy: worst error / bound {worst:.3f}")


def test_case_conditions():
    for cases, sizes, slots, cap in ((HOST, cc.HOST_N, cc.HOST_SLOTS, cc.LU_MAX_SLOTS), (RES, cc.RES_N, cc.RES_SLOTS, cc.RES_MAX_SLOTS)):
        assert tuple(N for N, _ in cases) == sizes and max(slots) == cap
        seen_slots, seen_spikes = set(), set()
        for N, cs in cases:
            for case in cs:
                assert case.N == N and 1 <= case.ns <= cap
                seen_slots.add(case.ns)
                for s in range(case.ns):
                    diff = np.flatnonzero(case.jd_old[s] != case.jd_now)
                    if case.name.startswith(("placement", "slots", "exact")):
                        assert len(diff) == 1                                         # single spike: every other element has drift 0
                        seen_spikes.add((N, int(diff[0])))
            pl = cs[0]
            assert sorted(int(np.flatnonzero(pl.jd_old[s] != pl.jd_now)[0]) for s in range(pl.ns)) == cc.spike_positions(N)
            assert len(set(pl.c)) == pl.ns
        assert set(slots) <= seen_slots
        for N in sizes:
            for p in (0, 63, 64, 1023, 1024, N - 1):
                assert p >= N or (N, p) in seen_spikes
    mixed = [c for _, cs in HOST + RES for c in cs if c.name.startswith("slots") and c.ns >= 8]
    assert mixed and all(0 < c.valid.sum() < c.ns for c in mixed)
    for c in mixed:
        assert np.all(c.ref[c.valid == 0] == 0.0) and not c.dropped[c.valid == 0].any()
    assert any(c.dropped.any() and not c.dropped[c.valid != 0].all() for c in mixed)
    # growth and shrinkage of the diagonal both lead to drops somewhere
    grow = shrink = False
    for c in ALL:
        for s in np.flatnonzero(c.dropped & np.isfinite(c.ref)):
            p = np.flatnonzero(c.jd_old[s] != c.jd_now)
            if len(p) == 1:
                q = (1 - c.c[s] * c.jd_old[s, p[0]]) / (1 - c.c[s] * c.jd_now[p[0]])
                grow |= q > 1; shrink |= q < 1
    assert grow and shrink
    names = {c.name.split(" N=")[0] for c in ALL}
    assert {"NaN today", "NaN saved", "sign change", "M_new zero", "positive diagonal", "never a reactant", "poisoned off-diagonals"} <= names
    for c in ALL:
        if c.name.startswith("M_new zero"):
            assert 1.0 - c.c[1] * c.jd_now[c.N // 3] == 0.0
        if c.name.startswith("sign change"):
            assert 1.0 - c.c[1] * c.jd_now[c.N // 3] < -2.9
        if c.name.startswith("positive diagonal"):
            assert 0.7 < c.c[1] * c.jd_now[c.N // 3] < 0.8
        if c.name.startswith("never a reactant"):
            assert c.jd_now[c.N // 3] == 0.0 and np.all(c.jd_old[:, c.N // 3] == 0.0)


def test_slot_rule_table_edges():
    exp = {name: e for name, _, _, e in ROWS}
    assert exp["empty"] == [(-1, None)] and exp["all invalid"] == [(-1, 0)]
    assert exp["exact tie"] == [(1, 3), (1, 3)]
    assert [n for n, _ in exp["band edge"]] == [0, -1, 0, -1]
    assert [n for n, _ in exp["restart age"]] == [0, 0, -1, 1, 0, -1]
    assert [n for n, _ in exp["step age"]] == [0, 1, 0, -1, 1, 0, -1]
    assert exp["nearest outside the band"] == [(1, 0), (0, 0)]
    assert [v for _, v in exp["first free"]] == [1, 1, 1, 0] and [v for _, v in exp["first expired"]] == [2, 3, 0]
    assert [v for _, v in exp["lru"]] == [1, 0, 1]
    assert exp["beyond n_slots"] == [(1, 1), (2, 2), (2, 3), (0, 0)]
    assert exp["full 64"][0] == (3, 17) and exp["full 128"][0] == (3, 17)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_slot_rules_through_the_host_templates(row):
    name, t, qs, exp = row
    for q, (near, victim) in zip(qs, exp):
        got = res_host.slot_rules(t, q)
        assert got[0] == near, (name, q)
        assert victim is None or got[1] == victim, (name, q)


@pytest.mark.parametrize("row", [r for r in ROWS if len(r[1]["valid"]) > 0], ids=[r[0] for r in ROWS if len(r[1]["valid"]) > 0])
def test_slot_rules_through_the_oracle(row):
    """oracle/bdf.py keeps valid slots only, in a list: the table's valid entries below n_slots, in order"""
    name, t, qs, exp = row
    for q, (near, _) in zip(qs, exp):
        idx = [i for i in range(min(q["n_slots"], len(t["valid"]))) if t["valid"][i]]
        slots = [dict(c_fact=float(t["c_fact"][i]), jac_stamp=int(t["jac_stamp"][i]), step_stamp=int(t["step_stamp"][i])) for i in idx]
        got = obdf.nearest_slot(slots, q["c"], q["band"], q["n_restarts"], q["max_age"], q["n_steps"], q["step_age"])
        assert (idx[got] if got >= 0 else -1) == near, (name, q)


def test_drift_cases_through_the_oracle():
    for case in ALL:
        for s in np.flatnonzero(case.valid):
            got = obdf.slot_drift(case.c[s], case.jd_old[s], case.jd_now)
            if np.isfinite(case.ref[s]):
                assert abs(got - case.ref[s]) <= case.bound[s], (case.name, s)
                assert not case.exact or got == case.ref[s]
            else:
                assert got >= cc.UNBOUNDED, (case.name, s)
            assert (not got <= case.max_drift) == bool(case.dropped[s]), (case.name, s)


@pytest.mark.parametrize("N", sorted(set(cc.RES_N) | {1025}))
def test_drift_cases_through_the_host_replay(N):
    """HostBackend::factor's copy of the diagonal and HostBackend::drift_check's decisions"""
    cases = dict(HOST).get(N, []) + [c for c in dict(RES).get(N, []) if N not in dict(HOST)]
    if N == 65:
        cases = cases + [c for c in dict(RES)[65] if c.name.startswith("slots")]
    net = cc.chain_net(N)
    ref = Reference(net)
    hr = res_host.HostResident(net)
    for case in cases:
        jv_slots, jv_now = cc.jac_values(case, ref.rowptr, ref.cols)
        jd, after, n = hr.drift_check(jv_slots, case.c, case.valid, jv_now, case.max_drift)
        assert np.array_equal(jd, case.jd_old, equal_nan=True), case.name
        assert np.array_equal(after != 0, (case.valid != 0) & ~case.dropped), case.name
        assert n == int(case.dropped.sum()), case.name
    hr.close()


def test_oracle_counts_dropped_slots():
    """n_lu_dropped of oracle/bdf.py: a rate jump between two segments drops slots, unchanged rates drop none"""
    net = cc.chain_net(6)
    from oracle import oracle as orc
    on = orc.OracleNetwork.from_flat(net)
    k = np.full(net.n_reactions, 100.0)
    u0 = np.full(6, 1.0 / 6); u0[0] += 0.01
    out = {}
    for name, f in (("same", 1.0), ("up", 16.0)):
        table = np.stack([k, k * f])
        _, _, rc, st = obdf.solve_network_oracle(lambda kk: (lambda y: on.rhs(kk, y)), lambda kk: (lambda y: on.jac(kk, y)), 6,
                                                 dict(tspan=(0.0, 2.0), solve_chunks=False, save_interval=1.0), u0,
                                                 tstops=np.array([0.0, 1.0]), k_of_stop=lambda i: table[i])
        assert rc == 0
        out[name] = st
    assert out["same"]["n_lu_dropped"] == 0 and 1 <= out["up"]["n_lu_dropped"] <= out["up"]["n_factor"]
