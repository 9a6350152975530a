"""CPU tests of the flux-pass case list (flux_cases.py) against the plan query kin_flux_plan_host, which needs no device: every
case takes the instantiation it is named after, the cases together take every instantiation the launchers can dispatch and the
plans of the benchmark configurations, and the references are self-consistent."""
import math

import numpy as np
import pytest

from kinetica_jl_amd import capi

import flux_cases as fc

CASES = fc.all_cases()
N_CUS = (256, 64)


@pytest.fixture(autouse=True)
def _no_row_override(monkeypatch):
    monkeypatch.delenv("KIN_FLUX_ROWS", raising=False)


def _reached(monkeypatch, n_cu):
    """What the plan query says the cases run: {(path, rows, many parts, k mode, rates mode)}, {(path, rows, many parts, k mode)}."""
    sweep, seg = set(), set()
    for c in CASES:
        monkeypatch.setenv("KIN_FLUX_LDS", c.lds)
        for v in c.variants:
            q = fc.query(c, v, n_cu, 3)
            sweep.add((q["path"], q["rows"], q["parts"] > 1, q["k_mode"], q["rates_mode"]))
        for v in c.seg_variants:
            q = fc.query(c, v, n_cu, fc.S_ * fc.L_, segmented=True)
            seg.add((q["path"], q["rows"], q["parts"] > 1, q["k_mode"]))
    return sweep, seg


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_takes_the_instantiation_it_is_named_after(case, monkeypatch):
    monkeypatch.setenv("KIN_FLUX_LDS", case.lds)
    for n_cu in N_CUS:
        G = fc.g_max(n_cu, case.parts)
        for v in case.variants:
            for B in fc.batch_sizes(case.n, G):
                q = fc.query(case, v, n_cu, B)
                assert fc.as_inst(q) == case.inst(v), (n_cu, v, B)
                assert q["G"] == min(B, G)
        for v in case.seg_variants:
            q = fc.query(case, v, n_cu, fc.S_ * fc.L_, segmented=True)
            assert fc.as_seg_inst(q) == case.seg_inst(v), (n_cu, v)


def test_the_cases_reach_every_instantiation_the_launchers_dispatch(monkeypatch):
    # flux_go_rows: ROWS 1, 2, 4, 8 on path 0 and 1, 2, 4 on paths 1 and 2 for K16 / K8, ROWS 1, 2 for the temperature form, each with
    # RATES 0, 1, 2: 78; flux_seg_go_rows: ROWS 1, 2, 4 for K16 / K8 and 1, 2 for the temperature form on every path: 24
    want_sweep, want_seg = fc.allowed_instantiations()
    assert len(want_sweep) == 78 and len(want_seg) == 24
    for n_cu in N_CUS:
        sweep, seg = _reached(monkeypatch, n_cu)
        got_sweep = {(p, r, m, x) for p, r, _, m, x in sweep}
        got_seg = {(p, r, m) for p, r, _, m in seg}
        assert not (want_sweep - got_sweep), f"per-state pass, (path, rows, k mode, rates mode) never run: {sorted(want_sweep - got_sweep)}"
        assert not (want_seg - got_seg), f"segmented pass, (path, rows, k mode) never run: {sorted(want_seg - got_seg)}"
        assert not (got_sweep - want_sweep) and not (got_seg - want_seg)      # ... and nothing the launchers would refuse


@pytest.mark.parametrize("n,R", [(10000, 50000), (50000, 250000)])
def test_the_plans_of_the_benchmark_configurations_are_reached(n, R, monkeypatch):
    sweep, seg = _reached(monkeypatch, 256)
    monkeypatch.delenv("KIN_FLUX_LDS", raising=False)
    for temperature, rates_bits in ((False, None), (False, 0), (True, 0)):       # flux alone; what DRG, DRGEP and PFA ask for
        q = capi.flux_plan_host(n, R, 600, 256, temperature_form=temperature, rates_bits=rates_bits)
        assert q["parts"] > 1
        assert (q["path"], q["rows"], True, q["k_mode"], q["rates_mode"]) in sweep, q
        q = capi.flux_plan_host(n, R, 600, 256, temperature_form=temperature, segmented=True)
        assert (q["path"], q["rows"], True, q["k_mode"]) in seg, q
    # the two plans themselves (flux_kernels.hip: flux_plan)
    q = capi.flux_plan_host(n, R, 600, 256, rates_bits=0)
    assert (q["path"], q["rows"], q["parts"]) == ((0, 8, 4) if n == 10000 else (2, 4, 31))


def test_the_query_reads_the_switches_of_a_real_call(monkeypatch):
    base = capi.flux_plan_host(1000, 5000, 600, 256)
    assert (base["path"], base["rows"], base["parts"], base["G"], base["k_mode"], base["rates_mode"]) == (0, 4, 1, 256, fc.K16, 0)
    monkeypatch.setenv("KIN_FLUX_ROWS", "1")
    q = capi.flux_plan_host(1000, 5000, 600, 256)
    assert (q["rows"], q["parts"], q["G"]) == (1, 3, 85)
    monkeypatch.setenv("KIN_FLUX_LDS", "0")
    assert capi.flux_plan_host(1000, 5000, 600, 256)["path"] == 2
    monkeypatch.delenv("KIN_FLUX_LDS")
    monkeypatch.delenv("KIN_FLUX_ROWS")
    # the alignment rules: an odd R, an odd stride or a k row 8 bytes off take 8-byte loads; a shared row does not care about R's stride
    assert capi.flux_plan_host(1000, 4999, 7, 256, rates_bits=0)["k_mode"] == fc.K8
    assert capi.flux_plan_host(1000, 4999, 7, 256, rates_bits=0)["rates_mode"] == 2
    assert capi.flux_plan_host(1000, 5000, 7, 256, k_stride=5001)["k_mode"] == fc.K8
    assert capi.flux_plan_host(1000, 5000, 7, 256, k_stride=0, k_bits=8)["k_mode"] == fc.K8
    assert capi.flux_plan_host(1000, 5000, 7, 256, k_stride=0)["k_mode"] == fc.K16
    assert capi.flux_plan_host(1000, 5000, 7, 256, temperature_form=True, k_bits=8)["k_mode"] == fc.KT
    assert capi.flux_plan_host(1000, 5000, 7, 256, u_bits=8)["path"] == 1
    assert capi.flux_plan_host(1000, 5000, 7, 256, segmented=True)["rows"] == 4 and capi.flux_plan_host(1000, 20000, 7, 256, segmented=True)["rows"] == 4
    for bad in (dict(n_species=0), dict(B=0), dict(n_cu=0), dict(u_bits=16), dict(k_bits=-1), dict(rates_bits=16), dict(segmented=True, rates_bits=0)):
        kw = dict(n_species=300, n_reactions=1500, B=7, n_cu=256)
        kw.update(bad)
        with pytest.raises(capi.KineticaHipError) as e:
            capi.flux_plan_host(**kw)
        assert e.value.code == capi.KIN_ERR_INVALID_ARG


@pytest.mark.parametrize("n", fc.SIZES)
@pytest.mark.parametrize("layout", ["adjacent", "irregular"])
def test_size_networks_use_the_species_at_the_ends_of_a_staged_state(n, layout):
    net, Ea, A = fc.size_network(n, layout)
    x0, x1 = fc.operands(net)
    want = {0, 1, n - 2, n - 1} | {m + d for m in range(2048, n, 2048) for d in (-1, 0) if n > 2048}
    want = {s for s in want if 0 <= s < n}
    assert set(fc.boundary_species(n)) == want
    assert want <= set(x0.tolist()) and want <= set(x1.tolist())
    assert np.any((x0 == n - 1) & (x1 < 0))                    # the dummy entry right behind the last staged species
    assert net.n_reactions % 2 == 0 and len(Ea) == len(A) == net.n_reactions
    # operands() is the oracle's reading of the network: k u[x0] u[x1]
    from oracle import oracle as orc
    rng = np.random.default_rng(n)
    u, k = rng.choice([0.5, 1.0, 2.0], n), rng.integers(1, 9, net.n_reactions).astype(float)
    assert np.array_equal(orc.OracleNetwork.from_flat(net).rates(k, u), k * u[x0] * np.where(x1 >= 0, u[np.maximum(x1, 0)], 1.0))


def test_size_paths_are_the_boundaries_of_the_dispatch():
    paths = {n: fc.size_path(n) for n in fc.SIZES}
    assert [paths[n] for n in (2, 3, 4, 10240, 10241, 10242, 20478, 20479, 65534, 65535)] == [0, 1, 0, 0, 1, 1, 1, 2, 2, 2]


@pytest.mark.parametrize("name", ["pointers-300x1500", "N2047-irregular", "path0-R4098"])
def test_exact_class_is_exact(name):
    case = next(c for c in CASES if c.name == name)
    d = fc.Data(case, fc.EXACT_MAX_TERMS, "exact")
    x0, x1 = fc.operands(d.net)
    for ksrc in ("k", "k_row", "shared"):
        r = d.rates(ksrc)
        assert np.array_equal(r * 4, np.rint(r * 4)) and r.min() >= 0.25 and r.max() <= 32.0            # multiples of 1/4 below 2^6
        # no product rounds: the oracle's rates are the plain products, in either order of the factors
        k = np.stack([d.k_of(ksrc, b) for b in range(d.B)])
        ub = np.where(x1 >= 0, d.U[:, np.maximum(x1, 0)], 1.0)
        assert np.array_equal(r, k * d.U[:, x0] * ub) and np.array_equal(r, k * (d.U[:, x0] * ub))
        terms = d.w[:, None] * r
        assert np.array_equal(terms * 4, np.rint(terms * 4)) and np.abs(terms).max() <= 64.0
        assert d.B * 64.0 * 4 < 2.0 ** 53                                                             # no partial sum can round
        ref, _ = d.flux(ksrc, d.B)
        assert np.array_equal(ref, terms.sum(axis=0)) and np.array_equal(ref, terms[::-1].sum(axis=0))
        assert np.array_equal(ref, np.cumsum(terms, axis=0)[-1])
        assert np.array_equal(ref, np.array([math.fsum(terms[:, j]) for j in range(terms.shape[1])]))
        sref, _ = d.seg_flux(ksrc)
        for s in range(fc.S_):
            rows = s * fc.L_ + np.arange(fc.SEG_N[s])
            assert np.array_equal(sref[s], terms[rows].sum(axis=0))


def test_log_class_references_hold_their_own_bounds():
    case = next(c for c in CASES if c.name == "pointers-300x1500")
    d = fc.Data(case, 130, "log")
    assert d.U[0, 0] == 1.0 and np.count_nonzero(d.U[0]) == 1 and np.any(d.U[1] == 0.0) and np.sum(d.U[2] == -1e-14) == 5
    assert len(set(d.T.tolist())) == d.B and not np.array_equal(d.K[0], d.K[1])
    x0, x1 = fc.operands(d.net)
    for ksrc in ("k", "T", "k_row", "shared"):
        r = d.rates(ksrc)
        k = np.stack([d.k_of(ksrc, b) for b in range(d.B)])
        plain = k * d.U[:, x0] * np.where(x1 >= 0, d.U[:, np.maximum(x1, 0)], 1.0)
        assert np.all(np.abs(plain - r) <= 4 * fc.EPS * np.abs(r) + 1e-300)
        for B in (1, 35, 130):
            ref, bound = d.flux(ksrc, B)
            assert np.all(np.abs((d.w[:B, None] * r[:B]).sum(axis=0) - ref) <= bound)
        sref, sbound = d.seg_flux(ksrc)
        assert np.all(sref[1] == 0.0) and np.all(sbound[1] == 1e-300)                                  # the empty segment
    U, w, T, K, row = d.seg_inputs()
    for s in range(fc.S_):
        live = slice(s * fc.L_, s * fc.L_ + fc.SEG_N[s])
        dead = slice(s * fc.L_ + fc.SEG_N[s], (s + 1) * fc.L_)
        assert np.array_equal(U[live], d.U[live]) and np.all(np.isnan(U[dead])) and np.all(np.isnan(w[dead])) and np.all(row[dead] == 1 << 40)
