"""CPU tests of the batched sweeps' case lists (tests/sweep_cases.py): the references against the oracle, the CPU replay of the
tiled sweep against the exact reference bit for bit, and the host plan queries (kin_sweep_plan_host, kin_tiled_sweep_plan_host:
no device) against the instantiation every case is named after - so the case list is checked where there is no GPU."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from oracle import oracle as orc
from tests import sweep_cases as sc
from tests import tiled_replay

SMALL_SWEEP = ("reg_bs256_tr4_adj", "gen_colliders_odd_R", "lds_odd_N_blk", "big_10242_colliders", "lds_tiles_65534_adj")


@pytest.mark.parametrize("name", SMALL_SWEEP)
def test_references_agree_with_the_oracle(name):
    """exact inputs: exact_rhs == the oracle's float64 RHS bit for bit (both exact); random inputs: the longdouble reference and the
    oracle agree within the bound the devices are judged with"""
    net, ref = sc.built("sweep", name)
    on = orc.OracleNetwork.from_flat(net)
    Ux, Kx = sc.exact_inputs(3, ref.N, ref.R, 1)
    ex = sc.exact_rhs(ref, Ux, Kx)
    for b in range(3):
        assert np.array_equal(ex[b], on.rhs(Kx[b], Ux[b]))
    assert np.array_equal(sc.exact_rhs(ref, Ux, Kx[0]), np.stack([on.rhs(Kx[0], Ux[b]) for b in range(3)]))     # shared k
    assert np.abs(ex).max() > 0
    Ur, Kr = sc.random_inputs(2, ref.N, ref.R, 1)
    for b in range(2):
        ok, ratio, worst = sc.judge_rhs(ref, Kr[b], Ur[b], on.rhs(Kr[b], Ur[b]))
        assert ok, worst


def test_sample_holds_first_last_and_every_trip():
    for grid in (3, 256, 2048):
        for B in sc.trip_batches(grid):
            s = sc.sample_states(B, grid)
            assert len(s) <= 8 and s[0] == 0 and s[-1] == B - 1
            assert {b // grid for b in s} == set(range((B + grid - 1) // grid))


@pytest.mark.parametrize("name", list(sc.SWEEP_CASES))
def test_sweep_plan_of_every_case(name):
    c = sc.SWEEP_CASES[name]
    net, ref = sc.built("sweep", name)
    p = capi.sweep_plan_host(net, sc.N_CU, 100000, *c.bits)
    assert {q: p[q] for q in c.expect} == c.expect, (name, p)
    if p["kernel"] != "per_state":
        assert p["grid"] == sc.N_CU * p["per_cu"]
        assert capi.sweep_plan_host(net, sc.N_CU, 5, *c.bits)["grid"] == 5
    if c.against:                                   # the aligned run of the same network takes another instantiation
        a = sc.SWEEP_CASES[c.against]
        assert a.bits == (0, 0, 0) and a.inst != c.inst
        assert sc.built("sweep", c.against)[0].n_reactions == net.n_reactions


def test_every_sweep_instantiation_has_a_case():
    got = {c.inst for c in sc.SWEEP_CASES.values()}
    assert got == set(sc.INSTANTIATIONS_SWEEP), set(sc.INSTANTIATIONS_SWEEP) ^ got
    copies = {capi.sweep_plan_host(sc.built("sweep", n)[0], sc.N_CU, 1)["n_copy"] > 0 for n in ("reg_bs256_tr8_adj", "reg_stream_bs256_R6658")}
    assert copies == {False, True}                  # one register-resident case with split accumulators, one without
    assert capi.sweep_plan_host(sc.built("sweep", "gen_colliders_odd_R")[0], sc.N_CU, 1)["n_expl"] == 2
    assert sc.built("sweep", "gen_colliders_odd_R")[0].n_reactions % 2 == 1
    assert capi.sweep_plan_host(sc.built("sweep", "gen_records_1_mod_1024")[0], sc.N_CU, 1)["records"] % 1024 == 1


def test_plan_query_argument_errors():
    net, _ = sc.built("sweep", "reg_bs256_tr0_adj")
    for bad in (dict(n_cu=0), dict(B=0), dict(u_bits=16), dict(k_bits=-1)):
        kw = dict(n_cu=sc.N_CU, B=4, u_bits=0, k_bits=0, du_bits=0); kw.update(bad)
        with pytest.raises(capi.KineticaHipError) as e:
            capi.sweep_plan_host(net, **kw)
        assert e.value.code == capi.KIN_ERR_INVALID_ARG
    with pytest.raises(capi.KineticaHipError):
        capi.tiled_sweep_plan_host(net, 0, 4)


@pytest.mark.parametrize("name", list(sc.TILED_CASES))
def test_tiled_layout_plan_and_replay_of_every_case(name):
    c = sc.TILED_CASES[name]
    net, ref, Ea, A = sc.built("tiled", name)
    with sc.tiled_env(c):
        L = capi.lib_layout_host(net)
        pk = capi.tiled_sweep_plan_host(net, sc.N_CU, 100000)
        pT = capi.tiled_sweep_plan_host(net, sc.N_CU, 100000, True)
    sc.check_tiled_layout(c, L, pk, pT)
    assert pk["grid"] == sc.N_CU * pk["per_cu"] and pT["grid"] == sc.N_CU * pT["per_cu"]
    # the replay of the kernel's arithmetic from the library-order tables equals the exact reference bit for bit
    Ux, Kx = sc.exact_inputs(2, ref.N, ref.R, 2)
    ex = sc.exact_rhs(ref, Ux, Kx)
    for b in range(2):
        du_lib = tiled_replay.replay(L, Ux[b][L["species_of_lib"]], tiled_replay.k_to_lib(L, Kx[b]))
        assert np.array_equal(du_lib, ex[b][L["species_of_lib"]]), name


def test_every_tiled_instantiation_has_a_case_or_a_name():
    got = {i for c in sc.TILED_CASES.values() for i in c.insts()}
    assert got == set(sc.INSTANTIATIONS_TILED), set(sc.INSTANTIATIONS_TILED) ^ got
    cs = sc.TILED_CASES.values()
    assert "windowed_UN10" in sc.NO_LAYOUT and not any(c.expect["UN"] == 10 and len(c.expect["rows"]) > 1 for c in cs)
    # the odd number of batches: four rows per batch in a windowed layout, two rows per batch (UN = 10, both forms)
    assert any(len(c.expect["rows"]) > 1 and c.expect["rows"][0] % 8 == 4 for c in cs)
    assert any(c.expect["UN"] == 10 and c.expect["rows"][0] % 4 == 2 for c in cs)
    assert any(len(set(c.expect["rows"])) > 1 for c in cs)          # segments of different row counts
    assert {c.n % 2 for c in cs if c.n > 8192} == {0, 1}            # two conversion pieces, N odd and even
