"""GPU tests of the reduction passes with MANY states per task. Every launcher cuts a block's states into Y slices and a task
walks its slice state after state; KIN_SLICES_MAX caps Y (a test knob, read per call), so with B = 7 states and a cap of 1,
2, 3 every task walks 7, 4 / 3 and 3 / 2 / 2 states - whatever the device's size. That runs what exists only for the second
and later state of a task: the barrier that protects the workgroup's partial sums, the running maxima and extrema in
registers, the row buffer the PFA read-out must leave zero, its staged out-edges, its register columns and its spill.

Every result is compared bit for bit with the same call without the cap, and on the exact inputs of reduction_edge_cases.py
with the exact reference as well."""
import numpy as np
import pytest

import drg_cases as dc
import reduction_edge_cases as rx
from kinetica_jl_amd import capi
from test_gpu_drgep import check_paths
from test_gpu_timescale import OUTPUTS, all_outputs, assert_exact
from tests import jac_cases as jc
from tests import timescale_cases as tc
from tests.linalg_cases import hub_net

pytestmark = pytest.mark.gpu

CAPS = ("1", "2", "3")
WG_COSTS = ("0", "1000000000")        # KIN_PFA_WG_COST: every row by a workgroup, every row by a wavefront
_handles = {}


def handle(key, net):
    if key not in _handles:
        _handles[key] = capi.HipNetwork.from_flat(net)
    return _handles[key]


def flat(x):
    """the arrays of a call's result, in a fixed order"""
    if isinstance(x, dict):
        return [x[q] for q in sorted(x)]
    return list(x) if isinstance(x, tuple) else [x]


def under_caps(monkeypatch, call):
    """call() without the cap; then with every cap, each bit-identical to it. Returns the uncapped result."""
    monkeypatch.delenv("KIN_SLICES_MAX", raising=False)
    whole = call()
    for cap in CAPS:
        monkeypatch.setenv("KIN_SLICES_MAX", cap)
        got = call()
        for a, b in zip(flat(got), flat(whole)):
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), cap
    monkeypatch.delenv("KIN_SLICES_MAX")
    return whole


def test_trip_lengths_are_hubs_of_the_cases():
    for name in ("collider", "paired"):
        assert set(rx.TRIP_LENGTHS) <= {hub["n"] for hub in rx.gather_case(name).hubs} and rx.gather_case(name).B == 7
    assert {9, 257} <= set(rx.gather_case("paired_small").lengths) and rx.gather_case("paired_1025").B == 3


# ------------------------------------------------------------------------------------------- exact inputs, exact reference
@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", ["collider", "paired"])
def test_gather_passes_walk_many_states(name, pairing, monkeypatch):
    c = rx.gather_case(name)
    h = handle(name, c.net)
    targets = [hub["A"] for hub in c.hubs]
    coef = under_caps(monkeypatch, lambda: h.drg_batched(c.U, k=c.K, pairing=pairing))
    assert np.array_equal(coef, c.ref("drg", pairing)[0])
    imp, r, R, rounds = under_caps(monkeypatch, lambda: h.drgep_batched(c.U, targets, k=c.K, pairing=pairing, stages=True))
    assert np.array_equal(r, c.ref("drgep", pairing))
    check_paths(c.drgep(pairing), r, targets, imp, R, rounds)
    imp, I = under_caps(monkeypatch, lambda: h.reaction_importance_batched(c.U, k=c.K, pairing=pairing, per_state=True))
    assert np.array_equal(I, c.ref("ri", pairing)[1]) and np.array_equal(imp, c.ref("ri", pairing)[0])
    assert np.array_equal(under_caps(monkeypatch, lambda: h.reaction_importance_batched(c.U, k=c.K, pairing=pairing)), imp)


@pytest.mark.parametrize("wg_cost", WG_COSTS)
@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", rx.PFA_GATHER)
def test_pfa_walks_many_states(name, pairing, wg_cost, monkeypatch):
    c = rx.gather_case(name)
    h = handle(name, c.net)
    monkeypatch.setenv("KIN_PFA_WG_COST", wg_cost)
    coef, rp, rcn, r = under_caps(monkeypatch, lambda: h.pfa_batched(c.U, k=c.K, pairing=pairing, stages=True))
    rp_ref, rc_ref = c.ref("pfa", pairing)
    assert np.array_equal(rp, rp_ref) and np.array_equal(rcn, rc_ref) and np.array_equal(coef, r.max(axis=0))
    assert np.array_equal(under_caps(monkeypatch, lambda: h.pfa_batched(c.U, k=c.K, pairing=pairing)), coef)    # the KEEP form


@pytest.mark.parametrize("stages", [True, False])
@pytest.mark.parametrize("wg_cost", WG_COSTS)
@pytest.mark.parametrize("name", sorted(rx.PFA_PARTS))
def test_pfa_second_stage_walks_many_states(name, wg_cost, stages, monkeypatch):
    """the four instantiations on the double stars and brooms: the row buffer, the staged out-edges of a one-chunk row, the
    register columns and the spill are carried from state to state"""
    c = rx.pfa_case(name)
    h = handle(("pfa", name), c.net)
    monkeypatch.setenv("KIN_PFA_WG_COST", wg_cost)
    ref = c.r()
    if stages:
        coef, r = under_caps(monkeypatch, lambda: h.pfa_paths(c.rp, c.rc, stages=True))
        assert np.array_equal(r, ref)
    else:
        coef = under_caps(monkeypatch, lambda: h.pfa_paths(c.rp, c.rc))
    assert np.array_equal(coef, ref.max(axis=0))


@pytest.mark.parametrize("kind", ["hub", "fan_in"])
@pytest.mark.parametrize("L", rx.TRIP_LENGTHS)
def test_timescale_walks_many_states(L, kind, monkeypatch):
    """hub_net(L): Jacobian entries of L contributions (the entry gather); fan_in_net(L - 1): a row of L stored entries (the row
    pass). Seven exact states, every output bit for bit the reference under every cap."""
    net = hub_net(L) if kind == "hub" else tc.fan_in_net(L - 1)
    ref = jc.Reference(net)
    monkeypatch.delenv("KIN_SLICES_MAX", raising=False)
    whole, want = assert_exact(net, ref, seed=L, B=7)
    assert len({want["diag"][b].tobytes() + want["vals"][b].tobytes() for b in range(7)}) == 7      # the states differ
    for cap in CAPS:
        monkeypatch.setenv("KIN_SLICES_MAX", cap)
        got, _ = assert_exact(net, ref, seed=L, B=7)
        for q in ("vals",) + OUTPUTS:
            assert np.array_equal(got[q], whole[q]), (cap, q)


# ------------------------------------------------------------------------------ the synthetic network, per-state constants
def test_synthetic_300x1500_is_bit_identical_under_every_cap(monkeypatch):
    """the uncapped results are what test_gpu_drg / drgep / pfa / reaction_importance / timescale hold to their derived bounds"""
    case = dc.synth_case("300x1500")
    h = handle("300x1500", case.net)
    U, K = case.U[:7], case.K[:7]
    for pairing in (1, 0):
        under_caps(monkeypatch, lambda: h.drg_batched(U, k=K, pairing=pairing))
        under_caps(monkeypatch, lambda: h.drgep_batched(U, [0, 1, 2], k=K, pairing=pairing, stages=True))
        under_caps(monkeypatch, lambda: h.reaction_importance_batched(U, k=K, pairing=pairing, per_state=True))
        for wg_cost in WG_COSTS:
            monkeypatch.setenv("KIN_PFA_WG_COST", wg_cost)
            staged = under_caps(monkeypatch, lambda: h.pfa_batched(U, k=K, pairing=pairing, stages=True))
            assert np.array_equal(under_caps(monkeypatch, lambda: h.pfa_batched(U, k=K, pairing=pairing)), staged[0])
        monkeypatch.delenv("KIN_PFA_WG_COST")
    under_caps(monkeypatch, lambda: all_outputs(h, U, k=K))
    # blocks and slices together: blocks of 4 and 3 states, two slices each
    whole = h.drg_batched(U, k=K)
    monkeypatch.setenv("KIN_DRG_BLOCK_STATES", "4")
    monkeypatch.setenv("KIN_SLICES_MAX", "2")
    assert np.array_equal(h.drg_batched(U, k=K), whole)


def test_values_below_one_are_ignored(monkeypatch):
    case = dc.synth_case("300x1500")
    h = handle("300x1500", case.net)
    whole = h.drg_batched(case.U[:7], k=case.K[:7])
    for v in ("0", "-3", "x"):
        monkeypatch.setenv("KIN_SLICES_MAX", v)
        assert np.array_equal(h.drg_batched(case.U[:7], k=case.K[:7]), whole)
