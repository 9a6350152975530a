"""GPU tests of the reduction passes' gather kernels at every row edge (cases and references: reduction_edge_cases.py, whose
claims test_reduction_edge_cases.py proves on the CPU).

1. Every instantiation of drg_gather_kernel on every row class - short, medium, long, long in several passes; records with a
   reverse (b >= 0) and without - on exact inputs, BIT FOR BIT against the references of drg_cases, drgep_cases, pfa_cases and
   reaction_importance_cases (math.fsum, one float64 division): <false> and <true> through drg_batched, <false, true> and
   <true, true> through drgep_batched, <true, true, true> through pfa_batched; reaction_importance_batched reads <false>'s
   denominators. One case per pass runs in the temperature form as well, which is not exact: against the bounds derived in
   those modules, under their condition (at most 1 % of the compared bounds above 1e-9; the host test checks it on the CPU).
2. pfa_second_kernel in its four instantiations <256, 0>, <64, 0>, <256, PFA_KEEP>, <64, PFA_KEEP> on double stars and brooms
   at every chunk, look-ahead, long-M and register-column edge, bit for bit on coefficients in {0, 1/4, 1/2, 1}.
3. drgep_path_kernel in the LDS and in the global form at every in-degree class edge, bit for bit against the NumPy search."""
import numpy as np
import pytest

import reduction_edge_cases as rx
from kinetica_jl_amd import capi
from test_gpu_drgep import check_paths

pytestmark = pytest.mark.gpu

T_CASE = "paired_small"
_handles = {}


def handle(key, net):
    if key not in _handles:
        _handles[key] = capi.HipNetwork.from_flat(net)
    return _handles[key]


def gather(name):
    c = rx.gather_case(name)
    return c, handle(name, c.net)


# ------------------------------------------------------------------- 1. the five gather instantiations on every row class
@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", ["collider", "paired"])
def test_drg_coefficients_bit_for_bit(name, pairing):
    c, h = gather(name)
    coef, r = c.ref("drg", pairing)
    assert np.array_equal(h.drg_batched(c.U, k=c.K, pairing=pairing), coef)
    for b in range(c.B):                                   # state by state: a maximum hides nothing
        assert np.array_equal(h.drg_batched(c.U[b:b + 1], k=c.K[b:b + 1], pairing=pairing), r[b]), b
    assert np.all(r[rx.ZERO_STATE] == 0.0)                 # (compared above: exactly 0.0, never NaN)
    g = c.drg(pairing)
    for hub in c.hubs:
        assert 0.0 < coef[rx.edge_of(g, hub["A"], hub["B"])] < 1.0


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", ["collider", "paired"])
def test_drgep_coefficients_bit_for_bit(name, pairing):
    c, h = gather(name)
    targets = [hub["A"] for hub in c.hubs]
    imp, r, R, rounds = h.drgep_batched(c.U, targets, k=c.K, pairing=pairing, stages=True)
    assert np.array_equal(r, c.ref("drgep", pairing))
    assert np.all(r[rx.ZERO_STATE] == 0.0)
    check_paths(c.drgep(pairing), r, targets, imp, R, rounds)


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", rx.PFA_GATHER)
def test_pfa_split_coefficients_bit_for_bit(name, pairing):
    c, h = gather(name)
    coef, rp, rcn, r = h.pfa_batched(c.U, k=c.K, pairing=pairing, stages=True)
    rp_ref, rc_ref = c.ref("pfa", pairing)
    assert np.array_equal(rp, rp_ref) and np.array_equal(rcn, rc_ref)
    if c.B > rx.ZERO_STATE:
        assert np.all(rp[rx.ZERO_STATE] == 0.0) and np.all(rcn[rx.ZERO_STATE] == 0.0) and np.all(r[rx.ZERO_STATE] == 0.0)
    assert np.array_equal(coef, r.max(axis=0))             # the maximum over the states is exact
    if c.second:                                           # the second stage on these ratios: within its own derived bound
        g = c.pfa(pairing)
        ref = g.second_all(rp, rcn)
        assert np.all(np.abs(r - ref) <= g.second_bound(ref)) and np.all(r[ref == 0.0] == 0.0)


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", ["collider", "paired"])
def test_reaction_importance_bit_for_bit(name, pairing):
    c, h = gather(name)
    imp, I = h.reaction_importance_batched(c.U, k=c.K, pairing=pairing, per_state=True)
    imp_ref, I_ref = c.ref("ri", pairing)
    assert np.array_equal(I, I_ref) and np.array_equal(imp, imp_ref)
    assert np.all(I[rx.ZERO_STATE] == 0.0)
    # a species list (the mask path of the kernel): the hubs' own species judge, the shared partners X_i, Y_i do not
    sel = [hub[s] for hub in c.hubs for s in ("A", "B", "C", "D")]
    imp_sel, I_sel = h.reaction_importance_batched(c.U, species=sel, k=c.K, pairing=pairing, per_state=True)
    want = np.stack([c.ri(pairing).state(c.rates[b], selected=sel)[0] for b in range(c.B)])
    assert np.array_equal(I_sel, want) and np.array_equal(imp_sel, want.max(axis=0))


def within(got, ref, bound, bounds):
    frac = float(np.mean(bounds > 1e-9))
    err = np.abs(got - ref)
    print(f"max err {err.max():.3e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, {100 * frac:.3f} % of the bounds above 1e-9")
    assert frac <= 0.01
    assert np.all(np.isfinite(got)) and np.all(err <= bound)


@pytest.mark.parametrize("pairing", [1, 0])
def test_temperature_form_within_the_derived_bounds(pairing):
    c, h = gather(T_CASE)
    h.set_arrhenius(c.Ea, c.A)
    coef, bound, bounds = c.t_ref("drg", pairing)
    within(h.drg_batched(c.U, T=c.T, pairing=pairing), coef, bound, bounds)
    r_ref, r_bounds = c.t_ref("drgep", pairing)
    within(h.drgep_batched(c.U, [0], T=c.T, pairing=pairing, stages=True)[1], r_ref, r_bounds, r_bounds)
    rp_ref, rc_ref, bp, bc = c.t_ref("pfa", pairing)
    _, rp, rcn, _ = h.pfa_batched(c.U, T=c.T, pairing=pairing, stages=True)
    within(rp, rp_ref, bp, bp)
    within(rcn, rc_ref, bc, bc)
    imp_ref, ibound, ibounds = c.t_ref("ri", pairing)
    within(h.reaction_importance_batched(c.U, T=c.T, pairing=pairing), imp_ref, ibound, ibounds)


# ------------------------------------------------------------------------- 2. the second stage of PFA, four instantiations
WG_COSTS = {"workgroup": "0", "wavefront": "1000000000"}      # KIN_PFA_WG_COST: every row with a cost above it by a workgroup


@pytest.mark.parametrize("stages", [True, False])
@pytest.mark.parametrize("form", sorted(WG_COSTS))
@pytest.mark.parametrize("name", sorted(rx.PFA_PARTS))
def test_pfa_second_stage_bit_for_bit(name, form, stages, monkeypatch):
    """stages=True is KEEP = 0 (every column through part, r written), stages=False KEEP = PFA_KEEP (register columns, then the spill)"""
    c = rx.pfa_case(name)
    h = handle(("pfa", name), c.net)
    monkeypatch.setenv("KIN_PFA_WG_COST", WG_COSTS[form])
    if form == "workgroup":
        assert np.all(c.row_cost()[[A for _, _, _, A, _ in c.where]] > 0)
    ref = c.r()
    if stages:
        coef, r = h.pfa_paths(c.rp, c.rc, stages=True)
        assert np.array_equal(r, ref)
    else:
        coef = h.pfa_paths(c.rp, c.rc)
    assert np.array_equal(coef, ref.max(axis=0))
    # one state at a time: what a row leaves behind for the next state does not matter here - and must not matter above
    for b in (0, rx.ZERO_STATE, len(ref) - 1):
        assert np.array_equal(h.pfa_paths(c.rp[b:b + 1], c.rc[b:b + 1]), ref[b]), b


def test_pfa_register_columns_and_spill_are_met():
    """the rows the KEEP forms are tested on: 1537 columns spill past a workgroup's 6 x 256 registers, 385 past a wavefront's"""
    c = rx.pfa_case("brooms")
    row2 = np.diff(c.g.rowptr2)
    assert {capi.PFA_KEEP * 256, capi.PFA_KEEP * 256 + 1, capi.PFA_KEEP * 64, capi.PFA_KEEP * 64 + 1} <= set(row2[[A for _, _, _, A, _ in c.where]])


# ----------------------------------------------------------------------------------------------------- 3. the path stage
@pytest.mark.parametrize("form", ["lds", "global"])
def test_path_stage_at_every_in_degree_edge(form, monkeypatch):
    c = rx.path_case()
    h = handle("path", c.net)
    if form == "global":
        monkeypatch.setenv("KIN_DRGEP_LDS_SPECIES", "100")
    assert c.g.n > 100
    rowptr, colidx = h.drg_pattern(1)
    assert np.array_equal(colidx, c.g.g.colidx) and np.array_equal(rowptr, c.g.g.rowptr)
    targets = [2, c.g.n - 1, c.where[-1][3]]
    imp, R, rounds = h.drgep_paths(c.r, targets, pairing=1, stages=True)
    check_paths(c.g, c.r, targets, imp, R, rounds)
    assert np.sum(imp > 0) > len(targets)
    # the winner on the last incoming edge of every centre, whatever its class
    imp2, R2, rounds2 = h.drgep_paths(c.planted, c.leaves, pairing=1, stages=True)
    assert np.all(imp2[c.centres] == 0.5)
    check_paths(c.g, c.planted, c.leaves, imp2, R2, rounds2)
