"""GPU tests of what the host entries of the six analysis passes (flux, DRG, reaction importance, DRGEP, PFA, timescale) do
with bad input: the status code AND the exact message, which of two faults is reported, that a refused call leaves the handle
usable, and the empty batch. Every entry is called through ctypes directly, so that nulls and wrong counts reach the library.

The expected messages are literals, copied from the library's source as it stood before the passes' host side was put on one
staging layer: they pin the behaviour, they are not read back from the code under test. Every bad call is refused by the host
checks before any launch.

The network: 4 species, 3 reactions - A + B -> C, its reverse (one reversible pair, so pairing matters) and C -> D. B = 3 states;
a stored solve of 5 rows; a stored ensemble of K = 2 members of which the second fails at once (n_saved = [5, 1]: rows 1 .. 4
of member 1 are not live); on a third handle an ensemble solved with per-member Arrhenius parameters."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists
from timescale_cases import identity

pytestmark = pytest.mark.gpu

INV, UNS, STATE = capi.KIN_ERR_INVALID_ARG, capi.KIN_ERR_UNSUPPORTED, capi.KIN_ERR_STATE
N, R, B, ROWS, K = 4, 3, 3, 5, 2
NS = [5, 1]
OUT_LEN, FILL = 256, -7.25

M_BOTH = "give rate constants or temperatures, not both"
M_ROW_NO_K = "k_row given without rate constants to index"
M_NO_ARR = "temperatures given but Arrhenius parameters were never set"
M_WRONG_ROWS = {"batched": "k without k_row needs one row per state (n_k_rows == B)",
                "segmented": "k without k_row needs one row per state (n_k_rows == S L)",
                "solution": "k without k_row needs one row per saved state (n_k_rows == n_saved)",
                "ensemble": "k without k_row needs one row per saved row (n_k_rows == K n_rows)"}
M_ROW_RANGE = "k_row: row index out of range"
M_NULL_OUT = "null output buffer"
M_NO_SOL = "no solution stored"
M_NO_ENS = "no ensemble stored (kin_solve_ensemble* first)"
M_NO_TABLE = "no rate table resident (kin_rate_table / kin_solve with a table first)"
M_MEMBER = ("the stored ensemble was solved with per-member Arrhenius parameters: T_rows would use the handle's; give the rate "
            "constants explicitly (k with k_row, one kin_arrhenius_eval row per member and temperature)")
M_TARGET_RANGE, M_TARGET_NONE = "target species out of range", "DRGEP needs at least one target species"
M_SPECIES_RANGE, M_SPECIES_NONE = "species out of range", "a species list needs at least one entry"
M_R = "r: coefficients must be finite and in [0, 1]"
M_RP = "rp, rc: coefficients must be finite and not negative"

# entry -> form; the argument lists are in _args
ENTRIES = {
    "kin_flux_batched": "batched", "kin_solution_flux": "solution", "kin_flux_segmented": "segmented", "kin_ensemble_flux": "ensemble",
    "kin_drg_batched": "batched", "kin_solution_drg": "solution", "kin_ensemble_drg": "ensemble",
    "kin_reaction_importance_batched": "batched", "kin_solution_reaction_importance": "solution",
    "kin_ensemble_reaction_importance": "ensemble",
    "kin_drgep_batched": "batched", "kin_solution_drgep": "solution", "kin_ensemble_drgep": "ensemble", "kin_drgep_paths": "paths",
    "kin_pfa_batched": "batched", "kin_solution_pfa": "solution", "kin_ensemble_pfa": "ensemble", "kin_pfa_paths": "paths",
    "kin_jac_batched": "batched", "kin_timescale_batched": "batched", "kin_solution_timescale": "solution",
    "kin_ensemble_timescale": "ensemble",
}
N_STATES = {"batched": B, "segmented": B, "solution": ROWS, "ensemble": K * ROWS, "paths": B}
LAST_LIVE = {"batched": B - 1, "segmented": B - 1, "solution": ROWS - 1, "ensemble": ROWS}      # (member 1 has one row)


def null_out_message(name):
    if name in ("kin_flux_batched", "kin_solution_flux"):
        return "neither flux nor rates requested"
    if name in ("kin_jac_batched", "kin_timescale_batched"):
        return "no output requested"
    return M_NULL_OUT


def takes_list(name):
    return "drgep" in name or "reaction_importance" in name


def list_messages(name):
    return (M_TARGET_RANGE, M_TARGET_NONE) if "drgep" in name else (M_SPECIES_RANGE, M_SPECIES_NONE)


def kp(**kw):
    d = dict(tspan0=0.0, tspan1=1e-3, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1, ban_negatives=0,
             solve_chunkstep=1e-3, maxiters=100000, save_interval=2.5e-4, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


class World:
    """The handles the cases run on. a: Arrhenius parameters and rates, a stored solve, a stored ensemble. n: the same with
    rates only (no Arrhenius parameters). p: an ensemble solved with per-member parameters. e: nothing stored."""

    def __init__(self):
        net = from_lists(N, [[(0, 1), (1, 1)], [(2, 1)], [(2, 1)]], [[(2, 1)], [(0, 1), (1, 1)], [(3, 1)]])
        Ea, A = np.array([2.0e4, 5.0e4, 3.0e4]), np.array([1e6, 1e7, 1e5])
        k0 = np.full(R, 1e12)
        u0 = np.array([1.0, 0.5, 0.0, 0.0])
        self.handles = {}
        for key in "anpe":
            h = capi.HipNetwork.from_flat(net)
            if key != "n":
                h.set_arrhenius(Ea, A, k_max=1e12)
            h.set_rates(k0)
            if key in "an":
                t, us, rc, _, _ = h.solve(kp(), u0)
                assert rc == 0 and len(t) == ROWS
                # the second member blows up in its first step: one saved row
                _, _, ns, rcs, _ = h.solve_ensemble(kp(maxiters=3000), np.tile(u0, (K, 1)), k=np.stack([k0, k0 * 1e40]))
                assert list(ns) == NS and rcs[0] == 0 and rcs[1] != 0, (ns, rcs)
                self.us = us
            if key == "p":
                nodes = [(np.array([0.0, 1e-3]), np.array([900.0, 1100.0])), (np.array([0.0, 5e-4, 1e-3]), np.array([1000.0, 1200.0, 1000.0]))]
                _, _, ns, rcs, _ = h.solve_ensemble_continuous(kp(), np.tile(u0, (K, 1)), nodes, Ea=np.stack([Ea, Ea * 1.1]),
                                                               A=np.stack([A, A * 2]))
                assert list(ns) == [ROWS, ROWS] and (rcs == 0).all()
            self.handles[key] = h
        a = self.handles["a"]
        self.E, self.E2 = len(a.drg_pattern(True)[1]), len(a.pfa_pattern(True)[1])
        assert self.E > 0 and self.E2 >= self.E
        rng = np.random.default_rng(5)
        self.U = 10.0 ** rng.uniform(-6, 0, (B, N))
        self.r = rng.uniform(0.0, 1.0, (B, self.E))
        self.rp, self.rc = rng.uniform(0.0, 2.0, (B, self.E)), rng.uniform(0.0, 2.0, (B, self.E))

    def close(self):
        for h in self.handles.values():
            h.close()

    def n_result(self, name):
        """doubles of the accumulating (or, flux and Jacobian, the only) result of entry `name`; an upper bound for the
        segmented flux entries and the Jacobian values"""
        for q, v in (("drgep", N), ("drg", self.E), ("reaction_importance", R), ("pfa", self.E2), ("timescale", 3 * N), ("jac", B * N * N),
                     ("flux_batched", R), ("solution_flux", R), ("flux", K * R)):
            if q in name:
                return v
        raise KeyError(name)


@pytest.fixture(scope="module")
def worlds():
    """Two identical sets of handles: every refused call of this module goes to `dirty`, none to `clean`."""
    w = SimpleNamespace(dirty=World(), clean=World())
    assert np.array_equal(w.dirty.us, w.clean.us)
    yield w
    w.dirty.close()
    w.clean.close()


def _ptr(x):
    if x is None or isinstance(x, (int, np.integer)):
        return x
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float64, np.int64), x.dtype
    return x.ctypes.data_as(ctypes.POINTER(ctypes.c_double if x.dtype == np.float64 else ctypes.c_int64))


def _args(name, a):
    src, sel = (a.k, a.nk, a.k_row, a.T), (a.sel, a.nsel, a.base)
    return {
        "kin_flux_batched": (a.B, a.u, *src, None, a.out, None),
        "kin_solution_flux": (None, *src, a.out, None),
        "kin_flux_segmented": (1, a.B, None, a.u, *src, None, a.out),
        "kin_ensemble_flux": (None, *src, a.out),
        "kin_drg_batched": (1, a.B, a.u, *src, a.acc, a.out),
        "kin_solution_drg": (1, *src, a.acc, a.out),
        "kin_ensemble_drg": (1, *src, a.acc, a.out),
        "kin_reaction_importance_batched": (1, a.B, a.u, *src, *sel, a.acc, a.out, None),
        "kin_solution_reaction_importance": (1, *src, *sel, a.acc, a.out),
        "kin_ensemble_reaction_importance": (1, *src, *sel, a.acc, a.out),
        "kin_drgep_batched": (1, a.B, a.u, *src, *sel, a.acc, a.out, None, None, None),
        "kin_solution_drgep": (1, *src, *sel, a.acc, a.out),
        "kin_ensemble_drgep": (1, *src, *sel, a.acc, a.out),
        "kin_drgep_paths": (1, a.B, a.r, *sel, a.acc, a.out, None, None),
        "kin_pfa_batched": (1, a.B, a.u, *src, a.acc, a.out, None, None, None),
        "kin_solution_pfa": (1, *src, a.acc, a.out),
        "kin_ensemble_pfa": (1, *src, a.acc, a.out),
        "kin_pfa_paths": (1, a.B, a.rp, a.rc, a.acc, a.out, None),
        "kin_jac_batched": (a.B, a.u, *src, a.out),
        "kin_timescale_batched": (a.B, a.u, *src, a.acc, a.out, None, None, None),
        "kin_solution_timescale": (*src, a.row_begin, a.acc, a.out, None),
        "kin_ensemble_timescale": (*src, a.row_begin, a.acc, a.out, None),
    }[name]


def call(world, name, handle="a", **over):
    """One call of entry `name` on world.handles[handle]: a good call (the handle's own rate constants, every species or target
    0) with the fields in `over` replaced. Returns (status, message, the output buffer)."""
    out = np.full(OUT_LEN, FILL)
    a = SimpleNamespace(B=B, u=world.U, k=None, nk=0, k_row=None, T=None, acc=0, out=out, row_begin=0, r=world.r, rp=world.rp, rc=world.rc,
                        sel=np.array([0], np.int64) if "drgep" in name else None, nsel=1 if "drgep" in name else 0, base=0)
    for q, v in over.items():
        assert hasattr(a, q), q
        setattr(a, q, v)
    h = world.handles[handle]
    st = getattr(capi.lib(), name)(h.handle, *[_ptr(x) for x in _args(name, a)])
    return st, capi.lib().kin_last_error(h.handle).decode() if st != capi.KIN_OK else "", out


def with_k(form, rows=None):
    """k[B][R] with one row per state (rows None), or the two rows of K2 indexed by `rows`."""
    n = N_STATES[form]
    if rows is None:
        return dict(k=np.tile([2.0, 3.0, 0.5], (n, 1)), nk=n)
    return dict(k=np.array([[2.0, 3.0, 0.5], [0.25, 4.0, 1.5]]), nk=2, k_row=np.asarray(rows, np.int64))


def bad_rows(form, at):
    rows = np.arange(N_STATES[form], dtype=np.int64) % 2
    rows[at] = 2 if at else -1      # one past the last row of k; below the first
    return rows


def good_rows(form):
    return np.arange(N_STATES[form], dtype=np.int64) % 2


def cases(name):
    """(id, handle, overrides, status, message) for every bad input entry `name` can be given, the precedence cases last."""
    form = ENTRIES[name]
    n, null_msg = N_STATES[form], null_out_message(name)
    temps = np.linspace(900.0, 1100.0, n)
    out = []
    if form != "paths":
        out += [("k_with_T", "a", dict(with_k(form), T=temps), INV, M_BOTH),
                ("T_without_arrhenius", "n", dict(T=temps), STATE, M_NO_ARR),
                ("k_wrong_row_count", "a", dict(with_k(form), nk=n - 1), INV, M_WRONG_ROWS[form]),
                ("k_row_bad_at_first_state", "a", with_k(form, bad_rows(form, 0)), INV, M_ROW_RANGE),
                ("k_row_bad_at_last_state", "a", with_k(form, bad_rows(form, LAST_LIVE[form])), INV, M_ROW_RANGE),
                ("null_output", "a", dict(out=None), INV, null_msg),
                ("both_sources_and_bad_k_row", "a", dict(with_k(form, bad_rows(form, 0)), T=temps), INV, M_BOTH),
                ("null_output_and_bad_k_row", "a", dict(with_k(form, bad_rows(form, 0)), out=None), INV, null_msg)]
        if form == "solution":
            out += [("no_resident_table", "a", dict(k_row=good_rows(form)), STATE, M_NO_TABLE),
                    ("no_solution_stored", "e", {}, STATE, M_NO_SOL),
                    ("null_output_and_no_solution", "e", dict(out=None), INV, null_msg),
                    ("both_sources_and_no_solution", "e", dict(with_k(form), T=temps), INV, M_BOTH)]
        else:
            out += [("k_row_without_k", "a", dict(k_row=good_rows(form)), INV, M_ROW_NO_K)]
        if form == "ensemble":
            flux = name == "kin_ensemble_flux"      # the one ensemble entry that forms each member's rate constants from its own parameters
            dead = good_rows(form)
            dead[ROWS + 1:] = 99                    # keys of rows member 1 never saved: not looked at
            out += [("no_ensemble_stored", "e", {}, STATE, M_NO_ENS),
                    ("null_output_and_no_ensemble", "e", dict(out=None), INV if flux else STATE, M_NULL_OUT if flux else M_NO_ENS),
                    ("k_row_bad_past_the_saved_rows", "a", with_k(form, dead), capi.KIN_OK, ""),
                    ("T_rows_on_member_parameters", "p", dict(T=temps), capi.KIN_OK if flux else UNS, "" if flux else M_MEMBER),
                    ("T_rows_on_member_parameters_and_k", "p", dict(with_k(form), T=temps), INV, M_BOTH),
                    ("T_rows_on_member_parameters_and_null_output", "p", dict(T=temps, out=None), INV, M_NULL_OUT)]
        if name in ("kin_solution_timescale", "kin_ensemble_timescale"):
            out += [("negative_row_begin_and_null_output", "a", dict(row_begin=-1, out=None), INV, "row_begin < 0")]
    if takes_list(name):
        m_range, m_none = list_messages(name)
        out += [("list_entry_above_range", "a", dict(sel=np.array([0, N], np.int64), nsel=2), INV, m_range),
                ("list_entry_below_range", "a", dict(sel=np.array([0, 1], np.int64), nsel=2, base=1), INV, m_range),
                ("empty_list", "a", dict(sel=np.array([0], np.int64), nsel=0), INV, m_none)]
        if "drgep" in name:
            out += [("null_list", "a", dict(sel=None, nsel=1), INV, m_none)]
        if form != "paths":
            out += [("bad_list_and_bad_k_row", "a", dict(with_k(form, bad_rows(form, 0)), sel=np.array([N], np.int64), nsel=1), INV, M_ROW_RANGE)]
    if name == "kin_drgep_paths":
        hi, neg = np.full((B, 1), 0.5).repeat(64, axis=1), np.full((B, 64), 0.5)
        hi[B - 1, 0], neg[0, 0] = 1.5, -0.25
        out += [("r_above_one", "a", dict(r=hi), INV, M_R), ("r_below_zero", "a", dict(r=neg), INV, M_R),
                ("null_output", "a", dict(out=None), INV, M_NULL_OUT), ("negative_B", "a", dict(B=-1), INV, "B out of range"),
                ("null_output_and_r_above_one", "a", dict(out=None, r=hi), INV, M_NULL_OUT),
                ("r_above_one_and_bad_target", "a", dict(r=hi, sel=np.array([N], np.int64)), INV, M_R)]
    if name == "kin_pfa_paths":
        neg = np.full((B, 64), 0.5)
        neg[B - 1, 0] = -0.25
        out += [("negative_rp", "a", dict(rp=neg), INV, M_RP), ("negative_rc", "a", dict(rc=neg), INV, M_RP),
                ("null_output", "a", dict(out=None), INV, M_NULL_OUT), ("negative_B", "a", dict(B=-1), INV, "B out of range"),
                ("null_output_and_negative_rp", "a", dict(out=None, rp=neg), INV, M_NULL_OUT)]
    return out


ALL_CASES = [pytest.param(name, c, id=f"{name}-{c[0]}") for name in ENTRIES for c in cases(name)]


@pytest.mark.parametrize("name, case", ALL_CASES)
def test_bad_input_is_refused_with_its_code_and_message(worlds, name, case):
    _, handle, over, status, message = case
    if "r" in over or "rp" in over or "rc" in over:      # (built for any number of edges: the first E columns are the coefficients)
        over = {q: (np.ascontiguousarray(v[:, :worlds.dirty.E]) if q in ("r", "rp", "rc") else v) for q, v in over.items()}
    st, msg, out = call(worlds.dirty, name, handle, **over)
    assert (st, msg) == (status, message)
    if st != capi.KIN_OK:
        assert np.all(out == FILL)      # a refused call writes nothing


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_good_call_after_a_refused_one_matches_a_fresh_handle(worlds, name):
    """The refused call fails at the LAST state's key (or coefficient), behind every check that precedes the uploads; the good
    call then stages keys of its own through the same buffers."""
    form = ENTRIES[name]
    E = worlds.dirty.E
    if name == "kin_drgep_paths":
        bad = dict(r=np.full((B, E), 1.5))
        good = {}
    elif name == "kin_pfa_paths":
        bad = dict(rp=np.full((B, E), -1.0))
        good = {}
    else:
        bad, good = with_k(form, bad_rows(form, LAST_LIVE[form])), with_k(form, good_rows(form))
    st, _, _ = call(worlds.dirty, name, **bad)
    assert st == INV
    got, want = call(worlds.dirty, name, **good), call(worlds.clean, name, **good)
    assert got[0] == capi.KIN_OK and want[0] == capi.KIN_OK
    assert np.array_equal(got[2], want[2], equal_nan=True)
    assert np.any(got[2] != FILL)
    assert np.all(got[2][worlds.dirty.n_result(name):] == FILL)


@pytest.mark.parametrize("name", ["kin_flux_batched", "kin_drg_batched", "kin_reaction_importance_batched", "kin_drgep_batched",
                                  "kin_drgep_paths", "kin_pfa_batched", "kin_pfa_paths", "kin_timescale_batched"])
def test_the_empty_batch(worlds, name):
    """No state: zeros - the identity summary for the timescale pass - or, accumulating, the caller's values untouched."""
    w = worlds.clean
    n = w.n_result(name)
    st, _, out = call(w, name, B=0, u=None, r=None, rp=None, rc=None)
    assert st == capi.KIN_OK
    assert np.array_equal(out[:n], identity(N).ravel() if "timescale" in name else np.zeros(n)) and np.all(out[n:] == FILL)
    if name != "kin_flux_batched":      # (the flux pass has no accumulating form)
        st, _, out = call(w, name, B=0, u=None, r=None, rp=None, rc=None, acc=1)
        assert st == capi.KIN_OK and np.all(out == FILL)
