"""What the Python binding hands to the library (no device, no built library for all but the last test): every public method
of HipNetwork's analysis sections - reaction fluxes to Sobol indices - and the two per-member ensemble solves, called on a
recording stand-in for the library. Of each call the entry name, the number of arguments and every argument are compared
with a list written from the declaration in include/kinetica_hip.h: integers by value, pointers by what is read back through
them at the documented shape. Then the refusals (class and message, and no call made), the results (shape, the buffer the
library wrote, no alias of the caller's array) and, on the real library, the argtypes of every symbol."""
import ctypes
from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from kinetica_jl_amd import capi

HANDLE = 0xDEAD0
N, R = 4, 3                     # species and reactions of the stand-in handle
N_SAVED = 5                     # kin_solution_size
ENS_K, ENS_ROWS, ENS_SAVED = 2, 5, (5, 1)      # kin_ensemble_size
E, E2, JNNZ = 7, 9, 6           # kin_drg_pattern, kin_pfa_pattern, kin_jac_nnz
COUNT = 3                       # the participants the moments entries report
SOLVE_ROWS = 3                  # the save grid of an ensemble solve


class FakeLib:
    """Stands in for the loaded library: records (entry, args), answers the size queries, returns KIN_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("kin_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            if name == "kin_last_error":
                return b"stand-in"
            if name == "kin_solution_size":
                for a, v in zip(args[1:], (N_SAVED, N)):
                    if a is not None:
                        a._obj.value = v
            elif name == "kin_ensemble_size":
                for a, v in zip(args[1:4], (ENS_K, ENS_ROWS, N)):
                    if a is not None:
                        a._obj.value = v
                if args[4] is not None:
                    for i, v in enumerate(ENS_SAVED):
                        args[4][i] = v
            elif name in ("kin_drg_pattern", "kin_pfa_pattern"):
                if args[3] is not None:
                    args[3]._obj.value = E if name == "kin_drg_pattern" else E2
            elif name == "kin_jac_nnz":
                args[1]._obj.value = JNNZ
            elif name in ("kin_members_moments", "kin_members_moments_dev"):
                args[5]._obj.value = COUNT
            elif name == "kin_ensemble_moments":
                args[2]._obj.value = COUNT
            elif name.startswith("kin_solve_ensemble_"):
                args[-6]._obj.value = SOLVE_ROWS
            return capi.KIN_OK
        return entry

    def of(self, name):
        """The calls of an entry that are no pure size query."""
        if name in ("kin_drg_pattern", "kin_pfa_pattern"):
            return [a for n, a in self.calls if n == name and a[4] is not None]
        if name.startswith("kin_solve_ensemble_"):
            return [a for n, a in self.calls if n == name and a[-5] is not None]
        return [a for n, a in self.calls if n == name]


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(capi, "lib", lambda: f)
    return f


@pytest.fixture
def h(fake):
    net = object.__new__(capi.HipNetwork)
    net._h, net.n, net.nr = c_void_p(HANDLE), N, R
    yield net
    net._h = None       # (nothing to destroy)


# ---- what an argument must be --------------------------------------------------------------------------------------------
class _Handle:
    pass


class _Ref:
    pass


H, REF = _Handle(), _Ref()


class F:
    """A non-null pointer to doubles holding `a` (read at a's shape)."""
    ctype = c_double

    def __init__(self, a):
        self.a = np.asarray(a, dtype=np.dtype(self.ctype))


class I64(F):
    ctype = c_int64


class I32(F):
    ctype = c_int32


class Out:
    """A non-null pointer to `ctype`: an output. get(result): the returned array, which must be of `shape` and start at the
    pointer's address; seed: the values the buffer must hold at the call (accumulate)."""

    def __init__(self, get=None, shape=None, seed=None, ctype=c_double):
        self.get, self.shape, self.seed, self.ctype = get, shape, seed, ctype


class Dev:
    """A device pointer given as the int v: a c_void_p of that value; NULL for 0."""

    def __init__(self, v):
        self.v = v


def _address(p):
    return ctypes.cast(p, c_void_p).value


def check_call(got, want, result=None):
    assert len(got) == len(want), f"{len(got)} arguments, the declaration has {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        where = f"argument {i}"
        if w is H:
            assert isinstance(g, c_void_p) and g.value == HANDLE, where
        elif w is REF:
            assert hasattr(g, "_obj"), where
        elif w is None:
            assert g is None, where
        elif isinstance(w, (int, np.integer)):
            assert isinstance(g, (int, np.integer)) and g == w, f"{where}: {g!r}, expected {w}"
        elif isinstance(w, Dev):
            if w.v == 0:
                assert g is None or (isinstance(g, c_void_p) and not g.value), where
            else:
                assert isinstance(g, c_void_p) and g.value == w.v, where
        elif isinstance(w, F):
            assert isinstance(g, POINTER(w.ctype)) and _address(g), where
            if w.a.size:
                np.testing.assert_array_equal(np.ctypeslib.as_array(g, w.a.shape), w.a, err_msg=where)
        elif isinstance(w, Out):
            assert isinstance(g, POINTER(w.ctype)) and _address(g), where
            if w.seed is not None:
                seed = np.asarray(w.seed)
                np.testing.assert_array_equal(np.ctypeslib.as_array(g, seed.shape), seed, err_msg=where)
            if w.get is not None:
                r = w.get(result)
                assert isinstance(r, np.ndarray) and r.shape == w.shape and r.dtype == np.dtype(w.ctype), f"{where}: {r.shape}"
                assert r.size == 0 or r.ctypes.data == _address(g), f"{where}: the result is not the buffer the library wrote"
        else:
            raise TypeError(w)


# ---- the rate-constant sources of a pass over B states: keywords, and the C arguments (k, n_k_rows, k_row, T) -----------------
K_TABLE = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])


def sources(B, t_name="T"):
    k_state = np.arange(3.0 * B).reshape(B, R) + 0.5
    rows = np.arange(B) % 2
    T = 300.0 + 10.0 * np.arange(B)
    return {"none": ({}, [None, 0, None, None]),
            "k": (dict(k=k_state), [F(k_state), B, None, None]),
            "k_row": (dict(k=K_TABLE, k_row=rows), [F(K_TABLE), 2, I64(rows), None]),
            "T": ({t_name: T}, [None, 0, None, F(T)])}


U = np.arange(8.0).reshape(2, N) + 1.0          # B = 2 states
B = 2
SOL, ENS = N_SAVED, ENS_K * ENS_ROWS           # the states of the stored solution / the stored ensemble
CASES = []


def case(name, method, args, kw, entry, want):
    CASES.append(pytest.param(method, args, kw, entry, want, id=name))


def whole(r):
    return r


def item(i):
    return lambda r: r[i]


# --- reaction fluxes: kin_flux_batched(h, B, u, k, n_k_rows, k_row, T, w, flux, rates)
W2, W5, W10 = np.array([0.5, 2.0]), np.arange(5.0) + 1.0, np.arange(10.0) - 3.0
for s, (kw, ks) in sources(B).items():
    case(f"flux_batched-{s}", "flux_batched", (U,), kw, "kin_flux_batched", [H, 2, F(U)] + ks + [None, Out(whole, (R,)), None])
kw, ks = sources(B)["k"]
case("flux_batched-w-rates", "flux_batched", (U,), dict(kw, w=W2, want_rates=True), "kin_flux_batched",
     [H, 2, F(U)] + ks + [F(W2), Out(item(0), (R,)), Out(item(1), (2, R))])
case("flux_batched-rates-only", "flux_batched", (U,), dict(want_rates=True, want_flux=False), "kin_flux_batched",
     [H, 2, F(U), None, 0, None, None, None, None, Out(item(1), (2, R))])
case("flux_batched-one-state", "flux_batched", (U[0],), {}, "kin_flux_batched",
     [H, 1, F(U[:1]), None, 0, None, None, None, Out(whole, (R,)), None])
# kin_flux_batched_dev(h, B, d_u, d_k, d_k_row, d_T, d_w, d_flux, d_rates, stream)
case("flux_batched_dev-all", "flux_batched_dev", (6, 0x100), dict(d_k=0x200, d_k_row=0x300, d_T=0x400, d_w=0x500, d_flux=0x600, d_rates=0x700,
                                                                  stream=0x800), "kin_flux_batched_dev",
     [H, 6] + [Dev(v) for v in (0x100, 0x200, 0x300, 0x400, 0x500, 0x600, 0x700, 0x800)])
case("flux_batched_dev-least", "flux_batched_dev", (6, 0x100), dict(d_flux=0x600), "kin_flux_batched_dev",
     [H, 6, Dev(0x100), Dev(0), Dev(0), Dev(0), Dev(0), Dev(0x600), Dev(0), Dev(0)])
# kin_solution_flux(h, w, k, n_k_rows, k_row, T_rows, flux, rates)
kw, ks = sources(SOL, "T_rows")["k_row"]
case("solution_flux-k_row", "solution_flux", (), dict(kw, w=W5, want_rates=True), "kin_solution_flux",
     [H, F(W5)] + ks + [Out(item(0), (R,)), Out(item(1), (SOL, R))])
kw, ks = sources(SOL, "T_rows")["T"]
case("solution_flux-T", "solution_flux", (), kw, "kin_solution_flux", [H, None] + ks + [Out(whole, (R,)), None])
case("solution_flux-table", "solution_flux", (), dict(k_row=np.arange(5)), "kin_solution_flux",
     [H, None, None, 0, I64(np.arange(5)), None, Out(whole, (R,)), None])
# kin_flux_segmented(h, S, L, seg_n, u, k, n_k_rows, k_row, T, w, flux)
U3 = np.arange(24.0).reshape(2, 3, N)
kw, ks = sources(6)["k_row"]
case("flux_segmented-k_row", "flux_segmented", (U3,), dict(kw, seg_n=[3, 1], w=np.arange(6.0).reshape(2, 3)), "kin_flux_segmented",
     [H, 2, 3, I64([3, 1]), F(U3)] + ks + [F(np.arange(6.0)), Out(whole, (2, R))])
kw, ks = sources(6)["T"]
case("flux_segmented-T", "flux_segmented", (U3,), kw, "kin_flux_segmented", [H, 2, 3, None, F(U3)] + ks + [None, Out(whole, (2, R))])
# kin_flux_segmented_dev(h, S, L, d_seg_n, d_u, d_k, d_k_row, d_T, d_w, d_flux, stream)
case("flux_segmented_dev-all", "flux_segmented_dev", (2, 3, 0x100, 0x200), dict(d_seg_n=0x300, d_k=0x400, d_k_row=0x500, d_T=0x600, d_w=0x700,
                                                                              stream=0x800), "kin_flux_segmented_dev",
     [H, 2, 3] + [Dev(v) for v in (0x300, 0x100, 0x400, 0x500, 0x600, 0x700, 0x200, 0x800)])
case("flux_segmented_dev-least", "flux_segmented_dev", (2, 3, 0x100, 0x200), {}, "kin_flux_segmented_dev",
     [H, 2, 3, Dev(0), Dev(0x100), Dev(0), Dev(0), Dev(0), Dev(0), Dev(0x200), Dev(0)])
# the stored ensemble: kin_ensemble_max(h, out), kin_ensemble_dot(h, w, out), kin_ensemble_flux(h, w, k, n_k_rows, k_row, T_rows, flux)
case("ensemble_max", "ensemble_max", (), {}, "kin_ensemble_max", [H, Out(whole, (ENS_K, N))])
case("ensemble_dot", "ensemble_dot", ([1.0, 2.0, 3.0, 4.0],), {}, "kin_ensemble_dot", [H, F([1.0, 2.0, 3.0, 4.0]), Out(whole, (ENS_K, ENS_ROWS))])
for s, (kw, ks) in sources(ENS, "T_rows").items():
    if s in ("T", "k"):
        case(f"ensemble_flux-{s}", "ensemble_flux", (), dict(kw, w=W10.reshape(2, 5)), "kin_ensemble_flux",
             [H, F(W10)] + ks + [Out(whole, (ENS_K, R))])
case("ensemble_flux-none", "ensemble_flux", (), {}, "kin_ensemble_flux", [H, None, None, 0, None, None, Out(whole, (ENS_K, R))])

# --- directed relation graph: all three forms with every source
COEF, COEF2 = np.arange(7.0) / 8.0, np.arange(9.0) / 16.0
case("drg_pattern", "drg_pattern", (), {}, "kin_drg_pattern", [H, 1, 0, None, Out(item(0), (N + 1,), ctype=c_int64), Out(item(1), (E,), ctype=c_int64)])
case("drg_pattern-unpaired", "drg_pattern", (False,), {}, "kin_drg_pattern",
     [H, 0, 0, None, Out(item(0), (N + 1,), ctype=c_int64), Out(item(1), (E,), ctype=c_int64)])
case("pfa_pattern", "pfa_pattern", (), {}, "kin_pfa_pattern", [H, 1, 0, None, Out(item(0), (N + 1,), ctype=c_int64), Out(item(1), (E2,), ctype=c_int64)])
case("pfa_pattern-unpaired", "pfa_pattern", (), dict(pairing=False), "kin_pfa_pattern",
     [H, 0, 0, None, Out(item(0), (N + 1,), ctype=c_int64), Out(item(1), (E2,), ctype=c_int64)])
for s, (kw, ks) in sources(B).items():
    # kin_drg_batched(h, pairing, B, u, k, n_k_rows, k_row, T, accumulate, coef)
    case(f"drg_batched-{s}", "drg_batched", (U,), kw, "kin_drg_batched", [H, 1, 2, F(U)] + ks + [0, Out(whole, (E,))])
for form, nb in (("solution", SOL), ("ensemble", ENS)):
    for s, (kw, ks) in sources(nb, "T_rows").items():
        # kin_solution_drg / kin_ensemble_drg(h, pairing, k, n_k_rows, k_row, T_rows, accumulate, coef)
        case(f"{form}_drg-{s}", f"{form}_drg", (), kw, f"kin_{form}_drg", [H, 1] + ks + [0, Out(whole, (E,))])
    case(f"{form}_drg-accumulate-unpaired", f"{form}_drg", (), dict(pairing=False, coef=COEF), f"kin_{form}_drg",
         [H, 0, None, 0, None, None, 1, Out(whole, (E,), seed=COEF)])
    # ... and the same of kin_solution_pfa / kin_ensemble_pfa
    kw, ks = sources(nb, "T_rows")["k_row" if form == "solution" else "T"]
    case(f"{form}_pfa", f"{form}_pfa", (), kw, f"kin_{form}_pfa", [H, 1] + ks + [0, Out(whole, (E2,))])
    case(f"{form}_pfa-accumulate-unpaired", f"{form}_pfa", (), dict(pairing=False, coef=COEF2), f"kin_{form}_pfa",
         [H, 0, None, 0, None, None, 1, Out(whole, (E2,), seed=COEF2)])
case("drg_batched-accumulate-unpaired", "drg_batched", (U,), dict(pairing=False, coef=COEF), "kin_drg_batched",
     [H, 0, 2, F(U), None, 0, None, None, 1, Out(whole, (E,), seed=COEF)])
# kin_drg_batched_dev / kin_pfa_batched_dev(h, pairing, B, d_u, d_k, d_k_row, d_T, accumulate, d_coef, stream)
for p in ("drg", "pfa"):
    case(f"{p}_batched_dev-all", f"{p}_batched_dev", (6, 0x100, 0x200), dict(d_k=0x300, d_k_row=0x400, d_T=0x500, pairing=False, accumulate=True,
                                                                            stream=0x600), f"kin_{p}_batched_dev",
         [H, 0, 6, Dev(0x100), Dev(0x300), Dev(0x400), Dev(0x500), 1, Dev(0x200), Dev(0x600)])
    case(f"{p}_batched_dev-least", f"{p}_batched_dev", (6, 0x100, 0x200), {}, f"kin_{p}_batched_dev",
         [H, 1, 6, Dev(0x100), Dev(0), Dev(0), Dev(0), 0, Dev(0x200), Dev(0)])

# --- DRGEP: kin_drgep_batched(h, pairing, B, u, k, n_k_rows, k_row, T, targets, n_targets, index_base, accumulate, importance, r_out,
#     R_out, rounds_out)
IMP_N, IMP_R = np.array([0.25, 0.5, 0.0, 1.0]), np.array([0.125, 0.0, 0.75])
kw, ks = sources(B)["none"]
case("drgep_batched-none", "drgep_batched", (U, [2, 0]), kw, "kin_drgep_batched",
     [H, 1, 2, F(U)] + ks + [I64([2, 0]), 2, 0, 0, Out(whole, (N,), seed=np.zeros(N)), None, None, None])
kw, ks = sources(B)["k"]
case("drgep_batched-k-stages-accumulate", "drgep_batched", (U, [3]), dict(kw, pairing=False, importance=IMP_N, stages=True), "kin_drgep_batched",
     [H, 0, 2, F(U)] + ks + [I64([3]), 1, 0, 1, Out(item(0), (N,), seed=IMP_N), Out(item(1), (2, E)), Out(item(2), (2, N)),
                             Out(item(3), (2,), ctype=c_int32)])
# kin_drgep_paths(h, pairing, B, r, targets, n_targets, index_base, accumulate, importance, R_out, rounds_out)
R_IN = np.arange(14.0).reshape(2, E) / 16.0
case("drgep_paths", "drgep_paths", (R_IN, [1]), {}, "kin_drgep_paths",
     [H, 1, 2, F(R_IN), I64([1]), 1, 0, 0, Out(whole, (N,), seed=np.zeros(N)), None, None])
case("drgep_paths-stages-accumulate", "drgep_paths", (R_IN.ravel(), [1, 2]), dict(pairing=False, importance=IMP_N, stages=True), "kin_drgep_paths",
     [H, 0, 2, F(R_IN), I64([1, 2]), 2, 0, 1, Out(item(0), (N,), seed=IMP_N), Out(item(1), (2, N)), Out(item(2), (2,), ctype=c_int32)])
# kin_solution_drgep / kin_ensemble_drgep(h, pairing, k, n_k_rows, k_row, T_rows, targets, n_targets, index_base, accumulate, importance)
kw, ks = sources(SOL, "T_rows")["k_row"]
case("solution_drgep-k_row", "solution_drgep", ([0, 3],), kw, "kin_solution_drgep",
     [H, 1] + ks + [I64([0, 3]), 2, 0, 0, Out(whole, (N,), seed=np.zeros(N))])
kw, ks = sources(ENS, "T_rows")["T"]
case("ensemble_drgep-T-accumulate", "ensemble_drgep", ([1],), dict(kw, pairing=False, importance=IMP_N), "kin_ensemble_drgep",
     [H, 0] + ks + [I64([1]), 1, 0, 1, Out(whole, (N,), seed=IMP_N)])
# kin_drgep_batched_dev(h, pairing, B, d_u, d_k, d_k_row, d_T, d_targets, n_targets, accumulate, d_importance, stream)
case("drgep_batched_dev-all", "drgep_batched_dev", (6, 0x100, 0x200, 2, 0x300),
     dict(d_k=0x400, d_k_row=0x500, d_T=0x600, pairing=False, accumulate=True, stream=0x700), "kin_drgep_batched_dev",
     [H, 0, 6, Dev(0x100), Dev(0x400), Dev(0x500), Dev(0x600), Dev(0x200), 2, 1, Dev(0x300), Dev(0x700)])
case("drgep_batched_dev-least", "drgep_batched_dev", (6, 0x100, 0x200, 2, 0x300), {}, "kin_drgep_batched_dev",
     [H, 1, 6, Dev(0x100), Dev(0), Dev(0), Dev(0), Dev(0x200), 2, 0, Dev(0x300), Dev(0)])

# --- reaction elimination: kin_reaction_importance_batched(h, pairing, B, u, k, n_k_rows, k_row, T, species, n_sel, index_base,
#     accumulate, importance, per_state)
kw, ks = sources(B)["none"]
case("reaction_importance_batched-none", "reaction_importance_batched", (U,), kw, "kin_reaction_importance_batched",
     [H, 1, 2, F(U)] + ks + [None, 0, 0, 0, Out(whole, (R,), seed=np.zeros(R)), None])
kw, ks = sources(B)["k"]
case("reaction_importance_batched-k-species-per_state-accumulate", "reaction_importance_batched", (U,),
     dict(kw, species=[3, 1], pairing=False, importance=IMP_R, per_state=True), "kin_reaction_importance_batched",
     [H, 0, 2, F(U)] + ks + [I64([3, 1]), 2, 0, 1, Out(item(0), (R,), seed=IMP_R), Out(item(1), (2, R))])
case("reaction_importance_batched-empty-list", "reaction_importance_batched", (U,), dict(species=[]), "kin_reaction_importance_batched",
     [H, 1, 2, F(U), None, 0, None, None, Out(ctype=c_int64), 0, 0, 0, Out(whole, (R,)), None])
# kin_solution_ / kin_ensemble_reaction_importance(h, pairing, k, n_k_rows, k_row, T_rows, species, n_sel, index_base, accumulate, importance)
kw, ks = sources(SOL, "T_rows")["k_row"]
case("solution_reaction_importance-k_row", "solution_reaction_importance", (), dict(kw, species=[2]), "kin_solution_reaction_importance",
     [H, 1] + ks + [I64([2]), 1, 0, 0, Out(whole, (R,), seed=np.zeros(R))])
case("solution_reaction_importance-empty-list", "solution_reaction_importance", ([],), {}, "kin_solution_reaction_importance",
     [H, 1, None, 0, None, None, Out(ctype=c_int64), 0, 0, 0, Out(whole, (R,))])
kw, ks = sources(ENS, "T_rows")["T"]
case("ensemble_reaction_importance-T-accumulate", "ensemble_reaction_importance", (), dict(kw, pairing=False, importance=IMP_R),
     "kin_ensemble_reaction_importance", [H, 0] + ks + [None, 0, 0, 1, Out(whole, (R,), seed=IMP_R)])
case("ensemble_reaction_importance-empty-list", "ensemble_reaction_importance", (), dict(species=[]), "kin_ensemble_reaction_importance",
     [H, 1, None, 0, None, None, Out(ctype=c_int64), 0, 0, 0, Out(whole, (R,))])
# kin_reaction_importance_batched_dev(h, pairing, B, d_u, d_k, d_k_row, d_T, d_species, n_sel, accumulate, d_importance, stream)
case("reaction_importance_batched_dev-all", "reaction_importance_batched_dev", (6, 0x100, 0x200),
     dict(d_species=0x300, n_sel=2, d_k=0x400, d_k_row=0x500, d_T=0x600, pairing=False, accumulate=True, stream=0x700),
     "kin_reaction_importance_batched_dev", [H, 0, 6, Dev(0x100), Dev(0x400), Dev(0x500), Dev(0x600), Dev(0x300), 2, 1, Dev(0x200), Dev(0x700)])
case("reaction_importance_batched_dev-least", "reaction_importance_batched_dev", (6, 0x100, 0x200), {}, "kin_reaction_importance_batched_dev",
     [H, 1, 6, Dev(0x100), Dev(0), Dev(0), Dev(0), Dev(0), 0, 0, Dev(0x200), Dev(0)])

# --- path flux analysis: kin_pfa_batched(h, pairing, B, u, k, n_k_rows, k_row, T, accumulate, coef, rp_out, rc_out, r_out)
kw, ks = sources(B)["none"]
case("pfa_batched-none", "pfa_batched", (U,), kw, "kin_pfa_batched", [H, 1, 2, F(U)] + ks + [0, Out(whole, (E2,), seed=np.zeros(E2)), None, None, None])
kw, ks = sources(B)["k"]
case("pfa_batched-k-stages-accumulate", "pfa_batched", (U,), dict(kw, pairing=False, coef=COEF2, stages=True), "kin_pfa_batched",
     [H, 0, 2, F(U)] + ks + [1, Out(item(0), (E2,), seed=COEF2), Out(item(1), (2, E)), Out(item(2), (2, E)), Out(item(3), (2, E2))])
# kin_pfa_paths(h, pairing, B, rp, rc, accumulate, coef, r_out)
case("pfa_paths", "pfa_paths", (R_IN, R_IN[::-1]), {}, "kin_pfa_paths",
     [H, 1, 2, F(R_IN), F(R_IN[::-1]), 0, Out(whole, (E2,), seed=np.zeros(E2)), None])
case("pfa_paths-stages-accumulate", "pfa_paths", (R_IN, 2.0 * R_IN), dict(pairing=False, coef=COEF2, stages=True), "kin_pfa_paths",
     [H, 0, 2, F(R_IN), F(2.0 * R_IN), 1, Out(item(0), (E2,), seed=COEF2), Out(item(1), (2, E2))])

# --- timescale analysis: kin_jac_batched(h, B, u, k, n_k_rows, k_row, T, vals)
for s in ("none", "k_row"):
    kw, ks = sources(B)[s]
    case(f"jac_batched-{s}", "jac_batched", (U,), kw, "kin_jac_batched", [H, 2, F(U)] + ks + [Out(whole, (2, JNNZ))])
# kin_jac_batched_dev(h, B, d_u, d_k, d_k_row, d_T, d_vals, stream)
case("jac_batched_dev-all", "jac_batched_dev", (6, 0x100, 0x200), dict(d_k=0x300, d_k_row=0x400, d_T=0x500, stream=0x600), "kin_jac_batched_dev",
     [H, 6, Dev(0x100), Dev(0x300), Dev(0x400), Dev(0x500), Dev(0x200), Dev(0x600)])
case("jac_batched_dev-least", "jac_batched_dev", (6, 0x100, 0x200), {}, "kin_jac_batched_dev",
     [H, 6, Dev(0x100), Dev(0), Dev(0), Dev(0), Dev(0x200), Dev(0)])
# kin_timescale_batched(h, B, u, k, n_k_rows, k_row, T, accumulate, summary, diag, err, norm)
SUMMARY = np.arange(12.0).reshape(3, N) - 2.0
kw, ks = sources(B)["none"]
case("timescale_batched-none", "timescale_batched", (U,), kw, "kin_timescale_batched",
     [H, 2, F(U)] + ks + [0, Out(lambda r: r["summary"], (3, N)), None, None, Out(lambda r: r["norm"], (2,))])
kw, ks = sources(B)["k"]
case("timescale_batched-k-all-accumulate", "timescale_batched", (U,), dict(kw, summary=SUMMARY, want_diag=True, want_err=True),
     "kin_timescale_batched", [H, 2, F(U)] + ks + [1, Out(lambda r: r["summary"], (3, N), seed=SUMMARY), Out(lambda r: r["diag"], (2, N)),
                                                   Out(lambda r: r["err"], (2, N)), Out(lambda r: r["norm"], (2,))])
kw, ks = sources(B)["T"]
case("timescale_batched-T-diag-only", "timescale_batched", (U,), dict(kw, want_summary=False, want_diag=True, want_norm=False),
     "kin_timescale_batched", [H, 2, F(U)] + ks + [0, None, Out(lambda r: r["diag"], (2, N)), None, None])
# kin_timescale_batched_dev(h, B, d_u, d_k, d_k_row, d_T, accumulate, d_summary, d_diag, d_err, d_norm, stream)
case("timescale_batched_dev-all", "timescale_batched_dev", (6, 0x100),
     dict(d_summary=0x200, d_diag=0x300, d_err=0x400, d_norm=0x500, d_k=0x600, d_k_row=0x700, d_T=0x800, accumulate=True, stream=0x900),
     "kin_timescale_batched_dev", [H, 6, Dev(0x100), Dev(0x600), Dev(0x700), Dev(0x800), 1, Dev(0x200), Dev(0x300), Dev(0x400), Dev(0x500), Dev(0x900)])
case("timescale_batched_dev-least", "timescale_batched_dev", (6, 0x100), dict(d_norm=0x500), "kin_timescale_batched_dev",
     [H, 6, Dev(0x100), Dev(0), Dev(0), Dev(0), 0, Dev(0), Dev(0), Dev(0), Dev(0x500), Dev(0)])
# kin_solution_timescale / kin_ensemble_timescale(h, k, n_k_rows, k_row, T_rows, row_begin, accumulate, summary, norm)
kw, ks = sources(SOL, "T_rows")["k_row"]
case("solution_timescale-k_row", "solution_timescale", (), dict(kw, row_begin=2), "kin_solution_timescale",
     [H] + ks + [2, 0, Out(item(0), (3, N)), Out(item(1), (SOL,))])
case("solution_timescale-accumulate-no-norm", "solution_timescale", (), dict(summary=SUMMARY, want_norm=False), "kin_solution_timescale",
     [H, None, 0, None, None, 0, 1, Out(item(0), (3, N), seed=SUMMARY), None])
kw, ks = sources(ENS, "T_rows")["T"]
case("ensemble_timescale-T", "ensemble_timescale", (), dict(kw, row_begin=1), "kin_ensemble_timescale",
     [H] + ks + [1, 0, Out(item(0), (3, N)), Out(item(1), (ENS_K, ENS_ROWS))])
case("ensemble_timescale-accumulate-no-norm", "ensemble_timescale", (), dict(summary=SUMMARY, want_norm=False), "kin_ensemble_timescale",
     [H, None, 0, None, None, 0, 1, Out(item(0), (3, N), seed=SUMMARY), None])

# --- cross-member statistics over u[K][L][N], K = 3 members of L = 2 rows
UM = np.arange(24.0).reshape(3, 2, N)
USE3, USE2 = [1, 0, 2], [0, 7]             # (truthy: takes part; the entries take 0 / 1)
key = lambda q: (lambda r: r[q])
# kin_members_moments(h, K, L, u, use, count, mean, var, min, max)
case("members_moments", "members_moments", (UM,), {}, "kin_members_moments",
     [H, 3, 2, F(UM), None, REF] + [Out(key(q), (2, N)) for q in ("mean", "var", "min", "max")])
case("members_moments-use-some", "members_moments", (UM,), dict(use=USE3, want=("var", "max")), "kin_members_moments",
     [H, 3, 2, F(UM), I32([1, 0, 1]), REF, None, Out(key("var"), (2, N)), None, Out(key("max"), (2, N))])
# kin_members_moments_dev(h, K, L, d_u, use, count, d_mean, d_var, d_min, d_max, stream)
case("members_moments_dev-all", "members_moments_dev", (3, 2, 0x100), dict(use=USE3, d_mean=0x200, d_var=0x300, d_min=0x400, d_max=0x500, stream=0x600),
     "kin_members_moments_dev", [H, 3, 2, Dev(0x100), I32([1, 0, 1]), REF, Dev(0x200), Dev(0x300), Dev(0x400), Dev(0x500), Dev(0x600)])
case("members_moments_dev-least", "members_moments_dev", (3, 2, 0x100), dict(d_min=0x400), "kin_members_moments_dev",
     [H, 3, 2, Dev(0x100), None, REF, Dev(0), Dev(0), Dev(0x400), Dev(0), Dev(0)])
# kin_ensemble_moments(h, use, count, mean, var, min, max)
case("ensemble_moments", "ensemble_moments", (), {}, "kin_ensemble_moments", [H, None, REF] + [Out(key(q), (ENS_ROWS, N)) for q in ("mean", "var", "min", "max")])
case("ensemble_moments-use-some", "ensemble_moments", (), dict(use=USE2, want=("count", "mean")), "kin_ensemble_moments",
     [H, I32([0, 1]), REF, Out(key("mean"), (ENS_ROWS, N)), None, None, None])
# kin_members_quantiles(h, K, L, u, use, species, n_sel, p, Q, out)
PQ = [0.25, 0.5, 1.0]
case("members_quantiles", "members_quantiles", (UM, PQ), {}, "kin_members_quantiles", [H, 3, 2, F(UM), None, None, 0, F(PQ), 3, Out(whole, (3, 2, N))])
case("members_quantiles-species-use", "members_quantiles", (UM, 0.5), dict(species=[2, 0], use=USE3), "kin_members_quantiles",
     [H, 3, 2, F(UM), I32([1, 0, 1]), I64([2, 0]), 2, F([0.5]), 1, Out(whole, (1, 2, 2))])
case("members_quantiles-empty-list", "members_quantiles", (UM, PQ), dict(species=[]), "kin_members_quantiles",
     [H, 3, 2, F(UM), None, Out(ctype=c_int64), 0, F(PQ), 3, Out(whole, (3, 2, 0))])
# kin_members_quantiles_dev(h, K, L, d_u, use, species, n_sel, p, Q, d_out, stream)
case("members_quantiles_dev-all", "members_quantiles_dev", (3, 2, 0x100, PQ, 0x200), dict(species=[1], use=USE3, stream=0x300), "kin_members_quantiles_dev",
     [H, 3, 2, Dev(0x100), I32([1, 0, 1]), I64([1]), 1, F(PQ), 3, Dev(0x200), Dev(0x300)])
case("members_quantiles_dev-least", "members_quantiles_dev", (3, 2, 0x100, PQ, 0x200), {}, "kin_members_quantiles_dev",
     [H, 3, 2, Dev(0x100), None, None, 0, F(PQ), 3, Dev(0x200), Dev(0)])
case("members_quantiles_dev-empty-list", "members_quantiles_dev", (3, 2, 0x100, PQ, 0x200), dict(species=[]), "kin_members_quantiles_dev",
     [H, 3, 2, Dev(0x100), None, Out(ctype=c_int64), 0, F(PQ), 3, Dev(0x200), Dev(0)])
# kin_ensemble_quantiles(h, use, species, n_sel, p, Q, out)
case("ensemble_quantiles", "ensemble_quantiles", (PQ,), {}, "kin_ensemble_quantiles", [H, None, None, 0, F(PQ), 3, Out(whole, (3, ENS_ROWS, N))])
case("ensemble_quantiles-species-use", "ensemble_quantiles", (PQ,), dict(species=[3], use=USE2), "kin_ensemble_quantiles",
     [H, I32([0, 1]), I64([3]), 1, F(PQ), 3, Out(whole, (3, ENS_ROWS, 1))])
case("ensemble_quantiles-empty-list", "ensemble_quantiles", (PQ,), dict(species=[]), "kin_ensemble_quantiles",
     [H, None, Out(ctype=c_int64), 0, F(PQ), 3, Out(whole, (3, ENS_ROWS, 0))])
# kin_members_correlate(h, K, L, u, use, species, n_sel, X, P, rank, out)
X3, X2 = np.arange(6.0).reshape(3, 2) * 0.5, np.array([[1.0, 2.0, 4.0], [0.0, 8.0, 3.0]])
case("members_correlate", "members_correlate", (UM, X3), {}, "kin_members_correlate", [H, 3, 2, F(UM), None, None, 0, F(X3), 2, 1, Out(whole, (2, N, 2))])
case("members_correlate-species-pearson-use", "members_correlate", (UM, X3), dict(species=[1, 3, 0], rank=False, use=USE3), "kin_members_correlate",
     [H, 3, 2, F(UM), I32([1, 0, 1]), I64([1, 3, 0]), 3, F(X3), 2, 0, Out(whole, (2, 3, 2))])
case("members_correlate-empty-list", "members_correlate", (UM, X3), dict(species=[]), "kin_members_correlate",
     [H, 3, 2, F(UM), None, Out(ctype=c_int64), 0, F(X3), 2, 1, Out(whole, (2, 0, 2))])
# kin_members_correlate_dev(h, K, L, d_u, use, species, n_sel, X, P, rank, d_out, stream)
case("members_correlate_dev-all", "members_correlate_dev", (3, 2, 0x100, X3, 0x200), dict(species=[2], rank=False, use=USE3, stream=0x300),
     "kin_members_correlate_dev", [H, 3, 2, Dev(0x100), I32([1, 0, 1]), I64([2]), 1, F(X3), 2, 0, Dev(0x200), Dev(0x300)])
case("members_correlate_dev-least", "members_correlate_dev", (3, 2, 0x100, X3, 0x200), {}, "kin_members_correlate_dev",
     [H, 3, 2, Dev(0x100), None, None, 0, F(X3), 2, 1, Dev(0x200), Dev(0)])
case("members_correlate_dev-empty-list", "members_correlate_dev", (3, 2, 0x100, X3, 0x200), dict(species=[]), "kin_members_correlate_dev",
     [H, 3, 2, Dev(0x100), None, Out(ctype=c_int64), 0, F(X3), 2, 1, Dev(0x200), Dev(0)])
# kin_ensemble_correlate(h, use, species, n_sel, X, P, rank, out)
case("ensemble_correlate", "ensemble_correlate", (X2,), {}, "kin_ensemble_correlate", [H, None, None, 0, F(X2), 3, 1, Out(whole, (ENS_ROWS, N, 3))])
case("ensemble_correlate-species-pearson-use", "ensemble_correlate", (X2,), dict(species=[0, 1], rank=False, use=USE2), "kin_ensemble_correlate",
     [H, I32([0, 1]), I64([0, 1]), 2, F(X2), 3, 0, Out(whole, (ENS_ROWS, 2, 3))])
case("ensemble_correlate-empty-list", "ensemble_correlate", (X2,), dict(species=[]), "kin_ensemble_correlate",
     [H, None, Out(ctype=c_int64), 0, F(X2), 3, 1, Out(whole, (ENS_ROWS, 0, 3))])

# --- Sobol indices: a design of M = 2 base samples and P = 1 input is 6 members; L = 2 rows
US = np.arange(48.0).reshape(6, 2, N)
sobol_out = lambda nsel, L=2, P=1: [Out(key("first"), (L, nsel, P)), Out(key("total"), (L, nsel, P)), Out(key("mean"), (L, nsel)), Out(key("var"), (L, nsel))]
# kin_members_sobol(h, M, P, L, u, w, species, n_sel, S1, ST, mean, var)
case("members_sobol", "members_sobol", (US, 2, 1), {}, "kin_members_sobol", [H, 2, 1, 2, F(US), None, None, 0] + sobol_out(N))
case("members_sobol-species-w", "members_sobol", (US, 2, 1), dict(species=[3, 0], w=[2, 0]), "kin_members_sobol",
     [H, 2, 1, 2, F(US), I32([2, 0]), I64([3, 0]), 2] + sobol_out(2))
case("members_sobol-empty-list", "members_sobol", (US, 2, 1), dict(species=[]), "kin_members_sobol",
     [H, 2, 1, 2, F(US), None, Out(ctype=c_int64), 0] + sobol_out(0))
# kin_members_sobol_dev(h, M, P, L, d_u, w, species, n_sel, d_S1, d_ST, d_mean, d_var, stream)
case("members_sobol_dev-all", "members_sobol_dev", (2, 1, 2, 0x100), dict(d_first=0x200, d_total=0x300, d_mean=0x400, d_var=0x500, species=[1],
                                                                        w=np.array([1, 3]), stream=0x600), "kin_members_sobol_dev",
     [H, 2, 1, 2, Dev(0x100), I32([1, 3]), I64([1]), 1, Dev(0x200), Dev(0x300), Dev(0x400), Dev(0x500), Dev(0x600)])
case("members_sobol_dev-least", "members_sobol_dev", (2, 1, 2, 0x100), dict(d_total=0x300), "kin_members_sobol_dev",
     [H, 2, 1, 2, Dev(0x100), None, None, 0, Dev(0), Dev(0x300), Dev(0), Dev(0), Dev(0)])
case("members_sobol_dev-empty-list", "members_sobol_dev", (2, 1, 2, 0x100), dict(d_total=0x300, species=[]), "kin_members_sobol_dev",
     [H, 2, 1, 2, Dev(0x100), None, Out(ctype=c_int64), 0, Dev(0), Dev(0x300), Dev(0), Dev(0), Dev(0)])


@pytest.mark.parametrize("method, args, kw, entry, want", CASES)
def test_the_one_call_of_a_method(fake, h, method, args, kw, entry, want):
    given = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in list(args) + list(kw.values())]
    result = getattr(h, method)(*args, **kw)
    calls = fake.of(entry)
    assert len(calls) == 1, [n for n, _ in fake.calls]
    check_call(calls[0], want, result)
    # every other call is a size query of the handle
    assert {n for n, _ in fake.calls} <= {entry, "kin_solution_size", "kin_ensemble_size", "kin_drg_pattern", "kin_pfa_pattern", "kin_jac_nnz"}
    # the caller's arrays are left alone, and no result aliases one of them
    results = list(result.values()) if isinstance(result, dict) else list(result) if isinstance(result, tuple) else [result]
    for a, before in zip(list(args) + list(kw.values()), given):
        if isinstance(a, np.ndarray):
            np.testing.assert_array_equal(a, before)
            assert not any(isinstance(r, np.ndarray) and np.shares_memory(r, a) for r in results)


def test_dev_methods_return_what_is_documented(fake, h):
    assert h.flux_batched_dev(6, 0x100, d_flux=0x200) is None
    assert h.members_moments_dev(3, 2, 0x100, d_mean=0x200) == COUNT
    assert h.members_quantiles_dev(3, 2, 0x100, [0.5], 0x200) is None
    assert h.members_sobol_dev(2, 1, 2, 0x100, d_first=0x200) is None
    assert not any(n.endswith("_size") or n.endswith("_pattern") or n == "kin_jac_nnz" for n, _ in fake.calls)      # (only enqueue)


def test_ensemble_size_and_the_counts_that_come_back(fake, h):
    K, rows, n, ns = h.ensemble_size()
    assert (K, rows, n) == (ENS_K, ENS_ROWS, N) and ns.dtype == np.int64
    np.testing.assert_array_equal(ns, ENS_SAVED)
    assert all(a[0].value == HANDLE for _, a in fake.calls)
    assert h.members_moments(UM)["count"] == COUNT and h.ensemble_moments()["count"] == COUNT
    assert "count" not in h.members_moments(UM, want=("mean",)) and sorted(h.ensemble_moments(want=("min", "count"))) == ["count", "min"]
    # Sobol: the sum of the weights; of a stored ensemble without weights, the samples all of whose members completed the grid
    assert h.members_sobol(US, 2, 1)["count"] == 2 and h.members_sobol(US, 2, 1, w=[3, 4])["count"] == 7
    with pytest.raises(capi.KineticaHipError, match=r"the stored ensemble has 2 members, not M \(P \+ 2\) = 6") as e:
        h.ensemble_sobol_weights(2, 1)
    assert e.value.code == capi.KIN_ERR_INVALID_ARG


def test_ensemble_sobol_on_a_stored_design(fake, h, monkeypatch):
    """A stored ensemble of M (P + 2) = 2 * 3 = 6 members of 2 rows; sample 1's AB_0 member stopped early."""
    monkeypatch.setitem(globals(), "ENS_K", 6)
    monkeypatch.setitem(globals(), "ENS_ROWS", 2)
    monkeypatch.setitem(globals(), "ENS_SAVED", (2, 2, 2, 2, 2, 1))
    np.testing.assert_array_equal(h.ensemble_sobol_weights(2, 1), [1, 0])
    assert h.ensemble_sobol_weights(2, 1).dtype == np.int32
    # kin_ensemble_sobol(h, M, P, w, species, n_sel, S1, ST, mean, var)
    fake.calls.clear()
    res = h.ensemble_sobol(2, 1)
    check_call(fake.of("kin_ensemble_sobol")[0], [H, 2, 1, None, None, 0] + sobol_out(N), res)
    assert len(fake.of("kin_ensemble_sobol")) == 1 and res["count"] == 1
    fake.calls.clear()
    res = h.ensemble_sobol(2, 1, species=[2], w=np.array([2, 5]))
    check_call(fake.of("kin_ensemble_sobol")[0], [H, 2, 1, I32([2, 5]), I64([2]), 1] + sobol_out(1), res)
    assert res["count"] == 7
    fake.calls.clear()
    res = h.ensemble_sobol(2, 1, species=[])
    check_call(fake.of("kin_ensemble_sobol")[0], [H, 2, 1, None, Out(ctype=c_int64), 0] + sobol_out(0), res)


# ---- the per-member ensemble solves ------------------------------------------------------------------------------------------
def _params():
    return capi.KinParams(tspan0=0.0, tspan1=1.0, abstol=1e-10, reltol=1e-8)


@pytest.mark.parametrize("kind", ["continuous", "discrete"])
@pytest.mark.parametrize("member_params", [False, True])
@pytest.mark.parametrize("trajectories", [True, False])
def test_ensemble_solve_entries(fake, h, kind, member_params, trajectories):
    """kin_solve_ensemble_continuous / _discrete(h, params, K, u0, ptr, t, T, n_rows, out_t, out_u, n_saved, retcodes, stats) and the
    _params forms with Ea[K][R], A[K][R] between u0 and ptr: the size query with null outputs, then the solve."""
    u0 = np.arange(8.0).reshape(2, N)
    pairs = [([0.0, 0.5, 1.0], [300.0, 400.0, 500.0]), ([0.0, 1.0], [350.0, 450.0])]
    Ea, A = np.arange(6.0).reshape(2, R) + 1e4, np.arange(6.0).reshape(2, R) + 0.5
    pars = _params()
    kw = dict(Ea=Ea, A=A) if member_params else {}
    t, u, ns, rcs, stats = getattr(h, "solve_ensemble_" + kind)(pars, u0, pairs, trajectories=trajectories, **kw)
    entry = f"kin_solve_ensemble_{kind}" + ("_params" if member_params else "")
    assert [n for n, _ in fake.calls] == [entry, entry]
    inputs = [H, REF, 2, F(u0)] + ([F(Ea), F(A)] if member_params else []) + \
        [I64([0, 3, 5]), F([0.0, 0.5, 1.0, 0.0, 1.0]), F([300.0, 400.0, 500.0, 350.0, 450.0]), REF]
    check_call(fake.calls[0][1], inputs + [None] * 5)
    assert ctypes.addressof(fake.calls[0][1][1]._obj) == ctypes.addressof(pars)
    (call,) = fake.of(entry)
    result = dict(t=t, u=u, ns=ns, rcs=rcs)
    check_call(call[:-1], inputs + [Out(key("t"), (SOLVE_ROWS,)), Out(key("u"), (2, SOLVE_ROWS, N)) if trajectories else None,
                                    Out(key("ns"), (2,), ctype=c_int64), Out(key("rcs"), (2,), ctype=c_int32)], result)
    assert isinstance(call[-1], ctypes.Array) and call[-1]._type_ is capi.KinStats and len(call[-1]) == 2
    assert (u is None) == (not trajectories) and len(stats) == 2 and stats[0]["n_steps"] == 0


def test_ensemble_keeps_its_signature(fake, h):
    """HipNetwork._ensemble(fn, params, K, *inputs, trajectories=): the entry's arguments between K and n_rows, as given."""
    pars = _params()
    t, u, ns, rcs, stats = h._ensemble(fake.kin_solve_ensemble_anything, pars, 3, 11, None, 13, trajectories=False)
    assert [a[2:6] for _, a in fake.calls] == [(3, 11, None, 13)] * 2 and u is None and t.shape == (SOLVE_ROWS,) and ns.shape == (3,)


# ---- refusals: the exception of today, and no call of the entry ------------------------------------------------------------------
def _refused(fake, exc, match, call, *entries):
    with pytest.raises(exc, match=match) as e:
        call()
    made = {n for n, _ in fake.calls}
    assert not made & set(entries), made
    return e.value


BATCHED = [("flux_batched", (), "kin_flux_batched"), ("drg_batched", (), "kin_drg_batched"), ("drgep_batched", ([0],), "kin_drgep_batched"),
           ("reaction_importance_batched", (), "kin_reaction_importance_batched"), ("pfa_batched", (), "kin_pfa_batched"),
           ("jac_batched", (), "kin_jac_batched"), ("timescale_batched", (), "kin_timescale_batched")]


@pytest.mark.parametrize("method, more, entry", BATCHED)
def test_refusals_of_the_batched_forms(fake, h, method, more, entry):
    f = getattr(h, method)
    _refused(fake, AssertionError, None, lambda: f(np.ones((2, N + 1)), *more), entry)           # u of the wrong width
    _refused(fake, AssertionError, None, lambda: f(U, *more, k=K_TABLE, k_row=[0, 1, 0]), entry)
    _refused(fake, AssertionError, None, lambda: f(U, *more, T=[300.0]), entry)
    _refused(fake, AssertionError, None, lambda: f(U, *more, k=np.ones((2, R + 1))), entry)


@pytest.mark.parametrize("form, nb", [("solution", SOL), ("ensemble", ENS)])
@pytest.mark.parametrize("p, more", [("flux", ()), ("drg", ()), ("drgep", ([0],)), ("reaction_importance", ()), ("pfa", ()), ("timescale", ())])
def test_refusals_of_the_stored_forms(fake, h, form, nb, p, more):
    f, entry = getattr(h, f"{form}_{p}"), f"kin_{form}_{p}"
    _refused(fake, AssertionError, None, lambda: f(*more, k=K_TABLE, k_row=np.zeros(nb + 1, int)), entry)
    _refused(fake, AssertionError, None, lambda: f(*more, T_rows=np.ones(nb - 1)), entry)


def test_refusals_of_weights_and_seeded_outputs(fake, h):
    _refused(fake, AssertionError, None, lambda: h.flux_batched(U, w=[1.0]), "kin_flux_batched")
    _refused(fake, AssertionError, None, lambda: h.solution_flux(w=np.ones(SOL + 1)), "kin_solution_flux")
    _refused(fake, AssertionError, None, lambda: h.ensemble_flux(w=np.ones(ENS_ROWS)), "kin_ensemble_flux")
    _refused(fake, AssertionError, None, lambda: h.flux_segmented(U3, w=np.ones(5)), "kin_flux_segmented")
    _refused(fake, AssertionError, None, lambda: h.flux_segmented(U3, seg_n=[3]), "kin_flux_segmented")
    _refused(fake, AssertionError, None, lambda: h.flux_segmented(U), "kin_flux_segmented")
    _refused(fake, AssertionError, None, lambda: h.ensemble_dot([1.0, 2.0]), "kin_ensemble_dot")
    for f, more, entry in ((h.drg_batched, (U,), "kin_drg_batched"), (h.solution_drg, (), "kin_solution_drg"), (h.ensemble_drg, (), "kin_ensemble_drg")):
        _refused(fake, AssertionError, None, lambda: f(*more, coef=np.ones(E + 1)), entry)
    for f, more, entry in ((h.pfa_batched, (U,), "kin_pfa_batched"), (h.solution_pfa, (), "kin_solution_pfa"), (h.ensemble_pfa, (), "kin_ensemble_pfa"),
                           (h.pfa_paths, (R_IN, R_IN), "kin_pfa_paths")):
        err = _refused(fake, capi.KineticaHipError, "coef has 7 entries, the PFA pattern 9 pairs", lambda: f(*more, coef=np.ones(E)), entry)
        assert err.code == capi.KIN_ERR_INVALID_ARG
    for f, more, entry in ((h.drgep_batched, (U, [0]), "kin_drgep_batched"), (h.drgep_paths, (R_IN, [0]), "kin_drgep_paths"),
                           (h.solution_drgep, ([0],), "kin_solution_drgep"), (h.ensemble_drgep, ([0],), "kin_ensemble_drgep")):
        _refused(fake, AssertionError, None, lambda: f(*more, importance=np.ones(N + 1)), entry)
    for f, more, entry in ((h.reaction_importance_batched, (U,), "kin_reaction_importance_batched"),
                           (h.solution_reaction_importance, (), "kin_solution_reaction_importance"),
                           (h.ensemble_reaction_importance, (), "kin_ensemble_reaction_importance")):
        _refused(fake, AssertionError, None, lambda: f(*more, importance=np.ones(N)), entry)
    for f, more, entry in ((h.timescale_batched, (U,), "kin_timescale_batched"), (h.solution_timescale, (), "kin_solution_timescale"),
                           (h.ensemble_timescale, (), "kin_ensemble_timescale")):
        _refused(fake, AssertionError, None, lambda: f(*more, summary=np.ones((2, N))), entry)
        _refused(fake, AssertionError, None, lambda: f(*more, summary=np.ones((N, 3))), entry)
    _refused(fake, AssertionError, None, lambda: h.pfa_paths(R_IN, R_IN[:1]), "kin_pfa_paths")


def test_refusals_of_the_statistics(fake, h):
    every = ("kin_members_moments", "kin_members_moments_dev", "kin_ensemble_moments", "kin_members_quantiles", "kin_members_quantiles_dev",
             "kin_ensemble_quantiles", "kin_members_correlate", "kin_members_correlate_dev", "kin_ensemble_correlate", "kin_members_sobol",
             "kin_members_sobol_dev", "kin_ensemble_sobol")
    block = r"u must be \[K\]\[L\]\[4\] \(member, row, species\); got \(3, 2, 5\)"
    wide = np.ones((3, 2, N + 1))
    for call in (lambda: h.members_moments(wide), lambda: h.members_quantiles(wide, PQ), lambda: h.members_correlate(wide, X3),
                 lambda: h.members_sobol(wide, 1, 1)):
        _refused(fake, ValueError, block, call, *every)
    _refused(fake, ValueError, r"u must be \[K\]\[L\]\[4\]", lambda: h.members_moments(U), *every)
    use = r"use must have one entry per member \(3\); got 2"
    for call in (lambda: h.members_moments(UM, use=[1, 1]), lambda: h.members_moments_dev(3, 2, 0x100, use=[1, 1], d_mean=0x200),
                 lambda: h.members_quantiles(UM, PQ, use=[1, 1]), lambda: h.members_quantiles_dev(3, 2, 0x100, PQ, 0x200, use=[1, 1]),
                 lambda: h.members_correlate(UM, X3, use=[1, 1]), lambda: h.members_correlate_dev(3, 2, 0x100, X3, 0x200, use=[1, 1])):
        _refused(fake, ValueError, use, call, *every)
    use = r"use must have one entry per member \(2\); got 3"
    for call in (lambda: h.ensemble_moments(use=USE3), lambda: h.ensemble_quantiles(PQ, use=USE3), lambda: h.ensemble_correlate(X2, use=USE3)):
        _refused(fake, ValueError, use, call, *every)
    names = r"unknown moments \['median'\]; choose among \('mean', 'var', 'min', 'max', 'count'\)"
    _refused(fake, ValueError, names, lambda: h.members_moments(UM, want=("mean", "median")), *every)
    _refused(fake, ValueError, names, lambda: h.ensemble_moments(want=("median",)), *every)
    rows = r"inputs must be \[K = 3\]\[P\] \(one row per member\); got \(2, 3\)"
    for call in (lambda: h.members_correlate(UM, X2), lambda: h.members_correlate_dev(3, 2, 0x100, X2, 0x200)):
        _refused(fake, ValueError, rows, call, *every)
    _refused(fake, ValueError, r"inputs must be \[K = 2\]\[P\] \(one row per member\); got \(3, 2\)", lambda: h.ensemble_correlate(X3), *every)
    _refused(fake, ValueError, r"inputs must be \[K = 3\]\[P\]", lambda: h.members_correlate(UM, np.ones(3)), *every)
    weights = r"w must be 2 integer multiplicities, one per base sample; got float64 \(2,\)"
    for call in (lambda: h.members_sobol(US, 2, 1, w=[1.0, 1.0]), lambda: h.members_sobol_dev(2, 1, 2, 0x100, d_first=0x200, w=[1.0, 1.0]),
                 lambda: h.ensemble_sobol(2, 1, w=np.array([1.0, 1.0]))):
        _refused(fake, ValueError, weights, call, *every)
    _refused(fake, ValueError, r"w must be 2 integer multiplicities, one per base sample; got int64 \(3,\)",
             lambda: h.members_sobol(US, 2, 1, w=[1, 1, 1]), *every)
    _refused(fake, ValueError, r"u must hold M \(P \+ 2\) = 8 members; got 6", lambda: h.members_sobol(US, 2, 2), *every)


@pytest.mark.parametrize("kind", ["continuous", "discrete"])
def test_refusals_of_the_ensemble_solves(fake, h, kind):
    f = getattr(h, "solve_ensemble_" + kind)
    u0 = np.ones((2, N))
    pairs = [([0.0, 1.0], [300.0, 400.0])] * 2
    Ea = np.ones((2, R))
    both = "per-member Arrhenius parameters: give both Ea and A, or neither"
    _refused(fake, ValueError, both, lambda: f(_params(), u0, pairs, Ea=Ea))
    _refused(fake, ValueError, both, lambda: f(_params(), u0, pairs, A=Ea))
    _refused(fake, ValueError, r"per-member A must be \[K\]\[R\] = \(2, 3\), got \(3,\)", lambda: f(_params(), u0, pairs, Ea=Ea, A=np.ones(R)))
    _refused(fake, ValueError, "per-member Ea must be real numbers, got dtype complex128", lambda: f(_params(), u0, pairs, Ea=Ea * 1j, A=Ea))
    _refused(fake, AssertionError, None, lambda: f(_params(), np.ones((2, N + 1)), pairs))
    _refused(fake, AssertionError, None, lambda: f(_params(), u0, pairs[:1]))
    _refused(fake, AssertionError, None, lambda: f(_params(), u0, [([0.0, 1.0], [300.0])] * 2))
    assert fake.calls == []


# ---- the argtypes of the real library -----------------------------------------------------------------------------------------
def test_every_symbol_has_argtypes():
    """After lib() has loaded the library the build step made, every entry that takes arguments has them declared."""
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = capi.lib()
    missing = [name for name in capi.SYMBOLS if name not in ("kin_abi_version", "kin_version") and getattr(L, name).argtypes is None]
    assert missing == []
