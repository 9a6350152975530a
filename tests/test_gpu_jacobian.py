"""GPU tests of the right-hand side, the Jacobian and the Newton residual in every kernel that forms them, entry by entry against
the extended-precision reference of tests/jac_cases.py (built from the reaction lists, never from the compiled tables) with the
bounds derived there - (L + 3) u S per Jacobian entry, (L + 4) u S per RHS component, (L + 6) u scale per residual component,
u = 2^-53, L the entry's term count, S the sum of its absolute terms - and BIT FOR BIT on the exact inputs (u in {1/2, 1, 2},
integer k in 1 .. 8), where a missing, doubled or misplaced term shows whatever its size. Nothing is judged by a maximum over
the matrix. tests/test_jac_cases.py checks the references, the bounds and the cases' plan classes on machines without a GPU.

Routes: kin_jac_pattern / kin_jac_values / kin_rhs; kin_eval_probe path 0 (rates_kernel, drates_kernel, rates_skip_kernel and
segsum_kernel with SEG_COEF_SET and SEG_COEF_BDF through the handle's rhs_plan / jac_plan and the Solver's resid_plan; with a
pending temperature rates_T_kernel, drates_T_kernel, rates_skip_T_kernel); path 2 (e_rates_kernel in its three source modes,
e_drates_kernel, e_segsum_kernel with SEL 0, 1, 2 through ens_rhs, ens_jac, ens_resid); kin_resident_probe (du, jac) for the
networks the resident kernel takes; kin_rhs_block_dev on torch buffers. Every test asserts from the probe's info that the plan it
ran is the one the reference's row lengths predict and the class the case is named after.

Path 2 runs every case with K = 1, 3 and 64 members in one launch (the five state kinds in turn, so each kind has its RHS in
the three modes, its Jacobian and an un-skipped residual judged in every case); above SAMPLE_ABOVE species a sample of the 64
members that holds every kind is judged and compared with its own K = 1 launch, below every member named.

The largest error / bound ratio per route is printed at the end of the module (pytest -s). Measured on an MI355X:
  kin_rhs 0.374, kin_jac_values 0.429; path 0: rhs 0.374, jac 0.429, resid 0.420; path 0 with a pending temperature: rhs 0.400,
  jac 0.481, resid 0.497; path 2: rhs 0.374 in each of the three modes, jac 0.431, resid 0.420; resident du 0.355, jac 0.429;
  rhs_block_dev 0.374. (A float64 sum of the same terms in reversed order on the CPU: 0.374, 0.397, 0.502.)

Mutation check (value-only changes on a scratch build, one at a time, nothing of it kept): which tests of this file fail, and
what the suite before this file did (run to its first failure).
  1 seg_store<SEG_COEF_SET> writes 0 where |acc| < 1e-10: 235 of the 275 tests fail - pattern_values_and_rhs,
    single_state_kernels, pending_temperature_kernels, both lockstep tests, resident_kernel and rhs_block_dev on every case whose
    log-uniform states have a value that small (28 .. 39 of the 39 cases each).
    Before: the first failure came after 297 tests, test_vanished_pivot_in_the_dense_block[single-48-5] of the Newton module (a
    side effect on a pivot; the normwise comparisons of test_gpu_parity and test_gpu_resident_linalg were not reached).
  2 a medium row of exactly 256 entries drops its last entry in seg_traverse: 6 fail - hub_256_wave in
    pattern_values_and_rhs, single_state_kernels, pending_temperature_kernels, both lockstep tests and rhs_block_dev (the resident
    kernel walks its rows itself and passes).
    Before: first failure test_c5_two_chunk_solve_against_truth, a trajectory against a stored truth.
  3 e_segsum_kernel with SEL == 1 reads member 0's dr: 78 fail - every case of both lockstep tests (a member's K = 1
    launch passes inside them; in a launch of several, every member but member 0 differs).
    Before: first failure test_thread_and_lockstep_routes[lockstep] of the ensemble analysis, after 139 tests.
  4 rates_skip_kernel ignores the flag: 39 fail - every single_state_kernels case (the rate buffer of a skipped launch
    lost the sentinel).
    Before: MISSED - all 996 GPU tests of the previous suite passed.
  5 seg_store<SEG_COEF_BDF> subtracts psi twice and d not at all: 157 fail - every single_state_kernels,
    pending_temperature_kernels and lockstep case, and a_solve_after_the_probes (the solve fails).
    Before: the second test that ran, test_dtmin_ends_in_dtlessthanmin_and_the_retry_loop_answers (every implicit solve breaks).
  6 drates_T_kernel stores k but differentiates with the old k: 39 fail - every pending_temperature_kernels case.
    Before: first failure test_return_integrator_with_continuous_rates_and_the_explicit_guard, the fifth test that ran (an
    integrator's state after steps under a temperature profile).
  So the previous suite missed mutation 4 outright; it noticed 1, 2, 3 and 6 only through a pivot flag, a stored trajectory or an
  ensemble comparison far from the cause, never through a comparison of the values themselves."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import synthetic_crn
from oracle import oracle as orc
from tests import jac_cases as jc
from tests.jac_cases import LD, SENTINEL

pytestmark = pytest.mark.gpu

ALL = list(jc.CASES)
SAMPLE_ABOVE = 400
MEASURED = {}
_H, _REF = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nrhs / jacobian / residual: largest error / bound per route (exact inputs are compared bit for bit)")
        for route, v in sorted(MEASURED.items()):
            print(f"  {route:34s} {v:.3f}")
    for h in _H.values():
        h.close()
    _H.clear()


def handle(name):
    if name not in _H:
        _H[name] = capi.HipNetwork.from_flat(jc.case(name)[0])
    return _H[name]


def refs(name, kind, member=0):
    """(u, k, rhs (value, S, L), jac (value, S, L)) of a state, computed once"""
    key = (name, kind, member)
    if key not in _REF:
        ref = jc.case(name)[1]
        u, k = jc.state(name, kind, member)
        _REF[key] = (u, k, ref.rhs(k, u), ref.jac(k, u))
    return _REF[key]


def judge(route, dev, val, bound, exact, what):
    """entry by entry inside the bound; on the exact inputs bit for bit"""
    if exact:
        bad = np.nonzero(np.asarray(dev).astype(LD) != val)[0]
        assert len(bad) == 0, (route, what, "not bit for bit", int(bad[0]), float(np.asarray(dev)[bad[0]]), float(val[bad[0]]), len(bad))
        return
    ok, ratio = jc.compare(dev, val, bound)
    MEASURED[route] = max(MEASURED.get(route, 0.0), ratio)
    assert ok, (route, what, jc.worst(dev, val, bound))


def judge_rhs(route, dev, r, exact, what):
    judge(route, dev, r[0], jc.bound_rhs(r[1], r[2]), exact, what)


def judge_jac(route, dev, r, exact, what):
    judge(route, dev, r[0], jc.bound_jac(r[1], r[2]), exact, what)


def judge_resid(route, out, ref, k, u, c, psi, d, exact, what):
    """the window of the solve vectors: the residual at yloc, the sentinel everywhere else"""
    vec, yloc = out["out"], out["yloc"]
    g, scale, L = ref.resid(k, u, c, psi, d)
    judge(route, vec[yloc], g, jc.bound_resid(scale, L), exact, what)
    rest = np.ones(len(vec), bool); rest[yloc] = False
    assert np.all(vec[rest] == SENTINEL), (route, what, "a position outside yloc was written")


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------- kin_jac_pattern / kin_jac_values / kin_rhs
@pytest.mark.parametrize("name", ALL)
def test_pattern_values_and_rhs(name):
    net, ref = jc.case(name)
    h = handle(name)
    rowptr, col = h.jac_pattern()
    assert np.array_equal(rowptr, ref.rowptr) and np.array_equal(col, ref.cols)
    for kind in jc.STATE_KINDS:
        u, k, r, J = refs(name, kind)
        h.set_rates(k)
        judge_rhs("kin_rhs", h.rhs(u), r, kind == "exact", (name, kind))
        judge_jac("kin_jac_values", h.jac_values(u), J, kind == "exact", (name, kind))


# ------------------------------------------------------------------------------------------------------ kin_eval_probe, path 0
@pytest.mark.parametrize("name", ALL)
def test_single_state_kernels(name):
    net, ref = jc.case(name)
    h = handle(name)
    for kind in jc.STATE_KINDS:
        u, k, r, J = refs(name, kind)
        exact = kind == "exact"
        h.set_rates(k)
        o = h.eval_probe(0, "rhs", u)
        jc.check_class(name, "rhs", o["info"])
        judge_rhs("path 0 rhs", o["out"][0], r, exact, (name, kind))
        o = h.eval_probe(0, "jac", u)
        jc.check_class(name, "jac", o["info"])
        judge_jac("path 0 jac", o["out"][0], J, exact, (name, kind))
        c, psi, d = jc.resid_inputs(name, kind)
        o = h.eval_probe(0, "resid", u, c=c, psi=psi, d=d, done=0)
        jc.check_class(name, "rhs", o["info"])
        assert sorted(o["yloc"]) == sorted(set(o["yloc"])) and len(o["out"][0]) == o["info"]["vec_len"] >= ref.N
        judge_resid("path 0 resid", dict(out=o["out"][0], yloc=o["yloc"]), ref, k, u, c, psi, d, exact, (name, kind))
        assert np.array_equal(o["rate"][0].astype(LD), ref.rates(k, u)) if exact else np.all(o["rate"][0] != SENTINEL)
        o = h.eval_probe(0, "resid", u, c=c, psi=psi, d=d, done=1)
        assert np.all(o["out"][0] == SENTINEL) and np.all(o["rate"][0] == SENTINEL), (name, kind, "a skipped launch wrote")


def arrhenius_params(name):
    net, ref = jc.case(name)
    if name == "synthetic_300":
        return synthetic_crn(300, 1500)[1:]
    if name == "synthetic_1000":
        return synthetic_crn(1000, 5000)[1:]
    rng = np.random.default_rng(len(name) + ref.R)
    Ea = np.where(rng.random(ref.R) < 0.25, 0.0, rng.uniform(0.0, 6e5, ref.R))
    return Ea, 10.0 ** rng.uniform(8.8, 12.3, ref.R)


@pytest.mark.parametrize("name", ALL)
def test_pending_temperature_kernels(name):
    """the kernels that form k from a pending temperature on the spot: k is poisoned before every launch, so what comes back from
    kin_get_rates is what the kernel stored; the values are judged against the reference evaluated with that stored k"""
    net, ref = jc.case(name)
    h = handle(name)
    Ea, A = arrhenius_params(name)
    poison = np.full(ref.R, 7.0)
    for kind in (q for q in jc.STATE_KINDS if q != "exact"):          # (k comes from the Arrhenius law: no exact inputs here)
        u = jc.state(name, kind)[0]
        c, psi, d = jc.resid_inputs(name, kind)
        for T, k_max in ((500.0, None), (500.0, 1e12), (1500.0, None), (1500.0, 1e12)):
            h.set_arrhenius(Ea, A, k_max=k_max)
            want = orc.arrhenius(Ea, A, T, k_max=k_max)
            what = (name, kind, T, k_max)

            def stored():
                k = h.get_rates()
                np.testing.assert_allclose(k, want, rtol=2e-15, atol=0)
                return k
            h.set_rates(poison)
            o = h.eval_probe(0, "rhs", u, T=T)
            k = stored()
            judge_rhs("path 0 rhs at T", o["out"][0], ref.rhs(k, u), False, what)
            h.set_rates(poison)
            o = h.eval_probe(0, "jac", u, T=T)
            k = stored()
            judge_jac("path 0 jac at T", o["out"][0], ref.jac(k, u), False, what)
            h.set_rates(poison)
            o = h.eval_probe(0, "resid", u, T=T, c=c, psi=psi, d=d, done=0)
            k = stored()
            judge_resid("path 0 resid at T", dict(out=o["out"][0], yloc=o["yloc"]), ref, k, u, c, psi, d, False, what)
            h.set_rates(poison)
            o = h.eval_probe(0, "resid", u, T=T, c=c, psi=psi, d=d, done=1)
            stored()                                        # k is stored whether or not the iteration is skipped
            assert np.all(o["out"][0] == SENTINEL) and np.all(o["rate"][0] == SENTINEL), (what, "a skipped launch wrote")


# ------------------------------------------------------------------------------------------------------ kin_eval_probe, path 2
def members_of(name, K):
    """K members with states and rate constants of their own: the state kinds in turn"""
    kinds = [jc.STATE_KINDS[m % len(jc.STATE_KINDS)] for m in range(K)]
    sts = [jc.state(name, kinds[m], member=m // len(jc.STATE_KINDS)) for m in range(K)]
    return kinds, np.array([s[0] for s in sts]), np.array([s[1] for s in sts])


def lockstep_case(name, K, entries, judged, done):
    """one launch of every operation with `entries` of the K members; the members of `judged` against the reference and
    against their own K = 1 launch, the members not named against the fill patterns"""
    net, ref = jc.case(name)
    h = handle(name)
    N, R = ref.N, ref.R
    kinds, U, Kk = members_of(name, K)
    left_out = sorted(set(range(K)) - set(entries))
    rin = [jc.resid_inputs(name, kinds[m], member=m) for m in range(K)]
    C = np.array([r[0] for r in rin]); PSI = np.array([r[1] for r in rin]); D = np.array([r[2] for r in rin])
    done = np.asarray(done, np.int32)
    nan_n, nan_2n, nan_j = np.full(N, np.nan), np.full(2 * N, np.nan), np.full(ref.nnz, np.nan)

    def solo(m, op, **kw):
        """member m's own K = 1 launch"""
        return h.eval_probe(2, op, U[m], k=Kk[m], **kw)

    rhs_ref = {m: ref.rhs(Kk[m], U[m]) for m in judged}
    for mode in (0, 1, 2):
        o = h.eval_probe(2, "rhs", U, k=Kk, members=entries, mode=mode)
        jc.check_class(name, "rhs", o["info"])
        w, other = (slice(N, 2 * N), slice(0, N)) if mode == 1 else (slice(0, N), slice(N, 2 * N))
        for m in left_out:
            assert same_bits(o["out"][m], nan_2n) and np.all(o["rate"][m] == SENTINEL), (name, K, mode, m)
        for m in judged:
            judge_rhs(f"path 2 rhs mode {mode}", o["out"][m, w], rhs_ref[m], kinds[m] == "exact", (name, K, m))
            assert same_bits(o["out"][m, other], nan_n), (name, K, mode, m, "the other output was written")
            if K > 1:
                s1 = solo(m, "rhs", mode=mode)
                assert same_bits(o["out"][m], s1["out"][0]) and same_bits(o["rate"][m], s1["rate"][0]), (name, K, mode, m)
    o = h.eval_probe(2, "jac", U, k=Kk, members=entries)
    jc.check_class(name, "jac", o["info"])
    for m in left_out:        # values and operand derivatives of a member not named: the fill patterns, bit for bit
        assert same_bits(o["out"][m], nan_j) and np.all(o["rate"][m] == SENTINEL) and o["rate"][m].shape == (2 * R,), (name, K, m)
    for m in judged:
        judge_jac("path 2 jac", o["out"][m], ref.jac(Kk[m], U[m]), kinds[m] == "exact", (name, K, m))
        if kinds[m] == "exact":
            assert np.array_equal(o["rate"][m].reshape(R, 2).astype(LD), ref.drates(Kk[m], U[m])), (name, K, m, "operand derivatives")
        if K > 1:
            s1 = solo(m, "jac")
            assert same_bits(o["out"][m], s1["out"][0]) and same_bits(o["rate"][m], s1["rate"][0]), (name, K, m)
    o = h.eval_probe(2, "resid", U, k=Kk, members=entries, c=C, psi=PSI, d=D, done=done)
    jc.check_class(name, "rhs", o["info"])
    for m in range(K):
        if m in left_out or done[m]:
            assert np.all(o["out"][m] == SENTINEL) and np.all(o["rate"][m] == SENTINEL), (name, K, m, "a skipped or absent member was written")
    for m in judged:
        if not done[m]:
            judge_resid("path 2 resid", dict(out=o["out"][m], yloc=o["yloc"]), ref, Kk[m], U[m], C[m], PSI[m], D[m], kinds[m] == "exact",
                        (name, K, m))
        if K > 1:
            s1 = solo(m, "resid", c=C[m], psi=PSI[m], d=D[m], done=done[m])
            assert same_bits(o["out"][m], s1["out"][0]) and same_bits(o["rate"][m], s1["rate"][0]), (name, K, m)


@pytest.mark.parametrize("name", ALL)
def test_lockstep_kernels_one_and_three_members(name):
    lockstep_case(name, 1, [0], [0], [0])
    # fewer entries than members, permuted: member 1 is not named
    lockstep_case(name, 3, [2, 0], [0, 2], [0, 0, 0])


# K = 64: the kinds in turn (member m has kind m % 5), members 6 and 41 not named, the skip flag set for every seventh member from 5
# on; the sample judged on the large networks holds every kind without the flag (0 .. 4), a member with it (33) and both ends
K64_LEFT_OUT = (6, 41)
K64_DONE = [1 if m % 7 == 5 else 0 for m in range(64)]
K64_SAMPLE = [0, 1, 2, 3, 4, 33, 62, 63]


@pytest.mark.parametrize("name", ALL)
def test_lockstep_kernels_sixty_four_members(name):
    N = jc.case(name)[1].N
    entries = [m for m in reversed(range(64)) if m not in K64_LEFT_OUT]
    judged = sorted(entries) if N <= SAMPLE_ABOVE else K64_SAMPLE
    assert {m % 5 for m in judged if not K64_DONE[m]} == set(range(5)) and any(K64_DONE[m] for m in judged)
    lockstep_case(name, 64, entries, judged, K64_DONE)


# -------------------------------------------------------------------------------------------------------- kin_resident_probe
# the networks beyond the resident kernel's capacity (their state, rates and solve vectors do not fit one compute unit's LDS):
# it must refuse exactly these, every other case is judged
RESIDENT_REFUSES = ("hub_12288_block1", "hub_12289_block2", "hub_24577_block3")


@pytest.mark.parametrize("name", [q for q in ALL if q not in RESIDENT_REFUSES])
def test_resident_kernel(name):
    net, ref = jc.case(name)
    h = handle(name)
    rng = np.random.default_rng(3)
    for kind in jc.STATE_KINDS:
        u, k, r, J = refs(name, kind)
        h.set_rates(k)
        out = h.resident_probe(u, 2.0 ** -10, rng.standard_normal(ref.N))
        judge_rhs("resident du", out["du"][0], r, kind == "exact", (name, kind))
        judge_jac("resident jac", out["jac"][0], J, kind == "exact", (name, kind))


@pytest.mark.parametrize("name", RESIDENT_REFUSES)
def test_resident_kernel_refuses_what_it_cannot_hold(name):
    net, ref = jc.case(name)
    h = handle(name)
    u, k, r, J = refs(name, "exact")
    h.set_rates(k)
    with pytest.raises(capi.KineticaHipError) as e:
        h.resident_probe(u, 2.0 ** -10, np.ones(ref.N))
    assert e.value.code == capi.KIN_ERR_UNSUPPORTED


# --------------------------------------------------------------------------------------------------------- kin_rhs_block_dev
@pytest.mark.parametrize("name", ALL)
def test_rhs_block_dev(name):
    import torch
    net, ref = jc.case(name)
    h = handle(name)
    R, N = ref.R, ref.N
    cuts = [0, R // 3 + (1 if R > 4 else 0), (2 * R) // 3, R]
    d_du = torch.empty(N, dtype=torch.float64, device="cuda:0")
    for kind in jc.STATE_KINDS:
        u, k, r, J = refs(name, kind)
        exact = kind == "exact"
        h.set_rates(k)
        d_u = torch.tensor(u, dtype=torch.float64, device="cuda:0")

        def block(lo, hi):
            d_du.fill_(float("nan"))
            torch.cuda.synchronize()          # torch's fill runs on torch's stream, the library on the handle's own
            h.rhs_block_dev(lo, hi, d_u.data_ptr(), d_du.data_ptr())
            h.get_rates()                     # (synchronises the handle's stream)
            torch.cuda.synchronize()
            return d_du.cpu().numpy().copy()
        empty = block(0, 0)
        assert np.all(empty == 0.0) and not np.any(np.signbit(empty)), (name, kind, "the empty block")
        judge_rhs("rhs_block_dev", block(0, R), r, exact, (name, kind, "whole"))
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            parts.append(block(lo, hi))
            judge_rhs("rhs_block_dev", parts[-1], ref.rhs(k, u, lo, hi), exact, (name, kind, lo, hi))
            if kind == "zeros":
                assert np.all(parts[-1] == 0.0), (name, lo, hi, "a block of the all-zero state was not written as 0.0")
        if exact:
            assert np.array_equal((parts[0] + parts[1] + parts[2]).astype(LD), r[0]), (name, "the three parts do not sum to the RHS")
    for lo, hi in ((-1, R), (0, R + 1), (2, 1) if R >= 2 else (1, 0)):
        with pytest.raises(capi.KineticaHipError) as e:
            h.rhs_block_dev(lo, hi, d_u.data_ptr(), d_du.data_ptr())
        assert e.value.code == capi.KIN_ERR_INVALID_ARG


# -------------------------------------------------------------------------------------------------------- argument checks
def test_probe_argument_checks():
    name = "triple_product"
    net, ref = jc.case(name)
    h = handle(name)
    u, k = jc.state(name, "exact")
    h.set_rates(k)

    def code(fn):
        with pytest.raises(capi.KineticaHipError) as e:
            fn()
        return e.value.code
    assert code(lambda: h.eval_probe(1, "rhs", u)) == capi.KIN_ERR_INVALID_ARG                       # no such path
    assert code(lambda: h.eval_probe(0, "rhs", u, k=k)) == capi.KIN_ERR_INVALID_ARG                  # k on path 0
    assert code(lambda: h.eval_probe(2, "rhs", u)) == capi.KIN_ERR_INVALID_ARG                       # no k on path 2
    assert code(lambda: h.eval_probe(2, "rhs", u, k=k, mode=3)) == capi.KIN_ERR_INVALID_ARG
    assert code(lambda: h.eval_probe(0, "rhs", u, mode=1)) == capi.KIN_ERR_INVALID_ARG
    assert code(lambda: h.eval_probe(2, "rhs", u, k=k, T=500.0)) == capi.KIN_ERR_INVALID_ARG
    assert code(lambda: h.eval_probe(0, "rhs", u, T=-1.0)) == capi.KIN_ERR_INVALID_ARG
    U3, K3 = np.tile(u, (3, 1)), np.tile(k, (3, 1))
    assert code(lambda: h.eval_probe(2, "jac", U3, k=K3, members=[0, 0])) == capi.KIN_ERR_INVALID_ARG
    assert code(lambda: h.eval_probe(2, "jac", U3, k=K3, members=[0, 3])) == capi.KIN_ERR_INVALID_ARG
    assert code(lambda: h.eval_probe(2, "jac", U3, k=K3, members=[0, 1, 2, 1])) == capi.KIN_ERR_INVALID_ARG
    assert code(lambda: h.eval_probe(0, "jac", U3)) == capi.KIN_ERR_INVALID_ARG                      # path 0 takes one member
    h2 = capi.HipNetwork.from_flat(net)
    try:
        assert code(lambda: h2.eval_probe(0, "rhs", u)) == capi.KIN_ERR_STATE                         # no rates
        h2.set_rates(k)
        assert code(lambda: h2.eval_probe(0, "rhs", u, T=500.0)) == capi.KIN_ERR_STATE                # no Arrhenius parameters
    finally:
        h2.close()
    # the handle is as usable as before
    judge_rhs("path 0 rhs", h.eval_probe(0, "rhs", u)["out"][0], ref.rhs(k, u), True, (name, "after the refusals"))


def test_a_solve_after_the_probes_is_that_of_a_fresh_handle(monkeypatch):
    """path 0's residual borrows the Solver's slot 0, its step vectors and its control block, path 2 builds the ensemble's
    analysis: a host-driven solve afterwards is bit for bit the solve of a handle that was never probed"""
    monkeypatch.setenv("KIN_RESIDENT", "0")
    name = "special_stoichiometries_60"
    net, ref = jc.case(name)
    u = jc.state(name, "loguniform")[0]
    k = 10.0 ** np.random.default_rng(5).uniform(0, 4, ref.R)
    c, psi, d = jc.resid_inputs(name, "loguniform")
    pars = capi.KinParams(tspan0=0.0, tspan1=1e-3, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1,
                          ban_negatives=0, solve_chunkstep=1e-3, maxiters=20000, save_interval=-1.0)
    runs = []
    for probed in (True, False):
        h = capi.HipNetwork.from_flat(net)
        try:
            h.set_rates(k)
            if probed:
                for done in (0, 1):
                    h.eval_probe(0, "resid", u, c=c, psi=psi, d=d, done=done)
                    h.eval_probe(2, "resid", u, k=k, c=c, psi=psi, d=d, done=done)
                h.eval_probe(0, "jac", u)
            t, us, rc, st, status = h.solve(pars, u)
            st.pop("wall_seconds", None)
            runs.append((t, us, rc, st, status))
        finally:
            h.close()
    (t1, u1, rc1, st1, s1), (t2, u2, rc2, st2, s2) = runs
    assert rc1 == rc2 == 0 and s1 == s2 and st1 == st2
    assert np.array_equal(t1, t2) and np.array_equal(u1, u2)
