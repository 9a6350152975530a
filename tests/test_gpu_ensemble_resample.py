"""GPU tests of resampling over stored trajectories: kin_ensemble_resample reads the members' saved states where the last
kin_solve_ensemble* call left them and, with store, puts its result in their place; kin_solution_resample reads those of the
last kin_solve; solving.resample_ensemble and solve_network_ensemble(resample=...) on top.

The ensemble is the one of test_gpu_ensemble_event_times.py's last test: synthetic_crn(300, 1500), four members on ramps from
900 K to 1300 K at 1e5 .. 4e5 K/s, 2 ms, a row every 2.5e-4 s. After 2 ms the slowest member is at 1100 K, the fastest two sit on
the 1300 K plateau. Axis: the temperature; queries 900 : 50 : 1300."""
import math

import numpy as np
import pytest

import event_cases as ec
import resample_cases as rc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import synthetic_crn
from test_gpu_ensemble_analysis import kp

pytestmark = pytest.mark.gpu
N = 300
RATES = [1e5 * (1.0 + 3.0 * f) for f in (0.0, 0.3, 0.7, 1.0)]
K = len(RATES)
AT = np.arange(900.0, 1300.0 + 1.0, 50.0)
T1, SAVE = 2e-3, 2.5e-4


def _nodes(rate):
    """(t, T) of a ramp from 900 K at `rate` that holds at 1300 K, over [0, T1]."""
    te = 400.0 / rate
    if te < T1:
        return np.array([0.0, te, T1]), np.array([900.0, 1300.0, 1300.0])
    return np.array([0.0, T1]), np.array([900.0, round(900.0 + rate * T1, 6)])


def _solve(h, trajectories):
    U0 = np.zeros((K, N)); U0[:, 0] = 1.0
    return h.solve_ensemble_continuous(kp(T1, save=SAVE), U0, [_nodes(r) for r in RATES], trajectories=trajectories)


@pytest.fixture(scope="module")
def stored():
    """A handle that holds the ensemble, the download of it, every member's temperature at the saved times and the restatement."""
    net, Ea, A = synthetic_crn(N, 5 * N)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    t, u, ns, rcs, _ = _solve(h, True)
    assert u.shape == (K, 9, N) and np.all(rcs == 0) and np.all(ns == 9)
    T = np.array([np.interp(t, *_nodes(r)) for r in RATES])
    assert T[0, -1] == 1100.0 and T[-1, -1] == 1300.0 and T[-1, -2] == 1300.0
    ref = rc.ref_resample(u, T, AT, seg_n=ns)
    yield dict(h=h, t=t, u=u, ns=ns, T=T, ref=ref)
    h.close()


def _restore(d):
    """The solve again: the stored ensemble is the solve's own once more."""
    t, u, ns, _, _ = _solve(d["h"], True)
    assert u.tobytes() == d["u"].tobytes() and np.array_equal(ns, d["ns"])


def test_stored_entry_host_entry_and_restatement_agree(stored):
    h, u, T, ns = stored["h"], stored["u"], stored["T"], stored["ns"]
    for kw in (dict(), dict(mode="hold", fill=-1.0), dict(row_begin=2), dict(mode="hold", row_begin=3)):
        got = h.ensemble_resample(T, AT, **kw)
        host = h.resample_segmented(u, T, AT, seg_n=ns, **kw)
        ref = rc.ref_resample(u, T, AT, seg_n=ns, **kw)[0]
        assert got.shape == (K, len(AT), N) and ec.same_bits(got, host) and ec.same_bits(got, ref), kw
    per = h.ensemble_resample(T, np.tile(AT, (K, 1)))
    assert ec.same_bits(per, stored["ref"][0])
    assert h.ensemble_size()[1] == 9                                       # nothing was stored
    # the save grid itself as axis and queries: the download's bytes
    assert h.ensemble_resample(stored["t"], stored["t"]).tobytes() == u.tobytes()
    rs = S.resample_ensemble(h, stored["t"], stored["t"], axis="t", store=False, download=True)
    assert rs.u.tobytes() == u.tobytes() and rs.covered.all() and rs.n_covered.tolist() == [9] * K
    rel = S.resample_ensemble(h, stored["t"], [0.0, 0.5, 1.0], axis="t_rel", store=False)
    assert ec.same_bits(rel.u, rc.ref_resample(u, stored["t"] / stored["t"][-1], [0.0, 0.5, 1.0])[0])
    assert rel.u[:, 0].tobytes() == u[:, 0].tobytes() and rel.u[:, 2].tobytes() == u[:, 8].tobytes() and rel.jc[:, 2].tolist() == [8] * K


def test_a_stored_result_is_the_record_every_ensemble_pass_reads(stored):
    h, T, ns = stored["h"], stored["T"], stored["ns"]
    ref, jc, _ = stored["ref"]
    run = rc.covered_run(jc, "fill")
    assert run.tolist() == [5, 8, 9, 9]                                    # 1100 K, 1280 K, and two members on the plateau
    try:
        assert h.ensemble_resample(T, AT, store=True, download=False) is None
        Kk, rows, n, ns2 = h.ensemble_size()
        assert (Kk, rows, n) == (K, len(AT), N) and np.array_equal(ns2, run)
        block = ref.copy()
        for m in range(K):
            block[m, run[m]:] = 0.0                                        # the record's invariant: zeros past a member's rows
        # the save grid of the new record is AT: the same record resampled at its own axis gives its rows, zeros included
        assert h.ensemble_resample(AT, AT, mode="hold").tobytes() == rc.ref_resample(block, AT, AT, seg_n=run, mode="hold")[0].tobytes()
        assert h.ensemble_max().tobytes() == np.array([block[m, :run[m]].max(axis=0) for m in range(K)]).tobytes()
        mom = h.ensemble_moments()
        assert mom["count"] == int((run == len(AT)).sum()) == 2
        full = h.members_moments(block, use=run == len(AT))
        assert all(ec.same_bits(mom[q], full[q]) for q in ("mean", "var", "min", "max"))
        ev_kw = dict(level=0.5, kind="of_start", direction="fall")
        ev, ev_ref = h.ensemble_events(AT, **ev_kw), h.events_segmented(block, AT, seg_n=run, **ev_kw)
        assert all(ec.same_bits(ev[q], ev_ref[q]) for q in ec.OUTPUTS)
        assert all(ec.same_bits(ev[q], ec.ref_events(block, AT, seg_n=run, **ev_kw)[q]) for q in ec.OUTPUTS)
        # a second resample, of the resampled record: the restatement applied twice
        at2 = np.array([925.0, 1000.0, 1290.0, 1100.0])
        twice = rc.ref_resample(block, AT, at2, seg_n=run)
        got = h.ensemble_resample(AT, at2, store=True)
        assert ec.same_bits(got, twice[0]) and h.ensemble_size()[1] == 4
        run2 = rc.covered_run(twice[1], "fill")
        assert np.array_equal(h.ensemble_size()[3], run2) and run2.tolist() == [2, 2, 4, 4]
        block2 = twice[0].copy()
        for m in range(K):
            block2[m, run2[m]:] = 0.0
        assert h.ensemble_max().tobytes() == np.array([block2[m, :run2[m]].max(axis=0) for m in range(K)]).tobytes()
        third = h.ensemble_resample(np.arange(4.0), np.array([0.0, 1.0]), store=True)      # and back into the first of the two buffers
        assert third.tobytes() == block2[:, :2].tobytes()
    finally:
        _restore(stored)
    assert h.ensemble_size()[1] == 9 and ec.same_bits(h.ensemble_resample(T, AT), ref)      # the next solve replaces the record


def _stored_block(ref, run):
    """What a stored result has to be: the restatement, zeros from each member's first uncovered query on."""
    block = ref.copy()
    for m in range(K):
        block[m, run[m]:] = 0.0
    return block


def test_the_zero_tail_of_a_stored_result_byte_for_byte(stored):
    """resample_zero_tail_kernel over the record as it lies on the device (res_host.stored_record: no entry of the library reads
    the rows past a member's n_saved): every member's tail short (the fixture's queries), every member's whole block (a first
    query below every range: n_saved' = 0) and 450 queries - Q N = 135 000 entries, more than 64 x 2048: the cap of 64
    workgroup rows and a second grid-stride trip."""
    from tests import res_host
    h, T, ns, u = stored["h"], stored["T"], stored["ns"], stored["u"]
    assert res_host.stored_record(h).tobytes() == u.tobytes()                  # the solve's own record, as downloaded
    many = np.linspace(900.0, 1300.0, 450)
    assert len(many) * N > 64 * 256 * 8
    try:
        for at, expect in ((AT, [5, 8, 9, 9]), (np.concatenate([[850.0], AT]), [0, 0, 0, 0]), (many, None)):
            _restore(stored)
            ref, jc, _ = rc.ref_resample(u, T, at, seg_n=ns)
            run = rc.covered_run(jc, "fill")
            assert expect is None or run.tolist() == expect
            assert h.ensemble_resample(T, at, store=True, download=False) is None
            Kk, rows, n, ns2 = h.ensemble_size()
            assert (Kk, rows, n) == (K, len(at), N) and np.array_equal(ns2, run), (len(at), ns2, run)
            got, block = res_host.stored_record(h), _stored_block(ref, run)
            assert got.tobytes() == block.tobytes(), (len(at), np.argwhere(got.view(np.int64) != block.view(np.int64))[:5])
        assert 0 < run[0] < run[1] < len(many) and run[2] == len(many)           # (of the 450: tails of two lengths, and none)
        assert not got[0, run[0]:].any() and got[0, :run[0]].any()
    finally:
        _restore(stored)
    assert h.ensemble_size()[1] == 9


def test_resample_before_any_ensemble_solve_is_a_state_error():
    net, Ea, A = synthetic_crn(20, 60)
    h = capi.HipNetwork.from_flat(net)
    for kw in (dict(), dict(store=True, download=False)):
        with pytest.raises(capi.KineticaHipError) as e:
            h.ensemble_resample(np.arange(3.0), np.arange(2.0), **kw)
        assert e.value.code == capi.KIN_ERR_STATE
    h.close()


def test_solve_network_ensemble_resamples_before_the_statistics():
    from kinetica_jl_amd import conditions as C
    net, Ea, A = synthetic_crn(N, 5 * N)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(N)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    methods = []
    for rate in RATES:
        u0 = np.zeros(N); u0[0] = 1.0
        pars = S.ODESimulationParams(tspan=(0.0, T1), u0=u0, save_interval=SAVE, low_k_cutoff="none")
        methods.append(S.VariableODESolve(pars, C.ConditionSet({"T": C.LinearGradientProfile(rate=rate, X_start=900.0, X_end=1300.0)}), calc))
    rs_kw = dict(axis="T", at=AT)
    plain = S.solve_network_ensemble(methods, sd, rd, fluxes=True)
    assert all(o.sol.resampled is None for o in plain)                    # the default: the call as it always was
    full = S.solve_network_ensemble(methods, sd, rd, fluxes=True, statistics=True, events=dict(level=0.5, kind="of_start", direction="fall"),
                                    resample=rs_kw)
    lean = S.solve_network_ensemble(methods, sd, rd, trajectories=False, statistics=True, resample=rs_kw)
    rs = full[0].sol.resampled
    assert isinstance(rs, S.ResampledEnsemble) and all(o.sol.resampled is rs for o in full) and rs.axis == "T"
    assert all(o.sol.resampled is lean[0].sol.resampled for o in lean) and lean[0].sol.resampled.u is None and lean[0].sol.u is None
    u = np.stack([o.sol.u for o in plain])
    T = np.array([o.sol_vcs["T"] for o in plain])
    ref, jc, _ = rc.ref_resample(u, T, AT)
    assert ec.same_bits(rs.u, ref) and np.array_equal(rs.jc, jc) and np.array_equal(lean[0].sol.resampled.jc, jc)
    assert np.array_equal(rs.covered, jc >= 0) and np.array_equal(rs.n_covered, rc.covered_run(jc, "fill")) and rs.n_covered[0] < len(AT) == rs.n_covered[-1]
    for a, b in zip(full, plain):      # what refers to the solve's own rows is the plain call's
        np.testing.assert_array_equal(a.sol.u, b.sol.u)
        np.testing.assert_array_equal(a.sol.t, b.sol.t)
        np.testing.assert_array_equal(a.sol.umax, b.sol.umax)
        assert a.sol.fluxes.flux.tobytes() == b.sol.fluxes.flux.tobytes()
    st, st_lean = full[0].sol.ensemble_stats, lean[0].sol.ensemble_stats
    assert np.array_equal(st.t, AT) and st.mean.shape == (len(AT), N) and st.count == int((rs.n_covered == len(AT)).sum())
    assert ec.same_bits(st.mean, st_lean.mean) and ec.same_bits(st.var, st_lean.var)
    ev = full[0].sol.events
    assert np.array_equal(ev.t, AT) and np.all((ev.t_peak >= 900.0) & (ev.t_peak <= 1300.0))      # a peak temperature
    one = S.resample_solution(plain[1], AT, axis="T")
    assert ec.same_bits(one.u, ref[1]) and np.array_equal(one.jc, jc[1]) and one.n_covered == rs.n_covered[1]


def test_solution_resample_of_a_first_order_decay():
    """A -> B with rate constant k, rows dt apart, queried at the midpoints of the save intervals against exp(-k t). The gate is
    derived as test_gpu_ensemble_event_times.py derives the half-life's: the sum of
      the chord's error: u_A = exp(-k t) is convex, the chord between two rows dt apart lies above it by at most
        k^2 dt^2 max(u) / 8 <= k^2 dt^2 / 8 (1.25e-3 for k = 1000 / s, dt = 1e-4 s) since u <= 1;
      the solve's error: the saved values are within C (reltol u + abstol) of exp(-k t), C = 100 for the growth of the local
        error the controller holds at (reltol, abstol) = (1e-8, 1e-10) into a global one and for the interpolation onto the save
        grid; a chord's value is a convex combination of two such rows (1.01e-6)."""
    k, dt, C = 1000.0, 1e-4, 100.0
    h = capi.HipNetwork(2, [0, 1], [0], [1], [0, 1], [1], [1])
    h.set_rates([k])
    p = kp(2e-3, save=dt)
    t, u, rcode, _, _ = h.solve(p, np.array([1.0, 0.0]))
    assert rcode == 0 and len(t) == 21
    mid = 0.5 * (t[:-1] + t[1:])
    got = h.solution_resample(mid)
    gate = k * k * dt * dt / 8.0 + C * (p.reltol * 1.0 + p.abstol)
    worst = np.abs(got[:, 0] - np.exp(-k * mid)).max()
    print(f"worst deviation from exp(-k t) at the midpoints {worst!r}, gate {gate!r}")
    assert worst <= gate and np.all(got[:, 0] >= np.exp(-k * mid) - C * (p.reltol + p.abstol))      # (the chord lies above)
    assert ec.same_bits(got, rc.ref_resample(u[None], t, mid)[0][0])
    assert h.solution_resample(t).tobytes() == u.tobytes()                # at the saved times: the saved rows
    own = h.solution_resample(np.array([0.5]), x=np.arange(21.0) / 20.0, mode="hold")      # an axis of the caller's
    assert own[0].tobytes() == u[10].tobytes()
    out = h.solution_resample(np.array([-1.0, 1.0, math.nan]), mode="hold", fill=7.0)
    assert out[0].tobytes() == u[0].tobytes() and out[1].tobytes() == u[-1].tobytes() and np.all(out[2] == 7.0)
    h.close()
