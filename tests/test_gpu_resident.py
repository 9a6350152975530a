"""GPU parity tests of the resident integrator (kinetica_jl_amd/csrc/resident.hip: one workgroup owns one trajectory for the
whole solve) through the C ABI: kin_solve on small networks (routed there automatically), kin_solve_ensemble. References: the
committed Radau truths, the compiled CPU port at tight tolerances, the host-driven multi-kernel integrator (KIN_RESIDENT=0),
and the CPU replay of the very controller the kernel runs (tests/res_host.py). Trajectories cannot see a subtly wrong Jacobian
or inverse (the corrector iterates on the true residual): the kernel's RHS, Jacobian, factorisation, dense inverse and solve
are compared with references phase by phase in tests/test_gpu_resident_linalg.py (kin_resident_probe). Reference semantics: solve_network's chunk
loop, discrete rate updates and adaptive_solve! retries (methods.jl:185-303, 717-865; solve_utils.jl:376-424, 435-509)."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from oracle import cpu_bdf
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def kp(t1, chunk=1e-3, save=None, chunks=True, **kw):
    d = dict(tspan0=0.0, tspan1=t1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1 if chunks else 0,
             ban_negatives=0, solve_chunkstep=chunk, maxiters=100000, save_interval=-1.0 if save is None else save, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


def units(u, ref, atol=1e-10, rtol=1e-8):
    return float((np.abs(u - ref) / (atol + rtol * np.abs(ref))).max())


ROB = from_lists(3, [[(0, 1)], [(1, 2)], [(1, 1), (2, 1)]], [[(1, 1)], [(1, 1), (2, 1)], [(0, 1), (2, 1)]])
ROB_K = np.array([0.04, 3e7, 1e4])


def host_path(monkeypatch, on):
    if on:
        monkeypatch.setenv("KIN_RESIDENT", "0")
    else:
        monkeypatch.delenv("KIN_RESIDENT", raising=False)


def test_small_network_against_tight_truth_host_path_and_replay(monkeypatch):
    """300 species, 4 default chunks: the resident kernel, the host-driven path and the CPU replay of the kernel's controller
    against a 1000x tighter integration of the CPU port. Resident kernel and replay run the SAME controller: same step counts up
    to rounding of the linear algebra."""
    from tests.res_host import HostResident
    net, Ea, A = synthetic_crn(300, 1500)
    k = orc.arrhenius(Ea, A, 1000.0, k_max=1e12)
    u0 = np.zeros(300); u0[0] = 1.0
    tt, ut, rct, _ = cpu_bdf.CpuSolver(net).solve(dict(tspan=(0.0, 4e-3), abstol=1e-13, reltol=1e-11, dtmin=1e-300, adaptive_tols=False), u0, k0=k)
    assert rct == 0
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    host_path(monkeypatch, False)
    t, u, rc, st, status = h.solve(kp(4e-3), u0)
    assert status == capi.KIN_OK and rc == 0 and st["n_chunks"] == 4 and st["n_restarts"] == 4
    assert st["lu_slots"] <= 64 and st["n_lu_reused"] > 0.8 * st["n_steps"]          # the resident path's cache has 64 slots at most
    np.testing.assert_array_equal(t, tt)
    assert units(u, ut) < 100
    host_path(monkeypatch, True)
    th, uh, rch, sth, _ = h.solve(kp(4e-3), u0)
    assert rch == 0 and sth["lu_slots"] > 64 and units(uh, ut) < 100
    assert abs(st["n_steps"] - sth["n_steps"]) <= 0.05 * sth["n_steps"] + 5
    hr = HostResident(net)
    tr, ur, rcr, sr = hr.solve(kp(4e-3), u0, k0=k)
    assert rcr == 0 and abs(st["n_steps"] - sr["n_steps"]) <= 0.03 * sr["n_steps"] + 3
    assert abs(st["n_factor"] - sr["n_factor"]) <= 0.15 * sr["n_factor"] + 5
    assert units(u, ur) < 100
    hr.close(); h.close()


def test_tight_tolerances_against_a_radau_truth(golden_dir, monkeypatch):
    """at rtol = 1e-10 the resident and the host-driven integrator were known to end thousands of tolerance units apart
    without a statement of which one is off. Both against `truth_tight_200.npz` - SciPy's Radau IIA at 10x tighter tolerances
    (tests/golden/make_truth_tight.py; its 1e-10 sibling sits 8.5 units away) - in units of the TIGHT tolerances
    (1e-12 + 1e-10 |u|). Every implementation runs on the rounding floor of the right-hand side there (most steps are corrector
    failures) and lands by the accuracy of its linear algebra and by how far its corrector is asked to converge: with the corrector
    tolerance at 0.1 of the error weight (round 5, where rtol <= 1e-9: bdf_rules.hpp bdf_newton_frac) the CPU port (pivoted LU) ends rms 61 / max 378 in 4 073 steps, the resident kernel
    55 / p99.9 496 / max 757 in 5 656, the host-driven path 394 / 3 758 / 5 572 in 9 785 (profiles/r05_tight_tol_truth.jsonl; at
    0.03 they were 153, 385 and 885 in 6 692, 9 531 and 17 618 steps, profiles/r05_newton_tol_ab.txt). Bounds: 2x the measurement.
    In DEFAULT units (100x larger) all of them are within 60 - a tolerance below ~1e-9 buys little on these networks in FP64
    (DESIGN 4.0), and the resident kernel is the more accurate of the two device integrators there."""
    z = np.load(golden_dir + "/truth_tight_200.npz")
    assert float(z["self_check"]) < 20.0
    n, seed, T = int(z["n"]), int(z["seed"]), float(z["T"])
    monkeypatch.setenv("KIN_RESIDENT_MAX_N", "600"); monkeypatch.setenv("KIN_RESIDENT_MAX_DENSE", "512")
    net, Ea, A = synthetic_crn(n, 5 * n, seed=seed)
    k = orc.arrhenius(Ea, A, T, k_max=1e12)
    u0 = np.zeros(n); u0[0] = 1.0
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    p = capi.KinParams(tspan0=0.0, tspan1=1e-2, abstol=1e-12, reltol=1e-10, adaptive_tols=1, update_tols=0, solve_chunks=1, ban_negatives=0,
                       solve_chunkstep=1e-3, maxiters=400000, save_interval=1e-3, dtmin=1e-30)
    res = {}
    for name, host in (("resident", False), ("host_driven", True)):
        host_path(monkeypatch, host)
        t, u, rc, st, status = h.solve(p, u0)
        assert status == capi.KIN_OK and rc == 0 and st["n_retries"] == 0
        e = np.abs(u[1:] - z["u"]) / (1e-12 + 1e-10 * np.abs(z["u"]))
        res[name] = (float(np.sqrt((e ** 2).mean(axis=1)).max()), float(np.percentile(e, 99.9)), st["n_steps"])
    assert res["resident"][0] <= 110 and res["resident"][1] <= 1000, res
    assert res["host_driven"][0] <= 790 and res["host_driven"][1] <= 7500, res
    h.close()


def test_known_answers_ramp_and_grids(golden_dir, monkeypatch):
    host_path(monkeypatch, False)
    z = np.load(golden_dir + "/truth_small.npz")
    h = capi.HipNetwork.from_flat(ROB)
    h.set_rates(ROB_K)
    t, u, rc, st, _ = h.solve(kp(40.0, chunks=False, save=4.0), [1.0, 0.0, 0.0])
    assert rc == 0 and st["lu_slots"] <= 64
    np.testing.assert_allclose(t, z["rober_t"])
    assert units(u, z["rober_u"]) < 100
    # a save interval that does not divide the chunk (the chunk end is a save point on the last chunk only)
    t2, u2, rc2, _, _ = h.solve(kp(8.0, chunk=4.0, save=1.5), [1.0, 0.0, 0.0])
    tc, uc, rcc, _ = cpu_bdf.CpuSolver(ROB).solve(dict(tspan=(0.0, 8.0), solve_chunkstep=4.0, save_interval=1.5), [1.0, 0.0, 0.0], k0=ROB_K)
    assert rc2 == 0
    np.testing.assert_allclose(t2, tc, rtol=0, atol=1e-15)
    assert units(u2, uc) < 10
    h.close()
    # 60 species under a temperature ramp: rates from T_stops on the device, and from a table; complete and chunkwise
    net, Ea, A = synthetic_crn(60, 300, seed=11)
    u0 = np.zeros(60); u0[0] = 1.0
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e3)
    tst = np.arange(8) * 0.125
    t, u, rc, st, _ = h.solve(kp(1.0, chunks=False, save=0.0625), u0, tstops=tst, T_stops=z["ramp_T"])
    assert rc == 0 and st["n_restarts"] == 8
    np.testing.assert_allclose(t, z["ramp_t"], rtol=0, atol=1e-15)
    assert units(u, z["ramp_u"]) < 100
    ks = orc.rate_table(Ea, A, z["ramp_T"], k_max=1e3)
    t2, u2, rc2, st2, _ = h.solve(kp(1.0, chunk=0.25, save=0.0625), u0, tstops=tst, k_table=ks)
    assert rc2 == 0 and st2["n_chunks"] == 4 and st2["n_restarts"] == 8
    assert units(u2, z["ramp_u"]) < 100
    # the rates in force at the end of the solve are what the handle holds afterwards
    np.testing.assert_allclose(h.get_rates(), ks[-1], rtol=1e-14)
    h.rates_at(1000.0)
    t3, u3, rc3, _, _ = h.solve(kp(1.0, chunks=False, save=0.0625), u0)
    assert rc3 == 0 and units(u3, z["syn_u"]) < 100
    h.close()


def test_failure_semantics_match_the_host_path(monkeypatch):
    h = capi.HipNetwork.from_flat(ROB)
    h.set_rates(ROB_K)
    for bad, want in ((dict(dtmin=1.0), 2), (dict(maxiters=5), 1)):
        res = {}
        for on in (False, True):
            host_path(monkeypatch, on)
            t, u, rc, st, status = h.solve(kp(40.0, chunks=False, save=4.0, **bad), [1.0, 0.0, 0.0])
            res[on] = (len(t), rc, st["n_retries"], status, st["final_abstol"])
            assert status == capi.KIN_ERR_SOLVE_FAILED and rc == want and st["n_retries"] == 4
        assert res[False] == res[True]
    host_path(monkeypatch, False)
    t, u, rc, st, status = h.solve(kp(40.0, chunks=False, save=4.0, dtmin=1.0, adaptive_tols=0), [1.0, 0.0, 0.0])
    assert rc == 2 and st["n_retries"] == 0
    # ban_negatives: no negative concentration in any saved state
    net, Ea, A = synthetic_crn(200, 1000)
    hh = capi.HipNetwork.from_flat(net)
    hh.set_arrhenius(Ea, A, k_max=1e12)
    hh.rates_at(1400.0)
    u0 = np.zeros(200); u0[0] = 1.0
    t, u, rc, st, _ = hh.solve(kp(2e-3, ban_negatives=1), u0)
    assert rc == 0 and u.min() >= 0.0
    hh.close(); h.close()


def test_ensemble_members_are_bit_identical_to_solo_solves():
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    rng = np.random.default_rng(7)
    K = 12
    U0 = np.zeros((K, 300)); U0[:, 0] = 1.0
    U0[:, 1:4] = rng.uniform(0.0, 0.1, (K, 3))
    T = np.linspace(900.0, 1400.0, K)
    # per-member temperatures
    t, u, ns, rcs, sts = h.solve_ensemble(kp(2e-3), U0, T=T)
    assert (rcs == 0).all() and (ns == 3).all() and len(t) == 3
    for i in (0, 5, K - 1):
        h.rates_at(float(T[i]))
        ts, us, rc, st, _ = h.solve(kp(2e-3), U0[i])
        assert rc == 0 and np.array_equal(ts, t) and np.array_equal(us, u[i]) and st["n_steps"] == sts[i]["n_steps"]
    # per-member rate constants (any calculator), and the handle's own rates for every member
    ks = np.array([h.rates_at(float(Ti)) for Ti in T])     # the device's own Arrhenius values: bit-identical inputs
    t2, u2, ns2, rcs2, _ = h.solve_ensemble(kp(2e-3), U0, k=ks)
    assert np.array_equal(u2, u)
    h.set_rates(ks[3])
    t3, u3, _, rcs3, _ = h.solve_ensemble(kp(2e-3), U0[:4])
    assert (rcs3 == 0).all() and np.array_equal(u3[3], u[3])
    # shared discrete rate updates (zero-order hold at tstops)
    tst = np.arange(4) * 0.5e-3
    Ts = np.array([900.0, 1000.0, 1100.0, 1200.0])
    t4, u4, ns4, rcs4, sts4 = h.solve_ensemble(kp(2e-3, save=2.5e-4), U0[:5], tstops=tst, T_stops=Ts)
    assert (rcs4 == 0).all() and sts4[0]["n_restarts"] == 4
    ts, us, rc, _, _ = h.solve(kp(2e-3, save=2.5e-4), U0[2], tstops=tst, T_stops=Ts)
    assert np.array_equal(ts, t4) and np.array_equal(us, u4[2])
    # argument errors
    with pytest.raises(capi.KineticaHipError):
        h.solve_ensemble(kp(2e-3), U0, k=ks, T=T)
    with pytest.raises(capi.KineticaHipError):
        h.solve_ensemble(kp(2e-3, chunks=False), U0, T=T)          # no save grid
    h.close()


def test_more_members_than_compute_units_take_the_shared_cu_build(monkeypatch):
    """K > the chip's compute units: the launch uses the kernel built with half the registers per lane, two workgroups per
    compute unit (resident_w4.hip). Same source, same arithmetic: members equal their solo solves (the one-workgroup-per-CU
    build) bit for bit; forced on for a small ensemble and forced off for the large one as well."""
    net, Ea, A = synthetic_crn(100, 500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    K = 300
    U0 = np.zeros((K, 100)); U0[:, 0] = 1.0
    T = np.linspace(900.0, 1300.0, K)
    t, u, ns, rcs, sts = h.solve_ensemble(kp(2e-3), U0, T=T)
    assert (rcs == 0).all() and (ns == 3).all()
    for i in (0, 137, K - 1):
        h.rates_at(float(T[i]))
        ts, us, rc, st, _ = h.solve(kp(2e-3), U0[i])
        assert rc == 0 and np.array_equal(us, u[i]) and st["n_steps"] == sts[i]["n_steps"]
    monkeypatch.setenv("KIN_RESIDENT_SHARED_CU", "0")
    _, u0_, _, rcs0, _ = h.solve_ensemble(kp(2e-3), U0, T=T)
    monkeypatch.setenv("KIN_RESIDENT_SHARED_CU", "1")
    _, u1_, _, rcs1, _ = h.solve_ensemble(kp(2e-3), U0[:5], T=T[:5])
    assert np.array_equal(u0_, u) and np.array_equal(u1_, u[:5]) and (rcs0 == 0).all() and (rcs1 == 0).all()
    h.close()


def test_shared_cu_build_is_bit_identical_without_look_ahead(monkeypatch):
    """The two builds (KIN_RESIDENT_SHARED_CU=1 / 0) bit for bit at a dense block of nb = 8 block steps, where the Gauss-Jordan
    runs without look-ahead, on a network that fits two workgroups per compute unit (else the switch falls back silently)."""
    from tests.test_gpu_resident_linalg import core_net
    net = core_net(120)
    assert capi.lu_analyze_host(net, min_round=2)["m"] == 120                 # nb = 8
    rng = np.random.default_rng(120)
    k = 10.0 ** rng.uniform(0.0, 3.0, net.n_reactions)
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    n = net.n_species
    info = h.resident_probe(np.ones(n), 1e-3, np.ones(n))["info"]
    assert info["m"] == 120 and 2 * (info["dyn_lds"] + 16 * 1024) <= 160 * 1024   # (static LDS of the kernel < 16 KiB)
    K = 16
    U0 = np.zeros((K, n)); U0[:, :120] = rng.uniform(0.0, 1.0, (K, 120))
    ks = k[None, :] * rng.uniform(0.5, 2.0, (K, 1))
    monkeypatch.setenv("KIN_RESIDENT_SHARED_CU", "0")
    t0, u0_, _, rcs0, sts0 = h.solve_ensemble(kp(2e-3), U0, k=ks)
    monkeypatch.setenv("KIN_RESIDENT_SHARED_CU", "1")
    t1, u1_, _, rcs1, sts1 = h.solve_ensemble(kp(2e-3), U0, k=ks)
    assert (rcs0 == 0).all() and (rcs1 == 0).all() and sts0[0]["n_factor"] > 0
    assert np.array_equal(t0, t1) and np.array_equal(u0_, u1_) and [q["n_steps"] for q in sts0] == [q["n_steps"] for q in sts1]
    h.close()


def test_warm_chunk_continuation_in_all_three_drivers(monkeypatch):
    """kin_params.solve_chunks = 2 through the resident kernel, the host-driven integrator and - as ensemble members - the
    resident ensemble and the lockstep rounds: same save times as the re-initialising run, fewer steps, results within the
    step-sequence tolerance of each other and of the re-initialising run."""
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    h.rates_at(1000.0)
    u0 = np.zeros(300); u0[0] = 1.0
    cold = kp(1e-2)
    warm = kp(1e-2, solve_chunks=2)
    tc, uc, rcc, stc, _ = h.solve(cold, u0)
    tw, uw, rcw, stw, _ = h.solve(warm, u0)
    assert rcc == 0 and rcw == 0 and np.array_equal(tc, tw) and stw["n_restarts"] == 10
    assert stw["n_steps"] < 0.95 * stc["n_steps"] and units(uw, uc) < 150         # 987 against 1 091 (970 / 1 129 before the re-initialisations got cheaper in round 5)
    monkeypatch.setenv("KIN_RESIDENT", "0")
    th, uh, rch, sth, _ = h.solve(warm, u0)
    monkeypatch.delenv("KIN_RESIDENT")
    assert rch == 0 and np.array_equal(th, tw) and sth["lu_slots"] > 64 and abs(sth["n_steps"] - stw["n_steps"]) <= 0.1 * stw["n_steps"]
    assert units(uh, uw) < 150
    te, ue, _, rcs, sts = h.solve_ensemble(warm, np.tile(u0, (2, 1)), T=np.array([1000.0, 1100.0]))
    assert (rcs == 0).all() and np.array_equal(ue[0], uw) and sts[0]["n_steps"] == stw["n_steps"]
    monkeypatch.setenv("KIN_ENSEMBLE_BATCHED", "1")
    tl, ul, _, rcl, stl = h.solve_ensemble(warm, np.tile(u0, (2, 1)), T=np.array([1000.0, 1100.0]))
    assert (rcl == 0).all() and units(ul[0], uw) < 150 and abs(stl[0]["n_steps"] - stw["n_steps"]) <= 0.1 * stw["n_steps"]
    h.close()


def test_a_member_that_fails_does_not_disturb_the_others():
    h = capi.HipNetwork.from_flat(ROB)
    ks = np.array([ROB_K, ROB_K * np.array([1.0, 1e30, 1.0]), ROB_K])      # member 1: rates that overflow the state
    U0 = np.tile([1.0, 0.0, 0.0], (3, 1))
    t, u, ns, rcs, sts = h.solve_ensemble(kp(40.0, chunks=False, save=4.0, maxiters=2000), U0, k=ks)
    assert rcs[0] == 0 and rcs[2] == 0 and np.array_equal(u[0], u[2]) and ns[0] == 11
    h.set_rates(ROB_K)
    ts, us, rc, _, _ = h.solve(kp(40.0, chunks=False, save=4.0, maxiters=2000), [1.0, 0.0, 0.0])
    assert np.array_equal(us, u[0])
    h.close()


def test_mid_size_network_through_the_ensemble_entry_point():
    """1 000 species: beyond the single-solve routing threshold (the host-driven path is faster for ONE trajectory there) but
    inside the resident kernel's LDS budget: kin_solve_ensemble integrates it, members against the host-driven kin_solve."""
    net, Ea, A = synthetic_crn(1000, 5000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(1000); u0[0] = 1.0
    T = np.linspace(1000.0, 1100.0, 32)                           # 32 members: below that the call goes to kin_solve on threads
    t, u, ns, rcs, sts = h.solve_ensemble(kp(2e-3), np.tile(u0, (32, 1)), T=T)
    assert (rcs == 0).all() and sts[0]["lu_dense_dim"] > 100
    assert all(q["lu_slots"] <= 64 for q in sts)                  # the resident kernel (a thread member: kin_solve, > 64 slots)
    for i in (0, 31):
        h.rates_at(float(T[i]))
        ts, us, rc, st, _ = h.solve(kp(2e-3), u0)
        assert rc == 0 and st["lu_slots"] > 64                    # host-driven path
        assert units(u[i], us) < 150                              # two integrators, each within ~50 units of the truth
    h.close()


def test_few_members_of_a_large_network_are_kin_solve_calls_on_threads():
    """kin_solve_ensemble beyond the resident kernel's size with K <= KIN_ENSEMBLE_THREADS (12): K solve-only copies of the
    handle, one host thread each - every member bit-identical to kin_solve on its inputs, statistics included; per-member rate
    constants, temperatures, shared rate updates; a failing member does not disturb the others."""
    net, Ea, A = synthetic_crn(2000, 10000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(2000); u0[0] = 1.0
    T = np.array([950.0, 1050.0, 1150.0])
    t, u, ns, rcs, sts = h.solve_ensemble(kp(2e-3), np.tile(u0, (3, 1)), T=T)
    assert (rcs == 0).all() and (ns == 3).all() and sts[0]["lu_slots"] > 64          # the host-driven integrator's cache
    for i in range(3):
        h.rates_at(float(T[i]))
        ts, us, rc, st, _ = h.solve(kp(2e-3), u0)
        assert rc == 0 and np.array_equal(ts, t) and np.array_equal(us, u[i])
        assert st["n_steps"] == sts[i]["n_steps"] and st["n_factor"] == sts[i]["n_factor"]
    ks = np.array([h.rates_at(float(Ti)) for Ti in T])
    t2, u2, _, rcs2, _ = h.solve_ensemble(kp(2e-3), np.tile(u0, (3, 1)), k=ks)
    assert (rcs2 == 0).all() and np.array_equal(u2, u)
    tst = np.arange(4) * 0.5e-3
    Ts = np.array([900.0, 1000.0, 1100.0, 1200.0])
    t3, u3, _, rcs3, sts3 = h.solve_ensemble(kp(2e-3, save=5e-4), np.tile(u0, (2, 1)), tstops=tst, T_stops=Ts)
    ts, us, rc, st, _ = h.solve(kp(2e-3, save=5e-4), u0, tstops=tst, T_stops=Ts)
    assert (rcs3 == 0).all() and rc == 0 and np.array_equal(ts, t3) and np.array_equal(us, u3[0]) and np.array_equal(u3[0], u3[1])
    kbad = ks.copy(); kbad[1] *= 1e40
    t4, u4, ns4, rcs4, _ = h.solve_ensemble(kp(2e-3, maxiters=3000), np.tile(u0, (3, 1)), k=kbad)
    assert rcs4[1] != 0 and rcs4[0] == 0 and rcs4[2] == 0 and np.array_equal(u4[0], u[0]) and np.array_equal(u4[2], u[2])
    h.close()


def test_threads_take_several_members_each_beyond_the_thread_limit(monkeypatch):
    """KIN_ENSEMBLE_ROUTE=threads with more members than threads (5 members, 2 threads: member m on thread m mod 2, one after
    the other on the thread's replica of the handle): still bit for bit kin_solve per member, in the members' order."""
    monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", "threads")
    monkeypatch.setenv("KIN_ENSEMBLE_THREADS", "2")
    net, Ea, A = synthetic_crn(2000, 10000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(2000); u0[0] = 1.0
    T = np.array([950.0, 1000.0, 1050.0, 1100.0, 1150.0])
    t, u, ns, rcs, sts = h.solve_ensemble(kp(2e-3), np.tile(u0, (5, 1)), T=T)
    assert (rcs == 0).all() and (ns == 3).all()
    for i in range(5):
        h.rates_at(float(T[i]))
        ts, us, rc, st, _ = h.solve(kp(2e-3), u0)
        assert rc == 0 and np.array_equal(ts, t) and np.array_equal(us, u[i]) and st["n_steps"] == sts[i]["n_steps"]
    h.close()


def test_lockstep_ensemble_of_a_large_network(monkeypatch):
    """kin_solve_ensemble beyond the resident kernel's size (ensemble.cpp): members advance in lockstep rounds of batched
    launches, each with the controller the resident kernel runs. At C3 size against solo kin_solve runs of the same inputs
    (the host-driven integrator: same kernels' arithmetic, an independent controller implementation), and - forced at 1 000
    species - against the resident kernel's ensemble of the same members."""
    monkeypatch.setenv("KIN_ENSEMBLE_BATCHED", "1")       # (three members would otherwise be three kin_solve calls on threads)
    net, Ea, A = synthetic_crn(10000, 50000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(10000); u0[0] = 1.0
    T = np.array([1000.0, 1040.0, 1080.0])
    t, u, ns, rcs, sts = h.solve_ensemble(kp(2e-3), np.tile(u0, (3, 1)), T=T)
    assert (rcs == 0).all() and (ns == 3).all() and sts[0]["lu_dense_dim"] > 900
    for i in range(3):
        h.rates_at(float(T[i]))
        ts, us, rc, st, _ = h.solve(kp(2e-3), u0)
        assert rc == 0 and np.array_equal(ts, t)
        assert units(u[i], us) < 50                                              # measured 0 - 8
        assert abs(sts[i]["n_steps"] - st["n_steps"]) <= 0.02 * st["n_steps"] + 2
    # the members' dense inverses as one batched Gauss-Jordan chain (default) and as chains of their own: the same arithmetic
    monkeypatch.setenv("KIN_ENSEMBLE_GJ_BATCHED", "0")
    t1, u1, _, rcs1, sts1 = h.solve_ensemble(kp(2e-3), np.tile(u0, (3, 1)), T=T)
    monkeypatch.delenv("KIN_ENSEMBLE_GJ_BATCHED")
    assert (rcs1 == 0).all() and np.array_equal(u1, u) and [q["n_steps"] for q in sts1] == [q["n_steps"] for q in sts]
    # shared discrete rate updates through the lockstep path
    tst = np.arange(4) * 0.5e-3
    Ts = np.array([900.0, 1000.0, 1100.0, 1200.0])
    t2, u2, ns2, rcs2, sts2 = h.solve_ensemble(kp(2e-3, save=5e-4), np.tile(u0, (2, 1)), tstops=tst, T_stops=Ts)
    ts, us, rc, st, _ = h.solve(kp(2e-3, save=5e-4), u0, tstops=tst, T_stops=Ts)
    assert (rcs2 == 0).all() and rc == 0 and np.array_equal(ts, t2) and sts2[0]["n_restarts"] == 4
    assert units(u2[0], us) < 50 and np.array_equal(u2[0], u2[1])
    h.close()
    monkeypatch.delenv("KIN_ENSEMBLE_BATCHED")
    net, Ea, A = synthetic_crn(1000, 5000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(1000); u0[0] = 1.0
    T = np.array([950.0, 1050.0, 1150.0, 1250.0])
    # the resident kernel takes 1 000 species in one launch from 32 members on (fewer go to kin_solve on threads); its first four
    # members are the four the lockstep rounds run below
    T32 = np.concatenate([T, np.linspace(950.0, 1250.0, 28)])
    tr, ur, _, rcr, str_ = h.solve_ensemble(kp(2e-3), np.tile(u0, (32, 1)), T=T32)
    assert all(q["lu_slots"] <= 64 for q in str_)
    tr, ur, rcr = tr, ur[:4], rcr[:4]
    monkeypatch.setenv("KIN_ENSEMBLE_BATCHED", "1")
    tb, ub, _, rcb, stb = h.solve_ensemble(kp(2e-3), np.tile(u0, (4, 1)), T=T)
    assert (rcr == 0).all() and (rcb == 0).all() and np.array_equal(tr, tb)
    assert units(ub, ur) < 100
    # more members than KIN_ENSEMBLE_MAX_MEMBERS (a host thread each): block after block, the same members
    monkeypatch.setenv("KIN_ENSEMBLE_MAX_MEMBERS", "3")
    tm, um, nsm, rcm, _ = h.solve_ensemble(kp(2e-3), np.tile(u0, (4, 1)), T=T)
    monkeypatch.delenv("KIN_ENSEMBLE_MAX_MEMBERS")
    assert (rcm == 0).all() and np.array_equal(tm, tb) and np.array_equal(um, ub) and (nsm == 3).all()
    # a member that fails (rate constants that overflow its state) leaves the rounds; the others finish as without it
    ks = np.array([h.rates_at(float(Ti)) for Ti in T])
    kbad = ks.copy(); kbad[1] *= 1e40
    tf, uf, nsf, rcf, stf = h.solve_ensemble(kp(2e-3, maxiters=3000), np.tile(u0, (4, 1)), k=kbad)
    tg, ug, _, rcg, _ = h.solve_ensemble(kp(2e-3, maxiters=3000), np.tile(u0, (4, 1)), k=ks)
    assert rcf[1] != 0 and (rcf[[0, 2, 3]] == 0).all() and (rcg == 0).all()
    assert np.array_equal(uf[[0, 2, 3]], ug[[0, 2, 3]])
    h.close()
