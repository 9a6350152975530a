"""GPU tests of the Sobol indices over a stored ensemble: kin_ensemble_sobol reads the members' saved states where the last
kin_solve_ensemble* call left them; solving.sobol_indices and solve_network_ensemble(statistics=dict(sobol=...)) on top.

A Saltelli design over uncertain rate constants: synthetic_crn(300, 1500) on the resident route at 1000 K, 21 saved rows,
M = 16 base samples of P = 4 inputs (K = 96 members): inputs 0-2 are log-multipliers k0 exp(0.6 (x - 1/2)) on the three
reactions with the largest time-integrated flux of the unperturbed solve, input 3 changes nothing.
  the dummy input: block AB_3 is block A byte for byte, its S1 and ST exactly 0.0 everywhere
  the start row (all members at u0): all zeros
  stored ensemble, trajectories downloaded or not, against the host entry over the download: bit for bit
  both within the derived gates of sobol_cases.ref_sobol on the download (columns whose variance is 0 or above 1e-250: squares
  of values near the bottom of the double range underflow on the device, the header says so)"""
import numpy as np
import pytest

import member_stats_cases as mc
import sobol_cases as sc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import synthetic_crn
from test_gpu_ensemble_analysis import kp

pytestmark = pytest.mark.gpu
OUTPUTS = ("first", "total", "mean", "var")


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_saltelli_design_over_rate_constants():
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    k0 = h.rates_at(1000.0)
    u0 = np.zeros(300); u0[0] = 1.0
    p = kp(2e-3, save=1e-4)
    h.set_rates(k0)
    t, us, rc, _, _ = h.solve(p, u0)
    assert rc == 0 and len(t) == 21
    top = np.argsort(-np.abs(h.solution_flux(w=S.flux_weights(t))))[:3]
    M, P = 16, 4
    K = M * (P + 2)
    X = S.sobol_design(M, P, seed=7)
    k = np.tile(k0, (K, 1))
    k[:, top] *= np.exp(0.6 * (X[:, :3] - 0.5))
    U0 = np.tile(u0, (K, 1))

    t0, none, ns0, rcs0, _ = h.solve_ensemble(p, U0, k=k, trajectories=False)
    assert none is None and np.all(rcs0 == 0) and np.all(ns0 == 21)
    a = h.ensemble_sobol(M, P)
    t1, u, ns, rcs, _ = h.solve_ensemble(p, U0, k=k, trajectories=True)
    assert u.shape == (K, 21, 300) and np.array_equal(ns, ns0)
    b = h.ensemble_sobol(M, P)
    host = h.members_sobol(u, M, P)
    assert a["count"] == b["count"] == host["count"] == M
    for q in OUTPUTS:
        assert _same(a[q], host[q]) and _same(b[q], host[q]), q
    # the dummy input and the start row
    assert u[5 * M:6 * M].tobytes() == u[:M].tobytes()
    assert np.all(a["first"][:, :, 3] == 0.0) and np.all(a["total"][:, :, 3] == 0.0)
    assert np.all(a["first"][0] == 0.0) and np.all(a["total"][0] == 0.0) and np.all(a["var"][0] == 0.0) and np.array_equal(a["mean"][0], u0)
    # the gates of the restatement on the download
    ref = sc.ref_sobol(u, M, P)
    ok = (ref["var"] == 0.0) | (ref["var"] > 1e-250)
    assert ok[-1].sum() > 100 and np.all(np.isfinite(a["first"])) and np.all(np.isfinite(a["total"]))
    for q in OUTPUTS:
        sel = ok if a[q].ndim == 2 else np.broadcast_to(ok[:, :, None], a[q].shape)
        assert sc.within(a[q][sel], ref[q][sel], ref["gate_" + q][sel]), (q, sc.worst(a[q][sel], ref[q][sel], ref["gate_" + q][sel]))
    # the inputs matter, the dummy does not
    lively = int(np.argmax(a["var"][-1]))
    print(f"species {lively} at the last row: S1 = {a['first'][-1, lively]}, ST = {a['total'][-1, lively]}")
    assert a["total"][-1, lively, :3].max() > 0.1
    # selections, the high-level call, the peak values, the bootstrap
    sel = [0, 7, 150, 299, lively]
    s = h.ensemble_sobol(M, P, species=sel)
    for q in OUTPUTS:
        assert _same(s[q], np.ascontiguousarray(host[q][:, sel])), q
    si = S.sobol_indices(h, t1, M, P, species=sel)
    assert isinstance(si, S.SobolIndices) and si.count == M and np.array_equal(si.t, t1) and si.species.tolist() == sel
    assert _same(si.first, s["first"]) and _same(si.total, s["total"]) and _same(si.mean, s["mean"]) and _same(si.var, s["var"])
    assert si.first_ci is None and si.total_ci is None and si.ranking(species=lively)[-1] == 3
    umax = h.ensemble_max()
    assert np.array_equal(umax, u.max(axis=1))
    peak, peak_ref = S.sobol_indices(h, t1, M, P, of="max"), h.members_sobol(umax[:, None, :], M, P)
    assert peak.first.shape == (1, 300, P) and peak.count == M
    assert _same(peak.first, peak_ref["first"]) and _same(peak.total, peak_ref["total"]) and _same(peak.var, peak_ref["var"])
    boot = S.sobol_indices(h, t1, M, P, species=sel, n_boot=8, seed=5)
    assert _same(boot.first, si.first) and boot.first_ci.shape == boot.total_ci.shape == (2, 21, len(sel), P)
    assert np.all(boot.first_ci[0] <= boot.first_ci[1]) and np.all(boot.total_ci[0] <= boot.total_ci[1])
    again = S.sobol_indices(h, t1, M, P, species=sel, n_boot=8, seed=5)
    assert _same(again.first_ci, boot.first_ci) and _same(again.total_ci, boot.total_ci)
    other = S.sobol_indices(h, t1, M, P, species=sel, n_boot=8, seed=6)
    assert not _same(other.total_ci, boot.total_ci)
    # a design that is not the stored ensemble's
    for Mb, Pb in ((16, 3), (12, 5), (96, 1)):
        with pytest.raises(capi.KineticaHipError) as e:
            h.ensemble_sobol(Mb, Pb)
        assert e.value.code == capi.KIN_ERR_INVALID_ARG
    h.close()


def test_a_sample_with_a_failed_member_takes_no_part():
    """The recipe of test_gpu_ensemble_statistics.py inside a design with M = 4, P = 1 over the temperature: member 5 (block B,
    sample 1) has absurd rate constants and a step budget that ends it early."""
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(300); u0[0] = 1.0
    M, P = 4, 1
    T = 900.0 + 300.0 * S.sobol_design(M, P, seed=3)[:, 0]
    kbad = np.array([h.rates_at(float(Ti)) for Ti in T]); kbad[5] *= 1e40
    p = kp(2e-3, save=1e-4, maxiters=3000)
    t, u, ns, rcs, _ = h.solve_ensemble(p, np.tile(u0, (12, 1)), k=kbad, trajectories=True)
    assert rcs[5] != 0 and ns[5] < 21 and all(ns[m] == 21 for m in range(12) if m != 5)
    assert h.ensemble_sobol_weights(M, P).tolist() == [1, 0, 1, 1]
    got = h.ensemble_sobol(M, P)
    assert got["count"] == 3
    up = u.copy(); up[[1, 5, 9]] = np.nan                    # never read: the host entry over the download with the same weights
    ref = h.members_sobol(up, M, P, w=np.array([1, 0, 1, 1]))
    for q in OUTPUTS:
        assert got[q].tobytes() == ref[q].tobytes() and np.all(np.isfinite(got[q])), q
    assert S.sobol_indices(h, t, M, P).count == 3
    two = h.ensemble_sobol(M, P, w=np.array([2, 0, 0, 1]))
    assert two["count"] == 3 and two["first"].tobytes() == h.members_sobol(up, M, P, w=np.array([2, 0, 0, 1]))["first"].tobytes()
    for w in ([1, 1, 1, 1], [0, 3, 0, 0]):
        with pytest.raises(capi.KineticaHipError) as e:
            h.ensemble_sobol(M, P, w=np.array(w))
        assert e.value.code == capi.KIN_ERR_INVALID_ARG
    with pytest.raises(capi.KineticaHipError) as e:
        h.ensemble_sobol(M, P, w=np.array([1, 0, -1, 1]))
    assert e.value.code == capi.KIN_ERR_INVALID_ARG
    h.close()


def test_solve_network_ensemble_sobol_over_heating_rates():
    from kinetica_jl_amd import conditions as C
    n = 300
    net, Ea, A = synthetic_crn(n, 5 * n)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(n)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    M, P = 2, 1
    X = S.sobol_design(M, P, seed=1)
    methods = []
    for x in X[:, 0]:
        u0 = np.zeros(n); u0[0] = 1.0
        pars = S.ODESimulationParams(tspan=(0.0, 2e-3), u0=u0, save_interval=2.5e-4, low_k_cutoff="none")
        methods.append(S.VariableODESolve(pars, C.ConditionSet({"T": C.LinearGradientProfile(rate=1e5 * (1.0 + 3.0 * x), X_start=900.0,
                                                                                             X_end=1300.0)}), calc))
    plain = S.solve_network_ensemble(methods, sd, rd)
    assert all(o.sol.ensemble_stats is None for o in plain)      # the default: the call as it always was
    sel = [0, 5, 17]
    with pytest.raises(ValueError):
        S.solve_network_ensemble(methods, sd, rd, statistics=dict(sobol=dict(M=3, P=1)))
    with pytest.raises(ValueError):
        S.solve_network_ensemble(methods, sd, rd, statistics=dict(sobol=dict(M=M, P=P, species=[n])))
    full = S.solve_network_ensemble(methods, sd, rd, statistics=dict(quantiles=None, sobol=dict(M=M, P=P, species=sel, n_boot=4)))
    st = full[0].sol.ensemble_stats
    assert isinstance(st, S.EnsembleStatistics) and all(o.sol.ensemble_stats is st for o in full)
    sb = st.sobol
    rows = len(full[0].sol.t)
    assert isinstance(sb, S.SobolIndices) and sb.count == M and sb.species.tolist() == sel and np.array_equal(sb.t, full[0].sol.t)
    assert sb.first.shape == sb.total.shape == (rows, 3, P) and sb.first_ci.shape == (2, rows, 3, P) and st.count == len(methods)
    for a, b in zip(full, plain):
        np.testing.assert_array_equal(a.sol.u, b.sol.u)
        assert a.sol.retcode == b.sol.retcode == "Success"
    # against the host entry over the downloaded trajectories of the plain call
    u = np.stack([o.sol.u for o in plain])
    hn = capi.HipNetwork(*mc.chain_network(n))
    ref = hn.members_sobol(u, M, P, species=sel)
    hn.close()
    assert _same(sb.first, ref["first"]) and _same(sb.total, ref["total"]) and _same(sb.mean, ref["mean"]) and _same(sb.var, ref["var"])
    assert np.all(sb.total[-1] >= 0.0) and sb.total[-1].max() > 0.0
    lean = S.solve_network_ensemble(methods, sd, rd, trajectories=False, statistics=True)
    assert lean[0].sol.ensemble_stats.sobol is None and lean[0].sol.ensemble_stats.quantiles.shape == (3, rows, n)
