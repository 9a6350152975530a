"""GPU tests of the library-order batched sweep (tiled_kernels.hip: tiled_sweep_kernel in its 18 instantiations, the layout
kernels permute_staged_kernel / rates_to_lib_pairs_kernel / gather_rows_kernel, rate_table_lib_kernel) through every entry:
kin_rhs_tiled_dev (k stream and temperature), kin_rhs_batched_klib_dev, kin_rhs_batched_T_dev, the three conversions and
kin_rate_table_lib_dev. Cases, inputs, references and bounds: tests/sweep_cases.py (checked without a GPU by
tests/test_sweep_cases.py, where the CPU replay of the kernel equals the exact reference on every layout).

For every case: kin_tiled_sweep_plan on the live handle reports the instantiation the case is named after and the handle's
layout is the host's; du starts as NaN; on the exact inputs EVERY state of B = 1, grid, grid + 1, 2 grid + 3 (grid from the
query; every state its own u and its own k row) equals the float64 reference bit for bit; on the random inputs and in the
temperature form every entry of the sampled states (first, last, one per trip) is inside its bound against the longdouble
reference - (L + 4) u S, plus (2 |Ea / (R T)| + 16) u per term where the device forms the rate constants.

Measured on one MI355X (printed at the end of the module, pytest -s; 67 tests, 52 s): largest error / bound against the
longdouble reference - k stream 0.43, one-slot records (SINGLES) 0.48, temperature form 0.73 on the realistic parameters and
0.06 on the structural ones. Every exact-input run equals the reference bit for bit; no kernel was found wrong. No windowed
layout with UN = 10 exists at test size (sweep_cases.NO_LAYOUT).

Mutation check (value-only changes, one at a time on a scratch build selected through KIN_LIB_PATH, nothing of them kept):
failing tests of this file (of 67), and what test_gpu_tiled.py (16 tests) - the suite's view of these kernels before - did.
  a tiled_sweep_kernel skips the fourth field's atomic for the last row of a batch: 40 fail - k stream and temperature form of
    every case but t256_un5_one_row (no second product among its 50 records). Before: 12 of 16 failed.
  b the odd-batch tail consumes G0 twice instead of moving G1 down: 17 fail - the k stream of every layout with an odd number
    of batches (rows 12 at NB = 4, the windowed t256_windows_odd_tail* and t256_windows_uneven_rows among them; rows 10 at
    NB = 2) and the temperature form of the rows-10 layouts; the even ones (rows 8, rows 12 at NB = 2) pass. Before: 7 failed.
  c the SINGLES path hands an odd one-slot record kk.x: the k stream of all 9 *_singles cases fails. Before: 5 failed.
  d the fold of the split accumulators leaves out the last copy entry: 38 fail - both forms of every case with n_copy > 0
    (t256_un5_one_row has none). Before: 12 failed. (sweep_reg_kernel's fold: test_gpu_sweep_exact.py.)
  h permute_staged_kernel<false, true> drops the last double2 of a piece: 19 fail - every windowed layout with an even N in
    the k stream (7), the temperature form (7) and test_conversions_are_permutations[*-aligned] (5); odd N and the
    8-byte-off buffers take <false, false> and pass. Before: 2 failed.
  (e) - (g): test_gpu_sweep_exact.py."""
import numpy as np
import pytest
import torch

from kinetica_jl_amd import capi
from tests import sweep_cases as sc
from tests.jac_cases import LD

pytestmark = pytest.mark.gpu

RATIOS = {}


def _dev(a, off_bytes=0):
    a = np.ascontiguousarray(a, np.float64)
    own = torch.empty(a.size + 2, dtype=torch.float64, device="cuda")
    o = off_bytes // 8 + (1 if own.data_ptr() % 16 else 0)
    v = own[o:o + a.size]
    v.copy_(torch.from_numpy(a.reshape(-1)))
    assert v.data_ptr() % 16 == off_bytes
    return v.view(a.shape)


def _nan(shape, off_bytes=0):
    return _dev(np.full(shape, np.nan), off_bytes)


def _sync():
    torch.cuda.synchronize()


def _handle(case):
    net, ref, Ea, A = sc.built("tiled", case.name)
    with sc.tiled_env(case):
        h = capi.HipNetwork.from_flat(net)
        lay = h.lib_layout()                 # the layout is built here, under the case's switches
        L = capi.lib_layout_host(net)
    assert np.array_equal(lay["species_of_lib"], L["species_of_lib"]) and np.array_equal(lay["slot_of_reaction"], L["slot_of_reaction"])
    assert lay["k_len"] == L["k_len"]
    return h, net, ref, Ea, A, L


def _k_ld(Ea, A, T, k_max):
    """the Arrhenius law in longdouble (calculator.jl: k = A N_A exp(-Ea / RT), capped harmonically by k_max)"""
    k = A.astype(LD) * LD(sc.N_A) * np.exp(-Ea.astype(LD) / (LD(sc.R_GAS) * LD(T)))
    return k if k_max is None else 1 / (1 / LD(k_max) + 1 / k)


def _first_diff(du, want, grid, what):
    if not np.array_equal(du, want):
        b, i = np.argwhere(du != want)[0]
        raise AssertionError((what, f"state {b} (trip {b // grid}) species {i}: {du[b, i]} != {want[b, i]}", f"{int((du != want).sum())} entries differ"))


@pytest.mark.parametrize("name", list(sc.TILED_CASES))
def test_k_stream_every_state_of_every_trip(name):
    case = sc.TILED_CASES[name]
    h, net, ref, Ea, A, L = _handle(case)
    N, R, KL = ref.N, ref.R, L["k_len"]
    sp, slot = L["species_of_lib"], L["slot_of_reaction"]
    try:
        pk, pT = h.tiled_sweep_plan(10 ** 6), h.tiled_sweep_plan(10 ** 6, True)
        sc.check_tiled_layout(case, L, pk, pT)
        grid = pk["grid"]
        assert grid == h.compute_units() * pk["per_cu"]
        Bs = sc.trip_batches(grid)
        Bmax = max(Bs)
        form = "singles" if pk["SINGLES"] else "k"
        for kind in ("exact", "random"):
            U_, K = (sc.exact_inputs if kind == "exact" else sc.random_inputs)(Bmax, N, R, 7)
            want = sc.exact_rhs(ref, U_, K) if kind == "exact" else None
            d_u, d_k = _dev(U_), _dev(K)
            d_ul, d_kl = _nan((Bmax, N)), _nan((Bmax, KL))
            _sync()
            h.states_to_lib_dev(Bmax, d_u.data_ptr(), d_ul.data_ptr())
            h.rates_to_lib_dev(Bmax, d_k.data_ptr(), d_kl.data_ptr())
            _sync()
            if kind == "exact":                     # the conversions are permutations; slots no reaction owns are written, zero
                assert np.array_equal(d_ul.cpu().numpy(), U_[:, sp])
                rows = np.r_[0:min(Bmax, 32), max(0, Bmax - 2):Bmax]      # (all rows: test_conversions_are_permutations)
                kl = np.zeros((len(rows), KL)); kl[:, slot] = K[rows]
                assert np.array_equal(d_kl[torch.from_numpy(rows).cuda()].cpu().numpy(), kl)
            for B in Bs:
                assert h.tiled_sweep_plan(B)["grid"] == min(B, grid)
                d_dul, d_du, d_du2 = _nan((B, N)), _nan((B, N)), _nan((B, N))
                _sync()
                h.rhs_tiled_dev(B, d_ul.data_ptr(), d_dul.data_ptr(), d_k_lib=d_kl.data_ptr())
                h.states_from_lib_dev(B, d_dul.data_ptr(), d_du.data_ptr())
                h.rhs_batched_klib_dev(B, d_u.data_ptr(), d_kl.data_ptr(), d_du2.data_ptr())
                _sync()
                dul, du, du2 = d_dul.cpu().numpy(), d_du.cpu().numpy(), d_du2.cpu().numpy()
                assert np.array_equal(du[:, sp], dul, equal_nan=True)
                if kind == "exact":
                    _first_diff(dul, want[:B][:, sp], grid, (name, "kin_rhs_tiled_dev", B))
                    _first_diff(du2, want[:B], grid, (name, "kin_rhs_batched_klib_dev", B))
                else:
                    for b in sc.sample_states(B, grid):
                        for dev, what in ((du[b], "tiled"), (du2[b], "klib")):
                            ok, ratio, worst = sc.judge_rhs(ref, K[b], U_[b], dev)
                            assert ok, (name, what, B, b, worst)
                            RATIOS[form] = max(RATIOS.get(form, 0.0), ratio)
    finally:
        h.close()


@pytest.mark.parametrize("name", list(sc.TILED_CASES))
def test_temperature_form_every_trip(name):
    """realistic: the case's Arrhenius parameters under k_max = 1e12, random states; structural: Ea = 0, k ~ 1 .. 8, u in
    {1/2, 1, 2} - a lost or doubled term is far outside the bound whatever its species. Both through kin_rhs_tiled_dev(T) on
    library-order states and kin_rhs_batched_T_dev on caller-order states."""
    case = sc.TILED_CASES[name]
    h, net, ref, Ea, A, L = _handle(case)
    N, R = ref.N, ref.R
    sp = L["species_of_lib"]
    try:
        pT = h.tiled_sweep_plan(10 ** 6, True)
        assert (pT["BS"], pT["TMODE"], pT["UN"], pT["SINGLES"], pT["NB"]) == (case.expect["BS"], 1, case.expect["UN"], 0, 2)
        grid = pT["grid"]
        Bs = sc.trip_batches(grid)
        Bmax = max(Bs)
        T = np.random.default_rng(11).uniform(600.0, 1200.0, Bmax)
        d_T = _dev(T)
        for kind in ("structural", "realistic"):
            if kind == "structural":
                ea, a, j = sc.structural_arrhenius(R, 13)
                kmax = None
                U_ = sc.exact_inputs(Bmax, N, R, 7, shared_k=True)[0]
                s_ref, s_bound = sc.structural_bound(ref, U_, j)
            else:
                ea, a, kmax = Ea, A, 1e12
                U_ = sc.random_inputs(Bmax, N, R, 7, shared_k=True)[0]
            h.set_arrhenius(ea, a, k_max=kmax)
            d_u, d_ul = _dev(U_), _dev(U_[:, sp])
            for B in Bs:
                d_dul, d_du = _nan((B, N)), _nan((B, N))
                _sync()
                h.rhs_tiled_dev(B, d_ul.data_ptr(), d_dul.data_ptr(), d_T=d_T.data_ptr())
                h.rhs_batched_T_dev(B, d_u.data_ptr(), d_T.data_ptr(), d_du.data_ptr())
                _sync()
                dul, du = d_dul.cpu().numpy(), d_du.cpu().numpy()
                assert np.isfinite(dul).all() and np.isfinite(du).all(), (name, kind, B)
                if kind == "structural":            # EVERY state: a term is >= 1/4, the bound ~1e-14 S
                    for dev, what in ((_rows_from_lib(dul, sp), "tiled_T"), (du, "batched_T")):
                        bad = np.abs(dev - s_ref[:B]) > s_bound[:B]
                        if bad.any():
                            b, i = np.argwhere(bad)[0]
                            raise AssertionError((name, what, f"B={B} state {b} (trip {b // grid}) species {i}: {dev[b, i]} vs {s_ref[b, i]}",
                                                  f"{int(bad.sum())} entries outside"))
                    assert np.abs(du).max() > 0
                for b in sc.sample_states(B, grid):
                    k = _k_ld(ea, a, T[b], kmax)
                    ex = sc.arrhenius_allowance(ea, T[b])
                    for dev, what in ((dul[b], "tiled_T"), (du[b][sp], "batched_T")):
                        ok, ratio, worst = sc.judge_rhs(ref, k, U_[b], _from_lib(dev, sp), ex)
                        assert ok, (name, kind, what, B, b, worst)
                        RATIOS["T_" + kind] = max(RATIOS.get("T_" + kind, 0.0), ratio)
    finally:
        h.close()


def _rows_from_lib(m_lib, sp):
    out = np.empty_like(m_lib)
    out[:, sp] = m_lib
    return out


def _from_lib(v_lib, sp):
    out = np.empty_like(v_lib)
    out[sp] = v_lib
    return out


CONVERSION_CASES = ("t256_windows_odd_tail", "t256_windows_odd_tail_singles", "t512_windows", "t1024_windows_odd_N_two_pieces",
                    "t1024_windows_even_N_two_pieces", "t1024_windows_two_pieces_singles", "t256_un5_copies")


@pytest.mark.parametrize("off", [0, 8], ids=["aligned", "off8"])
@pytest.mark.parametrize("name", CONVERSION_CASES)
def test_conversions_are_permutations(name, off):
    """kin_states_to_lib_dev / kin_states_from_lib_dev / kin_rates_to_lib_dev bit for bit, on aligned buffers (16-byte moves where
    N is even; the record-wise rate conversion where every record has two slots) and on buffers 8 bytes off (the 8-byte paths;
    the slot-wise gather). The two-piece layouts have N = 8193 / 8194: a ragged second piece of 1 / 2 species."""
    case = sc.TILED_CASES[name]
    h, net, ref, Ea, A, L = _handle(case)
    N, R, KL = ref.N, ref.R, L["k_len"]
    sp, slot = L["species_of_lib"], L["slot_of_reaction"]
    try:
        # the network has pairs the library flipped (the reverse became the record's forward reaction) and straight ones
        ev = np.arange(0, R - 1, 2)
        assert np.any((slot[ev + 1] % 2 == 0) & (slot[ev] == slot[ev + 1] + 1)) and np.any((slot[ev] % 2 == 0) & (slot[ev + 1] == slot[ev] + 1))
        if N > 8192:
            assert 0 < N - 8192 <= 2
        B = 5
        rng = np.random.default_rng(3)
        U_, K = rng.uniform(1, 2, (B, N)), rng.uniform(1, 2, (B, R))
        d_u, d_k = _dev(U_, off), _dev(K, off)
        d_ul, d_back, d_kl = _nan((B, N), off), _nan((B, N), off), _nan((B, KL), off)
        _sync()
        h.states_to_lib_dev(B, d_u.data_ptr(), d_ul.data_ptr())
        h.rates_to_lib_dev(B, d_k.data_ptr(), d_kl.data_ptr())
        _sync()
        h.states_from_lib_dev(B, d_ul.data_ptr(), d_back.data_ptr())
        _sync()
        assert np.array_equal(d_ul.cpu().numpy(), U_[:, sp])
        assert np.array_equal(d_back.cpu().numpy(), U_)
        kl = np.zeros((B, KL)); kl[:, slot] = K
        assert np.array_equal(d_kl.cpu().numpy(), kl)
        if off:        # the sweep refuses a k_lib row that is not 16-byte aligned (include/kinetica_hip.h), before any launch
            for call in (lambda: h.rhs_tiled_dev(B, d_ul.data_ptr(), d_back.data_ptr(), d_k_lib=d_kl.data_ptr()),
                         lambda: h.rhs_batched_klib_dev(B, d_u.data_ptr(), d_kl.data_ptr(), d_back.data_ptr())):
                with pytest.raises(capi.KineticaHipError) as e:
                    call()
                assert e.value.code == capi.KIN_ERR_INVALID_ARG
    finally:
        h.close()


@pytest.mark.parametrize("n_stops", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("name", ["t256_windows_odd_tail_singles", "t512_un5"])
def test_rate_table_in_library_order(name, n_stops):
    """kin_rate_table_lib_dev against kin_rate_table_dev permuted, bit for bit, at the edges of the kernel's blocks of 32 stops;
    slots no reaction owns (missing reverses, pad slots) are written and zero"""
    case = sc.TILED_CASES[name]
    h, net, ref, Ea, A, L = _handle(case)
    try:
        h.set_arrhenius(Ea, A, k_max=1e12)
        T = np.linspace(500.0, 1500.0, n_stops)
        d_tl, d_t = _nan((n_stops + 1, L["k_len"])), _nan((n_stops, ref.R))
        _sync()
        h.rate_table_lib_dev(T, d_tl.data_ptr())
        _sync()
        h.rate_table_dev(T, d_t.data_ptr())
        _sync()
        tl, t = d_tl.cpu().numpy(), d_t.cpu().numpy()
        assert np.isnan(tl[n_stops]).all()                       # nothing behind the last stop
        assert np.array_equal(tl[:n_stops][:, L["slot_of_reaction"]], t) and np.all(t > 0)
        unowned = np.ones(L["k_len"], bool); unowned[L["slot_of_reaction"]] = False
        assert unowned.any() == bool(case.expect["singles"])
        assert np.all(tl[:n_stops][:, unowned] == 0.0)
    finally:
        h.close()


def test_zz_report():
    """(last in the file) the largest error / bound per form on the random inputs, against the longdouble reference"""
    print("\ntiled error / bound:", {k: round(v, 3) for k, v in sorted(RATIOS.items())})
    assert all(v <= 1.0 for v in RATIOS.values())
