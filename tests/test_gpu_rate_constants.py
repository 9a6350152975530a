"""GPU tests of rate-constant formation in every form the device has, each against the long double reference and the classes
of tests/arrhenius_cases.py (never against another device path, except where two paths share their arithmetic and must
agree bit for bit):
  literal           arrhenius_kernel (kin_rates_at, kin_arrhenius_eval), flux_sweep_kernel / flux_seg_kernel with T
  fast, 512 table   rate_table_kernel (kin_rate_table, kin_rate_table_dev)
  fast, lib order   tiled_params_kernel + rate_table_lib_kernel (kin_rate_table_lib_dev)
  fast, 128 table   tiled_sweep_kernel<BS, TMODE> (kin_rhs_batched_T_dev, kin_rhs_tiled_dev with T)
Where a rate constant is only visible through a sweep or a flux pass the network is R disjoint reactions A_i -> B_i with
every u = 1: rate_i = k_i, du[2i+1] = k_i, du[2i] = -k_i, all exact. Every output buffer starts as NaN and is 64 elements
longer than the entry may write; the tail must keep its bits.

Measured on one MI355X (printed at the end of the module, pytest -s; 215 tests, 5 s): largest error / bound in the normal
class - literal form 0.91 (rates_at) and 0.77 (flux kernels, constructed inputs only), rate table 0.97, library-order table
0.77, sweep 0.77. Subnormal band: the literal form uses 0.02 of the bound beyond the scaled quantum, the fast forms stay
inside the quantum. Every exact class (zero_limit, cap_limit, literal_overflow, undefined) holds bit for bit in every form.

What the tests found (the parent commit fails 112 of the 212 tests of the forms, all at the T = 0 rows / states of the fast forms): with
1/RT = inf the quotient's residual correction is inf * 0, q is NaN for EVERY Ea and the form returned 0 - also for Ea < 0,
where the law's limit is +inf / k_max and the literal form returns it. On the host replay, additionally, the element with
|q| > 2.9e6 (Ea = -6e5 at T = 0.02): the table index leaves the int range there, right on the device only because its
conversion saturates; and a cap of +inf under an overflowing k_r: the capped form takes the reciprocal of x = 0 (NaN).
Fixed in exp_tab.hpp (q clamped at both ends, arrhenius_inv_RT caps 1/RT at 1e300 once per row / state) and in
kin_set_arrhenius (a cap at +inf is no cap). No other kernel was found wrong: every store path, grid edge, record kind and
pad slot holds.

The rate kernels inside a solve (all call the literal form's arrhenius_one): on the host-driven path a continuous profile's
pending temperature is consumed by rates_T_kernel / drates_T_kernel / rates_skip_T_kernel, which store k into the handle's
vector; after kin_integrator_init_continuous + one kin_integrator_step on a constant profile kin_get_rates returns what the
last of them stored (arrhenius_kernel runs only if a temperature is still pending at the end - the same bits then). The
resident kernel forms the rate constants of a temperature stop itself and kin_solve copies the last stop's back. Both are
compared bit for bit with kin_rates_at and with the literal form's classes (continuous_profile_kernels..., resident_kernel...).
Not covered: e_apply_rates_kernel (ensembles keep their members' k in the ensemble's own buffers) and the resident kernel under
a CONTINUOUS profile (its k stays in the trajectory's workspace; only stops are copied back).

Mutation check (one change at a time on a scratch build, selected through KIN_LIB_PATH, nothing of it kept): failing tests of
this file (of its 212 tests of the forms; the three solve-path tests came later), and what test_gpu_parity.py + test_gpu_tiled.py (40 tests) - the suite's view of these kernels before - did.
  1 rate_table_kernel always takes the double2 store: NOT run (a misaligned 16-byte store for every second row of an odd R).
    From the code: rate_table_every_row at R = 3, 511, 513, 1023, 1025 with n_stops >= 2 reads those rows; whether the
    hardware splits the store or faults, no test before had an odd R.
  2 the second reaction of a pair computed with e0 (double2 branch): 33 fail - rate_table at every even R (15 of its cases; odd R
    takes the other branch and passes), library_order (18: compared with rate_table_dev at an even R). Before: 9 of 40 failed.
  3 s1 without the min: NOT run (writes past the table). Instead the rt_s fill stops one row short (the block's last row on
    stale LDS): 65 fail - rate_table at every n_stops >= 1 (40), library_order (23), the forms pairwise. Before: 9 failed.
  4 exp_tab_t<128> without its extra series term: 30 fail - temperature_form_of_the_sweep (24), every_instantiation (6); the
    512-table tests pass. Before: all 40 passed. CPU: exp_tab_normal_results[128] and two more fail.
  5 one entry of exp2_tab.inc one ulp up (host replay only): table_entries_are_correctly_rounded, exp_tab_normal_results[512]
    (2.5 x 2^-53 exceeded) and the subnormal test fail on the CPU.
  6 `lo` dropped from the argument reduction: 94 fail in every fast-form test. Before: 12 failed. CPU: 6 of 10 fail.
  7 fmin(q, 800) removed (the index is masked into the table, nothing leaves LDS: run): 125 fail - every zero_limit element
    with q > 2.9e6 or infinite is NaN. Before: all 40 passed. CPU: the class rules fail for both tables.
  8 one Newton step removed after v_rcp_f64: 94 fail - rate_table (45), library_order (23), sweep (26): every capped case.
    Before: all 40 passed. CPU: passes (the replay's seed is a division) - the device tests are the check.
  9 tiled_params_kernel gives the missing reverse 0.0 under a cap: 58 fail - sweep (45) and every_instantiation (6): the
    reverse then contributes k_max; library_order (6: the two-slot disjoint network's missing slots hold k_max); the forms
    pairwise. Before: 5 failed (one_slot_records).
 10 rate_table_lib_kernel skips the pad slots: 3 fail - library_order on the disjoint network (R = 257: one pad). Before: 4 failed.
 11 x < 1e300 replaced by x < inf: 68 fail - zero_limit elements under a cap come out as ~1e-301 or NaN. Before: all 40 passed.
 12 arrhenius_inv_RT without its cap (the parent's arithmetic at T = 0): 112 fail, as on the parent. Before: all 40 passed.
 13 the lower clamp fmax(q, -800) removed: 112 fail on the device (the T = 0 rows: q = Ea * 1e300 overflows n); the CPU class
    rules fail as well (there also at |q| > 2.9e6). Before: all 40 passed."""
import ctypes
import time
from ctypes import POINTER, c_double

import numpy as np
import pytest
import torch

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from tests import arrhenius_cases as ac
from tests import linalg_cases as lc

pytestmark = pytest.mark.gpu

NAN_BITS = np.array(np.nan).view(np.int64)
TAIL = 64
CAP_IDS = [ac.cap_id(c) for c in ac.CAPS]
FORM_LABELS = ("literal rates_at", "literal flux", "fast 512 table", "fast 512 lib order", "fast 128 sweep")
MEASURED = {}       # (label, class) -> largest error / bound
COUNTS = {}         # label -> {class: elements}
DENSE_EA, DENSE_A = ac.dense_parameters(1025, 5)
DENSE_T = ac.dense_temperatures(65, 6)
_BASE, _NETS, NET_OF = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    for h in _NETS.values():
        h.close()
    _NETS.clear()
    print(f"\nrate constants: largest error / bound per form and class (module took {time.time() - t0:.1f} s)")
    for label in FORM_LABELS:
        if label in COUNTS:
            print(f"  {label:20s}", ", ".join(f"{c} {MEASURED.get((label, c), 0.0):.3f} ({n})" for c, n in COUNTS[label].items() if n))


# ---- cases: the classification is computed once per (inputs, cap, form) and indexed ----------------------------------------
def params(kind, R):
    return ac.edge_parameters(R) if kind == "edge" else (DENSE_EA[:R].copy(), DENSE_A[:R].copy())


def temps(kind, n):
    """(T[n], row index into the kind's temperature list)"""
    idx = np.arange(n) % len(ac.T_LIST) if kind == "edge" else np.arange(n)
    return (ac.T_LIST if kind == "edge" else DENSE_T)[idx].copy(), idx


def info_for(kind, cap, form, t_idx, R):
    key = (kind, ac.cap_id(cap), form)
    if key not in _BASE:
        Ea, A = ac.edge_parameters(40) if kind == "edge" else (DENSE_EA, DENSE_A)
        T = ac.T_LIST if kind == "edge" else DENSE_T
        _BASE[key] = ac.classify(Ea[None, :], A[None, :], T[:, None], cap[0], cap[1], form)
    cols = np.arange(R) % 40 if kind == "edge" else np.arange(R)
    return {k: v[np.ix_(np.asarray(t_idx), cols)] for k, v in _BASE[key].items()}


def judge(label, dev, info, what=""):
    """Every element of dev[rows][R] obeys its class's rule; records the margins and the class counts of `label`."""
    dev = np.asarray(dev)
    assert dev.shape == info["cls"].shape
    ok, ratio = ac.check(dev, info)
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (label, what, len(bad), [(tuple(i), ac.CLASSES[info["cls"][tuple(i)]], dev[tuple(i)], float(info["ref"][tuple(i)]),
                                                     info["q"][tuple(i)]) for i in bad[:4]])
    cnt = COUNTS.setdefault(label, dict.fromkeys(ac.CLASSES, 0))
    for i, c in enumerate(ac.CLASSES):
        m = info["cls"] == i
        cnt[c] += int(m.sum())
        if m.any():
            MEASURED[(label, c)] = max(MEASURED.get((label, c), 0.0), float(ratio[m].max()))
    assert (info["cls"] == ac.CLS["left_out"]).sum() <= 0.01 * dev.size


# ---- networks and buffers ------------------------------------------------------------------------------------------------------
def disjoint_net(R):
    return from_lists(2 * R, [[(2 * i, 1)] for i in range(R)], [[(2 * i + 1, 1)] for i in range(R)])


def rev_pairs_net(n):
    """n disjoint pairs A_i -> B_i, B_i -> A_i (forwards first): exact reverses, one two-slot library record per pair"""
    return from_lists(2 * n, [[(2 * i, 1)] for i in range(n)] + [[(2 * i + 1, 1)] for i in range(n)],
                      [[(2 * i + 1, 1)] for i in range(n)] + [[(2 * i, 1)] for i in range(n)])


def cutoff_net():
    """as test_gpu_tiled.test_one_slot_records_after_the_low_k_cutoff, at its smallest size"""
    net0, _, _ = synthetic_crn(300, 1500)
    keep = np.sort(np.random.default_rng(21).choice(1500, 1050, replace=False))
    return net0.subset(keep)


def network(kind, n):
    key = (kind, n)
    if key not in _NETS:
        net = {"disjoint": disjoint_net, "rev_pairs": rev_pairs_net, "pairs": lc.pairs_net}[kind](n) if kind != "cutoff" else cutoff_net()
        NET_OF[key] = net
        _NETS[key] = capi.HipNetwork.from_flat(net)
    return _NETS[key]


def _pd(a):
    return a.ctypes.data_as(POINTER(c_double))


def host_buf(n):
    return np.full(n + TAIL, np.nan)


def host_out(buf, n):
    assert np.all(buf[n:].view(np.int64) == NAN_BITS), "written past the end"
    return buf[:n]


def dev_buf(n):
    return torch.full((n + TAIL,), float("nan"), dtype=torch.float64, device="cuda")


def dev_out(buf, n):
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    return host_out(a, n)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _sync():
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the handle's own


def same_bits(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def rates_at(h, T):
    buf = host_buf(h.nr)
    h._chk(capi.lib().kin_rates_at(h.handle, float(T), _pd(buf)))
    return host_out(buf, h.nr)


def rate_table_host(h, T):
    n = len(T)
    buf = host_buf(n * h.nr)
    Tp = np.ascontiguousarray(np.append(T, 0.0))      # (a valid pointer for n = 0 too)
    h._chk(capi.lib().kin_rate_table(h.handle, _pd(Tp), n, _pd(buf)))
    return host_out(buf, n * h.nr).reshape(n, h.nr)


# ---- literal form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", ac.CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("R", [1, 255, 256, 257, 1025])
def test_literal_form_rates_at_and_arrhenius_eval(R, cap):
    h = network("disjoint", R)
    for kind, n_T in (("edge", len(ac.T_LIST)), ("dense", 4)):
        Ea, A = params(kind, R)
        h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
        T, idx = temps(kind, n_T)
        dev = np.stack([rates_at(h, t) for t in T])
        judge("literal rates_at", dev, info_for(kind, cap, "literal", idx, R), (kind, R))
        for s in (0, n_T - 1):          # the entry without a handle: the same kernel, the same bits
            buf = host_buf(R)
            st = capi.lib().kin_arrhenius_eval(_pd(Ea), _pd(A), R, float("nan") if cap[0] is None else cap[0], cap[1], float(T[s]), _pd(buf))
            assert st == capi.KIN_OK and same_bits(host_out(buf, R), dev[s])


@pytest.mark.parametrize("cap", ac.CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("R", [1, 2, 257, 1025])
def test_literal_form_inside_the_flux_kernels(R, cap):
    """flux_sweep_kernel (per-state rates) and flux_seg_kernel (one state per segment: the sum is its only term) form k from
    T[b] themselves, two reactions per double2 of Ea / A - an odd R leaves the last one alone. Bit for bit what
    arrhenius_kernel gives, and each in its class."""
    h = network("disjoint", R)
    Ea, A = params("edge", R)
    h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
    u = np.ones((3, 2 * R))
    L = capi.lib()
    for idx in ([0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 0, 5]):
        T = ac.T_LIST[idx].copy()
        buf = host_buf(3 * R)
        h._chk(L.kin_flux_batched(h.handle, 3, _pd(u), None, 0, None, _pd(T), None, None, _pd(buf)))
        rates = host_out(buf, 3 * R).reshape(3, R)
        judge("literal flux", rates, info_for("edge", cap, "literal", idx, R), ("flux_batched", R))
        buf2 = host_buf(3 * R)
        h._chk(L.kin_flux_segmented(h.handle, 3, 1, None, _pd(u), None, 0, None, _pd(T), None, _pd(buf2)))
        seg = host_out(buf2, 3 * R).reshape(3, R)
        for b in range(3):
            want = rates_at(h, T[b])
            assert same_bits(rates[b], want), ("flux_batched", b)
            # (a segment's sum starts from +0.0: a rate of -0.0 would come out as +0.0; rate constants are never negative)
            assert same_bits(seg[b], want), ("flux_segmented", b)


# ---- fast form, 512-entry table: the rate table -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_stops", [0, 1, 31, 32, 33, 65])
@pytest.mark.parametrize("R", [1, 2, 3, 511, 512, 513, 1023, 1024, 1025])
def test_rate_table_every_row_odd_and_even_row_lengths(R, n_stops):
    """rate_table_kernel: 512 reactions per workgroup, 32 rows per grid.y, double2 stores for an even R and scalar stores
    for an odd one (every second row of an odd table is misaligned for 16 bytes). Every element of every row in its class;
    the device-buffer entry and the host download agree bit for bit."""
    h = network("disjoint", R)
    for kind in ("edge", "dense"):
        Ea, A = params(kind, R)
        T, idx = temps(kind, n_stops)
        for cap in ac.CAPS:
            h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
            tab = rate_table_host(h, T)
            d = dev_buf(n_stops * R)
            _sync()
            Tp = np.ascontiguousarray(np.append(T, 0.0))
            h._chk(capi.lib().kin_rate_table_dev(h.handle, _pd(Tp), n_stops, ctypes.c_void_p(d.data_ptr())))
            tab_d = dev_out(d, n_stops * R).reshape(n_stops, R)
            assert same_bits(tab, tab_d)
            if n_stops:
                judge("fast 512 table", tab, info_for(kind, cap, "fast", idx, R), (kind, R, n_stops, cap))


# ---- fast form in library order --------------------------------------------------------------------------------------------------
LIB_NETS = [("rev_pairs", 1, None), ("rev_pairs", 255, None), ("rev_pairs", 256, None), ("rev_pairs", 257, None), ("pairs", 257, None),
            ("disjoint", 257, None), ("disjoint", 257, "0"), ("cutoff", 0, None)]


@pytest.mark.parametrize("n_stops", [1, 32, 33])
@pytest.mark.parametrize("kind,n,singles", LIB_NETS, ids=[f"{k}{n}{'-two_slot' if s else ''}" for k, n, s in LIB_NETS])
def test_library_order_table_slots_pads_and_missing_reverses(monkeypatch, kind, n, singles, n_stops):
    """tiled_params_kernel + rate_table_lib_kernel. rev_pairs: two-slot records (256 records per workgroup: 255 / 256 / 257);
    pairs_net (2B -> A is no exact reverse of A -> B) and the disjoint network: one-slot records; the disjoint network with
    KIN_TILED_SINGLES=0: two-slot records whose reverse is missing (the constant that makes k = 0, +inf under a cap); the
    network after the low-k cutoff: both kinds in one row. A reaction's slot holds what rate_table_kernel gives, bit for bit;
    a pad slot and the slot of a missing reverse hold exactly +0.0 at every T (T = 0 included); no other slot exists."""
    if singles is not None:
        monkeypatch.setenv("KIN_TILED_SINGLES", singles)          # read when the layout is built
        net = disjoint_net(n)
        h = capi.HipNetwork.from_flat(net)
    else:
        h, net = network(kind, n), NET_OF[(kind, n)]
    try:
        R = h.nr
        lay, hl = h.lib_layout(), capi.lib_layout_host(net)
        KL, slot, P = lay["k_len"], lay["slot_of_reaction"], lay["records"]
        assert lay["windows"] == 1 and hl["T"] == 1 and hl["P"] == P and hl["k_len"] == KL and np.array_equal(hl["slot_of_reaction"], slot)
        # one segment (tiled.cpp): its first n2 records take two slots, the rest one; one pad slot where that leaves the row odd
        n2 = int(hl["seg_k"][0][1])
        used = 2 * n2 + (P - n2)
        assert KL - used in (0, 1) and KL % 2 == 0
        pads = np.arange(used, KL)
        owned = np.zeros(KL, bool); owned[slot] = True
        assert owned.sum() == R and not owned[pads].any()
        missing = np.nonzero(~owned[:used])[0]
        assert np.all(missing < 2 * n2)          # only a two-slot record has a slot without a reaction
        if kind == "rev_pairs":
            assert n2 == P and KL == R and len(missing) == 0
        elif singles == "0":
            assert n2 == P and len(missing) == R
        elif kind in ("pairs", "disjoint"):
            assert n2 == 0 and len(pads) == (R & 1)
        else:
            assert 0 < n2 < P and len(missing) > 0
        Ea, A = params("edge", R)
        T, idx = temps("edge", n_stops)
        for cap in ac.CAPS:
            h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
            d_l, d_t = dev_buf(n_stops * KL), dev_buf(n_stops * R)
            _sync()
            h.rate_table_lib_dev(T, d_l.data_ptr())
            h.rate_table_dev(T, d_t.data_ptr())
            tl = dev_out(d_l, n_stops * KL).reshape(n_stops, KL)
            t = dev_out(d_t, n_stops * R).reshape(n_stops, R)
            assert same_bits(tl[:, slot], t), cap
            for name, cols in (("pad", pads), ("missing reverse", missing)):
                z = tl[:, cols]
                assert np.all(z == 0.0) and not np.signbit(z).any(), (name, cap)
            judge("fast 512 lib order", tl[:, slot], info_for("edge", cap, "fast", idx, R), (kind, n, n_stops, cap))
    finally:
        if singles is not None:
            h.close()          # (the other handles are the module's, closed at its end)


# ---- fast form, 128-entry table: rate constants formed inside the sweep ---------------------------------------------------
def _sweep(h, B, T):
    """du[B][N] of the disjoint network at u = 1 through both entries (caller order; library order)"""
    N = h.n
    lay = h.lib_layout()
    d_u, d_T = torch.ones((B, N), dtype=torch.float64, device="cuda"), _dev(T)
    d_a, d_b = dev_buf(B * N), dev_buf(B * N)
    _sync()
    h.rhs_batched_T_dev(B, d_u.data_ptr(), d_T.data_ptr(), d_a.data_ptr())
    h.rhs_tiled_dev(B, d_u.data_ptr(), d_b.data_ptr(), d_T=d_T.data_ptr())
    du = dev_out(d_a, B * N).reshape(B, N)
    du_lib = dev_out(d_b, B * N).reshape(B, N)
    assert same_bits(du[:, lay["species_of_lib"]], du_lib)
    return du, lay


def _judge_sweep(du, cap, idx, R, what):
    k = du[:, 1::2]
    assert np.array_equal(du[:, 0::2], -k, equal_nan=True), what
    judge("fast 128 sweep", k, info_for("edge", cap, "fast", idx, R), what)


@pytest.mark.parametrize("cap", ac.CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("B", [1, 7, 130])
@pytest.mark.parametrize("R", [1, 64, 257, 1025])
def test_temperature_form_of_the_sweep(R, B, cap):
    """tiled_sweep_kernel<256, TMODE>: du[2i+1] = k_i(T[b]) in its class, du[2i] = -du[2i+1]. Every record's reverse is
    missing: its constant must contribute exactly 0 at every T, T = 0 included (a NaN there would show in du)."""
    h = network("disjoint", R)
    Ea, A = params("edge", R)
    h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
    T, idx = temps("edge", B)
    du, lay = _sweep(h, B, T)
    assert lay["block"] == 256
    _judge_sweep(du, cap, idx, R, (R, B, cap))


@pytest.mark.parametrize("R,BS,UN", [(257, 256, 5), (1025, 256, 10), (1151, 512, 5), (1281, 512, 10), (2426, 1024, 5), (2561, 1024, 10)])
def test_every_instantiation_of_the_temperature_form(R, BS, UN):
    """launch_tiled_sweep picks tiled_sweep_kernel<BS, true, UN, false>: BS from the species count (N = 2 R: 256 up to 2300,
    512 up to 4850, 1024 above), UN = 5 while the staged-in set (here the whole state: hubs = N) has at most 5 BS entries,
    else 10. The layout reports BS and the hub count, not UN: which UN ran is INFERRED here with the launcher's own rule, not
    observed - what the test adds is a run of each size that selects another instantiation, every element in its class."""
    h = network("disjoint", R)
    Ea, A = params("edge", R)
    T, idx = temps("edge", 7)
    for cap in (ac.CAPS[0], ac.CAPS[2]):
        h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
        du, lay = _sweep(h, 7, T)
        assert lay["block"] == BS and lay["windows"] == 1 and lay["hubs"] == 2 * R
        assert (5 if lay["hubs"] <= 5 * BS else 10) == UN
        _judge_sweep(du, cap, idx, R, (R, BS, UN, cap))


# ---- the literal form inside a solve ----------------------------------------------------------------------------------------------
def _solve_net():
    """257 reactions (odd) on 100 species: a size the resident kernel takes, with the generator's own parameters"""
    net0, Ea, A = synthetic_crn(100, 258)
    keep = np.arange(257)
    return net0.subset(keep), Ea[keep], A[keep]


def _kp(t1, chunkstep=None):
    return capi.KinParams(tspan0=0.0, tspan1=t1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0,
                          solve_chunks=int(chunkstep is not None), ban_negatives=0, solve_chunkstep=chunkstep or t1, maxiters=100000,
                          save_interval=-1.0)


def _judge_literal(label, k, Ea, A, T, cap):
    info = ac.classify(Ea[None, :], A[None, :], np.array([[T]]), cap[0], cap[1], "literal")
    ok, _ = ac.check(k[None, :], info)
    assert ok.all(), (label, np.nonzero(~ok))
    assert (info["cls"] == ac.CLS["normal"]).any()


@pytest.mark.parametrize("cap", [ac.CAPS[1], ac.CAPS[2]], ids=[CAP_IDS[1], CAP_IDS[2]])
def test_continuous_profile_kernels_store_the_literal_rate_constants(monkeypatch, cap):
    """Host-driven integrator under a constant profile T(t) = T0: the restart's f0 / J and the step's corrector consume the
    pending temperature through rates_T_kernel, drates_T_kernel and rates_skip_T_kernel, each of which stores k; kin_get_rates
    then returns the last one's. Equal to arrhenius_kernel's bit for bit, R = 257 (two workgroups, the second one partial)."""
    monkeypatch.setenv("KIN_RESIDENT", "0")
    net, Ea, A = _solve_net()
    h = capi.HipNetwork.from_flat(net)
    try:
        h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
        u0 = np.zeros(net.n_species); u0[0] = 1.0
        for T0 in (900.0, 1371.5):
            h.integrator_init_continuous(_kp(1e-3), u0, [0.0, 1e-3], [T0, T0])
            h.integrator_step(1)
            t, _, rc, st = h.integrator_state(with_u=False)
            assert rc == 0 and t > 0.0 and st["n_rhs"] > 0 and st["n_jac"] > 0
            k = h.get_rates()                       # before kin_rates_at, which overwrites the handle's k
            assert same_bits(k, rates_at(h, T0)), T0
            _judge_literal("continuous", k, Ea, A, T0, cap)
    finally:
        h.close()


def test_resident_kernel_forms_the_rate_constants_of_a_stop(monkeypatch):
    """kin_solve with temperature stops on a resident size: the kernel evaluates arrhenius_one at every stop in its own
    workspace and the call copies the last stop's k back into the handle."""
    monkeypatch.delenv("KIN_RESIDENT", raising=False)
    net, Ea, A = _solve_net()
    cap = ac.CAPS[1]
    h = capi.HipNetwork.from_flat(net)
    try:
        h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
        u0 = np.zeros(net.n_species); u0[0] = 1.0
        Ta, Tb = 800.0, 1250.25
        # (chunkwise: the resident kernel takes calls whose save times form a grid)
        t, u, rc, st, status = h.solve(_kp(1e-3, 5e-4), u0, tstops=[0.0, 5e-4], T_stops=[Ta, Tb])
        assert status == capi.KIN_OK and rc == 0 and st["n_restarts"] >= 1
        assert st["lu_slots"] <= 64                 # the resident path (its LU cache has 64 slots at most; host-driven: more)
        k = h.get_rates()
        assert same_bits(k, rates_at(h, Tb))
        _judge_literal("resident stop", k, Ea, A, Tb, cap)
    finally:
        h.close()


# ---- all forms on the same inputs --------------------------------------------------------------------------------------------------
def test_the_forms_agree_pairwise_within_their_bounds():
    R, n_T = 257, 6
    h = network("disjoint", R)
    Ea, A = params("dense", R)
    T, idx = temps("dense", n_T)
    n_normal = 0
    for cap in (ac.CAPS[0], ac.CAPS[1], ac.CAPS[2]):
        h.set_arrhenius(Ea, A, k_max=cap[0], t_mult=cap[1])
        lay = h.lib_layout()
        lit = np.stack([rates_at(h, t) for t in T])
        buf = host_buf(n_T * R)
        h._chk(capi.lib().kin_flux_batched(h.handle, n_T, _pd(np.ones((n_T, 2 * R))), None, 0, None, _pd(T), None, None, _pd(buf)))
        flux = host_out(buf, n_T * R).reshape(n_T, R)
        tab = rate_table_host(h, T)
        d_l = dev_buf(n_T * lay["k_len"])
        _sync()
        h.rate_table_lib_dev(T, d_l.data_ptr())
        lib = dev_out(d_l, n_T * lay["k_len"]).reshape(n_T, -1)[:, lay["slot_of_reaction"]]
        sweep = _sweep(h, n_T, T)[0][:, 1::2]
        forms = {"literal": lit, "flux": flux, "table": tab, "lib": lib, "sweep": sweep}
        il, ifa = info_for("dense", cap, "literal", idx, R), info_for("dense", cap, "fast", idx, R)
        m = (il["cls"] == ac.CLS["normal"]) & (ifa["cls"] == ac.CLS["normal"])
        n_normal += int(m.sum())
        ref = il["ref"].astype(np.float64)
        names = list(forms)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                assert np.all(np.abs(forms[a] - forms[b])[m] <= (2 * il["b"] * ref)[m]), (a, b, cap)
        assert same_bits(lit, flux) and same_bits(tab, lib)
    assert n_normal > 1000


def test_every_class_occurs_in_every_form():
    """(after the tests above: they record what they classified)"""
    assert COUNTS, "run together with the tests of the forms"
    for label, cnt in COUNTS.items():
        assert all(cnt[c] > 0 for c in ac.CLASSES if c != "left_out"), (label, cnt)
