"""GPU tests of the flux passes in every instantiation and at every boundary of their dispatch: the cases of flux_cases.py through
kin_flux_batched_dev (flux and rates, and each alone) and kin_flux_segmented_dev (S = 5, L = 7, seg_n = 7, 0, 3, 1, 5, NaN behind
seg_n) on buffers made by torch, against the oracle's per-state rates and math.fsum of w_b rate_b (references and bounds:
flux_cases.py; no tolerance is new here). Before a result is compared, the instantiation that ran is asserted from
kin_flux_plan_host, fed with the handle's compute units and the low bits of the real pointers.

Every call runs on B in {1, G - 1, 2 G + 3} states (G: the state slices of the plan; B = 3 for N >= 20 479) with rate constants
or a temperature of its own per state, once on the log-uniform states of test_gpu_flux.py (derived bounds) and once on the exact
class (np.array_equal). Every output starts as NaN and is 64 elements longer than the call may write - one more in front where
the buffer starts 8 bytes behind a 16-byte boundary: what lies outside must keep its bits (the kernels' stores are
unconditional and clamped). The per-state and the segmented pass see the same states and sources and each sits within its own
bound of the same reference.

Measured on an MI355X (pytest -s prints a line per test): the file's 128 tests - 2 828 calls of the two passes - take 22 s, the
slowest (pointers-300x1500, 81 calls) 2.3 s. Largest error / bound on the log-uniform states, per case group:
  group                          per-state rates   flux    segmented flux
  row cases, k given                  0.873        0.137       0.282
  row cases, temperature form         0.244        0.071       0.158
  size cases                          0.803        0.277       0.304
  pointer cases                       0.740        0.059       0.255
The exact class agreed bit for bit everywhere. No case found the kernels wrong.

Mutation check (one change of flux_kernels.hip at a time in a scratch build selected through KIN_LIB_PATH, nothing of it
committed, one process per mutant; every mutation keeps all index ranges and barriers - a change that could move an address out
of its buffer, such as a wider clamp or a missing min(), was not run). Failing tests of this file (of 128), and of
test_gpu_flux.py + test_gpu_flux_segmented.py as they were before it (of 91):
  mutation                                                           here   which                                        before
  1 ROWS 8 with rates: the second k batch loads the first's rows        4   per-state path0-R8194, R14337, R14338, R16386     0
  2 path 1 staging stops at i < N - 1                                  44   every path 1 case, both passes (301-species      7
                                                                            rows, odd N, N 10 242 .. 20 478, the state         (N = 3 hand values, test_odd_species_count)
                                                                            pointer 8 bytes off); none on paths 0, 2
  3 path 0 staging store i < N - 2                                     52   every path 0 case, both passes                   77
  4 K8 loads kb[2 jc] for both reactions of a pair                    116   every case with k given, both passes              2
                                                                                                                             (the two odd-R tests)
  5 RATES 2 stores r0 for every odd reaction                           64   every per-state test                              1
                                                                                                                             (the odd-R test)
  6 path 2 reads q.y for the second reaction's second operand          34   every path 2 case, both passes                   12
  7 flux_reduce_kernel without its remainder loop (G % 8 != 0)         64   every per-state test                             28
  8 flux_seg_kernel loads k at j == 0 only                             64   every segmented test                             18
  9 the temperature form evaluates ea[0], aa[0] for every row          12   the six temperature row cases, both passes        9
                                                                                                                             (1000x5000 T, T_kmax; test_one_part_of_four_rows)
The existing files did catch mutations 2, 6 and 9 (at N = 3, with ROWS 1, and on path 0), not on the instantiations named in the
table: under 1 they pass, under 4 and 5 only their one odd-R test fails, under 2 nothing with a second trip of the staging loop.
The temperature form runs without k_max here. With k_max = 1e12 nearly every rate constant of these networks sits at the cap,
within 2e-13 of each other: a first version of this file with the cap let the segmented pass of path1-R2050-T pass under 9
(11 failures), its one pair of the second row taking pair 0's constants; the cap's arithmetic is test_gpu_rate_constants.py's."""
import numpy as np
import pytest

from kinetica_jl_amd import capi

import flux_cases as fc

pytestmark = pytest.mark.gpu
# cases of one network next to each other: its handle, inputs and references are made once
CASES = sorted(fc.all_cases(), key=lambda c: (c.kind, c.n, c.R, c.temperature, c.name))
NAN_BITS = np.array([np.nan]).view(np.uint64)[0]
GUARD = 64
DEV = "cuda:0"


def _torch():
    import torch
    return torch


def _dev(a, off=0, dtype=None):
    """A copy of `a` on the device that starts `off` bytes behind a 16-byte boundary: (tensor that owns it, pointer)."""
    torch = _torch()
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 2, dtype=dtype or torch.float64, device=DEV)
    view = buf[off // 8: off // 8 + a.size]
    view.copy_(torch.from_numpy(a.ravel()))
    assert view.data_ptr() % 16 == off
    return buf, view.data_ptr()


class Out:
    """An output of n doubles, NaN everywhere, GUARD more behind it (and `off` bytes in front of it)."""

    def __init__(self, n, off=0):
        torch = _torch()
        self.n, self.lo = n, off // 8
        self.buf = torch.full((self.lo + n + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
        self.ptr = self.buf.data_ptr() + off
        assert self.ptr % 16 == off

    def get(self):
        """The n values; asserts that nothing outside them was written."""
        a = self.buf.cpu().numpy()
        outside = np.concatenate([a[:self.lo], a[self.lo + self.n:]]).view(np.uint64)
        assert len(outside) == self.lo + GUARD and np.all(outside == NAN_BITS), "a store outside the output"
        return a[self.lo:self.lo + self.n]


class Shared:
    """What the cases of one network share: handle, inputs of both classes on the device (aligned and 8 bytes off), references."""

    def __init__(self, case):
        self.net, self.Ea, self.A = case.network()
        self.h = capi.HipNetwork.from_flat(self.net)
        self.h.set_arrhenius(self.Ea, self.A)
        self.n_cu = self.h.compute_units()
        self.B = fc.S_ * fc.L_ if case.n >= fc.BIG_N else 2 * self.n_cu + 3
        self._data = {}

    def data(self, case, cls):
        if cls not in self._data:
            torch = _torch()
            d = fc.Data(case, self.B, cls)
            dev = {}
            for off in (0, 8):
                dev["U", off] = _dev(d.U, off)
                dev["K", off] = _dev(d.K, off)
                dev["K3", off] = _dev(d.K3, off)
            sU, sw, sT, sK, srow = d.seg_inputs()
            for off in (0, 8):
                dev["sU", off] = _dev(sU, off)
                dev["sK", off] = _dev(sK, off)
            dev["T"], dev["w"], dev["row"] = _dev(d.T), _dev(d.w), _dev(d.row3, dtype=torch.int64)
            dev["sT"], dev["sw"], dev["srow"] = _dev(sT), _dev(sw), _dev(srow, dtype=torch.int64)
            dev["segn"] = _dev(fc.SEG_N, dtype=torch.int64)
            self._data[cls] = (d, dev)
        return self._data[cls]

    def close(self):
        self._data.clear()
        self.h.close()


_shared = {}


def shared(case):
    key = (case.kind == "size", case.n, case.R, case.layout)
    if key not in _shared:
        for s in _shared.values():
            s.close()
        _shared.clear()
        _shared[key] = Shared(case)
    return _shared[key]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for s in _shared.values():
        s.close()
    _shared.clear()


def _source(sh, d, dev, v, seg):
    """(keywords of the device entry, low bits of the k pointer) of variant v."""
    p = "s" if seg else ""
    if v.ksrc == "T":
        return dict(d_T=dev[p + "T"][1]), 0
    if v.ksrc == "k":
        ptr = dev[p + "K", v.k_off][1]
        return dict(d_k=ptr), ptr % 16
    if v.ksrc == "k_row":
        ptr = dev["K3", v.k_off][1]
        return dict(d_k=ptr, d_k_row=dev[p + "row"][1]), ptr % 16
    sh.h.set_rates(d.k0)          # the handle's own row: an allocation of the library's, aligned
    return {}, 0


def _classes(v):
    return ("log",) if v.ksrc == "T" else ("log", "exact")


def _compare(got, ref, bound, exact, worst, what):
    if exact:
        assert np.array_equal(got, ref), what
    else:
        err = np.abs(got - ref)
        worst[0] = max(worst[0], float(np.max(err / bound)))
        assert np.all(err <= bound), what


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_per_state_pass(case, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("KIN_FLUX_LDS", case.lds)
    monkeypatch.delenv("KIN_FLUX_ROWS", raising=False)
    sh = shared(case)
    R, N = case.R, case.n
    stream = torch.cuda.current_stream().cuda_stream
    worst, runs = {"rates": [0.0], "flux": [0.0]}, 0
    for v in case.variants:
        for cls in _classes(v):
            d, dev = sh.data(case, cls)
            for B in fc.batch_sizes(N, fc.g_max(sh.n_cu, case.parts)):
                kw, k_bits = _source(sh, d, dev, v, False)
                u_ptr = dev["U", v.u_off][1]
                flux = Out(R) if v.out != "rates" else None
                rates = Out(B * R, v.r_off) if v.out != "flux" else None
                q = fc.query(case, v, sh.n_cu, B, u_bits=u_ptr % 16, k_bits=k_bits, rates_bits=rates.ptr % 16 if rates else None)
                what = f"{case} {v} {cls} B={B}"
                assert fc.as_inst(q) == case.inst(v), what
                torch.cuda.synchronize()      # torch's fills run on torch's stream
                sh.h.flux_batched_dev(B, u_ptr, d_w=dev["w"][1], d_flux=flux.ptr if flux else 0, d_rates=rates.ptr if rates else 0,
                                      stream=stream, **kw)
                torch.cuda.synchronize()
                runs += 1
                if rates:
                    _compare(rates.get().reshape(B, R), d.rates(v.ksrc)[:B], d.rates_bound(v.ksrc, B), cls == "exact", worst["rates"], what)
                if flux:
                    ref, bound = d.flux(v.ksrc, B)
                    _compare(flux.get(), ref, bound, cls == "exact", worst["flux"], what)
    print(f"{case}: {runs} calls, max err/bound rates {worst['rates'][0]:.3f} flux {worst['flux'][0]:.3f}")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_segmented_pass(case, monkeypatch):
    torch = _torch()
    monkeypatch.setenv("KIN_FLUX_LDS", case.lds)
    monkeypatch.delenv("KIN_FLUX_ROWS", raising=False)
    sh = shared(case)
    R = case.R
    stream = torch.cuda.current_stream().cuda_stream
    worst, runs = [0.0], 0
    for v in case.seg_variants:
        for cls in _classes(v):
            d, dev = sh.data(case, cls)
            kw, k_bits = _source(sh, d, dev, v, True)
            u_ptr = dev["sU", v.u_off][1]
            out = Out(fc.S_ * R)
            q = fc.query(case, v, sh.n_cu, fc.S_ * fc.L_, segmented=True, u_bits=u_ptr % 16, k_bits=k_bits)
            what = f"{case} {v} {cls}"
            assert fc.as_seg_inst(q) == case.seg_inst(v), what
            torch.cuda.synchronize()
            sh.h.flux_segmented_dev(fc.S_, fc.L_, u_ptr, out.ptr, d_seg_n=dev["segn"][1], d_w=dev["sw"][1], stream=stream, **kw)
            torch.cuda.synchronize()
            runs += 1
            got = out.get().reshape(fc.S_, R)
            ref, bound = d.seg_flux(v.ksrc)
            assert np.all(np.isfinite(got)) and np.all(got[fc.SEG_N == 0] == 0.0), what
            _compare(got, ref, bound, cls == "exact", worst, what)
    print(f"{case} segmented: {runs} calls, max err/bound {worst[0]:.3f}")
