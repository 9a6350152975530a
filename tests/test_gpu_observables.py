"""GPU tests of the observables pass on caller-given blocks: kin_observables_segmented (host arrays) and
kin_observables_segmented_dev (buffers made by torch, sentinel-filled with a guard behind them) over every case of
observable_cases.py and every pitch of the case, bit for bit against observable_cases.ref_observables (a NaN by its place, -0.0
as -0.0). Both paths - the rows staged into LDS, and KIN_OBSERVABLES_LDS=0, the gather from global memory - and
KIN_OBSERVABLES_ROWS 1, 3, 16 and unset give the same bytes: a form's class depends on its length only. Every entry of the
written range is written, nothing behind it is touched, a repeat gives the same bytes, buffers 8 bytes off a 16-byte boundary
give the same bytes, and every refused argument has its status and leaves the handle usable."""
import numpy as np
import pytest

import member_stats_cases as mc
import observable_cases as oc
from kinetica_jl_amd import capi

pytestmark = pytest.mark.gpu
SENTINEL = -9.75e99      # what the device entry's output holds before the call: every entry must be written
GUARD = 67               # entries behind the device output that must keep the sentinel


def network(N, index_base=0):
    """A handle with N species (the pass never looks at the reactions)."""
    if N == 1:
        return capi.HipNetwork(1, [0, 1], [index_base], [1], [0, 1], [index_base], [1], index_base=index_base)
    return capi.HipNetwork(*mc.chain_network(N, index_base), index_base=index_base)


def observables_dev(h, u, forms, num, den, pitch, seg_n=None, offset=0):
    """kin_observables_segmented_dev on torch buffers; returns out[S][L][pitch] and checks the guard behind it. offset: doubles
    by which the states and the output start behind their 16-byte aligned allocations."""
    import torch
    dev = torch.device("cuda")
    S, L, N = u.shape
    n_out = S * L * pitch
    d_u = torch.zeros(u.size + offset, dtype=torch.float64, device=dev)
    d_u[offset:] = torch.tensor(np.ascontiguousarray(u).ravel(), dtype=torch.float64, device=dev)
    d_n = None if seg_n is None else torch.tensor(np.ascontiguousarray(seg_n), dtype=torch.int64, device=dev)
    out = torch.full((offset + n_out + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    assert d_u.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the stream it is handed
    h.observables_segmented_dev(S, L, d_u.data_ptr() + 8 * offset if u.size else 0, *forms, num, den, pitch,
                                out.data_ptr() + 8 * offset if n_out else 0, d_seg_n=0 if d_n is None else d_n.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[:offset] == SENTINEL) and np.all(out[offset + n_out:] == SENTINEL)
    assert not np.any(out[offset:offset + n_out] == SENTINEL)      # every column of every row was written
    return out[offset:offset + n_out].reshape(S, L, pitch)


def _knobs(monkeypatch, rows, lds):
    for name, value in (("KIN_OBSERVABLES_ROWS", rows), ("KIN_OBSERVABLES_LDS", lds)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


@pytest.mark.parametrize("case", oc.CASES, ids=[c["id"] for c in oc.CASES])
def test_every_case_bit_for_bit(case, monkeypatch):
    u, seg_n, forms, num, den = case["u"], case["seg_n"], case["forms"], case["num"], case["den"]
    h = network(u.shape[2])
    checked = 0
    for pitch in case["pitches"]:
        ref = oc.at(case, pitch)
        for lds in oc.LDS:
            for rows in oc.ROWS:
                _knobs(monkeypatch, rows, lds)
                host = h.observables_segmented(u, *forms, num, den, pitch=pitch, seg_n=seg_n)
                dev = observables_dev(h, u, forms, num, den, pitch, seg_n=seg_n)
                for name, got in (("host", host), ("device", dev)):
                    assert got.shape == ref.shape and oc.same_bits(got, ref), (case["id"], pitch, lds, rows, name)
                checked += 1
    assert checked == len(case["pitches"]) * len(oc.LDS) * len(oc.ROWS)
    _knobs(monkeypatch, None, None)
    # a second call repeats the bytes; buffers 8 bytes off a 16-byte boundary give the same ones
    pitch = case["pitches"][-1]
    a = h.observables_segmented(u, *forms, num, den, pitch=pitch, seg_n=seg_n)
    b = h.observables_segmented(u, *forms, num, den, pitch=pitch, seg_n=seg_n)
    assert a.tobytes() == b.tobytes()
    for lds in oc.LDS:
        _knobs(monkeypatch, None, lds)
        off = observables_dev(h, u, forms, num, den, pitch, seg_n=seg_n, offset=1)
        assert off.tobytes() == a.tobytes(), (case["id"], lds)
    h.close()


def test_one_based_species_and_a_changed_plan():
    """A handle of index base 1 takes the species of the forms in that base; a call with other forms, then the first ones again,
    gives the first bytes (the handle's cached plan follows the call)."""
    case = oc.CASES[6]
    u, seg_n, (ptr, idx, w), num, den = case["u"], case["seg_n"], case["forms"], case["num"], case["den"]
    h = network(u.shape[2], index_base=1)
    G = len(num)
    first = h.observables_segmented(u, ptr, idx + 1, w, num, den, seg_n=seg_n)
    assert oc.same_bits(first, oc.at(case, G))
    w2 = w.copy(); w2[w2 == 0.0] = 0.0      # -0.0 weights become 0.0: other bits, the same values
    other = h.observables_segmented(u, ptr, idx + 1, w2 * 2.0, num, den, seg_n=seg_n)
    ref2 = oc.ref_observables(u, seg_n, (ptr, idx, w2 * 2.0), num, den, G)
    assert oc.same_bits(other, ref2)
    again = h.observables_segmented(u, ptr, idx + 1, w, num, den, seg_n=seg_n)
    assert again.tobytes() == first.tobytes()
    h.close()


def test_a_segment_does_not_depend_on_its_neighbours():
    case = oc.CASES[10]
    u, seg_n, forms, num, den = case["u"], case["seg_n"], case["forms"], case["num"], case["den"]
    h = network(u.shape[2])
    full = h.observables_segmented(u, *forms, num, den, seg_n=seg_n)
    for s in range(u.shape[0]):
        alone = h.observables_segmented(u[s:s + 1], *forms, num, den, seg_n=seg_n[s:s + 1])
        assert alone[0].tobytes() == full[s].tobytes(), s
    h.close()


def test_empty_calls_write_nothing():
    h = network(5)
    ptr, idx, w, num, den = [0, 2], [0, 3], [1.0, 2.0], [0], [-1]
    assert h.observables_segmented(np.zeros((0, 4, 5)), ptr, idx, w, num, den).shape == (0, 4, 1)
    assert h.observables_segmented(np.zeros((3, 0, 5)), ptr, idx, w, num, den).shape == (3, 0, 1)
    assert h.observables_segmented(np.ones((2, 4, 5)), ptr, idx, w, [], [], pitch=0).shape == (2, 4, 0)
    out = observables_dev(h, np.ones((2, 4, 5)), (ptr, idx, w), [], [], 0)
    assert out.size == 0
    h.close()


def test_statuses_of_refused_arguments():
    N, S, L = 5, 2, 4
    h = network(N)
    lib = capi.lib()
    u = np.arange(1.0, S * L * N + 1).reshape(S, L, N)
    seg = np.array([L, 2], np.int64)
    i64 = lambda *v: np.array(v, np.int64)
    ptr, idx, w, num, den = i64(0, 2, 3), i64(0, 3, 4), np.array([1.0, 2.0, -1.0]), i64(0, 1, 0), i64(-1, -1, 1)
    out = np.full((S, L, 4), SENTINEL)
    pd, p64 = capi._pd, capi._p64

    def call(S_=S, L_=L, seg_n=seg, u_=u, H=2, ptr_=ptr, idx_=idx, w_=w, G=3, num_=num, den_=den, pitch=4, out_=out):
        return lib.kin_observables_segmented(h.handle, S_, L_, p64(seg_n), pd(u_), H, p64(ptr_), p64(idx_), pd(w_), G, p64(num_), p64(den_),
                                             pitch, pd(out_))

    assert call() == capi.KIN_OK
    good = out.copy()
    assert oc.same_bits(good, oc.ref_observables(u, seg, (ptr, idx, w), num, den, 4))
    refused = [dict(S_=-1), dict(L_=-1), dict(H=-1), dict(G=-1), dict(pitch=-1), dict(u_=None), dict(out_=None), dict(ptr_=None),
               dict(idx_=None), dict(w_=None), dict(num_=None), dict(den_=None), dict(ptr_=i64(1, 2, 3)), dict(ptr_=i64(0, 3, 2)),
               dict(idx_=i64(0, N, 4)), dict(idx_=i64(-1, 3, 4)), dict(num_=i64(0, 2, 0)), dict(num_=i64(-1, 1, 0)),
               dict(den_=i64(-1, -2, 1)), dict(den_=i64(-1, 2, 1)), dict(pitch=2), dict(seg_n=i64(L + 1, 0)), dict(seg_n=i64(-1, 0))]
    for kw in refused:
        assert call(**kw) == capi.KIN_ERR_INVALID_ARG, kw
        assert lib.kin_last_error(h.handle)
    # (the sizes are looked at before any buffer is: nothing is read or written in these calls)
    for kw in (dict(S_=1 << 31, L_=0, seg_n=None), dict(L_=1 << 31, S_=0, seg_n=None), dict(S_=1 << 16, L_=1 << 15, seg_n=None),
               dict(pitch=1 << 30, S_=0, seg_n=None)):
        assert call(**kw) == capi.KIN_ERR_UNSUPPORTED, kw
    assert out.tobytes() == good.tobytes()            # a refused call writes nothing
    # the device entry: the same argument rules (it does not read seg_n)
    for kw in (dict(num=i64(0, 2, 0)), dict(pitch=2)):
        with pytest.raises(capi.KineticaHipError) as e:
            observables_dev(h, u, (ptr, idx, w), kw.get("num", num), den, kw.get("pitch", 4))
        assert e.value.code == capi.KIN_ERR_INVALID_ARG, kw
    with pytest.raises(capi.KineticaHipError) as e:
        h.observables_segmented_dev(S, L, 0, ptr, idx, w, num, den, 4, 0)
    assert e.value.code == capi.KIN_ERR_INVALID_ARG
    # the stored forms without a stored ensemble / solution
    spec = (2, p64(ptr), p64(idx), pd(w), 3, p64(num), p64(den))
    assert lib.kin_ensemble_observables(h.handle, *spec, 4, 0, pd(out)) == capi.KIN_ERR_STATE
    assert lib.kin_ensemble_observables(h.handle, *spec, N, 1, None) == capi.KIN_ERR_STATE
    assert lib.kin_solution_observables(h.handle, *spec, 4, pd(out)) == capi.KIN_ERR_STATE
    with pytest.raises(capi.KineticaHipError) as e:
        h.ensemble_observable_count()
    assert e.value.code == capi.KIN_ERR_STATE
    # the handle is as it was: the next call gives the first call's bytes
    assert call() == capi.KIN_OK and out.tobytes() == good.tobytes()
    h.close()
