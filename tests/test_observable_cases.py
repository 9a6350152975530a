"""CPU tests of the observables pass: kin_observables_host - the definition of include/kinetica_hip.h in plain C++ loops, no
handle, no device - against observable_cases.ref_observables bit for bit on every case and pitch; the order of a long form's sum
(64 chains and the butterfly, not one sequential sum); the bits of a copied -0.0; every refusal of the host entry; and what
solving.observables / mole_fractions build and refuse. _statistics_arguments and _sobol_arguments give what they gave before
the observables keyword existed: the observables travel beside those dictionaries, not inside them."""
import numpy as np
import pytest

import observable_cases as oc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S


@pytest.mark.parametrize("case", oc.CASES, ids=[c["id"] for c in oc.CASES])
def test_host_entry_is_the_restatement_bit_for_bit(case):
    for pitch in case["pitches"]:
        got = capi.observables_host(case["u"], *case["forms"], case["num"], case["den"], pitch=pitch, seg_n=case["seg_n"])
        ref = oc.at(case, pitch)
        assert got.shape == ref.shape and oc.same_bits(got, ref), (case["id"], pitch)
    # species in index base 1: the same bits
    ptr, idx, w = case["forms"]
    one = capi.observables_host(case["u"], ptr, idx + 1, w, case["num"], case["den"], seg_n=case["seg_n"], index_base=1)
    assert oc.same_bits(one, oc.reference(case))


def test_the_cases_hold_what_they_are_meant_to_hold():
    """Inf and NaN from zero denominators, -0.0 results, rows behind a segment's end that are zeros although the states there
    are NaN, more than 64 denominators, and forms on both sides of the threshold of 64 terms."""
    r = oc.reference(oc.CASES[6])
    assert np.isinf(r).any() and np.isnan(r).any() and (np.signbit(r) & (r == 0.0)).any()
    case = oc.CASES[8]
    assert len(set(case["den"][case["den"] >= 0].tolist())) > 64
    assert np.isnan(case["u"][2]).all() and not oc.reference(case)[2].any()
    lengths = np.diff(oc.CASES[10]["forms"][0]).tolist()
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 1025} <= set(lengths)


def test_a_long_form_is_not_a_sequential_sum():
    """65 terms: 1e16, 63 ones, -1e16. One sequential sum loses every 1.0 against 1e16 and gives 0.0; the definition puts the
    first and the last term on chain 0 - 1e16 - 1e16 = 0 - and folds the 63 ones of the other chains exactly: 63.0."""
    N = 65
    u = np.ones((1, 1, N)); u[0, 0, 0], u[0, 0, 64] = 1e16, -1e16
    ptr, idx, w = [0, N], np.arange(N), np.ones(N)
    got = capi.observables_host(u, ptr, idx, w, [0], [-1])
    assert oc.sequential_form(idx.tolist(), w.tolist(), u[0, 0].tolist()) == 0.0
    assert got[0, 0, 0] == 63.0 == oc.ref_form(idx.tolist(), w.tolist(), u[0, 0].tolist())
    # the same terms as a short form of 64 (the last two merged): one sequential sum
    u64 = np.ones((1, 1, 64)); u64[0, 0, 0], u64[0, 0, 63] = 1e16, -1e16
    assert capi.observables_host(u64, [0, 64], np.arange(64), np.ones(64), [0], [-1])[0, 0, 0] == 0.0


def test_a_singleton_of_weight_one_copies_the_bits():
    u = np.array([[[-0.0, 0.0, 5e-324, -np.inf, 1.5]]])
    got = capi.observables_host(u, np.arange(6), np.arange(5), np.ones(5), np.arange(5), np.full(5, -1))
    assert got.tobytes() == u.tobytes()
    assert np.signbit(got[0, 0, 0]) and not np.signbit(got[0, 0, 1])
    # an empty form is +0.0, and -0.0 weights give the product's sign
    got = capi.observables_host(np.array([[[2.0]]]), [0, 0, 1], [0], [-0.0], [0, 1], [-1, -1])
    assert got[0, 0, 0] == 0.0 and not np.signbit(got[0, 0, 0]) and got[0, 0, 1] == 0.0 and np.signbit(got[0, 0, 1])


def test_statuses_of_the_host_entry():
    N, S_, L = 5, 2, 4
    lib = capi.lib()
    u = np.arange(1.0, S_ * L * N + 1).reshape(S_, L, N)
    seg = np.array([L, 2], np.int64)
    i64 = lambda *v: np.array(v, np.int64)
    ptr, idx, w, num, den = i64(0, 2, 3), i64(0, 3, 4), np.array([1.0, 2.0, -1.0]), i64(0, 1, 0), i64(-1, -1, 1)
    out = np.full((S_, L, 4), -7.0)
    pd, p64 = capi._pd, capi._p64

    def call(N_=N, base=0, S=S_, L_=L, seg_n=seg, u_=u, H=2, ptr_=ptr, idx_=idx, w_=w, G=3, num_=num, den_=den, pitch=4, out_=out):
        return lib.kin_observables_host(N_, base, S, L_, p64(seg_n), pd(u_), H, p64(ptr_), p64(idx_), pd(w_), G, p64(num_), p64(den_), pitch,
                                        pd(out_))

    assert call() == capi.KIN_OK
    good = out.copy()
    assert oc.same_bits(good, oc.ref_observables(u, seg, (ptr, idx, w), num, den, 4))
    refused = [dict(N_=-1), dict(S=-1), dict(L_=-1), dict(H=-1), dict(G=-1), dict(pitch=-1), dict(u_=None), dict(out_=None),
               dict(ptr_=None), dict(idx_=None), dict(w_=None), dict(num_=None), dict(den_=None), dict(ptr_=i64(1, 2, 3)),
               dict(ptr_=i64(0, 3, 2)), dict(idx_=i64(0, N, 4)), dict(idx_=i64(-1, 3, 4)), dict(base=1), dict(num_=i64(0, 2, 0)),
               dict(num_=i64(-1, 1, 0)), dict(den_=i64(-1, -2, 1)), dict(den_=i64(-1, 2, 1)), dict(pitch=2), dict(seg_n=i64(L + 1, 0)),
               dict(seg_n=i64(-1, 0))]
    for kw in refused:
        assert call(**kw) == capi.KIN_ERR_INVALID_ARG, kw
    assert out.tobytes() == good.tobytes()            # a refused call writes nothing
    # what is allowed: nothing to write, no forms, no segment lengths
    assert call(S=0, u_=None, out_=None, seg_n=None) == capi.KIN_OK and call(pitch=0, G=0, out_=None) == capi.KIN_OK
    assert call(H=0, G=0, ptr_=None, idx_=None, w_=None, num_=None, den_=None) == capi.KIN_OK and not out.any()
    assert call(seg_n=None) == capi.KIN_OK and out[1, 3, 0] == u[1, 3, 0] + 2.0 * u[1, 3, 3]
    with pytest.raises(capi.KineticaHipError) as e:
        capi.observables_host(u, ptr, idx, w, num, i64(-1, 5, 1))
    assert e.value.code == capi.KIN_ERR_INVALID_ARG
    for bad in (dict(form_w=w[:2]), dict(den=den[:2]), dict(form_ptr=i64(0, 2, 9))):      # lengths the binding compares itself
        kw = dict(form_ptr=ptr, form_idx=idx, form_w=w, num=num, den=den)
        kw.update(bad)
        with pytest.raises(ValueError):
            capi.observables_host(u, **kw)


# ---- solving.observables / mole_fractions ----------------------------------------------------------------------------------
SD = S.SpeciesData.from_names(["A", "B", "C", "D"])


def test_observables_builds_the_csr():
    s = S.observables(SD, {"a": "A", "bc": ["B", "C", "B"], "w": {"A": 2.0, 3: -1}, "sel": ("ratio", "a", "bc"), "self": ("ratio", "w", "w")})
    assert s.names == ("a", "bc", "w", "sel", "self") and (s.N, s.H, s.G) == (4, 3, 5)
    assert s.form_ptr.tolist() == [0, 1, 4, 6] and s.form_idx.tolist() == [0, 1, 2, 1, 0, 3] and s.form_w.tolist() == [1, 1, 1, 1, 2, -1]
    assert s.num.tolist() == [0, 1, 2, 0, 2] and s.den.tolist() == [-1, -1, -1, 1, 2]
    assert s.arrays(1)[1].tolist() == [1, 2, 3, 2, 1, 4] and s.form_idx.dtype == np.int64 and s.form_w.dtype == np.float64
    ids = S.observables(4, {"x": 2, "y": [np.int64(0), 3]})
    assert ids.form_idx.tolist() == [2, 0, 3] and ids.den.tolist() == [-1, -1]
    # what the spec says is what the restatement computes
    u = np.array([[[1.0, 2.0, 4.0, 8.0]]])
    v = capi.observables_host(u, *s.arrays())
    assert v[0, 0].tolist() == [1.0, 8.0, -6.0, 0.125, 1.0]


def test_mole_fractions_spec():
    m = S.mole_fractions(SD)
    assert (m.H, m.G, m.N) == (5, 4, 4) and m.names == ("x[A]", "x[B]", "x[C]", "x[D]")
    assert m.form_ptr.tolist() == [0, 1, 2, 3, 4, 8] and m.form_idx.tolist() == [0, 1, 2, 3, 0, 1, 2, 3] and np.all(m.form_w == 1.0)
    assert m.num.tolist() == [0, 1, 2, 3] and m.den.tolist() == [4, 4, 4, 4]
    sub = S.mole_fractions(4, species=[3, 1])
    assert sub.names == ("x[3]", "x[1]") and sub.num.tolist() == [3, 1] and sub.den.tolist() == [4, 4] and sub.H == 5
    assert S.mole_fractions(SD, ["C"]).num.tolist() == [2]
    u = np.array([[[1.0, 2.0, 4.0, 9.0]]])
    assert capi.observables_host(u, *m.arrays())[0, 0].tolist() == [1 / 16, 2 / 16, 4 / 16, 9 / 16]


@pytest.mark.parametrize("spec", [
    {}, None, [("a", "A")], {"a": "Z"}, {"a": 4}, {"a": -1}, {"a": 1.5}, {"a": True}, {"a": ["A", "Z"]}, {"a": {"Z": 1.0}},
    {"a": {"A": "x"}}, {"a": {"A": True}}, {"r": ("ratio", "a", "b")}, {"a": "A", "r": ("ratio", "a", "b")},
    {"a": "A", "r": ("ratio", "b", "a")}, {"a": "A", "r": ("ratio", "a", "a"), "q": ("ratio", "r", "a")}, {"a": None},
])
def test_observables_refuses_a_malformed_spec(spec):
    with pytest.raises(ValueError):
        S.observables(SD, spec)


def test_observables_refuses_before_the_device():
    with pytest.raises(ValueError):
        S.observables(4, {"a": "A"})                  # a name without a SpeciesData
    for first in (0, -3, 2.5, True, None, "A"):
        with pytest.raises(ValueError):
            S.observables(first, {"a": 0})
        with pytest.raises(ValueError):
            S.mole_fractions(first)
    with pytest.raises(ValueError, match="at most as many"):      # G > N where a store is asked for
        S.observables(2, {"a": 0, "b": 1, "c": [0, 1]}, store=True)
    assert S.observables(2, {"a": 0, "b": 1, "c": [0, 1]}).G == 3
    for species in ([], ["Z"], [4], [0.5]):
        with pytest.raises(ValueError):
            S.mole_fractions(SD, species)
    # a spec built for another network, and solve_network_ensemble's argument before anything is solved
    with pytest.raises(ValueError, match="built for"):
        S._observable_spec(5, S.mole_fractions(4))
    with pytest.raises(ValueError, match="observables"):
        S.solve_network_ensemble([object()], None, None, observables=[1, 2])

    class NoDevice:
        n, index_base = 4, 0

        def ensemble_observables(self, *a, **k):
            raise AssertionError("the device was reached")

    for kw in (dict(spec={"a": 9}), dict(spec={"a": 0}, download=False), dict(spec={"a": 0, "b": 1, "c": 2, "d": 3, "e": 0}, store=True)):
        with pytest.raises(ValueError):
            S.ensemble_observables(NoDevice(), **kw)


def test_observables_reach_the_handle_with_its_index_base():
    """ensemble_observables hands the forms to the handle in the handle's index base, asks for pitch N with store and the compact
    pitch without, and returns the first G columns."""
    calls = []

    class Handle:
        n, index_base = 4, 1

        def ensemble_observables(self, ptr, idx, w, num, den, pitch=None, store=False, download=True):
            calls.append((idx.tolist(), pitch, store, download))
            return np.arange(2.0 * 3 * pitch).reshape(2, 3, pitch) if download else None

    spec = S.observables(4, {"a": 0, "b": [1, 3]})
    r = S.ensemble_observables(Handle(), spec, store=True)
    assert calls[-1] == ([1, 2, 4], 4, True, True) and r.values.shape == (2, 3, 2) and r.G == 2 and r.names == ("a", "b") and r.spec is spec
    assert r.values[1, 2].tolist() == [20.0, 21.0]
    r = S.ensemble_observables(Handle(), {"a": 0, "b": [1, 3]}, store=True, download=False)
    assert calls[-1] == ([1, 2, 4], 4, True, False) and r.values is None
    r = S.ensemble_observables(Handle(), spec)
    assert calls[-1] == ([1, 2, 4], 2, False, True) and r.values.shape == (2, 3, 2)


# ---- the keyword dictionaries are what they were -----------------------------------------------------------------------------
def test_statistics_and_sobol_arguments_are_unchanged():
    kw = S._statistics_arguments(True, 4)
    assert sorted(kw) == ["inputs", "quantiles", "rank", "species", "use"]
    assert kw["quantiles"].tolist() == [0.05, 0.5, 0.95] and kw["species"] is None and kw["inputs"] is None and kw["rank"] is True
    assert S._statistics_arguments(None, 4) is None
    kw = S._statistics_arguments(dict(quantiles=None, species=(3, 1), inputs=np.ones((4, 2)), rank=0), 4)
    assert sorted(kw) == ["inputs", "quantiles", "rank", "species", "use"]
    assert kw["quantiles"].tolist() == [] and kw["species"].tolist() == [3, 1] and kw["inputs"].shape == (4, 2) and kw["rank"] is False
    kw = S._statistics_arguments(dict(sobol=dict(M=4, P=1)), 12)
    assert kw["sobol"] == dict(M=4, P=1, species=None, w=None, of="states", n_boot=0, seed=0, level=0.95)
    assert S._sobol_arguments(dict(M=4, P=1), 12) == dict(M=4, P=1, species=None, w=None, of="states", n_boot=0, seed=0, level=0.95)
    kw = S._statistics_arguments(dict(of="t_cross", events=dict(level=0.5, kind="of_start", direction="fall")), 6)
    assert sorted(kw) == ["events", "inputs", "of", "quantiles", "rank", "species", "use"] and kw["of"] == "t_cross"
    for bad in (dict(observables={"a": 0}), dict(sobol=dict(M=4, P=1, observables={"a": 0}))):      # no such key in either
        with pytest.raises(ValueError):
            S._statistics_arguments(bad, 12)


def test_solution_containers():
    import dataclasses
    assert [f.name for f in dataclasses.fields(S.ODESolution)][-2:] == ["resampled", "observables"]
    assert S.ODESolution(np.zeros(1), np.zeros((1, 1)), "Success").observables is None
    assert [f.name for f in dataclasses.fields(S.Observables)] == ["names", "values", "G", "spec"]
