"""Reference, classes and constructed cases for the tests of rate-constant formation (tests/test_arrhenius_cases.py on
the host replay of exp_tab.hpp, tests/test_gpu_rate_constants.py on the device) - TEST INFRASTRUCTURE, no product code.

The law: k_r = A exp(-Ea / RT) N_A t_mult, with a cap k = 1 / (1/k_max + 1/k_r). RT is the DOUBLE product
fl(8.314462618 * T), as in every implementation and in the reference's functor; everything after it is taken in long double
(64-bit significand), with the quotient Ea / RT carried as a head and a tail so that the reference keeps ~3e-19 relative
at any |Ea/RT| (a plain long double quotient would lose |q| * 2^-64: 4e-17 at |q| = 700).

Two forms are classified (FORMS):
  literal  arrhenius_one: A * exp(-Ea/RT) * N_A * t_mult evaluated left to right, the cap with three divisions
  fast     arrhenius_fast_t: q = min(max(Ea/RT, -800), 800), c = fl(fl(A N_A) t_mult), k = c * exp_tab(-q), or with a cap
           x = fma(1/c, exp_tab(q), 1/k_max), k = x < 1e300 ? 1/x : 0; 1/RT is capped at 1e300 (T = 0)
A cap at +inf is no cap (kin_set_arrhenius), here as there.

`classify` follows the form's own chain of double operations on the TRUE values: every stage whose true value is below the
smallest normal double is widened by one quantum 2^-1074 (what the issue measured for exp_tab in the subnormal band; a
value below 0.49 quanta becomes exactly zero), every stage above the largest double becomes +inf. That yields an interval
[lo, hi] of values the form may return before the relative bound (|q| + 8) * 2^-53 is applied - the single bound of all
forms against this reference: |q| half-ulps of the rounded quotient amplified by exp, ~2 for exp, 3 - 4 for the products and
the reciprocal. Classes (every element is in exactly one):
  normal            no stage widened, the result a normal double:  |dev - ref| <= (|q| + 8) 2^-53 ref
  subnormal_exp     some stage subnormal (exp itself for 708.4 < q < 745.2; for the literal form also A * exp, for a capped
                    form 1/k_r):  lo (1 - b) <= dev <= hi (1 + b), i.e. the bound plus the scaled quantum
  zero_limit        exactly +0.0: A = 0, exp(-q) below 2^-1075, q >= 800 (T = 0 with Ea > 0 included), and for the capped fast
                    form an overflowing exp(+q) or x >= 1e300
  cap_limit         the form's k_r is +inf and so is the true one (or 1/k_r vanishes next to 1/k_max): exactly +inf without a
                    cap; with one exactly k_max - or fl(1 / fl(1/k_max)), the image of k_max under the formula's own two
                    reciprocals, which differs from k_max by an ulp for k_max = 1e300 (1e12 and 1e-300 are fixed points)
  literal_overflow  a stage of the form overflows while the true k_r is a finite double: same rule as cap_limit. The literal
                    form's left-to-right product with t_mult < 1 is the case the class is named after; an overflowing
                    exp(-q) under a tiny A puts both forms there
  undefined         the formula itself is 0/0 (Ea = 0 at T = 0) or 0 * inf (A = 0 under an overflowing exp): no value is
                    right, so what each form returns is pinned, one value per form and case. The literal form: NaN. The
                    fast form at Ea = 0, T = 0: the value Ea = 0 has at every T > 0 (q = 0 * 1e300 = 0); the fast form at
                    A = 0 under an overflowing exp: NaN without a cap (0 * inf), +0.0 with one (x is inf or NaN, not < 1e300)
  left_out          within 1e-9 relative of a threshold between two exact classes (a stage at the largest double, x at 1e300)
"""
import numpy as np

LD = np.longdouble
R_GAS = np.float64(8.314462618)
N_A = np.float64(6.02214076e23)
U53 = 2.0 ** -53
FORMS = ("literal", "fast")
CLASSES = ("normal", "subnormal_exp", "zero_limit", "cap_limit", "literal_overflow", "undefined", "left_out")
CLS = {n: i for i, n in enumerate(CLASSES)}

_TINY = LD(2) ** -1022
_QUANT = LD(2) ** -1074
_DMAX = LD(np.finfo(np.float64).max)
_EDGE = LD(1e-9)

# the constructed inputs (edge_parameters): reaction i takes EA_LIST[i % 8] and A_LIST[(i // 8) % 5] - 40 combinations
EA_LIST = np.array([0.0, 1.0, 1e3, 5e4, 2.5e5, 6.5e5, -5e4, -6e5])
A_LIST = np.array([10.0 ** 8.8, 0.0, 1e-300, 10.0 ** 12.3, 1.0 / 6.02214076e23])   # the last: c ~ 1, k is the bare table exp
T_LIST = np.array([0.0, 1e-3, 0.02, 85.0, 100.0, 101.9, 300.0, 1000.0, 1500.0, 1e5])
CAPS = [(None, 1.0), (1e12, 1.0), (1e12, 1e-3), (np.inf, 1.0), (1e300, 1.0), (1e-300, 1.0)]      # (k_max, t_mult)


def cap_id(cap):
    return f"kmax={cap[0]}-tmult={cap[1]}"


def edge_parameters(R):
    i = np.arange(R)
    return EA_LIST[i % 8].copy(), A_LIST[(i // 8) % 5].copy()


def dense_parameters(R, seed):
    """The interior: log-uniform A, Ea uniform in +-6.5e5 with 20 % exact zeros."""
    rng = np.random.default_rng(seed)
    A = 10.0 ** rng.uniform(8.8, 12.3, R)
    Ea = rng.uniform(-6.5e5, 6.5e5, R)
    Ea[rng.random(R) < 0.2] = 0.0
    return Ea, A


def dense_temperatures(n, seed):
    return np.random.default_rng(seed).uniform(120.0, 2000.0, n)


def rint_ties(TAB, per_sign=4000, seed=0):
    """Arguments x in [-708, 708] with x * TAB / ln 2 within 2^-40 of a half-integer - where the table index flips."""
    ln2 = LD("0.693147180559945309417232121458176568")
    step = ln2 / LD(TAB)
    m_max = int(708.0 / float(step)) - 1
    m = np.arange(-m_max, m_max, dtype=np.int64)
    x = ((m.astype(LD) + LD(0.5)) * step).astype(np.float64)
    off = np.abs(x.astype(LD) / step - (m.astype(LD) + LD(0.5)))
    x = x[off < LD(2) ** -40]
    rng = np.random.default_rng(seed)
    neg, pos = x[x < 0], x[x > 0]
    return np.concatenate([rng.choice(neg, min(per_sign, len(neg)), replace=False), rng.choice(pos, min(per_sign, len(pos)), replace=False)])


def _two_prod(a, b):
    """a * b = p + e exactly in long double (Dekker's product with Veltkamp's split, 64-bit significand)."""
    p = a * b
    s = LD(2) ** 32 + LD(1)
    ah = a * s; ah = ah - (ah - a); al = a - ah
    bh = b * s; bh = bh - (bh - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _q_parts(Ea, T):
    """Ea / fl(R T) as head + tail in long double; the head is what the bound's |q| means."""
    RT = (R_GAS * np.asarray(T, np.float64)).astype(LD)
    Ea = np.asarray(Ea, np.float64).astype(LD)
    q = Ea / RT
    p, e = _two_prod(q, RT)
    tail = ((Ea - p) - e) / RT
    tail = np.where(np.isfinite(q) & np.isfinite(tail), tail, LD(0))
    return q, tail


def _exp_neg(q, tail, sign=-1):
    """exp(sign * (q + tail))"""
    return np.exp(LD(sign) * q) * (LD(1) + LD(sign) * tail)


def k_ref(Ea, A, T, k_max=None, t_mult=1.0):
    """The law in long double on the double product RT (see the module docstring); NaN where the formula is 0/0 or 0 * inf."""
    with np.errstate(all="ignore"):
        Ea, A, T = np.broadcast_arrays(np.asarray(Ea, np.float64), np.asarray(A, np.float64), np.asarray(T, np.float64))
        q, tail = _q_parts(Ea, T)
        kr = A.astype(LD) * _exp_neg(q, tail) * LD(N_A) * LD(t_mult)
        if k_max is None:
            return kr
        return LD(1) / (LD(1) / LD(k_max) + LD(1) / kr)


class _Iv:
    """Interval [lo, hi] of non-negative long doubles with the flags the classes are made of."""

    def __init__(self, lo, hi=None):
        self.lo = lo
        self.hi = lo if hi is None else hi
        z = np.zeros(np.shape(lo), bool)
        self.sub, self.edge = z.copy(), z.copy()

    def _carry(self, o):
        o.sub, o.edge = self.sub.copy(), self.edge.copy()
        return o

    def stage(self):
        """The value as a double: widened by a quantum where subnormal, +inf above the largest double."""
        o = self._carry(_Iv(self.lo, self.hi))
        for name in ("lo", "hi"):
            v = getattr(self, name)
            small = (v > 0) & (v < _TINY)
            o.sub |= small
            if name == "lo":
                w = np.where(small, np.maximum(v - _QUANT, LD(0)), v)
            else:
                w = np.where(small, np.where(v < LD(0.49) * _QUANT, LD(0), v + _QUANT), v)
            o.edge |= np.isfinite(v) & (np.abs(v / _DMAX - LD(1)) < _EDGE)
            w = np.where(v > _DMAX, LD(np.inf), w)
            setattr(o, name, w)
        return o

    def times(self, c):
        return self._carry(_Iv(self.lo * c, self.hi * c))

    def plus(self, c):
        return self._carry(_Iv(self.lo + c, self.hi + c))

    def recip(self):
        return self._carry(_Iv(LD(1) / self.hi, LD(1) / self.lo))


def classify(Ea, A, T, k_max=None, t_mult=1.0, form="fast"):
    """dict(cls[int8, index into CLASSES], ref[LD], lo[LD], hi[LD], b[float64 relative bound], q[float64], expect[float64: the
    exact value of the exact classes, NaN elsewhere], expect2[the second admitted image of k_max]) for every element of the
    broadcast of Ea, A, T."""
    assert form in FORMS
    if k_max is not None and np.isinf(k_max):
        k_max = None                      # kin_set_arrhenius takes a cap at +inf as no cap
    with np.errstate(all="ignore"):
        Ea, A, T = np.broadcast_arrays(np.asarray(Ea, np.float64), np.asarray(A, np.float64), np.asarray(T, np.float64))
        capped = k_max is not None
        q, tail = _q_parts(Ea, T)
        ref = k_ref(Ea, A, T, k_max, t_mult)
        kr_true = k_ref(Ea, A, T, None, t_mult)
        Al = A.astype(LD)
        forced_zero = np.zeros(Ea.shape, bool)
        ik = (np.float64(1.0) / np.float64(k_max)).astype(LD) if capped else LD(0)      # 1/k_max as the forms take it
        if form == "literal":
            iv = _Iv(_exp_neg(q, tail)).stage().times(Al).stage().times(LD(N_A)).stage().times(LD(t_mult)).stage()
            kr_inf = np.isinf(iv.lo)
            if capped:
                iv = iv.recip().stage().plus(ik).stage().recip().stage()
        else:
            c = (np.float64(A * N_A) * np.float64(t_mult)).astype(LD)
            forced_zero |= q >= 800
            if not capped:
                iv = _Iv(_exp_neg(q, tail)).stage().times(c).stage()
                kr_inf = np.isinf(iv.lo)
            else:
                E = _Iv(_exp_neg(q, tail, +1)).stage()
                forced_zero |= np.isinf(E.lo)                               # an overflowing exp(+q): x = inf
                kr_inf = E.hi == 0                                          # exp(+q) has vanished: x = 1/k_max exactly
                t = E.times(LD(1) / c)                                      # 1/k_r
                # x < 1e300 is decided on the rounded sum; the threshold counts as near where 1e-9 on 1/k_r moves the decision
                x_lo = (t.lo * (1 - _EDGE) + ik).astype(np.float64)
                x_hi = (t.hi * (1 + _EDGE) + ik).astype(np.float64)
                forced_zero |= x_lo >= 1e300
                x = t.plus(ik).stage()
                x.edge |= ~((x_lo >= 1e300) | (x_hi < 1e300)) & ~np.isinf(E.lo)
                iv = x.recip().stage()
        lo, hi = iv.lo, iv.hi
        qd = q.astype(np.float64)
        b = (np.minimum(np.abs(np.nan_to_num(qd, nan=0.0, posinf=1e30, neginf=1e30)), 1e30) + 8.0) * U53
        top = np.float64(k_max) if capped else np.float64(np.inf)
        top_img = np.float64(1.0) / (np.float64(1.0) / top)                 # k_max after the formula's own two reciprocals

        cls = np.full(Ea.shape, -1, np.int8)
        expect = np.full(Ea.shape, np.nan)

        def put(mask, name, value=None):
            m = mask & (cls < 0)
            cls[m] = CLS[name]
            if value is not None:
                expect[m] = value

        put(np.isnan(q) | np.isnan(ref) | np.isnan(lo) | np.isnan(hi) | np.isnan(kr_true), "undefined")
        put((A == 0) | forced_zero | ((lo == 0) & (hi == 0)), "zero_limit", 0.0)
        put(iv.edge, "left_out")
        if capped and np.isfinite(top):
            near = ref >= LD(top) * (LD(1) - LD(2) ** -56)                  # 1/k_max + 1/k_r rounds to 1/k_max
            exact_top = kr_inf | near
        else:
            near = np.zeros(Ea.shape, bool)
            exact_top = np.isinf(lo) & np.isinf(hi)
        put(exact_top & (kr_true <= _DMAX) & ~near, "literal_overflow", top)
        put(exact_top, "cap_limit", top)
        put(iv.sub | (ref < _TINY) | (lo != hi), "subnormal_exp")
        put(cls < 0, "normal")
        expect2 = np.where(expect == 0.0, 0.0, np.where(np.isnan(expect), np.nan, top_img))
        alt = k_ref(np.zeros_like(Ea), A, np.full_like(T, 300.0), k_max, t_mult)      # (undefined: the Ea = 0 value)
        # what each form returns where the formula is undefined (NaN = NaN is expected)
        if form == "literal":
            uexp = np.full(Ea.shape, np.nan)
        else:
            uexp = np.where(np.isnan(qd), alt.astype(np.float64), 0.0 if capped else np.nan)
        return dict(cls=cls, ref=ref, lo=lo, hi=hi, b=b, q=qd, expect=expect, expect2=expect2, uexp=uexp)


def check(dev, info):
    """(ok[bool], ratio[float64]) per element: does `dev` obey its class's rule; ratio = error / bound for the two bounded
    classes (0 elsewhere). left_out elements are ok by definition."""
    dev = np.asarray(dev, np.float64)
    cls = info["cls"]
    ok = np.zeros(dev.shape, bool)
    ratio = np.zeros(dev.shape)
    with np.errstate(all="ignore"):
        d = dev.astype(LD)
        m = (cls == CLS["normal"]) | (cls == CLS["subnormal_exp"])
        b = info["b"].astype(LD)
        ok[m] = ((d >= info["lo"] * (1 - b)) & (d <= info["hi"] * (1 + b)))[m]
        err = np.maximum(info["lo"] - d, d - info["hi"])
        err = np.maximum(err, LD(0)) / (b * np.where(m, info["ref"], LD(1)))
        n = cls == CLS["normal"]
        errn = np.abs(d - info["ref"]) / (b * np.where(n, info["ref"], LD(1)))
        ratio[m] = err[m].astype(np.float64)
        ratio[n] = errn[n].astype(np.float64)
        z = cls == CLS["zero_limit"]
        ok[z] = (dev[z] == 0.0) & ~np.signbit(dev[z])
        for name in ("cap_limit", "literal_overflow"):
            t = cls == CLS[name]
            ok[t] = (dev[t] == info["expect"][t]) | (dev[t] == info["expect2"][t])
        u = cls == CLS["undefined"]
        want = info["uexp"][u]
        ok[u] = np.where(np.isnan(want), np.isnan(dev[u]),
                         (np.abs(dev[u] - want) <= 16 * U53 * np.abs(want)) & ((want != 0.0) | ~np.signbit(dev[u])))
        ok[cls == CLS["left_out"]] = True
    return ok, ratio


def class_counts(info):
    return {n: int(np.sum(info["cls"] == i)) for i, n in enumerate(CLASSES)}


def mp_reference(Ea, A, T, k_max=None, t_mult=1.0, digits=50):
    """The same law with mpmath at `digits` digits (the witness of k_ref); object array of mpf, None where undefined."""
    import mpmath
    Ea, A, T = np.broadcast_arrays(np.asarray(Ea, np.float64), np.asarray(A, np.float64), np.asarray(T, np.float64))
    out = np.empty(Ea.shape, object)
    with mpmath.workdps(digits):
        for idx in np.ndindex(Ea.shape):
            RT = mpmath.mpf(float(R_GAS * T[idx]))
            ea, a = mpmath.mpf(float(Ea[idx])), mpmath.mpf(float(A[idx]))
            if RT == 0 or a == 0:
                out[idx] = None
                continue
            kr = a * mpmath.exp(-ea / RT) * mpmath.mpf(float(N_A)) * mpmath.mpf(float(t_mult))
            if k_max is None:
                out[idx] = kr
            else:
                ik = mpmath.mpf(0) if np.isinf(k_max) else 1 / mpmath.mpf(float(k_max))
                out[idx] = 1 / (ik + 1 / kr)
    return out
