"""The cases of the flux-pass tests (test_flux_cases.py on the CPU, test_gpu_flux_paths.py on the GPU) and their references.

The flux pass (flux_kernels.hip: flux_sweep_kernel + flux_reduce_kernel, flux_seg_kernel) is compiled once per
(ROWS, MODE, PATH, RATES); flux_plan and flux_modes choose among the instantiations from N, R, the alignment of three
pointers and KIN_FLUX_LDS / KIN_FLUX_ROWS. Every case here is the smallest input that takes one of them and says which -
Case.inst / Case.seg_inst; the tests ask kin_flux_plan_host whether that is what runs.

References: per-state rates from OracleNetwork.rates, flux as math.fsum of w_b rate_b.
Bounds: those of test_gpu_flux.py / test_gpu_flux_segmented.py, derived in their docstrings (EPS = 2^-53):
  per-state rates   |got - ref| <= 4 EPS |ref| + 1e-300
  flux, k given     |got - ref| <= (B + 8) EPS sum_b |w_b rate_b| + 1e-300        ((L + 8) in the segmented pass)
  temperature form  + (2 |Ea_r / (R T_b)| + 16) EPS per term
The exact class needs no bound: u in {1/2, 1, 2}, k an integer 1 .. 8, w in {-2 .. 2}. A rate is k u u' - a multiple of 1/4,
at most 32 - and a term w rate a multiple of 1/4, at most 64; a sum of up to 600 of them stays below 2^16: no product and no
partial sum rounds, in any order, with or without fused multiply-adds. Device and oracle agree bit for bit."""
import math
from collections import namedtuple

import numpy as np

from kinetica_jl_amd.synth import from_lists, synthetic_crn

EPS = 2.0 ** -53
RGAS = 8.314462618
K16, K8, KT = 0, 1, 2                    # k modes (flux_kernels.hpp: FluxMode)
S_, L_ = 5, 7                            # the segmented pass: the shape of test_gpu_flux_segmented.py
SEG_N = np.array([7, 0, 3, 1, 5], np.int64)
EXACT_MAX_TERMS = 600
STAGE = 2048                             # species a workgroup stages per trip on path 0 (1 024 threads, one double2 each)
SIZES = (2, 3, 4, 2046, 2047, 2048, 2050, 4096, 10238, 10239, 10240, 10241, 10242, 20477, 20478, 20479, 20480, 65534, 65535, 65536)
BIG_N = 20479                            # from here on the states are large: B = 3 only

Inst = namedtuple("Inst", "path rows parts k_mode rates_mode")         # flux_sweep_kernel<ROWS, MODE, PATH, RATES>, gridDim.y
SegInst = namedtuple("SegInst", "path rows parts k_mode")              # flux_seg_kernel<ROWS, MODE, PATH>, gridDim.y
# One call of a case. ksrc: "k" one row per state, "T" temperatures, "k_row" three rows indexed per state, "shared" the handle's row;
# u_off / k_off / r_off: bytes the state / k / rates buffer starts behind a 16-byte boundary; out: "flux", "both" or "rates"
Variant = namedtuple("Variant", "ksrc u_off k_off r_off out")


def variants(odd_R, temperature, pointers=False):
    """The calls of a case: every k mode and rates mode its R allows. R odd leaves only 8-byte loads and stores."""
    v = []
    if temperature:
        v += [Variant("T", 0, 0, 0, "flux"), Variant("T", 0, 0, 0, "both"), Variant("T", 0, 0, 8, "both"), Variant("T", 0, 0, 0, "rates")]
    else:
        v += [Variant("k", 0, 0, 0, "flux"), Variant("k", 0, 0, 0, "both"), Variant("k", 0, 0, 0, "rates")]
        if not odd_R:
            v += [Variant("k", 0, 0, 8, "both"), Variant("k", 0, 8, 0, "flux"), Variant("k", 0, 8, 0, "both"), Variant("k", 0, 8, 8, "both")]
    if pointers:
        v += [Variant("k", 8, 0, 0, "both"), Variant("k", 8, 8, 8, "both"), Variant("T", 8, 0, 0, "both"),
              Variant("k_row", 0, 0, 0, "both"), Variant("k_row", 0, 8, 0, "flux"), Variant("shared", 0, 0, 0, "both"),
              Variant("shared", 8, 0, 8, "rates")]
    return v


def seg_variants(odd_R, temperature, pointers=False):
    """The calls of the segmented pass (no per-state rates there)."""
    v = [Variant("T", 0, 0, 0, "flux")] if temperature else [Variant("k", 0, 0, 0, "flux")]
    if not temperature and not odd_R:
        v.append(Variant("k", 0, 8, 0, "flux"))
    if pointers:
        v += [Variant("k", 8, 0, 0, "flux"), Variant("T", 8, 0, 0, "flux"), Variant("k_row", 0, 0, 0, "flux"), Variant("k_row", 8, 8, 0, "flux"),
              Variant("shared", 0, 0, 0, "flux")]
    return v


class Case:
    """A network by recipe and the instantiation it is meant to reach: path / rows / parts of the per-state pass and rows / parts
    of the segmented pass (its path is the same). lds: the value of KIN_FLUX_LDS the case runs under."""

    def __init__(self, name, kind, n, R, lds, path, rows, parts, seg_rows, seg_parts, temperature=False, also_temperature=False,
                 pointers=False, layout=None):
        self.name, self.kind, self.n, self.R, self.lds = name, kind, n, R, lds
        self.path, self.rows, self.parts, self.seg_rows, self.seg_parts = path, rows, parts, seg_rows, seg_parts
        self.temperature, self.pointers, self.layout = temperature, pointers, layout
        self.odd = R % 2 == 1
        self.variants = variants(self.odd, temperature, pointers)
        self.seg_variants = seg_variants(self.odd, temperature, pointers)
        if also_temperature:
            self.variants += variants(self.odd, True)[:3]
            self.seg_variants += seg_variants(self.odd, True)

    def __repr__(self):
        return self.name

    def k_mode(self, v):
        if v.ksrc == "T":
            return KT
        return K16 if not self.odd and v.k_off == 0 else K8

    def path_of(self, v):
        return 1 if self.path == 0 and v.u_off else self.path         # a misaligned state cannot be staged as double2

    def inst(self, v):
        rates = 0 if v.out == "flux" else (1 if not self.odd and v.r_off == 0 else 2)
        return Inst(self.path_of(v), self.rows, self.parts, self.k_mode(v), rates)

    def seg_inst(self, v):
        return SegInst(self.path_of(v), self.seg_rows, self.seg_parts, self.k_mode(v))

    def network(self):
        """(net, Ea, A), built once per (recipe)."""
        key = (self.kind == "size", self.n, self.R, self.layout)
        if key not in _nets:
            if len(_nets) >= 3:
                _nets.pop(next(iter(_nets)))
            if self.kind == "size":
                _nets[key] = size_network(self.n, self.layout)
            else:
                net, Ea, A = synthetic_crn(self.n, self.R + self.R % 2)
                if self.odd:            # the last pair half filled
                    net, Ea, A = net.subset(np.arange(self.R)), Ea[:self.R], A[:self.R]
                _nets[key] = (net, Ea, A)
        return _nets[key]


_nets = {}


# ---- the row cases: the smallest networks that take each (path, ROWS, parts) ---------------------------------------------------
# P = ceil(R / 2) pairs over 1 024 threads: need = ceil(P / 1024) rows. Per-state pass, path 0: up to 8 rows; paths 1, 2 and the
# segmented pass: up to 4; temperature form: up to 2.
def _row_cases():
    out = []
    for path, n, lds in ((0, 300, "1"), (1, 301, "1"), (2, 300, "0")):
        tag = f"path{path}"
        lim = 8 if path == 0 else 4
        #        R     per-state (rows, parts) on path 0 / elsewhere          segmented
        table = [(4096, (2, 1), (2, 1), (2, 1)),        # two full rows
                 (4098, (4, 1), (4, 1), (4, 1)),        # need 3: the third row holds one pair in lane 0, the fourth none
                 (6146, (4, 1), (4, 1), (4, 1)),        # need 4: the last row holds one pair
                 (8194, (8, 1), (4, 2), (4, 2)),        # need 5: path 0 takes 8 rows; elsewhere the second part holds one pair
                 (14338, (8, 1), (4, 2), (4, 2))]       # need 8: row 7 holds one pair, lanes 1 .. 1023 clamped
        if path == 0:
            table += [(14337, (8, 1), None, (4, 2)),    # ... and that pair half filled (K8, RATES 2)
                      (16386, (8, 2), None, (4, 3))]    # need 9: two parts of 8, the second holds one real pair
        for R, p0, p12, seg in table:
            rows, parts = p0 if lim == 8 else p12
            out.append(Case(f"{tag}-R{R}", "rows", n, R, lds, path, rows, parts, seg[0], seg[1]))
        for R, parts in ((2050, 1), (4098, 2)):         # temperature form: ROWS 2, one part / two parts
            out.append(Case(f"{tag}-R{R}-T", "rows", n, R, lds, path, 2, parts, 2, parts, temperature=True))
    return out


# ---- the size cases: few reactions at every N where the dispatch or the staging changes -----------------------------------------
def boundary_species(N):
    """The species at the ends of a staged state: 0, 1, N - 2, N - 1 and, for N > STAGE, both sides of every multiple of STAGE below N."""
    s = {0, 1, N - 2, N - 1}
    if N > STAGE:
        for m in range(STAGE, N, STAGE):
            s |= {m - 1, m}
    return sorted(x for x in s if 0 <= x < N)


def _random_net(rng, n, n_pairs, layout):
    """The few-reaction networks of test_gpu_parity.py (A->B, A->B+C, A+B->C+D, 2A->B+C, A->2B with their reverses; "irregular":
    every third reverse missing) as (reacs, prods) lists."""
    fwd = []
    while len(fwd) < n_pairs:
        kind = rng.integers(5)
        if n < 4:
            a, b = (0, 1) if rng.random() < 0.5 else (1, 0)
            fwd.append(([(a, 1)], [(b, 1)]))
            continue
        a, b, c, d = (int(x) for x in rng.choice(n, size=4, replace=False))
        fwd.append([([(a, 1)], [(b, 1)]), ([(a, 1)], sorted([(b, 1), (c, 1)])), (sorted([(a, 1), (b, 1)]), sorted([(c, 1), (d, 1)])),
                    ([(a, 2)], sorted([(b, 1), (c, 1)])), ([(a, 1)], [(b, 2)])][kind])
    reacs, prods = [], []
    for i, (r, p) in enumerate(fwd):
        reacs.append(r); prods.append(p)
        if layout == "adjacent" or i % 3:
            reacs.append(p); prods.append(r)
    return reacs, prods


def operands(net):
    """(x0[R], x1[R]) as the network compiler takes them: the reactant molecules in list order, x1 = -1 for a single one."""
    first = net.reac_idx[net.reac_ptr[:-1]]
    nmol = np.add.reduceat(net.reac_sto, net.reac_ptr[:-1])
    second_at = np.where(net.reac_sto[net.reac_ptr[:-1]] == 2, net.reac_ptr[:-1], np.minimum(net.reac_ptr[:-1] + 1, len(net.reac_idx) - 1))
    return first, np.where(nmol == 2, net.reac_idx[second_at], -1)


def size_network(n, layout):
    """150 random pairs on n species (one for n < 4) plus, for every boundary species s, s -> t (first operand, no second: the dummy
    entry u_s[N] is read right behind it) and t + s -> p (second operand). R is even."""
    seed = {"adjacent": 1, "irregular": 3}[layout] * 100003 + n
    rng = np.random.default_rng(seed)
    reacs, prods = _random_net(rng, n, 150 if n >= 4 else 1, layout)
    for s in boundary_species(n):
        t = (s + n // 2) % n if n > 2 else 1 - s
        p = (s + n // 3 + 1) % n if n > 3 else t
        reacs.append([(s, 1)]); prods.append([(t, 1)])
        reacs.append([(t, 1), (s, 1)]); prods.append([(p, 1)])
    if len(reacs) % 2:
        reacs.append([(n - 1, 2)]); prods.append([(0, 1)])
    net = from_lists(n, reacs, prods)
    x0, x1 = operands(net)
    for s in boundary_species(n):         # the membership the cases exist for
        assert s in x0 and s in x1, (n, layout, s)
    assert np.any((x0 == n - 1) & (x1 < 0)) and net.n_reactions % 2 == 0 and net.n_reactions <= 2048
    R = net.n_reactions
    Ea = np.where(rng.random(R) < 0.25, 0.0, rng.uniform(0.0, 2.0e5, R))
    return net, Ea, 10.0 ** rng.uniform(8.8, 12.3, R)


def size_path(n):
    """The path flux_plan documents for an aligned state of n species (flux_kernels.hpp)."""
    if n >= BIG_N:
        return 2                                        # 8 (n + 2) bytes exceed 160 KiB of LDS
    return 0 if n % 2 == 0 and 2 <= n <= 10240 else 1


def _size_cases():
    # (R is what the recipe gives: even and at most 2 048, asserted there - one row, one part)
    return [Case(f"N{n}-{layout}", "size", n, size_network(n, layout)[0].n_reactions, "1", size_path(n), 1, 1, 1, 1,
                 also_temperature=True, layout=layout) for n in SIZES for layout in ("adjacent", "irregular")]


def _pointer_cases():
    # one even N, one even R (ROWS 1, one part): every misaligned pointer and the k_row / shared sources
    return [Case("pointers-300x1500", "rows", 300, 1500, "1", 0, 1, 1, 1, 1, pointers=True)]


def all_cases():
    return _row_cases() + _size_cases() + _pointer_cases()


# every instantiation flux_go_rows / flux_seg_go_rows can dispatch: (path, rows, k mode[, rates mode])
def allowed_instantiations():
    sweep, seg = set(), set()
    for path in (0, 1, 2):
        for mode in (K16, K8, KT):
            rows_sweep = (1, 2) if mode == KT else ((1, 2, 4, 8) if path == 0 else (1, 2, 4))
            rows_seg = (1, 2) if mode == KT else (1, 2, 4)
            sweep |= {(path, r, mode, rates) for r in rows_sweep for rates in (0, 1, 2)}
            seg |= {(path, r, mode) for r in rows_seg}
    return sweep, seg


def query(case, v, n_cu, B, segmented=False, u_bits=None, k_bits=None, rates_bits=None):
    """kin_flux_plan_host for variant v of a case (under the caller's KIN_FLUX_* environment). The address bits are the variant's
    offsets unless the caller passes those of real buffers."""
    from kinetica_jl_amd import capi
    want_rates = not segmented and v.out != "flux"
    return capi.flux_plan_host(case.n, case.R, B, n_cu, temperature_form=v.ksrc == "T", segmented=segmented,
                               k_stride=0 if v.ksrc == "shared" else case.R, u_bits=v.u_off if u_bits is None else u_bits,
                               k_bits=v.k_off if k_bits is None else k_bits,
                               rates_bits=(v.r_off if rates_bits is None else rates_bits) if want_rates else None)


def as_inst(q):
    return Inst(q["path"], q["rows"], q["parts"], q["k_mode"], q["rates_mode"])


def as_seg_inst(q):
    return SegInst(q["path"], q["rows"], q["parts"], q["k_mode"])


def g_max(n_cu, parts):
    """State slices of a call with more states than the device takes at once (flux_plan: one workgroup per compute unit)."""
    return max(1, n_cu // parts)


def batch_sizes(n, G):
    """B of a case whose plan has up to G state slices: 1; G - 1 (3 where that is not above 1): every workgroup one state, the
    prefetch of the state behind the last clamped; 2 G + 3: three workgroups make a third trip of the state loop, the others two."""
    if n >= BIG_N:
        return [3]
    return sorted({1, G - 1 if G - 1 > 1 else 3, 2 * G + 3})


# ---- inputs and references -------------------------------------------------------------------------------------------------
class Data:
    """B states of one case and one input class with the rate constants of every source, the oracle's per-state rates and the
    references of both passes. cls "log": the states of test_gpu_flux.py (10^U(-12, 0), a one-hot row, exact zeros, entries of
    -1e-14); cls "exact": the exact class of the module docstring (no temperature form there)."""

    def __init__(self, case, B, cls):
        from oracle import oracle as orc
        self.orc, self.case, self.cls = orc, case, cls
        self.B = B = max(B, S_ * L_)
        self.net, self.Ea, self.A = case.network()
        self.on = orc.OracleNetwork.from_flat(self.net)
        n, R = self.net.n_species, self.net.n_reactions
        rng = np.random.default_rng(7)
        if cls == "exact":
            assert B <= EXACT_MAX_TERMS
            self.U = rng.choice([0.5, 1.0, 2.0], (B, n))
            self.K = rng.integers(1, 9, (B, R)).astype(np.float64)
            self.w = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0], B)
            self.k0 = rng.integers(1, 9, R).astype(np.float64)
        else:
            self.U = 10.0 ** rng.uniform(-12, 0, (B, n))
            self.U[0] = 0.0; self.U[0, 0] = 1.0
            self.U[1, rng.random(n) < 0.3] = 0.0
            self.U[2, rng.choice(n, min(5, n), replace=False)] = -1e-14
            self.k0 = orc.arrhenius(self.Ea, self.A, 1000.0, k_max=1e12)
            self.K = self.k0[None, :] * rng.uniform(0.5, 2.0, (B, 1)) * rng.uniform(0.9, 1.1, (B, R))
            self.w = rng.normal(size=B)
            self.w[::5] = 0.0
            self.w[1::7] = -np.abs(self.w[1::7])
        self.K3 = self.K[:3].copy()
        self.row3 = rng.integers(0, 3, B).astype(np.int64)
        self.T = rng.uniform(600.0, 1200.0, B)                  # one temperature per state, none repeated
        self._rates, self._rbound, self._flux, self._seg = {}, {}, {}, {}

    def k_of(self, ksrc, b):
        if ksrc == "k":
            return self.K[b]
        if ksrc == "k_row":
            return self.K3[self.row3[b]]
        if ksrc == "shared":
            return self.k0
        # (no k_max: under the cap nearly every constant of these networks sits at the cap, and one reaction's could pass for another's)
        return self.orc.arrhenius(self.Ea, self.A, self.T[b])

    def rates(self, ksrc):
        """The oracle's rates[B][R]."""
        if ksrc not in self._rates:
            self._rates[ksrc] = np.stack([self.on.rates(self.k_of(ksrc, b), self.U[b]) for b in range(self.B)])
        return self._rates[ksrc]

    def extra(self, ksrc, rows):
        """Per-term relative slack of the temperature form for the given states (0 with rate constants given)."""
        if ksrc != "T":
            return 0.0
        return (2.0 * np.abs(self.Ea[None, :] / (RGAS * self.T[rows, None])) + 16.0) * EPS

    def rates_bound(self, ksrc, B):
        if ksrc not in self._rbound:
            self._rbound[ksrc] = (4 * EPS + self.extra(ksrc, np.arange(self.B))) * np.abs(self.rates(ksrc)) + 1e-300
        return self._rbound[ksrc][:B]

    def _sum(self, ksrc, rows, n_add):
        """(fsum reference [R], bound [R]) of sum over `rows` of w_b rate_b, summed on the device with n_add + 8 roundings allowed."""
        terms = self.w[rows, None] * self.rates(ksrc)[rows]
        ref = np.array([math.fsum(col) for col in terms.T.tolist()]) if len(rows) else np.zeros(terms.shape[1])
        a = np.abs(terms)
        return ref, (n_add + 8) * EPS * a.sum(axis=0) + (self.extra(ksrc, rows) * a).sum(axis=0) + 1e-300

    def flux(self, ksrc, B):
        if (ksrc, B) not in self._flux:
            self._flux[(ksrc, B)] = self._sum(ksrc, np.arange(B), B)
        return self._flux[(ksrc, B)]

    def seg_flux(self, ksrc):
        """(reference [S][R], bound [S][R]) of the segmented pass over the first S L states, segment s = states s L .. s L + seg_n[s] - 1."""
        if ksrc not in self._seg:
            got = [self._sum(ksrc, s * L_ + np.arange(SEG_N[s]), L_) for s in range(S_)]
            self._seg[ksrc] = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        return self._seg[ksrc]

    def seg_inputs(self):
        """The first S L states laid out [S][L] with NaN (and row indices out of range) behind seg_n: never read."""
        n = S_ * L_
        U, w, T, K = self.U[:n].copy(), self.w[:n].copy(), self.T[:n].copy(), self.K[:n].copy()
        row = self.row3[:n].copy()
        for s in range(S_):
            dead = slice(s * L_ + SEG_N[s], (s + 1) * L_)
            U[dead] = np.nan; w[dead] = np.nan; T[dead] = np.nan; K[dead] = np.nan; row[dead] = 1 << 40
        return U, w, T, K, row
