"""Shared by tests/test_sweep_cases.py (no GPU), tests/test_gpu_sweep_exact.py and tests/test_gpu_tiled_exact.py: the references,
inputs and case lists of the two batched RHS sweeps - the caller-layout sweep (kernels.hip: sweep_reg_kernel, sweep_gen_kernel,
sweep_lds_kernel, sweep_big_kernel) and the library-order sweep (tiled_kernels.hip: tiled_sweep_kernel and its layout kernels).
A plain module: no fixtures, no test collection.

Exact inputs (the set of jac_cases and test_gpu_sweep_batches): u in {1/2, 1, 2}, integer k in 1 .. 8. A term nu k u_a [u_b] is a
multiple of 1/4 of magnitude at most 2 * 8 * 4 = 2^6, so every partial sum of up to 2^45 terms is a multiple of 1/4 below 2^51:
representable, whatever the order. The reference `exact_rhs` is therefore computed in FLOAT64 (not in integers): every product
and every sum it forms is exact for the same reason, so it is THE value, for all states at once (a sparse stoichiometry matrix
times the rate matrix - the order in which the sparse product adds does not matter). It is built from the reaction lists
(jac_cases.Reference reads net.reaction(r)), never from the compiled records or the library-order tables. A kernel that loses,
doubles or misplaces one term on any state differs from it; comparison by value (np.array_equal: -0.0 == 0.0).

Random inputs (test_gpu_timescale.Synth's): positive over 12 decades, ~1 % exact zeros, ~1 % entries at -1e-12; judged per entry
with jac_cases.Reference.rhs (longdouble) and jac_cases.bound_rhs(S, L) = (L + 4) u S, which holds for ANY summation order and
so covers the LDS atomics and the split accumulators. At most eight states per run are judged: the first, the last, and one
from each trip of the state loop (`sample_states`).

Temperature form. The tiled kernel forms its rate constants with arrhenius_fast_t<128> on the parameters tiled_params_kernel
stores. tests/exp_host.py replays that form on the host, but not the way the device enters it bit for bit: the device's
reciprocals (1 / (A N_A t_mult), 1 / RT) start from v_rcp_f64 and Newton steps, the replay divides (test_gpu_rate_constants,
mutation 8: "CPU: passes (the replay's seed is a division)"). So the SECOND option of the two holds here: the reference's k is
the longdouble Arrhenius law (oracle.arrhenius) and every term of reaction r carries the relative allowance
(2 |Ea_r / (R T)| + 16) u of timescale_cases / test_gpu_flux on top of bound_rhs (`bound_rhs_T`). Nothing is fitted to a device.
The structural case next to the realistic one has Ea = 0, A = j / N_A (k within a few ulp of j = 1 .. 8) and u in {1/2, 1, 2}:
every term is within 2^7 of every other, the allowance is 16 u per term, and a lost or doubled term is ~2^45 bounds away.

Cases. Each is the smallest network found that takes its path and carries the plan the query must report
(capi.sweep_plan_host / capi.tiled_sweep_plan_host at n_cu = 256; the GPU tests ask the live handle). `INSTANTIATIONS_*` list
every instantiation of the sweep kernels; test_sweep_cases.py asserts each is reached by a case or named in `NO_LAYOUT`."""
import os

import numpy as np

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from tests import jac_cases as jc
from tests.jac_cases import LD, U

N_CU = 256
R_GAS = 8.314462618
N_A = 6.02214076e23
K_BYTES_MAX = 150e6          # above this a per-state k of the largest batch is replaced by shared rate constants


# ------------------------------------------------------------------------------------------------------------ references
_SP_CACHE = {}


def _stoich(ref):
    """(R x N) sparse net stoichiometry of a Reference, from its term lists"""
    import scipy.sparse as sp
    key = id(ref)
    if key not in _SP_CACHE:
        _SP_CACHE[key] = (ref, sp.csr_matrix((ref.t_nu.astype(np.float64), (ref.t_rx, ref.t_sp)), shape=(ref.R, ref.N)))
    return _SP_CACHE[key][1]


def exact_rhs(ref, U_, K):
    """du[B][N] in float64 for ALL states: exact on the exact inputs (module docstring). K[B][R] or K[R] (shared)."""
    U_ = np.asarray(U_, np.float64)
    two = ref.b >= 0
    ub = np.where(two[None, :], U_[:, np.where(two, ref.b, 0)], 1.0)
    rates = np.asarray(K, np.float64) * U_[:, ref.a] * ub          # (B, R); K broadcasts when shared
    return np.asarray((_stoich(ref).T @ rates.T).T)


def exact_scale(ref, U_, K):
    """S[B][N] = sum of the absolute terms, float64 (exact on the exact inputs, where every rate is positive)"""
    U_ = np.asarray(U_, np.float64)
    two = ref.b >= 0
    ub = np.where(two[None, :], U_[:, np.where(two, ref.b, 0)], 1.0)
    rates = np.abs(np.asarray(K, np.float64) * U_[:, ref.a] * ub)
    return np.asarray((abs(_stoich(ref)).T @ rates.T).T)


def exact_inputs(B, N, R, seed, shared_k=False):
    rng = np.random.default_rng([seed, 17])
    U_ = 2.0 ** rng.integers(-1, 2, (B, N)).astype(np.float64)
    K = rng.integers(1, 9, R if shared_k else (B, R)).astype(np.float64)
    return U_, K


def random_inputs(B, N, R, seed, shared_k=False):
    rng = np.random.default_rng([seed, 29])
    U_ = 10.0 ** rng.uniform(-12, 0, (B, N))
    U_[rng.random((B, N)) < 0.01] = 0.0
    U_[rng.random((B, N)) < 0.01] = -1e-12
    K = 10.0 ** rng.uniform(-3, 9, R if shared_k else (B, R))
    return U_, K


def sample_states(B, grid):
    """at most eight states: the first, the last, one from each trip of the state loop (trip t = states [t grid, (t + 1) grid))"""
    trips = (B + grid - 1) // grid
    s = {0, B - 1}
    for t in range(trips):
        lo, hi = t * grid, min(B, (t + 1) * grid)
        s.add(lo + (hi - lo) // 2)
        if len(s) >= 8:
            break
    return sorted(s)[:8]


def trip_batches(grid):
    """the batch sizes of the state-loop test: one state, exactly one trip, one state into the second, three into the third"""
    return sorted({1, grid, grid + 1, 2 * grid + 3})


def judge_rhs(ref, k, u, dev, ex=None):
    """(inside, error / bound, worst entry) of one state against the longdouble reference; ex[R]: extra relative allowance per
    reaction (temperature form)"""
    f, S, L = ref.rhs(k, u)
    bound = jc.bound_rhs(S, L)
    if ex is not None:
        ts, tv = ref.rhs_terms(k, u)
        bound = bound + jc.accumulate(ts, np.abs(tv) * np.asarray(ex).astype(LD)[ref.t_rx], ref.N)[0]
    ok, ratio = jc.compare(dev, f, bound)
    return ok, ratio, jc.worst(dev, f, bound)


def arrhenius_allowance(Ea, T):
    """(2 |Ea / (R T)| + 16) u per reaction: the device's Arrhenius law against the longdouble one (timescale_cases)"""
    return (2 * np.abs(np.asarray(Ea).astype(LD) / (LD(R_GAS) * LD(T))) + 16) * U


def structural_arrhenius(R, seed):
    """(Ea = 0, A = j / N_A, j) with j in 1 .. 8: the device's k is j within the 16 u of arrhenius_allowance at any temperature"""
    j = np.random.default_rng([seed, 41]).integers(1, 9, R).astype(np.float64)
    return np.zeros(R), j / N_A, j


def structural_bound(ref, U_, j):
    """(reference, bound)[B][N] of the structural temperature case for ALL states in float64: the reference is exact_rhs with
    k = j (exact); the device's terms carry 16 u each for its rate constants and the sum (L + 4) u S, and two more units cover
    the float64 evaluation of this bound itself"""
    S = exact_scale(ref, U_, j)
    return exact_rhs(ref, U_, j), (ref.L_rhs[None, :] + 4 + 16 + 2) * float(U) * S


# --------------------------------------------------------------------------------------------------------------- networks
def pair_net(N, P, seed):
    """P forward reactions over uniformly drawn, distinct species, each followed by its exact reverse (adjacent pairs); the
    forward types of synthetic_crn (A -> B, A -> B + C, A -> 2B, A + B -> C + D, 2A -> B + C). Unlike synthetic_crn it does
    not tie the reaction count to the species count (species without any reaction keep an empty row) and has no hubs."""
    rng = np.random.default_rng([seed, N, P])
    M = P + P // 2 + 64                                     # candidates: rows with a repeated species or a repeated reaction go
    s = rng.integers(0, N, (M, 4))
    kind = rng.choice(5, M, p=[0.25, 0.35, 0.05, 0.30, 0.05])
    reacs, prods, seen = [], [], set()
    for (a, b, c, d), t in zip(s.tolist(), kind.tolist()):
        if len({a, b, c, d}) < 4:
            continue
        rs, ps = [([(a, 1)], [(b, 1)]), ([(a, 1)], [(b, 1), (c, 1)]), ([(a, 1)], [(b, 2)]), ([(a, 1), (b, 1)], [(c, 1), (d, 1)]),
                  ([(a, 2)], [(b, 1), (c, 1)])][t]
        key = frozenset((tuple(sorted(rs)), tuple(sorted(ps))))
        if key in seen:
            continue
        seen.add(key)
        reacs += [rs, ps]; prods += [ps, rs]
        if len(reacs) == 2 * P:
            break
    assert len(reacs) == 2 * P
    return from_lists(N, reacs, prods)


def block_order(net):
    """the same reactions presented as (p, P + p): all forward reactions, then their reverses (test_gpu_sweep_batches._block_order)"""
    return net.subset(np.concatenate([np.arange(0, net.n_reactions, 2), np.arange(1, net.n_reactions, 2)]))


def thinned(net, seed, frac=0.7):
    """minus a seeded 30 % of the reactions: pairs lose their partners (what the low-k cutoff leaves behind)"""
    keep = np.sort(np.random.default_rng(seed).choice(net.n_reactions, int(frac * net.n_reactions), replace=False))
    return net.subset(keep)


def _lists(net):
    rp = [net.reaction(r) for r in range(net.n_reactions)]
    return [[(int(s), int(c)) for s, c in x[0]] for x in rp], [[(int(s), int(c)) for s, c in x[1]] for x in rp]


def with_extra(net, reacs, prods):
    r0, p0 = _lists(net)
    return from_lists(net.n_species, r0 + reacs, p0 + prods)


def colliders_odd(net):
    """plus A + C -> B + C (C on both sides: an explicit-operand record), its reverse elsewhere in the list, 2A + C... is not
    expressible (molecularity 2), so a second collider with a different C, and one unpaired A -> B to make R odd"""
    n = net.n_species
    out = with_extra(net, [[(0, 1), (2, 1)], [(5, 1), (n - 1, 1)], [(3, 1)]], [[(1, 1), (2, 1)], [(6, 1), (n - 1, 1)], [(4, 1)]])
    if out.n_reactions % 2 == 0:
        out = with_extra(out, [[(7, 1)]], [[(8, 1)]])
    return out


def records_mod(net, mod, want):
    """plus unpaired reactions X -> Y until the general sweep's record count is `want` modulo `mod`"""
    P = capi.sweep_plan_host(net, N_CU, 1)["records"]
    add = (want - P) % mod
    n = net.n_species
    reacs = [[(i % n, 1), ((i + 1) % n, 1)] for i in range(add)]
    prods = [[((i + 2) % n, 2)] for i in range(add)]          # A + B -> 2C: no such reverse in the synthetic types
    out = with_extra(net, reacs, prods)
    assert capi.sweep_plan_host(out, N_CU, 1)["records"] % mod == want
    return out


BIG_H = 10000


def big_net(N, colliders=False):
    """A network for the large-N sweep with references to hubs AND tail species. The hub set is the 10 000 species referenced
    most often (ties by index): three passes of hub-hub records A + B <-> C + D over shifted groups of four give every species
    below 10 000 three references; no species from 10 000 on gets more than two, so the hubs are species [0, 10 000) exactly.
    Tail-tail records cover the first and the last tail species (996 each; 60 at N = 10 242; the rest of the tail has no
    reaction: rows written as 0), up to 100 hub-tail records. colliders: six one-directional reactions X + C -> Y + C (explicit-operand records; such a network is
    never `adjacent`: a reaction with a species on both sides has no partner) with the collider a hub, a tail species, and
    with X, Y hubs or tail species."""
    reacs, prods = [], []

    def pair(rs, ps):
        reacs.extend([rs, ps]); prods.extend([ps, rs])

    for o in range(3):                                              # hub-hub: A + B <-> C + D, 7 500 records
        for i in range(o, BIG_H + o, 4):
            a, b, c, d = [(i + j) % BIG_H for j in range(4)]
            pair([(a, 1), (b, 1)], [(c, 1), (d, 1)])
    t0 = BIG_H
    tt = min(996, (N - BIG_H) // 4 // 3 * 3)                        # species per tail-tail block (242 tail species at N = 10 242)
    nht = min(100, (N - BIG_H) // 8)
    for base in (t0, N - tt):                                       # tail-tail: A <-> B + C and 2A <-> B + C alternating
        for j in range(0, tt, 3):
            a, b, c = base + j, base + j + 1, base + j + 2
            pair([(a, 2 if j % 2 else 1)], [(b, 1), (c, 1)])
    for j in range(nht):                                            # hub-tail: H + T <-> H' + T'
        pair([(j, 1), (t0 + tt + 2 * j, 1)], [(j + 100, 1), (t0 + tt + 2 * j + 1, 1)])
    if colliders:
        q = t0 + tt + 2 * nht
        assert q + 10 < N - tt - 2
        for x, y, c in ((q, q + 1, 5), (6, 7, q + 2), (q + 3, q + 4, q + 5), (q + 6, 8, q + 7), (9, q + 8, 10), (N - tt - 1, q + 9, N - tt - 2)):
            reacs.append([(x, 1), (c, 1)]); prods.append([(y, 1), (c, 1)])
    return from_lists(N, reacs, prods)


def wide_net(N, P=150):
    """a few hundred reactions over a very wide species range (sweep_lds_kernel<false, *> and the per-state path): species
    drawn from the whole range, so every species tile of 16 384 and both ends of the row are hit"""
    net = pair_net(N, P - 2, 3)
    return with_extra(net, [[(N - 1, 1)], [(N - 2, 1), (0, 1)], [(16383, 1)], [(16384, 2)]],
                      [[(N - 2, 1), (0, 1)], [(N - 1, 1)], [(16384, 2)], [(16383, 1)]])


# ------------------------------------------------------------------------------------------------ caller-layout sweep cases
class SweepCase:
    def __init__(self, name, build, expect, bits=(0, 0, 0), batches=None, against=None):
        self.name, self.build, self.expect, self.bits, self.batches, self.against = name, build, expect, bits, batches, against

    @property
    def inst(self):
        e = self.expect
        k = e["kernel"]
        if k == "reg":
            return ("reg", e["TR"], e["BLK"], e["BS"])
        if k == "gen":
            return ("gen", e["BS"])
        if k == "lds":
            return ("lds", e["U_IN_LDS"], e["ADJ"])
        if k == "big":
            return ("big", e["ADJ"])
        return ("per_state",)


INSTANTIATIONS_SWEEP = ([("reg", tr, blk, bs) for tr in (0, 4, 8) for blk in (0, 1) for bs in (256, 512, 1024)] +
                        [("gen", bs) for bs in (256, 512, 1024)] + [("lds", u, a) for u in (0, 1) for a in (0, 1)] +
                        [("big", a) for a in (0, 1)] + [("per_state",)])
assert len(INSTANTIATIONS_SWEEP) == 18 + 3 + 4 + 2 + 1


def _stream(P, bs, tr, ilp=4):
    """n_a batches of ILP rows and n_b of ILP + 1 over the S = ceil(P / BS) - TR streamed rows, in ceil(S / (ILP + 1)) rounds"""
    S = max(0, -(-P // bs) - tr)
    rounds = -(-S // (ilp + 1))
    n_b = max(0, S - ilp * rounds)
    return rounds - n_b, n_b


def _reg_expect(bs, P, blk, **more):
    tr = 8 if P // bs >= 8 else (4 if P // bs >= 4 else 0)
    n_a, n_b = _stream(P, bs, tr)
    return dict(kernel="reg", BS=bs, TR=tr, ILP=4, BLK=blk, ADJ=1 - blk, U_IN_LDS=1, n_a=n_a, n_b=n_b, records=P, **more)


def _sweep_cases():
    cs = []
    # sweep_reg_kernel: BS x TR x pairing; P below 4 BS, in [4 BS, 8 BS), at or above 8 BS
    for bs, N in ((256, 300), (512, 2562), (1024, 5122)):
        for tr, P in ((0, 3 * bs + 1), (4, 6 * bs + 1), (8, 13 * bs + 1)):
            for blk in (0, 1):
                build = (lambda N=N, P=P, blk=blk: block_order(pair_net(N, P, 1)) if blk else pair_net(N, P, 1))
                e = _reg_expect(bs, P, blk)
                assert e["TR"] == tr
                cs.append(SweepCase(f"reg_bs{bs}_tr{tr}_{'blk' if blk else 'adj'}", build, e))
    # the stream plans of test_gpu_sweep_batches (synthetic CRNs: split accumulators)
    for N, bs, Rs in ((300, 256, (2000, 4098, 6144, 6658, 6500, 8392)), (5200, 1024, (16386, 26626, 25576))):
        for R in Rs:
            cs.append(SweepCase(f"reg_stream_bs{bs}_R{R}", lambda N=N, R=R: synthetic_crn(N, R)[0], _reg_expect(bs, R // 2, 0)))
    cs.append(SweepCase("reg_stream_bs256_R6658_blk", lambda: block_order(synthetic_crn(300, 6658)[0]), _reg_expect(256, 3329, 1)))
    # sweep_gen_kernel
    for bs, N, R in ((256, 300, 6658), (512, 2562, 9218), (1024, 5122, 16386)):
        cs.append(SweepCase(f"gen_bs{bs}_thinned", lambda N=N, R=R: thinned(synthetic_crn(N, R)[0], R),
                            dict(kernel="gen", BS=bs, ADJ=0, U_IN_LDS=1, n_expl=0)))
    cs.append(SweepCase("gen_colliders_odd_R", lambda: colliders_odd(thinned(synthetic_crn(300, 2000)[0], 5)),
                        dict(kernel="gen", BS=256, n_expl=2)))
    cs.append(SweepCase("gen_records_1_mod_1024", lambda: records_mod(thinned(synthetic_crn(300, 2000)[0], 6), 1024, 1),
                        dict(kernel="gen", BS=256)))
    # sweep_lds_kernel<true, ADJ>: the fallbacks of the register-resident kernel
    lds = dict(kernel="lds", BS=1024, U_IN_LDS=1, n_tiles=1)
    cs.append(SweepCase("lds_odd_N_adj", lambda: pair_net(301, 700, 2), dict(lds, ADJ=1)))
    cs.append(SweepCase("lds_odd_N_blk", lambda: block_order(pair_net(301, 700, 2)), dict(lds, ADJ=0)))
    even = lambda: pair_net(300, 700, 2)
    cs.append(SweepCase("lds_even_N_aligned_is_reg", even, _reg_expect(256, 700, 0)))
    cs.append(SweepCase("lds_even_N_u_off8", even, dict(lds, ADJ=1), bits=(8, 0, 0), against="lds_even_N_aligned_is_reg"))
    cs.append(SweepCase("lds_even_N_du_off8", even, dict(lds, ADJ=1), bits=(0, 0, 8), against="lds_even_N_aligned_is_reg"))
    cs.append(SweepCase("lds_even_N_k_off8", even, dict(lds, ADJ=0, BLK=0), bits=(0, 8, 0), against="lds_even_N_aligned_is_reg"))
    # sweep_lds_kernel<false, *>: N = 65 534 (beyond the large-N tables' label space, within 16-bit species ids), B = 3
    wide = dict(kernel="lds", BS=1024, U_IN_LDS=0, n_tiles=4)
    cs.append(SweepCase("lds_tiles_65534_adj", lambda: wide_net(65534), dict(wide, ADJ=1), batches=(3,)))
    cs.append(SweepCase("lds_tiles_65534_blk", lambda: block_order(wide_net(65534)), dict(wide, ADJ=0), batches=(3,)))
    cs.append(SweepCase("per_state_65535", lambda: wide_net(65535), dict(kernel="per_state"), batches=(3,)))
    # sweep_big_kernel<ADJ>: both values of tail_by_species; k 8 bytes off, or a collider, runs the index-gather instantiation
    for N, by_sp, tiles in ((10242, 1, 1), (55472, 0, 3)):
        big = dict(kernel="big", BS=1024, hubs=BIG_H, tail_by_species=by_sp, tail_tiles=tiles)
        cs.append(SweepCase(f"big_{N}_adj", lambda N=N: big_net(N), dict(big, ADJ=1, n_expl=0)))
        cs.append(SweepCase(f"big_{N}_k_off8", lambda N=N: big_net(N), dict(big, ADJ=0, n_expl=0), bits=(0, 8, 0), against=f"big_{N}_adj"))
        cs.append(SweepCase(f"big_{N}_colliders", lambda N=N: big_net(N, True), dict(big, ADJ=0, n_expl=6)))
    return {c.name: c for c in cs}


SWEEP_CASES = _sweep_cases()

# ---------------------------------------------------------------------------------------------------------- tiled sweep cases
class TiledCase:
    """expect: BS, UN, rows (iteration rows per segment), singles, identity, n_copy (exact), odd_batches_k / odd_batches_T
    (some segment has an odd number of batches in that form)"""

    def __init__(self, name, n, r, entries=None, thin=False, **expect):
        self.name, self.n, self.r, self.entries, self.thin, self.expect = name, n, r, entries, thin, expect

    def env(self):
        return {"KIN_TILED_ENTRIES": self.entries} if self.entries else {}

    def build(self):
        net, Ea, A = synthetic_crn(self.n, self.r)
        if self.thin:
            keep = np.sort(np.random.default_rng(21).choice(self.r, int(0.7 * self.r), replace=False))
            return net.subset(keep), Ea[keep], A[keep]
        return net, Ea, A

    def insts(self):
        e = self.expect
        return [(e["BS"], "singles" if e["singles"] else "k", e["UN"]), (e["BS"], "T", e["UN"])]


INSTANTIATIONS_TILED = [(bs, form, un) for bs in (256, 512, 1024) for form in ("k", "singles", "T") for un in (5, 10)]
# instantiations (and layout kinds) for which no layout of test size was found, by name
NO_LAYOUT = {
    "windowed_UN10": "a windowed layout with more than 5 BS hubs or window entries: KIN_TILED_ENTRIES caps E at 10 176 and a window "
                     "needs room next to the hubs; none turned up for N <= 8 194 at any cap tried (UN = 10 runs on one-segment "
                     "layouts only in this list)",
}


def _tiled_cases():
    T = TiledCase
    cs = [
        T("t256_un5_one_row", 40, 100, BS=256, UN=5, rows=[8], singles=0, identity=1, n_copy=0),
        T("t256_un5_copies", 300, 6000, BS=256, UN=5, rows=[12], singles=0, identity=1, n_copy=35),
        T("t256_un5_copies_singles", 300, 6000, thin=True, BS=256, UN=5, rows=[12], singles=1, identity=1, n_copy=21),
        T("t256_un10_five_batches", 1500, 5000, BS=256, UN=10, rows=[10], singles=0, identity=1, n_copy=14),
        T("t256_un10_singles", 1500, 5000, thin=True, BS=256, UN=10, rows=[10], singles=1, identity=1, n_copy=14),
        T("t256_windows_odd_tail", 2300, 11500, "2000", BS=256, UN=5, rows=[12, 12], singles=0, identity=0, n_copy=49),
        T("t256_windows_odd_tail_singles", 2300, 11500, "2000", thin=True, BS=256, UN=5, rows=[12, 12], singles=1, identity=0, n_copy=42),
        T("t256_windows_uneven_rows", 2000, 14000, "1200", BS=256, UN=5, rows=[12, 8, 8], singles=0, identity=0, n_copy=63),
        T("t512_un5", 2301, 11500, BS=512, UN=5, rows=[12], singles=0, identity=1, n_copy=56),
        T("t512_un5_singles", 2301, 11500, thin=True, BS=512, UN=5, rows=[12], singles=1, identity=1, n_copy=49),
        T("t512_un10", 3000, 11000, BS=512, UN=10, rows=[12], singles=0, identity=1, n_copy=49),
        T("t512_un10_singles", 3000, 11000, thin=True, BS=512, UN=10, rows=[10], singles=1, identity=1, n_copy=42),
        T("t512_windows", 3000, 15000, "1400", BS=512, UN=5, rows=[8, 8, 8, 8], singles=0, identity=0, n_copy=56),
        T("t512_windows_singles", 3000, 15000, "1400", thin=True, BS=512, UN=5, rows=[8, 8, 8, 8], singles=1, identity=0, n_copy=56),
        T("t1024_un10", 6000, 22000, BS=1024, UN=10, rows=[12], singles=0, identity=1, n_copy=84),
        T("t1024_un10_singles", 6000, 22000, thin=True, BS=1024, UN=10, rows=[10], singles=1, identity=1, n_copy=77),
        T("t1024_un5", 4900, 24500, BS=1024, UN=5, rows=[12], singles=0, identity=1, n_copy=98),
        T("t1024_un5_singles", 4900, 24500, thin=True, BS=1024, UN=5, rows=[12], singles=1, identity=1, n_copy=91),
        T("t1024_windows_odd_N_two_pieces", 8193, 41000, "4200", BS=1024, UN=5, rows=[8, 8, 8], singles=0, identity=0, n_copy=175),
        T("t1024_windows_even_N_two_pieces", 8194, 41000, "4200", BS=1024, UN=5, rows=[8, 8, 8], singles=0, identity=0, n_copy=175),
        T("t1024_windows_two_pieces_singles", 8194, 41000, "4200", thin=True, BS=1024, UN=5, rows=[8, 8, 8], singles=1, identity=0, n_copy=161),
    ]
    return {c.name: c for c in cs}


TILED_CASES = _tiled_cases()

_BUILT = {}


def built(kind, name):
    """(network, Reference[, Ea, A]) of a case, built once per process"""
    key = (kind, name)
    if key not in _BUILT:
        if kind == "sweep":
            net = SWEEP_CASES[name].build()
            _BUILT[key] = (net, jc.Reference(net))
        else:
            net, Ea, A = TILED_CASES[name].build()
            _BUILT[key] = (net, jc.Reference(net), Ea, A)
    return _BUILT[key]


class tiled_env:
    """the layout switches of a tiled case, set while a layout is built (host query or handle)"""

    def __init__(self, case):
        self.env = case.env()

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ("KIN_TILED_ENTRIES", "KIN_TILED_SINGLES")}
        for k in self.old:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def batches_per_segment(rows, nb):
    return [r // nb for r in rows]


def check_tiled_layout(case, L, plan_k, plan_T):
    """what a tiled case is named after, from the layout tables and the two plans"""
    e = case.expect
    rows = np.diff(L["seg_q"]).tolist()
    assert L["BS"] == e["BS"] == plan_k["BS"] == plan_T["BS"], (case.name, L["BS"])
    assert rows == e["rows"], (case.name, rows)
    assert L["n_copy"] == e["n_copy"] == plan_k["n_copy"], (case.name, L["n_copy"])
    assert int(L["has_singles"]) == e["singles"] == plan_k["SINGLES"] == plan_k["has_singles"], case.name
    assert plan_T["SINGLES"] == 0 and plan_T["TMODE"] == 1 and plan_k["TMODE"] == 0
    assert plan_k["UN"] == plan_T["UN"] == e["UN"], (case.name, plan_k["UN"])
    assert plan_k["NB"] == (4 if e["UN"] == 5 else 2) and plan_T["NB"] == 2
    ident = bool(np.array_equal(L["species_of_lib"], np.arange(len(L["species_of_lib"]))))
    assert int(ident) == e["identity"] == plan_k["identity"], case.name
    assert plan_k["windows"] == L["T"] == len(rows) and (L["T"] > 1) == (not ident)
    for r in rows:                                  # whole batches, two at least (tiled.hpp)
        assert r % plan_k["NB"] == 0 and r >= 8
