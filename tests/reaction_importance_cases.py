"""Reaction importance written plainly in NumPy - the reference of the reaction-elimination tests.

Definition (include/kinetica_hip.h, "reaction elimination"). Records, pairing, nu_A and den_A are drg_cases.py's: records()
gives the records, DrgRef the denominator contributions, den_A = math.fsum of |nu_A| |w| over the records with nu_A != 0.
    I_rho(b)      = max over the selected species A with nu_A(rho) != 0 of |nu_A| |w(b)| / den_A(b)   (0.0 where den_A == 0)
    importance[r] = max over the states of I_rho(b) for every reaction r of record rho

Bound (derived, not measured), per (record, species, state), with eps = 2^-53 and the error model of test_gpu_drg.py: a term
t = |nu| |q_f - q_r| is off by dterm <= |nu| ((6 eps + ex_f) |q_f| + (6 eps + ex_r) |q_r|) (DrgRef._terms; ex: the temperature
form's extra error of a rate), a denominator of n terms by dden <= sum of the dterm + n eps den (DrgRef._rowsum, as
DrgRef.state forms it), and the quotient by
    |I_got - I_ref| <= (dterm + I_ref dden) / den + 2 eps,      inf where den == 0 but dden > 0 (pure cancellation).
The maximum over a record's species and over the states moves by no more than the largest of these."""
import numpy as np

import drg_cases as dc

EPS = dc.EPS


class RiRef:
    """The per-reaction table of one (network, pairing) and the importance of given per-state rates."""

    def __init__(self, net, pairing):
        self.net, self.pairing, self.n, self.R = net, bool(pairing), net.n_species, net.n_reactions
        self.graph = dc.DrgRef(net, pairing)
        self.records = dc.records(net, pairing)
        self.partner = np.full(self.R, -1, np.int64)
        self.rec_of = np.full(self.R, -1, np.int64)
        ent = []                                     # (record, A, kf, kr, |nu|)
        self.slots = [dict() for _ in range(self.R)]     # per reaction {species: signed nu}: the forward's, flipped for the reverse
        for i, (kf, kr, nu, _) in enumerate(self.records):
            self.rec_of[kf] = i
            self.slots[kf] = dict(nu)
            if kr >= 0:
                self.rec_of[kr] = i
                self.partner[kf], self.partner[kr] = kr, kf
                self.slots[kr] = {s: -c for s, c in nu.items()}
            ent.extend((i, A, kf, kr, abs(c)) for A, c in nu.items())
        self.ent = np.array(ent, np.int64).reshape(-1, 5)

    def info(self):
        """The sizes kin_reaction_importance_plan_host reports."""
        return dict(records=len(self.records), paired_reactions=int(np.sum(self.partner >= 0)),
                    empty_reactions=int(sum(1 for s in self.slots if not s)))

    def state(self, q, ex=None, selected=None):
        """(I[R], bound[R]) of one state's rates q[R]; ex[R]: extra relative error of every rate (temperature form);
        selected: species ids (duplicates allowed) a reaction is judged by, None: all."""
        g = self.graph
        ex = np.zeros(len(q)) if ex is None else ex
        td, ed = g._terms(g.den, 1, q, ex)
        den, dden = g._rowsum(td, g.den_ptr), g._rowsum(ed, g.den_ptr)
        dden = dden + np.diff(g.den_ptr) * EPS * den
        term, dterm = g._terms(self.ent, 2, q, ex)
        A = self.ent[:, 1]
        dA, ddA = den[A], dden[A]
        pos = dA > 0
        safe = np.where(pos, dA, 1.0)
        I = np.where(pos, term / safe, 0.0)
        bound = np.where(pos, (dterm + I * ddA) / safe + 2 * EPS, np.where(ddA > 0, np.inf, 0.0))
        if selected is not None:
            on = np.zeros(self.n, bool)
            on[np.asarray(list(selected), dtype=np.int64)] = True
            I, bound = np.where(on[A], I, 0.0), np.where(on[A], bound, 0.0)
        rec_I, rec_b = np.zeros(len(self.records)), np.zeros(len(self.records))
        np.maximum.at(rec_I, self.ent[:, 0], I)
        np.maximum.at(rec_b, self.ent[:, 0], bound)
        return rec_I[self.rec_of], rec_b[self.rec_of]

    def importance(self, rates, ex=None, selected=None):
        """(importance[R], bound[R], I[B][R], bounds[B][R]) of rates[B][R]."""
        rates = np.atleast_2d(rates)
        if not len(rates):
            z = np.zeros(self.R)
            return z, z.copy(), np.zeros((0, self.R)), np.zeros((0, self.R))
        Is, bs = zip(*[self.state(rates[b], None if ex is None else ex[b], selected) for b in range(len(rates))])
        I, b = np.stack(Is), np.stack(bs)
        return I.max(axis=0), b.max(axis=0), I, b


# network -> [(species list or None, {pairing: importance})]: the hand values (dyadic: exact); species by position A, B, C / M
HAND = {
    "A_to_B": [(None, {1: [1.0], 0: [1.0]})],
    "A_eq_B_balanced": [(None, {1: [0.0, 0.0], 0: [0.5, 0.5]})],      # paired: w = 0, den = 0 -> exactly 0.0
    "2A_to_B": [(None, {1: [1.0], 0: [1.0]})],
    "A_M_to_B_M": [(None, {1: [1.0], 0: [1.0]}), ([2], {1: [0.0], 0: [0.0]})],      # the collider M never counts
    "A_B_to_2B": [(None, {1: [1.0, 1.0], 0: [1.0, 1.0]}), ([0], {1: [0.5, 0.5], 0: [0.5, 0.5]})],
}


_refs = {}


def ref_of(name, pairing):
    """RiRef of a drg_cases.synth_case network (cached)."""
    key = (name, bool(pairing))
    if key not in _refs:
        _refs[key] = RiRef(dc.synth_case(name).net, pairing)
    return _refs[key]


def case_rates(name, mode, B):
    """rates[B][R] (oracle) of a synth_case in a rate-constant mode, shared with the DRG reference's cache."""
    case = dc.synth_case(name)
    if mode not in case._rates or case._rates[mode].shape[0] < B:
        case._rates[mode] = np.stack([case.on.rates(case.k_of(mode, b), case.U[b]) for b in range(B)])
    return case._rates[mode][:B]
