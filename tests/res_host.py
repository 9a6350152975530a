"""ctypes binding of tests/native/libkin_resident_host.so - TEST INFRASTRUCTURE: the CPU replay of the resident integrator
(the controller of kinetica_jl_amd/csrc/resident_core.hpp over a sequential backend)."""
import ctypes
import os
import subprocess
from ctypes import POINTER, c_double, c_int, c_int32, c_int64, c_void_p

import numpy as np

from kinetica_jl_amd import capi

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
_LIB = os.environ.get("KIN_RES_HOST_PATH", os.path.join(_HERE, "libkin_resident_host.so"))   # (override: mutation checks)
_lib = None


class ResResult(ctypes.Structure):
    _fields_ = [("retcode", c_int32), ("pad", c_int32), ("n_saved", c_int64), ("final_abstol", c_double), ("final_reltol", c_double)] + \
               [(n, c_int64) for n in ("n_steps", "n_rejected", "n_rhs", "n_jac", "n_factor", "n_linsolve", "n_newton_fail", "n_chunks",
                                        "n_restarts", "n_retries", "n_lu_reused", "n_bad_pivot", "n_lu_dropped")] + [("prof", c_int64 * 20)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "prof"}


def build():
    subprocess.check_call(["make", "-C", _HERE, "-s"])


def lib():
    global _lib
    if _lib is None:
        capi.lib()                      # libkinetica_hip.so first (the replay links its host-side C++)
        if not os.path.exists(_LIB):
            build()
        L = ctypes.CDLL(_LIB)
        P64, PD = POINTER(c_int64), POINTER(c_double)
        L.res_host_create.restype = c_void_p
        L.res_host_create.argtypes = [c_int64, c_int64, P64, P64, P64, P64, P64, P64, c_int, POINTER(c_int), P64]
        L.res_host_destroy.argtypes = [c_void_p]
        L.res_host_set_arrhenius.argtypes = [c_void_p, PD, PD, c_double, c_double]
        L.res_host_newton_solve.argtypes = [c_void_p, c_double, PD, PD, PD, PD]
        L.res_host_rows.restype = c_int64
        L.res_host_rows.argtypes = [POINTER(capi.KinParams)]
        L.res_host_solve.argtypes = [c_void_p, POINTER(capi.KinParams), PD, PD, PD, PD, PD, c_int64, c_int, PD, PD, P64, POINTER(ResResult)]
        P32 = POINTER(c_int32)
        L.res_host_slot_rules.restype = None
        L.res_host_slot_rules.argtypes = [c_int, P32, PD, P64, P64, P64, c_int, c_double, c_double, c_int64, c_int64, c_int64, c_int64, P32]
        L.res_host_drift_check.argtypes = [c_void_p, c_int, PD, PD, P32, PD, c_double, PD, P32]
        L.res_host_step_op.argtypes = [c_void_p, c_int, P32, PD, PD, PD, PD]
        L.res_host_corrector_loop.restype = None
        L.res_host_corrector_loop.argtypes = [c_int, c_int, PD, PD, PD]
        # the host parts of the ensemble call layer (tests/native/ensemble_call_host.cpp)
        L.ens_host_block.restype = None
        L.ens_host_block.argtypes = [POINTER(capi.KinParams), c_int64, c_int64, c_int64, P64, P64, c_int64, c_int64, c_int64, P64]
        L.ens_host_thread_share.restype = None
        L.ens_host_thread_share.argtypes = [c_int64, c_int64, P64, P64]
        L.ens_host_finish.restype = c_int64
        L.ens_host_finish.argtypes = [c_int64, c_int64, P64, P32, P64, PD, PD, P64, P32, POINTER(capi.KinStats), P64]
        L.ens_host_runner.argtypes = [c_int64, c_int64, P32, P64, ctypes.c_char_p, c_int64]
        # the launch plans of the event-time and resampling passes and the stored record as it lies (tests/native/pass_plan_host.cpp)
        L.plan_host_constants.restype = None
        L.plan_host_constants.argtypes = [P32]
        for f in (L.plan_host_event, L.plan_host_resample):
            f.restype = None
            f.argtypes = [c_int64, c_int64, c_int64, c_int, P32]
        L.plan_host_record_download.argtypes = [c_void_p, PD, c_int64]
        _lib = L
    return _lib


def _plan(entry, a, b, c, n_cu):
    out = np.zeros(2, np.int32)
    getattr(lib(), entry)(int(a), int(b), int(c), int(n_cu), out.ctypes.data_as(POINTER(c_int32)))
    return int(out[0]), int(out[1])


def event_plan(S, L, N, n_cu):
    """kin::event_plan: (wavefronts, rows of a part); reads KIN_EVENT_WAVES and KIN_EVENT_PART_ROWS."""
    return _plan("plan_host_event", S, L, N, n_cu)


def resample_plan(S, Q, N, n_cu):
    """kin::resample_plan: (queries of a tile, wavefronts); reads KIN_RESAMPLE_TILE_QUERIES and KIN_RESAMPLE_WAVES."""
    return _plan("plan_host_resample", S, Q, N, n_cu)


def plan_constants():
    out = np.zeros(6, np.int32)
    lib().plan_host_constants(out.ctypes.data_as(POINTER(c_int32)))
    return dict(zip(("EVENT_LANES", "EVENT_WAVES_MAX", "EVENT_ROWS_IN_FLIGHT", "RESAMPLE_SLICE", "RESAMPLE_WAVES_MAX", "RESAMPLE_TILE_MAX"),
                    (int(v) for v in out)))


def stored_record(h):
    """The stored ensemble of a capi.HipNetwork as it lies on the device, [K][n_rows][N]: the rows past a member's n_saved too."""
    K, rows, n, _ = h.ensemble_size()
    out = np.empty((K, rows, n))
    rc = lib().plan_host_record_download(h.handle, _pd(out), out.size)
    assert rc == 0, f"plan_host_record_download: {rc}"
    return out


def _pd(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def slot_rules(table, q):
    """(nearest, victim) of bdf_rules.hpp's slot_nearest / slot_first_free / slot_lru over HostBackend's slot records. table: dict of
    valid, c_fact, jac_stamp, step_stamp, last_use arrays; q: dict of c, band, n_restarts, max_age, n_steps, step_age, n_slots"""
    v = np.ascontiguousarray(table["valid"], np.int32)
    cf = np.ascontiguousarray(table["c_fact"], np.float64)
    st = [np.ascontiguousarray(table[k], np.int64) for k in ("jac_stamp", "step_stamp", "last_use")]
    out = np.zeros(2, np.int32)
    P32, P64 = POINTER(c_int32), POINTER(c_int64)
    lib().res_host_slot_rules(len(v), v.ctypes.data_as(P32), _pd(cf), *[a.ctypes.data_as(P64) for a in st], int(q["n_slots"]), q["c"], q["band"],
                              int(q["n_restarts"]), int(q["max_age"]), int(q["n_steps"]), int(q["step_age"]), out.ctypes.data_as(P32))
    return int(out[0]), int(out[1])


STEP_OPS = dict(vec=0, save_y=1, set_time=2, norms=3, init_D=4, predict=5, accept=6, change_D=7, interp=8, newton=9, corrector=10)
STEP_DARGS = ("atol", "rtol", "h", "t", "h_abs", "ts", "c_fact", "c", "upd", "rate_max", "crate0", "tol_first", "tol", "dy_first_max", "ec",
              "ec_m", "ec_p")
ATTEMPT_FIELDS = ("done", "converged", "nonfinite", "any_negative", "deep_negative", "n_iter", "err", "err_m", "err_p", "crate", "predicts",
                  "iterations")


def corrector_loop(n_species, sums, order=3, c=1.0, upd=1.0, rate_max=1.0, crate0=1.0, tol_first=-1.0, tol=0.03, dy_first_max=0.2):
    """res_corrector_loop (resident_core.hpp) over a scripted backend whose iteration i returns sums[i] = (s, se, sm, sp, neg):
    dict of ATTEMPT_FIELDS"""
    sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 5)
    cin = np.array([order, c, upd, rate_max, crate0, tol_first, tol, dy_first_max], np.float64)
    out = np.zeros(len(ATTEMPT_FIELDS))
    lib().res_host_corrector_loop(int(n_species), len(sums), _pd(sums), _pd(cin), _pd(out))
    return dict(zip(ATTEMPT_FIELDS, out))


class HostResident:
    def __init__(self, net, lu_opt=None):
        arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (net.reac_ptr, net.reac_idx, net.reac_sto, net.prod_ptr, net.prod_idx, net.prod_sto)]
        self.n, self.nr = int(net.n_species), int(net.n_reactions)
        info = np.zeros(8, np.int64)
        opt = (c_int * 5)(*(lu_opt or [0, 0, 0, 0, 0]))
        self._h = lib().res_host_create(self.n, self.nr, *[a.ctypes.data_as(POINTER(c_int64)) for a in arrs], 0, opt, info.ctypes.data_as(POINTER(c_int64)))
        assert self._h, "res_host_create failed"
        self.info = dict(ns=int(info[0]), m=int(info[1]), rounds=int(info[2]), solve_mode=int(info[3]), w_size=int(info[4]))

    def close(self):
        if getattr(self, "_h", None):
            lib().res_host_destroy(self._h)
            self._h = None

    __del__ = close

    def set_arrhenius(self, Ea, A, k_max=None, t_mult=1.0):
        Ea, A = np.ascontiguousarray(Ea, np.float64), np.ascontiguousarray(A, np.float64)
        lib().res_host_set_arrhenius(self._h, _pd(Ea), _pd(A), float("nan") if k_max is None else k_max, t_mult)

    def newton_solve(self, c, k, u, b):
        k, u, b = (np.ascontiguousarray(a, np.float64) for a in (k, u, b))
        x = np.empty(self.n)
        bad = lib().res_host_newton_solve(self._h, c, _pd(k), _pd(u), _pd(b), _pd(x))
        return x, bad

    def step_op(self, op, state, ctrl, entry, k=None):
        """one operation of the replay's backend or controller on a state block of kin_step_probe's layout (res_host_step_op):
        op: a key of STEP_OPS (vec: entry['aux'] = the vector operation 0 .. 5); entry: order, aux, row and the keys of STEP_DARGS,
        everything left out 0 except order = 1. Returns (state, ctrl) after the operation, or None for arguments out of range."""
        st = np.array(state, dtype=np.float64, order="C"); ct = np.array(ctrl, dtype=np.float64, order="C")
        assert st.shape == (capi.STEP_ROWS, self.n) and ct.shape == (capi.STEP_CTRL,)
        ia = np.array([entry.get("order", 1), entry.get("aux", 0), entry.get("row", 0)], np.int32)
        da = np.array([float(entry.get(q, 0.0)) for q in STEP_DARGS])
        kk = None if k is None else np.ascontiguousarray(k, np.float64)
        rc = lib().res_host_step_op(self._h, STEP_OPS[op], ia.ctypes.data_as(POINTER(c_int32)), _pd(da), _pd(kk), _pd(st), _pd(ct))
        return (st, ct) if rc == 0 else None

    def drift_check(self, jv_slots, c_fact, valid, jv_now, max_drift):
        """HostBackend::drift_check on slots made from the given Jacobian values (pattern order): (jd[ns][N], valid afterwards[ns],
        number dropped)"""
        jv_slots = np.ascontiguousarray(jv_slots, np.float64); jv_now = np.ascontiguousarray(jv_now, np.float64)
        c_fact = np.ascontiguousarray(c_fact, np.float64); valid = np.ascontiguousarray(valid, np.int32)
        ns = len(c_fact)
        assert jv_slots.shape == (ns, len(jv_now))
        jd = np.empty((ns, self.n)); after = np.zeros(ns, np.int32)
        P32 = POINTER(c_int32)
        n = lib().res_host_drift_check(self._h, ns, _pd(jv_slots), _pd(c_fact), valid.ctypes.data_as(P32), _pd(jv_now), float(max_drift),
                                       _pd(jd), after.ctypes.data_as(P32))
        return jd, after, n

    def solve(self, pars, u0, k0=None, tstops=None, T_stops=None, k_table=None, n_slots=0):
        u0 = np.ascontiguousarray(u0, np.float64)
        rows = lib().res_host_rows(ctypes.byref(pars))
        t = np.empty(rows); u = np.empty((rows, self.n))
        ns = c_int64(0)
        res = ResResult()
        n_stops = 0 if tstops is None else len(tstops)
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
        k0, tstops, T_stops, k_table = f(k0), f(tstops), f(T_stops), f(k_table)
        rc = lib().res_host_solve(self._h, ctypes.byref(pars), _pd(u0), _pd(k0), _pd(tstops), _pd(T_stops), _pd(k_table), n_stops, n_slots,
                                  _pd(t), _pd(u), ctypes.byref(ns), ctypes.byref(res))
        return t[:ns.value], u[:ns.value], rc, res.as_dict()
