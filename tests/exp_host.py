"""ctypes binding of tests/native_exp/libkin_exp_host.so - TEST INFRASTRUCTURE: the CPU replay of
kinetica_jl_amd/csrc/exp_tab.hpp (table-driven exp, division-free Arrhenius form)."""
import ctypes
import os
import subprocess
from ctypes import POINTER, c_double, c_int, c_int64

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_exp")
_LIB = os.environ.get("KIN_EXP_HOST_PATH", os.path.join(_HERE, "libkin_exp_host.so"))   # (override: mutation checks)
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = ctypes.CDLL(_LIB)
        PD = POINTER(c_double)
        L.exp2_table.argtypes = [PD]
        for n in ("exp_tab_512", "exp_tab_128"):
            getattr(L, n).argtypes = [PD, c_int64, PD]
        for n in ("arrhenius_fast_512", "arrhenius_fast_128", "arrhenius_literal"):
            getattr(L, n).argtypes = [PD, PD, c_int64, c_double, c_int, c_double, c_double, PD]
        _lib = L
    return _lib


def _pd(a):
    return a.ctypes.data_as(POINTER(c_double))


def exp2_table():
    out = np.empty(512)
    lib().exp2_table(_pd(out))
    return out


def exp_tab(x, TAB=512):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    getattr(lib(), f"exp_tab_{TAB}")(_pd(x), x.size, _pd(out))
    return out


def arrhenius(Ea, A, T, k_max=None, t_mult=1.0, form="fast_512"):
    """form: fast_512 / fast_128 (arrhenius_fast_t entered as rate_table_kernel enters it) or literal (arrhenius_one, host exp)"""
    Ea, A = np.ascontiguousarray(Ea, np.float64), np.ascontiguousarray(A, np.float64)
    out = np.empty_like(Ea)
    if k_max is not None and np.isinf(k_max):
        k_max = None                      # as kin_set_arrhenius: a cap at +inf is no cap
    fn = getattr(lib(), "arrhenius_" + form)
    fn(_pd(Ea), _pd(A), Ea.size, float(T), int(k_max is not None), float("nan") if k_max is None else float(k_max), float(t_mult), _pd(out))
    return out
