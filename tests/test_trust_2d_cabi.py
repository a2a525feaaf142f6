"""CPU-only checks of the public surface of the 2D trust-region step and rounds: vch2d_hess_cg_tr and
vch2d_pgd_trust are declared in include/vch.h, exported by the built library and bound in _lib.SIGNATURES with as many ctypes
arguments as the header declares parameters; Engine2D and GD2_configured carry the Python side.  No compute calls."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vch2d_hess_cg_tr", "vch2d_pgd_trust")


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _declared_params(name):
    """The parameters of `name` as include/vch.h declares them, comments removed."""
    src = open(os.path.join(ROOT, "include", "vch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/vch.h"
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound_with_the_headers_argument_count(V, name):
    params = _declared_params(name)
    lib = ctypes.CDLL(V.LIB_PATH)
    assert hasattr(lib, name), f"{name} is not exported"
    sigs = import_module(V.PKG_NAME + "._lib").SIGNATURES
    assert name in sigs
    restype, argtypes = sigs[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params), (len(argtypes), params)


def test_the_tr_entry_point_is_hess_cg_plus_two_arguments(V):
    base, tr = _declared_params("vch2d_hess_cg"), _declared_params("vch2d_hess_cg_tr")
    assert tr[:len(base)] == base and len(tr) == len(base) + 2
    assert tr[-2].replace(" ", "") == "constdouble*radius" and tr[-1].replace(" ", "") == "double*xnorm_out"
    sigs = import_module(V.PKG_NAME + "._lib").SIGNATURES
    assert sigs["vch2d_hess_cg_tr"][1][:len(base)] == sigs["vch2d_hess_cg"][1]


def test_pgd_trust_has_the_1d_arguments_with_rtol_after_tol():
    one = [p.replace("vch1d_ctx", "vch2d_ctx") for p in _declared_params("vch1d_pgd_trust")]
    two = _declared_params("vch2d_pgd_trust")
    at = [p.split()[-1] for p in one].index("tol")
    assert two == one[:at + 1] + ["double rtol"] + one[at + 1:]


def test_engine_and_driver_surface(V):
    E = V.Engine2D
    assert callable(E.hess_cg_trust) and callable(E.pgd_trust)
    assert E.TRUST_CG_STATUS[4] == "boundary" and E.TRUST_CG_STATUS[:4] == E.CG_STATUS
    assert E.TRUST_STATUS[6] == "rejected" and E.TRUST_STATUS[:6] == E.NEWTON_STATUS
    sig = inspect.signature(E.hess_cg_trust)
    assert list(sig.parameters)[1:4] == ["k", "radius", "rhs"]
    base = [p for p in inspect.signature(E.hess_cg).parameters]
    assert [p for p in sig.parameters if p != "radius"] == base
    sig = inspect.signature(E.pgd_trust)
    assert list(sig.parameters)[1:] == ["n_rounds", "radius0", "k", "cg_tol", "precond", "tol", "rtol", "radius_max", "radius_min"]
    assert (sig.parameters["k"].default, sig.parameters["cg_tol"].default, sig.parameters["radius_max"].default) == (50, 1e-8, None)
    G2 = V.module("Vch_control_2D.GD2_configured")
    sig = inspect.signature(G2.trust_refine)
    assert {"n_trust", "radius0", "on_device"} <= set(sig.parameters) and sig.parameters["on_device"].default is False
    sig = inspect.signature(G2.run_sweep)
    assert sig.parameters["n_trust"].default == 0 and sig.parameters["radius0"].default == 1.0
    assert sig.parameters["n_newton"].default == 0
