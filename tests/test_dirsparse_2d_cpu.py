"""CPU-only checks of the directional sparsity functionals of the 2D engine: the public surface (the three
entry points are declared in include/vch.h, exported by the built library and bound in _lib.SIGNATURES with as many ctypes
arguments as the header declares parameters; Engine2D and GD2_configured carry the Python side), the 2D restatement
(tests/_group_prox_ref_2d.py) against a brute-force optimality search on product-weight planes and wt-weighted pencils, its
j4 and kkt on a hand-made control, and that the seeds of the GPU seam test keep every decision away from its threshold.
No compute calls."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest

import _group_prox_ref as G1
import _group_prox_ref_2d as G
import _dirsparse_2d_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vch2d_pgd_init_g", "vch2d_grad_prox_g", "vch2d_cost_g")
BOXES = K.BOXES


# ---- the public surface (fails without the feature) ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


def _header():
    src = open(os.path.join(ROOT, "include", "vch.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declared_params(name):
    """The parameters of `name` as include/vch.h declares them, comments removed."""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header()[1], flags=re.S)
    assert m, f"{name} is not declared in include/vch.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound_with_the_headers_argument_count(V, name):
    params = _declared_params(name)
    lib = ctypes.CDLL(V.LIB_PATH)
    assert hasattr(lib, name), f"{name} is not exported"
    sigs = import_module(V.PKG_NAME + "._lib").SIGNATURES
    assert name in sigs
    restype, argtypes = sigs[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params), (len(argtypes), params)


def test_the_new_entry_points_extend_the_old_ones():
    base, g = _declared_params("vch2d_pgd_init_v"), _declared_params("vch2d_pgd_init_g")
    assert g[:len(base) - 1] == base[:-1] and g[-1] == base[-1] == "double *J0_out"
    assert g[len(base) - 1:-1] == ["const int32_t *sparsity", "int n_sparsity"]
    base, g = _declared_params("vch2d_cost"), _declared_params("vch2d_cost_g")
    assert g == base[:-1] + ["int sparsity"] + base[-1:]
    g = _declared_params("vch2d_grad_prox_g")
    assert [p.split()[-1].lstrip("*") for p in g] == ["ctx", "u", "r", "rows", "x", "y", "t_hist", "alpha", "opt", "sparsity",
                                                       "u_out", "scale_out"]
    assert re.search(r"int\s+vch_abi_version", _header()[1])


def test_python_surface_defaults_mean_todays_behaviour(V):
    E = V.Engine2D
    assert E.SPARSITY == ("full", "time", "space") == V.Engine1D.SPARSITY
    p = inspect.signature(E.pgd_init).parameters
    assert list(p)[-1] == "sparsity" and p["sparsity"].default is None
    assert list(p)[1:12] == ["phi0", "phi_T", "t_hist", "opt", "phi_Q", "ramp", "T", "x", "y", "u0", "alpha0"]
    p = inspect.signature(E.grad_prox).parameters
    assert list(p)[1:5] == ["u", "r", "alpha", "opt"]
    assert [p[k].default for k in ("sparsity", "x", "y", "t_hist", "return_scale")] == ["full", None, None, None, False]
    p = inspect.signature(E.cost).parameters
    assert list(p)[1:9] == ["phi_hist", "u", "phi_Q", "phi_T", "t_hist", "opt", "x", "y"] and p["sparsity"].default == "full"
    assert list(inspect.signature(E.pgd_kkt).parameters) == ["self", "refresh", "tol"]
    for word in ("time", "space", "levels", "pencils"):
        assert word in E.pgd_kkt.__doc__
    G2 = V.module("Vch_control_2D.GD2_configured")
    assert inspect.signature(G2.run_optimization).parameters["sparsity"].default is None
    assert inspect.signature(G2.run_sweep).parameters["sparsity"].default is None
    with pytest.raises(ValueError):
        E._mode("rows")


# ---- the restatement -----------------------------------------------------------------------------------------------------
def _grids(rng, nx1, ny1, rows):
    mk = lambda n: np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, n - 1)])
    return mk(nx1), mk(ny1), mk(rows)


@pytest.mark.parametrize("mode", ["time", "space"])
def test_restatement_against_brute_force(mode):
    """No feasible perturbation of a group's u+ lowers 1/2 ||z - v||_w^2 + lam ||z||_w by more than rounding, the groups
    being the levels under the product weights W_ij = wx_i wy_j or the pencils under wt, with the five boxes of the 1D
    tests; every kind of group occurs."""
    rng = np.random.default_rng(21 + (mode == "space"))
    nx1, ny1, rows = 4, 3, 5
    kinds = {"zero": 0, "closed": 0, "box": 0}
    for lo, hi in BOXES:
        for _ in range(6):
            x, y, t = _grids(rng, nx1, ny1, rows)
            ng = rows if mode == "time" else nx1 * ny1
            amp = 10.0 ** rng.uniform(-1.5, 0.7, ng)
            amp = amp[:, None, None] if mode == "time" else amp.reshape(1, nx1, ny1)
            u = amp * rng.standard_normal((rows, nx1, ny1))
            r = 0.1 * rng.standard_normal(u.shape)
            alpha, b3 = 0.5, 0.1
            w = G.weights(mode, x, y, t)
            ks = float(np.median(G.group_norms(u, x, y, t, mode))) / alpha
            up, s, kd = G.prox(u, r, alpha, b3, ks, lo, hi, mode, x, y, t)
            assert s.shape == ((rows,) if mode == "time" else (nx1, ny1))
            assert np.all(up >= lo) and np.all(up <= hi) and np.all((s >= 0) & (s < 1))
            v = u - alpha * (r + b3 * u)
            for vg, ug, kind in zip(G.groups(v, mode), G.groups(up, mode), kd):
                kinds[kind] += 1
                gain, f0 = G1.brute_force_improvement(vg, w, alpha * ks, lo, hi, ug, rng, tries=60)
                assert gain <= 1e-13 * max(f0, 1.0), (mode, kind, gain, f0, lo, hi)
    assert min(kinds.values()) >= 10, kinds


def test_groups_and_weights_are_the_planes_and_the_pencils():
    rng = np.random.default_rng(3)
    x, y, t = _grids(rng, 3, 4, 5)
    a = rng.standard_normal((5, 3, 4))
    wx, wy, wt = G.trapz_w(x), G.trapz_w(y), G.trapz_w(t)
    nt = G.group_norms(a, x, y, t, "time")
    ns = G.group_norms(a, x, y, t, "space")
    for k in range(5):
        assert np.isclose(nt[k], np.sqrt(sum(wx[i] * wy[j] * a[k, i, j] ** 2 for i in range(3) for j in range(4))), rtol=1e-14)
    for i in range(3):
        for j in range(4):
            assert np.isclose(ns[i, j], np.sqrt(sum(wt[k] * a[k, i, j] ** 2 for k in range(5))), rtol=1e-14)
    for mode in ("time", "space"):
        assert np.array_equal(G.ungroup(G.groups(a, mode), a.shape, mode), a)


def test_j4_and_kkt_on_a_hand_made_control():
    """u = 2 on level 1 alone (time) / on the pencil (1, 0) alone (space) of a 3 x 3 x 2 control on unit grids."""
    x, y, t = np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0]), np.array([0.0, 1.0, 3.0])
    wx, wy, wt = np.array([0.5, 1.0, 0.5]), np.array([0.5, 0.5]), np.array([0.5, 1.5, 1.0])
    assert np.array_equal(G.trapz_w(x), wx) and np.array_equal(G.trapz_w(t), wt)
    u = np.zeros((3, 3, 2))
    u[1] = 2.0
    # ||u_1||_W = 2 sqrt(sum W) = 2 sqrt(2); J4 = ks wt_1 ||u_1||
    assert np.isclose(G.j4(u, x, y, t, 0.3, "time"), 0.3 * 1.5 * 2.0 * np.sqrt(2.0), rtol=1e-15)
    # every pencil has norm 2 sqrt(wt_1); J4 = ks sum W * that
    assert np.isclose(G.j4(u, x, y, t, 0.3, "space"), 0.3 * 2.0 * 2.0 * np.sqrt(1.5), rtol=1e-15)
    r = np.zeros_like(u)
    r[1] = -1.0                                   # ||r_1||_W = sqrt(2), the other levels 0
    cnt, stat = G.kkt(u, r, x, y, t, 0.0, 1.0, -5.0, 5.0, "time")
    assert cnt.tolist() == [2, 2, 3, 3]          # levels 0, 2: zero and small; level 1: neither
    # prox_1: v = u - r = 3 on level 1, s = 1 - 1 / (3 sqrt 2)
    s = 1.0 - 1.0 / (3.0 * np.sqrt(2.0))
    assert np.isclose(stat, abs(3.0 * s - 2.0) / (2.0 + 1e-9 / np.sqrt(6.0)), rtol=1e-9)
    cnt, _ = G.kkt(u, r, x, y, t, 0.0, 2.0, -5.0, 5.0, "time")
    assert cnt.tolist() == [2, 3, 2, 3]          # ks = 2 > sqrt 2: level 1 is small but not zero
    u = np.zeros((3, 3, 2))
    u[:, 1, 0] = 2.0
    r = np.zeros_like(u)
    r[:, 1, 0] = -1.0                             # ||r_g|| = sqrt(sum wt) = sqrt 3
    assert np.isclose(G.j4(u, x, y, t, 0.3, "space"), 0.3 * (1.0 * 0.5) * 2.0 * np.sqrt(3.0), rtol=1e-15)
    cnt, _ = G.kkt(u, r, x, y, t, 0.0, 1.0, -5.0, 5.0, "space")
    assert cnt.tolist() == [5, 5, 6, 6]
    cnt, _ = G.kkt(u, r, x, y, t, 0.0, 1.8, -5.0, 5.0, "space")
    assert cnt.tolist() == [5, 6, 5, 6]


def test_loop_of_the_restatement_is_the_oracles_in_full_mode():
    """With mode "full" the 2D loop of the restatement is oracle.pgd: the same costs and control after two iterations."""
    from oracle import vch2d_oracle as O2
    P = O2.Params2D(Nx=8, Ny=8, T=0.03, dt_initial=1e-2)
    Op = O2.OptParams()
    ref = O2.pgd(P, Op, n_iter=2)
    mine = G.pgd(O2, P, Op, "full", 2)
    assert np.array_equal(np.array(ref.costs), np.array(mine["costs"]))
    assert np.array_equal(ref.u, mine["u"]) and list(ref.attempts) == mine["attempts"]


@pytest.mark.parametrize("mode", ["time", "space"])
@pytest.mark.parametrize("shape", K.SHAPES)
def test_seam_cases_keep_every_decision_1e9_from_its_threshold(mode, shape):
    """The inputs of the GPU seam test (tests/_dirsparse_2d_cases.py), checked here in long double on the restatement
    alone: every group's c / lam and every live group's max|s0 v| / bound is at least 1e-9 (relative) from 1, and every
    call has zero, closed-form and (finite box) box-active groups."""
    Nx, Ny = shape
    for rows in K.ROWS:
        for lo, hi in BOXES:
            case = K.seam_case(mode, Nx, Ny, rows, lo, hi)
            m_c, m_b = K.decision_margins(case)
            assert m_c >= 1e-9 and m_b >= 1e-9, (mode, shape, rows, lo, hi, m_c, m_b)
            kinds = set()
            for b in range(K.BATCH):
                kinds |= set(G.prox(case["u"][b], case["r"][b], case["alpha"], 0.0, case["ks"], lo, hi, mode, case["x"],
                                    case["y"], case["t"])[2])
            assert kinds == ({"zero", "closed"} if np.isinf(hi) else {"zero", "closed", "box"}), (mode, shape, rows, lo, hi)
