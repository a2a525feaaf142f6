"""CPU-only checks of the directional sparsity functionals of the 1D engine: the NumPy restatement
(tests/_group_prox_ref.py) against a brute-force optimality search and on the degenerate cases, and the public surface:
the three entry points are declared in include/vch.h, exported by the built library and bound in _lib.SIGNATURES with as
many ctypes arguments as the header declares parameters; Engine1D and GD_1D carry the Python side.  No compute calls."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest

import _group_prox_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vch1d_pgd_init_g", "vch1d_grad_prox_g", "vch1d_cost_g")
BOXES = ((-1.0, 1.0), (-0.3, 2.0), (0.0, 1.0), (-1.0, 0.0), (-np.inf, np.inf))


def _random_group(rng):
    n = int(rng.integers(2, 12))
    w = rng.uniform(0.2, 1.5, n)
    if rng.random() < 0.4:
        w[int(rng.integers(n))] = 0.0                       # a node of zero inner weight
    lo, hi = BOXES[int(rng.integers(len(BOXES)))]
    v = rng.standard_normal(n) * 10.0 ** rng.uniform(-1, 0.7)
    lam = G.wnorm(v, w) * rng.uniform(0.05, 1.3)
    return v, w, lam, lo, hi


def test_restatement_against_brute_force_on_300_random_groups():
    """No feasible perturbation of the formula's u+ lowers 1/2 ||z - v||_w^2 + lam ||z||_w by more than rounding: 300
    groups over every box, weights that include a zero, and all three kinds of group."""
    rng = np.random.default_rng(7)
    kinds = {"zero": 0, "closed": 0, "box": 0}
    for _ in range(300):
        v, w, lam, lo, hi = _random_group(rng)
        u, s, kind = G.group_prox(v, w, lam, lo, hi)
        kinds[kind] += 1
        assert 0.0 <= s < 1.0 and np.all(u >= lo) and np.all(u <= hi)
        gain, f0 = G.brute_force_improvement(v, w, lam, lo, hi, u, rng)
        assert gain <= 1e-13 * max(f0, 1.0), (kind, gain, f0, lo, hi)
    assert min(kinds.values()) >= 20, kinds


def test_box_root_solves_its_equation():
    rng = np.random.default_rng(8)
    seen = 0
    while seen < 50:
        v, w, lam, lo, hi = _random_group(rng)
        u, s, kind = G.group_prox(v, w, lam, lo, hi)
        if kind != "box":
            continue
        seen += 1
        rho = G.wnorm(u, w)
        assert abs(rho * (1.0 - s) - lam * s) <= 8 * np.finfo(float).eps * (rho + lam)
        assert np.array_equal(u, np.clip(s * v, lo, hi))


def test_side_by_side_bisection_is_the_scalar_one():
    rng = np.random.default_rng(9)
    for lo, hi in BOXES:
        w = rng.uniform(0.2, 1.5, 9)
        w[2] = 0.0
        V = rng.standard_normal((40, 9)) * 10.0 ** rng.uniform(-1.5, 0.7, (40, 1))
        U, s, kinds = G.group_prox_many(V, w, 0.4, lo, hi)
        for g in range(40):
            u1, s1, k1 = G.group_prox(V[g], w, 0.4, lo, hi)
            assert k1 == kinds[g] and abs(s1 - s[g]) <= 4e-16 and np.max(np.abs(u1 - U[g])) <= 1e-15 * np.max(np.abs(V[g]))


def test_degenerate_cases():
    w = np.array([0.5, 1.0, 1.0, 0.5])
    v = np.array([0.3, -0.2, 0.1, 0.4])
    # c <= lam: the whole group vanishes, also at equality
    c = G.wnorm(v, w)
    for lam in (c, 2 * c):
        u, s, kind = G.group_prox(v, w, lam, -1.0, 1.0)
        assert kind == "zero" and s == 0.0 and not u.any()
    # infinite box: the closed form, exactly s0 v
    u, s, kind = G.group_prox(v, w, 0.25 * c, -np.inf, np.inf)
    assert kind == "closed" and s == 1.0 - 0.25 * c / c and np.array_equal(u, s * v)
    # u_min = 0: the negative entries do not count towards c, and a group with nothing positive vanishes for every lam
    u, s, kind = G.group_prox(-np.abs(v), w, 1e-9, 0.0, 1.0)
    assert kind == "zero" and not u.any()
    cpos = G.wnorm(np.maximum(v, 0.0), w)
    assert G.group_prox(v, w, 1.01 * cpos, 0.0, 1.0)[2] == "zero" and 1.01 * cpos < c
    u, s, kind = G.group_prox(v, w, 0.5 * cpos, 0.0, 1.0)
    assert kind == "box" and u[1] == 0.0 and np.all(u >= 0.0)
    # a zero weight: the node does not enter any norm and is scaled and clipped like the others
    w0 = np.array([0.0, 1.0, 1.0, 0.5])
    v0 = np.array([50.0, -0.2, 0.1, 0.4])
    u, s, kind = G.group_prox(v0, w0, 0.1, -1.0, 1.0)
    assert kind == "box" and u[0] == 1.0
    assert abs(s - (1.0 - 0.1 / G.wnorm(v0[1:], w0[1:]))) < 1e-15        # the rest of the group is inside the box
    # lam = 0 is the projection
    u, s, kind = G.group_prox(3 * v, w, 0.0, -1.0, 1.0)
    assert np.array_equal(u, np.clip(3 * v, -1.0, 1.0))


def test_modes_costs_and_kkt_of_the_restatement():
    rng = np.random.default_rng(3)
    x = np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, 6)])
    t = np.r_[0.0, np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, 4)])]       # t = 0 twice: wt[0] = 0
    u, r = rng.standard_normal((6, 7)), rng.standard_normal((6, 7))
    trapz = getattr(np, "trapezoid", None) or np.trapz
    assert G.trapz_w(t)[0] == 0.0
    assert np.isclose(G.j4(u, x, t, 0.3, "time"), 0.3 * trapz(np.sqrt(trapz(u * u, x=x, axis=1)), x=t), rtol=1e-14)
    assert np.isclose(G.j4(u, x, t, 0.3, "space"), 0.3 * trapz(np.sqrt(trapz(u * u, x=t, axis=0)), x=x), rtol=1e-14)
    for mode, ng in (("time", 6), ("space", 7)):
        up, s, kinds = G.prox(u, r, 0.5, 0.1, 1.2, -1.0, 1.0, mode, x, t)
        assert s.shape == (ng,) and len(kinds) == ng and up.shape == u.shape
        cnt, stat = G.kkt(up, r, x, t, 0.1, 1.2, -1.0, 1.0, mode)
        assert cnt[3] == ng and cnt[0] == kinds.count("zero") and stat >= 0.0
    # a group of the prox image is zero exactly when ||v_g|| <= lam (open box)
    up, s, kinds = G.prox(u, r, 0.5, 0.0, 1.2, -np.inf, np.inf, "time", x, t)
    vn = G.group_norms(u - 0.5 * r, x, t, "time")
    assert [k == "zero" for k in kinds] == list(vn <= 0.6)


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
    base, g = _declared_params("vch1d_pgd_init_v"), _declared_params("vch1d_pgd_init_g")
    assert g[:len(base) - 1] == base[:-1] and g[-1] == base[-1] == "double *J0_out"
    assert g[len(base) - 1:-1] == ["const int32_t *sparsity", "int n_sparsity"]
    base, g = _declared_params("vch1d_cost"), _declared_params("vch1d_cost_g")
    assert g == base[:-1] + ["int sparsity"] + base[-1:]
    g = _declared_params("vch1d_grad_prox_g")
    assert [p.split()[-1].lstrip("*") for p in g] == ["ctx", "u", "r", "rows", "x", "t_hist", "alpha", "opt", "sparsity", "u_out",
                                                       "scale_out"]
    src = _header()[0]
    for k, name in enumerate(("FULL", "TIME", "SPACE")):
        assert re.search(rf"#define\s+VCH_SPARSITY_{name}\s+{k}\b", src)


def test_python_surface_defaults_mean_todays_behaviour(V):
    E = V.Engine1D
    assert E.SPARSITY == ("full", "time", "space")
    p = inspect.signature(E.pgd_init).parameters
    assert list(p)[-1] == "sparsity" and p["sparsity"].default is None
    p = inspect.signature(E.grad_prox).parameters
    assert list(p)[1:5] == ["u", "r", "alpha", "opt"]
    assert (p["sparsity"].default, p["x"].default, p["t_hist"].default, p["return_scale"].default) == ("full", None, None, False)
    p = inspect.signature(E.cost).parameters
    assert list(p)[1:8] == ["phi_hist", "u", "phi_Q", "phi_T", "x", "t_hist", "opt"] and p["sparsity"].default == "full"
    for word in ("time", "space", "rows", "columns"):
        assert word in E.pgd_kkt.__doc__
    G1 = V.module("Vch_control_1D.GD_1D")
    assert inspect.signature(G1.run_optimization).parameters["sparsity"].default == "full"
    assert inspect.signature(G1.run_optimization_resident).parameters["sparsity"].default == "full"
    assert inspect.signature(G1.run_sweep).parameters["sparsity"].default is None
    with pytest.raises(ValueError):
        E._mode("rows")
