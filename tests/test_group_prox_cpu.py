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


def test_long_double_variant_of_the_side_by_side_bisection():
    """dtype=np.longdouble runs the same formulas on the same doubles in extended precision: it returns long doubles, agrees
    with the double variant on the kind and to a few ulps of a double on s, and is exact to its own precision where the
    answer is known in closed form."""
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18
    rng = np.random.default_rng(10)
    for lo, hi in BOXES:
        w = rng.uniform(0.2, 1.5, 9)
        w[2] = 0.0
        V = rng.standard_normal((40, 9)) * 10.0 ** rng.uniform(-1.5, 0.7, (40, 1))
        U, s, kinds = G.group_prox_many(V, w, 0.4, lo, hi)
        Ul, sl, kl = G.group_prox_many(V, w, 0.4, lo, hi, dtype=LD)
        assert Ul.dtype == LD and sl.dtype == LD and s.dtype == np.float64 and U.dtype == np.float64
        assert kinds == kl and np.max(np.abs(s - sl)) <= 1e-15 and np.max(np.abs(U - Ul)) <= 1e-15 * np.max(np.abs(V))
    # ||(3, 4)|| = 5, lam = 1: s = 4/5, which no double holds
    s = G.group_prox_many(np.array([[3.0, 4.0]]), np.ones(2), 1.0, -np.inf, np.inf, dtype=LD)[1]
    assert abs(s[0] - LD(4) / LD(5)) <= 2 * np.finfo(LD).eps
    # v = (3, 8) under u_max = 2: at s = 1/2 the second entry is cut, rho = ||(3/2, 2)|| = 5/2 and rho (1 - s) = lam s for lam = 5/2
    U, s, kinds = G.group_prox_many(np.array([[3.0, 8.0]]), np.ones(2), 2.5, -1.0, 2.0, dtype=LD)
    assert kinds == ["box"] and abs(s[0] - LD(0.5)) <= 2 * np.finfo(LD).eps and np.max(np.abs(U[0] - [1.5, 2.0])) <= 4 * np.finfo(LD).eps
    for mode in ("time", "space"):
        u, r = rng.standard_normal((2, 6, 7))
        x, t = np.linspace(0, 1, 7), np.r_[0.0, np.linspace(0, 1, 5)]
        a, b = G.prox(u, r, 0.5, 0.1, 1.2, -1.0, 1.0, mode, x, t), G.prox(u, r, 0.5, 0.1, 1.2, -1.0, 1.0, mode, x, t, dtype=LD)
        assert a[2] == b[2] and b[0].shape == u.shape and np.max(np.abs(a[1] - b[1])) <= 1e-15


def test_loop_of_the_restatement_from_a_warm_start():
    """pgd's u0, alpha0 and change: the defaults are the run from u = 0 with alpha_max; alpha0 is capped at alpha_max; a
    warm start is where the first step starts from; change[k] is ||u_{k+1} - u_k||_F / (||u_k||_F + 1e-9)."""
    from oracle import vch1d_oracle as O1
    P = O1.Params1D(N=16, T=0.03, dt_initial=1e-2)
    same = lambda a, b: a["costs"] == b["costs"] and a["trials"] == b["trials"] and a["change"] == b["change"] and np.array_equal(a["u"], b["u"])
    for mode, ks in (("time", 0.03), ("space", 0.005)):             # some groups of the first step vanish, some do not
        O = O1.OptParams1D(kappa_sparsity=ks, alpha_max=40.0, u_min=-0.3, u_max=0.5)
        base = G.pgd(O1, P, O, mode, 2)
        gn = G.group_norms(G.pgd(O1, P, O, mode, 1)["u"], base["x"], base["t_hist"], mode)[1:]
        assert 0 < np.count_nonzero(gn) < gn.size
        assert len(base["change"]) == 2 and base["u"].shape == (5, 17)
        assert same(base, G.pgd(O1, P, O, mode, 2, u0=np.zeros((5, 17)), alpha0=40.0))
        assert same(base, G.pgd(O1, P, O, mode, 2, alpha0=1e9))
        assert not same(base, G.pgd(O1, P, O, mode, 2, alpha0=5.0))
        one = G.pgd(O1, P, O, mode, 1)
        assert base["change"][0] == np.linalg.norm(one["u"]) / 1e-9                  # from u = 0: the quotient means nothing
        assert base["change"][1] == np.linalg.norm(base["u"] - one["u"]) / (np.linalg.norm(one["u"]) + 1e-9)
        # a warm start outside the box is taken as given: the loop continued from `one` is the loop of two iterations,
        # given the step size it would have had
        rng = np.random.default_rng(4)
        u0 = 0.6 * rng.standard_normal((5, 17))
        w1, w2 = G.pgd(O1, P, O, mode, 1, u0=u0, alpha0=3.0), G.pgd(O1, P, O, mode, 2, u0=u0, alpha0=3.0)
        assert w1["costs"][0] == w2["costs"][0] and w1["costs"][0] != base["costs"][0]
        assert w2["change"][0] == np.linalg.norm(w1["u"] - u0) / (np.linalg.norm(u0) + 1e-9) < 10.0
        a1 = min(O.alpha_max, 3.0 * 0.8 ** (w1["trials"][0] - 1 + (w1["costs"][1] >= w1["costs"][0])) * 1.2)
        cont = G.pgd(O1, P, O, mode, 1, u0=w1["u"], alpha0=a1)
        assert cont["trials"][0] == w2["trials"][1] and np.allclose(cont["u"], w2["u"], rtol=0, atol=1e-12)
        assert np.isclose(cont["change"][0], w2["change"][1], rtol=1e-10)


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
