"""Builders of group-prox inputs at the decisions of the directional sparsity prox, shared by the 1D
and the 2D edge tests.  Each `build_*` takes a generator, the number of groups, their length, the weight vector of the
group norm, the threshold lam and the box, and returns the (G, m) block v of gradient steps; nothing here knows whether a
group is a row, a column, a plane or a pencil.  `_margins` measures, in long double, what a block keeps of the distances
it was built with."""
import numpy as np

import _group_prox_ref as G

LD = np.longdouble
DELTAS = np.array([1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3])
MARGIN = 5e-10                                      # what the inputs keep of the 1e-9 they are built with, checked in long double


def _ldnorm(Z, w):
    return np.sqrt(np.sum(w.astype(LD) * Z.astype(LD) ** 2, axis=-1))


def _right_sign(lo, hi):
    return 1.0 if lo == 0.0 else (-1.0 if hi == 0.0 else 0.0)


def build_alive(rng, ng, m, w, lam, lo, hi):
    """Groups with ||cone(v)|| = lam (1 + d), d = +-1e-9, +-1e-6, +-1e-3 in turn.  On a one-sided box the right-signed part
    carries that norm and about half the entries are wrong-signed and 400 times larger: a group that is barely alive then
    has s0 close to 1, its root at s = 1 - lam / c = d and the whole of [0, 1] to cross."""
    d = DELTAS[(np.arange(ng) + rng.integers(6)) % 6]
    z = rng.standard_normal((ng, m))
    sg = _right_sign(lo, hi)
    if sg:
        right = rng.random((ng, m)) < 0.5
        right[:, 1] = True                          # one right-signed entry of positive weight at least
        z = np.where(right, sg * np.abs(z), -sg * 400.0 * np.abs(z))
    return z * (lam * (1.0 + d.astype(LD)) / _ldnorm(G.cone(z, lo, hi), w)).astype(np.float64)[:, None]


def build_edge(rng, ng, m, w, lam, lo, hi):
    """Groups whose largest |s0 v| sits at (1 -+ 1e-9) or (1 -+ 1e-6) of a finite bound, so that the vote closed form /
    iteration is decided: v = c z with c = target / max|z| + lam / ||z||, which makes s0 c max|z| = target.  The entries
    towards the other bound are 20 times smaller (none on a one-sided box, where any would decide the vote)."""
    sides = [s for s, bound in ((1.0, hi), (-1.0, lo)) if np.isfinite(bound) and bound != 0.0]
    side = np.array(sides)[np.arange(ng) % len(sides)]
    bound = np.where(side > 0, hi, -lo)
    d = np.array([-1e-9, 1e-9, -1e-6, 1e-6])[(np.arange(ng) // 2 + rng.integers(4)) % 4]
    z = np.abs(rng.standard_normal((ng, m))) + 0.1
    if not _right_sign(lo, hi):
        z = np.where(rng.random((ng, m)) < 0.3, -0.05 * z, z)
    z *= side[:, None]
    c = bound * (1.0 + d.astype(LD)) / np.max(np.abs(z), axis=1) + lam / _ldnorm(z, w)
    return z * c.astype(np.float64)[:, None]


def build_mixed(rng, ng, m, w, lam, lo, hi):
    """Amplitude 3 (box-active where the box is finite) and 0.05 (inactive; one-signed where the box is one-sided) in turn."""
    big = (np.arange(ng) + rng.integers(2)) % 2 == 0
    z = rng.standard_normal((ng, m))
    sg = _right_sign(lo, hi)
    if sg:
        z = np.where(big[:, None], z, sg * np.abs(z))
    return z * np.where(big, 3.0, 0.05)[:, None]


def build_lam0(rng, ng, m, w, lam, lo, hi):
    """build_mixed with group 0 all zero and every other group holding a right-signed entry of positive weight."""
    v = build_mixed(rng, ng, m, w, lam, lo, hi)
    sg = _right_sign(lo, hi)
    v[:, 1] = sg * np.abs(v[:, 1]) if sg else v[:, 1]
    v[0] = 0.0
    return v


def build_zero_weight(rng, ng, m, w, lam, lo, hi):
    """Entries of size 50 on the nodes of weight zero, next to a rest of amplitude 0.001 (the group vanishes whatever stands
    on the weightless node), 0.05 or 3."""
    amp = np.array([0.001, 0.05, 3.0])[(np.arange(ng) + rng.integers(3)) % 3]
    v = rng.standard_normal((ng, m)) * amp[:, None]
    sg = _right_sign(lo, hi)
    if sg:
        v = np.where((amp == 0.05)[:, None], sg * np.abs(v), v)
    light = w == 0.0
    assert light.any()
    v[:, light] = 50.0 * (sg if sg else 1.0) * np.where(rng.random((ng, int(light.sum()))) < 0.8, 1.0, -1.0)
    return v


def _margins(vg, w, lam, lo, hi):
    """In long double: c / lam - 1 of every group (inf at lam = 0), and for the groups with c > lam how far the largest
    s0 v / bound is from 1 (inf where an entry is on the wrong side of a zero bound, -1 with an infinite box)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        c = _ldnorm(G.cone(vg, lo, hi), w)
        alive = np.where(lam > 0.0, c / LD(lam) - 1.0, np.where(c > 0.0, np.inf, -1.0))
        s0 = 1.0 - LD(lam) / _ldnorm(vg, w)
        sv = s0[:, None] * vg.astype(LD)
        ratio = np.full(vg.shape[0], LD(0.0))
        for bound, sign in ((hi, 1.0), (lo, -1.0)):
            if bound == 0.0:
                ratio = np.where(np.any(sign * sv > 0.0, axis=1), np.inf, ratio)
            elif np.isfinite(bound):
                ratio = np.maximum(ratio, np.max(sign * sv, axis=1) / abs(bound))
    return alive, (ratio - 1.0)[alive > 0.0]
