"""Plain NumPy restatement, in np.longdouble, of the three by-products every accepted iteration of the PGD loops reports
next to cost / alpha / attempts: the relative control change (the input of the stop rule) and the relative tracking /
terminal errors (oracle/vch2d_oracle.py::pgd, ::error_metrics and their 1D twins).  It takes fields pulled from the
engine (pgd_get) or made by the oracle and returns doubles; nothing here is shared with the code under test.
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def _ld(a):
    return np.asarray(a, dtype=LD)


def _trapz(f, x, axis=-1):
    """np.trapz arithmetic along `axis` on the grid x, in long double."""
    f = np.moveaxis(_ld(f), axis, -1)
    d = np.diff(_ld(x))
    return np.sum(d * (f[..., 1:] + f[..., :-1]) / LD(2.0), axis=-1)


def change(u_new, u_old):
    """||u_new - u_old||_F / (||u_old||_F + 1e-9) over the grid nodes of one trajectory."""
    un, uo = _ld(u_new), _ld(u_old)
    return float(np.sqrt(np.sum((un - uo) ** 2)) / (np.sqrt(np.sum(uo ** 2)) + LD(1e-9)))


def _ratios(numQ2, denQ2, numT2, denT2, extent, tl):
    zero = LD(0.0)
    rms = np.sqrt(max(LD(extent), LD(1e-30)) * max(LD(tl), LD(1e-30)))
    den = np.sqrt(max(denQ2, zero))
    fallback = bool(den < LD(1e-9) * rms)
    used = rms if fallback else den
    track = np.sqrt(max(numQ2, zero)) / (used + LD(1e-12))
    term = np.sqrt(max(numT2, zero)) / (np.sqrt(max(denT2, zero)) + LD(1e-12))
    return dict(track=float(track), term=float(term), den=float(den), rms=float(rms), fallback=fallback,
                den_T=float(np.sqrt(max(denT2, zero))))


def errors_2d_parts(phi, phi_Q, phi_T, x, y, t):
    """error_metrics of the 2D oracle with what decided it: dict(track, term, den = ||phi_Q||_L2(Q), rms = sqrt(|Omega| T),
    fallback = den < 1e-9 rms, den_T = ||phi_T||_L2(Omega)).  Histories (M+1, Nx+1, Ny+1), phi_T (Nx+1, Ny+1)."""
    l2xy2 = lambda a: _trapz(_trapz(_ld(a) ** 2, y, -1), x, -1)           # per level: trapezoid in y, then in x
    l2xyt2 = lambda a: _trapz(l2xy2(a), t)
    x, y, t = _ld(x), _ld(y), _ld(t)
    return _ratios(l2xyt2(_ld(phi) - _ld(phi_Q)), l2xyt2(phi_Q), l2xy2(_ld(phi)[-1] - _ld(phi_T)), l2xy2(phi_T),
                   (x[-1] - x[0]) * (y[-1] - y[0]), t[-1] - t[0])


def errors_2d(phi, phi_Q, phi_T, x, y, t):
    """(tracking, terminal) = O2.error_metrics(phi, phi_Q, phi_T, x, y, t)."""
    p = errors_2d_parts(phi, phi_Q, phi_T, x, y, t)
    return p["track"], p["term"]


def errors_1d_parts(phi, phi_Q, phi_T, x, t):
    """errors_2d_parts for the 1D oracle: histories (rows, N+1) with t = 0 twice, phi_T (N+1,)."""
    l2x2 = lambda a: _trapz(_ld(a) ** 2, x, -1)
    l2xt2 = lambda a: _trapz(l2x2(a), t)
    x, t = _ld(x), _ld(t)
    return _ratios(l2xt2(_ld(phi) - _ld(phi_Q)), l2xt2(phi_Q), l2x2(_ld(phi)[-1] - _ld(phi_T)), l2x2(phi_T),
                   x[-1] - x[0], t[-1] - t[0])


def errors_1d(phi, phi_Q, phi_T, x, t):
    """(tracking, terminal) = O1.error_metrics(phi, phi_Q, phi_T, x, t)."""
    p = errors_1d_parts(phi, phi_Q, phi_T, x, t)
    return p["track"], p["term"]


def gap(got, ref):
    """|got - ref| / |ref|, 0.0 where both are exactly zero (zero is compared exactly: inf where only one is)."""
    got, ref = float(got), float(ref)
    if ref == 0.0 or got == 0.0:
        return 0.0 if got == ref else float("inf")
    return abs(got - ref) / abs(ref)
