"""Thin numpy-facing wrapper of the C ABI (include/vch.h): one object per GPU context.

No arithmetic happens here: every method marshals numpy buffers into one engine call.
Batched arguments have a leading axis B (the context's batch); with B == 1 the leading
axis may be omitted and is then omitted from the results as well.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import _lib
from ._lib import OptParams, Params1D, Params2D, Stats, VchError, check


def _dp(a):
    return None if a is None else a.ctypes.data_as(_lib._D)


def time_grid(T: float, dt: float, time_tol: float = 1e-10):
    """The reference's accumulated-time rule (Forward2_solver.py:539-585, Forward_solver.py:
    326-373): `t += min(dt, T - t)` while `t < T - 1e-10`, stored as `min(t, T)`.
    Returns (t_hist with a leading 0, per-step dt)."""
    t, ts, dts = 0.0, [0.0], []
    while t < T - time_tol:
        d = min(dt, T - t)
        dts.append(d)
        t += d
        ts.append(min(t, T))
    return np.array(ts), np.array(dts)


def make_opt(opt=None, **kw) -> OptParams:
    """OptParams from an object with the reference's OptimizationConfig field names."""
    names = [f for f, _ in OptParams._fields_]
    defaults = dict(b1=5.0, b2=10.0, b3=1e-4, kappa_sparsity=1e-4, alpha_max=50.0, max_iter=500,
                    u_min=-1.0, u_max=1.0)
    vals = dict(defaults)
    if opt is not None:
        for n in names:
            if hasattr(opt, n):
                vals[n] = getattr(opt, n)
    vals.update(kw)
    o = OptParams()
    for n in names:
        setattr(o, n, int(vals[n]) if n == "max_iter" else float(vals[n]))
    return o


class Engine2D:
    """One GPU context for `batch` trajectories on an (Nx+1) x (Ny+1) grid."""

    def __init__(self, Nx, Ny, Lx=1.0, Ly=1.0, tau=0.05, gamma=10.0, c1=0.75, c2=1.0, kappa=1e-4,
                 batch=1, max_steps=128, device=0):
        self.lib = _lib.load()
        n = self.lib.vch_device_count()
        if n <= 0:
            raise VchError("no HIP device visible: the engine has no CPU path")
        self.p = Params2D(int(Nx), int(Ny), float(Lx), float(Ly), float(tau), float(gamma), float(c1),
                          float(c2), float(kappa))
        self.B, self.max_steps, self.device = int(batch), int(max_steps), int(device)
        self.Nx, self.Ny = int(Nx), int(Ny)
        self.shape = (self.Nx + 1, self.Ny + 1)
        self.ctx = self.lib.vch2d_create(C.byref(self.p), self.B, self.max_steps, self.device)
        if not self.ctx:
            raise ValueError("vch2d_create failed: " + _lib.last_error())
        self.uses_fft = bool(self.lib.vch2d_uses_fft(self.ctx))
        self.x = np.linspace(0.0, float(Lx), self.Nx + 1)
        self.y = np.linspace(0.0, float(Ly), self.Ny + 1)

    @classmethod
    def from_config(cls, cfg, **kw):
        return cls(cfg.Nx, cfg.Ny, cfg.Lx, cfg.Ly, cfg.tau, cfg.gamma, cfg.c1, cfg.c2, cfg.kappa, **kw)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.vch2d_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- marshalling ----------------------------------------------------------------
    def _fld(self, a, name="field"):
        """(B, Nx+1, Ny+1) float64 C-contiguous view/copy; ValueError on a wrong shape
        (Forward2_solver.py:148-149)."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape == self.shape and self.B == 1:
            a = a.reshape((1,) + self.shape)
        if a.shape != (self.B,) + self.shape:
            raise ValueError(f"{name} must have shape ({self.Nx + 1}, {self.Ny + 1}) "
                             f"[batch {self.B}], got {a.shape}")
        return a

    def _hist(self, a, rows, name="history"):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim == 3 and self.B == 1:
            a = a.reshape((1,) + a.shape)
        if a.ndim != 4 or a.shape[0] != self.B or a.shape[2:] != self.shape or (rows and a.shape[1] != rows):
            raise ValueError(f"{name} must have shape (M, {self.Nx + 1}, {self.Ny + 1}), got {a.shape}")
        return a

    def _out(self, squeeze=True, rows=None):
        shp = (self.B,) + ((rows,) if rows else ()) + self.shape
        return np.empty(shp, dtype=np.float64)

    def _sq(self, a):
        return a[0] if self.B == 1 else a

    # -- operators --------------------------------------------------------------------
    def apply_laplacian(self, v):
        v = self._fld(v)
        out = self._out()
        check(self.lib.vch2d_apply_laplacian(self.ctx, _dp(v), _dp(out)))
        return self._sq(out)

    def initialize_mu(self, phi, w):
        phi, w = self._fld(phi), self._fld(w)
        out = self._out()
        check(self.lib.vch2d_initialize_mu(self.ctx, _dp(phi), _dp(w), _dp(out)))
        return self._sq(out)

    def solve_w(self, w_old, dt, u_n=None, u_np1=None):
        w_old = self._fld(w_old)
        u_n = None if u_n is None else self._fld(u_n)
        u_np1 = None if u_np1 is None else self._fld(u_np1)
        out = self._out()
        check(self.lib.vch2d_solve_w(self.ctx, _dp(w_old), float(dt), _dp(u_n), _dp(u_np1), _dp(out)))
        return self._sq(out)

    def residuals(self, phi_new, phi_old, mu_new, mu_old, w_new, w_old, dt):
        a = [self._fld(v) for v in (phi_new, phi_old, mu_new, mu_old, w_new, w_old)]
        Rp, Rm = self._out(), self._out()
        nrm = np.empty(self.B)
        check(self.lib.vch2d_residuals(self.ctx, *[_dp(v) for v in a], float(dt), _dp(Rp), _dp(Rm), _dp(nrm)))
        return self._sq(Rp), self._sq(Rm), (nrm[0] if self.B == 1 else nrm)

    def jacobian_apply(self, phi_new, dt, dphi, dmu):
        a = [self._fld(v) for v in (phi_new, dphi, dmu)]
        o1, o2 = self._out(), self._out()
        check(self.lib.vch2d_jacobian_apply(self.ctx, _dp(a[0]), float(dt), _dp(a[1]), _dp(a[2]), _dp(o1), _dp(o2)))
        return self._sq(o1), self._sq(o2)

    def jacobian_solve(self, phi_new, dt, rhs_phi, rhs_mu):
        a = [self._fld(v) for v in (phi_new, rhs_phi, rhs_mu)]
        o1, o2 = self._out(), self._out()
        st = Stats()
        check(self.lib.vch2d_jacobian_solve(self.ctx, _dp(a[0]), float(dt), _dp(a[1]), _dp(a[2]), _dp(o1), _dp(o2),
                                            C.byref(st)))
        return self._sq(o1), self._sq(o2), st.as_dict()

    def schur_apply(self, phi_new, dt, x):
        a = [self._fld(v) for v in (phi_new, x)]
        out = self._out()
        check(self.lib.vch2d_schur_apply(self.ctx, _dp(a[0]), float(dt), _dp(a[1]), _dp(out)))
        return self._sq(out)

    def adjoint_apply(self, which, phi, dt, v):
        a = [self._fld(z) for z in (phi, v)]
        out = self._out()
        check(self.lib.vch2d_adjoint_apply(self.ctx, {"A": 0, "B": 1}[which], _dp(a[0]), float(dt), _dp(a[1]), _dp(out)))
        return self._sq(out)

    def adjoint_solve(self, phi_n, dt, rhs):
        phi_n = None if phi_n is None else self._fld(phi_n)
        rhs = self._fld(rhs)
        out = self._out()
        st = Stats()
        check(self.lib.vch2d_adjoint_solve(self.ctx, _dp(phi_n), float(dt), _dp(rhs), _dp(out), C.byref(st)))
        return self._sq(out), st.as_dict()

    def spectral_solve(self, c0, c1, c2, v):
        v = self._fld(v)
        out = self._out()
        check(self.lib.vch2d_spectral_solve(self.ctx, float(c0), float(c1), float(c2), _dp(v), _dp(out)))
        return self._sq(out)

    # -- Newton / march / sweep --------------------------------------------------------
    def newton_raphson(self, phi_old, mu_old, w_old, w_new, dt, hist_cap=512):
        a = [self._fld(v) for v in (phi_old, mu_old, w_old, w_new)]
        pn, mn = self._out(), self._out()
        hist = np.zeros((self.B, hist_cap))
        nh = np.zeros(self.B, dtype=np.int32)
        st = Stats()
        check(self.lib.vch2d_newton_raphson(self.ctx, *[_dp(v) for v in a], float(dt), _dp(pn), _dp(mn), _dp(hist),
                                            int(hist_cap), nh.ctypes.data_as(_lib._I32), C.byref(st)))
        hists = [hist[b, :nh[b]].copy() for b in range(self.B)]
        return self._sq(pn), self._sq(mn), (hists[0] if self.B == 1 else hists), st.as_dict()

    def forward(self, phi0, dt, u=None, store=True):
        """March len(dt) steps.  u: (B, rows, ...) control, None, or "resident".
        Returns (phi_hist or None, stats)."""
        phi0 = self._fld(phi0, "phi0")
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        M = int(dt.size)
        rows = 0
        if isinstance(u, str) and u == "resident":
            up = C.cast(C.c_void_p(1), _lib._D)
        elif u is None:
            up = None
        else:
            if u.ndim == 3 and self.B == 1:
                u = u.reshape((1,) + u.shape)
            if u.ndim != 4 or u.shape[0] != self.B or u.shape[2:] != self.shape:
                raise ValueError(f"control_input must have shape (M, {self.Nx + 1}, {self.Ny + 1})")
            u = np.ascontiguousarray(u, dtype=np.float64)
            rows = int(u.shape[1])
            up = _dp(u)
        out = self._out(rows=M + 1) if store else None
        st = Stats()
        check(self.lib.vch2d_forward(self.ctx, _dp(phi0), up, rows, _dp(dt), M, _dp(out), C.byref(st)))
        self._base = ("forward", M, rows if up is not None else 0)      # what hessvec's g_rows=None resolves against
        return (self._sq(out) if store else None), st.as_dict()

    def backward(self, phi_hist, t_hist, b1, b2, phi_Q=None, phi_T=None, hx=None, hy=None,
                 want=("p", "q", "r")):
        """Adjoint sweep; phi_hist None = resident history of the last forward call."""
        t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
        M = int(t_hist.size) - 1
        ph = None if phi_hist is None else self._hist(phi_hist, M + 1, "phi_hist")
        pq = None if phi_Q is None else self._hist(phi_Q, M + 1, "phi_Q")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        outs = {k: (self._out(rows=M + 1) if k in want else None) for k in ("p", "q", "r")}
        st = Stats()
        hx = float(self.x[1] - self.x[0]) if hx is None else float(hx)
        hy = float(self.y[1] - self.y[0]) if hy is None else float(hy)
        check(self.lib.vch2d_backward(self.ctx, _dp(ph), M, _dp(t_hist), hx, hy, float(b1), float(b2), _dp(pq),
                                      _dp(pt), _dp(outs["p"]), _dp(outs["q"]), _dp(outs["r"]), C.byref(st)))
        return tuple(None if outs[k] is None else self._sq(outs[k]) for k in ("p", "q", "r")) + (st.as_dict(),)

    # the sparsity functional: index = VCH_SPARSITY_* of include/vch.h
    SPARSITY = ("full", "time", "space")

    @classmethod
    def _mode(cls, sparsity):
        if sparsity not in cls.SPARSITY:
            raise ValueError(f"sparsity must be one of {cls.SPARSITY}, got {sparsity!r}")
        return cls.SPARSITY.index(sparsity)

    def cost(self, phi_hist, u, phi_Q, phi_T, t_hist, opt, x=None, y=None, sparsity="full"):
        """J (B, 5) = {J1, J2, J3, J4, J}.  `sparsity`: J4 = kappa_s int int |u| ("full"), kappa_s int ||u(., t)||_L2(Omega) dt
        ("time") or kappa_s int_Omega ||u(x, .)||_L2(0,T) dx ("space")."""
        mode = self._mode(sparsity)
        t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
        M = int(t_hist.size) - 1
        ph = None if phi_hist is None else self._hist(phi_hist, M + 1, "phi_hist")
        uu = None if u is None else self._hist(u, M + 1, "u")
        pq = None if phi_Q is None else self._hist(phi_Q, M + 1, "phi_Q_target")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        x = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
        y = np.ascontiguousarray(self.y if y is None else y, dtype=np.float64)
        if x.shape != (self.Nx + 1,) or y.shape != (self.Ny + 1,):
            raise ValueError("x, y must have Nx+1, Ny+1 entries")
        J = np.empty((self.B, 5))
        o = opt if isinstance(opt, OptParams) else make_opt(opt)
        if mode == 0:
            check(self.lib.vch2d_cost(self.ctx, _dp(ph), _dp(uu), _dp(pq), _dp(pt), M, _dp(x), _dp(y), _dp(t_hist),
                                      C.byref(o), _dp(J)))
        else:
            check(self.lib.vch2d_cost_g(self.ctx, _dp(ph), _dp(uu), _dp(pq), _dp(pt), M, _dp(x), _dp(y), _dp(t_hist),
                                        C.byref(o), mode, _dp(J)))
        return J[0] if self.B == 1 else J

    def grad_prox(self, u, r, alpha, opt, sparsity="full", x=None, y=None, t_hist=None, return_scale=False):
        """prox of the sparsity term at u - alpha (r + b3 u) under the box of `opt`.  `sparsity` "time" / "space": the prox
        of the group norm over the levels (weights: product trapezoid in `x`, `y`, default the engine's grid) or the pencils
        u[:, i, j] (weights: trapezoid in `t_hist`, required) of the control; the box must contain 0.  return_scale=True:
        (u+, s) with s the factor of every group, (B, rows) or (B, Nx+1, Ny+1): u+ = clip(s v), 0 for a group that vanishes."""
        mode = self._mode(sparsity)
        u = self._hist(u, 0, "u")
        r = self._hist(r, u.shape[1], "r")
        rows = int(u.shape[1])
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (self.B,)))
        out = np.empty_like(u)
        o = opt if isinstance(opt, OptParams) else make_opt(opt)
        if mode == 0:
            if return_scale:
                raise ValueError('return_scale needs sparsity "time" or "space": the node-wise prox has no group factor')
            check(self.lib.vch2d_grad_prox(self.ctx, _dp(u), _dp(r), rows, _dp(al), C.byref(o), _dp(out)))
            return self._sq(out)
        xx = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
        yy = np.ascontiguousarray(self.y if y is None else y, dtype=np.float64)
        if mode == 2 and t_hist is None:
            raise ValueError('sparsity "space" needs t_hist: the weights of the pencil norm')
        tt = None if t_hist is None else np.ascontiguousarray(t_hist, dtype=np.float64)
        if xx.shape != (self.Nx + 1,) or yy.shape != (self.Ny + 1,) or (tt is not None and tt.shape != (rows,)):
            raise ValueError(f"x, y must have Nx+1, Ny+1 entries and t_hist {rows}")
        s = np.empty((self.B, rows) if mode == 1 else (self.B,) + self.shape)
        check(self.lib.vch2d_grad_prox_g(self.ctx, _dp(u), _dp(r), rows, _dp(xx), _dp(yy), _dp(tt), _dp(al), C.byref(o), mode,
                                         _dp(out), _dp(s)))
        return (self._sq(out), self._sq(s)) if return_scale else self._sq(out)

    # -- device-resident PGD -------------------------------------------------------------
    def pgd_init(self, phi0, phi_T, t_hist, opt, phi_Q=None, ramp=True, T=None, x=None, y=None, u0=None, alpha0=None,
                 sparsity=None):
        """Load the problem and evaluate J(u^0); returns J0 [B][5].  `opt`: one parameter object for the whole batch or
        a sequence of B (trajectory b runs with opt[b]: weights, sparsity parameter, box and alpha_max).  `u0` [B][M+1][..]:
        start control (taken as given, not clipped; default zeros).  `alpha0` [B] or a scalar: first step size, capped at
        each trajectory's alpha_max (default: alpha_max).  A single `opt` without u0 / alpha0 goes through vch2d_pgd_init.
        `sparsity`: a name of Engine2D.SPARSITY for the whole batch or a list of B names (vch2d_pgd_init_g: the prox, J4 and
        the KKT statistic of a "time" / "space" trajectory go by levels / pencils of the control; its box must contain 0);
        None takes the calls above exactly, every trajectory "full"."""
        phi0, phi_T = self._fld(phi0, "phi0"), self._fld(phi_T, "phi_T_target")
        t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
        M = int(t_hist.size) - 1
        pq = None if phi_Q is None else self._hist(phi_Q, M + 1, "phi_Q_target")
        x = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
        y = np.ascontiguousarray(self.y if y is None else y, dtype=np.float64)
        J0 = np.empty((self.B, 5))
        Tq = float(t_hist[-1] if T is None else T)
        many = isinstance(opt, (list, tuple))
        if sparsity is None and not many and u0 is None and alpha0 is None:
            o = opt if isinstance(opt, OptParams) else make_opt(opt)
            check(self.lib.vch2d_pgd_init(self.ctx, _dp(phi0), _dp(phi_T), _dp(pq), int(bool(ramp)), Tq, _dp(t_hist), M,
                                          _dp(x), _dp(y), C.byref(o), _dp(J0)))
        else:
            seq = list(opt) if many else [opt]
            arr = (OptParams * len(seq))(*[o if isinstance(o, OptParams) else make_opt(o) for o in seq])
            uu = None if u0 is None else self._hist(u0, M + 1, "u0")
            al = None if alpha0 is None else np.ascontiguousarray(
                np.broadcast_to(np.asarray(alpha0, dtype=np.float64), (self.B,)))
            if sparsity is None:
                check(self.lib.vch2d_pgd_init_v(self.ctx, _dp(phi0), _dp(phi_T), _dp(pq), int(bool(ramp)), Tq, _dp(t_hist), M,
                                                _dp(x), _dp(y), arr, len(seq), _dp(uu), _dp(al), _dp(J0)))
            else:
                names = [sparsity] if isinstance(sparsity, str) else list(sparsity)
                if len(names) not in (1, self.B):
                    raise ValueError(f"sparsity must be one name or {self.B}, got {len(names)}")
                modes = np.array([self._mode(s) for s in names], dtype=np.int32)
                check(self.lib.vch2d_pgd_init_g(self.ctx, _dp(phi0), _dp(phi_T), _dp(pq), int(bool(ramp)), Tq, _dp(t_hist), M,
                                                _dp(x), _dp(y), arr, len(seq), _dp(uu), _dp(al),
                                                modes.ctypes.data_as(_lib._I32), len(names), _dp(J0)))
        self._pgd_M = M
        self._base = ("pgd", M, M + 1)
        return J0

    def pgd_kkt(self, refresh=True, tol=1e-6):
        """KKT sparsity statistic `u* = 0 <=> |r*| <= kappa_sparsity` of the resident iterate, counted on the device.
        refresh=True recomputes the adjoint of the resident state first; refresh=False takes the resident r (the adjoint of
        the iterate before the last accepted step).  Returns dict(n_zero, n_small, n_match, total: int64 [B]; pct [B][3],
        the three percentages of verify_sparsity_condition; stationarity [B] = ||prox_1(u) - u|| / (||u|| + 1e-9)).
        What is counted depends on the trajectory's sparsity mode (pgd_init): "full" counts nodes; "time" counts the levels
        of the control and "space" its pencils, ||u_g|| < tol and ||r_g|| <= kappa_sparsity in the group's weighted norm,
        total = M+1 or (Nx+1)(Ny+1); prox_1 is the mode's prox at alpha = 1."""
        cnt = np.zeros((self.B, 4), dtype=np.int64)
        stat = np.empty(self.B)
        check(self.lib.vch2d_pgd_kkt(self.ctx, int(bool(refresh)), float(tol), cnt.ctypes.data_as(C.POINTER(C.c_int64)),
                                     _dp(stat)))
        return dict(n_zero=cnt[:, 0].copy(), n_small=cnt[:, 1].copy(), n_match=cnt[:, 2].copy(), total=cnt[:, 3].copy(),
                    pct=100.0 * cnt[:, :3] / cnt[:, 3:4], stationarity=stat)

    def pgd_iterate(self, n_iters):
        n = int(n_iters)
        cost = np.full((self.B, n), np.nan)
        alpha = np.full((self.B, n), np.nan)
        att = np.zeros((self.B, n), dtype=np.int32)
        chg = np.full((self.B, n), np.nan)
        sec = np.zeros(5)
        done = check(self.lib.vch2d_pgd_iterate(self.ctx, n, _dp(cost), _dp(alpha), att.ctypes.data_as(_lib._I32),
                                                _dp(chg), _dp(sec)))
        self._base = ("pgd", self._pgd_M, self._pgd_M + 1)
        trk, trm = np.full((self.B, n), np.nan), np.full((self.B, n), np.nan)
        check(self.lib.vch2d_pgd_errors(self.ctx, n, _dp(trk), _dp(trm)))
        return dict(iters=done, cost=cost, alpha=alpha, attempts=att, change=chg, tracking_error=trk, terminal_error=trm,
                    seconds=dict(zip(("backward", "gradprox", "optimistic_forward", "cost", "backtracking"), sec)))

    def pgd_get(self, what):
        out = self._out(rows=self._pgd_M + 1)
        check(self.lib.vch2d_pgd_get(self.ctx, {"u": 0, "phi": 1, "r": 2, "phi_Q": 3}[what], _dp(out)))
        return self._sq(out)

    SECOND_ORDER_KEYS = ("s_state", "s_ctrl", "c_gn", "c_state", "c_ctrl", "n_h")

    def second_order(self, h, dt=None, t_hist=None, opt=None, phi_Q=None, phi_T=None, x=None, y=None, order=2, rtol=0.0,
                     histories=False):
        """Exact J'(u)h and J''(u)[h,h] of the smooth part J1 + J2 + J3 about the resident control and state history
        (vch2d_second_order): tangent marches, two linear solves per step and direction, no finite differences.
        After forward(): dt, t_hist are required, x / y default to the engine's grid, phi_Q / phi_T None are zeros.  After
        pgd_init() / pgd_iterate(): the current iterate with the problem's grid, time levels and targets (leave dt, t_hist,
        x, y, phi_Q, phi_T None).
        h: (B, rows, Nx+1, Ny+1), the row rule of a control.  opt: one parameter object or a sequence of B (only b1, b2, b3
        are read).  Returns a dict of [B] arrays: the six scalars of SECOND_ORDER_KEYS, slope = s_state + s_ctrl,
        curvature = c_gn + c_state + c_ctrl (NaN with order=1), `stats`, and with histories=True dphi, d2phi [B][M+1][..]."""
        h = self._hist(h, 0, "h")
        if dt is None or t_hist is None:
            if not hasattr(self, "_pgd_M"):
                raise ValueError("dt and t_hist are required without a resident PGD problem")
            dt = t_hist = None
            M = self._pgd_M
        else:
            dt = np.ascontiguousarray(dt, dtype=np.float64)
            t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
            M = int(dt.size)
            if t_hist.size != M + 1:
                raise ValueError("t_hist must have len(dt) + 1 entries")
            x = self.x if x is None else x
            y = self.y if y is None else y
        if x is not None or y is not None:
            x = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
            y = np.ascontiguousarray(self.y if y is None else y, dtype=np.float64)
            if x.shape != (self.Nx + 1,) or y.shape != (self.Ny + 1,):
                raise ValueError("x, y must have Nx+1, Ny+1 entries")
        pq = None if phi_Q is None else self._hist(phi_Q, M + 1, "phi_Q_target")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        seq = list(opt) if isinstance(opt, (list, tuple)) else [opt]
        arr = (OptParams * len(seq))(*[o if isinstance(o, OptParams) else make_opt(o) for o in seq])
        out = np.empty((self.B, 6))
        d1 = self._out(rows=M + 1) if histories else None
        d2 = self._out(rows=M + 1) if histories else None
        if d2 is not None:
            d2[...] = 0.0
        st = Stats()
        check(self.lib.vch2d_second_order(self.ctx, _dp(h), int(h.shape[1]), _dp(dt), M, _dp(t_hist), _dp(x), _dp(y), _dp(pq),
                                          _dp(pt), arr, len(seq), int(order), float(rtol), _dp(out), _dp(d1), _dp(d2),
                                          C.byref(st)))
        res = {k: out[:, i].copy() for i, k in enumerate(self.SECOND_ORDER_KEYS)}
        res["slope"] = out[:, 0] + out[:, 1]
        res["curvature"] = (out[:, 2] + out[:, 3]) + out[:, 4]
        res["stats"] = st.as_dict()
        if histories:
            res["dphi"], res["d2phi"] = d1, d2
        return res

    def hessvec(self, h, dt=None, t_hist=None, opt=None, phi_Q=None, phi_T=None, x=None, y=None, order=2, rtol=0.0,
                g_rows=None):
        """Exact gradient field and Hessian-vector product of the smooth part J1 + J2 + J3 of the discrete cost about the
        resident control and state history (vch2d_hessvec): the transposed sweep of second_order's tangent march, one
        linear solve per step for the gradient, three for H h; no finite differences and no nonlinear march.
        Base point and arguments as for second_order (after forward(): dt, t_hist required; after pgd_init() /
        pgd_iterate(): leave dt, t_hist, x, y, phi_Q, phi_T None).  h: (B, rows, Nx+1, Ny+1) or None with order=1.
        g_rows: rows of the control the gradient refers to; None resolves to M + 1 about a PGD iterate, to
        min(rows of the control, M + 1) after forward() with a control, and to M + 1 after a forward() without one.
        Returns dict(grad (B, g_rows, ..), hv (B, rows, ..) or None, dots (B, 2), slope = sum(grad h), curvature =
        sum(h hv): [B], reduced on the device, NaN where a factor is missing; stats).  grad and hv are EUCLIDEAN
        derivatives with respect to the entries of u: J'(u)h = sum(grad * h) and J''(u)[h,h] = sum(h * hv) as plain
        sums, second_order's slope and curvature when h has g_rows rows."""
        order = int(order)
        h = None if h is None else self._hist(h, 0, "h")
        if dt is None or t_hist is None:
            if not hasattr(self, "_pgd_M"):
                raise ValueError("dt and t_hist are required without a resident PGD problem")
            dt = t_hist = None
            M = self._pgd_M
        else:
            dt = np.ascontiguousarray(dt, dtype=np.float64)
            t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
            M = int(dt.size)
            if t_hist.size != M + 1:
                raise ValueError("t_hist must have len(dt) + 1 entries")
            x = self.x if x is None else x
            y = self.y if y is None else y
        if x is not None or y is not None:
            x = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
            y = np.ascontiguousarray(self.y if y is None else y, dtype=np.float64)
            if x.shape != (self.Nx + 1,) or y.shape != (self.Ny + 1,):
                raise ValueError("x, y must have Nx+1, Ny+1 entries")
        if g_rows is None:
            kind, _, rows = getattr(self, "_base", ("forward", M, 0))
            g_rows = M + 1 if (kind == "pgd" or rows == 0) else min(rows, M + 1)
        g_rows = int(g_rows)
        pq = None if phi_Q is None else self._hist(phi_Q, M + 1, "phi_Q_target")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        seq = list(opt) if isinstance(opt, (list, tuple)) else [opt]
        arr = (OptParams * len(seq))(*[o if isinstance(o, OptParams) else make_opt(o) for o in seq])
        h_rows = 1 if h is None else int(h.shape[1])
        grad = np.empty((self.B, max(g_rows, 0)) + self.shape)
        hv = np.empty((self.B, h_rows) + self.shape) if order == 2 and h is not None else None
        dots = np.full((self.B, 2), np.nan)
        st = Stats()
        check(self.lib.vch2d_hessvec(self.ctx, _dp(h), h_rows, g_rows, _dp(dt), M, _dp(t_hist), _dp(x), _dp(y), _dp(pq),
                                     _dp(pt), arr, len(seq), order, float(rtol), _dp(grad), _dp(hv), _dp(dots),
                                     C.byref(st)))
        return dict(grad=grad, hv=hv, dots=dots, slope=dots[:, 0].copy(), curvature=dots[:, 1].copy(), stats=st.as_dict())

    def exact_gradient(self, dt=None, t_hist=None, opt=None, phi_Q=None, phi_T=None, x=None, y=None, rtol=0.0, g_rows=None):
        """The exact discrete gradient d(J1+J2+J3)/du about the resident base point as a field (B, g_rows, Nx+1, Ny+1):
        hessvec with order=1 and no direction.  Euclidean, see hessvec; unlike the hand-derived adjoint of backward() it
        carries the cost's quadrature weights and the transpose of the mass fix."""
        return self.hessvec(None, dt=dt, t_hist=t_hist, opt=opt, phi_Q=phi_Q, phi_T=phi_T, x=x, y=y, order=1, rtol=rtol,
                            g_rows=g_rows)["grad"]

    def hess_lanczos(self, q0, k, dt=None, t_hist=None, opt=None, phi_Q=None, phi_T=None, x=None, y=None, mask=None, tol=0.0,
                     reorth=True, rtol=0.0):
        """Lanczos on the reduced Hessian P H P about the resident base point with the basis, the free set and the
        recurrence on the device (vch2d_hess_lanczos); base point and arguments as for hessvec.  q0: (B, M+1, Nx+1, Ny+1)
        start vector.  mask: the free set as (B, M+1, Nx+1, Ny+1) booleans / bytes, or None: built on the device from the
        resident control and every trajectory's own u_min, u_max of `opt` with `tol` (<= 0: 1e-8).  reorth: full
        reorthogonalisation (k + 1 resident vectors) or the three-term recurrence (3 resident vectors).
        Returns dict(alpha, beta: (B, k), NaN beyond steps; steps, n_free: [B]; stats)."""
        k = int(k)
        if dt is None or t_hist is None:
            if not hasattr(self, "_pgd_M"):
                raise ValueError("dt and t_hist are required without a resident PGD problem")
            dt = t_hist = None
            M = self._pgd_M
        else:
            dt = np.ascontiguousarray(dt, dtype=np.float64)
            t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
            M = int(dt.size)
            if t_hist.size != M + 1:
                raise ValueError("t_hist must have len(dt) + 1 entries")
            x = self.x if x is None else x
            y = self.y if y is None else y
        if x is not None or y is not None:
            x = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
            y = np.ascontiguousarray(self.y if y is None else y, dtype=np.float64)
            if x.shape != (self.Nx + 1,) or y.shape != (self.Ny + 1,):
                raise ValueError("x, y must have Nx+1, Ny+1 entries")
        q0 = None if q0 is None else self._hist(q0, M + 1, "q0")
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if mask.ndim == 3 and self.B == 1:
                mask = mask.reshape((1,) + mask.shape)
            if mask.shape != (self.B, M + 1) + self.shape:
                raise ValueError(f"mask must have shape ({self.B}, {M + 1}, {self.Nx + 1}, {self.Ny + 1}), got {mask.shape}")
        pq = None if phi_Q is None else self._hist(phi_Q, M + 1, "phi_Q_target")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        seq = list(opt) if isinstance(opt, (list, tuple)) else [opt]
        arr = (OptParams * len(seq))(*[o if isinstance(o, OptParams) else make_opt(o) for o in seq])
        kk = max(k, 1)
        alpha, beta = np.full((self.B, kk), np.nan), np.full((self.B, kk), np.nan)
        steps, n_free = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int64)
        st = Stats()
        check(self.lib.vch2d_hess_lanczos(self.ctx, _dp(dt), M, _dp(t_hist), _dp(x), _dp(y), _dp(pq), _dp(pt), arr, len(seq),
                                          float(rtol), None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          float(tol), _dp(q0), k, int(reorth), _dp(alpha), _dp(beta),
                                          steps.ctypes.data_as(_lib._I32), n_free.ctypes.data_as(C.POINTER(C.c_int64)),
                                          C.byref(st)))
        self._kr_rows = M + 1
        return dict(alpha=alpha, beta=beta, steps=steps, n_free=n_free, stats=st.as_dict())

    def krylov_vector(self, coef):
        """(B, M+1, Nx+1, Ny+1): sum_j coef[b][j] q_j from the basis the last hess_lanczos left resident
        (vch2d_krylov_vector).  coef: (B, m), or (m,) with batch 1."""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim == 1 and self.B == 1:
            coef = coef.reshape(1, -1)
        if coef.ndim != 2 or coef.shape[0] != self.B:
            raise ValueError(f"coef must have shape ({self.B}, m), got {coef.shape}")
        out = self._out(rows=getattr(self, "_kr_rows", 1))
        check(self.lib.vch2d_krylov_vector(self.ctx, _dp(coef), int(coef.shape[1]), _dp(out)))
        return out

    def _base_point(self, dt, t_hist, x, y):
        """dt, t_hist, x, y as the calls about a resident base point pass them on, and M: all None about a resident PGD
        problem, checked arrays (x, y defaulting to the engine's grid) after forward()."""
        if dt is None or t_hist is None:
            if not hasattr(self, "_pgd_M"):
                raise ValueError("dt and t_hist are required without a resident PGD problem")
            dt = t_hist = None
            M = self._pgd_M
        else:
            dt = np.ascontiguousarray(dt, dtype=np.float64)
            t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
            M = int(dt.size)
            if t_hist.size != M + 1:
                raise ValueError("t_hist must have len(dt) + 1 entries")
            x = self.x if x is None else x
            y = self.y if y is None else y
        if x is not None or y is not None:
            x = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
            y = np.ascontiguousarray(self.y if y is None else y, dtype=np.float64)
            if x.shape != (self.Nx + 1,) or y.shape != (self.Ny + 1,):
                raise ValueError("x, y must have Nx+1, Ny+1 entries")
        return dt, t_hist, x, y, M

    def _free_mask(self, mask, M):
        """A free set as (B, M+1, Nx+1, Ny+1) bytes (None stays None: built on the device)."""
        if mask is None:
            return None
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.ndim == 3 and self.B == 1:
            mask = mask.reshape((1,) + mask.shape)
        if mask.shape != (self.B, M + 1) + self.shape:
            raise ValueError(f"mask must have shape ({self.B}, {M + 1}, {self.Nx + 1}, {self.Ny + 1}), got {mask.shape}")
        return mask

    CG_STATUS = ("limit", "converged", "negcurv", "breakdown")      # VCH_CG_LIMIT .. VCH_CG_BREAKDOWN

    def hess_cg(self, k, rhs=None, cg_tol=0.0, precond=True, mask=None, tol=0.0, dt=None, t_hist=None, opt=None, phi_Q=None,
                phi_T=None, x=None, y=None, rtol=0.0):
        """(Preconditioned) conjugate gradients on P H P x = P b about the resident base point with x, r, p, the free set
        and the recurrence on the device (vch2d_hess_cg); base point, mask and tol as for hess_lanczos.  rhs: (B, M+1,
        Nx+1, Ny+1), or None: the Newton right-hand side -(grad(J1+J2+J3) + kappa_sparsity wt W_cost sign(u)) of the full
        cost on the free set, built on the device.  precond: scale by the L2(Q) mass diag(wt W_cost) of the control.
        cg_tol: relative residual at which a trajectory stops (<= 0: 1e-8); k: steps at most.
        Returns dict(steps, status (indices of CG_STATUS), n_free: [B]; resid, curv: (B, k), NaN beyond steps (curv[steps]
        is the stopping curvature after "negcurv"); pred: [B] decrease of the quadratic model; rnorm0: [B] ||P b||; stats)."""
        k = int(k)
        dt, t_hist, x, y, M = self._base_point(dt, t_hist, x, y)
        rhs = None if rhs is None else self._hist(rhs, M + 1, "rhs")
        mask = self._free_mask(mask, M)
        pq = None if phi_Q is None else self._hist(phi_Q, M + 1, "phi_Q_target")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        seq = list(opt) if isinstance(opt, (list, tuple)) else [opt]
        arr = (OptParams * len(seq))(*[o if isinstance(o, OptParams) else make_opt(o) for o in seq])
        kk = max(k, 1)
        resid, curv = np.full((self.B, kk), np.nan), np.full((self.B, kk), np.nan)
        pred, rnorm0 = np.full(self.B, np.nan), np.full(self.B, np.nan)
        steps, status, n_free = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int64)
        st = Stats()
        precond = int(precond) if isinstance(precond, (bool, int, np.integer)) else -1
        check(self.lib.vch2d_hess_cg(self.ctx, _dp(dt), M, _dp(t_hist), _dp(x), _dp(y), _dp(pq), _dp(pt), arr, len(seq),
                                     float(rtol), None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     float(tol), _dp(rhs), k, float(cg_tol), precond, _dp(resid), _dp(curv), _dp(pred),
                                     _dp(rnorm0), steps.ctypes.data_as(_lib._I32), status.ctypes.data_as(_lib._I32),
                                     n_free.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st)))
        self._cg_rows = M + 1
        return dict(steps=steps, status=status, n_free=n_free, resid=resid, curv=curv, pred=pred, rnorm0=rnorm0,
                    stats=st.as_dict())

    def cg_vector(self, which="x"):
        """(B, M+1, Nx+1, Ny+1): the solution x, the residual r or the direction p the last hess_cg left resident
        (vch2d_cg_vector); masked-off nodes are exact zeros."""
        if which not in ("x", "r", "p"):
            raise ValueError(f"which must be 'x', 'r' or 'p', got {which!r}")
        out = self._out(rows=getattr(self, "_cg_rows", 1))
        check(self.lib.vch2d_cg_vector(self.ctx, "xrp".index(which), _dp(out)))
        return out

    NEWTON_STATUS = ("accepted", "stationary", "negcurv", "breakdown", "stalled", "idle")   # VCH_NEWTON_ACCEPTED .. _IDLE

    def pgd_newton(self, n_rounds, k=50, cg_tol=1e-8, precond=True, tol=0.0, rtol=0.0, max_halvings=10):
        """Damped Newton rounds on the free set about the resident PGD iterate (vch2d_pgd_newton), every trajectory with
        its own parameters and decisions; no history crosses the bus.  Per round: the Newton-CG step of hess_cg(rhs=None)
        on the free set of the iterate, then trials clip(u + s x, box) for s = 1, 1/2, ... (a free node whose sign the trial
        flips is set to 0), at most `max_halvings` halvings; the first s with J(trial) <= J(u) - 1e-4 s pred is accepted.
        A trajectory ends with "stationary" (zero right-hand side or empty free set), "negcurv" (the first CG direction has
        non-positive curvature), "breakdown" (CG broke down: no march is started) or "stalled" (no s accepted) and is "idle"
        in all later rounds.  Returns dict(rounds: rounds run; cost, cost_new, s, pred, rnorm0: (B, n_rounds), NaN where idle;
        halvings, cg_steps, cg_status (indices of CG_STATUS), status (indices of NEWTON_STATUS): int32 (B, n_rounds);
        n_free, pinned, clipped: int64 (B, n_rounds); seconds).  pgd_get, hess_cg, ... then work about the new iterate and
        a following pgd_iterate is that of pgd_init(u0 = the Newton iterate)."""
        n = max(int(n_rounds), 1)
        dbl = [np.full((self.B, n), np.nan) for _ in range(5)]
        i32 = [np.zeros((self.B, n), dtype=np.int32) for _ in range(4)]
        cnt = np.zeros((self.B, n, 3), dtype=np.int64)
        sec = np.zeros(4)
        precond = int(precond) if isinstance(precond, (bool, int, np.integer)) else -1
        done = check(self.lib.vch2d_pgd_newton(self.ctx, int(n_rounds), int(k), float(cg_tol), precond, float(tol), float(rtol),
                                               int(max_halvings), *[_dp(a) for a in dbl],
                                               *[a.ctypes.data_as(_lib._I32) for a in i32],
                                               cnt.ctypes.data_as(C.POINTER(C.c_int64)), _dp(sec)))
        self._base = ("pgd", self._pgd_M, self._pgd_M + 1)
        self._cg_rows = self._pgd_M + 1
        out = dict(zip(("cost", "cost_new", "s", "pred", "rnorm0"), dbl), rounds=done)
        out.update(zip(("halvings", "cg_steps", "cg_status", "status"), i32))
        out.update(n_free=cnt[:, :, 0].copy(), pinned=cnt[:, :, 1].copy(), clipped=cnt[:, :, 2].copy(),
                   seconds=dict(zip(("solve", "trial", "forward", "cost"), sec)))
        return out

    def newton_trial(self, s, want_u=True):
        """The trial control t = clip(u + s_b x, box_b) of the step lengths `s` ([B] or a scalar, finite and > 0) about the
        resident control, with x, the free set and the box of the last hess_cg (vch2d_newton_trial): a free node with
        t u < 0 becomes 0.  Writes only the trial-control scratch.  Returns dict(u: (B, M+1, Nx+1, Ny+1) or None,
        change: (B, 2) = {sum (t - u)^2, sum u^2}, pinned, clipped: int64 [B])."""
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(s, dtype=np.float64), (self.B,)))
        out = self._out(rows=getattr(self, "_cg_rows", 1)) if want_u else None
        chg = np.full((self.B, 2), np.nan)
        cnt = np.zeros((self.B, 2), dtype=np.int64)
        check(self.lib.vch2d_newton_trial(self.ctx, _dp(s), _dp(out), _dp(chg), cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(u=out, change=chg, pinned=cnt[:, 0].copy(), clipped=cnt[:, 1].copy())

    TRUST_CG_STATUS = CG_STATUS + ("boundary",)                     # VCH_CG_LIMIT .. VCH_CG_BOUNDARY
    TRUST_STATUS = NEWTON_STATUS + ("rejected",)                    # VCH_NEWTON_ACCEPTED .. _REJECTED

    def hess_cg_trust(self, k, radius, rhs=None, cg_tol=0.0, precond=True, mask=None, tol=0.0, dt=None, t_hist=None, opt=None,
                      phi_Q=None, phi_T=None, x=None, y=None, rtol=0.0):
        """Truncated (Steihaug-Toint) conjugate gradients on P H P x = P b inside ||x||_D <= radius_b (vch2d_hess_cg_tr):
        hess_cg with a trust region in the preconditioner's norm, ||x||_D^2 = sum D x^2, D = diag(wt W_cost) with precond and
        the identity without.  radius: [B] or a scalar, > 0, +inf allowed.  A step that would leave the region, or a
        direction of non-positive curvature, is followed to the boundary: "boundary" and "negcurv" of TRUST_CG_STATUS.
        Returns hess_cg's dict (status: indices of TRUST_CG_STATUS) plus xnorm: [B] ||x||_D by the recurrence.  With
        radius = inf everything equals hess_cg's bit for bit on a trajectory that ends "converged" or "limit".  A radius
        whose square is not finite (>= 2^512) has no boundary and acts as +inf; a radius whose square underflows gives a zero
        step (x = 0 after one counted step)."""
        k = int(k)
        dt, t_hist, x, y, M = self._base_point(dt, t_hist, x, y)
        rhs = None if rhs is None else self._hist(rhs, M + 1, "rhs")
        mask = self._free_mask(mask, M)
        pq = None if phi_Q is None else self._hist(phi_Q, M + 1, "phi_Q_target")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        seq = list(opt) if isinstance(opt, (list, tuple)) else [opt]
        arr = (OptParams * len(seq))(*[o if isinstance(o, OptParams) else make_opt(o) for o in seq])
        radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.B,)))
        kk = max(k, 1)
        resid, curv = np.full((self.B, kk), np.nan), np.full((self.B, kk), np.nan)
        pred, rnorm0, xnorm = np.full(self.B, np.nan), np.full(self.B, np.nan), np.full(self.B, np.nan)
        steps, status, n_free = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int64)
        st = Stats()
        precond = int(precond) if isinstance(precond, (bool, int, np.integer)) else -1
        check(self.lib.vch2d_hess_cg_tr(self.ctx, _dp(dt), M, _dp(t_hist), _dp(x), _dp(y), _dp(pq), _dp(pt), arr, len(seq),
                                        float(rtol), None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        float(tol), _dp(rhs), k, float(cg_tol), precond, _dp(resid), _dp(curv), _dp(pred),
                                        _dp(rnorm0), steps.ctypes.data_as(_lib._I32), status.ctypes.data_as(_lib._I32),
                                        n_free.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st), _dp(radius), _dp(xnorm)))
        self._cg_rows = M + 1
        return dict(steps=steps, status=status, n_free=n_free, resid=resid, curv=curv, pred=pred, rnorm0=rnorm0, xnorm=xnorm,
                    stats=st.as_dict())

    def pgd_trust(self, n_rounds, radius0, k=50, cg_tol=1e-8, precond=True, tol=0.0, rtol=0.0, radius_max=None, radius_min=None):
        """Trust-region (Steihaug) Newton-CG rounds on the free set about the resident PGD iterate (vch2d_pgd_trust), every
        trajectory with its own parameters, radius and decisions; no history crosses the bus.  Per round: the step of
        hess_cg_trust(rhs=None) inside the trajectory's radius (a direction of non-positive curvature is followed to the
        boundary and does not end the trajectory), one trial clip(u + x, box) as newton_trial(1) builds it,
        rho = (J(u) - J(trial)) / pred.  The trial is accepted iff J(trial) is finite and <= J(u) - 1e-4 pred; otherwise the
        trajectory stays unmoved, "rejected", and goes on.  The radius: rho < 1/4 or not finite: min(radius, ||x||_D) / 4;
        else rho > 3/4 after a "boundary" or "negcurv" exit: min(2 radius, radius_max).  A trajectory ends "stationary",
        "breakdown", or "stalled" (rejected with the radius below radius_min) and is "idle" afterwards.  radius0: [B] or a
        scalar, finite and > 0; radius_max / radius_min default to 1024 max(radius0) and 1e-10 min(radius0).  Returns the
        keys of Engine1D.pgd_trust: dict(rounds; cost, cost_new, pred, rnorm0, radius (the round's), ratio, xnorm:
        (B, n_rounds), NaN where idle; cg_steps, cg_status (indices of TRUST_CG_STATUS), status (indices of TRUST_STATUS):
        int32 (B, n_rounds); n_free, pinned, clipped: int64 (B, n_rounds); seconds)."""
        n = max(int(n_rounds), 1)
        radius0 = np.ascontiguousarray(np.broadcast_to(np.asarray(radius0, dtype=np.float64), (self.B,)))
        radius_max = 1024.0 * float(np.max(radius0)) if radius_max is None else float(radius_max)
        radius_min = 1e-10 * float(np.min(radius0)) if radius_min is None else float(radius_min)
        dbl = [np.full((self.B, n), np.nan) for _ in range(7)]
        i32 = [np.zeros((self.B, n), dtype=np.int32) for _ in range(3)]
        cnt = np.zeros((self.B, n, 3), dtype=np.int64)
        sec = np.zeros(4)
        precond = int(precond) if isinstance(precond, (bool, int, np.integer)) else -1
        done = check(self.lib.vch2d_pgd_trust(self.ctx, int(n_rounds), int(k), float(cg_tol), precond, float(tol), float(rtol),
                                              _dp(radius0), radius_max, radius_min, *[_dp(a) for a in dbl],
                                              *[a.ctypes.data_as(_lib._I32) for a in i32],
                                              cnt.ctypes.data_as(C.POINTER(C.c_int64)), _dp(sec)))
        self._base = ("pgd", self._pgd_M, self._pgd_M + 1)
        self._cg_rows = self._pgd_M + 1
        out = dict(zip(("cost", "cost_new", "pred", "rnorm0", "radius", "ratio", "xnorm"), dbl), rounds=done)
        out.update(zip(("cg_steps", "cg_status", "status"), i32))
        out.update(n_free=cnt[:, :, 0].copy(), pinned=cnt[:, :, 1].copy(), clipped=cnt[:, :, 2].copy(),
                   seconds=dict(zip(("solve", "trial", "forward", "cost"), sec)))
        return out

    def mass_shifts(self):
        """(B, M): what the march's interior mass fix subtracted at the end of every step of the resident state history
        (vch2d_mass_shifts; zeros where the fix was not applied); M = the steps of that history."""
        buf = np.empty(self.B * self.max_steps)
        M = check(self.lib.vch2d_mass_shifts(self.ctx, _dp(buf)))
        return buf[:self.B * M].reshape(self.B, M).copy()

    def pgd_cost_device_ptr(self):
        p = C.c_void_p()
        check(self.lib.vch2d_pgd_cost_dev(self.ctx, C.byref(p)))
        return p.value

    def free_energy(self, phi_hist, hx=None, hy=None, w_hist=None, eps=None):
        """Free energy of every level (F2:256-319): phi_hist (B, rows, Nx+1, Ny+1) or "resident".
        Returns (B, rows) (or (rows,) for one trajectory)."""
        hx = float(self.x[1] - self.x[0]) if hx is None else float(hx)
        hy = float(self.y[1] - self.y[0]) if hy is None else float(hy)
        if isinstance(phi_hist, str) and phi_hist == "resident":
            if w_hist is None:
                raise ValueError("free_energy('resident') needs the number of levels: pass w_hist or use free_energy_resident(rows)")
            ph, rows = C.cast(C.c_void_p(1), _lib._D), None
        else:
            ph = self._hist(phi_hist, 0, "phi_hist")
            rows = int(ph.shape[1])
        wh = None if w_hist is None else self._hist(w_hist, rows or 0, "w_hist")
        if rows is None:
            rows = int(wh.shape[1])
        E = np.empty((self.B, rows))
        check(self.lib.vch2d_free_energy(self.ctx, ph if not isinstance(ph, np.ndarray) else _dp(ph), rows, _dp(wh), hx, hy,
                                         float(eps or 0.0), _dp(E)))
        return self._sq(E)

    def free_energy_resident(self, rows, hx=None, hy=None, eps=None):
        """Free energy of the first `rows` levels of the state history left by the last march."""
        hx = float(self.x[1] - self.x[0]) if hx is None else float(hx)
        hy = float(self.y[1] - self.y[0]) if hy is None else float(hy)
        E = np.empty((self.B, int(rows)))
        check(self.lib.vch2d_free_energy(self.ctx, C.cast(C.c_void_p(1), _lib._D), int(rows), None, hx, hy, float(eps or 0.0), _dp(E)))
        return self._sq(E)

    # -- in-situ kernel timing -------------------------------------------------------------
    PROF_CLASSES = ("schur_p", "dct_gemm", "residual", "adj_q", "cg_update", "adj_rhs", "cost", "prox", "dct_rows_fwd",
                    "dct_cols", "dct_rows_inv", "schur_p_first", "cg_rows_fwd", "cg_rows_fwd_first", "event_pair_noop", "guess",
                    "adj_guess", "cheb_rows", "cheb_rows_first", "residual_first")

    def counters(self):
        """(kernel launches, blocking looks of the host at the device state) since the context was created."""
        out = np.zeros(2, dtype=np.int64)
        check(self.lib.vch2d_counters(self.ctx, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return int(out[0]), int(out[1])

    def prof_begin(self, max_launches=200000):
        check(self.lib.vch2d_prof_begin(self.ctx, int(max_launches)))

    def prof_end(self):
        n = len(self.PROF_CLASSES)
        ms = np.zeros(n)
        cnt = np.zeros(n, dtype=np.int64)
        check(self.lib.vch2d_prof_end(self.ctx, _dp(ms), cnt.ctypes.data_as(C.POINTER(C.c_int64)), n))
        return {k: dict(ms=float(ms[i]), launches=int(cnt[i])) for i, k in enumerate(self.PROF_CLASSES)}

    def prof_spans(self):
        """{class: float32 array of the event-pair spans (us) of every launch recorded between prof_begin and prof_end}."""
        cap = 1 << 20
        cls = np.zeros(cap, dtype=np.int32)
        ms = np.zeros(cap, dtype=np.float32)
        n = check(self.lib.vch2d_prof_spans(self.ctx, cls.ctypes.data_as(C.POINTER(C.c_int32)),
                                            ms.ctypes.data_as(C.POINTER(C.c_float)), cap))
        n = min(int(n), cap)
        return {k: 1e3 * ms[:n][cls[:n] == i] for i, k in enumerate(self.PROF_CLASSES)}


class Engine1D:
    """One GPU context for `batch` 1D trajectories on N+1 nodes (N <= 4096)."""

    def __init__(self, N, Lx=1.0, tau=0.05, gamma=10.0, c1=0.75, c2=1.0, kappa=0.03 ** 2, batch=1,
                 max_steps=128, device=0):
        self.lib = _lib.load()
        if self.lib.vch_device_count() <= 0:
            raise VchError("no HIP device visible: the engine has no CPU path")
        self.p = Params1D(int(N), float(Lx), float(tau), float(gamma), float(c1), float(c2), float(kappa))
        self.B, self.max_steps, self.N, self.n = int(batch), int(max_steps), int(N), int(N) + 1
        self.ctx = self.lib.vch1d_create(C.byref(self.p), self.B, self.max_steps, int(device))
        if not self.ctx:
            raise ValueError("vch1d_create failed: " + _lib.last_error())
        self.x = np.linspace(0, float(Lx), self.n)

    @classmethod
    def from_config(cls, cfg, **kw):
        return cls(cfg.N, cfg.Lx, cfg.tau, cfg.gamma, cfg.c1, cfg.c2, cfg.kappa, **kw)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.vch1d_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fld(self, a, name="field"):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape == (self.n,) and self.B == 1:
            a = a.reshape(1, self.n)
        if a.shape != (self.B, self.n):
            raise ValueError(f"{name} must have shape ({self.n},) [batch {self.B}], got {a.shape}")
        return a

    def _hist(self, a, rows=0, name="history"):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim == 2 and self.B == 1:
            a = a.reshape((1,) + a.shape)
        if a.ndim != 3 or a.shape[0] != self.B or a.shape[2] != self.n or (rows and a.shape[1] != rows):
            raise ValueError(f"{name} must have shape (rows, {self.n}), got {a.shape}")
        return a

    def _sq(self, a):
        return a[0] if self.B == 1 else a

    def apply_laplacian(self, v):
        v = self._fld(v)
        out = np.empty_like(v)
        check(self.lib.vch1d_apply_laplacian(self.ctx, _dp(v), _dp(out)))
        return self._sq(out)

    def residuals(self, phi_new, phi_old, mu_new, mu_old, w_new, w_old, dt):
        a = [self._fld(v) for v in (phi_new, phi_old, mu_new, mu_old, w_new, w_old)]
        Rp, Rm = np.empty_like(a[0]), np.empty_like(a[0])
        check(self.lib.vch1d_residuals(self.ctx, *[_dp(v) for v in a], float(dt), _dp(Rp), _dp(Rm)))
        return self._sq(Rp), self._sq(Rm)

    def jacobian_solve(self, phi_new, dt, rhs_phi, rhs_mu):
        a = [self._fld(v) for v in (phi_new, rhs_phi, rhs_mu)]
        o1, o2 = np.empty_like(a[0]), np.empty_like(a[0])
        check(self.lib.vch1d_jacobian_solve(self.ctx, _dp(a[0]), float(dt), _dp(a[1]), _dp(a[2]), _dp(o1), _dp(o2)))
        return self._sq(o1), self._sq(o2)

    def adjoint_solve(self, phi_n, dt, rhs):
        phi_n = None if phi_n is None else self._fld(phi_n)
        rhs = self._fld(rhs)
        out = np.empty_like(rhs)
        check(self.lib.vch1d_adjoint_solve(self.ctx, _dp(phi_n), float(dt), _dp(rhs), _dp(out)))
        return self._sq(out)

    def newton_raphson(self, phi_old, mu_old, w_old, w_new, dt, hist_cap=64):
        a = [self._fld(v) for v in (phi_old, mu_old, w_old, w_new)]
        pn, mn = np.empty_like(a[0]), np.empty_like(a[0])
        hist = np.zeros((self.B, hist_cap))
        nh = np.zeros(self.B, dtype=np.int32)
        check(self.lib.vch1d_newton_raphson(self.ctx, *[_dp(v) for v in a], float(dt), _dp(pn), _dp(mn), _dp(hist),
                                            int(hist_cap), nh.ctypes.data_as(_lib._I32)))
        hists = [hist[b, :nh[b]].copy() for b in range(self.B)]
        return self._sq(pn), self._sq(mn), (hists[0] if self.B == 1 else hists)

    def forward(self, phi0, dt, u=None, store=True):
        """Returns (phi_hist with M+2 rows or None, stats)."""
        phi0 = self._fld(phi0, "phi0")
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        M = int(dt.size)
        rows = 0
        if u is not None:
            u = self._hist(u, 0, "control_input")
            rows = int(u.shape[1])
            if rows < M:          # the reference indexes control_input[step] for every step (F1:347-353)
                raise IndexError(f"index {rows} is out of bounds for axis 0 with size {rows}")
            if rows > M + 2:
                u = np.ascontiguousarray(u[:, :M + 2])
                rows = M + 2
        out = np.empty((self.B, M + 2, self.n)) if store else None
        st = Stats()
        check(self.lib.vch1d_forward(self.ctx, _dp(phi0), _dp(u), rows, _dp(dt), M, _dp(out), C.byref(st)))
        return (self._sq(out) if store else None), st.as_dict()

    def backward(self, phi_hist, t_hist, b1, b2, phi_Q=None, phi_T=None, h=None):
        t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
        rows = int(t_hist.size)
        ph = None if phi_hist is None else self._hist(phi_hist, rows, "phi_hist")
        pq = None if phi_Q is None else self._hist(phi_Q, rows, "phi_Q")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        p, q, r = (np.empty((self.B, rows, self.n)) for _ in range(3))
        h = float(self.x[1] - self.x[0]) if h is None else float(h)
        check(self.lib.vch1d_backward(self.ctx, _dp(ph), rows, _dp(t_hist), h, float(b1), float(b2), _dp(pq), _dp(pt),
                                      _dp(p), _dp(q), _dp(r)))
        return self._sq(p), self._sq(q), self._sq(r)

    # the sparsity functional: index = VCH_SPARSITY_* of include/vch.h
    SPARSITY = ("full", "time", "space")

    @classmethod
    def _mode(cls, sparsity):
        if sparsity not in cls.SPARSITY:
            raise ValueError(f"sparsity must be one of {cls.SPARSITY}, got {sparsity!r}")
        return cls.SPARSITY.index(sparsity)

    def cost(self, phi_hist, u, phi_Q, phi_T, x, t_hist, opt, sparsity="full"):
        """J (B, 5) = {J1, J2, J3, J4, J}.  `sparsity`: J4 = kappa_s int int |u| ("full"), kappa_s int ||u(., t)||_L2(Omega) dt
        ("time") or kappa_s int ||u(x, .)||_L2(0,T) dx ("space")."""
        mode = self._mode(sparsity)
        t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
        rows = int(t_hist.size)
        ph = self._hist(phi_hist, rows, "phi_hist")
        uu = None if u is None else self._hist(u, rows, "u")
        pq = None if phi_Q is None else self._hist(phi_Q, rows, "phi_Q_target")
        pt = None if phi_T is None else self._fld(phi_T, "phi_T_target")
        x = np.ascontiguousarray(x, dtype=np.float64)
        J = np.empty((self.B, 5))
        o = opt if isinstance(opt, OptParams) else make_opt(opt)
        if mode == 0:
            check(self.lib.vch1d_cost(self.ctx, _dp(ph), _dp(uu), _dp(pq), _dp(pt), rows, _dp(x), _dp(t_hist), C.byref(o), _dp(J)))
        else:
            check(self.lib.vch1d_cost_g(self.ctx, _dp(ph), _dp(uu), _dp(pq), _dp(pt), rows, _dp(x), _dp(t_hist), C.byref(o), mode,
                                        _dp(J)))
        return J[0] if self.B == 1 else J

    def grad_prox(self, u, r, alpha, opt, sparsity="full", x=None, t_hist=None, return_scale=False):
        """prox of the sparsity term at u - alpha (r + b3 u) under the box of `opt`.  `sparsity` "time" / "space": the prox
        of the group norm over the rows (weights: trapezoid in `x`, default the engine's grid) or the columns (weights:
        trapezoid in `t_hist`, required) of the control; the box must contain 0.  return_scale=True: (u+, s) with s the
        factor of every group, (B, rows) or (B, N+1): u+ = clip(s v), 0 for a group that vanishes."""
        mode = self._mode(sparsity)
        u = self._hist(u, 0, "u")
        r = self._hist(r, u.shape[1], "r")
        rows = int(u.shape[1])
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (self.B,)))
        out = np.empty_like(u)
        o = opt if isinstance(opt, OptParams) else make_opt(opt)
        if mode == 0:
            if return_scale:
                raise ValueError('return_scale needs sparsity "time" or "space": the node-wise prox has no group factor')
            check(self.lib.vch1d_grad_prox(self.ctx, _dp(u), _dp(r), rows, _dp(al), C.byref(o), _dp(out)))
            return self._sq(out)
        xx = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
        if mode == 2 and t_hist is None:
            raise ValueError('sparsity "space" needs t_hist: the weights of the column norm')
        tt = None if t_hist is None else np.ascontiguousarray(t_hist, dtype=np.float64)
        if xx.shape != (self.n,) or (tt is not None and tt.shape != (rows,)):
            raise ValueError(f"x must have {self.n} entries and t_hist {rows}")
        s = np.empty((self.B, rows if mode == 1 else self.n))
        check(self.lib.vch1d_grad_prox_g(self.ctx, _dp(u), _dp(r), rows, _dp(xx), _dp(tt), _dp(al), C.byref(o), mode, _dp(out),
                                         _dp(s)))
        return (self._sq(out), self._sq(s)) if return_scale else self._sq(out)

    def free_energy(self, phi_hist, h=None, w_hist=None, eps=None):
        """Free energy of every level (F1:243-262): phi_hist (B, rows, N+1) -> (B, rows)."""
        ph = self._hist(phi_hist, 0, "phi_hist")
        rows = int(ph.shape[1])
        wh = None if w_hist is None else self._hist(w_hist, rows, "w_hist")
        h = float(self.x[1] - self.x[0]) if h is None else float(h)
        E = np.empty((self.B, rows))
        check(self.lib.vch1d_free_energy(self.ctx, _dp(ph), rows, _dp(wh), h, float(eps or 0.0), _dp(E)))
        return self._sq(E)

    # -- device-resident PGD (G1:333-477) ----------------------------------------------------
    def pgd_init(self, phi0, phi_T, t_hist, dt, opt, phi_Q=None, x=None, u0=None, alpha0=None, sparsity=None):
        """Initial march + targets + J0; t_hist has M+2 entries, dt M.  Returns J0 (B, 5).  `opt`: one parameter object
        for the whole batch or a list / tuple of B (trajectory b runs with opt[b]: weights, sparsity parameter, box and
        alpha_max).  `u0` (B, rows, N+1): start control (taken as given, not clipped; default zeros).  `alpha0` [B] or a
        scalar: first step size, capped at each trajectory's alpha_max (default: alpha_max).  A single `opt` without
        u0 / alpha0 goes through vch1d_pgd_init.  `sparsity`: a name of Engine1D.SPARSITY for the whole batch or a list of
        B names (vch1d_pgd_init_g: the prox, J4 and the KKT statistic of a "time" / "space" trajectory go by rows / columns
        of the control; its box must contain 0); None takes the calls above exactly, every trajectory "full"."""
        phi0, phi_T = self._fld(phi0, "phi0"), self._fld(phi_T, "phi_T_target")
        t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        rows = int(t_hist.size)
        if dt.size != rows - 2:
            raise ValueError(f"dt must have len(t_hist) - 2 = {rows - 2} entries, got {dt.size}")
        pq = None if phi_Q is None else self._hist(phi_Q, rows, "phi_Q_target")
        x = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
        J0 = np.empty((self.B, 5))
        many = isinstance(opt, (list, tuple))
        if sparsity is None and not many and u0 is None and alpha0 is None:
            o = opt if isinstance(opt, OptParams) else make_opt(opt)
            check(self.lib.vch1d_pgd_init(self.ctx, _dp(phi0), _dp(phi_T), _dp(pq), _dp(x), _dp(t_hist), rows, _dp(dt),
                                          C.byref(o), _dp(J0)))
        else:
            seq = list(opt) if many else [opt]
            arr = (OptParams * len(seq))(*[o if isinstance(o, OptParams) else make_opt(o) for o in seq])
            uu = None if u0 is None else self._hist(u0, rows, "u0")
            al = None if alpha0 is None else np.ascontiguousarray(
                np.broadcast_to(np.asarray(alpha0, dtype=np.float64), (self.B,)))
            if sparsity is None:
                check(self.lib.vch1d_pgd_init_v(self.ctx, _dp(phi0), _dp(phi_T), _dp(pq), _dp(x), _dp(t_hist), rows, _dp(dt),
                                                arr, len(seq), _dp(uu), _dp(al), _dp(J0)))
            else:
                names = [sparsity] if isinstance(sparsity, str) else list(sparsity)
                if len(names) not in (1, self.B):
                    raise ValueError(f"sparsity must be one name or {self.B}, got {len(names)}")
                modes = np.array([self._mode(s) for s in names], dtype=np.int32)
                check(self.lib.vch1d_pgd_init_g(self.ctx, _dp(phi0), _dp(phi_T), _dp(pq), _dp(x), _dp(t_hist), rows, _dp(dt),
                                                arr, len(seq), _dp(uu), _dp(al), modes.ctypes.data_as(_lib._I32), len(names),
                                                _dp(J0)))
        self._pgd_rows = rows
        return J0

    def pgd_kkt(self, refresh=True, tol=1e-6):
        """KKT sparsity statistic `u* = 0 <=> |r*| <= kappa_sparsity` of the resident iterate, counted on the device.
        refresh=True recomputes the adjoint of the resident state first; refresh=False takes the resident r (the adjoint of
        the iterate before the last accepted step).  Returns dict(n_zero, n_small, n_match, total: int64 [B]; pct [B][3],
        the three percentages of verify_sparsity_condition; stationarity [B] = ||prox_1(u) - u|| / (||u|| + 1e-9)).
        What is counted depends on the trajectory's sparsity mode (pgd_init): "full" counts nodes, |u| < tol and |r| <=
        kappa_sparsity, total = rows (N+1); "time" counts the rows of the control and "space" its columns, ||u_g|| < tol and
        ||r_g|| <= kappa_sparsity in the group's weighted norm (sum_i wx_i z_i^2 over a row, sum_k wt_k z_k^2 over a
        column), total = rows or N+1; prox_1 is the mode's prox at alpha = 1."""
        cnt = np.zeros((self.B, 4), dtype=np.int64)
        stat = np.empty(self.B)
        check(self.lib.vch1d_pgd_kkt(self.ctx, int(bool(refresh)), float(tol), cnt.ctypes.data_as(C.POINTER(C.c_int64)),
                                     _dp(stat)))
        return dict(n_zero=cnt[:, 0].copy(), n_small=cnt[:, 1].copy(), n_match=cnt[:, 2].copy(), total=cnt[:, 3].copy(),
                    pct=100.0 * cnt[:, :3] / cnt[:, 3:4], stationarity=stat)

    def pgd_iterate(self, n_iters):
        n = int(n_iters)
        cost = np.full((self.B, n), np.nan)
        alpha = np.full((self.B, n), np.nan)
        trials = np.zeros((self.B, n), dtype=np.int32)
        chg = np.full((self.B, n), np.nan)
        sec = np.zeros(3)
        done = check(self.lib.vch1d_pgd_iterate(self.ctx, n, _dp(cost), _dp(alpha), trials.ctypes.data_as(_lib._I32),
                                                _dp(chg), _dp(sec)))
        trk, trm = np.full((self.B, n), np.nan), np.full((self.B, n), np.nan)
        check(self.lib.vch1d_pgd_errors(self.ctx, n, _dp(trk), _dp(trm)))
        return dict(iters=done, cost=cost, alpha=alpha, trials=trials, change=chg, tracking_error=trk, terminal_error=trm,
                    seconds=dict(zip(("backward", "optimistic", "backtracking"), sec)))

    def pgd_get(self, what):
        out = np.empty((self.B, self._pgd_rows, self.n))
        check(self.lib.vch1d_pgd_get(self.ctx, {"u": 0, "phi": 1, "r": 2, "phi_Q": 3}[what], _dp(out)))
        return self._sq(out)

    SECOND_ORDER_KEYS = Engine2D.SECOND_ORDER_KEYS
    RESIDENT = "resident"

    def _base_point(self, t_hist, phi_hist, u, phi_Q, phi_T, dt, x, opt, shared_base):
        """The arguments second_order and hessvec share, checked and as ctypes pointers: (t_hist, rows, n_base,
        [(array kept alive, pointer)] of phi_hist / u / phi_Q / phi_T, dt, x, the OptParams array)."""
        t_hist = np.ascontiguousarray(t_hist, dtype=np.float64)
        rows = int(t_hist.size)
        nb = 1 if shared_base else self.B
        resident = C.cast(C.c_void_p(1), _lib._D)

        def base(a, name, field=False):
            if a is None:
                return None, None
            if isinstance(a, str):
                if a != self.RESIDENT:
                    raise ValueError(f"{name}: expected an array, None or Engine1D.RESIDENT")
                return None, resident
            a = np.ascontiguousarray(a, dtype=np.float64)
            want = (self.n,) if field else (rows, self.n)
            if a.shape == want and nb == 1:
                a = a.reshape((1,) + want)
            if a.shape != (nb,) + want:
                raise ValueError(f"{name} must have shape {(nb,) + want}, got {a.shape}")
            return a, _dp(a)

        if isinstance(phi_hist, str):
            raise ValueError("phi_hist: pass None for the resident history")
        keep = [base(phi_hist, "phi_hist"), base(u, "u"), base(phi_Q, "phi_Q_target"), base(phi_T, "phi_T_target", True)]
        if dt is not None:
            dt = np.ascontiguousarray(dt, dtype=np.float64)
            if dt.shape != (rows - 2,):
                raise ValueError(f"dt must have len(t_hist) - 2 = {rows - 2} entries, got {dt.shape}")
        x = np.ascontiguousarray(self.x if x is None else x, dtype=np.float64)
        if x.shape != (self.n,):
            raise ValueError(f"x must have {self.n} entries")
        seq = list(opt) if isinstance(opt, (list, tuple)) else [opt]
        arr = (OptParams * len(seq))(*[o if isinstance(o, OptParams) else make_opt(o) for o in seq])
        return t_hist, rows, nb, keep, dt, x, arr

    def second_order(self, h, t_hist, opt, phi_hist=None, u=None, phi_Q=None, phi_T=None, dt=None, x=None, order=2,
                     histories=False, shared_base=False):
        """Exact J'(u)h and J''(u)[h,h] of the smooth part J1 + J2 + J3 (vch1d_second_order): one tangent march per
        direction on the device, two linear solves per step, no finite differences and no nonlinear march.
        h: (B, rows, N+1) directions, rows = M + 2 = len(t_hist).  phi_hist None: the resident history (last forward() or
        the PGD iterate).  u / phi_Q / phi_T: arrays, None (zeros) or Engine1D.RESIDENT (the PGD's control / targets).
        shared_base=True: phi_hist, u, phi_Q are (rows, N+1) and phi_T (N+1,), one base point for all B directions (of
        resident arrays, trajectory 0's).  dt None: t_hist[n+2] - t_hist[n+1]; x None: the engine's grid.  opt: one
        parameter object or a sequence of B (only b1, b2, b3 are read).
        Returns a dict of [B] arrays: the six scalars of SECOND_ORDER_KEYS, slope = s_state + s_ctrl, curvature = c_gn +
        c_state + c_ctrl (NaN with order=1), `stats`, and with histories=True dphi, d2phi (B, rows, N+1)."""
        t_hist, rows, nb, keep, dt, x, arr = self._base_point(t_hist, phi_hist, u, phi_Q, phi_T, dt, x, opt, shared_base)
        h = self._hist(h, rows, "h")
        out = np.empty((self.B, 6))
        d1 = np.empty((self.B, rows, self.n)) if histories else None
        d2 = np.empty((self.B, rows, self.n)) if histories else None
        st = Stats()
        check(self.lib.vch1d_second_order(self.ctx, keep[0][1], keep[1][1], nb, _dp(h), rows, _dp(dt), _dp(t_hist), _dp(x),
                                          keep[2][1], keep[3][1], arr, len(arr), int(order), _dp(out), _dp(d1), _dp(d2),
                                          C.byref(st)))
        res = {k: out[:, i].copy() for i, k in enumerate(self.SECOND_ORDER_KEYS)}
        res["slope"] = out[:, 0] + out[:, 1]
        res["curvature"] = (out[:, 2] + out[:, 3]) + out[:, 4]
        res["stats"] = st.as_dict()
        if histories:
            res["dphi"], res["d2phi"] = d1, d2
        return res

    def hessvec(self, h, t_hist, opt, phi_hist=None, u=None, phi_Q=None, phi_T=None, dt=None, x=None, order=2,
                shared_base=False):
        """Exact gradient field and Hessian-vector product of the smooth part J1 + J2 + J3 of the discrete cost
        (vch1d_hessvec): transposed tangent sweeps on the device, one launch, one linear solve per step for the gradient,
        one tangent and two transposed solves per step for H h; no finite differences and no nonlinear march.
        Arguments as for second_order; h may be None with order=1.
        Returns dict(grad, hv: (B, rows, N+1); gh = sum(grad h), hHh = sum(h hv): [B], reduced on the device; stats).
        grad and hv are EUCLIDEAN derivatives with respect to the entries of u, not divided by quadrature weights:
        J'(u)h = sum(grad * h) and J''(u)[h,h] = sum(h * hv) as plain sums (row 0 has quadrature weight 0 and still a
        non-zero gradient; the last row holds its b3 term alone).  With order=1 hv is None and hHh NaN; without h, gh is
        NaN."""
        t_hist, rows, nb, keep, dt, x, arr = self._base_point(t_hist, phi_hist, u, phi_Q, phi_T, dt, x, opt, shared_base)
        h = None if h is None else self._hist(h, rows, "h")
        order = int(order)
        grad = np.empty((self.B, rows, self.n))
        hv = np.empty((self.B, rows, self.n)) if order == 2 else None
        dots = np.empty((self.B, 2))
        st = Stats()
        check(self.lib.vch1d_hessvec(self.ctx, keep[0][1], keep[1][1], nb, _dp(h), rows, _dp(dt), _dp(t_hist), _dp(x),
                                     keep[2][1], keep[3][1], arr, len(arr), order, _dp(grad), _dp(hv), _dp(dots),
                                     C.byref(st)))
        return dict(grad=grad, hv=hv, gh=dots[:, 0].copy(), hHh=dots[:, 1].copy(), stats=st.as_dict())

    def exact_gradient(self, t_hist, opt, phi_hist=None, u=None, phi_Q=None, phi_T=None, dt=None, x=None,
                       shared_base=False):
        """The exact discrete gradient d(J1+J2+J3)/du as a field (B, rows, N+1): hessvec with order=1 and no direction.
        Euclidean, see hessvec; on the run-time physical parameters, unlike the hand-derived adjoint of backward()."""
        return self.hessvec(None, t_hist, opt, phi_hist=phi_hist, u=u, phi_Q=phi_Q, phi_T=phi_T, dt=dt, x=x, order=1,
                            shared_base=shared_base)["grad"]

    def _free_mask(self, mask, rows, nb):
        """A free set as (nb, rows, N+1) bytes (None stays None: built on the device)."""
        if mask is None:
            return None
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape == (rows, self.n) and nb == 1:
            mask = mask.reshape((1,) + mask.shape)
        if mask.shape != (nb, rows, self.n):
            raise ValueError(f"mask must have shape ({nb}, {rows}, {self.n}), got {mask.shape}")
        return mask

    def hess_lanczos(self, q0, k, t_hist, opt, phi_hist=None, u=None, phi_Q=None, phi_T=None, dt=None, x=None, mask=None,
                     tol=0.0, reorth=True, shared_base=False):
        """Lanczos on the reduced Hessian P H P with the basis, the free set and the recurrence on the device
        (vch1d_hess_lanczos); base point and arguments as for hessvec.  q0: (B, rows, N+1) start vectors.  mask: the free
        set as booleans / bytes, (B, rows, N+1), or (rows, N+1) with shared_base=True; None: built on the device from the
        base control `u` and every trajectory's own u_min, u_max of `opt` with `tol` (<= 0: 1e-8).  reorth: full
        reorthogonalisation (k + 1 resident vectors) or the three-term recurrence (3 resident vectors).
        Returns dict(alpha, beta: (B, k), NaN beyond steps; steps, n_free: [B]; stats)."""
        t_hist, rows, nb, keep, dt, x, arr = self._base_point(t_hist, phi_hist, u, phi_Q, phi_T, dt, x, opt, shared_base)
        k = int(k)
        q0 = None if q0 is None else self._hist(q0, rows, "q0")
        mask = self._free_mask(mask, rows, nb)
        kk = max(k, 1)
        alpha, beta = np.full((self.B, kk), np.nan), np.full((self.B, kk), np.nan)
        steps, n_free = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int64)
        st = Stats()
        check(self.lib.vch1d_hess_lanczos(self.ctx, keep[0][1], keep[1][1], nb, rows, _dp(dt), _dp(t_hist), _dp(x), keep[2][1],
                                          keep[3][1], arr, len(arr),
                                          None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), float(tol),
                                          _dp(q0), k, int(reorth), _dp(alpha), _dp(beta), steps.ctypes.data_as(_lib._I32),
                                          n_free.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st)))
        self._kr_rows = rows
        return dict(alpha=alpha, beta=beta, steps=steps, n_free=n_free, stats=st.as_dict())

    def krylov_vector(self, coef):
        """(B, rows, N+1): sum_j coef[b][j] q_j from the basis the last hess_lanczos left resident (vch1d_krylov_vector).
        coef: (B, m), or (m,) with batch 1."""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim == 1 and self.B == 1:
            coef = coef.reshape(1, -1)
        if coef.ndim != 2 or coef.shape[0] != self.B:
            raise ValueError(f"coef must have shape ({self.B}, m), got {coef.shape}")
        out = np.empty((self.B, getattr(self, "_kr_rows", 1), self.n))
        check(self.lib.vch1d_krylov_vector(self.ctx, _dp(coef), int(coef.shape[1]), _dp(out)))
        return out

    CG_STATUS = ("limit", "converged", "negcurv", "breakdown")      # VCH_CG_LIMIT .. VCH_CG_BREAKDOWN

    def hess_cg(self, k, t_hist, opt, rhs=None, cg_tol=0.0, precond=True, mask=None, tol=0.0, phi_hist=None, u=None,
                phi_Q=None, phi_T=None, dt=None, x=None, shared_base=False):
        """(Preconditioned) conjugate gradients on P H P x = P b with x, r, p, the free set and the recurrence on the
        device (vch1d_hess_cg); base point, mask and tol as for hess_lanczos.  rhs: (B, rows, N+1), or None: the Newton
        right-hand side -(grad(J1+J2+J3) + kappa_sparsity wt wx sign(u)) of the full cost on the free set, built on the
        device.  precond: scale by diag(wt' wx), the L2(Q) mass of the control with row 0 taking the time weight of row 1.
        cg_tol: relative residual at which a trajectory stops (<= 0: 1e-8); k: steps at most.
        Returns dict(steps, status (indices of CG_STATUS), n_free: [B]; resid, curv: (B, k), NaN beyond steps (curv[steps]
        is the stopping curvature after "negcurv"); pred: [B] decrease of the quadratic model; rnorm0: [B] ||P b||; stats)."""
        t_hist, rows, nb, keep, dt, x, arr = self._base_point(t_hist, phi_hist, u, phi_Q, phi_T, dt, x, opt, shared_base)
        k = int(k)
        rhs = None if rhs is None else self._hist(rhs, rows, "rhs")
        mask = self._free_mask(mask, rows, nb)
        kk = max(k, 1)
        resid, curv = np.full((self.B, kk), np.nan), np.full((self.B, kk), np.nan)
        pred, rnorm0 = np.full(self.B, np.nan), np.full(self.B, np.nan)
        steps, status, n_free = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int64)
        st = Stats()
        precond = int(precond) if isinstance(precond, (bool, int, np.integer)) else -1
        check(self.lib.vch1d_hess_cg(self.ctx, keep[0][1], keep[1][1], nb, rows, _dp(dt), _dp(t_hist), _dp(x), keep[2][1],
                                     keep[3][1], arr, len(arr),
                                     None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), float(tol),
                                     _dp(rhs), k, float(cg_tol), precond, _dp(resid), _dp(curv), _dp(pred), _dp(rnorm0),
                                     steps.ctypes.data_as(_lib._I32), status.ctypes.data_as(_lib._I32),
                                     n_free.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st)))
        self._cg_rows = rows
        return dict(steps=steps, status=status, n_free=n_free, resid=resid, curv=curv, pred=pred, rnorm0=rnorm0,
                    stats=st.as_dict())

    def cg_vector(self, which="x"):
        """(B, rows, N+1): the solution x, the residual r or the direction p the last hess_cg left resident
        (vch1d_cg_vector); masked-off nodes are exact zeros."""
        if which not in ("x", "r", "p"):
            raise ValueError(f"which must be 'x', 'r' or 'p', got {which!r}")
        out = np.empty((self.B, getattr(self, "_cg_rows", 1), self.n))
        check(self.lib.vch1d_cg_vector(self.ctx, "xrp".index(which), _dp(out)))
        return out

    NEWTON_STATUS = Engine2D.NEWTON_STATUS      # VCH_NEWTON_ACCEPTED .. _IDLE

    def pgd_newton(self, n_rounds, k=50, cg_tol=1e-8, precond=True, tol=0.0, max_halvings=10):
        """Damped Newton rounds on the free set about the resident PGD iterate (vch1d_pgd_newton), every trajectory with
        its own parameters and decisions; no history crosses the bus.  Per round: the Newton-CG step of hess_cg(rhs=None)
        in its resident mode on the free set of the iterate (all rows, the duplicated t = 0 row included), then trials
        clip(u + s x, box) for s = 1, 1/2, ... (a free node whose sign the trial flips is set to 0), at most `max_halvings`
        halvings; the first s with J(trial) <= J(u) - 1e-4 s pred is accepted.  A trajectory ends with "stationary" (zero
        right-hand side or empty free set), "negcurv" (the first CG direction has non-positive curvature), "breakdown" (CG
        broke down: no march is started) or "stalled" (no s accepted) and is "idle" in all later rounds.  A trial whose march
        reports a non-finite mass defect counts as not accepted.  A trajectory that the PGD stop rule ended has its state and
        stored cost brought up to its control first.  Returns the keys of Engine2D.pgd_newton: dict(rounds: rounds run;
        cost, cost_new, s, pred, rnorm0: (B, n_rounds), NaN where idle; halvings, cg_steps, cg_status (indices of
        CG_STATUS), status (indices of NEWTON_STATUS): int32 (B, n_rounds); n_free, pinned, clipped: int64 (B, n_rounds);
        seconds).  pgd_get, hess_cg, ... then work about the new iterate and a following pgd_iterate is that of
        pgd_init(u0 = the Newton iterate)."""
        n = max(int(n_rounds), 1)
        dbl = [np.full((self.B, n), np.nan) for _ in range(5)]
        i32 = [np.zeros((self.B, n), dtype=np.int32) for _ in range(4)]
        cnt = np.zeros((self.B, n, 3), dtype=np.int64)
        sec = np.zeros(4)
        precond = int(precond) if isinstance(precond, (bool, int, np.integer)) else -1
        done = check(self.lib.vch1d_pgd_newton(self.ctx, int(n_rounds), int(k), float(cg_tol), precond, float(tol), int(max_halvings),
                                               *[_dp(a) for a in dbl], *[a.ctypes.data_as(_lib._I32) for a in i32],
                                               cnt.ctypes.data_as(C.POINTER(C.c_int64)), _dp(sec)))
        self._cg_rows = self._pgd_rows
        out = dict(zip(("cost", "cost_new", "s", "pred", "rnorm0"), dbl), rounds=done)
        out.update(zip(("halvings", "cg_steps", "cg_status", "status"), i32))
        out.update(n_free=cnt[:, :, 0].copy(), pinned=cnt[:, :, 1].copy(), clipped=cnt[:, :, 2].copy(),
                   seconds=dict(zip(("solve", "trial", "forward", "cost"), sec)))
        return out

    def newton_trial(self, s, want_u=True):
        """The trial control t = clip(u + s_b x, box_b) of the step lengths `s` ([B] or a scalar, finite and > 0) about the
        base control of the last hess_cg (stateless or resident), with its x, free set and box (vch1d_newton_trial): a free
        node with t u < 0 becomes 0.  Writes only the trial-control scratch.  Returns dict(u: (B, rows, N+1) or None,
        change: (B, 2) = {sum (t - u)^2, sum u^2}, pinned, clipped: int64 [B])."""
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(s, dtype=np.float64), (self.B,)))
        out = np.empty((self.B, getattr(self, "_cg_rows", 1), self.n)) if want_u else None
        chg = np.full((self.B, 2), np.nan)
        cnt = np.zeros((self.B, 2), dtype=np.int64)
        check(self.lib.vch1d_newton_trial(self.ctx, _dp(s), _dp(out), _dp(chg), cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(u=out, change=chg, pinned=cnt[:, 0].copy(), clipped=cnt[:, 1].copy())

    TRUST_CG_STATUS = CG_STATUS + ("boundary",)                     # VCH_CG_LIMIT .. VCH_CG_BOUNDARY
    TRUST_STATUS = NEWTON_STATUS + ("rejected",)                    # VCH_NEWTON_ACCEPTED .. _REJECTED

    def hess_cg_trust(self, k, radius, t_hist, opt, rhs=None, cg_tol=0.0, precond=True, mask=None, tol=0.0, phi_hist=None,
                      u=None, phi_Q=None, phi_T=None, dt=None, x=None, shared_base=False):
        """Truncated (Steihaug-Toint) conjugate gradients on P H P x = P b inside ||x||_D <= radius_b (vch1d_hess_cg_tr):
        hess_cg with a trust region in the preconditioner's norm, ||x||_D^2 = sum D x^2, D = diag(wt' wx) with precond and
        the identity without.  radius: [B] or a scalar, > 0, +inf allowed.  A step that would leave the region, or a
        direction of non-positive curvature, is followed to the boundary: "boundary" and "negcurv" of TRUST_CG_STATUS.
        Returns hess_cg's dict (status: indices of TRUST_CG_STATUS) plus xnorm: [B] ||x||_D by the recurrence.  With
        radius = inf everything equals hess_cg's bit for bit on a trajectory that ends "converged" or "limit".  A radius
        whose square is not finite (>= 2^512) has no boundary and acts as +inf; a radius whose square underflows gives a zero
        step (x = 0 after one counted step)."""
        t_hist, rows, nb, keep, dt, x, arr = self._base_point(t_hist, phi_hist, u, phi_Q, phi_T, dt, x, opt, shared_base)
        k = int(k)
        rhs = None if rhs is None else self._hist(rhs, rows, "rhs")
        mask = self._free_mask(mask, rows, nb)
        radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.B,)))
        kk = max(k, 1)
        resid, curv = np.full((self.B, kk), np.nan), np.full((self.B, kk), np.nan)
        pred, rnorm0, xnorm = np.full(self.B, np.nan), np.full(self.B, np.nan), np.full(self.B, np.nan)
        steps, status, n_free = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int64)
        st = Stats()
        precond = int(precond) if isinstance(precond, (bool, int, np.integer)) else -1
        check(self.lib.vch1d_hess_cg_tr(self.ctx, keep[0][1], keep[1][1], nb, rows, _dp(dt), _dp(t_hist), _dp(x), keep[2][1],
                                        keep[3][1], arr, len(arr),
                                        None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), float(tol),
                                        _dp(rhs), k, float(cg_tol), precond, _dp(resid), _dp(curv), _dp(pred), _dp(rnorm0),
                                        steps.ctypes.data_as(_lib._I32), status.ctypes.data_as(_lib._I32),
                                        n_free.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st), _dp(radius), _dp(xnorm)))
        self._cg_rows = rows
        return dict(steps=steps, status=status, n_free=n_free, resid=resid, curv=curv, pred=pred, rnorm0=rnorm0, xnorm=xnorm,
                    stats=st.as_dict())

    def pgd_trust(self, n_rounds, radius0, k=50, cg_tol=1e-8, precond=True, tol=0.0, radius_max=None, radius_min=None):
        """Trust-region (Steihaug) Newton-CG rounds on the free set about the resident PGD iterate (vch1d_pgd_trust), every
        trajectory with its own parameters, radius and decisions.  Per round: the step of hess_cg_trust in its resident mode
        inside the trajectory's radius (a direction of non-positive curvature is followed to the boundary and does not end
        the trajectory), one trial clip(u + x, box) as newton_trial(1) builds it, rho = (J(u) - J(trial)) / pred.  The trial
        is accepted iff J(trial) is finite and <= J(u) - 1e-4 pred; otherwise the trajectory stays unmoved, "rejected", and
        goes on.  The radius: rho < 1/4 or not finite: min(radius, ||x||_D) / 4; else rho > 3/4 after a "boundary" or
        "negcurv" exit: min(2 radius, radius_max).  A trajectory ends "stationary", "breakdown", or "stalled" (rejected with
        the radius below radius_min) and is "idle" afterwards.  radius0: [B] or a scalar, finite and > 0; radius_max /
        radius_min default to 1024 max(radius0) and 1e-10 min(radius0).  Returns dict(rounds; cost, cost_new, pred, rnorm0,
        radius (the round's), ratio, xnorm: (B, n_rounds), NaN where idle; cg_steps, cg_status (indices of TRUST_CG_STATUS),
        status (indices of TRUST_STATUS): int32 (B, n_rounds); n_free, pinned, clipped: int64 (B, n_rounds); seconds)."""
        n = max(int(n_rounds), 1)
        radius0 = np.ascontiguousarray(np.broadcast_to(np.asarray(radius0, dtype=np.float64), (self.B,)))
        radius_max = 1024.0 * float(np.max(radius0)) if radius_max is None else float(radius_max)
        radius_min = 1e-10 * float(np.min(radius0)) if radius_min is None else float(radius_min)
        dbl = [np.full((self.B, n), np.nan) for _ in range(7)]
        i32 = [np.zeros((self.B, n), dtype=np.int32) for _ in range(3)]
        cnt = np.zeros((self.B, n, 3), dtype=np.int64)
        sec = np.zeros(4)
        precond = int(precond) if isinstance(precond, (bool, int, np.integer)) else -1
        done = check(self.lib.vch1d_pgd_trust(self.ctx, int(n_rounds), int(k), float(cg_tol), precond, float(tol), _dp(radius0),
                                              radius_max, radius_min, *[_dp(a) for a in dbl],
                                              *[a.ctypes.data_as(_lib._I32) for a in i32],
                                              cnt.ctypes.data_as(C.POINTER(C.c_int64)), _dp(sec)))
        self._cg_rows = self._pgd_rows
        out = dict(zip(("cost", "cost_new", "pred", "rnorm0", "radius", "ratio", "xnorm"), dbl), rounds=done)
        out.update(zip(("cg_steps", "cg_status", "status"), i32))
        out.update(n_free=cnt[:, :, 0].copy(), pinned=cnt[:, :, 1].copy(), clipped=cnt[:, :, 2].copy(),
                   seconds=dict(zip(("solve", "trial", "forward", "cost"), sec)))
        return out
