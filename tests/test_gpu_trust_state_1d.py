"""vch1d_hess_cg_tr / vch1d_pgd_trust on a context that has just done something else, and the branches of the radius rule that
tests/test_gpu_trust_1d.py does not reach through the engine.

A. Call order.  The six [B] cells of k1d_ncg_fin_tr (radius, xx, xp, pp, c, the pending exit) live in coef2 and ucoef of the
   Lanczos block, which vch1d_krylov_vector writes and a Lanczos call with re-orthogonalisation sizes; the trial kernel
   writes the step lengths, the trial control and the cost partials the PGD loop also uses.  Every sequence below ends in a
   call whose every output is compared bit for bit with the same call on a fresh context that holds the same problem, on the
   driver (one chunk, batch 1) and on n2051 at batch 2 (three chunks, depth 2, a batch stride).
B. The radius rule: STALLED through radius_min and IDLE after it, the cap radius_max binding, and a kept radius, each in a
   batch of three beside a member that goes on being accepted and a stationary one, against three single contexts bit for
   bit.  Every live member's radius sequence is replayed from the record with tests/_trust_ref.judge: radius[r + 1] is
   exactly what `judge` gives from radius[r], ratio[r], xnorm[r] and cg_status[r], and the status is `judge`'s for the trial
   cost (cost_new where accepted, cost - ratio pred otherwise).

Everything asserted here is an equality of bits or of decisions; there is no tolerance."""
import numpy as np
import pytest

from _cg_ref import CONVERGED, NEGCURV
from _trust_ref import BOUNDARY, replay
from test_gpu_hess_cg_1d import KEYS as CG_KEYS, _block, _cg, _mass, _negative_b3, refine          # noqa: F401 (fixture)
from test_gpu_krylov_1d import V, _q0, _tile, driver, small                                          # noqa: F401 (fixtures)
from test_gpu_newton_1d import OUT_KEYS as NEWTON_KEYS, PGD_KEYS, _pgd, _refine_case
from test_gpu_trust_1d import (ACCEPTED, IDLE, NT_NEGCURV, OUT_KEYS, REJECTED, STALLED, STATIONARY, TR_KEYS, _dnorm, _members,
                               _radius_of, _tr, _vectors)
from test_gpu_trust_2d import _radius_for_exit_at

pytestmark = pytest.mark.gpu

CASES = ["driver", "n2051 x 2"]


def _case(request, small, case):
    """(problem, the nb of Problem.kw, batch)."""
    return (request.getfixturevalue("driver"), 0, 1) if case == "driver" else (small("n2051"), 2, 2)


def _same_call(got, Vg, want, Vw, keys=TR_KEYS):
    for key in keys:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    for w, a, c in zip("xrp", Vg, Vw):
        assert np.array_equal(a, c), w


def _exit_radius(pr, b, j):
    Df = _mass(pr).ravel()[pr.free]
    return np.array([_radius_for_exit_at(_block(pr), bi.ravel()[pr.free], j, Df) for bi in b])


# ---------------------------------------------------------------------------------------------------------------------
# A1 - A3. the step after other Krylov calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_a_trust_step_after_lanczos_and_krylov_vector(request, small, case):
    pr, nb, B = _case(request, small, case)
    b = _q0((B,) + pr.shape, 51)
    radius = _exit_radius(pr, b, 3)
    k = 4 * len(pr.free)
    mask = _tile(pr.mask, nb) if nb else pr.mask
    call = lambda e: _tr(pr, e, k, radius, nb=nb, rhs=b, cg_tol=1e-8, mask=mask)
    fresh = pr.context(B)
    want = call(fresh)
    Vw = _vectors(fresh)
    fresh.close()
    eng = pr.context(B)
    L = eng.hess_lanczos(_q0((B,) + pr.shape, 52), 8, pr.t, pr.opt, mask=mask, reorth=True, **pr.kw(nb))
    coef = np.random.default_rng(53).standard_normal((B, 6))
    Q = eng.krylov_vector(coef)                                      # writes ucoef, where three of the cells live
    got = call(eng)
    Vg = _vectors(eng)
    with pytest.raises(pr.V.VchError, match="-3"):                   # the Lanczos basis is gone
        eng.krylov_vector(coef)
    eng.close()
    print(f"MEASURE A1 {case}: lanczos steps {list(L['steps'])}; trust status {list(got['status'])} steps {list(got['steps'])}")
    assert (L["steps"] == 8).all() and np.abs(Q).max() > 0
    assert (want["status"] == BOUNDARY).all() and (want["steps"] == 3).all()
    _same_call(got, Vg, want, Vw)


@pytest.mark.parametrize("case", CASES)
def test_hess_cg_and_an_infinite_radius_after_a_pending_boundary_exit(request, small, case):
    pr, nb, B = _case(request, small, case)
    b = _q0((B,) + pr.shape, 54)
    k = 400 if case == "driver" else 48
    mask = _tile(pr.mask, nb) if nb else pr.mask
    kw = dict(nb=nb, rhs=b, cg_tol=1e-8, mask=mask)
    fresh = pr.context(B)
    want = _cg(pr, fresh, k, **kw)
    Vw = _vectors(fresh)
    fresh.close()
    eng = pr.context(B)
    first = _tr(pr, eng, k, _exit_radius(pr, b, 1), **kw)            # leaves xx, xp and the pending cell set
    got = _cg(pr, eng, k, **kw)
    Vg = _vectors(eng)
    inf = _tr(pr, eng, k, np.inf, **kw)
    Vi = _vectors(eng)
    eng.close()
    print(f"MEASURE A2 {case}: boundary call status {list(first['status'])} steps {list(first['steps'])}; hess_cg steps {list(want['steps'])}")
    assert (first["status"] == BOUNDARY).all() and (first["steps"] == 1).all()
    assert (want["status"] == CONVERGED).all() and (want["steps"] > 1).all()
    _same_call(got, Vg, want, Vw, CG_KEYS)
    _same_call(inf, Vi, want, Vw, CG_KEYS)
    assert np.isfinite(inf["xnorm"]).all() and (inf["xnorm"] > 0).all()


@pytest.mark.parametrize("case", CASES)
def test_an_interior_solve_after_a_negative_curvature_exit(request, small, case):
    pr, nb, B = _case(request, small, case)
    b = _q0((B,) + pr.shape, 55)
    k = 4 * len(pr.free)
    mask = _tile(pr.mask, nb) if nb else pr.mask
    neg = pr.mask.copy()
    neg[0] = False                                                   # row 0 is not shifted by b3: left out, the block is negative definite
    neg = _tile(neg, nb) if nb else neg
    neg_opt = pr.V.make_opt(pr.opt, b3=_negative_b3(pr))
    # member 0 converges inside ten times its Newton step's norm, a second member leaves its region at step 2
    D = _mass(pr).ravel()[pr.free]
    xs = np.linalg.solve(_block(pr), b[0].ravel()[pr.free])
    radius = np.array([10.0 * float(np.sqrt(np.sum(D * xs * xs)))] + list(_exit_radius(pr, b[1:], 2)))
    call = lambda e: _tr(pr, e, k, radius, nb=nb, rhs=b, cg_tol=1e-8, mask=mask)
    fresh = pr.context(B)
    want = call(fresh)
    Vw = _vectors(fresh)
    fresh.close()
    eng = pr.context(B)
    first = _tr(pr, eng, 5, np.array([0.75, 0.5][:B]), nb=nb, rhs=b, mask=neg, opt=neg_opt)
    got = call(eng)
    Vg = _vectors(eng)
    eng.close()
    print(f"MEASURE A3 {case}: first call status {list(first['status'])} steps {list(first['steps'])}; second status {list(got['status'])} "
          f"steps {list(got['steps'])}")
    assert (first["status"] == NEGCURV).all() and (first["steps"] == 1).all()
    assert list(want["status"]) == [CONVERGED, BOUNDARY][:B] and want["xnorm"][0] < radius[0] and (B == 1 or want["steps"][1] == 2)
    _same_call(got, Vg, want, Vw)


# ---------------------------------------------------------------------------------------------------------------------
# A4 - A6. the rounds and the PGD loop on one context
# ---------------------------------------------------------------------------------------------------------------------
def _same_pgd(got, want):
    assert got["iters"] == want["iters"]
    for key in PGD_KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key


def test_iterations_after_an_accepting_call_are_those_of_an_init_at_its_iterate(refine):
    """The member the feature is for (negative curvature at the first direction), two accepted rounds, then two PGD
    iterations: those of pgd_init(u0 = the accepted iterate, alpha0 = the step length the run carried), as
    test_gpu_newton_1d.py continues the damped rounds.  The run starts with alpha0 = 1e-3, not the default, and takes no PGD
    step before the rounds: the carried step length is 1e-3 exactly if the rounds leave it alone, which the first
    iteration's `alpha` and `trials` then show (from the default alpha_max they differ)."""
    pr = refine
    opts, u0, radius0 = _members(pr)
    opt, u, r0 = opts[2], u0[2], radius0[2]
    eng = _pgd(pr, [opt], u[None], alpha0=1e-3)
    eng.pgd_kkt(refresh=True)
    eng.pgd_kkt(refresh=False)                           # the adjoint of the start is resident and valid
    R = eng.pgd_trust(2, r0)
    assert R["status"][0].tolist() == [ACCEPTED, ACCEPTED] and R["cg_status"][0, 0] == NEGCURV
    with pytest.raises(pr.V.VchError, match="-3"):       # vch1d_pgd_trust cleared pgd_r_valid with the move
        eng.pgd_kkt(refresh=False)
    un, phin = eng.pgd_get("u"), eng.pgd_get("phi")
    assert not np.array_equal(un, u)
    got = eng.pgd_iterate(2)
    u_got, phi_got = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    ref = _pgd(pr, [opt], un[None], alpha0=1e-3)
    assert np.array_equal(ref.pgd_get("phi"), phin)
    want = ref.pgd_iterate(2)
    _same_pgd(got, want)
    other = _pgd(pr, [opt], un[None])                  # the premise: from the default step length the iteration differs
    assert not np.array_equal(other.pgd_iterate(1)["alpha"], want["alpha"][:, :1])
    other.close()
    assert np.array_equal(ref.pgd_get("u"), u_got) and np.array_equal(ref.pgd_get("phi"), phi_got)
    ref.close()


def _outside(pr):
    """The member of DESIGN.md 10k with nodes outside its box under the negative b3: every trial clips them whatever the
    radius, which raises the cost by an amount that does not shrink with it; every round is rejected."""
    opts, _, radius0 = _members(pr)
    assert (np.abs(pr.u) > 0.9).any()
    return opts[2], pr.u, radius0[2]


def test_a_call_that_accepts_nothing_leaves_the_pgd_run_undisturbed(refine):
    """Member 0 is stationary (empty free set), member 1 is rejected: nothing moves, and the iteration that follows is that of
    a run without the call."""
    pr = refine
    opts_m, _, _ = _members(pr)
    out, u_out, r_out = _outside(pr)
    opts, u0 = [opts_m[1], out], np.stack([np.zeros_like(pr.u), u_out])
    plain = _pgd(pr, opts, u0)
    want = plain.pgd_iterate(1)
    u_want, phi_want = plain.pgd_get("u"), plain.pgd_get("phi")
    plain.close()
    eng = _pgd(pr, opts, u0)
    phi0 = eng.pgd_get("phi")
    R = eng.pgd_trust(1, np.array([1.0, r_out]))
    print(f"MEASURE A5: status {R['status'][:, 0].tolist()} ratio {R['ratio'][:, 0].tolist()} clipped {R['clipped'][:, 0].tolist()}")
    assert R["rounds"] == 1 and R["status"][:, 0].tolist() == [STATIONARY, REJECTED]
    assert np.array_equal(R["cost"][:, 0], R["cost_new"][:, 0]) and R["clipped"][1, 0] > 0
    assert np.array_equal(eng.pgd_get("u"), u0) and np.array_equal(eng.pgd_get("phi"), phi0)
    got = eng.pgd_iterate(1)
    _same_pgd(got, want)
    assert np.array_equal(eng.pgd_get("u"), u_want) and np.array_equal(eng.pgd_get("phi"), phi_want)
    eng.pgd_kkt(refresh=False)                           # nothing moved: the iteration's adjoint is the resident one
    eng.close()


def test_trust_newton_trust_on_one_context_equal_fresh_contexts(refine):
    """pgd_trust(1), pgd_newton(1), pgd_trust(1) on one context at batch 2, each against a fresh context started from the
    iterate before it: the trial's step lengths, control and cost partials of one kind of round are not seen by the other."""
    pr = refine
    opts_m, u0_m, rad_m = _members(pr)
    opts, state, rad = [opts_m[0], opts_m[2]], np.stack([u0_m[0], u0_m[2]]), rad_m[[0, 2]]
    run = dict(trust=lambda e, r: e.pgd_trust(1, r), newton=lambda e, r: e.pgd_newton(1))
    eng = _pgd(pr, opts, state)
    seen = []
    for kind, r in (("trust", rad), ("newton", None), ("trust", 2.0 * rad)):
        got = run[kind](eng, r)
        Ug, Pg = eng.pgd_get("u"), eng.pgd_get("phi")
        fresh = _pgd(pr, opts, state)
        want = run[kind](fresh, r)
        Uw, Pw = fresh.pgd_get("u"), fresh.pgd_get("phi")
        fresh.close()
        for key in (OUT_KEYS if kind == "trust" else NEWTON_KEYS):
            assert np.array_equal(got[key], want[key], equal_nan=True), (kind, key)
        assert np.array_equal(Ug, Uw) and np.array_equal(Pg, Pw), kind
        assert not np.array_equal(Ug[0], state[0])
        seen.append(got["status"][:, 0].tolist())
        state = Ug
    eng.close()
    print(f"MEASURE A6: statuses {seen}")
    assert seen[0] == [ACCEPTED, ACCEPTED] and seen[1] == [ACCEPTED, NT_NEGCURV] and seen[2][1] == ACCEPTED


def test_a_step_and_a_trial_between_two_iterations_leave_the_run_undisturbed(refine):
    pr = refine
    _, box, u0 = _refine_case(pr)
    plain = _pgd(pr, [box], u0[None], alpha0=1e-3)       # a short first step: the iterate keeps a free set
    plain.pgd_iterate(1)
    want = plain.pgd_iterate(1)
    u_want, phi_want = plain.pgd_get("u"), plain.pgd_get("phi")
    plain.close()
    eng = _pgd(pr, [box], u0[None], alpha0=1e-3)
    eng.pgd_iterate(1)
    u1 = eng.pgd_get("u")
    R = eng.RESIDENT
    S = eng.hess_cg_trust(6, 0.05 * _dnorm(pr, u1, True), pr.t, box, u=R, phi_Q=R, phi_T=R, dt=pr.dts, x=pr.x)
    T = eng.newton_trial(0.5)                            # writes alpha_dev, u_trial and cost_part, which the loop also uses
    assert S["status"][0] == BOUNDARY and S["n_free"][0] > 0 and not np.array_equal(T["u"][0], u1)
    got = eng.pgd_iterate(1)
    _same_pgd(got, want)
    assert np.array_equal(eng.pgd_get("u"), u_want) and np.array_equal(eng.pgd_get("phi"), phi_want)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# B. the remaining branches of the radius rule
# ---------------------------------------------------------------------------------------------------------------------
def _batch_and_singles(pr, opts, u0, n_rounds, radius0, k=50, **lim):
    eng = _pgd(pr, opts, u0)
    many = eng.pgd_trust(n_rounds, radius0, k=k, **lim)
    Um, Pm = eng.pgd_get("u"), eng.pgd_get("phi")
    eng.close()
    print(f"MEASURE B: status {many['status'].tolist()} cg {many['cg_status'].tolist()} in {many['cg_steps'].tolist()} radius "
          f"{many['radius'].tolist()} xnorm {many['xnorm'].tolist()} ratio {many['ratio'].tolist()} cost {many['cost'].tolist()} -> "
          f"{many['cost_new'].tolist()} limits {lim}")
    for i in range(len(opts)):
        one = _pgd(pr, [opts[i]], u0[i][None])
        got = one.pgd_trust(n_rounds, radius0[i], k=k, **lim)
        U1, P1 = one.pgd_get("u"), one.pgd_get("phi")
        one.close()
        for key in OUT_KEYS:
            assert np.array_equal(got[key][0], many[key][i], equal_nan=True), (key, i)
        assert np.array_equal(U1, Um[i]) and np.array_equal(P1, Pm[i]), i
        replay(many, i, lim["radius_max"], lim["radius_min"])
    return many, Um


def test_stalled_through_radius_min_then_idle(refine):
    """A rejection leaves at most a quarter of the radius, so with radius_min = radius0 / 10 the first round is REJECTED and
    the second STALLED, whatever ||x||_D is.  The ended member's solves go on ungated at its radius0 and its trial slots
    are frozen: the members beside it have the bits of their own contexts."""
    pr = refine
    opts_m, u0_m, rad_m = _members(pr)
    out, u_out, r_out = _outside(pr)
    opts, u0 = [out, opts_m[0], opts_m[1]], np.stack([u_out, u0_m[0], u0_m[1]])
    radius0 = np.array([r_out, rad_m[0], rad_m[1]])
    many, Um = _batch_and_singles(pr, opts, u0, 4, radius0, radius_max=1024.0 * float(radius0.max()), radius_min=r_out / 10.0)
    assert many["rounds"] == 4
    assert many["status"][0].tolist() == [REJECTED, STALLED, IDLE, IDLE]
    assert np.array_equal(Um[0].view(np.int64), u_out.view(np.int64))
    assert many["radius"][0, 1] <= 0.25 * r_out and many["radius"][0, 1] >= r_out / 10.0
    assert np.isnan(many["cost"][0, 2:]).all() and np.isnan(many["radius"][0, 2:]).all()
    assert many["status"][1].tolist() == [ACCEPTED] * 4 and many["status"][2].tolist() == [STATIONARY] + [IDLE] * 3


def test_the_radius_cap_binds(refine):
    """The member the feature is for (rho > 3/4 after NEGCURV exits, the radius doubling every round) under
    radius_max = 2 radius0."""
    pr = refine
    opts_m, u0_m, rad_m = _members(pr)
    r = float(rad_m[2])
    opts, u0 = [opts_m[2], opts_m[0], opts_m[1]], np.stack([u0_m[2], u0_m[0], u0_m[1]])
    many, _ = _batch_and_singles(pr, opts, u0, 4, np.array([r, r, r]), radius_max=2.0 * r, radius_min=1e-10 * r)
    bound = [q for q in range(3) if many["ratio"][0, q] > 0.75 and many["cg_status"][0, q] in (BOUNDARY, NEGCURV)
             and many["radius"][0, q] == 2.0 * r == many["radius"][0, q + 1]]
    print(f"MEASURE B cap: the cap bound in rounds {bound}")
    assert bound and many["radius"][0, 0] == r and (many["radius"][:2] <= 2.0 * r).all()
    assert many["status"][0].tolist() == [ACCEPTED] * 4 and (many["status"][1] != IDLE).all()


def test_the_radius_is_kept_after_an_interior_solve_and_in_the_middle_band(refine):
    """A ratio above 3/4 after an interior convergence does not double the radius, and a ratio in [1/4, 3/4] keeps it after
    any exit.  From ten times ||u||_D (k = 200) the first solve of member 0 still ends on the boundary with rho = 0.135 and the
    radius is quartered; its solves of rounds 1 and 2 converge inside.  (From a thousand times ||u||_D the first solve does
    converge inside, but its clipped trial has rho = 0.018 and the radius shrinks: no first radius gives this member an
    interior first solve that keeps it.)  Member 1, the same problem in a twentieth of ||u||_D, has rho = 0.68 in round 3."""
    pr = refine
    opts_m, u0_m, rad_m = _members(pr)
    opts, u0 = [opts_m[0], opts_m[0], opts_m[1]], np.stack([u0_m[0], u0_m[0], u0_m[1]])
    radius0 = np.array([_radius_of(pr, 10.0), rad_m[0], rad_m[1]])
    n = 5
    many, _ = _batch_and_singles(pr, opts, u0, n, radius0, k=200, radius_max=1024.0 * float(radius0.max()),
                                 radius_min=1e-10 * float(radius0.min()))
    kept = []
    for i in range(2):
        for r in range(n - 1):
            if many["status"][i, r] in (IDLE, STATIONARY) or many["status"][i, r + 1] == IDLE:
                continue
            rho, cgs = many["ratio"][i, r], many["cg_status"][i, r]
            branch = "middle" if 0.25 <= rho <= 0.75 else "interior" if rho > 0.75 and cgs == CONVERGED else None
            if branch:
                kept.append((i, r, branch))
                assert many["radius"][i, r + 1] == many["radius"][i, r], (i, r, branch)
    print(f"MEASURE B kept: (member, round, branch) {kept}")
    assert many["cg_status"][0, 1] == CONVERGED and many["xnorm"][0, 1] < many["radius"][0, 1]
    assert (0, 1, "interior") in kept and (1, 3, "middle") in kept
