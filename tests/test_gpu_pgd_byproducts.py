"""The three by-products of every accepted iteration of the device-resident 2D PGD loop -- `change` (the input of the stop
rule), `tracking_error` and `terminal_error` (what the drivers report and save) -- against a long-double restatement
(tests/_pgd_byproducts_ref.py) of the oracle's formulas applied to the fields pulled from the engine after every call.

The goldens pin them on 16 x 16 with Lx = Ly, uniform steps and one trajectory, where a swapped hx / hy, padding counted
in a sum, a uniform-dt trapezoid, a fallback or a weight taken from trajectory 0 and the sums of the optimistic candidate
reported for a backtracked step all go unseen.  Here: 70 x 20 and 20 x 70 (ragged tiles on both axes, hx != hy) next to
the 16 x 16 control, six time steps of which the last is half as long, and a batch of five with one parameter set and one
target set per member:
  a  defaults, ramp target
  b  b1 = 0, b2 = 4: the tracking error is still reported (the raw sums do not see the weights)
  c  phi_Q = 0: the RMS fallback of the tracking denominator, for this member only
  d  alpha_max = 4e4: the line search backtracks and returns its last try; `change` is the accepted candidate's
  e  kappa_sparsity = 10: u = 0 is the fixed point, ten backtracking marches, change == 0.0 exactly; phi_T = 0, so the
     terminal denominator is the bare 1e-12 guard

Tolerance: engine and restatement sum the same non-negative terms in another order, so each is within nodes * EPS relative
of the exact sum, nodes = (M+1)(Nx+1)(Ny+1), EPS = 2^-52 (the bound tests/test_gpu_newton_2d.py uses for the change sums);
the square roots halve that and the few operations after them add a few EPS, so nodes * EPS bounds the gap of the ratios too.
Zero is compared exactly.  Measured gaps: profiles/pgd_byproducts.txt.
"""
import numpy as np
import pytest

import _pgd_byproducts_ref as R

pytestmark = pytest.mark.gpu

DT, T = 1e-2, 0.055
GRIDS = [(70, 20, 1.3, 0.9), (20, 70, 0.9, 1.3), (16, 16, 1.0, 1.0)]
gid = lambda g: f"{g[0]}x{g[1]}"
NAMES = ("a", "b", "c", "d", "e")
SEEDS = (42, 43, 44, 45, 46)
CALLS = 4
KEYS = ("cost", "alpha", "attempts", "change", "tracking_error", "terminal_error")


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O2():
    from oracle import vch2d_oracle
    return vch2d_oracle


def _opts(O2):
    return [O2.OptParams(), O2.OptParams(b1=0.0, b2=4.0), O2.OptParams(), O2.OptParams(alpha_max=4e4),
            O2.OptParams(kappa_sparsity=10.0)]


def _problem(O2, V, g, seeds=SEEDS, names=NAMES):
    """phi0, phi_T (B, ..), phi_Q (B, M+1, ..), t, x, y and the parameter sets of the members `names`."""
    Nx, Ny, Lx, Ly = g
    t, dts = V.time_grid(T, DT)
    assert t.size == 7 and abs(dts[-1] - 0.5 * DT) < 1e-12 and abs(dts[0] - DT) < 1e-18      # six steps, the last 0.005
    x, y = np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1)
    by_name = dict(zip(NAMES, _opts(O2)))
    phi0, phi_T, phi_Q = [], [], []
    for name, seed in zip(names, seeds):
        p0 = O2.init_phi_random(Nx, Ny, 1e-2, amp=0.1, seed=seed)
        pT, pQ = O2.build_targets(x, y, t, p0, Lx, Ly, T)
        if name == "e":
            pT = np.zeros_like(pT)
            pQ = (1.0 - t / T)[:, None, None] * p0                          # the ramp towards the zero target
        if name == "c":
            pQ = np.zeros_like(pQ)
        phi0.append(p0), phi_T.append(pT), phi_Q.append(pQ)
    return dict(g=g, t=t, x=x, y=y, names=list(names), phi0=np.stack(phi0), phi_T=np.stack(phi_T), phi_Q=np.stack(phi_Q),
                opts=[by_name[n] for n in names])


def _run(V, prob, members, calls, pull=False):
    """The members `members` of prob as one batch: pgd_init, then pgd_iterate(n) for n in calls.  -> the outputs of every
    call, joined along the iteration axis, and with pull=True the (u, phi, phi_Q, r) pulled after pgd_init and after every
    call (r: the adjoint the call's last iteration started from; not yet computed after pgd_init)."""
    Nx, Ny, Lx, Ly = prob["g"]
    B = len(members)
    e = V.Engine2D(Nx=Nx, Ny=Ny, Lx=Lx, Ly=Ly, batch=B, max_steps=prob["t"].size - 1)
    try:
        sel = lambda a: np.ascontiguousarray(a[list(members)])
        e.pgd_init(sel(prob["phi0"]), sel(prob["phi_T"]), prob["t"], [V.make_opt(prob["opts"][m]) for m in members],
                   phi_Q=sel(prob["phi_Q"]), ramp=False, T=T)
        get = lambda: tuple(np.array(e.pgd_get(k)).reshape((B, prob["t"].size, Nx + 1, Ny + 1)) for k in ("u", "phi", "phi_Q", "r"))
        pulls = [get()] if pull else []
        outs = []
        for n in calls:
            outs.append(e.pgd_iterate(n))
            if pull:
                pulls.append(get())
    finally:
        e.close()
    out = {k: np.concatenate([o[k] for o in outs], axis=1) for k in KEYS}
    out["iters"] = [o["iters"] for o in outs]
    return out, pulls


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()                # NaN == NaN, -0.0 != 0.0


@pytest.fixture(scope="module")
def runs(V, O2):
    """grid -> the batch of five iterated CALLS times one iteration at a time, with the pulls; computed once per grid."""
    done = {}

    def get(g):
        if g not in done:
            prob = _problem(O2, V, g)
            out, pulls = _run(V, prob, range(5), [1] * CALLS, pull=True)
            done[g] = (prob, out, pulls)
        return done[g]
    return get


@pytest.mark.parametrize("g", GRIDS, ids=gid)
def test_byproducts_against_the_restatement(runs, O2, g):
    """change, tracking_error and terminal_error of every call and member within nodes * EPS of the restatement on the
    pulled fields; the batch qualifies: in one iteration a member backtracks while another accepts its optimistic step,
    member d backtracks to a step with change != 0 that the optimistic candidate (rebuilt from the pulled adjoint) does
    not share, member c takes the RMS fallback and member a does not (decided from the restatement's own den and rms),
    member e's terminal target norm is zero."""
    prob, out, pulls = runs(g)
    Nx, Ny = g[:2]
    nodes = prob["t"].size * (Nx + 1) * (Ny + 1)
    bound = nodes * R.EPS
    assert out["iters"] == [1] * CALLS and not np.isnan(np.concatenate([out[k] for k in KEYS], axis=1)).any()
    att = out["attempts"]
    print(f"attempts {gid(g)}: {att.tolist()}")
    assert any(att[:, k].max() > 0 and att[:, k].min() == 0 for k in range(CALLS)), att
    assert np.all(att[0] == 0) and np.all(att[4] == 10), att
    kd = [k for k in range(CALLS) if att[3, k] > 0 and att[0, k] == 0]
    assert kd and all(out["change"][3, k] > 0.0 for k in kd), (att, out["change"][3])
    worst, away_d = {}, []
    for k in range(CALLS):
        u_old, (u, phi, pq, r) = pulls[k][0], pulls[k + 1]
        assert np.array_equal(pq, prob["phi_Q"])
        if k in kd:
            # what the optimistic candidate's sums would have given: its step is alpha_prev = min(alpha_max, 1.2 alpha_{k-1})
            # (no plateau boost before the fifth iteration), the adjoint is the one the iteration started from
            o = prob["opts"][3]
            a_prev = o.alpha_max if k == 0 else min(o.alpha_max, 1.2 * out["alpha"][3, k - 1])
            u_opt = O2.prox_step(u_old[3], O2.gradient(r[3], u_old[3], o), a_prev, o)
            away_d.append(R.gap(out["change"][3, k], R.change(u_opt, u_old[3])))
            print(f"MEASURE 2d {gid(g)} it {k} member d: change of the optimistic candidate is {away_d[-1]:.2e} away")
        for b, name in enumerate(NAMES):
            parts = R.errors_2d_parts(phi[b], pq[b], prob["phi_T"][b], prob["x"], prob["y"], prob["t"])
            assert parts["fallback"] == (name == "c"), (name, parts)
            assert (parts["den_T"] == 0.0) == (name == "e"), (name, parts)
            ref = dict(change=R.change(u[b], u_old[b]), tracking_error=parts["track"], terminal_error=parts["term"])
            gaps = {key: R.gap(out[key][b, k], ref[key]) for key in ref}
            print(f"MEASURE 2d {gid(g)} it {k} member {name}: attempts {att[b, k]} change {out['change'][b, k]:.6e} gap "
                  f"{gaps['change']:.2e} tracking {out['tracking_error'][b, k]:.6e} gap {gaps['tracking_error']:.2e} terminal "
                  f"{out['terminal_error'][b, k]:.6e} gap {gaps['terminal_error']:.2e} (nodes * EPS {bound:.2e})")
            for key, gp in gaps.items():
                worst[key] = max(worst.get(key, 0.0), gp)
                assert gp <= bound, (gid(g), k, name, key, out[key][b, k], ref[key], gp, bound)
            if name == "e":
                assert out["change"][b, k] == 0.0 and not u[b].any()
    print(f"MEASURE 2d {gid(g)} worst: " + " ".join(f"{key} {v:.2e}" for key, v in worst.items()) + f" (nodes * EPS {bound:.2e})")
    assert max(away_d) > 100.0 * bound, (away_d, bound)                  # the sums of the optimistic candidate would not pass


@pytest.mark.parametrize("g", GRIDS, ids=gid)
def test_one_call_against_many(V, runs, g):
    """pgd_iterate(4) on a fresh engine: all six outputs have the bits of four calls of one iteration."""
    prob, out, _ = runs(g)
    one, _ = _run(V, prob, range(5), [CALLS])
    assert one["iters"] == [CALLS]
    for key in KEYS:
        assert _same_bits(one[key], out[key]), (key, one[key], out[key])


@pytest.mark.parametrize("b", range(5), ids=NAMES)
def test_members_against_single_runs(V, runs, b):
    """Every member of the 70 x 20 batch against its run alone (batch 1, its own parameters and targets): the six outputs
    bit for bit."""
    prob, out, _ = runs(GRIDS[0])
    single, _ = _run(V, prob, [b], [1] * CALLS)
    for key in KEYS:
        assert _same_bits(single[key][0], out[key][b]), (key, single[key][0], out[key][b])


def test_stop_rule_in_a_mixed_batch(V, O2):
    """20 x 70, members a, e and a second default member, pgd_iterate(24): member e (change == 0.0 in every iteration) stops
    at k = 21, the first k > 20; from index 22 on its double outputs are NaN ("NaN where no iteration ran", include/vch.h; the
    integer attempts stay as the caller passed them, zero here), before that its errors and cost are bit-constant.  The
    other members run all 24 iterations with the bits of the batch without e."""
    prob = _problem(O2, V, GRIDS[1], seeds=(42, 46, 47), names=("a", "e", "a"))
    out, _ = _run(V, prob, range(3), [24])
    assert out["iters"] == [24]
    for key in KEYS:
        if key == "attempts":
            assert np.all(out[key][1, :22] == 10) and np.all(out[key][1, 22:] == 0), out[key][1]
            continue
        assert np.isnan(out[key][1, 22:]).all() and not np.isnan(out[key][1, :22]).any(), (key, out[key][1])
        assert not np.isnan(out[key][[0, 2]]).any(), key
    assert np.all(out["change"][1, :22] == 0.0)
    for key in ("cost", "tracking_error", "terminal_error"):
        assert _same_bits(out[key][1, :22], np.repeat(out[key][1, :1], 22)), (key, out[key][1])
    assert np.all(out["change"][[0, 2]] > 1e-5)                              # the stop rule had nothing to act on there
    two, _ = _run(V, prob, [0, 2], [24])
    for key in KEYS:
        assert _same_bits(two[key], out[key][[0, 2]]), key
