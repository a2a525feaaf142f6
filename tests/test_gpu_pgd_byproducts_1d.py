"""The 1D twin of tests/test_gpu_pgd_byproducts.py: `change`, `tracking_error` and `terminal_error` of every accepted
iteration of the device-resident 1D PGD loop against the long-double restatement (tests/_pgd_byproducts_ref.py) applied
to the fields pulled after every call, off the N = 32 golden: N = 33 and 130 (one and three blocks of the column
kernels, no multiple of anything), Lx = 1.3, six steps of which the last is half as long (rows = 8 with the duplicated
t = 0 row), a batch of five in the full sparsity mode with one parameter and target set per member:
  a  defaults
  b  b1 = 0 and phi_T = 0: the tracking error is still reported, the terminal denominator is the bare 1e-12 guard
  c  phi_Q = 0: the RMS fallback of the tracking denominator, for this member only
  d  alpha_max of the golden g1d_pgd_32_bt (2e5): the line search runs out and returns its last try.  Every candidate of
     such a search sits on the box (u = +-1 whatever the step), so they all share one change
  f  member d with alpha_max = 1000: at N = 130 the oracle's loop accepts a fourth trial by descent and then runs out, with
     candidates up to 0.39 apart (at N = 33 members a and c run out at iteration 3 with distinct candidates)

Tolerance: nodes * EPS relative with nodes = rows (N+1), EPS = 2^-52, for the reason given in the 2D file; zero exactly.

The stop case adds the two ways the stop rule (change < 1e-5 and k > 10) can fire: kappa_sparsity = 10 keeps u = 0
(change == 0.0), and a warm start with alpha_max = 1e-5 moves the control by 2.7e-6 of its norm per iteration (picked on
the CPU with the restatement's loop over the oracle: every step descends at its first trial, the errors of consecutive
states differ by 5e-10 relative, 2000 times the bound).  On the stopping iteration the engine reports the errors of the
NEW iterate's state and takes the new control, but the resident state history stays the previous iterate's (the stop
quirk of include/vch.h, G1:462-465).
"""
import numpy as np
import pytest

import _pgd_byproducts_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu

DT, T, LX = 1e-2, 0.055, 1.3
SIZES = (33, 130)
NAMES = ("a", "b", "c", "d", "f")
SEEDS = (42, 43, 44, 45, 45)
CALLS = 4
KEYS = ("cost", "alpha", "trials", "change", "tracking_error", "terminal_error")


@pytest.fixture(scope="module")
def V():
    import vch_amd
    vch_amd.build()
    return vch_amd


@pytest.fixture(scope="module")
def O1():
    from oracle import vch1d_oracle
    return vch1d_oracle


def _grid(V, N):
    tg, dts = V.time_grid(T, DT)
    assert dts.size == 6 and abs(dts[-1] - 0.5 * DT) < 1e-12
    return np.linspace(0.0, LX, N + 1), np.r_[0.0, tg], dts


def _problem(O1, V, N):
    x, t, dts = _grid(V, N)
    bt = float(golden("g1d_pgd_32_bt.npz")["alpha_max"])
    assert bt == 2e5
    opts = [O1.OptParams1D(), O1.OptParams1D(b1=0.0), O1.OptParams1D(), O1.OptParams1D(alpha_max=bt),
            O1.OptParams1D(alpha_max=1000.0)]
    phi0, phi_T, phi_Q = [], [], []
    for name, seed in zip(NAMES, SEEDS):
        p0 = O1.init_phi_random(N, 1e-2, amp=0.01, seed=seed)
        pT, pQ = O1.build_targets(x, t, p0, LX, T)
        if name == "b":
            pT = np.zeros_like(pT)
            pQ = (1.0 - t / t[-1])[:, None] * p0                            # the ramp towards the zero target
        if name == "c":
            pQ = np.zeros_like(pQ)
        phi0.append(p0), phi_T.append(pT), phi_Q.append(pQ)
    return dict(N=N, x=x, t=t, dts=dts, phi0=np.stack(phi0), phi_T=np.stack(phi_T), phi_Q=np.stack(phi_Q), opts=opts,
                u0=None)


def _run(V, prob, members, calls, pull=False):
    """The members `members` of prob as one batch: pgd_init, then pgd_iterate(n) for n in calls.  -> the outputs joined
    along the iteration axis, and with pull=True the (u, phi, phi_Q, r) pulled after pgd_init and after every call (r: the
    adjoint the call's last iteration started from; not yet computed after pgd_init)."""
    N, B, rows = prob["N"], len(members), prob["t"].size
    e = V.Engine1D(N=N, Lx=LX, batch=B, max_steps=rows)
    try:
        sel = lambda a: np.ascontiguousarray(a[list(members)])
        e.pgd_init(sel(prob["phi0"]), sel(prob["phi_T"]), prob["t"], prob["dts"], [V.make_opt(prob["opts"][m]) for m in members],
                   phi_Q=sel(prob["phi_Q"]), x=prob["x"], u0=None if prob["u0"] is None else sel(prob["u0"]))
        get = lambda: tuple(np.array(e.pgd_get(k)).reshape((B, rows, N + 1)) for k in ("u", "phi", "phi_Q", "r"))
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
def runs(V, O1):
    done = {}

    def get(N):
        if N not in done:
            prob = _problem(O1, V, N)
            out, pulls = _run(V, prob, range(5), [1] * CALLS, pull=True)
            done[N] = (prob, out, pulls)
        return done[N]
    return get


def _gaps(out, b, k, u, u_old, parts):
    ref = dict(change=R.change(u, u_old), tracking_error=parts["track"], terminal_error=parts["term"])
    return {key: R.gap(out[key][b, k], ref[key]) for key in ref}


@pytest.mark.parametrize("N", SIZES)
def test_byproducts_against_the_restatement(runs, O1, N):
    """change, tracking_error and terminal_error of every call and member within nodes * EPS of the restatement on the
    pulled fields.  Member d backtracks (trials > 1) in an iteration where member a accepts its first trial; some
    backtracked step has a change that its first candidate (rebuilt from the pulled adjoint) does not share; member c
    takes the RMS fallback and member a does not (from the restatement's own den and rms); member b's target norm is 0."""
    prob, out, pulls = runs(N)
    bound = prob["t"].size * (N + 1) * R.EPS
    assert out["iters"] == [1] * CALLS and not np.isnan(np.concatenate([out[k] for k in KEYS], axis=1)).any()
    tr = out["trials"]
    print(f"trials N {N}: {tr.tolist()}")
    assert any(tr[3, k] > 1 and tr[0, k] == 1 for k in range(CALLS)), tr
    worst, away = {}, [0.0]
    for k in range(CALLS):
        u_old, (u, phi, pq, r) = pulls[k][0], pulls[k + 1]
        assert np.array_equal(pq, prob["phi_Q"])
        for b, name in enumerate(NAMES):
            parts = R.errors_1d_parts(phi[b], pq[b], prob["phi_T"][b], prob["x"], prob["t"])
            assert parts["fallback"] == (name == "c"), (name, parts)
            assert (parts["den_T"] == 0.0) == (name == "b"), (name, parts)
            gaps = _gaps(out, b, k, u[b], u_old[b], parts)
            print(f"MEASURE 1d N {N} it {k} member {name}: trials {tr[b, k]} change {out['change'][b, k]:.6e} gap "
                  f"{gaps['change']:.2e} tracking {out['tracking_error'][b, k]:.6e} gap {gaps['tracking_error']:.2e} terminal "
                  f"{out['terminal_error'][b, k]:.6e} gap {gaps['terminal_error']:.2e} (nodes * EPS {bound:.2e})")
            for key, gp in gaps.items():
                worst[key] = max(worst.get(key, 0.0), gp)
                assert gp <= bound, (N, k, name, key, out[key][b, k], gp, bound)
            if tr[b, k] > 1 and out["change"][b, k] > 0.0:
                # what the first candidate's sums would have given: its step is alpha_prev = min(alpha_max, 1.2 alpha_{k-1})
                # (no plateau boost before the tenth iteration), the adjoint is the one the iteration started from
                o = prob["opts"][b]
                a_prev = o.alpha_max if k == 0 else min(o.alpha_max, 1.2 * out["alpha"][b, k - 1])
                u_first = O1.prox_project(O1.gradient_step(u_old[b], O1.gradient(r[b], u_old[b], o.b3), a_prev), a_prev,
                                          o.kappa_sparsity, o.u_min, o.u_max)
                away.append(R.gap(out["change"][b, k], R.change(u_first, u_old[b])))
                print(f"MEASURE 1d N {N} it {k} member {name}: change of the first candidate is {away[-1]:.2e} away")
    print(f"MEASURE 1d N {N} worst: " + " ".join(f"{key} {v:.2e}" for key, v in worst.items()) + f" (nodes * EPS {bound:.2e})")
    assert max(away) > 100.0 * bound, (away, bound)                      # the sums of the first candidate would not pass


@pytest.mark.parametrize("N", SIZES)
def test_one_call_against_many(V, runs, N):
    """pgd_iterate(4) on a fresh engine: all six outputs have the bits of four calls of one iteration."""
    prob, out, _ = runs(N)
    one, _ = _run(V, prob, range(5), [CALLS])
    assert one["iters"] == [CALLS]
    for key in KEYS:
        assert _same_bits(one[key], out[key]), (key, one[key], out[key])


@pytest.mark.parametrize("b", range(5), ids=NAMES)
def test_members_against_single_runs(V, runs, b):
    """Every member of the N = 130 batch against its run alone: the six outputs bit for bit."""
    prob, out, _ = runs(130)
    single, _ = _run(V, prob, [b], [1] * CALLS)
    for key in KEYS:
        assert _same_bits(single[key][0], out[key][b]), (key, single[key][0], out[key][b])


def _stop_problem(O1, V, N):
    """Members: 0 alpha_max = 10 (with the oracle's loop its change stays above 1e-2 for 13 iterations at both sizes; with the
    default 100 the line search at N = 33 runs out from iteration 3 on and the member itself stops at k = 11), 1
    kappa_sparsity = 10 (u = 0 is the fixed point), 2 warm start 0.3 sin(2 pi x / Lx) cos(pi t / T) with alpha_max = 1e-5."""
    x, t, dts = _grid(V, N)
    opts = [O1.OptParams1D(alpha_max=10.0), O1.OptParams1D(kappa_sparsity=10.0), O1.OptParams1D(alpha_max=1e-5)]
    phi0 = np.stack([O1.init_phi_random(N, 1e-2, amp=0.01, seed=s) for s in (42, 46, 47)])
    tg = [O1.build_targets(x, t, p0, LX, T) for p0 in phi0]
    u0 = np.zeros((3, t.size, N + 1))
    u0[2] = 0.3 * np.sin(2.0 * np.pi * x / LX)[None, :] * np.cos(np.pi * t / t[-1])[:, None]
    return dict(N=N, x=x, t=t, dts=dts, phi0=phi0, phi_T=np.stack([a for a, _ in tg]), phi_Q=np.stack([q for _, q in tg]),
                opts=opts, u0=u0)


@pytest.mark.parametrize("N", SIZES)
def test_stop_rule_and_the_stop_quirk(V, O1, N):
    """13 iterations as calls of 11, 1 and 1: members 1 and 2 stop at k = 11, the first k > 10; their double outputs of the
    third call are NaN ("NaN where no iteration ran"; the integer trials stay as passed, zero here) and member 0 runs on.
    On the stopping iteration, for both: `change` is that of the pulled controls; the resident state history keeps the
    bits it had before the call; the reported errors are those of the state the NEW control produces (marched again on an
    engine of its own), which for member 2 differ from the resident state's by more than the bound.  One call of 13 gives
    the same bits, and members 0 and 2 have the bits of the batch without member 1."""
    prob = _stop_problem(O1, V, N)
    rows = prob["t"].size
    bound = rows * (N + 1) * R.EPS
    out, pulls = _run(V, prob, range(3), [11, 1, 1], pull=True)
    assert out["iters"] == [11, 1, 1]
    for key in KEYS:
        if key == "trials":
            assert np.all(out[key][1:, 12] == 0) and np.all(out[key][:, :12] >= 1), out[key]
            continue
        assert np.isnan(out[key][1:, 12]).all() and not np.isnan(out[key][:, :12]).any() and not np.isnan(out[key][0]).any(), key
    assert np.all(out["change"][1, :12] == 0.0) and np.all(out["trials"][1, :12] == 5)
    assert np.all(out["change"][0] > 1e-5)
    assert np.all((out["change"][2, :12] > 0.0) & (out["change"][2, :12] < 1e-5)) and np.all(out["trials"][2, :12] == 1)
    for key in ("cost", "tracking_error", "terminal_error"):
        assert _same_bits(out[key][1, :12], np.repeat(out[key][1, :1], 12)), (key, out[key][1])
    (u10, phi10, _, _), (u11, phi11, pq, _), (u12, phi12, _, _) = pulls[1], pulls[2], pulls[3]
    for b in (1, 2):
        assert np.array_equal(phi11[b], phi10[b]) and np.array_equal(phi12[b], phi11[b]) and np.array_equal(u12[b], u11[b])
    assert not np.array_equal(phi11[0], phi10[0]) and not np.array_equal(u11[2], u10[2]) and not u11[1].any()
    e1 = V.Engine1D(N=N, Lx=LX, batch=1, max_steps=rows)
    try:
        for b in (1, 2):
            phi_new = e1.forward(prob["phi0"][b], prob["dts"], u=u11[b])[0]
            new = R.errors_1d_parts(phi_new, pq[b], prob["phi_T"][b], prob["x"], prob["t"])
            old = R.errors_1d_parts(phi11[b], pq[b], prob["phi_T"][b], prob["x"], prob["t"])
            gaps = _gaps(out, b, 11, u11[b], u10[b], new)
            away = {key: R.gap(out[key][b, 11], old[k2]) for key, k2 in (("tracking_error", "track"), ("terminal_error", "term"))}
            print(f"MEASURE 1d N {N} stop member {b}: change {out['change'][b, 11]:.6e} gap {gaps['change']:.2e} tracking gap "
                  f"{gaps['tracking_error']:.2e} terminal gap {gaps['terminal_error']:.2e}; to the resident state's errors "
                  f"{away['tracking_error']:.2e} {away['terminal_error']:.2e} (nodes * EPS {bound:.2e})")
            assert max(gaps.values()) <= bound, (N, b, gaps, bound)
            if b == 2:
                assert min(away.values()) > 100.0 * bound, (N, away, bound)
    finally:
        e1.close()
    one, _ = _run(V, prob, range(3), [13])
    assert one["iters"] == [13]
    two, _ = _run(V, prob, [0, 2], [13])
    for key in KEYS:
        assert _same_bits(one[key], out[key]), (key, one[key], out[key])
        assert _same_bits(two[key], out[key][[0, 2]]), key
