"""The device-resident damped Newton rounds (csrc/vch_newton.h) on the CPU, without a device: the verdicts (the end states
after the solve, the Armijo test, the halving, who sits a trial or a round out) and the round loop that applies them and
keeps the call's record, vch_newton_rounds, the one both engines run.

tests/newton_replay_main.cpp is a third adapter of that loop; the outcomes of the solves and the trial costs come from a
script.  The program is compiled once per session with the address and undefined-behaviour sanitizers and run as an ordinary
child process.  Every decision is asserted exactly: the step lengths are powers of two and the Armijo bound is evaluated here
in the same order, cost - (1e-4 * s) * pred."""
import math
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "sparse-optimal-control-of-viscous-chan-hilliard-via-gradient-descent--1d-2d_amd")
ACCEPTED, STATIONARY, NEGCURV, BREAKDOWN, STALLED, IDLE = range(6)      # VCH_NEWTON_* of include/vch.h
CG_LIMIT, CG_CONVERGED, CG_NEGCURV, CG_BREAKDOWN = range(4)              # VCH_CG_*


@pytest.fixture(scope="session")
def replay_bin(tmp_path_factory):
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.fail("no C++ compiler: neither c++ on the path nor /opt/rocm/llvm/bin/clang++")
    out = str(tmp_path_factory.mktemp("newton_replay") / "newton_replay")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "newton_replay_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def entry(n_free=100, rnorm0=1.0, cg_status=CG_CONVERGED, cg_steps=5, pred=0.5, accept_at=0, cost_new=0.0):
    return (n_free, rnorm0, cg_status, cg_steps, pred, accept_at, cost_new)


def script_text(scripts, n_rounds, max_halvings):
    B = len(scripts)
    text = f"{B} {n_rounds} {max_halvings}\n"
    for J0, ents in scripts:
        text += f"{float(J0).hex()} {len(ents)}"
        for e in ents:
            text += f" {e[0]} {float(e[1]).hex()} {e[2]} {e[3]} {float(e[4]).hex()} {e[5]} {float(e[6]).hex()}"
        text += "\n"
    return text


def replay(binary, scripts, n_rounds, max_halvings):
    """scripts: per trajectory (J0, [entries]) -> (rounds run, rows {(b, r): (status, s, halvings, cost, cost_new)},
    trials {r: [(sit-out flags, step lengths)]})."""
    B = len(scripts)
    r = subprocess.run([binary], input=script_text(scripts, n_rounds, max_halvings), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rows, trials, rounds = {}, {}, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "row":
            rows[(int(w[1]), int(w[2]))] = (int(w[3]), float(w[4]), int(w[5]), float(w[6]), float(w[7]))
        elif w[0] == "trial":
            trials.setdefault(int(w[1]), []).append(([int(v) for v in w[2:2 + B]], [float(v) for v in w[2 + B:2 + 2 * B]]))
        elif w[0] == "rounds":
            rounds = int(w[1])
        else:
            assert w[0] == "round", line
    return rounds, rows, trials


def armijo_edge(cost, s, pred):
    return cost - 1e-4 * s * pred


def test_accept_at_full_step(replay_bin):
    edge = armijo_edge(2.0, 1.0, 0.5)
    rounds, rows, trials = replay(replay_bin, [(2.0, [entry(cost_new=edge), entry(cost_new=1.0)])], 2, 10)
    assert rounds == 2
    assert rows[(0, 0)] == (ACCEPTED, 1.0, 0, 2.0, edge)             # the bound itself is accepted (<=)
    assert rows[(0, 1)] == (ACCEPTED, 1.0, 0, edge, 1.0)             # the next round starts from the accepted cost
    assert trials == {0: [([0], [1.0])], 1: [([0], [1.0])]}


def test_just_above_the_bound_is_rejected(replay_bin):
    above = math.nextafter(armijo_edge(2.0, 1.0, 0.5), math.inf)
    _, rows, trials = replay(replay_bin, [(2.0, [entry(cost_new=above, accept_at=0)])], 1, 0)
    assert rows[(0, 0)][0] == STALLED and math.isnan(rows[(0, 0)][1]) and rows[(0, 0)][3:] == (2.0, 2.0)
    assert len(trials[0]) == 1


@pytest.mark.parametrize("j", [1, 3, 10])
def test_accept_after_j_halvings(replay_bin, j):
    s = 0.5 ** j
    edge = armijo_edge(2.0, s, 0.5)
    rounds, rows, trials = replay(replay_bin, [(2.0, [entry(accept_at=j, cost_new=edge)])], 1, 10)
    assert rounds == 1
    assert rows[(0, 0)] == (ACCEPTED, s, j, 2.0, edge)
    assert [t[1][0] for t in trials[0]] == [0.5 ** i for i in range(j + 1)]
    # the same trial cost one halving earlier is above that step's bound: the bound moves with s
    assert edge > armijo_edge(2.0, 2 * s, 0.5)


@pytest.mark.parametrize("max_halvings", [0, 2, 10])
def test_stall_after_max_halvings(replay_bin, max_halvings):
    rounds, rows, trials = replay(replay_bin, [(2.0, [entry(accept_at=-1), entry()])], 3, max_halvings)
    assert rounds == 1                                               # every trajectory has ended: the call stops early
    st, s, halv, cost, cost_new = rows[(0, 0)]
    assert (st, halv, cost, cost_new) == (STALLED, max_halvings, 2.0, 2.0) and math.isnan(s)
    assert [t[1][0] for t in trials[0]] == [0.5 ** i for i in range(max_halvings + 1)]


def test_accept_one_halving_too_late_is_a_stall(replay_bin):
    _, rows, trials = replay(replay_bin, [(2.0, [entry(accept_at=3, cost_new=0.0)])], 1, 2)
    assert rows[(0, 0)][0] == STALLED and len(trials[0]) == 3


def test_a_cost_that_is_not_finite_is_never_accepted(replay_bin):
    _, rows, _ = replay(replay_bin, [(2.0, [entry(accept_at=0, cost_new=float("nan"))])], 1, 1)
    assert rows[(0, 0)][0] == STALLED
    _, rows, _ = replay(replay_bin, [(2.0, [entry(accept_at=0, cost_new=float("inf"))])], 1, 1)
    assert rows[(0, 0)][0] == STALLED


@pytest.mark.parametrize("ent, want", [
    (entry(rnorm0=0.0, cg_steps=0), STATIONARY),
    (entry(n_free=0, rnorm0=0.0, cg_steps=0), STATIONARY),
    (entry(cg_status=CG_NEGCURV, cg_steps=0), NEGCURV),
    (entry(cg_status=CG_BREAKDOWN, cg_steps=0), BREAKDOWN),
    (entry(cg_status=CG_BREAKDOWN, cg_steps=4), BREAKDOWN),          # x may not be finite: no march is started
])
def test_end_states_without_a_trial(replay_bin, ent, want):
    rounds, rows, trials = replay(replay_bin, [(2.0, [ent, entry()])], 3, 10)
    assert rounds == 1 and trials == {}
    st, s, halv, cost, cost_new = rows[(0, 0)]
    assert (st, halv, cost, cost_new) == (want, 0, 2.0, 2.0) and math.isnan(s)


@pytest.mark.parametrize("status", [CG_CONVERGED, CG_LIMIT, CG_NEGCURV])
def test_statuses_whose_x_is_a_step(replay_bin, status):
    """converged, the step limit, and negative curvature after at least one step: x is tried."""
    _, rows, trials = replay(replay_bin, [(2.0, [entry(cg_status=status, cg_steps=2, cost_new=1.0)])], 1, 10)
    assert rows[(0, 0)] == (ACCEPTED, 1.0, 0, 2.0, 1.0) and len(trials[0]) == 1


def test_one_member_idle_while_another_goes_on(replay_bin):
    """Member 0 is stationary at round 0, member 1 accepts after 2 halvings, then at s = 1, then stalls; member 2 accepts
    at s = 1 and then meets negative curvature.  Who sits which trial out, and IDLE in every later round."""
    scripts = [
        (1.0, [entry(n_free=0, rnorm0=0.0, cg_steps=0)]),
        (2.0, [entry(accept_at=2, cost_new=1.5), entry(accept_at=0, cost_new=1.25), entry(accept_at=-1)]),
        (3.0, [entry(accept_at=0, cost_new=2.5), entry(cg_status=CG_NEGCURV, cg_steps=0)]),
    ]
    rounds, rows, trials = replay(replay_bin, scripts, 5, 1 + 1)
    assert rounds == 3
    assert [rows[(0, r)][0] for r in range(3)] == [STATIONARY, IDLE, IDLE]
    assert [rows[(1, r)][0] for r in range(3)] == [ACCEPTED, ACCEPTED, STALLED]
    assert [rows[(2, r)][0] for r in range(3)] == [ACCEPTED, NEGCURV, IDLE]
    assert rows[(1, 0)] == (ACCEPTED, 0.25, 2, 2.0, 1.5) and rows[(1, 1)] == (ACCEPTED, 1.0, 0, 1.5, 1.25)
    assert rows[(1, 2)][2:] == (2, 1.25, 1.25)
    assert rows[(2, 0)] == (ACCEPTED, 1.0, 0, 3.0, 2.5)
    # an idle member's record keeps its cost and moves nothing
    assert rows[(0, 2)][2:] == (0, 1.0, 1.0) and math.isnan(rows[(0, 2)][1])
    assert rows[(2, 2)][2:] == (0, 2.5, 2.5)
    assert trials[0] == [([1, 0, 0], [1.0, 1.0, 1.0]), ([1, 0, 1], [1.0, 0.5, 1.0]), ([1, 0, 1], [1.0, 0.25, 1.0])]
    assert trials[1] == [([1, 0, 1], [1.0, 1.0, 1.0])]
    assert trials[2] == [([1, 0, 1], [1.0, 1.0, 1.0]), ([1, 0, 1], [1.0, 0.5, 1.0]), ([1, 0, 1], [1.0, 0.25, 1.0])]


def test_batch_equals_single_replays(replay_bin):
    a = (2.0, [entry(accept_at=1, cost_new=1.0), entry(accept_at=-1)])
    b = (5.0, [entry(accept_at=0, cost_new=4.0), entry(accept_at=3, cost_new=3.0), entry(rnorm0=0.0)])
    _, both, _ = replay(replay_bin, [a, b], 3, 4)
    _, ra, _ = replay(replay_bin, [a], 3, 4)
    _, rb, _ = replay(replay_bin, [b], 3, 4)
    for r in range(2):
        assert repr(both[(0, r)]) == repr(ra[(0, r)])
    assert both[(0, 2)][0] == IDLE
    for r in range(3):
        assert repr(both[(1, r)]) == repr(rb[(0, r)])


# ---------------------------------------------------------------------------------------------------------------------
# the driver's record and its argument checks
# ---------------------------------------------------------------------------------------------------------------------
def record(binary, scripts, n_rounds, max_halvings):
    """-> (rounds run, {(b, r): (cost, cost_new, s, pred, rnorm0, halvings, cg_steps, cg_status, status, n_free, pinned,
    clipped)}): every cell of the record the driver keeps, [B][n_rounds]."""
    r = subprocess.run([binary, "--record"], input=script_text(scripts, n_rounds, max_halvings), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rounds, rec = None, {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "rounds":
            rounds = int(w[1])
        elif w[0] == "rec":
            rec[(int(w[1]), int(w[2]))] = tuple(float(v) for v in w[3:8]) + tuple(int(v) for v in w[8:15])
    assert len(rec) == len(scripts) * n_rounds
    return rounds, rec


def is_initial(cell):
    return all(math.isnan(v) for v in cell[:5]) and cell[5:8] == (0, 0, 0) and cell[8] == IDLE and cell[9:] == (0, 0, 0)


def test_record_of_an_ended_trajectory_keeps_its_initial_values(replay_bin):
    """Trajectory 0 ends in round 0, trajectory 1 runs three rounds: every cell of trajectory 0 in rounds 1 and 2 is as the
    driver initialised it, NaN in the five double arrays, 0 in the three counters and in counts, IDLE in status."""
    scripts = [
        (1.0, [entry(n_free=7, rnorm0=0.0, cg_steps=0, pred=0.0)]),
        (2.0, [entry(n_free=50, rnorm0=3.0, cg_steps=4, pred=0.5, accept_at=1, cost_new=1.5),
               entry(n_free=51, rnorm0=2.0, cg_status=CG_LIMIT, cg_steps=6, pred=0.25, accept_at=0, cost_new=1.25),
               entry(n_free=52, rnorm0=1.0, cg_steps=2, pred=0.125, accept_at=-1)]),
    ]
    rounds, rec = record(replay_bin, scripts, 3, 2)
    assert rounds == 3
    assert rec[(0, 0)][:2] == (1.0, 1.0) and math.isnan(rec[(0, 0)][2])
    assert rec[(0, 0)][3:] == (0.0, 0.0, 0, 0, CG_CONVERGED, STATIONARY, 7, 0, 0)
    assert is_initial(rec[(0, 1)]) and is_initial(rec[(0, 2)])
    # what the live trajectory's cells hold beside them: the solve's record, the accepted step, the cost before and after
    assert rec[(1, 0)] == (2.0, 1.5, 0.5, 0.5, 3.0, 1, 4, CG_CONVERGED, ACCEPTED, 50, 0, 0)
    assert rec[(1, 1)] == (1.5, 1.25, 1.0, 0.25, 2.0, 0, 6, CG_LIMIT, ACCEPTED, 51, 0, 0)
    assert rec[(1, 2)][:2] == (1.25, 1.25) and math.isnan(rec[(1, 2)][2])
    assert rec[(1, 2)][3:] == (0.125, 1.0, 2, 2, CG_CONVERGED, STALLED, 52, 0, 0)


def test_done_rounds_stops_early_and_later_rounds_stay_initial(replay_bin):
    scripts = [(2.0, [entry(accept_at=0, cost_new=1.0), entry(rnorm0=0.0, cg_steps=0)]),
               (3.0, [entry(cg_status=CG_BREAKDOWN, cg_steps=1)])]
    rounds, rec = record(replay_bin, scripts, 5, 3)
    assert rounds == 2                                              # every trajectory has ended: three rounds are never begun
    assert [rec[(0, r)][8] for r in range(2)] == [ACCEPTED, STATIONARY] and rec[(1, 0)][8] == BREAKDOWN
    assert is_initial(rec[(1, 1)])
    for b in range(2):
        for r in range(2, 5):
            assert is_initial(rec[(b, r)]), (b, r)


@pytest.mark.parametrize("n_rounds, max_halvings, options, message", [
    (0, 3, [], "n_rounds must be >= 1"),
    (2, 3, ["--k", "0"], "k must be >= 1"),
    (2, -1, [], "max_halvings must be >= 0"),
    (2, 3, ["--precond", "2"], "precond must be 0 or 1"),
    (2, 3, ["--cg-tol", "inf"], "cg_tol must be finite"),
    (2, 3, ["--cg-tol", "nan"], "cg_tol must be finite"),
    (2, 3, ["--null-s"], "NULL cost_out, cost_new_out, s_out, pred_out, rnorm0_out, halvings_out, cg_steps_out, cg_status_out, "
                         "status_out or counts_out"),
])
def test_bad_shared_arguments_are_refused_before_any_hook(replay_bin, n_rounds, max_halvings, options, message):
    text = script_text([(2.0, [entry(), entry()])], n_rounds, max_halvings)
    r = subprocess.run([replay_bin] + options, input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, r.stdout + r.stderr
    assert r.stdout == f"error -1 hooks 0 newton_replay: {message}\n"   # VCH_ERR_ARG, the entry point's name, no output before it


def test_the_options_leave_a_good_call_as_it_is(replay_bin):
    text = script_text([(2.0, [entry(accept_at=1, cost_new=1.0)])], 1, 4)
    plain = subprocess.run([replay_bin], input=text, capture_output=True, text=True, timeout=60)
    opts = subprocess.run([replay_bin, "--k", "5", "--precond", "1", "--cg-tol", "1e-6", "--record"], input=text, capture_output=True,
                          text=True, timeout=60)
    assert plain.returncode == 0 and opts.returncode == 0
    assert opts.stdout.startswith(plain.stdout) and opts.stdout[len(plain.stdout):].startswith("rec 0 0 ")
