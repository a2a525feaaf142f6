"""The trust-region rounds of csrc/vch_newton.h (vch_trust_state, vch_trust_check, vch_trust_rounds: what vch1d_pgd_trust
runs) on the CPU, without a device: acceptance at the Armijo edge, both branches of the radius rule, the clamp at radius_max,
STALLED below radius_min, a cost that is not finite, the end states without a trial, and one member idle while another goes
on.

tests/trust_replay_main.cpp is a scripted adapter of that loop, as tests/newton_replay_main.cpp is of the damped rounds'; the
program is compiled once per session with the address and undefined-behaviour sanitizers and run as an ordinary child
process.  Every decision is asserted exactly: the radii and costs are dyadic, and the Armijo bound is evaluated here in the
same order, cost - 1e-4 * pred."""
import math
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "sparse-optimal-control-of-viscous-chan-hilliard-via-gradient-descent--1d-2d_amd")
ACCEPTED, STATIONARY, NEGCURV, BREAKDOWN, STALLED, IDLE, REJECTED = range(7)      # VCH_NEWTON_* of include/vch.h
CG_LIMIT, CG_CONVERGED, CG_NEGCURV, CG_BREAKDOWN, CG_BOUNDARY = range(5)          # VCH_CG_*
KEYS = ("cost", "cost_new", "pred", "rnorm0", "radius", "ratio", "xnorm", "cg_steps", "cg_status", "status", "n_free", "pinned",
        "clipped")


@pytest.fixture(scope="session")
def replay_bin(tmp_path_factory):
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.fail("no C++ compiler: neither c++ on the path nor /opt/rocm/llvm/bin/clang++")
    out = str(tmp_path_factory.mktemp("trust_replay") / "trust_replay")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "trust_replay_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def entry(n_free=100, rnorm0=1.0, cg_status=CG_CONVERGED, cg_steps=5, pred=0.5, xnorm=0.5, cost_new=0.0):
    return (n_free, rnorm0, cg_status, cg_steps, pred, xnorm, cost_new)


def script_text(scripts, n_rounds, radius_max, radius_min):
    text = f"{len(scripts)} {n_rounds} {float(radius_max).hex()} {float(radius_min).hex()}\n"
    for J0, radius0, ents in scripts:
        text += f"{float(J0).hex()} {float(radius0).hex()} {len(ents)}"
        for e in ents:
            text += f" {e[0]} {float(e[1]).hex()} {e[2]} {e[3]} {float(e[4]).hex()} {float(e[5]).hex()} {float(e[6]).hex()}"
        text += "\n"
    return text


def replay(binary, scripts, n_rounds, radius_max=64.0, radius_min=2.0 ** -20, options=()):
    """scripts: per trajectory (J0, radius0, [entries]) -> dict(rounds, moved, rec {(b, r): dict of KEYS}, solves {r: radii},
    trials {r: sit-out flags}, J: final costs)."""
    r = subprocess.run([binary, *options], input=script_text(scripts, n_rounds, radius_max, radius_min), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(rec={}, solves={}, trials={})
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "rec":
            vals = [float(v) for v in w[3:10]] + [int(v) for v in w[10:16]]
            out["rec"][(int(w[1]), int(w[2]))] = dict(zip(KEYS, vals))
        elif w[0] == "round":
            out["solves"][int(w[1])] = [float(v) for v in w[2:]]
        elif w[0] == "trial":
            out["trials"][int(w[1])] = [int(v) for v in w[2:]]
        elif w[0] == "rounds":
            out["rounds"], out["moved"] = int(w[1]), int(w[3])
        else:
            assert w[0] == "J", line
            out["J"] = [float(v) for v in w[1:]]
    assert len(out["rec"]) == len(scripts) * n_rounds
    return out


def is_initial(cell):
    return (all(math.isnan(cell[k]) for k in KEYS[:7]) and cell["cg_steps"] == cell["cg_status"] == 0 and cell["status"] == IDLE
            and cell["n_free"] == cell["pinned"] == cell["clipped"] == 0)


def test_the_armijo_edge_is_accepted_and_the_next_value_is_not(replay_bin):
    edge = 2.0 - 1e-4 * 0.5
    R = replay(replay_bin, [(2.0, 1.0, [entry(cost_new=edge), entry(cost_new=1.0)])], 2)
    a, b = R["rec"][(0, 0)], R["rec"][(0, 1)]
    assert R["rounds"] == 2 and R["moved"] == 1 and R["J"] == [1.0]
    assert (a["status"], a["cost"], a["cost_new"]) == (ACCEPTED, 2.0, edge) and a["ratio"] == (2.0 - edge) / 0.5
    assert a["radius"] == 1.0 and b["radius"] == 0.125                 # rho = 1e-4 < 1/4: a quarter of min(radius, ||x||_D = 1/2)
    assert (b["status"], b["cost"], b["cost_new"]) == (ACCEPTED, edge, 1.0)          # the next round starts from the accepted cost
    above = math.nextafter(edge, math.inf)
    R = replay(replay_bin, [(2.0, 1.0, [entry(cost_new=above), entry(cost_new=1.0)])], 2)
    a, b = R["rec"][(0, 0)], R["rec"][(0, 1)]
    assert (a["status"], a["cost"], a["cost_new"]) == (REJECTED, 2.0, 2.0)           # unmoved, and it goes on
    assert (b["status"], b["cost"], b["cost_new"], b["radius"]) == (ACCEPTED, 2.0, 1.0, 0.125)
    assert R["trials"] == {0: [0], 1: [0]} and R["solves"] == {0: [1.0], 1: [0.125]}


@pytest.mark.parametrize("cg_status, xnorm, cost_new, radius_max, want", [
    (CG_BOUNDARY, 1.0, 1.5, 64.0, 2.0),         # rho = 1 on the boundary: doubled
    (CG_NEGCURV, 1.0, 1.5, 64.0, 2.0),          # and after negative curvature
    (CG_BOUNDARY, 1.0, 1.5, 1.5, 1.5),          # clamped at radius_max
    (CG_CONVERGED, 0.5, 1.5, 64.0, 1.0),        # an interior step: kept whatever rho
    (CG_LIMIT, 0.5, 1.5, 64.0, 1.0),
    (CG_BOUNDARY, 1.0, 1.625, 64.0, 1.0),       # rho = 3/4 is not above 3/4: kept
    (CG_BOUNDARY, 1.0, 1.875, 64.0, 1.0),       # rho = 1/4 is not below 1/4: kept
    (CG_BOUNDARY, 1.0, 1.9375, 64.0, 0.25),     # rho = 1/8: a quarter of the radius
    (CG_CONVERGED, 0.5, 1.9375, 64.0, 0.125),   # ... of ||x||_D where that is smaller
    (CG_BOUNDARY, 1.0, 2.5, 64.0, 0.25),        # the cost went up: rejected and shrunk
])
def test_the_radius_rule(replay_bin, cg_status, xnorm, cost_new, radius_max, want):
    ents = [entry(cg_status=cg_status, xnorm=xnorm, cost_new=cost_new), entry(cost_new=-1.0)]
    R = replay(replay_bin, [(2.0, 1.0, ents)], 2, radius_max=radius_max)
    a, b = R["rec"][(0, 0)], R["rec"][(0, 1)]
    assert a["ratio"] == (2.0 - cost_new) / 0.5 and a["radius"] == 1.0 and a["xnorm"] == xnorm
    assert a["status"] == (ACCEPTED if cost_new < 2.0 else REJECTED)
    assert b["radius"] == want and R["solves"][1] == [want]


def test_stalled_below_radius_min_and_idle_afterwards(replay_bin):
    ents = [entry(cg_status=CG_BOUNDARY, xnorm=1.0, cost_new=3.0)] * 2 + [entry(cost_new=0.0)]
    R = replay(replay_bin, [(2.0, 1.0, ents)], 4, radius_min=0.125)
    st = [R["rec"][(0, r)]["status"] for r in range(4)]
    assert st == [REJECTED, STALLED, IDLE, IDLE] and R["rounds"] == 2 and R["moved"] == 0 and R["J"] == [2.0]
    assert [R["rec"][(0, r)]["radius"] for r in range(2)] == [1.0, 0.25]              # 1/16 < radius_min ends it
    assert R["rec"][(0, 1)]["cost_new"] == 2.0 and is_initial(R["rec"][(0, 2)]) and is_initial(R["rec"][(0, 3)])
    # an accepted step whose radius falls below radius_min keeps ACCEPTED and ends the trajectory
    edge = 2.0 - 1e-4 * 0.5
    R = replay(replay_bin, [(2.0, 1.0, [entry(cost_new=edge), entry()])], 3, radius_min=0.5)
    assert [R["rec"][(0, r)]["status"] for r in range(3)] == [ACCEPTED, IDLE, IDLE] and R["rounds"] == 1 and R["J"] == [edge]


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_a_cost_that_is_not_finite_is_never_accepted(replay_bin, bad):
    R = replay(replay_bin, [(2.0, 1.0, [entry(cg_status=CG_BOUNDARY, xnorm=1.0, cost_new=bad), entry(cost_new=1.0)])], 2)
    a, b = R["rec"][(0, 0)], R["rec"][(0, 1)]
    assert a["status"] == REJECTED and a["cost_new"] == 2.0
    assert b["radius"] == 0.25 and b["status"] == ACCEPTED
    assert not math.isfinite(a["ratio"])


@pytest.mark.parametrize("ent, want", [
    (entry(rnorm0=0.0, cg_steps=0), STATIONARY),
    (entry(n_free=0, rnorm0=0.0, cg_steps=0), STATIONARY),
    (entry(cg_status=CG_BREAKDOWN, cg_steps=0), BREAKDOWN),
    (entry(cg_status=CG_BREAKDOWN, cg_steps=4), BREAKDOWN),
])
def test_end_states_without_a_trial(replay_bin, ent, want):
    R = replay(replay_bin, [(2.0, 1.0, [ent, entry()])], 3)
    a = R["rec"][(0, 0)]
    assert R["rounds"] == 1 and R["trials"] == {} and R["moved"] == 0
    assert (a["status"], a["cost"], a["cost_new"]) == (want, 2.0, 2.0) and math.isnan(a["ratio"])
    assert is_initial(R["rec"][(0, 1)]) and is_initial(R["rec"][(0, 2)])


def test_negative_curvature_at_step_zero_is_a_step(replay_bin):
    R = replay(replay_bin, [(2.0, 1.0, [entry(cg_status=CG_NEGCURV, cg_steps=1, xnorm=1.0, cost_new=1.5)])], 1)
    a = R["rec"][(0, 0)]
    assert (a["status"], a["cost_new"], a["cg_status"], a["cg_steps"]) == (ACCEPTED, 1.5, CG_NEGCURV, 1) and R["trials"] == {0: [0]}


def test_one_member_idle_while_another_goes_on(replay_bin):
    """Member 0 is stationary at round 0; member 1 is rejected, accepted, rejected; member 2 accepts and then breaks down.
    Who sits which trial out, the radius each solve gets (an idle member's: its radius0), IDLE in every later round."""
    scripts = [
        (1.0, 4.0, [entry(n_free=0, rnorm0=0.0, cg_steps=0)]),
        (2.0, 1.0, [entry(cg_status=CG_BOUNDARY, xnorm=1.0, cost_new=2.5), entry(cg_status=CG_BOUNDARY, xnorm=0.25, cost_new=1.5),
                    entry(cg_status=CG_BOUNDARY, xnorm=0.5, cost_new=1.75)]),
        (3.0, 2.0, [entry(cg_status=CG_BOUNDARY, xnorm=2.0, cost_new=2.5), entry(cg_status=CG_BREAKDOWN, cg_steps=2)]),
    ]
    R = replay(replay_bin, scripts, 3)
    st = lambda b: [R["rec"][(b, r)]["status"] for r in range(3)]
    assert R["rounds"] == 3 and R["moved"] == 1
    assert st(0) == [STATIONARY, IDLE, IDLE] and st(1) == [REJECTED, ACCEPTED, REJECTED] and st(2) == [ACCEPTED, BREAKDOWN, IDLE]
    assert R["trials"] == {0: [1, 0, 0], 1: [1, 0, 1], 2: [1, 0, 1]}
    assert R["solves"] == {0: [4.0, 1.0, 2.0], 1: [4.0, 0.25, 4.0], 2: [4.0, 0.5, 2.0]}
    assert R["J"] == [1.0, 1.5, 2.5]
    assert [R["rec"][(1, r)]["cost"] for r in range(3)] == [2.0, 2.0, 1.5] and R["rec"][(1, 2)]["cost_new"] == 1.5
    assert is_initial(R["rec"][(0, 1)]) and is_initial(R["rec"][(0, 2)]) and is_initial(R["rec"][(2, 2)])


def test_batch_equals_single_replays(replay_bin):
    a = (2.0, 1.0, [entry(cg_status=CG_BOUNDARY, xnorm=1.0, cost_new=2.5), entry(cost_new=1.0), entry(rnorm0=0.0)])
    b = (5.0, 0.5, [entry(cg_status=CG_NEGCURV, xnorm=0.5, cost_new=4.5), entry(cost_new=4.0), entry(cost_new=3.0)])
    both = replay(replay_bin, [a, b], 3)
    for i, one in enumerate((a, b)):
        alone = replay(replay_bin, [one], 3)
        for r in range(3):
            assert repr(both["rec"][(i, r)]) == repr(alone["rec"][(0, r)])


@pytest.mark.parametrize("n_rounds, radius0, radius_max, radius_min, options, message", [
    (0, 1.0, 64.0, 1e-6, [], "n_rounds must be >= 1"),
    (2, 1.0, 64.0, 1e-6, ["--k", "0"], "k must be >= 1"),
    (2, 1.0, 64.0, 1e-6, ["--precond", "2"], "precond must be 0 or 1"),
    (2, 1.0, 64.0, 1e-6, ["--cg-tol", "nan"], "cg_tol must be finite"),
    (2, 0.0, 64.0, 1e-6, [], "every radius0 must be finite and > 0"),
    (2, -1.0, 64.0, 1e-6, [], "every radius0 must be finite and > 0"),
    (2, math.inf, 64.0, 1e-6, [], "every radius0 must be finite and > 0"),
    (2, math.nan, 64.0, 1e-6, [], "every radius0 must be finite and > 0"),
    (2, 1.0, math.inf, 1e-6, [], "radius_max must be finite and > 0"),
    (2, 1.0, 0.0, 1e-6, [], "radius_max must be finite and > 0"),
    (2, 1.0, 64.0, 0.0, [], "radius_min must be finite and > 0"),
    (2, 1.0, 64.0, math.nan, [], "radius_min must be finite and > 0"),
    (2, 1.0, 64.0, 1e-6, ["--null-ratio"], "NULL cost_out, cost_new_out, pred_out, rnorm0_out, radius_out, ratio_out, xnorm_out, "
                                            "cg_steps_out, cg_status_out, status_out or counts_out"),
])
def test_bad_arguments_are_refused_before_any_hook(replay_bin, n_rounds, radius0, radius_max, radius_min, options, message):
    text = script_text([(2.0, radius0, [entry(), entry()])], n_rounds, radius_max, radius_min)
    r = subprocess.run([replay_bin] + options, input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, r.stdout + r.stderr
    assert r.stdout == f"error -1 hooks 0 trust_replay: {message}\n"
