"""The PGD line-search rule (csrc/vch_pgd.h: accept / reject, "return last try", plateau boost, stop rule, per-trajectory
books, parameter validation) replayed on the CPU against the reference-made goldens, without a device.

tests/pgd_replay_main.cpp drives the state machine as the engines do; the trial costs come from a script made of a golden's
`attempts` / `trials` (the round a step was accepted in), `costs` and `changes`.  The program is compiled once per session
with the address and undefined-behaviour sanitizers and run as an ordinary child process.

Every comparison of a step size is `==`: the rule multiplies by the same constants in the same order as the references, and
a transcription of the loops reproduces the seven goldens bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden

PKG = os.path.join(ROOT, "sparse-optimal-control-of-viscous-chan-hilliard-via-gradient-descent--1d-2d_amd")
GOLDENS_2D = ["g2d_pgd_16", "g2d_pgd_16_bt", "g2d_pgd_16_plateau", "g2d_pgd_16_stop"]
GOLDENS_1D = ["g1d_pgd_32", "g1d_pgd_32_bt", "g1d_pgd_32_stop"]
TRK, TRM = 2.0 / (1.0 + 1e-12), 3.0 / (1.0 + 1e-12)      # the program feeds raw sums 4 and 9 over target norms of 1


@pytest.fixture(scope="session")
def replay_bin(tmp_path_factory):
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.fail("no C++ compiler: neither c++ on the path nor /opt/rocm/llvm/bin/clang++")
    out = str(tmp_path_factory.mktemp("pgd_replay") / "pgd_replay")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "pgd_replay_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def run(binary, text):
    r = subprocess.run([binary], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


class Traj:
    """A script: entry i = (round of the accept, accepted cost, relative control change); costs[0] is the start's."""

    def __init__(self, rule, alpha_max, costs, rounds, changes, stopped_at=-1):
        self.rule, self.alpha_max, self.stopped_at = rule, float(alpha_max), int(stopped_at)
        self.costs, self.rounds, self.changes, self.n = np.asarray(costs), np.asarray(rounds), np.asarray(changes), len(rounds)

    @classmethod
    def from_golden(cls, name):
        g = golden(name + ".npz")
        rule = "1d" if name.startswith("g1d") else "2d"
        counts = g["trials"] if rule == "1d" else g["attempts"]
        t = cls(rule, g["alpha_max"], g["costs"], counts - 1 if rule == "1d" else counts,
                g["changes"] if "changes" in g.files else np.ones(len(counts)),
                g["stopped_at"] if "stopped_at" in g.files else -1)
        t.alphas, t.counts = g["alphas"], counts
        return t

    def text(self, alpha0=0.0):
        head = f"{float(self.alpha_max).hex()} {float(alpha0).hex()} {float(self.costs[0]).hex()} {self.n}"
        return head + "".join(f" {int(r)} {float(c).hex()} {float(d).hex()}"
                              for r, c, d in zip(self.rounds, self.costs[1:], self.changes)) + "\n"


def replay(binary, rule, trajs, n_iters, n_calls=1, alpha0=None):
    """-> per call (iterations, rows {(b, it): (alpha_k, count, cost, done, alpha_prev)}, tracking [B][n_iters], terminal)."""
    text = f"{rule} {len(trajs)} {n_iters} {n_calls} {int(alpha0 is not None)}\n"
    text += "".join(t.text(alpha0[b] if alpha0 is not None else 0.0) for b, t in enumerate(trajs))
    calls, rows = [], {}
    for line in run(binary, text).splitlines():
        w = line.split()
        if w[0] == "row":
            rows[(int(w[1]), int(w[2]))] = (float(w[3]), int(w[4]), float(w[5]), int(w[6]), float(w[7]))
        elif w[0] == "call":
            assert w[4:] == ["errors", "1", "0"], line      # the histories answer to this call's n_iters and to no other
            calls.append((int(w[3]), rows, np.full((len(trajs), n_iters), -1.0), np.full((len(trajs), n_iters), -1.0)))
            rows = {}
        else:
            assert w[0] == "err", line
            calls[-1][2][int(w[1]), int(w[2])], calls[-1][3][int(w[1]), int(w[2])] = float(w[3]), float(w[4])
    assert len(calls) == n_calls
    return calls


@pytest.fixture(scope="session")
def single(replay_bin):
    """Each golden replayed alone, once: name -> (Traj, iterations, rows, tracking, terminal)."""
    out = {}
    for name in GOLDENS_2D + GOLDENS_1D:
        t = Traj.from_golden(name)
        out[name] = (t,) + replay(replay_bin, t.rule, [t], t.n)[0]
    return out


@pytest.mark.parametrize("name", GOLDENS_2D + GOLDENS_1D)
def test_single_trajectory_replays_golden(single, name):
    t, iters, rows, trk, trm = single[name]
    assert iters == t.n
    alpha_k = np.array([rows[(0, it)][0] for it in range(t.n)])
    counts = np.array([rows[(0, it)][1] for it in range(t.n)])
    cost = np.array([rows[(0, it)][2] for it in range(t.n)])
    done = np.array([rows[(0, it)][3] for it in range(t.n)])
    print(name, "alpha_k", alpha_k, "golden", t.alphas, "counts", counts, "done", done)
    assert np.array_equal(alpha_k, t.alphas)
    assert np.array_equal(counts, t.counts)
    if t.stopped_at < 0:
        assert not done.any()
    else:
        assert {"g2d_pgd_16_stop": 21, "g1d_pgd_32_stop": 11}[name] == t.stopped_at == t.n - 1
        assert not done[:t.stopped_at].any() and done[t.stopped_at] == 1
    # the stored cost is the accepted one, except that the 1D stop keeps the previous iterate's (G1:462-465)
    want = t.costs[1:].copy()
    if t.rule == "1d" and t.stopped_at >= 0:
        want[t.stopped_at] = t.costs[t.stopped_at]
    assert np.array_equal(cost, want)
    assert np.all(trk == TRK) and np.all(trm == TRM)


def test_plateau_golden_takes_the_boost_and_the_last_try(single):
    """What the plateau golden is there for, seen in the replay's books: an iteration that returns the last try (10 attempts,
    cost not below the previous one) and, after 5 plateau steps in a row, alpha_prev = min(alpha_max, 1.5 alpha_k)."""
    t, _, rows, _, _ = single["g2d_pgd_16_plateau"]
    ratios = [rows[(0, it)][4] / rows[(0, it)][0] for it in range(t.n) if rows[(0, it)][4] < t.alpha_max]
    assert any(r == 1.5 for r in ratios) and all(r == 1.5 or abs(r - 1.2) < 1e-15 for r in ratios), ratios
    assert any(t.counts[i] == 10 and t.costs[i + 1] >= t.costs[i] for i in range(t.n))
    t1, _, rows1, _, _ = single["g1d_pgd_32_stop"]
    assert any(rows1[(0, it)][4] == 2.0 * rows1[(0, it)][0] for it in range(t1.n))       # the 1D rule's boost


@pytest.mark.parametrize("rule, k_stop", [("1d", 11), ("2d", 21)])
def test_cost_stored_on_a_stop(replay_bin, rule, k_stop):
    """In the stop goldens the stopping iteration's cost equals the previous one bit for bit, so here is a script in which
    it does not: a strictly falling cost, the control at rest.  The rule stops at its first k past the threshold; the 1D
    rule keeps the previous iterate's cost in its books (G1:462-465), the 2D rule takes the new one."""
    costs = 1.0 - 0.01 * np.arange(k_stop + 2)
    t = Traj(rule, 50.0, costs, np.zeros(k_stop + 1, dtype=int), np.zeros(k_stop + 1))
    (iters, rows, _, _), = replay(replay_bin, rule, [t], k_stop + 5)
    assert iters == k_stop + 1
    assert [rows[(0, it)][3] for it in range(iters)] == [0] * k_stop + [1]
    assert rows[(0, k_stop - 1)][2] == costs[k_stop]
    assert rows[(0, k_stop)][2] == (costs[k_stop] if rule == "1d" else costs[k_stop + 1])


def test_batch_of_two_equals_single_replays(replay_bin, single):
    a, b = single["g2d_pgd_16_plateau"], single["g2d_pgd_16_stop"]
    (iters, rows, trk, _), = replay(replay_bin, "2d", [a[0], b[0]], 9)
    assert iters == 9 and len(rows) == 18
    for it in range(9):
        assert rows[(0, it)] == a[2][(0, it)]
        assert rows[(1, it)] == b[2][(0, it)]
    assert np.all(trk == TRK)


def test_batch_stops_when_every_trajectory_has(replay_bin, single):
    t = single["g2d_pgd_16_stop"][0]
    first, second = replay(replay_bin, "2d", [t, t], 30, n_calls=2)
    assert first[0] == 22 and sorted(first[1]) == [(b, it) for b in range(2) for it in range(22)]
    assert np.all(first[2][:, :22] == TRK) and np.all(first[3][:, :22] == TRM)
    assert np.isnan(first[2][:, 22:]).all() and np.isnan(first[3][:, 22:]).all()
    assert second[0] == 0 and not second[1] and np.isnan(second[2]).all()


def test_warm_start_is_capped_at_alpha_max(replay_bin, single):
    t = single["g2d_pgd_16_bt"][0]
    (_, rows, _, _), = replay(replay_bin, "2d", [t], t.n, alpha0=[2.0 * t.alpha_max])
    assert rows[(0, 0)][0] == t.alpha_max
    (_, rows, _, _), = replay(replay_bin, "2d", [t], t.n, alpha0=[0.25 * t.alpha_max])
    assert rows[(0, 0)][0] == 0.25 * t.alpha_max


OK = dict(b1=1.0, b2=1.0, b3=1e-3, ks=0.0, alpha_max=50.0, u_min="-inf", u_max="inf", has_alpha0=0, alpha0=0.0)


@pytest.mark.parametrize("change, message, weights", [
    (dict(), "ok", "ok"),                                                    # infinite bounds are legal
    (dict(b2="nan"), "b1, b2, b3 must be finite", "b1, b2, b3 must be finite"),
    (dict(b3="inf"), "b1, b2, b3 must be finite", "b1, b2, b3 must be finite"),
    (dict(ks=-1e-3), "kappa_sparsity must be finite and >= 0", "ok"),
    (dict(ks="inf"), "kappa_sparsity must be finite and >= 0", "ok"),
    (dict(alpha_max=0.0), "alpha_max must be > 0", "ok"),
    (dict(alpha_max="nan"), "alpha_max must be > 0", "ok"),
    (dict(u_min=1.0, u_max=-1.0), "u_min must be <= u_max", "ok"),
    (dict(u_max="nan"), "u_min must be <= u_max", "ok"),
    (dict(has_alpha0=1, alpha0=0.0), "alpha0 must be finite and > 0", "ok"),
    (dict(has_alpha0=1, alpha0="inf"), "alpha0 must be finite and > 0", "ok"),
    (dict(has_alpha0=1, alpha0=3.0), "ok", "ok"),
])
def test_validation_messages(replay_bin, change, message, weights):
    out = run(replay_bin, "check " + " ".join(str(v) for v in {**OK, **change}.values()) + "\n")
    assert out.splitlines() == ["check " + message, "weights " + weights]
