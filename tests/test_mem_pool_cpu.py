"""The allocation pool of the engines (csrc/vch_mem.h: owner pointers, release, mark / rollback, the groups built on them
and the two process-wide diagnostics vch_mem_live / vch_mem_refuse_after) over a mock runtime, without a device.

tests/mem_pool_main.cpp includes the header and hands the pool a function table built on malloc / free that keeps its own
books: what it handed out, what came back and in which order, and how often it was called.  The program is compiled once per
session with the address and undefined-behaviour sanitizers and run as an ordinary child process; every check is on the
mock's books, none on a leak report at exit."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "sparse-optimal-control-of-viscous-chan-hilliard-via-gradient-descent--1d-2d_amd")


@pytest.fixture(scope="session")
def pool_bin(tmp_path_factory):
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.fail("no C++ compiler: neither c++ on the path nor /opt/rocm/llvm/bin/clang++")
    out = str(tmp_path_factory.mktemp("mem_pool") / "mem_pool")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "mem_pool_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.mark.parametrize("case, what", [
    (1, "twelve mixed allocations, release: each block freed once, newest first, owners NULL, live 0, second release idle"),
    (2, "the same twelve with request k refused, k = 0..11, then the teardown of a failed create: live 0, no foreign free"),
    (3, "a group of three behind a mark after two earlier blocks: refuse member 0, 1, 2; the earlier blocks stay; retry"),
    (4, "a refusal is for one request, and a negative count disarms"),
])
def test_pool(pool_bin, case, what):
    r = subprocess.run([pool_bin, str(case)], capture_output=True, text=True, timeout=60)
    print(what, "->", r.stdout.strip(), r.stderr.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == [f"ok {case}"]
