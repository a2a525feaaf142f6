"""Regenerates the qualified inputs of tests/_fix_band.py: `python tests/_fix_band_search.py GRID [seed [seconds]]`, GRID one
of the keys below.  Not a test and not imported by one.

Qualification is narrow (the plateau sits 2e-3 above the band's threshold and no node of a front's tail may land within
10 |s_n| of it), so the constants in _fix_band.INPUTS are draws of this random search that met fb.is_qualified, printed
with "OK".  It has to be re-run when the oracle's march changes (Newton tolerance, relaxation): the tests assert the
premises, so a disqualified input fails test_band_inputs_meet_their_premises and is replaced by a line printed here.
Search space, uniform: fronts in {1, 2, 3}; wig in {0, 0.02, 0.05, 0.1}; width in [0.015, 0.07]; off in [0, 1 / Nx); control
amplitude in {1, 5, 20}; relaxation steps in {0, 2, 4}.  About 5 % of the draws qualify on 32 x 16 and 12 x 9, 0.5 % on
50 x 36 and 128 x 32 (a few minutes each); prefer a draw with large min |s_n| and, where there is one, wig > 0."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the repository root, for `oracle`
import _fix_band as fb  # noqa: E402

GRIDS = {
    "32x16": (dict(Nx=32, Ny=16, Lx=1.0, Ly=0.5), 3),
    "128x32": (dict(Nx=128, Ny=32, Lx=1.0, Ly=0.5), 3),
    "50x36": (dict(Nx=50, Ny=36, Lx=1.3, Ly=0.9), 3),
    "12x9": (dict(Nx=12, Ny=9, Lx=1.3, Ly=0.9), 2),
}


def search(grid, seed=1, seconds=240.0):
    kw, M = GRIDS[grid]
    rng = np.random.default_rng(seed)
    end = time.time() + seconds
    while time.time() < end:
        draw = (kw, int(rng.choice([1, 2, 3])), float(rng.choice([0.0, 0.02, 0.05, 0.1])), float(rng.uniform(0.015, 0.07)),
                float(rng.uniform(0.0, 1.0 / kw["Nx"])), float(rng.choice([1.0, 5.0, 20.0])), int(rng.choice([0, 2, 4])), M)
        fb.INPUTS["draw"] = draw
        fb._CACHE.pop("draw", None)
        m = fb.build("draw")
        q = fb.qualify(m)
        if fb.is_qualified(q):
            print("OK", grid, draw[1:], f"min|s| {q['min_shift']:.1e} in {q['frac_in']:.2f} max|phi_c| {q['max_phi_c']:.5f}",
                  flush=True)


if __name__ == "__main__":
    search(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1, float(sys.argv[3]) if len(sys.argv) > 3 else 240.0)
