#!/usr/bin/env python3
"""Search the stress polynomials of the lazy transforms and write them as fixtures.

For every entry of tests/lazy_stress.py (the class forms of KERNEL_FORMS and the tightest modulus of every lazy class), at n = 2048 and
4096, for forward, inverse and forward -> (.) bhat -> inverse, and for both goals (largest value / 2^64, smallest margin): take the best
seed (model-free patterns, stage-state back-solves, the random polynomials of the family) and hill-climb on at most 256 coefficients with
a fixed seed and a fixed budget of model runs.  A model run that wraps 2^64 or goes negative stops the search: that is a finding.

Output: tests/golden/lazy_stress_<entry>.npz -- per (n, op, goal) the seed's name, the rewritten positions and their values, and the
peak (units of q and of 2^64) and margin the model showed (recorded results; tests/test_lazy_bounds_host.py re-runs the model).

Usage: python tests/golden/make_lazy_stress.py [budget per search at n = 2048, default 120; n = 4096 takes half of it]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lazy_stress as ls  # noqa: E402


def main():
    budget = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    for name, q, hl, near in ls.entries():
        out = {"q": np.uint64(q), "hl": np.int32(hl), "near": np.int32(near)}
        for n in ls.MODEL_SIZES:
            for op in ls.OPS:
                for goal in ls.GOALS:
                    seed, pos, val = ls.search(q, n, hl, near, op, goal, budget if n == 2048 else budget // 2)
                    a = ls.seeds(q, n, hl, near, op)[seed]().copy()
                    a[pos] = val
                    pk, p64, mg = ls.evaluate(q, n, hl, near, op, a)
                    key = "%d_%s_%s_" % (n, op, goal)
                    out.update({key + "seed": np.str_(seed), key + "pos": pos, key + "val": val,
                                key + "result": np.array([pk, p64, mg])})
                    print("%-20s n=%d %s %-6s seed %-18s changed %3d  peak %.3f q = %.4f * 2^64  margin %.3g q"
                          % (name, n, op, goal, seed, len(pos), pk, p64, mg), flush=True)
        np.savez_compressed(ls.fixture_path(name), **out)


if __name__ == "__main__":
    main()
