"""BFV evaluator, hoisted Galois automorphisms: microseconds per call at n = 2^15, t = 1024, for count in {1, 16, 64} and G in {2, 8}
Galois elements, with BASELINE configs[4] (r = 4) and the reference demo's 16-prime set (r = 15).  Each new call next to the chain of
existing calls it replaces, measured in the same process, alternating baseline / new / baseline (the two baseline figures give the
run-to-run spread):
  - apply_galois_hoisted                against G x apply_galois;
  - galois_sum without weights          against G x apply_galois + (G - 1) x add;
  - galois_sum with weights             against G x (apply_galois + multiply_plain_ntt shared) + (G - 1) x add.
Next to each time ratio the transform-count ratio it is judged against: (r^2 + 2 r G) / (G (r^2 + 2 r)) and
(r^2 + 3 r) / (G (r^2 + 2 r)); the weighted baseline also runs multiply_plain_ntt's 4 r transforms per element: (r^2 + 3 r) / (G (r^2 + 6 r)).
Device events, 3 warm-up calls, at least --seconds of timed calls per point.  Prints one JSON line.

    python tools/bench_bfv_hoist.py [--seconds 0.3] [--counts 1,16,64] [--elements 2,8] [--configs configs4,demo16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ntt-cuda_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from ntt_cuda_amd import bfv  # noqa: E402
import params as P  # noqa: E402
from bench_bfv_eval import N, demo16, timed, uniform  # noqa: E402


def run_config(name, qs, psis, counts, elements, seconds):
    ctx = bfv.BFVContext(N, qs, psis, 1024, P.GAMMA61)
    ev = bfv.BFVEvaluator(ctx)
    R, r = len(qs), len(qs) - 1
    one_key = uniform(qs, R, 2 * r).reshape(-1)                 # a galois key's shape; its values do not change the work
    ksz = one_key.numel()
    out = []
    for G in elements:
        gs = [3, 5, 25, 2 * N - 1, N + 1, 125, 625, 3125][:G]
        keys = one_key.repeat(G)                    # G keys at G distinct addresses
        m = torch.randint(0, 1024, (G * N,), dtype=torch.int64, device="cuda")
        w = torch.empty(G * r * N, dtype=torch.int64, device="cuda")
        ev.plain_ntt(w, m, G)
        for count in counts:
            a = uniform(qs, R, 2 * count)
            c, x, acc = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
            c_out = torch.empty(G * a.numel(), dtype=torch.int64, device="cuda")
            scr = ev.scratch(count)

            def base(weighted, add):
                for k, g in enumerate(gs):
                    dst = acc if k == 0 else x
                    ev.apply_galois(dst, a, keys[k * ksz: (k + 1) * ksz], g, count, scratch=scr)
                    if weighted:
                        ev.multiply_plain_ntt(dst, dst, w[k * r * N: (k + 1) * r * N], count, True, scratch=scr)
                    if add and k:
                        ev.add(acc, acc, x, count)

            rows = (("hoisted", lambda: ev.apply_galois_hoisted(c_out, a, keys, gs, count, scratch=scr), lambda: base(False, False),
                     (r * r + 2 * r * G) / (G * (r * r + 2 * r))),
                    ("sum", lambda: ev.galois_sum(c, a, keys, gs, count, scratch=scr), lambda: base(False, True),
                     (r * r + 3 * r) / (G * (r * r + 2 * r))),
                    ("sum_weighted", lambda: ev.galois_sum(c, a, keys, gs, count, weights=w, scratch=scr), lambda: base(True, True),
                     (r * r + 3 * r) / (G * (r * r + 6 * r))))
            pt = dict(config=name, r=r, count=count, G=G, hoist_group=ev.hoist_group)
            for tag, new, old, transforms in rows:
                b1 = timed(old, seconds)
                t = timed(new, seconds)
                b2 = timed(old, seconds)
                b = 0.5 * (b1 + b2)
                pt[tag + "_us"] = round(t, 1)
                pt[tag + "_baseline_us"] = [round(b1, 1), round(b2, 1)]
                pt[tag + "_baseline_spread"] = round(abs(b1 - b2) / b, 4)
                pt[tag + "_ratio"] = round(t / b, 3)
                pt[tag + "_transform_ratio"] = round(transforms, 3)
            out.append(pt)
            del a, c, x, acc, c_out, scr
            torch.cuda.empty_cache()
        del keys, m, w
    for o in (ev, ctx):
        o.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--counts", default="1,16,64")
    ap.add_argument("--elements", default="2,8")
    ap.add_argument("--configs", default="configs4,demo16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    counts = [int(x) for x in args.counts.split(",")]
    elements = [int(x) for x in args.elements.split(",")]
    assert all(1 <= G <= 8 for G in elements)
    sets = {"configs4": (P.Q60 + [P.Q60_SPECIAL], P.PSI60 + [P.PSI60_SPECIAL]), "demo16": demo16()}
    res = []
    for name in args.configs.split(","):
        res += run_config(name, *sets[name], counts, elements, args.seconds)
    print(json.dumps(dict(bench="bfv_hoist", n=N, t=1024, points=res)))


if __name__ == "__main__":
    main()
