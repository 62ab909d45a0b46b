"""BFV evaluator throughput: microseconds per mi355ntt_bfv_multiply_relin call at n = 2^15 for count in {1, 16, 64}, with BASELINE
configs[4] (4 x 60-bit + special, r = 4) and the reference demo's 16-prime set (r = 15), next to the same call's transforms alone (the same batches
through forward_batch / inverse_batch on contexts over Q and B_sk), measured in the same process.  Device events, 3 warm-up calls, at
least --seconds of timed calls per point.  Prints one JSON line.

    python tools/bench_bfv_eval.py [--seconds 0.5] [--counts 1,16,64]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ntt-cuda_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ntt_cuda_amd as ntt  # noqa: E402
from ntt_cuda_amd import bfv  # noqa: E402
import params as P  # noqa: E402

N = 32768


def demo16():
    """the reference demo's 16-prime set (demo.cu:35-36), as bench.py carries it"""
    from bench import DEMO_PSI16, DEMO_Q16
    return list(DEMO_Q16), list(DEMO_PSI16)


def timed(fn, seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, total_ms = 1, 0.0
    while True:
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        total_ms = s.elapsed_time(e)
        if total_ms >= seconds * 1e3:
            return total_ms * 1e3 / reps
        reps = max(reps * 2, int(reps * seconds * 1.2e3 / max(total_ms, 1e-3)))


def uniform(qs, polys_per_prime_group, groups):
    """[groups][len(qs)][n] uniform residues, on the device"""
    rng = np.random.default_rng(1)
    return ntt.to_device(np.stack([np.stack([rng.integers(0, q, size=N, dtype=np.uint64) for q in qs]) for _ in range(groups)]))


def run_config(name, qs, psis, counts, seconds):
    ctx = bfv.BFVContext(N, qs, psis, 1024, P.GAMMA61)
    ev = bfv.BFVEvaluator(ctx)
    R, r = len(qs), len(qs) - 1
    bs, ps = bfv.aux_primes(N, r)
    assert bs == ev.aux_primes
    cq = ntt.NTTContext(N, qs[:r], psis[:r])
    cb = ntt.NTTContext(N, bs, ps)
    rlk = uniform(qs, R, 2 * r)
    out = []
    for count in counts:
        a, b = uniform(qs, R, 2 * count), uniform(qs, R, 2 * count)
        c = torch.empty_like(a)
        scr = ev.scratch(count)
        us_call = timed(lambda: ev.multiply_relin(c, a, b, rlk, count, scratch=scr), seconds)
        xq = uniform(qs[:r], r, 4 * count)
        xb = uniform(bs, r + 1, 4 * count)
        dg = uniform(qs[:r], r, count * r)

        def transforms():
            cq.forward_batch(xq, 4 * count * r, r)
            cb.forward_batch(xb, 4 * count * (r + 1), r + 1)
            cq.inverse_batch(xq, 3 * count * r, r)
            cb.inverse_batch(xb, 3 * count * (r + 1), r + 1)
            cq.forward_batch(dg, count * r * r, r)
            cq.inverse_batch(xq, 2 * count * r, r)

        us_ntt = timed(transforms, seconds)
        n_transforms = count * (4 * r + 4 * (r + 1) + 3 * r + 3 * (r + 1) + r * r + 2 * r)
        out.append(dict(config=name, r=r, count=count, us_per_call=round(us_call, 1), us_per_ciphertext=round(us_call / count, 2),
                        us_transforms_alone=round(us_ntt, 1), transforms_per_call=n_transforms,
                        elementwise_share=round(max(0.0, 1 - us_ntt / us_call), 3),
                        bsk_kernel_class=ntt.lib().mi355ntt_ctx_kernel_class(cb._h), q_kernel_class=ntt.lib().mi355ntt_ctx_kernel_class(cq._h)))
        del a, b, c, scr, xq, xb, dg
        torch.cuda.empty_cache()
    for o in (cq, cb, ev, ctx):
        o.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--counts", default="1,16,64")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    counts = [int(x) for x in args.counts.split(",")]
    res = run_config("configs4", P.Q60 + [P.Q60_SPECIAL], P.PSI60 + [P.PSI60_SPECIAL], counts, args.seconds)
    res += run_config("demo16", *demo16(), counts, args.seconds)
    print(json.dumps(dict(bench="bfv_multiply_relin", n=N, t=1024, points=res)))


if __name__ == "__main__":
    main()
