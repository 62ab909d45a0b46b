"""Stress polynomials for the lazy transforms: the classes they are made for, the seeds, the fixed-seed hill-climb on the
whole-transform model of tests/lazy_model.py, and the reader of the committed winners (tests/golden/lazy_stress_*.npz, written by
tests/golden/make_lazy_stress.py).

A fixture holds, per (n, op, goal), the NAME of the seed the climb started from and the few hundred coefficients it changed: the seeds
are re-derived at test time (they are cheap), only the searched part is stored.  The model is used to FIND inputs; what the GPU must
return for them is the oracle's word (tests/test_gpu_lazy_stress.py)."""
import functools
import os

import numpy as np

import lazy_inputs as li
import lazy_model as lm
import test_gpu_parity as tp

fz = li.fz
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPS = ("fwd", "inv", "mul")            # forward, inverse, forward -> (.) bhat -> inverse
GOALS = ("peak", "margin")             # largest value / 2^64; smallest cq - T and X + cq - Y
MODEL_SIZES = (2048, 4096)
SEED = 20261018
NRANDOM = 16
MAX_CHANGED = 256


@functools.lru_cache(None)
def entries():
    """[(name, q, hl, near)]: the tightest Barrett-exact modulus of every lazy class (the largest of tests/lazy_inputs.py; where that
    one is Barrett-inexact, and so runs the literal kernels, the next prime of the class below it) and the first modulus of every
    class form of KERNEL_FORMS (tests/test_gpu_parity.py)"""
    out = []
    names = dict(li.moduli())
    for hl, near in lm.probe_policy()[1]:
        if hl == lm.HL_LIT:
            continue
        q = names[("top-%d" if near else "general-top-%d") % (64 - hl if hl < 6 else 58)]
        while not (li.barrett_exact(q) and lm.class_of(q) == (hl, near)):
            q = li._prime_below(q)
        out.append(("tight-hl%d-%s" % (hl, "near" if near else "general"), q, hl, near))
    tight = {e[1] for e in out}
    for form in sorted(tp.KERNEL_FORMS):
        q = tp.KERNEL_FORMS[form][0][0]
        hl, near = lm.class_of(q)
        assert form == "hl%d-%s" % (hl, "near" if near else "general") and li.barrett_exact(q), form
        if q not in tight:                    # (the near-2^k forms of 59 to 62 bits ARE the tightest modulus of their class)
            out.append(("form-" + form, q, hl, near))
    return out


@functools.lru_cache(None)
def tables(q, n):
    return lm.Tables(q, fz.psi_for(q, n), n)


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) & 0xffffffff for k in key])


@functools.lru_cache(None)
def bhat(q, n):
    """the second operand of the product, in the transform domain: non-zero residues, every fourth one q - 1"""
    b = _rng(n, q, 99).integers(1, q, n, dtype=np.uint64)
    b[::4] = q - 1
    return b


def randoms(q, n, op):
    """the random polynomials of the seed family"""
    return _rng(n, q, OPS.index(op)).integers(0, q, (NRANDOM, n), dtype=np.uint64)


def model_free_seeds(q, n):
    """name -> polynomial: all q - 1, alternating 0 / q - 1, a single q - 1 at 0, 1, n/2, n - 1"""
    out = {"allmax": np.full(n, q - 1, dtype=np.uint64), "alt": np.array([0, q - 1] * (n // 2), dtype=np.uint64)}
    for nm, i in (("one@0", 0), ("one@1", 1), ("one@half", n // 2), ("one@last", n - 1)):
        out[nm] = np.zeros(n, dtype=np.uint64)
        out[nm][i] = q - 1
    return out


def _mask_stages(mask, logn):
    """the reducing stages (set mask bits), the last stage, and the transform's end"""
    return sorted({s for s in range(1, logn) if (mask >> s) & 1} | {logn - 1, logn})


def seeds(q, n, hl, near, op):
    """name -> thunk: the model-free seeds, the stage-state back-solves (the canonical state entering each reducing stage, the last
    stage and the end all q - 1, earlier stages inverted exactly in Python integers) and the random polynomials of the family"""
    tb = tables(q, n)
    pol = lm.probe_policy()[0][(tb.logn, hl)]
    top = [q - 1] * n
    out = {nm: (lambda a=a: a) for nm, a in model_free_seeds(q, n).items()}
    if op in ("fwd", "mul"):
        for s in _mask_stages(pol["fwd_mask"], tb.logn):
            out["fwd-state@%d" % s] = lambda s=s: lm.arr(lm.undo_forward_stages(top, tb, s))
    if op == "inv":
        for s in _mask_stages(pol["inv_mask"], tb.logn):
            out["inv-state@%d" % s] = lambda s=s: lm.arr(lm.undo_inverse_stages(top, tb, s))
    if op == "mul":                 # the product that enters the inverse's last stage as all q - 1: a = INTT(state / bhat)
        def through_product(s):
            st = lm.undo_inverse_stages(top, tb, s)
            st = [x * pow(int(b), q - 2, q) % q for x, b in zip(st, bhat(q, n))]
            return lm.arr(lm.undo_forward_stages(st, tb, tb.logn))
        for s in (tb.logn - 1, tb.logn):
            out["mul-inv-state@%d" % s] = lambda s=s: through_product(s)
    rnd = randoms(q, n, op)
    for i in range(NRANDOM):
        out["random%d" % i] = lambda i=i: rnd[i]
    return out


def evaluate(q, n, hl, near, op, a):
    """(peak in units of q, peak / 2^64, smallest margin in units of q) of the model; raises lm.Wrapped where something wraps"""
    _, tr = lm.run_model(op, a, bhat(q, n) if op == "mul" else None, tables(q, n), hl, near)
    return tr.peak_q, tr.peak, tr.margin


def _score(goal, peak_q, margin):
    return (peak_q, -margin) if goal == "peak" else (-margin, peak_q)


def search(q, n, hl, near, op, goal, budget):
    """fixed seed, fixed budget: the best seed, then a hill-climb that rewrites at most MAX_CHANGED of its coefficients.
    Returns (seed name, positions, values)."""
    rng = _rng(n, q, OPS.index(op), GOALS.index(goal), 7)
    best = None
    for nm, thunk in seeds(q, n, hl, near, op).items():
        a = lm.arr(thunk())
        pk, _, mg = evaluate(q, n, hl, near, op, a)
        if best is None or _score(goal, pk, mg) > best[0]:
            best = (_score(goal, pk, mg), nm, a)
    score, name, base = best
    cur = base.copy()
    for _ in range(budget):
        pos = rng.integers(0, n, int(rng.choice([1, 2, 4, 16])))
        kind = int(rng.integers(0, 4))
        cand = cur.copy()
        if kind == 0:
            cand[pos] = 0
        elif kind == 1:
            cand[pos] = q - 1
        elif kind == 2:
            cand[pos] = rng.integers(0, q, len(pos), dtype=np.uint64)
        else:
            cand[pos] = np.uint64(q - 1) - cand[pos]
        if int((cand != base).sum()) > MAX_CHANGED:
            continue
        pk, _, mg = evaluate(q, n, hl, near, op, cand)
        if _score(goal, pk, mg) > score:
            score, cur = _score(goal, pk, mg), cand
    pos = np.nonzero(cur != base)[0]
    return name, pos.astype(np.int32), cur[pos]


def fixture_path(name):
    return os.path.join(GOLDEN, "lazy_stress_%s.npz" % name)


@functools.lru_cache(None)
def _fixture(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def crafted(entry, n, op, goal):
    """the committed winner of (entry, n, op, goal): its seed, re-derived, with the searched coefficients written in"""
    name, q, hl, near = entry
    z = _fixture(name)
    key = "%d_%s_%s_" % (n, op, goal)
    a = lm.arr(seeds(q, n, hl, near, op)[str(z[key + "seed"])]()).copy()
    a[z[key + "pos"]] = z[key + "val"]
    return a


def crafted_set(entry, n, op):
    """what the GPU test runs at a model size: both winners of the op and the model-free seeds"""
    out = [crafted(entry, n, op, g) for g in GOALS]
    if op == "mul":                                   # (the forward's winners stress the product's first half as well)
        out += [crafted(entry, n, "fwd", g) for g in GOALS]
    return out + list(model_free_seeds(entry[1], n).values())


# both sides of the small-batch switch at every size (use_latency_path, kernels_fast_impl.cuh): the counts of BATCHES in
# tests/test_gpu_fuzz_moduli.py, and for the two sizes it leaves out the large count of the next size up (above T12M = 256, T14M = 176)
BATCHES = dict(fz.BATCHES)
BATCHES[4096] = BATCHES[8192]
BATCHES[16384] = BATCHES[32768]


def replicated_forward_state(q, psi, n, s):
    """the polynomial whose state in front of CT stage s (s <= 12) is all q - 1, without a size-n table: stages 0 .. s-1 are n / 2^s
    interleaved size-2^s transforms with psi^(n / 2^s) (table entry t < 2^s of the big table is entry t of the small one), all with the
    same input here, so the size-2^s back-solve is repeated n / 2^s times"""
    small = lm.Tables(q, pow(psi, n >> s, q), 1 << s)
    v = lm.arr(lm.undo_forward_stages([q - 1] * (1 << s), small, s))
    return np.repeat(v, n >> s)


def large_patterns(q, psi, n, hl, forward_exact, inverse_exact):
    """op -> polynomials for n >= 8192 (no model there): the model-free seeds, the whole-transform back-solves through the exact
    transforms handed in (the oracle's), and the forward stage-state back-solves of the reducing stages up to 12"""
    logn = n.bit_length() - 1
    top = np.full(n, q - 1, dtype=np.uint64)
    free = list(model_free_seeds(q, n).values())
    mask = lm.probe_policy()[0][(min(logn, 15), hl)]["fwd_mask"]
    fwd = free + [inverse_exact(top)] + [replicated_forward_state(q, psi, n, s) for s in range(1, 13) if (mask >> s) & 1]
    return {"fwd": fwd, "inv": free + [forward_exact(top)], "mul": fwd}
