"""Moduli and crafted operands that drive the lazy primitives of csrc/ntt_core.cuh to the edges of their promised ranges
(tests/test_lazy_bounds_host.py proves on the CPU what each set reaches; tests/test_gpu_lazy_primitives.py runs them on the GPU)."""
import functools
import random

import numpy as np

import lazy_model as lm
import test_gpu_fuzz_moduli as fz

STEP = fz.STEP
BITS = (50, 55, 58, 59, 60, 61, 62)
M64 = lm.M64


def _prime_below(start):
    m = (start - 2) // STEP          # (strictly below start)
    while not fz.is_prime(m * STEP + 1):
        m -= 1
    return m * STEP + 1


@functools.lru_cache(None)
def moduli():
    """[(name, q)]: per bit length the largest prime = 1 (mod 2^17) (tightest headroom of its class, near 2^k), the largest one
    that fails the near-2^k test, one from the lower tenth of the range; the near-in / near-out threshold primes of
    test_gpu_fuzz_moduli.py; two Barrett-inexact primes (lit_barrett_mul, class HL_LIT)"""
    out = []
    for k in BITS:
        top = _prime_below(1 << k)
        assert lm.consts(top)["near_ok"]
        q = _prime_below((1 << k) - (1 << 24) + 2 * STEP)       # (k >= 50: only delta < 2^24 binds)
        while lm.consts(q)["near_ok"]:
            q = _prime_below(q)
        low = _prime_below((1 << (k - 1)) + (1 << (k - 1)) // 10)
        assert low.bit_length() == k and q.bit_length() == k
        out += [("top-%d" % k, top), ("general-top-%d" % k, q), ("low-%d" % k, low)]
    thr = fz.threshold_primes()
    out += [(nm, q) for nm, q in thr if nm.startswith("near-")]
    out += [(nm, q) for nm, q in thr if nm.startswith("barrett-inexact")]
    seen, uniq = set(), []
    for nm, q in out:                 # (a threshold prime may be the largest general prime of its bit length: once)
        if q not in seen:
            seen.add(q)
            uniq.append((nm, q))
    return uniq


def barrett_exact(q):
    return fz.barrett_margin(q) < 1


def classes_for(q):
    """every instantiated (HL, NEAR) this modulus may run in (a mixed context takes the weakest class of its primes); the lazy
    classes only for Barrett-exact moduli (the others run class HL_LIT), class HL_LIT for 34 ... 61 bits"""
    hl, near = min(64 - q.bit_length(), 6), lm.consts(q)["near_ok"]
    out = []
    if barrett_exact(q):
        out += [(h, nr) for h, nr in lm.probe_policy()[1] if h != lm.HL_LIT and h <= hl and (near or not nr)]
    if 34 <= q.bit_length() <= 61:
        out.append((lm.HL_LIT, False))
    return out


def bounds_of_class(hl):
    """(forward bounds, inverse bounds, final forward bound, final inverse bound) in units of q that the policy produces for class
    hl over n = 2^11 .. 2^16 -- every B with values in [0, B q)"""
    fwd, inv = {1, 2}, {1, 2}
    ff = fi = 0
    for logn in range(11, 16):
        pol = lm.probe_policy()[0][(logn, hl)]
        tq = pol["tq"]
        for start in (1, 2):                         # 2: the lower half behind the n = 2^16 coupling stage
            B = start
            fwd.add(1 + tq)
            for s in range(logn):
                if (pol["fwd_mask"] >> s) & 1:
                    B = 2
                B += tq
                fwd.add(B)
            ff = max(ff, B)
        B = 1
        for s in range(logn):
            cm = pol["cmul"][s]
            inv |= {2 * B, B + cm}
            Bn = max(2 * B, tq)
            if (pol["inv_mask"] >> s) & 1:
                Bn = max(tq, 2)
            B = Bn
        fi = max(fi, B)
    return sorted(fwd), sorted(inv), ff, fi


def _fit(xs):
    return sorted({x for x in xs if 0 <= x <= M64})


def around_multiples(q, mmax, limit=M64 + 1):
    """m q - {0, 1, 2} and m q + {0, 1} for m = 0 .. mmax, inside [0, limit)"""
    out = set()
    for m in range(mmax + 1):
        out |= {m * q - 2, m * q - 1, m * q, m * q + 1}
    return sorted(x for x in out if 0 <= x < min(limit, M64 + 1))


def w_corners(q):
    return [1, 2, q - 1, q // 2, (q + 1) // 2]


def y_corners(q, hl):
    fwd, inv, _, _ = bounds_of_class(hl)
    return _fit([0, 1, q - 1, q, 2 * q - 1, 2 * q, 4 * q - 1, M64] + [B * q - 1 for B in fwd + inv])


def reduce_domain(q):
    """reduce_2q: [0, B q) with B q <= 2^64 and B <= 66"""
    return min(66, (1 << 64) // q)


@functools.lru_cache(None)
def searched(q, seed=20261018, draws=40000):
    """fixed-seed search with the classification code: operands (y, w) of mul_shoup4m for every (quotient error, band) met, operands of
    mul_shoup2 for both bands, x of reduce_2q for both outcomes of the estimate"""
    rng = np.random.default_rng(seed ^ (q & 0xffffffff))
    out = {"shoup4m": {}, "shoup2": {}, "reduce": {}}
    hl = min(64 - q.bit_length(), 6)
    # y: 64-bit words, words just below 2^64, lazy words below B q; w: residues
    ys = np.concatenate([rng.integers(0, 1 << 64, draws, dtype=np.uint64), np.uint64(M64) - rng.integers(0, 1 << 40, draws, dtype=np.uint64),
                         rng.integers(0, min(4 * q, M64), draws, dtype=np.uint64)])
    ws = rng.integers(1, q, len(ys), dtype=np.uint64)
    err, band, wp = lm.classify_shoup4m(ys, ws, q)
    for e, b, y, w in zip(err.tolist(), band.tolist(), ys.tolist(), ws.tolist()):
        lst = out["shoup4m"].setdefault((e, b), [])
        if len(lst) < 4:
            lst.append((y, w))
    r2 = lm.w_mul_shoup2(ys, ws, wp, q) // np.uint64(q)
    for b, y, w in zip(r2.tolist(), ys.tolist(), ws.tolist()):
        lst = out["shoup2"].setdefault(b, [])
        if len(lst) < 4:
            lst.append((y, w))
    c = lm.consts(q)
    xs = lm.arr(around_multiples(q, reduce_domain(q), reduce_domain(q) * q))
    xs = np.concatenate([xs, rng.integers(0, min(reduce_domain(q) * q, M64), draws, dtype=np.uint64)])
    e, r = lm.w_reduce_2q(xs, c)
    exact = e == xs // np.uint64(q)
    for ok, x, rr in zip(exact.tolist(), xs.tolist(), r.tolist()):
        key = "exact" if ok else ("one-less" if q <= rr < 2 * q else "other")
        lst = out["reduce"].setdefault(key, [])
        if len(lst) < 8:
            lst.append(x)
    return out


def mul_tuples(q, hl, with_base, seed=1, fill=1536):
    """(y, w, base) for the Shoup products: the corners of the domain, the searched operands, random fill over a pool of twiddles"""
    rnd = random.Random(seed * 1000003 + q % 1000003)
    tq = lm.tq_of(hl if hl else 2)
    fwd, inv, _, _ = bounds_of_class(hl)
    bases = [0]
    if with_base:
        bases = _fit([0, 2 * q - 1] + [(B - tq) * q - 1 for B in fwd if B > tq])
    T = [(y, w, b) for y in y_corners(q, hl) for w in w_corners(q) for b in bases]
    s = searched(q)
    for key in ("shoup4m", "shoup2"):
        for lst in s[key].values():
            T += [(y, w, bases[i % len(bases)]) for i, (y, w) in enumerate(lst)]
    pool = [rnd.randrange(1, q) for _ in range(16)]
    for i in range(fill):
        y = rnd.getrandbits(64) if i % 2 else rnd.randrange(0, min(4 * q, M64))
        T.append((y, pool[i % 16], bases[i % len(bases)] if i % 3 else rnd.randrange(0, min(2 * q, M64))
                  if with_base else 0))
    return T


def by_workgroup(T, block=lm.BLOCK):
    """tuples regrouped so that every workgroup of `block` tuples shares one twiddle (the TWS forms): ([(y, base)], [w per group])"""
    groups = {}
    for y, w, b in T:
        groups.setdefault(w, []).append((y, b))
    yb, W = [], []
    for w in sorted(groups):
        g = groups[w]
        for i in range(0, len(g), block):
            chunk = g[i:i + block]
            chunk = chunk + [chunk[0]] * (block - len(chunk))
            yb += chunk
            W.append(w)
    return yb, W


def reduce_inputs(q, seed=2, fill=1024):
    rnd = random.Random(seed * 1000003 + q % 1000003)
    B = reduce_domain(q)
    xs = set(around_multiples(q, B, B * q))
    for lst in searched(q)["reduce"].values():
        xs |= set(lst)
    xs |= {rnd.randrange(0, min(B * q, M64 + 1)) for _ in range(fill)}
    return sorted(xs)


def near_inputs(q, seed=3, fill=1024):
    """reduce_2q_near takes ANY 64-bit word: the multiples of q, x >> k at its maximum with x mod 2^k = 2^k - 1 (2^64 - 1), the top of
    every 2^k block"""
    rnd = random.Random(seed * 1000003 + q % 1000003)
    k = q.bit_length()
    xs = set(around_multiples(q, (1 << 64) // q if (1 << 64) // q < 80 else 80))
    xs |= {M64, M64 - 1, (1 << 64) - (1 << k), (1 << 64) - (1 << k) - 1, (1 << k) - 1, (1 << k), ((1 << 64) // q) * q - 1}
    top = (1 << (64 - k)) - 1
    xs |= {(e << k) | ((1 << k) - 1) for e in (top, top - 1, top // 2, 1, 0)} | {(e << k) for e in (top, 1)}
    xs |= {rnd.getrandbits(64) for _ in range(fill)}
    return _fit(xs)


def fold_inputs(q, seed=4, fill=1024):
    """mul_fold_near: x < 2q, b < 2^k"""
    rnd = random.Random(seed * 1000003 + q % 1000003)
    k = q.bit_length()
    X = [0, 1, q - 1, q, q + 1, 2 * q - 2, 2 * q - 1]
    Bs = [0, 1, q - 1, q, (1 << k) - 1, (1 << k) - 2, q // 2, (1 << (k - 1))]
    T = [(x, b) for x in X for b in Bs]
    T += [(rnd.randrange(0, 2 * q), rnd.randrange(0, 1 << k)) for _ in range(fill)]
    # high F: Phi at its largest and P mod 2^k large -- x = 2q - 1 and b close to 2^k
    T += [(2 * q - 1, (1 << k) - 1 - i) for i in range(64)] + [(2 * q - 1 - i, (1 << k) - 1) for i in range(64)]
    return T


def lit_inputs(q, seed=5, fill=2048):
    """lit_barrett_mul / barrett_mul: any 64-bit y against table entries w < q; canonical pairs (where a Barrett-inexact modulus
    leaves q + r now and then)"""
    rnd = random.Random(seed * 1000003 + q % 1000003)
    T = [(y, w) for y in y_corners(q, min(64 - q.bit_length(), 6)) for w in w_corners(q)]
    T += [(rnd.randrange(0, q), rnd.randrange(0, q)) for _ in range(fill)]
    T += [(q - 1 - rnd.randrange(0, 1 << 20), q - 1 - rnd.randrange(0, 1 << 20)) for _ in range(fill)]
    T += [(rnd.getrandbits(64), rnd.randrange(0, q)) for _ in range(fill // 4)]
    return T


def canon_inputs(q, hl, near, forward, seed=6, fill=512):
    """words in front of canon_after_forward / canon_after_inverse of class (hl, near)"""
    rnd = random.Random(seed * 1000003 + q % 1000003 + hl)
    if hl == lm.HL_LIT:
        return _fit([0, 1, q - 1, q, q + 1, 2 * q - 1, M64] + [rnd.getrandbits(64) for _ in range(fill)])
    _, _, ff, fi = bounds_of_class(hl)
    if forward:
        B = ff
    elif near and hl > 2:
        B = max(fi, 2 * max(lm.probe_policy()[0][(15, hl)]["cmul"]))     # (a fold takes whatever the last sum leaves)
    else:
        B = lm.tq_of(hl)
    B = min(B, (1 << 64) // q)
    return sorted(set(around_multiples(q, B, B * q)) | {rnd.randrange(0, B * q) for _ in range(fill)})


def fused_inputs(q, hl, near, seed=7, fill=1024):
    rnd = random.Random(seed * 1000003 + q % 1000003 + hl)
    if hl == lm.HL_LIT:            # barrett_batch on what the literal forward left behind: canonical words, or q + r
        X = [0, 1, q - 1, q, q + 1, 2 * q - 1]
        B = 2
    else:
        B = min(bounds_of_class(hl)[2], (1 << 64) // q)
        X = around_multiples(q, B, B * q)
    Bs = [0, 1, 2, q - 1, q - 2, q // 2, (q + 1) // 2]
    T = [(x, b) for x in X for b in Bs]
    T += [(rnd.randrange(0, B * q), rnd.randrange(0, q)) for _ in range(fill)]
    return T


def records_for(q):
    """the probe records of one modulus: [(op, hl, near, consts, arrays)] and, in step, the operand tuples the contracts take"""
    c = lm.consts(q)
    hl = min(64 - q.bit_length(), 6)
    recs, tuples = [], []

    def add(op, arrays, tup, h=None, nr=None):
        recs.append((op, h, nr, c, arrays))
        tuples.append(tup)

    lit = lit_inputs(q)
    wide = [(y, w) for y, w in lit] + [(M64, M64), (M64, 1), (1 << 32, 1 << 32), ((1 << 32) - 1, (1 << 32) + 1), (0, M64)]
    for op in ("mul_hi", "mul_wide"):
        add(op, [[a for a, _ in wide], [b for _, b in wide]], wide)
    add("barrett_mul", [[a for a, _ in lit], [b for _, b in lit]], lit)
    if 34 <= c["k"] <= 61:
        add("lit_barrett_mul", [[a for a, _ in lit], [b for _, b in lit]], lit)
    T = mul_tuples(q, hl, False)
    full = [(y, w, lm.shoup(w, q), b) for y, w, b in T]
    for op in ("shoup_mul_lazy", "mul_shoup2", "mul_shoup4m"):
        add(op, [[t[0] for t in full], [t[1] for t in full], [t[2] for t in full]], full)
    yb, W = by_workgroup(T)
    tw = [(y, W[i // lm.BLOCK], lm.shoup(W[i // lm.BLOCK], q), 0) for i, (y, _) in enumerate(yb)]
    add("mul_shoup4m_tws", [[y for y, _ in yb], W, [lm.shoup(w, q) for w in W]], tw)
    Tb = mul_tuples(q, hl, True)
    fullb = [(y, w, lm.shoup(w, q), b) for y, w, b in Tb]
    add("mul_shoup4m_acc", [[t[0] for t in fullb], [t[1] for t in fullb], [t[2] for t in fullb], [t[3] for t in fullb]], fullb)
    yb, W = by_workgroup(Tb)
    tw = [(y, W[i // lm.BLOCK], lm.shoup(W[i // lm.BLOCK], q), b) for i, (y, b) in enumerate(yb)]
    add("mul_shoup4m_acc_tws", [[y for y, _ in yb], [b for _, b in yb], W, [lm.shoup(w, q) for w in W]], tw)
    xs = reduce_inputs(q)
    add("reduce_2q", [xs], [(x,) for x in xs])
    if c["near_ok"]:
        xs = near_inputs(q)
        add("reduce_2q_near", [xs], [(x,) for x in xs])
        fo = fold_inputs(q)
        add("mul_fold_near", [[x for x, _ in fo], [b for _, b in fo]], fo)
    for h, nr in classes_for(q):
        for op, fwd in (("canon_fwd", True), ("canon_inv", False)):
            xs = canon_inputs(q, h, nr, fwd)
            add(op, [xs], [(x,) for x in xs], h, nr)
        fu = fused_inputs(q, h, nr)
        add("fused_mul", [[x for x, _ in fu], [b for _, b in fu]], fu, h, nr)
    return recs, tuples
