"""Parameter sets and crafted inputs of the BFV launch-layer sweep (tests/test_gpu_bfv_launch_edges.py on the GPU,
tests/test_bfv_launch_edges_host.py for what can be verified on the CPU).  Plain numpy / Python-integer code; every expected word of the
sweep comes from the oracle, the integer restatements here only PLACE operands and say which branch a placed word reaches.

The identity-key construction ("Launch-layer edge sweep"): the drivers take their key operand in the NTT domain, so a key of
all ones is the polynomial 1 and the transform section of a driver returns its other operand unchanged (on Barrett-exact moduli, word for
word).  The operand of every element-wise step is then the caller's, word by word:
  decrypt  sk_hat = 1: sum = c1 + c0, so c0 = sum - c1 places any sum, and sum = v (ptg ipq)^-1 places any value v in front of the rounding;
  encrypt  pk_hat = (1, 1): the tail sees u + e in every slot;
  keygen   sk = (1, 0, 0, ...), pk1 = NTT(w): poly_add_negate_xq sees w + e.
Crafted words sit at every index i with i mod 64 in {0, 1, 2, 3, 62, 63}: word 0, word n - 1, both sides of every 256-thread block boundary,
both words of a 16-byte lane, and at n = 2^15 the first and last lane of every wave in all 32 register rows of the fused product's threads
(register row r of thread t holds word 1024 r + t)."""
import math
from fractions import Fraction

import numpy as np

import bfv_sweep_inputs as SW
import params as P
from test_gpu_fuzz_moduli import STEP, barrett_margin, expected_class, is_prime, psi_for

M64 = (1 << 64) - 1
_CACHE = {}
GAMMA50 = (1 << 50) - 27
GAMMAS = (P.GAMMA40, GAMMA50, P.GAMMA61)


# ---- the two exactness predicates of hostparams.cpp as exact fractions / integers
def margin_operand_q(q):
    """bound of barrett_exact_for_operand_q: barrett_margin with q (q - 1) in place of (q - 1)^2"""
    k = q.bit_length()
    mu = (1 << (2 * k)) // q
    f = Fraction((1 << (2 * k)) % q, q)
    return Fraction(q, 1 << k) * Fraction(q - 1, 1 << k) * f + Fraction(mu, 1 << (k + 2))


def exact_single(q):
    return barrett_margin(q) < 1


def exact_operand_q(q):
    return margin_operand_q(q) < 1


def both_predicates_int(q):
    """(single-subtraction exact, exact with an operand q) over the common denominator 4 q 2^(2k): integers only, for the search"""
    k = q.bit_length()
    two2k = 1 << (2 * k)
    mu, rem = divmod(two2k, q)
    rhs = 4 * q * two2k - mu * q * (1 << k)
    return 4 * rem * (q - 1) * (q - 1) < rhs, 4 * rem * q * (q - 1) < rhs


def primes_below(top, count, modulus=STEP, exclude=()):
    """the first `count` primes q = 1 (mod modulus) below `top`, walking down, on which both predicates hold"""
    out = []
    k = (top - 2) // modulus
    while len(out) < count:
        q = k * modulus + 1
        assert q > top // 2, "ran out of candidates"
        if q not in exclude and is_prime(q) and all(both_predicates_int(q)):
            out.append(q)
        k -= 1
    return out


def c_predicates(q):
    """the two predicates as hostparams.cpp evaluates them: bound < 1.0L - 1e-9L.  Restated over the integers with the threshold 1 - 10^-9
    (the long-double rounding of the bound, about 2^-63, is below the 2^-k by which the two bounds differ, k <= 61)"""
    k = q.bit_length()
    two2k = 1 << (2 * k)
    mu, rem = divmod(two2k, q)
    rhs = (10 ** 9 - 1) * 4 * q * two2k - 10 ** 9 * mu * q * (1 << k)
    return 10 ** 9 * 4 * rem * (q - 1) * (q - 1) < rhs, 10 ** 9 * 4 * rem * q * (q - 1) < rhs


EPI_OFF_BUDGET = 200000


def search_epi_off_prime():
    """A prime = 1 (mod 2^17) on which barrett_single_subtraction_exact holds and barrett_exact_for_operand_q does not: EPI_OFF_BUDGET
    numbers = 1 (mod 2^17) drawn (fixed seed) from the top tenth of the 55- to 61-bit ranges (about one in twenty of them is prime), tested
    with the predicates as the driver evaluates them (c_predicates).  The two bounds differ by rem (q - 1) / (q 2^(2k)) < 2^-k, so a hit needs
    the first bound within 2^-55 of the threshold.  Returns (prime or None, candidates examined)."""
    if "epi_off" in _CACHE:
        return _CACHE["epi_off"]
    import random
    rng = random.Random(20261017)
    _CACHE["epi_off"] = (None, EPI_OFF_BUDGET)
    for i in range(EPI_OFF_BUDGET):
        k = rng.randrange(55, 62)
        q = rng.randrange(int((1 << k) * 0.9) // STEP, (1 << k) // STEP) * STEP + 1
        single, with_q = c_predicates(q)
        if single and not with_q and q.bit_length() == k and is_prime(q):
            _CACHE["epi_off"] = (q, i + 1)
            break
    return _CACHE["epi_off"]


def gamma_bits_agree(g):
    """the oracle's log2-based bit length (demo.cu:69) against the integer one"""
    return int(math.log2(float(g)) + 1) == g.bit_length()


# ---- the reference's Barrett (Algorithm 7, one conditional subtraction) in Python integers
def barrett(a, q):
    k = q.bit_length()
    mu = (1 << (2 * k)) // q
    s = ((((a >> (k - 2)) & M64) * mu) >> (k + 2)) & M64
    r = (a - s * q) & M64
    return r - q if r >= q else r


def reduce64_as_kernel(x, q):
    """reduce64 of kernels_bfv.hip as written; returns (result, conditional subtractions taken, remainder before them)"""
    m64 = M64 // q
    r = (x - ((x * m64) >> 64) * q) & M64
    first = r
    taken = 0
    for _ in range(2):
        if r >= q:
            r, taken = r - q, taken + 1
    return r, taken, first


class ParamSet:
    def __init__(self, name, n, qs, psis, t, gamma):
        self.name, self.n, self.t, self.gamma = name, int(n), int(t), int(gamma)
        self.qs, self.psis = [int(q) for q in qs], [int(w) for w in psis]
        self.R, self.r = len(qs), len(qs) - 1
        qs, r, g = self.qs, self.r, self.gamma
        Qt = [SW.product(q for j, q in enumerate(qs[:r]) if j != i) for i in range(r)]
        self.ptg = [t * g % q for q in qs[:r]]
        self.ipq = [pow(Qt[i] % qs[i], -1, qs[i]) for i in range(r)]
        self.k = [self.ptg[i] * self.ipq[i] % qs[i] for i in range(r)]                  # the one constant of epi_scale
        self.kinv = [pow(x, -1, q) for x, q in zip(self.k, qs)]
        self.bg = [Qt[i] % g for i in range(r)]
        self.neg_inv_gamma = g - pow(SW.product(qs[:r]) % g, -1, g)
        self.q_last, self.half_last = qs[r], qs[r] >> 1
        self.hm = [self.half_last % q for q in qs[:r]]
        self.iql = [pow(qs[r] % q, -1, q) for q in qs[:r]]
        self.qdt = [q // t for q in qs]
        self.lazy = 1 if any(q.bit_length() > g.bit_length() for q in qs[:r]) else max(1, (M64 - g) // (2 * g))

    def __repr__(self):
        return self.name

    # ---- the element-wise steps on one column, Python integers
    def scale(self, sums):
        """k_decrypt_scale on the sums (after `>`): the two literal Barrett products per slot"""
        return [barrett(barrett(s * self.ptg[i], q) * self.ipq[i], q) for i, (s, q) in enumerate(zip(sums, self.qs))]

    def round(self, v):
        """k_decrypt_round on the scaled values: (x0, x1, result).  q_i = 1 (mod t) makes every constant mod t one: x0 = -sum v_i"""
        g, mask = self.gamma, self.t - 1
        acc = 0
        for vi, b in zip(v, self.bg):
            acc = (acc + barrett(vi * b, g)) % g
        x0 = (-sum(v)) & mask & 0xffffffff
        x1 = barrett(acc * self.neg_inv_gamma, g)
        return x0, x1, ((x0 + g - x1) if x1 > g >> 1 else (x0 - x1)) & mask

    def tail(self, x, last, m, h):
        """k_encrypt_tail on one column of half h: x[j] = u + e of the ordinary slots, last = u + e of the special slot, all as 64-bit sums.
        Returns (words of the R slots, flags)"""
        ql, t, flags = self.q_last, self.t, set()
        if last == ql:
            flags.add("last==q")
        if last > ql:
            last -= ql
        last += self.half_last
        flags.add("half:wrap" if last >= ql else "half:stay")
        if last >= ql:
            last -= ql
        num = (m + ((t + 1) >> 1)) & M64
        fix = num // t
        out = []
        for j, q in enumerate(self.qs[:self.r]):
            xj = x[j]
            if xj == q:
                flags.add("sum==q")
            if xj > q:
                xj -= q
            tmp, taken, first = reduce64_as_kernel(last, q)
            assert tmp == last % q
            flags.add("tmp%shm" % ("<" if tmp < self.hm[j] else "=" if tmp == self.hm[j] else ">"))
            if tmp < self.hm[j]:
                tmp += q
            tmp -= self.hm[j]
            flags.add("x<tmp" if xj < tmp else "x==tmp" if xj == tmp else "x>tmp")
            if xj < tmp:
                xj += q
            xj = barrett((xj - tmp) * self.iql[j], q)
            if h == 0:
                term = m * self.qdt[j] + fix
                if term > M64:
                    flags.add("term-wraps")
                if xj + (term & M64) > M64:
                    flags.add("sum-wraps")
                xj = ((xj + term) & M64) % q
            out.append(xj)
        if h == 0:
            flags.add("fix>=2" if fix >= 2 else "fix=%d" % fix)
            if m + ((t + 1) >> 1) > M64:
                flags.add("numerator-wraps")
        return out + [last], flags


def positions(n):
    i = np.arange(n)
    return [int(x) for x in i[np.isin(i % 64, (0, 1, 2, 3, 62, 63))]]


def uniform(rng, q, size):
    return rng.integers(0, q, size=size, dtype=np.uint64)


def split_sum(rng, s, q):
    """canonical (a, b), a + b = s as integers (0 <= s <= 2 q - 2)"""
    a = int(rng.integers(max(0, s - (q - 1)), min(s, q - 1) + 1))
    return a, s - a


# ---- decryption
SUM_KINDS = ("0", "1", "q-1", "q", "q+1", "2q-2")
X1_KINDS = ("x1=0", "x1=half", "x1=half+1", "x1=gamma-1")
DEC_KINDS = tuple("sum=" + s for s in SUM_KINDS) + ("v=q-1",) + X1_KINDS          # 11 kinds against 6 residues mod 64: every pairing occurs


def sum_value(kind, q):
    return {"0": 0, "1": 1, "q-1": q - 1, "q": q, "q+1": q + 1, "2q-2": 2 * q - 2}[kind]


def x1_is_approximate(ps):
    """x1 = -(sum v_i bg_i) / Q mod gamma is solved for v_0 with the other slots random; the solution lies below q_0 with probability
    q_0 / gamma.  With one slot there is nothing to redraw, and with gamma 2^12 times q_0 the redraws do not end: such sets take the
    reachable x1 nearest the target on the target's side of gamma / 2 (every set of item 1 with r >= 2 is solved exactly)"""
    return ps.r == 1 or ps.gamma >> 12 > ps.qs[0]


def solve_x1(ps, target, rng):
    """scaled values v_i < q_i with x1 = target (see x1_is_approximate).  Returns (v, x1 reached)"""
    g, qs, r = ps.gamma, ps.qs, ps.r
    ninv = pow(ps.neg_inv_gamma, -1, g)
    b0inv = pow(ps.bg[0], -1, g)
    if x1_is_approximate(ps) and r > 1:
        best = None
        for _ in range(512):
            v = [int(rng.integers(0, q)) for q in qs[:r]]
            x1 = ps.round(v)[1]
            if (x1 > g >> 1) == (target > g >> 1) and (best is None or abs(x1 - target) < abs(best[1] - target)):
                best = (v, x1)
        return best
    step = 1 if target in (0, (g >> 1) + 1) else -1                      # move away from the compare, staying on the target's side
    for tries in range(200000):
        v = [0] + [int(rng.integers(0, q)) for q in qs[1:r]]
        x1 = (target + step * tries) % g if r == 1 else target
        need = (x1 * ninv - sum(barrett(vi * b, g) for vi, b in zip(v[1:], ps.bg[1:]))) % g
        v0 = need * b0inv % g
        if v0 < qs[0]:
            v0 += g * int(rng.integers(0, (qs[0] - 1 - v0) // g + 1))     # (any representative below q_0: operands wider than gamma)
            v[0] = v0
            return v, x1
    raise AssertionError("x1 = %d not reachable on %s" % (target, ps.name))


def craft_decrypt(ps, seed, kinds=DEC_KINDS):
    """c [2][R][n] and the placements [(position, kind, sums per slot)] for the identity key"""
    rng = np.random.default_rng(seed)
    n, r, g = ps.n, ps.r, ps.gamma
    c = np.stack([np.stack([uniform(rng, q, n) for q in ps.qs]) for _ in range(2)])
    targets = {"x1=0": 0, "x1=half": g >> 1, "x1=half+1": (g >> 1) + 1, "x1=gamma-1": g - 1}
    placed = []
    for j, p in enumerate(positions(n)):
        kind = kinds[j % len(kinds)]
        if kind.startswith("sum="):
            sums = [sum_value(kind[4:], q) for q in ps.qs[:r]]
        else:
            v = [q - 1 for q in ps.qs[:r]] if kind == "v=q-1" else solve_x1(ps, targets[kind], rng)[0]
            sums = [vi * ki % q for vi, ki, q in zip(v, ps.kinv, ps.qs)]
            sums = [s + q if rng.integers(0, 2) and s + q <= 2 * q - 2 else s for s, q in zip(sums, ps.qs)]   # (either side of the `>`)
        for i, (s, q) in enumerate(zip(sums, ps.qs)):
            c[1, i, p], c[0, i, p] = split_sum(rng, s, q)
        placed.append((p, kind, sums))
    return c, placed


def identity_key(ps, polys):
    return np.ones((polys, ps.n), dtype=np.uint64)


def decrypt_model(ps, sums):
    """(scaled values, x0, x1, result) of one column whose sums (before `>`) are given"""
    v = ps.scale([s - q if s > q else s for s, q in zip(sums, ps.qs)])
    return (v,) + ps.round(v)


# ---- encryption
def messages(t):
    h = (t + 1) >> 1
    return [0, t - 1, t, 2 * t - 1, 2 * t, 1 << 63, (1 << 64) - h - 1, (1 << 64) - h, (1 << 64) - 1]


ENC_KINDS = ("ord=q", "ord=q-1", "ord=q+1", "last=0", "last=1", "last=q-1", "last=q", "x=tmp-1", "x=tmp", "x=tmp+1")   # 10 against 9 messages


def craft_encrypt(ps, seed):
    """c [2][R][n] (the same u in both halves), e [2][R][n], m [n] and the placements [(position, kind)] for pk_hat = 1"""
    rng = np.random.default_rng(seed)
    n, R, r, ql = ps.n, ps.R, ps.r, ps.q_last
    u = np.stack([uniform(rng, q, n) for q in ps.qs])
    e = np.stack([np.stack([uniform(rng, 20, n) for _ in ps.qs]) for _ in range(2)])
    neg = rng.integers(0, 2, size=e.shape).astype(bool)
    for i, q in enumerate(ps.qs):                                          # small errors of both signs elsewhere
        e[:, i] = np.where(neg[:, i] & (e[:, i] > 0), np.uint64(q) - e[:, i], e[:, i])
    m = rng.integers(0, ps.t, size=n, dtype=np.uint64)
    wide = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    m[1::2] = wide[1::2]
    msgs = messages(ps.t)
    placed = []
    for j, p in enumerate(positions(n)):
        kind = ENC_KINDS[j % len(ENC_KINDS)]
        m[p] = msgs[j % len(msgs)]
        last = {"last=0": 0, "last=1": 1, "last=q-1": ql - 1, "last=q": ql}.get(kind)
        if last is None:
            last = int(rng.integers(0, 2 * ql - 1))
        a, b = split_sum(rng, last, ql)
        u[r, p] = a
        e[:, r, p] = b
        L = ((last - ql if last > ql else last) + ps.half_last) % ql
        for i, q in enumerate(ps.qs[:r]):
            tmp = (L % q - ps.hm[i]) % q
            if kind.startswith("ord="):
                s = sum_value(kind[4:], q)
            elif kind.startswith("x="):
                s = (tmp + {"x=tmp-1": -1, "x=tmp": 0, "x=tmp+1": 1}[kind]) % q
            else:
                s = int(rng.integers(0, 2 * q - 1))
            a, b = split_sum(rng, s, q)
            u[i, p] = a
            e[:, i, p] = b
        placed.append((p, kind))
    return np.stack([u, u]), e, m, placed


# ---- key generation
KEY_KINDS = ("0", "q-1", "q", "q+1", "random")


def craft_keygen(ps, seed):
    """w, e [R][n] with w + e on the edges of poly_add_negate_xq, and the placements; the caller passes sk = (1, 0, ...) and pk1 = NTT(w)"""
    rng = np.random.default_rng(seed)
    w = np.stack([uniform(rng, q, ps.n) for q in ps.qs])
    e = np.stack([uniform(rng, q, ps.n) for q in ps.qs])
    placed = []
    for j, p in enumerate(positions(ps.n)):
        kind = KEY_KINDS[j % len(KEY_KINDS)]
        if kind != "random":
            for i, q in enumerate(ps.qs):
                w[i, p], e[i, p] = split_sum(rng, sum_value(kind, q), q)
        placed.append((p, kind))
    return w, e, placed


KEY_NTT_KINDS = ("0", "q-1", "q", "q+1", "2q-2", "a=0", "random")


def craft_keygen_ntt(ps, seed, e_hat=None):
    """The key generation of an exact context runs in the NTT domain: k_keygen_pk0 forms a_hat s_hat + NTT(e) word by word.  With
    s_hat = NTT((1, 0, ...)) = 1 its sum is a_hat[i] + e_hat[i], so the edges are placed on the transforms: a_hat (= pk1, any words below q)
    and e_hat [R][n] with a_hat + e_hat on the edges of `>=` and of `ra != q`; the caller passes e = INTT(e_hat).  With e_hat given (the
    exact transform of an e of the caller's), only a_hat is chosen: the sums a target leaves reachable with a_hat < q.
    Returns (a_hat, e_hat, [(position, kind, sums per slot)])"""
    rng = np.random.default_rng(seed)
    fixed = e_hat is not None
    a = np.stack([uniform(rng, q, ps.n) for q in ps.qs])
    eh = e_hat.copy() if fixed else np.stack([uniform(rng, q, ps.n) for q in ps.qs])
    placed = []
    for j, p in enumerate(positions(ps.n)):
        kind = KEY_NTT_KINDS[j % len(KEY_NTT_KINDS)]
        sums = []
        for i, q in enumerate(ps.qs):
            if kind == "random":
                pass
            elif kind == "a=0":
                a[i, p] = 0
            elif fixed:
                s = sum_value(kind, q)
                if 0 <= s - int(eh[i, p]) < q:
                    a[i, p] = s - int(eh[i, p])
            else:
                a[i, p], eh[i, p] = split_sum(rng, sum_value(kind, q), q)
            sums.append(int(a[i, p]) + int(eh[i, p]))
        placed.append((p, kind, sums))
    return a, eh, placed


def delta_key(ps):
    sk = np.zeros((ps.R, ps.n), dtype=np.uint64)
    sk[:, 0] = 1
    return sk


# ---- parameter sets
def lowered(psis, qs, n_from, n):
    return [pow(w, n_from // n, q) for w, q in zip(psis, qs)]


def q62(n):
    qs = [q for q, _ in P.Q62_N4096]
    return qs, lowered([w for _, w in P.Q62_N4096], qs, 4096, n)


def small_primes():
    """two 40-bit and one 25-bit prime = 1 (mod 2^17), the first below 2^40 / 2^25 on which both predicates hold"""
    if "small" not in _CACHE:
        _CACHE["small"] = primes_below(1 << 40, 2, exclude=(P.GAMMA40,)) + primes_below(1 << 25, 1)
    return _CACHE["small"]


def with_roots(qs, n):
    return qs, [psi_for(q, n) for q in qs]


CLASS_SPECS = (("6-general", 3 << 56, (6, False), True), ("6-near", 1 << 58, (6, True), True), ("5-near", 1 << 59, (5, True), True),
               ("4-near", 1 << 60, (4, True), True), ("3-near", 1 << 61, (3, True), True), ("4-general", 3 << 58, (4, False), False),
               ("3-general", 3 << 59, (3, False), False), ("2-general", 3 << 60, (2, False), False))


SINGLE_NAMES = ("n2048-R2-40+62-t2-g40", "n2048-R16-demo-t1024-g61", "n2048-R6-62bit-t1024-g50", "n2048-R3-61bit-t2^31-g61", "n4096-R6-62bit-t2^17-g40",
                "n4096-R6-62bit-t1024-g61", "n4096-R4-61bit-t2^31-g50", "n4096-R16-demo-t2-g61", "n4096-R4-40+40+25+62-t2^17-g50",
                "n4096-R3-40+40+62-t1024-g40", "n65536-R2-59+61-t1024-g61")
LITERAL_NAMES = ("kat1-n4096", "inexact60+exact60+inexact61-n2048")
CLASS_NAMES = tuple("class-" + spec[0] for spec in CLASS_SPECS)


def single_sets():
    """item 1 (built on first use: the test modules parametrise over the names above)"""
    if "single" in _CACHE:
        return _CACHE["single"]
    p40a, p40b, p25 = small_primes()
    e59, e61, e62 = (P.EDGE_PRIMES[b][0] for b in (59, 61, 62))
    wide = lambda n, r: SW.wide_subset(n, r, exact_single)
    S = [
        ParamSet("n2048-R2-40+62-t2-g40", 2048, *with_roots([p40a, e62], 2048), 2, P.GAMMA40),
        ParamSet("n2048-R16-demo-t1024-g61", 2048, *SW.demo_subset(2048, 15), 1024, P.GAMMA61),
        ParamSet("n2048-R6-62bit-t1024-g50", 2048, *q62(2048), 1024, GAMMA50),
        ParamSet("n2048-R3-61bit-t2^31-g61", 2048, *wide(2048, 2), 1 << 31, P.GAMMA61),
        ParamSet("n4096-R6-62bit-t2^17-g40", 4096, *q62(4096), 1 << 17, P.GAMMA40),
        ParamSet("n4096-R6-62bit-t1024-g61", 4096, *q62(4096), 1024, P.GAMMA61),
        ParamSet("n4096-R4-61bit-t2^31-g50", 4096, *wide(4096, 3), 1 << 31, GAMMA50),
        ParamSet("n4096-R16-demo-t2-g61", 4096, *SW.demo_subset(4096, 15), 2, P.GAMMA61),
        ParamSet("n4096-R4-40+40+25+62-t2^17-g50", 4096, *with_roots([p40a, p40b, p25, e62], 4096), 1 << 17, GAMMA50),
        ParamSet("n4096-R3-40+40+62-t1024-g40", 4096, *with_roots([p40a, p40b, e62], 4096), 1024, P.GAMMA40),
        ParamSet("n65536-R2-59+61-t1024-g61", 65536, [e59, e61], [P.EDGE_PRIMES[b][1][65536] for b in (59, 61)], 1024, P.GAMMA61),
    ]
    assert tuple(ps.name for ps in S) == SINGLE_NAMES
    _CACHE["single"] = S
    return S


def literal_sets():
    """item 2: the KAT-1 moduli (decryption_test.cu) and a set of INEXACT_PRIMES next to an EXACT_NEIGHBOURS prime"""
    from test_barrett_exactness import KAT_PSI, KAT_Q
    n = 2048
    qs = [P.INEXACT_PRIMES[60][0], P.EXACT_NEIGHBOURS[60][0], P.INEXACT_PRIMES[61][0]]
    psis = [P.INEXACT_PRIMES[60][1][n], P.EXACT_NEIGHBOURS[60][1][n], P.INEXACT_PRIMES[61][1][n]]
    return [ParamSet("kat1-n4096", 4096, KAT_Q, KAT_PSI, 1024, P.GAMMA61), ParamSet("inexact60+exact60+inexact61-n2048", n, qs, psis, 1024, P.GAMMA61)]


def class_sets():
    """item 4: R = 2 at n = 2^15, both primes of one kernel class: (set, class, whether k_polymul15_epi holds the epilogue for it).
    Near-2^k primes: the first below 2^k; general primes: the first below 3/4 2^k (2^k - q = 2^(k-2), far above the 2^24 of `near`)."""
    if "class" not in _CACHE:
        out = []
        for name, top, cls, fused in CLASS_SPECS:
            qs = primes_below(top, 2)
            assert expected_class(qs) == cls, (name, qs)
            out.append((ParamSet("class-" + name, 32768, *with_roots(qs, 32768), 1024, P.GAMMA61), cls, fused))
        _CACHE["class"] = out
    return _CACHE["class"]


def epi_off_set():
    """item 5: the set of item 4 on the prime search_epi_off_prime found (next to the first prime of its bit length), or None"""
    q, _ = search_epi_off_prime()
    if q is None:
        return None
    qs = [q, primes_below(1 << q.bit_length(), 1, exclude=(q,))[0]]
    return ParamSet("class-epi-off", 32768, *with_roots(qs, 32768), 1024, P.GAMMA61), expected_class(qs), False


# Batches of item 4 in polynomials num = count R, R = 2, from kernels_fast_impl.cuh / kernels_fast.hip / kernels.hpp:
#   use_latency_path<15>(num, fused = true): num <= 176 (lat_threshold), or 256 < num <= 384      -> the small-batch kernels, k_lat_inv_a_epi
#   otherwise one persistent launch (k_polymul15_epi where epi_class() holds, else the two-step path)
#   tail_split_head: CUs = 256; num > 256, num % 256 != 0 and a tail num - 256 floor(num / 256) <= kTailSplitMaxFused = 100 cut the call
#   into a head of 256 floor(num / 256) polynomials (> 176, <= 256: persistent) and the tail (small-batch kernels)
# count = 1, 3: num = 2, 6 (small batch); count = 100: num = 200 (persistent, no cut); count = 150: num = 300 = 256 + 44, cut between
# ciphertexts 127 and 128.
BATCH_COUNTS = (1, 3, 100, 150)
CUT_AT = 128


PLAIN_POOL = 37          # random ciphertexts the others of a batch cycle through: a prime above the tail's 22 ciphertexts, coprime to 128, 150, 256


def crafted_slots(count):
    """ciphertexts of a batch that are crafted: first, last, and both sides of the cut"""
    return sorted({0, count - 1} | ({CUT_AT - 1, CUT_AT} if count > CUT_AT else set()))
