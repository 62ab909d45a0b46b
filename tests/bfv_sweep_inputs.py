"""Parameter sets and crafted inputs of the BFV evaluator sweep (tests/test_gpu_bfv_eval_sweep.py on the GPU, tests/test_bfv_eval_sweep_host.py
for what can be verified on the CPU).  Everything here is exact Python-integer arithmetic written from the definitions of DESIGN.md,
"BFV evaluation"; nothing reads the library's folded constants.

  - prime search: 61-bit primes q = 1 (mod M) on which the reference's Barrett is exact, by a walk down from 2^61 whose start a seed fixes;
    wide_subset: r + 1 of them, the set the crafted inputs run on (Q about as large as B);
  - extension inputs: one coefficient x (as residues) whose small Montgomery factor r_m = -(sum_i tmp_i Q/q_i) Q^-1 mod 2^32 is a
    chosen word, tmp_i = [x_i m~ (Q/q_i)^-1]_{q_i}, m~ = 2^32;
  - rescale inputs: with the second operand b = (1, 0) the tensor coefficients are the extended a0 and a1, so integers 0, 1, Q - 1,
    floor(Q/2), ceil(Q/2), ceil(kQ/t) + {-1, 0, 1} and a plane of q_i - 1 put t D / Q on and next to integers with both signs of D; a
    ciphertext pair of constant floor(Q/2) polynomials gives the largest tensor coefficients (about n Q^2 / 2) of both signs;
  - relinearization inputs: a third component holding 0, q_i (which reads as 0), q_i - 1 and min(q) - 1 in every slot, and a key of
    q_j - 1 in every word: the largest 128-bit sums;
  - rescale_trace: the integers D, t D mod Q, y and the Shenoy-Kumaresan correction the model's multiply goes through, to assert
    that the crafted inputs reach what they were built to reach.
Ciphertext batches are numpy uint64 arrays [comp][count][R][n], the special prime's slot R - 1 last."""
import numpy as np

MT = 1 << 32
RM_TARGETS = (0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1)
_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)


def is_prime(n):
    """deterministic Miller-Rabin below 3.3e24 (the first twelve primes as bases)"""
    if n < 2:
        return False
    for p in _BASES:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in _BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def find_psi(q, n):
    """a primitive 2n-th root of unity mod q: the first x^((q - 1) / 2n), x = 2, 3, ..., whose n-th power is -1"""
    for x in range(2, 1000):
        w = pow(x, (q - 1) // (2 * n), q)
        if pow(w, n, q) == q - 1:
            return w
    raise AssertionError("no root found for %d" % q)


def primes61(count, modulus, barrett_is_exact, seed, exclude=()):
    """`count` primes q = 1 (mod modulus) in [2^60, 2^61), Barrett-exact (so that the model can use the C oracle's transforms), walking
    down from 2^61 - modulus * (seed-chosen offset); descending"""
    rng = np.random.default_rng(seed)
    k = (1 << 61) // modulus - 1 - int(rng.integers(0, 1 << 12))
    out = []
    while len(out) < count:
        q = k * modulus + 1
        assert q > (1 << 60), "ran out of 61-bit candidates"
        if q not in exclude and is_prime(q) and barrett_is_exact(q):
            out.append(q)
        k -= 1
    return out


def demo_subset(n, r):
    """the first r + 1 primes of the reference demo's 16-prime set (the last of them the special prime), roots raised to 32768 / n"""
    from bench import DEMO_PSI16, DEMO_Q16
    qs = list(DEMO_Q16[: r + 1])
    return qs, [pow(w, 32768 // n, q) for w, q in zip(DEMO_PSI16, qs)]


_WIDE = {}


def wide_subset(n, r, barrett_is_exact):
    """the first r + 1 of sixteen 61-bit primes = 1 (mod 2^31) (so = 1 (mod 2n) and (mod t) for every accepted n and t), with a root
    each.  They lie 2^31 and more below 2^61, under every auxiliary candidate, and within 2^-17 of it: Q is about B, so that
    y = floor(t D / Q) - alpha exceeds B and the Shenoy-Kumaresan correction takes both signs at every r.  The demo set's 55-bit primes
    leave Q below B / 2^(6 r) and cannot reach a negative correction from r = 4 on"""
    if not _WIDE:
        _WIDE["qs"] = primes61(16, 1 << 31, barrett_is_exact, 77)
    qs = _WIDE["qs"][: r + 1]
    return qs, [find_psi(q, n) for q in qs]


def product(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


def crt_int(res, mods):
    M = product(mods)
    x = 0
    for v, m in zip(res, mods):
        Mi = M // m
        x += (int(v) * pow(Mi % m, -1, m) % m) * Mi
    return x % M


def residues(x, mods):
    return [int(x) % m for m in mods]


# ---- the BEHZ size condition ("BFV evaluation"): qs the r primes of Q, bs the r + 1 primes of B_sk, m_sk last
def size_condition_bits(n, t, qs, bs):
    """sum bits(q_i) + log2 n + log2 t + 3 <= sum (bits(b_j) - 1), the form creation checks"""
    return sum(int(q).bit_length() for q in qs) + (n.bit_length() - 1) + (int(t).bit_length() - 1) + 3 <= sum(int(b).bit_length() - 1 for b in bs)


def size_condition_exact(n, t, qs, bs):
    """4 n t Q + 2 (r + 1) B < B m_sk"""
    Q, B = product(qs), product(bs[:-1])
    return 4 * n * t * Q + 2 * (len(qs) + 1) * B < B * int(bs[-1])


# ---- extension
def craft_extend(qs, target, rng):
    """residues x_0 .. x_{r-1} of one coefficient with r_m = target.  x_0 .. x_{r-2} are random; tmp_{r-1} gets the low 32 bits that
    make sum_i tmp_i (Q/q_i) = -target Q (mod 2^32) (Q/q_{r-1} is odd) and random high bits below q_{r-1}; x_{r-1} follows from it"""
    r, Q = len(qs), product(qs)
    x = [int(rng.integers(0, q)) for q in qs[:-1]]
    s = 0
    for xi, q in zip(x, qs[:-1]):
        Qi = Q // q
        s += (xi * MT % q) * pow(Qi % q, -1, q) % q * Qi
    q = qs[-1]
    Ql = Q // q
    lo = (-target * Q - s) * pow(Ql % MT, -1, MT) % MT
    tmp = lo + MT * int(rng.integers(0, (q - 1 - lo) // MT + 1))
    assert tmp < q
    c = MT % q * pow(Ql % q, -1, q) % q                       # tmp = x c mod q
    x.append(tmp * pow(c, -1, q) % q)
    return x


# ---- rescale
def rescale_values(qs, t):
    """(label, integer in [0, Q)) for the steerable tensor coefficients.  ceil(kQ/t) - 1 is the largest D with floor(t D / Q) = k - 1 and
    t D mod Q = Q - k (Q = 1 mod t); ceil(kQ/t) has t D mod Q = t - k.  k = 1 and k = t - 1 put t D mod Q at Q - 1 and at 1"""
    Q = product(qs)
    vals = [("0", 0), ("1", 1), ("Q-1", Q - 1), ("floor(Q/2)", Q // 2), ("ceil(Q/2)", (Q + 1) // 2)]
    for k in sorted({1, 2, t // 2 - 1, t // 2, t // 2 + 1, t - 2, t - 1} - {0, t}):
        c = -((-k * Q) // t)
        for d in (-1, 0, 1):
            vals.append(("ceil(%dQ/t)%+d" % (k, d), (c + d) % Q))
    return vals


def crafted_operands(qs_all, t, n, seed):
    """a, b [2][4][R][n] and the placements.  Ciphertext 0: random words with the extension cases in all four components; 1: the rescale
    values in a, b = (1, 0); 2: a = planes of q_i - 1, b = (1, 0); 3: every coefficient of all four components floor(Q/2).
    Returns (a, b, ext) with ext a list of (operand 'a'/'b', component, position, target)"""
    rng = np.random.default_rng(seed)
    R, r = len(qs_all), len(qs_all) - 1
    qs = [int(q) for q in qs_all[:r]]
    Q = product(qs)
    uni = lambda: np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs_all])
    a = np.stack([np.stack([uni() for _ in range(4)]) for _ in range(2)])
    b = np.stack([np.stack([uni() for _ in range(4)]) for _ in range(2)])
    ext = []
    for name, op in (("a", a), ("b", b)):
        for h in range(2):
            pos = [0, n - 1, 255, 256] + [int(p) for p in rng.choice(np.arange(1, n - 1), 3 * len(RM_TARGETS), replace=False)]
            pos = list(dict.fromkeys(pos))[: 3 * len(RM_TARGETS)]
            for k, p in enumerate(pos):
                target = RM_TARGETS[k % len(RM_TARGETS)]
                x = craft_extend(qs, target, rng)
                for i in range(r):
                    op[h, 0, i, p] = x[i]
                ext.append((name, h, p, target))
    # ciphertext 1: integers drawn below Q (both signs once centred) with the special values at two positions per component
    vals = rescale_values(qs, t)
    for h in range(2):
        ints = [int.from_bytes(rng.bytes((Q.bit_length() + 7) // 8 + 8), "little") % Q for _ in range(n)]
        pos = [0, n - 1] + [int(p) for p in rng.choice(np.arange(1, n - 1), 2 * len(vals) - 2, replace=False)]
        for k, p in enumerate(pos):
            ints[p] = vals[k % len(vals)][1]
        for i, q in enumerate(qs):
            a[h, 1, i] = np.array([x % q for x in ints], dtype=np.uint64)
    for z in (1, 2):
        b[:, z, :r] = 0
        b[0, z, :r, 0] = 1
    for i, q in enumerate(qs):
        a[:, 2, i] = q - 1
        a[:, 3, i] = (Q // 2) % q
        b[:, 3, i] = (Q // 2) % q
    return a, b, ext


def rescale_trace(M, a, b):
    """EvalModel.multiply of one ciphertext pair (a, b [2][R][n]) and what it goes through.  Returns (out, trace): out the model's
    product [3][R][n], trace per component the integer arrays D (the tensor coefficient, taken from the model's own centred CRT while
    it multiplies, so nothing is computed twice), tdq = t D mod Q, y = floor(t D / Q) - alpha and alpha_sk = (conv_B(y) - y) / B.
    The caller checks y mod q_i against out"""
    seen = []
    crt = M.crt

    def spy(res, mods, centred=False):
        x = crt(res, mods, centred)
        if centred:
            seen.append(x)
        return x

    M.crt = spy
    try:
        out = M.multiply(a, b)
    finally:
        del M.crt
    assert len(seen) == 3
    t, Q = M.t, M.Q
    base = M.bs[:-1]
    B = product(base)
    q_w = [(q, Q // q, pow(Q // q % q, -1, q)) for q in M.qs]
    b_w = [(bj, B // bj, pow(B // bj % bj, -1, bj)) for bj in base]
    trace = []
    for D in seen:
        tdq = (t * D) % Q
        conv = sum(((tdq % q) * inv % q) * Qi for q, Qi, inv in q_w)
        y = (t * D) // Q - (conv - tdq) // Q
        conv_b = sum(((y % bj) * inv % bj) * Bj for bj, Bj, inv in b_w)
        assert not np.any((conv_b - y) % B)
        trace.append(dict(D=D, tdq=tdq, y=y, alpha_sk=(conv_b - y) // B))
    return out, trace


# ---- relinearization
def floor_half_pair(qs_all, n):
    """a, b [2][1][R][n]: every coefficient of all four components floor(Q/2).  The tensor coefficients are (2k + 2 - n) floor(Q/2)^2
    and its double: both signs, up to n Q^2 / 2"""
    r = len(qs_all) - 1
    Q = product(qs_all[:r])
    a = np.zeros((2, 1, r + 1, n), dtype=np.uint64)
    for i, q in enumerate(qs_all[:r]):
        a[:, :, i] = (Q // 2) % int(q)
    return a, a.copy()


def crafted_relin(qs_all, n, seed):
    """c3 [3][1][R][n]: random first two components, the third cycling 0, q_i, q_i - 1, min(q) - 1 through the coefficients of every
    slot (shifted by the slot index, so that every combination across slots occurs); rlk [r][2][R][n] of q_j - 1 in every word"""
    rng = np.random.default_rng(seed)
    R, r = len(qs_all), len(qs_all) - 1
    qs = [int(q) for q in qs_all[:r]]
    c3 = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs_all]) for _ in range(3)]).reshape(3, 1, R, n)
    lo = min(qs)
    k = np.arange(n)
    for i, q in enumerate(qs):
        pat = np.array([0, q, q - 1, lo - 1], dtype=np.uint64)
        c3[2, 0, i] = pat[((k >> (2 * (i % 5))) + i) & 3]
    rlk = np.zeros((r, 2, R, n), dtype=np.uint64)
    for j, q in enumerate(qs):
        rlk[:, :, j] = q - 1
    return c3, rlk
