"""Crafted inputs of the BFV evaluator's key, plaintext and Galois edge sweep (tests/test_gpu_bfv_galois_edges.py on the GPU,
tests/test_bfv_galois_edges_host.py for what can be verified on the CPU).  Plain numpy / Python integers written from the definitions
of include/mi355ntt.h and DESIGN.md; nothing reads the library's folded constants.  None of these inputs is an encryption: they are
words chosen to reach a branch or a bound.

  - gather set: one ciphertext whose two components hold 0, 1, q_i - 1, q_i (which reads as 0) and q_i - 2 on coefficients that
    tau_g negates and on coefficients it does not, for every g of galois_elements(n);
  - peak sets: x^0-only polynomials.  tau_g fixes x^0 and the transform of c x^0 is c in every slot, so with keys of q_j - 1 in every
    word the NTT-domain inner products are the same number in every slot and for every g: the largest one (first set), or one that
    reduces to q_j - 1 (second set), which a weight of q_j - 1 then multiplies;
  - key set: secret key and uniform part as NTT-domain words drawn from {0, 1, q_j - 1}, every pair in every prime slot, errors
    c x^0 with c from the same three: a s + e = 0 (mod q) by both routes, and the largest a s + e;
  - plain set: c0 words on the wrap points of c0 +/- E(m) crossed with m on the boundaries of the encoding and of the centred lift;
  - mixed_width_set: a 30-bit prime among 61-bit ones, where the digit lift red64(x, q_j) has a quotient of about 2^31.
Ciphertexts are numpy uint64 arrays [comp][count][R][n]; the special prime's slot R - 1 holds SENT in every array built here."""
import numpy as np

from bfv_sweep_inputs import find_psi, is_prime, wide_subset

SENT = 0x5A5A5A5A5A5A5A5A           # tests/test_gpu_bfv_eval.py's sentinel word
GATHER_STRIDE = 3                   # coprime to the five values: position 3 p holds value (p + slot + component) mod 5
SUM_ELEMS = 17                      # galois_sum at r = 1, 2: more than one inner-product launch (kHoistSumChunk = 16)


def galois_elements(n):
    """the elements of the gather set: the identity (nothing negated), the smallest rotation, +/- 1 around n and the two largest
    (2n - 1 negates every coefficient but x^0)"""
    return [1, 3, n - 1, n + 1, 2 * n - 3, 2 * n - 1]


def five_values(q):
    return [0, 1, q - 1, q, q - 2]


def negated(n, g):
    """bool [n]: tau_g(x^i) = x^(g i mod 2n) has its sign flipped (exponent >= n)"""
    return (int(g) * np.arange(n, dtype=np.int64)) % (2 * n) >= n


def _uniform(rng, qs_all, n):
    x = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs_all])
    x[-1] = SENT
    return x


def gather_set(qs_all, n, seed):
    """a [2][1][R][n]: random words below q_i; every GATHER_STRIDE-th coefficient of component h, slot i holds
    five_values(q_i)[(p + i + h) mod 5], p the running index"""
    rng = np.random.default_rng(seed)
    r = len(qs_all) - 1
    a = np.stack([_uniform(rng, qs_all, n) for _ in range(2)]).reshape(2, 1, r + 1, n)
    pos = np.arange(0, n, GATHER_STRIDE)
    for h in range(2):
        for i in range(r):
            which = (np.arange(pos.size) + i + h) % 5
            a[h, 0, i, pos] = np.array(five_values(int(qs_all[i])), dtype=np.uint64)[which]
    return a


def _x0(values, n):
    """[len(values)][n]: values[i] x^0"""
    x = np.zeros((len(values), n), dtype=np.uint64)
    x[:, 0] = np.array(values, dtype=np.uint64)
    return x


def widest_min(qs):
    """the smallest of the primes of the largest width: min(q) where all have one width"""
    top = max(int(q).bit_length() for q in qs)
    return min(int(q) for q in qs if int(q).bit_length() == top)


def peak_set(qs_all, n):
    """c [2][1][R][n]: c0 = (q_j - 1) x^0, c1 = (min(q_i, qmin) - 1) x^0 with qmin = widest_min (qmin - 1 in every residue where
    the primes have one width).  Every digit lifts to (c1_i mod q_j) in every NTT slot, c0hat to q_j - 1"""
    qs = [int(q) for q in qs_all[:-1]]
    lo = widest_min(qs)
    c = np.full((2, 1, len(qs_all), n), SENT, dtype=np.uint64)
    c[0, 0, :-1] = _x0([q - 1 for q in qs], n)
    c[1, 0, :-1] = _x0([min(q, lo) - 1 for q in qs], n)
    return c


def peak_set_unit(qs_all, n):
    """c [2][1][R][n] whose inner products with the top keys reduce to q_j - 1: c0 = 0, c1 = 1 x^0 in slot 0 and 0 in the other slots
    (one digit of 1: with 1 x^0 in every slot the r digits would sum to r, and r (q_j - 1) = q_j - r)"""
    r = len(qs_all) - 1
    c = np.full((2, 1, r + 1, n), SENT, dtype=np.uint64)
    c[:, 0, :r] = 0
    c[1, 0, 0, 0] = 1
    return c


def top_keys(qs_all, n, G):
    """[G][r][2][R][n]: q_j - 1 in every Q-slot word of both halves"""
    r = len(qs_all) - 1
    k = np.full((G, r, 2, r + 1, n), SENT, dtype=np.uint64)
    for j, q in enumerate(qs_all[:r]):
        k[:, :, :, j] = int(q) - 1
    return k


def random_keys(qs_all, n, G, seed):
    rng = np.random.default_rng(seed)
    r = len(qs_all) - 1
    return np.stack([np.stack([np.stack([_uniform(rng, qs_all, n) for _ in range(2)]) for _ in range(r)]) for _ in range(G)])


def constant_message(n, c, count=1):
    """[count][n]: the plaintext c x^0"""
    m = np.zeros((count, n), dtype=np.uint64)
    m[:, 0] = c
    return m


def sum_elements(n, G):
    """G Galois elements with repeats, as the hoisted tests list them"""
    base = [3, n + 1, 3, 2 * n - 1, 5, 25, 2 * n - 3, 1, 5]
    return (base * (G // len(base) + 1))[:G]


# ---- key set
def key_values(q):
    return [0, 1, q - 1]


def key_set(qs_all, n, shift):
    """(sk_hat [R][n], a [r][R][n], e [r][R][n]).  Slot j of the secret key holds key_values(q_j)[k mod 3] at word k, of the uniform
    part of key part i key_values(q_j)[(k // 3 + i) mod 3]: all nine pairs in every slot of every part.  e_i = c x^0 with
    c = key_values(q_j)[(i + shift) mod 3], whose transform is c in every slot: shift = 0, 1, 2 give every part every c"""
    r = len(qs_all) - 1
    k = np.arange(n)
    sk = np.full((r + 1, n), SENT, dtype=np.uint64)
    a = np.full((r, r + 1, n), SENT, dtype=np.uint64)
    e = np.full((r, r + 1, n), SENT, dtype=np.uint64)
    for j, q in enumerate(qs_all[:r]):
        v = np.array(key_values(int(q)), dtype=np.uint64)
        sk[j] = v[k % 3]
        for i in range(r):
            a[i, j] = v[(k // 3 + i) % 3]
            e[i, j] = 0
            e[i, j, 0] = v[(i + shift) % 3]
    return sk, a, e


# ---- plain set
PLAIN_WORDS = ("0", "1", "q-1", "q", "E", "q-E", "E-1", "q-E+1")


def plain_messages(t):
    return [0, 1, t // 2 - 1, t // 2, t - 1, t, t + 3, (1 << 64) - 1]


def encode(m, q, t):
    """E(m) of include/mi355ntt.h for one prime: m floor(q / t) + floor((m + (t + 1) / 2) / t), m taken mod t"""
    m = int(m) % t
    return m * (q // t) + (m + (t + 1) // 2) // t


def plain_words(m, q, t):
    """the eight c0 words for the plaintext word m, in the order of PLAIN_WORDS: the wrap points of add_mod(c0, E) (c0 = q - E
    gives 0, one less stays below q) and of sub_mod(c0, E) (c0 = E gives 0, one less wraps).  E - 1 and q - E + 1 are taken mod q
    where E = 0 puts them outside [0, q]"""
    E = encode(m, q, t)
    assert 0 <= E < q
    return [0, 1, q - 1, q, E, q - E, (E - 1) % q, (q - E + 1) % q]


def plain_set(qs_all, n, t, seed):
    """(a [2][1][R][n], m [1][n]): random words, with the 64 pairs (word kind w, message u) at coefficients 8 w + u and again at
    n - 64 + 8 w + u (another block of the grid)"""
    rng = np.random.default_rng(seed)
    r = len(qs_all) - 1
    a = np.stack([_uniform(rng, qs_all, n) for _ in range(2)]).reshape(2, 1, r + 1, n)
    m = rng.integers(0, t, size=(1, n), dtype=np.uint64)
    ms = plain_messages(t)
    for base in (0, n - 64):
        for w in range(8):
            for u in range(8):
                m[0, base + 8 * w + u] = ms[u]
                for j, q in enumerate(qs_all[:r]):
                    a[0, 0, j, base + 8 * w + u] = plain_words(ms[u], int(q), t)[w]
    return a, m


# ---- mixed widths
def small_prime(n, t, barrett_is_exact, bits=30):
    """the largest Barrett-exact prime below 2^bits that is 1 (mod 2n) and (mod t)"""
    step = max(2 * n, t)
    q = (1 << bits) - step + 1
    while not (is_prime(q) and barrett_is_exact(q)):
        q -= step
        assert q > 1 << (bits - 1)
    return q


def mixed_width_set(n, t, barrett_is_exact, small_at):
    """r = 3: one 30-bit prime at position small_at among two 61-bit primes of wide_subset, a third 61-bit prime as the special one"""
    wide, _ = wide_subset(n, 2, barrett_is_exact)
    qs = list(wide[:2])
    qs.insert(small_at, small_prime(n, t, barrett_is_exact))
    qs.append(wide[2])
    return qs, [find_psi(q, n) for q in qs]
