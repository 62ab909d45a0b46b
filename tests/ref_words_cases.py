"""The requests sent to the reference binaries (oracle/_ref, built from the reference's own kernels) and what the oracle says each
must return.  Shared by tests/test_gpu_reference_words.py (reference binary = oracle = library on the GPU), tests/golden/make_ref_words.py
(records the binaries' responses) and tests/test_reference_words_host.py (holds the oracle to the recorded words on every CPU run).

A group is one harness invocation: (binary, [Item]).  Every input is re-derived from fixed seeds; nothing here reads a response.
"""
import numpy as np

import params as P
import ref_py as R
from bfv_launch_inputs import positions
from test_gpu_bfv_launch_edges import GAUSSIAN_WORDS, UNIFORM_WORDS

M64 = (1 << 64) - 1
SIZES = (2048, 4096, 8192, 16384, 32768)                 # every n the reference's 60-bit dispatch knows (ntt_60bit.cuh:314-386)
KAT1_INEXACT = (68719230977, 29008497)                   # the Barrett-inexact prime of decryption_test.cu:47-48 (n = 4096)
KAT1_PRIMES = ([68719403009, 68719230977, 137438822401], [24250113, 29008497, 8625844])
DEFAULT_KEY = bytes([1] * 32)                            # generate_random_default, distributions.cuh:261
# generate_random sets 32 bytes of 77 but uploads XSALSA20_CRYPTO_NONCEBYTES = 24 of them (distributions.cuh:232-235): the last eight
# key bytes are what the constant array held before -- zero in a fresh process, generate_random_default's ones after a call of that
RANDOM_KEY_FRESH = bytes([77] * 24 + [0] * 8)
RANDOM_KEY_AFTER_DEFAULT = bytes([77] * 24 + [1] * 8)


class Item:
    """one case.  expect: the oracle's words for the response (None where the oracle claims none); full: how much of the recorded
    response the fixture keeps next to its digest -- True the whole, k > 0 the first k words, 0 the digest alone"""

    def __init__(self, name, case, expect, full=0, meta=None):
        self.name, self.case, self.expect, self.full, self.meta = name, case, expect, full, meta or {}

    def stored_part(self, words):
        return words if self.full is True else words[:int(self.full)]


def mod_of(prm, i=0, tables=True):
    return (int(prm.q[i]), int(prm.mu[i]), int(prm.k[i]), int(prm.psi[i]) if tables else 0)


def root_for(q, psi32k, n):
    return pow(psi32k, 32768 // n, q)


def adversarial(oracle, q, n, seed):
    """the pattern of test_gpu_fuzz_moduli.py / test_gpu_parity.py over splitmix residues"""
    a = oracle.splitmix(n, seed, q)
    a[:8] = [0, 1, q - 1, q - 2, q - 1, 0, q - 1, 1]
    a[n // 2 - 2: n // 2 + 2] = [q - 1, 0, q - 1, q - 1]
    a[n - 4:] = [q - 1, q - 1, 0, q - 2]
    a[1000:1000 + 64] = q - 1
    return a


def ternary_like(q, n, seed):
    """test_gpu_round6.py's rows of {0, 1, q - 1, q - 2}: what ternary keys feed the transforms"""
    pick = np.random.default_rng(seed).integers(0, 4, size=n)
    return np.array([0, 1, q - 1, q - 2], dtype=np.uint64)[pick]


# seeds s for which ternary_like(q, n, 1000003 n + s) makes the reference's forward leave a word q + r (found by running the oracle over
# s = 0, 1, ...; the first hit).  The under-reduction needs a product in a window of relative width about 2^-(k+1) below a multiple of q,
# so one drawn polynomial of the 36- and 50-bit primes does not reach it within 2048 seeds: for those constructed_class0 below builds
# the input; the pointwise group reaches the event on every inexact prime through constructed operand pairs.
CLASS0_SEEDS = {
    (2048, 16717447169): 69, (2048, 1137833256315125761): 55, (2048, 2248020882338086913): 408,
    (4096, 16717447169): 7, (4096, 1137833256315125761): 49, (4096, 2248020882338086913): 275, (4096, 68719230977): 45,
    (8192, 16717447169): 1, (8192, 1137833256315125761): 83, (8192, 2248020882338086913): 99,
    (16384, 16717447169): 1, (16384, 1137833256315125761): 140, (16384, 2248020882338086913): 9,
    (32768, 16717447169): 0, (32768, 1137833256315125761): 15, (32768, 2248020882338086913): 26,
}


NOT_CONSTRUCTED = {(4096, 66607251457)}     # no twiddle / operand pair of the last stage qualifies within the search below


def constructed_class0(oracle, prm, n):
    """An input, all words below q, on which the reference's LAST forward stage must leave a word q + r -- for the primes whose
    under-reduction is too rare for a drawn polynomial (CLASS0_SEEDS has none).  The last stage pairs a[2p], a[2p + 1] under the twiddle
    w = table[n/2 + p] and stores its results; so: find p and x with w and x near q and x w = r (mod q), r small, that the oracle's
    Barrett returns as q + r; set the state in front of the last stage to ternary-like words with a[2p] = q - 1, a[2p + 1] = x (then
    a[2p] becomes q - 1 + r); undo the stages in front of it with exact arithmetic.  None where the search finds no such pair."""
    q, psi, mu, k = int(prm.q[0]), int(prm.psi[0]), int(prm.mu[0]), int(prm.k[0])
    if (n, q) in NOT_CONSTRUCTED:
        return None
    tab = [int(x) for x in prm.psi_tabs[0]]
    hit = None
    for shift, rmax in ((4, 64), (3, 256), (2, 1024)):
        for p in range(n // 2):
            w = tab[n // 2 + p]
            if w < q - (q >> shift):
                continue
            wi = pow(w, q - 2, q)
            for r in range(1, rmax):
                x = r * wi % q
                if x >= q - (q >> shift) and oracle.lib().orc_barrett(x, w, q, mu, k) >= q:
                    hit = (p, x)
                    break
            if hit:
                break
        if hit:
            break
    if hit is None:
        return None
    p, x = hit
    s = np.array([int(v) for v in ternary_like(q, n, n + 1)], dtype=object)
    s[2 * p], s[2 * p + 1] = q - 1, x
    half, length = (q + 1) // 2, n // 4
    while length >= 1:
        step = n // length // 2
        s = s.reshape(length, 2, step)
        wi = np.array([pow(tab[length + j], q - 2, q) for j in range(length)], dtype=object).reshape(length, 1)
        top, bottom = s[:, 0, :], s[:, 1, :]
        s = np.stack([(top + bottom) * half % q, (top - bottom) * half % q * wi % q], axis=1)
        length //= 2
    return np.array([int(v) for v in s.reshape(-1)], dtype=np.uint64)


def inexact_moduli(n):
    out = [(q, r[n]) for _, (q, r) in sorted(P.INEXACT_PRIMES.items())]
    if n == 4096:
        out.append(KAT1_INEXACT)
    return out


def exact_moduli(n):
    e62, e61, g62 = P.EDGE_PRIMES[62], P.EDGE_PRIMES[61], P.GENERAL_PRIMES[62]
    return [(P.REF_PARAMS[n][0], P.REF_PARAMS[n][1]),
            (e62[0], root_for(e62[0], e62[1][32768], n)), (e61[0], root_for(e61[0], e61[1][32768], n)),       # KERNEL_FORMS hl2-near
            (g62[0], root_for(g62[0], g62[1], n)), (P.Q60[1], root_for(P.Q60[1], P.PSI60[1], n))]             # KERNEL_FORMS hl2-general


# ---- 2. single transforms ---------------------------------------------------------------------------------------------------------
def transforms(oracle, n):
    items = []
    for inexact, moduli in ((False, exact_moduli(n)), (True, inexact_moduli(n))):
        for q, psi in moduli:
            prm = oracle.Params(n, [q], [psi])
            m = [mod_of(prm)]
            inputs = [("adversarial", adversarial(oracle, q, n, 4000 + n)), ("qm1", np.full(n, q - 1, dtype=np.uint64))]
            if inexact:
                forced = None if (n, q) in CLASS0_SEEDS else constructed_class0(oracle, prm, n)
                inputs.append(("ternary", ternary_like(q, n, 1000003 * n + CLASS0_SEEDS.get((n, q), 0)) if forced is None else forced))
            for label, a in inputs:
                f = oracle.forward(a, prm)
                meta = dict(q=q, psi=psi, n=n, inexact=inexact, input=a, class0=inexact and label == "ternary" and ((n, q) in CLASS0_SEEDS or forced is not None))
                full = 0
                items.append(Item("forwardNTT-n%d-q%d-%s" % (n, q, label), R.Case(R.FORWARD, n, m, words=a),
                                  (lambda f=f: f), bool(meta["class0"] and n == 2048), dict(meta, op="forward")))
                items.append(Item("inverseNTT-n%d-q%d-%s" % (n, q, label), R.Case(R.INVERSE, n, m, words=f),
                                  (lambda f=f, prm=prm: oracle.inverse(f, prm)), full, dict(meta, op="inverse", input=f)))
            if inexact:          # the reference does not round-trip here: the inverse of words that are no forward output
                w = oracle.splitmix(n, 9000 + n, q)
                items.append(Item("inverseNTT-n%d-q%d-arbitrary" % (n, q), R.Case(R.INVERSE, n, m, words=w),
                                  (lambda w=w, prm=prm: oracle.inverse(w, prm)), 0, dict(q=q, psi=psi, n=n, inexact=True, op="inverse", input=w)))
    return R.REF60, items


# ---- 3. batch forms ---------------------------------------------------------------------------------------------------------------
def batch_primes(n):
    """an exact, an inexact and another exact modulus: polynomial y must take prime y % division, or words change"""
    sel = [P.EXACT_NEIGHBOURS[60], P.INEXACT_PRIMES[60], P.EXACT_NEIGHBOURS[36]]
    return [q for q, _ in sel], [r[n] for _, r in sel]


def batches(oracle):
    items = []
    for n in (2048, 4096):
        qs, psis = batch_primes(n)
        for division, num in ((3, 7), (1, 3)):
            sub_q, sub_psi = (qs, psis) if division == 3 else (qs[1:2], psis[1:2])
            prm = oracle.Params(n, sub_q, sub_psi)
            mods = [mod_of(prm, i) for i in range(division)]
            a = oracle.synth_batch(n, num, sub_q, 100 * division + n)
            for y in range(num):
                q = sub_q[y % division]
                a[y, :4] = [q - 1, 0, 1, q - 2]
                a[y, n - 2:] = [q - 1, q - 1]
            a[num - 1, :] = sub_q[(num - 1) % division] - 1
            f = oracle.forward_batch(a, prm, division=division).reshape(num, n)
            meta = dict(n=n, qs=sub_q, psis=sub_psi, num=num, division=division)
            items.append(Item("forwardNTT_batch-n%d-div%d-num%d" % (n, division, num), R.Case(R.FORWARD_BATCH, n, mods, [num, division], a),
                              (lambda f=f: f.reshape(-1)), 0, dict(meta, op="forward_batch", input=a)))
            items.append(Item("inverseNTT_batch-n%d-div%d-num%d" % (n, division, num), R.Case(R.INVERSE_BATCH, n, mods, [num, division], f),
                              (lambda f=f, prm=prm, d=division: oracle.inverse_batch(f, prm, division=d).reshape(-1)), 0, dict(meta, op="inverse_batch", input=f)))
        for q, psi in ((qs[1], psis[1]), (qs[0], psis[0])):
            prm = oracle.Params(n, [q], [psi])
            m = [mod_of(prm)]
            a, b = adversarial(oracle, q, n, 71), ternary_like(q, n, 72)
            fa, fb = oracle.forward(a, prm), oracle.forward(b, prm)
            meta = dict(n=n, q=q, psi=psi, a=a, b=b)
            items.append(Item("forwardNTTdouble-n%d-q%d" % (n, q), R.Case(R.FORWARD_DOUBLE, n, m, words=[a, b]),
                              (lambda fa=fa, fb=fb: np.concatenate([fa, fb])), False, dict(meta, op="forward_double")))
            items.append(Item("half_poly_mul_device-n%d-q%d" % (n, q), R.Case(R.HALF_POLY_MUL, n, m, words=[a, fb]),
                              (lambda fa=fa, fb=fb, prm=prm: oracle.inverse(oracle.pointwise_batch(fa, fb, prm), prm)), 0,
                              dict(meta, op="half_poly_mul", b=fb)))
            items.append(Item("full_poly_mul_device-n%d-q%d" % (n, q), R.Case(R.FULL_POLY_MUL, n, m, words=[a, b]),
                              (lambda fa=fa, fb=fb, prm=prm: np.concatenate([oracle.pointwise_batch(fa, fb, prm), fb])), 0,
                              dict(meta, op="full_poly_mul")))
    return R.REF60, items


# ---- 4. pointwise and element-wise ------------------------------------------------------------------------------------------------
def noncanonical_pairs(oracle, prm, count, seed=0):
    """operand pairs below q whose reference product comes out as q + r, checked with the oracle's own Barrett.  Constructed, not
    drawn: the single subtraction falls short only when x y is large and just above a multiple of q, so x runs down from q - 1 and
    y = r / x (mod q) for small r, kept when y is in the top 1/32 of the range.  An exact modulus yields none."""
    q, mu, k = int(prm.q[0]), int(prm.mu[0]), int(prm.k[0])
    out = []
    for i in range(seed, seed + 512):
        x = q - 1 - i
        xi = pow(x, q - 2, q)
        for r in range(64):
            y = r * xi % q
            if y >= q - (q >> 5) and oracle.lib().orc_barrett(x, y, q, mu, k) >= q:
                out.append((x, y))
                if len(out) == count:
                    return out
    return out


def edge_operands(oracle, q, n, seed):
    """the edge operands of test_gpu_round4.py::test_elementwise_wrappers_match_the_reference_arithmetic and more: sums equal to q,
    a[i] < b[i], zero under negate"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, q, size=n, dtype=np.uint64)
    b = rng.integers(0, q, size=n, dtype=np.uint64)
    a[:6] = [0, 1, q - 1, q - 1, 5, 7]
    b[:6] = [0, q - 1, 1, q - 1, 7, 5]
    for i in range(6, 64):                                   # a + b = q exactly, from both ends of the range
        a[i] = (i - 5) if i % 2 else q - (i - 5)
        b[i] = q - int(a[i])
    a[64:72] = 0                                             # 0 under negate; 0 < b
    a[n - 1], b[n - 1] = q - 1, 1
    return a, b


def pointwise(oracle):
    n = 2048
    items = []
    qi, ri = P.INEXACT_PRIMES[60]
    qe = P.Q60[0]
    for q in (qi, P.INEXACT_PRIMES[36][0], P.INEXACT_PRIMES[50][0], qe, P.REF_PARAMS[2048][0]):
        prm = oracle.Params(n, [q], [1], tables=False)
        m = [mod_of(prm, 0, tables=False)]
        a, b = edge_operands(oracle, q, n, 5)
        pairs = noncanonical_pairs(oracle, prm, 64)
        for j, (x, y) in enumerate(pairs):
            a[100 + j], b[100 + j] = x, y
        meta = dict(q=q, n=n, a=a, b=b, noncanonical=len(pairs))
        items.append(Item("barrett-q%d" % q, R.Case(R.BARRETT, n, m, words=[a, b]),
                          (lambda a=a, b=b, prm=prm: oracle.pointwise_batch(a, b, prm)), 164 if q == qi else 0, dict(meta, op="barrett")))
        for k in (0, 1, q - 1, 12345678901234567 % q) + ((pairs[0][1],) if pairs else ()):
            items.append(Item("barrett_int-q%d-b%d" % (q, k), R.Case(R.BARRETT_INT, n, m, [k], a),
                              (lambda a=a, k=k, prm=prm: oracle.pointwise_scalar(a, k, prm)), 0, dict(meta, op="barrett_int", scalar=k)))
        items.append(Item("poly_add_device-q%d" % q, R.Case(R.POLY_ADD, n, m, words=[a, b]), (lambda a=a, b=b, q=q: oracle.poly_add(a, b, q)), 72 if q == qi else 0,
                          dict(meta, op="poly_add")))
        items.append(Item("poly_sub_device-q%d" % q, R.Case(R.POLY_SUB, n, m, words=[a, b]), (lambda a=a, b=b, q=q: oracle.poly_sub(a, b, q)), 72 if q == qi else 0,
                          dict(meta, op="poly_sub")))
        items.append(Item("poly_negate_device-q%d" % q, R.Case(R.POLY_NEGATE, n, m, words=a), (lambda a=a, q=q: oracle.poly_negate(a, q)), 72 if q == qi else 0,
                          dict(meta, op="poly_negate")))
        for k in (0, 1, q - 1, 12345678901234567):
            items.append(Item("poly_add_integer_device-q%d-b%d" % (q, k), R.Case(R.POLY_ADD_INTEGER, n, m, [k], a),
                              (lambda a=a, k=k, q=q: oracle.poly_add_integer(a, k, q)), 0, dict(meta, op="poly_add_integer", scalar=k)))
        # b a[i] >= 2^64 (the low word is what is masked) and a t whose t - 1 does not fit the reference's 32-bit mask
        for t, k in ((1024, 3), (1 << 16, q - 5), (1 << 40, 0x123456789abcdef), (1024, M64), (1 << 20, (1 << 63) + 12345)):
            items.append(Item("poly_mul_int_t-q%d-t%d-b%d" % (q, t, k), R.Case(R.POLY_MUL_INT_T, n, m, [k, t], a),
                              (lambda a=a, k=k, t=t: oracle.poly_mul_int_t(a, k, t)), (8 if t == 1 << 40 and q == qi else 0), dict(meta, op="poly_mul_int_t", scalar=k, t=t)))
    # the batch forms: num 7 over division 3 (exact, inexact, exact), the ragged tail of `y % division`
    qs, _ = batch_primes(n)
    prm = oracle.Params(n, qs, [1, 1, 1], tables=False)
    mods = [mod_of(prm, i, tables=False) for i in range(3)]
    num = 7
    a, b = oracle.synth_batch(n, num, qs, 31), oracle.synth_batch(n, num, qs, 32)
    one = oracle.Params(n, qs[1:2], [1], tables=False)
    pairs = noncanonical_pairs(oracle, one, 64, 3)
    for y in (1, 4):                                        # the rows of the inexact modulus
        for j, (x, z) in enumerate(pairs):
            a[y, 10 + j], b[y, 10 + j] = x, z
    for y in range(num):
        a[y, 0] = b[y, 0] = qs[y % 3] - 1
    want = oracle.pointwise_batch(a, b, prm, division=3)
    meta = dict(n=n, qs=qs, num=num, division=3, a=a, b=b, noncanonical=len(pairs))
    items.append(Item("barrett_batch", R.Case(R.BARRETT_BATCH, n, mods, [num, 3], [a, b]), (lambda w=want: w.reshape(-1)), 0, dict(meta, op="barrett_batch")))
    items.append(Item("barrett_batch_3param", R.Case(R.BARRETT_BATCH_3PARAM, n, mods, [num, 3], [a, b]), (lambda w=want: w.reshape(-1)), 0,
                      dict(meta, op="barrett_batch_3param")))
    return R.REF60, items


# ---- 5. keystream and samplers ----------------------------------------------------------------------------------------------------
def sampler_moduli():
    """25, 55 and 62 bits"""
    return [P.REF_PARAMS[4096][0], P.Q55[0], P.EDGE_PRIMES[62][0]]


def crafted_bytes(n, R_, seed=40):
    """crafted as test_gpu_bfv_launch_edges.py::test_samplers_on_crafted_bytes crafts its bytes (that test builds them inline; the edge
    words and their positions are imported from it): all 256 ternary bytes both ways, UNIFORM_WORDS / GAUSSIAN_WORDS at the head and
    tail of every 64-lane block"""
    rng = np.random.default_rng(seed)
    tern = np.concatenate([np.arange(256, dtype=np.uint8)[::-1], np.arange(256, dtype=np.uint8), rng.integers(0, 256, size=n - 512, dtype=np.uint8)])
    uni = rng.integers(0, 1 << 64, size=(R_, n), dtype=np.uint64)
    for i in range(R_):
        for j, p in enumerate(positions(n)):
            uni[i, p] = UNIFORM_WORDS[(i + j) % len(UNIFORM_WORDS)]
    gw = [rng.integers(0, 1 << 32, size=n, dtype=np.uint32) for _ in range(3)]
    for k, g in enumerate(gw):
        for j, p in enumerate(positions(n)):
            g[p] = GAUSSIAN_WORDS[(j + k) % len(GAUSSIAN_WORDS)]
    return tern, uni, gw


def samplers(oracle):
    n = 2048
    qs = sampler_moduli()
    mods = [R.modulus(q) for q in qs]
    Rn = len(qs)
    tern, uni, gw = crafted_bytes(n, Rn)
    nbytes = 64 * 40
    items = [
        Item("generate_random-fresh", R.Case(R.GENERATE_RANDOM, n, [], [nbytes + 17]),
             lambda: R.pack_bytes(oracle.salsa20_keystream(nbytes + 17, RANDOM_KEY_FRESH, 0)), False, dict(op="keystream", key=RANDOM_KEY_FRESH, nbytes=nbytes + 17)),
        Item("generate_random_default", R.Case(R.GENERATE_RANDOM_DEFAULT, n, [], [nbytes]),
             lambda: R.pack_bytes(oracle.salsa20_keystream(nbytes, DEFAULT_KEY, 0)), 16, dict(op="keystream", key=DEFAULT_KEY, nbytes=nbytes)),
        Item("generate_random-after-default", R.Case(R.GENERATE_RANDOM, n, [], [nbytes]),
             lambda: R.pack_bytes(oracle.salsa20_keystream(nbytes, RANDOM_KEY_AFTER_DEFAULT, 0)), False,
             dict(op="keystream", key=RANDOM_KEY_AFTER_DEFAULT, nbytes=nbytes)),
        Item("ternary_dist_xq", R.Case(R.TERNARY_XQ, n, mods, words=R.pack_bytes(tern)),
             lambda: oracle.sample_xq("ternary", tern, n, qs).reshape(-1), 512, dict(op="ternary", bytes=tern)),
        Item("uniform_dist_xq", R.Case(R.UNIFORM_XQ, n, mods, words=uni.reshape(-1)),
             lambda: oracle.sample_xq("uniform", uni.reshape(-1).view(np.uint8), n, qs).reshape(-1), 64, dict(op="uniform", words=uni)),
        # Gaussian: no oracle expectation word for word (its inverse normal CDF is AS241, the device's is normcdfinvf)
        Item("gaussian_dist_xq", R.Case(R.GAUSSIAN_XQ, n, mods, words=R.pack_u32(gw[0])), None, 0, dict(op="gaussian", words=gw[0])),
        Item("convert_ternary_gaussian_x2", R.Case(R.CONVERT_TERNARY_GAUSSIAN_X2, n, mods, words=R.pack_bytes(np.concatenate([tern, gw[1].view(np.uint8), gw[2].view(np.uint8)]))),
             None, 0, dict(op="convert_x2", bytes=tern, words=(gw[1], gw[2]))),
    ]
    return R.REF60, items, dict(n=n, qs=qs, tern=tern, uni=uni, gw=gw)


# ---- 6. complete drivers ----------------------------------------------------------------------------------------------------------
def driver_sets():
    q55 = P.Q55[:3]
    return [("n4096-kat1", 4096, KAT1_PRIMES[0], KAT1_PRIMES[1]),
            ("n2048-q55", 2048, q55, [root_for(q, p, 2048) for q, p in zip(q55, P.PSI55[:3])])]


def driver_constants(oracle, qs, psis, t, gamma):
    """what the harness uploads, from the oracle (bfv_constants); the base change matrix and mu_gamma are the two it does not export"""
    k = oracle.bfv_constants(qs, psis, t, gamma)
    r = len(qs) - 1
    bcm = []
    for base in (t, gamma):
        for j in range(r):
            v = 1
            for i in range(r):
                if i != j:
                    v = v * qs[i] % base
            bcm.append(v)
    k["base_change_matrix"] = np.array(bcm, dtype=np.uint64)
    k["mu_gamma"] = (1 << (2 * 61)) // gamma
    return k


def driver_args(k, t, gamma):
    return [t, gamma, k["mu_gamma"], 61] + [int(x) for x in k["neg_inv_q_mod_t_gamma"]] + [int(x) for x in k["inv_q_last_mod_q"]] + \
        [int(x) for x in k["qi_div_t"]] + [int(x) for x in k["inv_punctured_q"]] + [int(x) for x in k["prod_t_gamma_mod_q"]] + \
        [int(x) for x in k["base_change_matrix"]]


def driver_message(n, t):
    return (np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(3)) % np.uint64(t)


def signed_small(words, q):
    """residues of small signed values -> int8"""
    w = words.astype(np.int64)
    return np.where(w > q // 2, w - q, w).astype(np.int8)


def residues(small, qs, n):
    s = small.astype(np.int64)
    return np.stack([np.where(s < 0, s + int(q), s).astype(np.uint64) for q in qs])


def drivers_oracle(oracle, n, qs, psis, t, gamma, gauss):
    """keygen_rns -> encryption_rns -> decryption_rns with the oracle.  gauss: the three Gaussian polynomials as small signed values
    (keygen's e, encryption's e0 and e1) -- the one step whose words the oracle does not claim; everything else from the keystream."""
    Rn = len(qs)
    ks = oracle.salsa20_keystream(9 * Rn * n + 4 * n, DEFAULT_KEY, 0)
    tern = oracle.sample_xq("ternary", ks[:n], n, qs)
    uni = oracle.sample_xq("uniform", ks[n: n + 8 * Rn * n], n, qs)
    pk0 = np.zeros((2, Rn, n), dtype=np.uint64)
    pk0[1] = uni
    sk, pk = oracle.bfv_keygen_core(tern, pk0, residues(gauss[0], qs, n), qs, psis, n)
    c0 = np.stack([tern, tern])                                          # nonce 0 again: u is the secret key's ternary sample
    e = np.stack([residues(gauss[1], qs, n), residues(gauss[2], qs, n)])
    m = driver_message(n, t)
    c = oracle.bfv_encrypt_core(c0, pk, e, m, qs, psis, n, t)
    d = np.ascontiguousarray(c).reshape(-1).copy()
    lib = oracle.lib()
    qa, pa = np.array(qs, dtype=np.uint64), np.array(psis, dtype=np.uint64)
    out = np.empty(n, dtype=np.uint64)
    skc = np.ascontiguousarray(sk).reshape(-1)
    assert lib.orc_bfv_decrypt(oracle._p(d), oracle._p(skc), oracle._p(qa), oracle._p(pa), Rn, n, int(t), int(gamma), oracle._p(out), None) == 0
    return dict(sk=sk.reshape(-1), pk=pk.reshape(-1), c_enc=c.reshape(-1), c_dec=d, plain=out, m=m, keystream=ks)


def drivers(oracle):
    t, gamma = 1024, P.GAMMA61
    items = []
    for name, n, qs, psis in driver_sets():
        prm = oracle.Params(n, qs, psis)
        mods = [mod_of(prm, i) for i in range(len(qs))]
        k = driver_constants(oracle, qs, psis, t, gamma)
        m = driver_message(n, t)
        Rn = len(qs)
        # the Gaussian steps alone, on the bytes the drivers will read: their words feed the oracle's drivers
        ks = oracle.salsa20_keystream(9 * Rn * n + 4 * n, DEFAULT_KEY, 0)
        g_key = ks[n + 8 * Rn * n: n + 8 * Rn * n + 4 * n]
        meta = dict(n=n, qs=qs, psis=psis, t=t, gamma=gamma, constants=k, set=name)
        items.append(Item("drivers-%s-gaussian-keygen" % name, R.Case(R.GAUSSIAN_XQ, n, mods, words=R.pack_bytes(g_key)), None, False, dict(meta, op="gaussian")))
        items.append(Item("drivers-%s-gaussian-encrypt" % name, R.Case(R.CONVERT_TERNARY_GAUSSIAN_X2, n, mods, words=R.pack_bytes(ks[:9 * n])), None, False,
                          dict(meta, op="convert_x2")))
        items.append(Item("drivers-%s" % name, R.Case(R.BFV_DRIVERS, n, mods, driver_args(k, t, gamma), m), None, False, dict(meta, op="drivers")))
    return R.REF60, items


def driver_gauss_from_responses(items, outs):
    """per driver set: the three Gaussian polynomials (small signed) out of the two sampler responses that precede the driver case"""
    res = {}
    for i, it in enumerate(items):
        if it.meta["op"] != "drivers":
            continue
        n, qs = it.meta["n"], it.meta["qs"]
        Rn = len(qs)
        g0 = signed_small(outs[i - 2][:n], qs[0])
        e = outs[i - 1][2 * Rn * n:].reshape(2, Rn, n)
        res[it.meta["set"]] = [g0, signed_small(e[0, 0], qs[0]), signed_small(e[1, 0], qs[0])]
    return res


def sampler_gauss_from_responses(items, outs, n, qs):
    """the three Gaussian polynomials (small signed) of the samplers group: gaussian_dist_xq, then e0 and e1 of the merged kernel"""
    Rn = len(qs)
    by = {it.meta["op"]: w for it, w in zip(items, outs)}
    e = by["convert_x2"][2 * Rn * n:].reshape(2, Rn, n)
    return [signed_small(by["gaussian"][:n], qs[0]), signed_small(e[0, 0], qs[0]), signed_small(e[1, 0], qs[0])]


def sampler_gauss_oracle(oracle, n, qs, gw):
    return [signed_small(oracle.sample_xq("gaussian", g.view(np.uint8), n, qs)[0], qs[0]) for g in gw]


def driver_gauss_oracle(oracle, n, qs):
    """the same three polynomials by the oracle's own sampler (AS241) on the reference's keystream"""
    Rn = len(qs)
    ks = oracle.salsa20_keystream(9 * Rn * n + 4 * n, DEFAULT_KEY, 0)
    return [signed_small(oracle.sample_xq("gaussian", by, n, qs)[0], qs[0])
            for by in (ks[n + 8 * Rn * n: n + 8 * Rn * n + 4 * n], ks[n: 5 * n], ks[5 * n: 9 * n])]


def gauss_diff(reference, own):
    """rows (polynomial, index, the reference's value) wherever the reference binary's Gaussian words differ from the oracle's: what
    the fixture keeps, instead of whole polynomials"""
    rows = [(p, int(i), int(reference[p][i])) for p in range(3) for i in np.nonzero(reference[p] != own[p])[0]]
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


def gauss_patched(own, diff):
    out = [g.copy() for g in own]
    for p, i, v in diff:
        out[int(p)][int(i)] = v
    return out


# ---- 7. the 30-bit path -----------------------------------------------------------------------------------------------------------
SIZES30 = (2048, 8192, 32768, 65536)


def moduli30():
    import test_ntt30_moduli as T
    return [("top17", T.TOP17, 30), ("params30", T.NONCANON, 24), ("inexact", T.INEXACT_SHOWN[0], T.INEXACT_SHOWN[0].bit_length()), ("noncanon", T.NONCANON, 25)]


def thirty(oracle, n):
    import test_ntt30_moduli as T
    items = []
    for label, q, bits in moduli30():
        prm = T.params(oracle, q, bits, n)
        m = [(q, prm.mu, bits, prm.psi)]
        a = T.words(q, n, 3, 30 + n)
        b = T.words(q, n, 3, 31 + n)
        for y in range(3):
            f = oracle.forward30(a[y], prm).reshape(-1)
            meta = dict(n=n, q=q, bits=bits, prm=prm, label=label)
            full = label == "inexact" and n == 2048 and y == 0
            items.append(Item("forwardNTT30-n%d-%s-%d" % (n, label, y), R.Case(R.FORWARD, n, m, words=R.pack_u32(a[y])),
                              (lambda f=f: R.pack_u32(f)), full, dict(meta, op="forward30", input=a[y])))
            items.append(Item("inverseNTT30-n%d-%s-%d" % (n, label, y), R.Case(R.INVERSE, n, m, words=R.pack_u32(f)),
                              (lambda f=f, prm=prm: R.pack_u32(oracle.inverse30(f, prm).reshape(-1))), 0, dict(meta, op="inverse30", input=f)))
            items.append(Item("barrett_30bit-n%d-%s-%d" % (n, label, y), R.Case(R.BARRETT, n, m, words=[R.pack_u32(a[y]), R.pack_u32(b[y])]),
                              (lambda x=a[y], z=b[y], prm=prm: R.pack_u32(oracle.pointwise30(x, z, prm).reshape(-1))), 0,
                              dict(meta, op="barrett30", input=a[y], b=b[y])))
    return R.REF30, items


# ---- all groups, by name (the fixture and the host test walk this) -----------------------------------------------------------------
def groups(oracle):
    out = [("transforms-n%d" % n, (lambda n=n: transforms(oracle, n)[:2])) for n in SIZES]
    out += [("batches", lambda: batches(oracle)), ("pointwise", lambda: pointwise(oracle)), ("samplers", lambda: samplers(oracle)[:2]),
            ("drivers", lambda: drivers(oracle))]
    out += [("thirty-n%d" % n, (lambda n=n: thirty(oracle, n))) for n in SIZES30]
    return out


GROUP_NAMES = ["transforms-n%d" % n for n in SIZES] + ["batches", "pointwise", "samplers", "drivers"] + ["thirty-n%d" % n for n in SIZES30]
