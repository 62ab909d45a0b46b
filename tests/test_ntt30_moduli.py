"""The 30-bit path over its whole modulus range, against an exact reference (include/mi355ntt.h: any q < 2^30).

The reference's six 30-bit parameter sets (test_ntt30.py, PARAMS30) are 24- and 25-bit primes on which the single-subtraction
Barrett is exact, so they leave three parts of kernels_ntt30.hip unexercised: the lazy [0, 4q) domain of the native kernels
(k_ntt30x: 32-bit words, sums X + 2q - Y), whose margin is thinnest near q = 2^30; the routing of Barrett-inexact moduli and of
a bit length that is not q's own to the literal kernels (capi.cpp, ninv30_if_native); and the oracle itself away from those
primes.  Here the moduli are DRAWN per bit length 20 .. 30 from a fixed seed and PICKED at the edges (the largest primes below
2^30, small ones, Barrett-inexact ones, a non-canonical bit length), and every GPU word is compared with the exact transform
(plain numpy, exact in uint64 since q < 2^30) and / or the oracle (orc30_*, the reference's own arithmetic):
  * exact moduli: forward equal to the exact transform AND to the oracle, inverse of arbitrary words equal to the exact inverse,
    the round trip over the whole batch the identity;
  * inexact moduli and the non-canonical bit length: forward and inverse equal to the oracle's words (the reference's words need
    not round-trip there)."""
import random
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_fuzz_moduli import barrett_margin, is_prime, psi_for

SIZES = (2048, 8192, 32768, 65536)
STEP = 1 << 17                      # q = 1 (mod 2^17): a 2n-th root of unity up to n = 2^16


# ------------------------------------------------------------------------------------------------ the exact reference
def brv(n):
    lg = n.bit_length() - 1
    i = np.arange(n, dtype=np.int64)
    r = np.zeros(n, dtype=np.int64)
    for b in range(lg):
        r |= ((i >> b) & 1) << (lg - 1 - b)
    return r


def twiddles(x, q, n):
    """x^brv(i) mod q for i < n (the order of the reference's psi tables)"""
    pw = np.ones(n, dtype=np.uint64)
    filled = 1
    while filled < n:
        pw[filled:2 * filled] = pw[:filled] * np.uint64(pow(x, filled, q)) % np.uint64(q)
        filled *= 2
    return pw[brv(n)]


def exact_forward30(a, q, psi, n):
    """CT stages of the negacyclic transform (test_ntt30.exact_forward), vectorised per stage over any number of polynomials"""
    Q = np.uint64(q)
    tab = twiddles(psi, q, n)
    x = np.array(a, dtype=np.uint64).reshape(-1, n)
    length = 1
    while length < n:
        step = n // (2 * length)
        blk = x.reshape(-1, length, 2, step)
        u, v = blk[:, :, 0, :], blk[:, :, 1, :] * tab[length:2 * length, None] % Q
        x = np.stack(((u + v) % Q, (u + Q - v) % Q), axis=2).reshape(-1, n)
        length *= 2
    return x.astype(np.uint32).reshape(np.shape(a))


def exact_inverse30(A, q, psi, n):
    """GS stages with psi^-1, then n^-1 once"""
    Q = np.uint64(q)
    tab = twiddles(pow(psi, -1, q), q, n)
    x = np.array(A, dtype=np.uint64).reshape(-1, n)
    length = n // 2
    while length >= 1:
        step = n // (2 * length)
        blk = x.reshape(-1, length, 2, step)
        u, v = blk[:, :, 0, :], blk[:, :, 1, :]
        x = np.stack(((u + v) % Q, (u + Q - v) % Q * tab[length:2 * length, None] % Q), axis=2).reshape(-1, n)
        length //= 2
    x = x * np.uint64(pow(n, -1, q)) % Q
    return x.astype(np.uint32).reshape(np.shape(A))


# ------------------------------------------------------------------------------------------------ the moduli
def drawn_primes():
    """per bit length 20 .. 30: two primes = 1 (mod 2^17) drawn from a fixed seed; below 23 bits there is only one such prime,
    the second is then drawn = 1 (mod 2^14) (n <= 8192)"""
    rng = random.Random(20261015)
    out = []
    for k in range(20, 31):
        got = []
        for step in (STEP, 1 << 14):
            pool = [q for q in range(((1 << (k - 1)) // step + 1) * step + 1, 1 << k, step)
                    if is_prime(q) and abs(barrett_margin(q) - 1) > Fraction(1, 10 ** 6) and q not in got]
            got += rng.sample(pool, min(2 - len(got), len(pool)))
            if len(got) == 2:
                break
        out += [("drawn-%d-%d" % (k, i), q, k) for i, q in enumerate(got)]
    return out


TOP17, TOP14 = 1073479681, 1073692673       # the largest primes below 2^30 that are = 1 (mod 2^17) / = 1 (mod 2^12)
# Barrett-inexact moduli whose oracle words differ from the exact transform on the test input (all = 1 (mod 2^17)), and one
# that is inexact by the bound although its words agree on sampled data
INEXACT_SHOWN = (536215553, 1055260673, 268042241)
INEXACT_QUIET = 1070727169
# 24 bits, called with bit_length 25 and mu = floor(2^50 / q): the literal kernels.  (One bit of slack leaves the Barrett all
# but exact -- its words agree with the exact transform here, so this case checks the literal kernels on a bit length that
# is not q's own, not the routing.)
NONCANON = 13631489

CASES = drawn_primes() + [
    ("top-17", TOP17, 30), ("top-12", TOP14, 30),
    ("small-12289", 12289, 14), ("small-40961", 40961, 16), ("small-65537", 65537, 17),
] + [("inexact-%d" % q, q, q.bit_length()) for q in INEXACT_SHOWN] + [
    ("inexact-quiet-%d" % INEXACT_QUIET, INEXACT_QUIET, 30), ("bits25-%d" % NONCANON, NONCANON, 25)]


def sizes_of(q):
    """the sizes of SIZES this q has a 2n-th root for, and its largest one below 2^16 if that is not among them"""
    ok = [n for n in (2048, 4096, 8192, 16384, 32768, 65536) if (q - 1) % (2 * n) == 0]
    return [n for n in ok if n in SIZES] + [n for n in ok[-1:] if n not in SIZES]


def is_native(q, bits):
    """the words are the exact transform's: canonical bit length and an exact single-subtraction Barrett"""
    return bits == q.bit_length() and barrett_margin(q) < 1


def params(oracle, q, bits, n):
    prm = oracle.Params30(n, q, psi_for(q, n))
    prm.k, prm.mu = bits, (1 << (2 * bits)) // q             # (the caller's bit length, canonical or not)
    return prm


def words(q, n, num, seed):
    """uniform words below q with the adversarial patterns of test_gpu_fuzz_moduli.py in the first two polynomials (0, 1, q - 1,
    q - 2, a run of q - 1, both sides of n / 2) and, from three polynomials on, a last one of q - 1 only"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, q, size=(num, n), dtype=np.uint32)
    for y in range(min(num, 2)):
        a[y, :8] = [0, 1, q - 1, q - 2, q - 1, 0, q - 1, 1]
        a[y, n // 2 - 2: n // 2 + 2] = [q - 1, 0, q - 1, q - 1]
        a[y, n - 4:] = [q - 1, q - 1, 0, q - 2]
        a[y, 1000:1000 + 64] = q - 1
    if num >= 3:
        a[num - 1, :] = q - 1
    return a


SMALL = 3
# more polynomials than the native kernels keep resident (the counts of test_ntt30.py, test_gpu_30bit_persistent_loop_matches_oracle;
# n = 8192: four workgroups per CU)
LARGE = {2048: 4500, 4096: 2500, 8192: 1100, 32768: 601, 65536: 301}
# n = 2^16 on both sides of kPair30MinPolysFwd / kPair30MinPolysInv (kernels_ntt30.hip: pair launch from 32 / 384 polynomials)
PAIR_BATCHES = (31, 32, 383, 384)
PAIR_MODULI = (TOP17, INEXACT_SHOWN[0])
RUNS = [(idx, n) for idx, (_, q, _) in enumerate(CASES) for n in sizes_of(q)]


def test_exact_reference_is_pinned():
    """the vectorised transform against direct evaluation A[i] = a(psi^(2 brv(i) + 1)), and the inverse against the forward"""
    n = 2048
    for q in (12931073, TOP17):
        psi = psi_for(q, n)
        a = words(q, n, 2, q)
        A = exact_forward30(a, q, psi, n)
        r = brv(n)
        for i in (0, 1, 2, 777, n // 2, n - 1):
            x = pow(psi, 2 * int(r[i]) + 1, q)
            for y in range(2):
                assert int(A[y, i]) == sum(int(c) * pow(x, j, q) for j, c in enumerate(a[y])) % q, (q, i, y)
        assert np.array_equal(exact_inverse30(A, q, psi, n), a), q
        assert A.dtype == np.uint32 and int(A.max()) < q


def test_the_moduli_cover_the_range_and_both_routes(native, oracle):
    bits = {nm: k for nm, _, k in CASES}
    assert {int(nm.split("-")[1]) for nm in bits if nm.startswith("drawn-")} == set(range(20, 31))
    for k in range(20, 31):
        assert "drawn-%d-0" % k in bits and "drawn-%d-1" % k in bits, k
    assert all(is_prime(q) and q < (1 << 30) and q >> bits == 0 for _, q, bits in CASES)
    assert sum(q > (1 << 32) // 6 for _, q, _ in CASES) >= 3          # X + 2 * 2q - Y would wrap 32 bits there
    inexact = [q for _, q, _ in CASES if barrett_margin(q) >= 1]
    assert len(inexact) >= 4 and set(INEXACT_SHOWN) | {INEXACT_QUIET} <= set(inexact)
    for nm, q, _ in CASES:
        assert bool(native.barrett_is_exact(q)) == (barrett_margin(q) < 1), (nm, q)
        assert sizes_of(q), (nm, q)
    assert sizes_of(TOP17) == list(SIZES) and 2048 in sizes_of(TOP14) and sizes_of(12289) == [2048]
    assert sizes_of(40961) == [2048, 4096] and sizes_of(65537) == [2048, 8192, 32768]
    assert not is_native(NONCANON, 25) and is_native(NONCANON, 24)
    # the test input tells the routes apart: the oracle's forward differs from the exact transform on each shown-inexact modulus
    # (at some size, for the small batch the GPU test runs)
    for q in INEXACT_SHOWN:
        differs = []
        for n in sizes_of(q):
            a = words(q, n, SMALL, (q, n, SMALL))
            differs.append(not np.array_equal(oracle.forward30(a, params(oracle, q, q.bit_length(), n)), exact_forward30(a, q, psi_for(q, n), n)))
            if differs[-1]:
                break
        assert any(differs), q


def _sample(num):
    return sorted({0, 1, 2, num // 2, num - 2, num - 1} & set(range(num)))


@pytest.mark.gpu
@pytest.mark.parametrize("idx,n", RUNS, ids=["%s-n%d" % (CASES[i][0], n) for i, n in RUNS])
def test_gpu_30bit_modulus_against_exact_and_oracle(native, oracle, gpu, idx, n):
    import torch
    name, q, bits = CASES[idx]
    prm = params(oracle, q, bits, n)
    psi = prm.psi
    native_words = is_native(q, bits)
    dev32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(gpu)
    host32 = lambda t: t.cpu().numpy().view(np.uint32)
    d_psi, d_psiinv = dev32(prm.psi_tab), dev32(prm.psiinv_tab)
    batches = [SMALL]
    if (idx + sizes_of(q).index(n)) % 2 == 0:             # by turns: the persistent loop
        batches.append(LARGE[n])
    if n == 65536 and q in PAIR_MODULI:
        batches += PAIR_BATCHES
    for num in batches:
        a = words(q, n, num, (q, n, num))
        b = words(q, n, num, (q, n, num, 1))
        rows = _sample(num)
        d_a, d_b = dev32(a), dev32(b)
        native.forward30(d_a, n, q, prm.mu, bits, d_psi, num)
        native.inverse30(d_b, n, q, prm.mu, bits, d_psiinv, num)          # (any words below q are a valid input)
        A, Bi = host32(d_a), host32(d_b)
        want_A = oracle.forward30(a[rows], prm)
        assert np.array_equal(A[rows], want_A), (name, q, n, num, "forward vs oracle")
        if native_words:
            assert np.array_equal(A[rows], exact_forward30(a[rows], q, psi, n)), (name, q, n, num, "forward vs exact")
            assert np.array_equal(Bi[rows], exact_inverse30(b[rows], q, psi, n)), (name, q, n, num, "inverse vs exact")
            assert np.array_equal(Bi[rows], oracle.inverse30(b[rows], prm)), (name, q, n, num, "inverse vs oracle")
            native.inverse30(d_a, n, q, prm.mu, bits, d_psiinv, num)
            back = host32(d_a)
            bad = np.flatnonzero((back != a).any(axis=1))
            assert bad.size == 0, (name, q, n, num, "round trip", bad[:8])
        else:
            assert np.array_equal(Bi[rows], oracle.inverse30(b[rows], prm)), (name, q, n, num, "inverse vs oracle")
            native.inverse30(d_a, n, q, prm.mu, bits, d_psiinv, num)
            assert np.array_equal(host32(d_a)[rows], oracle.inverse30(want_A, prm)), (name, q, n, num, "inverse of forward vs oracle")


def _pointwise_operands(q, count, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, q, size=count, dtype=np.uint32)
    b = rng.integers(0, q, size=count, dtype=np.uint32)
    edge = [(q - 1, q - 1), (0, q - 1), (q - 1, 0), (1, q - 1), (q - 1, 1), (0, 0), (1, 1), (q - 2, q - 1), (q - 1, 2), (q // 2, 2)]
    for i, (x, y) in enumerate(edge):
        a[i], b[i] = x, y
        a[count - 1 - i], b[count - 1 - i] = x, y
    a[4096:4096 + 300], b[4096:4096 + 300] = q - 1, q - 1
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[nm for nm, _, _ in CASES])
def test_gpu_barrett30_against_exact_and_oracle(native, oracle, gpu, idx):
    import torch
    name, q, bits = CASES[idx]
    prm = params(oracle, q, bits, 2048)
    a, b = _pointwise_operands(q, 3 * 4096 + 37, q)
    dev32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(gpu)
    d_a = dev32(a)
    native.barrett30(d_a, dev32(b), q, prm.mu, bits)
    got = d_a.cpu().numpy().view(np.uint32)
    if is_native(q, bits):
        assert np.array_equal(got, (a.astype(np.uint64) * b % np.uint64(q)).astype(np.uint32)), (name, q)
    assert np.array_equal(got, oracle.pointwise30(a, b, prm)), (name, q)


@pytest.mark.gpu
@pytest.mark.parametrize("q,bits", [(TOP17, 30), (INEXACT_SHOWN[0], 29)])
def test_gpu_barrett30_grid_stride(native, oracle, gpu, q, bits):
    """more words than one pass of the grid (65536 workgroups of 256), and not a multiple of 256: the grid-stride loop and its tail"""
    import torch
    count = 65536 * 256 + 4099
    prm = params(oracle, q, bits, 2048)
    a, b = _pointwise_operands(q, count, count)
    d_a = torch.from_numpy(a.view(np.int32)).to(gpu)
    native.barrett30(d_a, torch.from_numpy(b.view(np.int32)).to(gpu), q, prm.mu, bits)
    got = d_a.cpu().numpy().view(np.uint32)
    want = oracle.pointwise30(a, b, prm)
    if is_native(q, bits):
        assert np.array_equal(want, (a.astype(np.uint64) * b % np.uint64(q)).astype(np.uint32))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (q, bad[:8], bad.size)


def _product_moduli():
    drawn = {nm: q for nm, q, _ in CASES}
    return [TOP17] + [next(drawn[nm] for nm in ("drawn-%d-0" % k, "drawn-%d-1" % k) if barrett_margin(drawn[nm]) < 1) for k in (26, 30)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2048, 4096])
@pytest.mark.parametrize("q", _product_moduli())
def test_gpu_30bit_product_against_schoolbook(native, oracle, gpu, q, n):
    """forward(a), forward(b), barrett30, inverse on the GPU: the negacyclic product, word for word the 128-bit schoolbook's"""
    import torch
    num = 2
    prm = params(oracle, q, q.bit_length(), n)
    assert is_native(q, prm.k)
    a, b = words(q, n, num, (q, n, 5)), words(q, n, num, (q, n, 6))
    dev32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(gpu)
    d_a, d_b = dev32(a), dev32(b)
    d_psi, d_psiinv = dev32(prm.psi_tab), dev32(prm.psiinv_tab)
    native.forward30(d_a, n, q, prm.mu, prm.k, d_psi, num)
    native.forward30(d_b, n, q, prm.mu, prm.k, d_psi, num)
    native.barrett30(d_a, d_b, q, prm.mu, prm.k)
    native.inverse30(d_a, n, q, prm.mu, prm.k, d_psiinv, num)
    got = d_a.cpu().numpy().view(np.uint32)
    for y in range(num):
        want = oracle.ref_polymul(a[y].astype(np.uint64), b[y].astype(np.uint64), q)
        assert np.array_equal(got[y].astype(np.uint64), want), (q, n, y)
