"""CPU: the BFV evaluator's host side (auxiliary primes) and the CPU model it is tested against (tests/bfv_eval_model.py):
the model's multiply + relinearize of oracle encryptions decrypts to the negacyclic product mod t, with noise below the
bound DESIGN.md states."""
import numpy as np
import pytest

import params as P
from bfv_eval_model import EvalModel, exact_forward, exact_inverse, negacyclic_mod_t


def is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
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


@pytest.mark.parametrize("n", [2048, 4096, 8192, 16384, 32768])
def test_aux_primes(native, n):
    from ntt_cuda_amd import bfv
    for r in range(1, 16):
        b, psi = bfv.aux_primes(n, r)
        assert len(b) == r + 1 and len(set(b)) == r + 1
        for p, w in zip(b, psi):
            assert is_prime(p) and p % (2 * n) == 1 and p < (1 << 61)
            assert native.barrett_is_exact(p)
            assert pow(w, n, p) == p - 1                      # primitive 2n-th root (order divides 2n, not n)
        assert bfv.aux_primes(n, r) == (b, psi)              # deterministic
        if r > 1:
            assert b[:r] == bfv.aux_primes(n, r - 1)[0]      # the largest candidates, in descending order
    with pytest.raises(Exception):
        bfv.aux_primes(n, 16)


def test_model_transforms_are_the_library_convention(oracle):
    n, q, psi = 2048, P.Q55[0], pow(P.PSI55[0], 32768 // 2048, P.Q55[0])
    rng = np.random.default_rng(5)
    a = rng.integers(0, q, size=n, dtype=np.uint64)
    prm = oracle.Params(n, [q], [psi])
    assert np.array_equal(exact_forward(a, q, psi), oracle.forward_batch(a, prm).reshape(n))
    assert np.array_equal(exact_inverse(exact_forward(a, q, psi), q, psi), a)


def setup_scheme(oracle, native, n, R, t, seed):
    from ntt_cuda_amd import bfv
    qs = P.Q55[:R]
    psis = [pow(w, 32768 // n, q) for w, q in zip(P.PSI55, qs)]
    r = R - 1
    bs, psis_b = bfv.aux_primes(n, r)
    model = EvalModel(oracle, n, qs[:r], psis[:r], bs, psis_b, t, native.barrett_is_exact)
    smp = oracle.bfv_sample(qs, n, seed)
    pk = np.zeros((2, R, n), dtype=np.uint64)
    pk[1] = smp["uniform"]
    sk_hat, pk = oracle.bfv_keygen_core(smp["ternary"], pk, smp["err"](), qs, psis, n)
    t0 = smp["ternary"][0].astype(np.int64)
    s_int = np.where(t0 > qs[0] // 2, t0 - qs[0], t0)

    def encrypt(m, s):
        u = oracle.bfv_sample(qs, n, s)["ternary"]
        e = np.stack([smp["err"](), smp["err"]()])
        return oracle.bfv_encrypt_core(np.stack([u, u]), pk, e, m, qs, psis, n, t).reshape(2, R, n)

    return dict(qs=qs, psis=psis, model=model, sk_hat=sk_hat.reshape(R, n), s_int=s_int, encrypt=encrypt, rng=smp["rng"], smp=smp)


@pytest.mark.parametrize("n,R", [(2048, 3), (4096, 4)])
def test_model_multiply_relin_decrypts_and_meets_noise_bound(oracle, native, n, R):
    t, gamma = 1024, P.GAMMA61
    S = setup_scheme(oracle, native, n, R, t, 31 + R)
    model, qs, psis, r = S["model"], S["qs"], S["psis"], R - 1
    rng = S["rng"]
    m1 = rng.integers(0, t, size=n, dtype=np.uint64)
    m2 = rng.integers(0, t, size=n, dtype=np.uint64)
    c1, c2 = S["encrypt"](m1, 501), S["encrypt"](m2, 502)
    v1, v2 = model.noise(c1, S["s_int"], m1), model.noise(c2, S["s_int"], m2)
    a = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(r)])
    e = np.stack([S["smp"]["err"]() for _ in range(r)])
    e_int = np.where(e[:, 0] > qs[0] // 2, e[:, 0].astype(object) - qs[0], e[:, 0].astype(object))
    b_e = int(max(abs(int(x)) for x in e_int.reshape(-1)))
    rlk = model.relin_keygen(S["sk_hat"], a, e)
    c3 = model.multiply(c1, c2)
    c = model.relinearize(c3, rlk)
    sk = np.ascontiguousarray(S["sk_hat"].reshape(-1)[: (R - 1) * n])
    want = negacyclic_mod_t(m1, m2, t)
    assert np.array_equal(oracle.bfv_decrypt(c.reshape(-1), sk, qs, psis, n, t, gamma), want)
    v = model.noise(c, S["s_int"], want)
    bound = model.noise_bound(v1, v2, b_e)
    assert v <= bound, (v, bound)
    assert bound < model.Q // (2 * t)                       # the bound itself leaves room for decryption
    # addition and subtraction, with words equal to q_i in place of zeros
    d = model.add(c1, c2)
    assert np.array_equal(oracle.bfv_decrypt(d.reshape(-1), sk, qs, psis, n, t, gamma), (m1 + m2) % t)
    d = model.add(c1, c2, sub=True)
    assert np.array_equal(oracle.bfv_decrypt(d.reshape(-1), sk, qs, psis, n, t, gamma), (m1 + t - m2) % t)
    c1q = c1.copy()
    for i, q in enumerate(qs[:r]):
        c1q[0, i][c1q[0, i] == 0] = q
        c1q[0, i][:3] = q
        c1[0, i][:3] = 0
    assert np.array_equal(model.multiply(c1q, c2), model.multiply(c1, c2))
