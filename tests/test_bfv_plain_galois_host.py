"""CPU: the model of the BFV evaluator's plaintext operations and Galois automorphisms (tests/bfv_galois_model.py) -- the NTT-slot
permutation the galois key kernel uses, the group law of the automorphisms, end-to-end decryption of the model's outputs with noise
below the bounds DESIGN.md states -- and the gfx950 compilation of kernels_bfv_galois.hip without scratch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import params as P
from bfv_eval_model import negacyclic_mod_t
from bfv_galois_model import GaloisModel, automorphism, slot_permutation
from test_bfv_eval_host import setup_scheme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2048, 4096])
def test_slot_permutation_is_the_automorphism_in_the_ntt_domain(oracle, native, n):
    q = P.Q55[0]
    psi = pow(P.PSI55[0], 32768 // n, q)
    S = setup_scheme(oracle, native, n, 2, 1024, 3)
    M = S["model"]
    rng = np.random.default_rng(n)
    x = rng.integers(0, q, size=n, dtype=np.uint64)
    a = M.inv(x, q, psi)
    for g in (3, 5, n + 1, 2 * n - 1, int(rng.integers(0, n)) * 2 + 1):
        want = M.fwd(automorphism(a, g, q), q, psi)
        assert np.array_equal(x[slot_permutation(n, g)], want), g


def test_automorphisms_compose():
    n, q = 2048, P.Q55[1]
    rng = np.random.default_rng(9)
    a = rng.integers(0, q, size=n, dtype=np.uint64)
    for g, h in ((3, 5), (2 * n - 1, n + 1), (5, 2 * n - 1), (1025, 77)):
        assert np.array_equal(automorphism(automorphism(a, h, q), g, q), automorphism(a, g * h % (2 * n), q))
    assert np.array_equal(automorphism(a, 1, q), a)


def galois_setup(oracle, native, n, R, t, seed):
    S = setup_scheme(oracle, native, n, R, t, seed)
    E = S["model"]
    S["model"] = GaloisModel(oracle, n, E.qs, E.psis, E.bs, E.psis_b, t, native.barrett_is_exact)
    return S


@pytest.mark.parametrize("n,R", [(2048, 3), (4096, 4)])
def test_model_plain_and_galois_decrypt_and_meet_noise_bounds(oracle, native, n, R):
    t, gamma = 1024, P.GAMMA61
    S = galois_setup(oracle, native, n, R, t, 61 + R)
    M, qs, psis, r = S["model"], S["qs"], S["psis"], R - 1
    rng = S["rng"]
    sk = np.ascontiguousarray(S["sk_hat"].reshape(-1)[: r * n])
    dec = lambda c: oracle.bfv_decrypt(np.ascontiguousarray(c).reshape(-1), sk, qs, psis, n, t, gamma)
    m1 = rng.integers(0, t, size=n, dtype=np.uint64)
    m2 = rng.integers(0, t, size=n, dtype=np.uint64)
    c1 = S["encrypt"](m1, 701)
    v1 = M.noise(c1, S["s_int"], m1)
    half = M.Q // (2 * t)
    # add_plain / sub_plain
    for sub in (False, True):
        want = (m1 + t - m2) % t if sub else (m1 + m2) % t
        c = M.add_plain(c1, m2, sub=sub)
        assert np.array_equal(dec(c), want)
        assert M.noise(c, S["s_int"], want) <= M.bound_add_plain(v1) < half
    # multiply_plain: the negacyclic product mod t
    c = M.multiply_plain(c1, m2)
    want = negacyclic_mod_t(m1, m2, t)
    assert np.array_equal(dec(c), want)
    v = M.noise(c, S["s_int"], want)
    assert v <= M.bound_multiply_plain(v1) < half, (v, M.bound_multiply_plain(v1))
    # apply_galois: tau_g(m) mod t
    a = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(r)])
    e = np.stack([S["smp"]["err"]() for _ in range(r)])
    e_int = np.where(e[:, 0] > qs[0] // 2, e[:, 0].astype(object) - qs[0], e[:, 0].astype(object))
    b_e = int(max(abs(int(x)) for x in e_int.reshape(-1)))
    for g in (3, 2 * n - 1):
        gk = M.galois_keygen(S["sk_hat"], g, a, e)
        c = M.apply_galois(c1, gk, g)
        want = automorphism(m1, g, t)
        assert np.array_equal(dec(c), want), g
        v = M.noise(c, S["s_int"], want)
        assert v <= M.bound_apply_galois(v1, b_e) < half, (g, v, M.bound_apply_galois(v1, b_e))
    # words equal to q_i read as 0
    c1q = c1.copy()
    for i, q in enumerate(qs[:r]):
        c1[:, i, :3] = 0
        c1q[:, i, :3] = q
    assert np.array_equal(M.add_plain(c1q, m2), M.add_plain(c1, m2))
    assert np.array_equal(M.multiply_plain(c1q, m2), M.multiply_plain(c1, m2))


def test_galois_kernels_compile_without_scratch():
    tool = os.path.join(ROOT, "tools", "kernel_resources.py")
    src = os.path.join(ROOT, "ntt-cuda_amd", "csrc", "kernels_bfv_galois.hip")
    p = subprocess.run([sys.executable, tool, src, "", "--require-no-scratch", "k_"], capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [l for l in p.stdout.splitlines() if "scratch" in l]
    assert len(rows) == 6, p.stdout
    assert all("scratch    0 B" in l for l in rows), p.stdout
