"""CPU: the model of the hoisted Galois automorphisms (tests/bfv_hoist_model.py) -- the block property of the NTT-slot permutation the
inner-product kernels' gather relies on, decryption of H_g and of the (weighted) sums with noise below the bounds DESIGN.md derives,
H_g against apply_galois (equal for g = 1, different for g = 2n - 1) -- and the gfx950 compilation of kernels_bfv_hoist.hip without
scratch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bfv_eval_model import negacyclic_mod_t
from bfv_galois_model import automorphism, slot_permutation
from bfv_hoist_model import HoistModel
from test_bfv_eval_host import setup_scheme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2048, 32768])
def test_slot_permutation_maps_aligned_blocks_onto_aligned_blocks(n):
    """every aligned block of 64 (a wavefront) and of 256 (a workgroup) consecutive slots is mapped onto ONE aligned block of the same
    size, permuted inside it: the gather of the inner product touches exactly the bytes it would touch without the permutation"""
    for g in (3, 5, 25, n + 1, 2 * n - 1, 12345):
        p = slot_permutation(n, g)
        assert np.array_equal(np.sort(p), np.arange(n)), g
        for size in (64, 256):
            blk = p.reshape(-1, size)
            assert np.all(blk // size == (blk // size)[:, :1]), (g, size)
            assert np.array_equal(np.sort(blk % size, axis=1), np.tile(np.arange(size), (n // size, 1))), (g, size)


def hoist_setup(oracle, native, n, R, t, seed):
    S = setup_scheme(oracle, native, n, R, t, seed)
    E = S["model"]
    S["model"] = HoistModel(oracle, n, E.qs, E.psis, E.bs, E.psis_b, t, native.barrett_is_exact)
    return S


@pytest.mark.parametrize("n,R", [(2048, 3), (4096, 4)])
def test_model_hoisted_and_sums_decrypt_and_meet_noise_bounds(oracle, native, n, R):
    t = 1024
    import params as P
    gamma = P.GAMMA61
    S = hoist_setup(oracle, native, n, R, t, 71 + R)
    M, qs, psis, r = S["model"], S["qs"], S["psis"], R - 1
    rng = S["rng"]
    sk = np.ascontiguousarray(S["sk_hat"].reshape(-1)[: r * n])
    dec = lambda c: oracle.bfv_decrypt(np.ascontiguousarray(c).reshape(-1), sk, qs, psis, n, t, gamma)
    m1 = rng.integers(0, t, size=n, dtype=np.uint64)
    c1 = S["encrypt"](m1, 801)
    v1 = M.noise(c1, S["s_int"], m1)
    half = M.Q // (2 * t)
    b_e = 0

    def key(g):
        nonlocal b_e
        a = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(r)])
        e = np.stack([S["smp"]["err"]() for _ in range(r)])
        e_int = np.where(e[:, 0] > qs[0] // 2, e[:, 0].astype(object) - qs[0], e[:, 0].astype(object))
        b_e = max(b_e, int(max(abs(int(x)) for x in e_int.reshape(-1))))
        return M.galois_keygen(S["sk_hat"], g, a, e)

    hoist = M.hoist(c1)
    for g in (3, 2 * n - 1, n + 1):
        gk = key(g)
        c = M.hoisted(c1, gk, g, hoist)
        want = automorphism(m1, g, t)
        assert np.array_equal(dec(c), want), g
        v = M.noise(c, S["s_int"], want)
        assert v <= M.bound_apply_galois(v1, b_e) < half, (g, v, M.bound_apply_galois(v1, b_e))
        if g == 2 * n - 1:
            # another decomposition than apply_galois': tau_g(D_i) holds -x where apply_galois' digit holds q_i - x
            assert not np.array_equal(c, M.apply_galois(c1, gk, g))
    # words equal to q_i read as 0
    c1z, c1q = c1.copy(), c1.copy()
    for i, q in enumerate(qs[:r]):
        c1z[:, i, :3] = 0
        c1q[:, i, :3] = q
    assert np.array_equal(M.hoisted(c1q, gk, n + 1), M.hoisted(c1z, gk, n + 1))
    gk1 = key(1)
    assert np.array_equal(M.hoisted(c1, gk1, 1, hoist), M.apply_galois(c1, gk1, 1))    # nothing negated: word for word
    # sums: G = 4 with one repeated element (a key of its own per entry, as galois_keygen_rns writes them)
    gs = [3, 2 * n - 1, 3, n + 1]
    gks = [key(g) for g in gs]
    G = len(gs)
    c = M.galois_sum(c1, gks, gs)
    want = np.zeros(n, dtype=np.uint64)
    for g in gs:
        want = (want + automorphism(m1, g, t)) % t
    assert np.array_equal(dec(c), want)
    v = M.noise(c, S["s_int"], want)
    bound = M.bound_galois_sum(v1, b_e, G)
    assert v <= bound < half, (v, bound)
    # the sum is the sum of the hoisted terms, word for word
    tot = np.zeros_like(c)
    for k, g in enumerate(gs):
        tot = M.add(tot, M.hoisted(c1, gks[k], g, hoist))
    assert np.array_equal(c, tot)
    ms = rng.integers(0, t, size=(G, n), dtype=np.uint64)
    ms[0, :4] = [0, t - 1, t // 2, t // 2 - 1]
    weights = [M.plain_ntt(ms[k]) for k in range(G)]
    c = M.galois_sum(c1, gks, gs, weights)
    want = np.zeros(n, dtype=np.uint64)
    for k, g in enumerate(gs):
        want = (want + negacyclic_mod_t(ms[k], automorphism(m1, g, t), t)) % t
    assert np.array_equal(dec(c), want)
    v = M.noise(c, S["s_int"], want)
    bound = M.bound_galois_sum_weighted(v1, b_e, G)
    assert v <= bound < half, (v, bound)


def test_hoist_kernels_compile_without_scratch():
    tool = os.path.join(ROOT, "tools", "kernel_resources.py")
    src = os.path.join(ROOT, "ntt-cuda_amd", "csrc", "kernels_bfv_hoist.hip")
    p = subprocess.run([sys.executable, tool, src, "", "--require-no-scratch", "k_"], capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [l for l in p.stdout.splitlines() if "scratch" in l]
    assert len(rows) == 3, p.stdout
    assert all("scratch    0 B" in l for l in rows), p.stdout
