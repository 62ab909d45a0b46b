"""CPU: what the GPU sweep of the BFV evaluator (tests/test_gpu_bfv_eval_sweep.py) relies on.
  - The crafted inputs of tests/bfv_sweep_inputs.py reach what they were built to reach: every target word of the extension's small
    Montgomery factor r_m (recomputed here from the definition), both signs of the tensor coefficient D, t D mod Q within r of 0 and
    of Q, both signs of the Shenoy-Kumaresan correction (at every r = 1 .. 15 for the constant floor(Q/2) pair), every digit case
    of the relinearization.  They run on 61-bit primes (wide_subset), where Q is about B.
  - The model the GPU is compared with is itself right at r = 1, 5 and 15: its outputs decrypt through the oracle with noise inside the
    DESIGN.md bounds.
  - The prime walk and the size-condition arithmetic the GPU tests use."""
import numpy as np
import pytest

import params as P
from bfv_eval_model import negacyclic_mod_t
from bfv_galois_model import automorphism
from bfv_hoist_model import HoistModel
from bfv_sweep_inputs import (MT, RM_TARGETS, crafted_operands, crafted_relin, demo_subset, find_psi, floor_half_pair, is_prime, primes61,
                              product, rescale_trace, rescale_values, size_condition_bits, size_condition_exact, wide_subset)

N, T = 2048, 1024
CRAFT_R = [1, 2, 4, 15]


def model_for(oracle, native, n, r, t, wide=False):
    """on the demo set's first r + 1 primes, or on wide_subset's; the auxiliary primes are the evaluator's first candidates, which
    neither set touches"""
    from ntt_cuda_amd import bfv
    qs, psis = wide_subset(n, r, native.barrett_is_exact) if wide else demo_subset(n, r)
    bs, psis_b = bfv.aux_primes(n, r)
    assert not set(bs) & set(qs)
    assert size_condition_bits(n, t, qs[:r], bs) and size_condition_exact(n, t, qs[:r], bs)
    return qs, psis, HoistModel(oracle, n, qs[:r], psis[:r], bs, psis_b, t, native.barrett_is_exact)


def extend_rm(x, qs):
    """the small Montgomery factor of EvalModel.extend for one coefficient given as residues, before centring: an integer in [0, 2^32)"""
    Q = product(qs)
    X = 0
    for xi, q in zip(x, qs):
        Qi = Q // q
        X += (int(xi) * pow(Qi % q, -1, q) % q) * Qi
    mx = (X % Q) * MT % Q
    conv = sum(((mx % q) * pow((Q // q) % q, -1, q) % q) * (Q // q) for q in qs)
    return (-conv * pow(Q, -1, MT)) % MT


def test_prime_walk(native):
    for modulus, count in ((1 << 31, 4), (1 << 16, 3)):
        qs = primes61(count, modulus, native.barrett_is_exact, 11)
        assert len(set(qs)) == count and qs == sorted(qs, reverse=True)
        for q in qs:
            assert is_prime(q) and q % modulus == 1 and q.bit_length() == 61 and native.barrett_is_exact(q)
            assert pow(find_psi(q, 32768), 32768, q) == q - 1
        assert primes61(count, modulus, native.barrett_is_exact, 11) == qs
        assert not set(primes61(2, modulus, native.barrett_is_exact, 11, exclude=qs[:1])) & set(qs[:1])


@pytest.mark.parametrize("r", CRAFT_R)
def test_crafted_extension_hits_every_target(oracle, native, r):
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    a, b, ext = crafted_operands(qs_all, T, N, 100 + r)
    assert {(name, h) for name, h, _, _ in ext} == {("a", 0), ("a", 1), ("b", 0), ("b", 1)}
    hit = {}
    for name, h, p, target in ext:
        op = a if name == "a" else b
        x = [int(op[h, 0, i, p]) for i in range(r)]
        assert all(0 <= xi < q for xi, q in zip(x, qs_all))
        rm = extend_rm(x, qs_all[:r])
        print("r=%d %s%d[%d]: r_m = %#x" % (r, name, h, p, rm))
        assert rm == target, (name, h, p, hex(rm), hex(target))
        hit.setdefault((name, h, target), set()).add(p)
    for name in "ab":
        for h in range(2):
            for target in RM_TARGETS:
                assert len(hit[(name, h, target)]) >= 3                   # several positions per case and component
    # the model's extension of these coefficients is x or x - Q, and with r_m centred as the target says (2^31 and above negative)
    # m~ x~ - r_m Q is the fast conversion's sum, in [0, r Q)
    for h in range(2):
        got = M.extend(M.canon(a[:, 0])[h])
        X = M.crt(M.canon(a[:, 0])[h], M.qs)
        for name, hh, p, target in ext:
            if name == "a" and hh == h:
                assert got[p] in (X[p], X[p] - M.Q)
                rm_c = target if target < MT // 2 else target - MT
                assert 0 <= got[p] * MT - rm_c * M.Q < r * M.Q, (h, p, hex(target))


@pytest.mark.parametrize("r", CRAFT_R)
def test_crafted_rescale_reaches_the_edges(oracle, native, r):
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    a, b, _ = crafted_operands(qs_all, T, N, 100 + r)
    Q, B = M.Q, product(M.bs[:-1])
    traces = []
    for z in range(4):
        want, tr = rescale_trace(M, a[:, z], b[:, z])                     # one model product per ciphertext
        traces.append(tr)
        for c in range(3):
            for i, q in enumerate(M.qs):                                  # the trace is the model's own path
                assert np.array_equal((tr[c]["y"] % q).astype(np.uint64), want[c, i])
    # b = (1, 0): the tensor coefficients of ciphertext 1 are the centred values that were placed
    vals = dict(rescale_values(M.qs, T))
    D0 = traces[1][0]["D"]
    placed = {int(v) for v in D0} | {int(v) + Q for v in D0}
    for label, v in vals.items():
        assert v in placed, label
    assert all(int(v) == 0 for v in traces[1][2]["D"])                    # D = 0: the whole third component
    assert all(int(v) == -1 for v in traces[2][0]["D"]) and all(int(v) == -1 for v in traces[2][1]["D"])
    D = np.concatenate([traces[z][c]["D"] for z in range(4) for c in range(3)])
    tdq = np.concatenate([traces[z][c]["tdq"] for z in range(4) for c in range(3)])
    al = np.concatenate([traces[z][c]["alpha_sk"] for z in range(4) for c in range(3)])
    y = np.concatenate([traces[z][c]["y"] for z in range(4) for c in range(3)])
    print("r=%d: D < 0: %d, D > 0: %d, D = 0: %d; alpha_sk < 0: %d, > 0: %d, = 0: %d; min t D mod Q: %d, Q - max: %d"
          % (r, np.sum(D < 0), np.sum(D > 0), np.sum(D == 0), np.sum(al < 0), np.sum(al > 0), np.sum(al == 0), min(tdq), Q - max(tdq)))
    assert np.any(D < 0) and np.any(D > 0) and np.any(D == 0)
    assert any(0 < int(v) <= r for v in tdq) and any(0 < Q - int(v) <= r for v in tdq)
    assert any(int(d) < 0 and int(v) != 0 for d, v in zip(D, tdq))        # a negative D off the integers: floor, not truncation
    assert max(abs(int(v)) for v in D) > N * (Q // 2) ** 2 // 2           # the constant floor(Q/2) pair: near the largest tensor
    # Shenoy-Kumaresan: y = conv_B(y) - alpha_sk B with 0 <= conv_B(y) < r B.  A negative y needs alpha_sk >= 1; alpha_sk < 0 needs
    # y >= B, and |y| reaches n t Q / 4 here, far above B on these primes
    assert np.any(al > 0) and np.any(al < 0)
    assert all(int(v) >= 1 for v, yy in zip(al, y) if int(yy) < 0)
    assert all(int(v) < 0 for v, yy in zip(al, y) if int(yy) >= r * B)
    assert max(abs(int(v)) for v in al) + r < M.bs[-1] // 2               # inside what the correction recovers


@pytest.mark.parametrize("r", CRAFT_R)
def test_crafted_relinearization_inputs(oracle, native, r):
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    c3, rlk = crafted_relin(qs_all, N, 200 + r)
    lo = min(M.qs)
    for i, q in enumerate(M.qs):
        assert {0, q, q - 1, lo - 1} == {int(v) for v in np.unique(c3[2, 0, i])}
        assert np.all(rlk[:, :, i] == np.uint64(q - 1))
    for i in range(r - 1):                                                # every pair of cases meets in the words of adjacent slots
        w0, w1 = c3[2, 0, i].tolist(), c3[2, 0, i + 1].tolist()
        assert len(set(zip(w0, w1))) == len(set(w0)) * len(set(w1)), i
    # q_i stands for the digit 0 in every slot ("A digit word equal to q_i reads as 0, as in every other step")
    z = c3[:, 0].copy()
    for i, q in enumerate(M.qs):
        z[2, i][z[2, i] == np.uint64(q)] = 0
    got = M.relinearize(c3[:, 0], rlk)
    assert np.array_equal(got, M.relinearize(z, rlk))
    # the key is the constant -1 in the transform domain, so from the definition, without the model's transforms or its reading of
    # words: c_h[j] - sum_i ([d_2]_{q_i} mod q_j), the digit of a word q_i being 0
    for j, qj in enumerate(M.qs):
        s = np.zeros(N, dtype=object)
        for i, qi in enumerate(M.qs):
            s = s + (c3[2, 0, i].astype(object) % qi) % qj
        for h in range(2):
            assert np.array_equal(got[h, j], ((c3[h, 0, j].astype(object) % qj - s) % qj).astype(np.uint64)), (h, j)


@pytest.mark.parametrize("r", range(1, 16))
def test_floor_half_pair_takes_both_correction_signs(oracle, native, r):
    """what the GPU sweep multiplies at every r to reach both sides of k_rescale<r>'s final select"""
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    a, b = floor_half_pair(qs_all, N)
    want, tr = rescale_trace(M, a[:, 0], b[:, 0])
    h = M.Q // 2
    k = np.arange(N).astype(object)
    for c, mult in enumerate((1, 2, 1)):
        assert np.array_equal(tr[c]["D"], mult * (2 * k + 2 - N) * h * h)
        for i, q in enumerate(M.qs):
            assert np.array_equal((tr[c]["y"] % q).astype(np.uint64), want[c, i])
        al = tr[c]["alpha_sk"]
        print("r=%d c%d: alpha_sk < 0: %d, > 0: %d, = 0: %d" % (r, c, np.sum(al < 0), np.sum(al > 0), np.sum(al == 0)))
        assert np.any(al < 0) and np.any(al > 0)
        assert max(abs(int(v)) for v in al) + r < M.bs[-1] // 2


def scheme_for(oracle, native, n, r, t, seed):
    qs, psis, M = model_for(oracle, native, n, r, t)
    R = r + 1
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

    return dict(qs=qs, psis=psis, model=M, sk_hat=sk_hat.reshape(R, n), s_int=s_int, encrypt=encrypt, rng=smp["rng"], smp=smp)


@pytest.mark.parametrize("r", [1, 5, 15])
def test_model_decrypts_and_meets_the_noise_bounds(oracle, native, r):
    """multiply + relinearize, the plaintext operations, apply_galois, the hoisted form and both sums at n = 2048 on the first r + 1
    primes of the demo set.  r = 1: Q is one 54-bit prime, so t = 16 (the multiplication bound n t (V1 + V2)(n + 4) must stay below
    Q / (2t)), and the key-switching keys carry no error: one digit as wide as Q multiplies the key's error by up to n q_0, beyond
    Q / (2t) for any nonzero error.  The bounds are DESIGN.md's with B_e = 0 there."""
    n, R, gamma = N, r + 1, P.GAMMA61
    t = 16 if r == 1 else T
    S = scheme_for(oracle, native, n, r, t, 900 + r)
    M, qs, psis, rng = S["model"], S["qs"], S["psis"], S["rng"]
    sk = np.ascontiguousarray(S["sk_hat"].reshape(-1)[: r * n])
    dec = lambda c: oracle.bfv_decrypt(np.ascontiguousarray(c).reshape(-1), sk, qs, psis, n, t, gamma)
    half = M.Q // (2 * t)
    m1 = rng.integers(0, t, size=n, dtype=np.uint64)
    m2 = rng.integers(0, t, size=n, dtype=np.uint64)
    m2[:4] = [0, t // 2 - 1, t // 2, t - 1]
    c1, c2 = S["encrypt"](m1, 901), S["encrypt"](m2, 902)
    assert np.array_equal(dec(c1), m1)
    v1, v2 = M.noise(c1, S["s_int"], m1), M.noise(c2, S["s_int"], m2)
    b_e = 0

    def samples():
        nonlocal b_e
        a = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(r)])
        e = np.stack([S["smp"]["err"]() for _ in range(r)])
        if r == 1:
            e = np.zeros_like(e)
        e_int = np.where(e[:, 0] > qs[0] // 2, e[:, 0].astype(object) - qs[0], e[:, 0].astype(object))
        b_e = max(b_e, int(max(abs(int(x)) for x in e_int.reshape(-1))))
        return a, e

    rlk = M.relin_keygen(S["sk_hat"], *samples())
    c = M.relinearize(M.multiply(c1, c2), rlk)
    want = negacyclic_mod_t(m1, m2, t)
    assert np.array_equal(dec(c), want)
    v, bound = M.noise(c, S["s_int"], want), M.noise_bound(v1, v2, b_e)
    print("r=%d multiply_relin: noise 2^%.1f, bound 2^%.1f, Q/2t 2^%.1f" % (r, np.log2(float(v) + 1), np.log2(float(bound)), np.log2(float(half))))
    assert v <= bound < half, (v, bound)
    for sub in (False, True):
        want = (m1 + t - m2) % t if sub else (m1 + m2) % t
        c = M.add(c1, c2, sub=sub)
        assert np.array_equal(dec(c), want)
        c = M.add_plain(c1, m2, sub=sub)
        assert np.array_equal(dec(c), want)
        assert M.noise(c, S["s_int"], want) <= M.bound_add_plain(v1) < half
    c = M.multiply_plain(c1, m2)
    want = negacyclic_mod_t(m1, m2, t)
    assert np.array_equal(dec(c), want)
    assert M.noise(c, S["s_int"], want) <= M.bound_multiply_plain(v1) < half
    gs = [3, 2 * n - 1, 3, n + 1]
    gks = [M.galois_keygen(S["sk_hat"], g, *samples()) for g in gs]
    hoist = M.hoist(c1)
    for g, gk in zip(gs[1:], gks[1:]):
        want = automorphism(m1, g, t)
        for c in (M.apply_galois(c1, gk, g), M.hoisted(c1, gk, g, hoist)):
            assert np.array_equal(dec(c), want), g
            v = M.noise(c, S["s_int"], want)
            assert v <= M.bound_apply_galois(v1, b_e) < half, (g, v)
    G = len(gs)
    c = M.galois_sum(c1, gks, gs)
    want = np.zeros(n, dtype=np.uint64)
    for g in gs:
        want = (want + automorphism(m1, g, t)) % t
    assert np.array_equal(dec(c), want)
    v, bound = M.noise(c, S["s_int"], want), M.bound_galois_sum(v1, b_e, G)
    assert v <= bound < half, (v, bound)
    ms = rng.integers(0, t, size=(G, n), dtype=np.uint64)
    ms[0, :4] = [0, t - 1, t // 2, t // 2 - 1]
    c = M.galois_sum(c1, gks, gs, [M.plain_ntt(ms[k]) for k in range(G)])
    want = np.zeros(n, dtype=np.uint64)
    for k, g in enumerate(gs):
        want = (want + negacyclic_mod_t(ms[k], automorphism(m1, g, t), t)) % t
    assert np.array_equal(dec(c), want)
    v, bound = M.noise(c, S["s_int"], want), M.bound_galois_sum_weighted(v1, b_e, G)
    assert v <= bound < half, (v, bound)


def test_size_condition_arithmetic(native):
    """the documented bit-count inequality on fifteen 61-bit primes at n = 2^15: the largest t it admits and the next one, and the
    exact condition 4 n t Q + 2 (r + 1) B < B m_sk it stands for, which holds at both (the bit count is the conservative side)"""
    from ntt_cuda_amd import bfv
    n, r = 32768, 15
    qs = primes61(r + 1, 1 << 31, native.barrett_is_exact, 41)
    bs, _ = bfv.aux_primes(n, r)
    assert not set(bs) & set(qs)
    accepted = [lt for lt in range(1, 32) if size_condition_bits(n, 1 << lt, qs[:r], bs)]
    assert accepted == list(range(1, accepted[-1] + 1)) and accepted[-1] < 31
    for lt in (accepted[-1], accepted[-1] + 1):
        assert size_condition_exact(n, 1 << lt, qs[:r], bs)
    # and a set the exact condition refuses is refused by the bit count too: t large enough, were it allowed
    lt = next(lt for lt in range(1, 200) if not size_condition_exact(n, 1 << lt, qs[:r], bs))
    assert lt > accepted[-1] + 1 and not size_condition_bits(n, 1 << lt, qs[:r], bs)
