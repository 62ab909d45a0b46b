"""GPU: the BFV evaluator against its CPU model (tests/bfv_hoist_model.py, which inherits the other two), every Q-slot word, over
what the other evaluator tests leave out: every r = 1 .. 15 on the demo set (each instantiation of k_extend<r> and k_rescale<r>, each
row and column of their constant tables) and on 61-bit primes (both sides of k_rescale<r>'s final select), the ring degrees 8192,
16384, 65536 and the 16-prime demo set at 32768, t = 2, 2^17 and 2^31, 61-bit q_i that coincide with the evaluator's auxiliary-prime
candidates, both sides of the size condition, and crafted words on the sign and boundary branches of the base conversions
(tests/bfv_sweep_inputs.py; tests/test_bfv_eval_sweep_host.py shows on the CPU that they reach those branches).  Whole arrays are
compared with np.array_equal; outputs start as sentinel words and the special prime's slot must keep them."""
import numpy as np
import pytest

import params as P
from bfv_hoist_model import HoistModel
from bfv_sweep_inputs import (crafted_operands, crafted_relin, demo_subset, find_psi, floor_half_pair, primes61, size_condition_bits,
                              size_condition_exact, wide_subset)
from test_gpu_bfv_eval import SENT, config4, demo16, q_slots, sentinel, special_untouched

GAMMA = P.GAMMA61
ALL = ("mul", "plain", "galois", "hoist")


class Sch:
    """keys, encryptions and the model for any (n, primes, t): tests/test_gpu_bfv_eval.py's Scheme with t a parameter"""

    def __init__(self, native, oracle, n, qs, psis, t, seed=7):
        import torch
        from ntt_cuda_amd import bfv
        self.native, self.oracle, self.n, self.qs, self.psis, self.t = native, oracle, n, list(qs), list(psis), t
        self.R, self.r = len(qs), len(qs) - 1
        self.ctx = bfv.BFVContext(n, qs, psis, t, GAMMA)
        self.ev = bfv.BFVEvaluator(self.ctx)
        self.smp = oracle.bfv_sample(qs, n, seed)
        self.rng = self.smp["rng"]
        pk = np.zeros((2, self.R, n), dtype=np.uint64)
        pk[1] = self.smp["uniform"]
        self.d_sk, self.d_pk = native.to_device(self.smp["ternary"]), native.to_device(pk)
        self.ctx.keygen(self.d_sk, self.d_pk, native.to_device(self.smp["err"]()))
        self.a = np.stack([np.stack([self.rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(self.r)])
        self.e = np.stack([self.smp["err"]() for _ in range(self.r)])
        self.d_rlk = torch.zeros(self.r * 2 * self.R * n, dtype=torch.int64, device="cuda")
        self.ev.relin_keygen(self.d_rlk, self.d_sk, native.to_device(self.a), native.to_device(self.e))
        torch.cuda.synchronize()
        self.sk_hat = native.to_host(self.d_sk).reshape(self.R, n)
        self.model = model_of(native, oracle, self.ev, n, qs, psis, t)

    def messages(self, count):
        return self.rng.integers(0, self.t, size=(count, self.n), dtype=np.uint64)

    def encrypt(self, m):
        """m [count][n] -> host ciphertexts [2][count][R][n] through mi355ntt_bfv_encrypt_batch"""
        count, n = m.shape[0], self.n
        u = np.stack([self.oracle.bfv_sample(self.qs, n, int(self.rng.integers(1 << 30)))["ternary"] for _ in range(count)])
        e = np.stack([np.stack([self.smp["err"]() for _ in range(count)]) for _ in range(2)])
        d_c = self.native.to_device(np.ascontiguousarray(np.stack([u, u])))
        self.ctx.encrypt_batch(d_c, self.d_pk, self.native.to_device(np.ascontiguousarray(e)), self.native.to_device(m), count)
        return self.native.to_host(d_c).reshape(2, count, self.R, n).copy()

    def close(self):
        self.ev.close()
        self.ctx.close()


def model_of(native, oracle, ev, n, qs, psis, t):
    bs = ev.aux_primes
    assert len(bs) == len(qs) and not set(bs) & set(qs)
    return HoistModel(oracle, n, qs[:-1], psis[:-1], bs, [find_psi(b, n) for b in bs], t, native.barrett_is_exact)


def compare(S, count, groups=ALL, galois=(3, None)):
    """every Q-slot word of the operations of `groups` on `count` ciphertexts, outputs written into sentinel-filled buffers"""
    import torch
    native, M, ev = S.native, S.model, S.ev
    R, r, n, t = S.R, S.r, S.n, S.t
    m = S.messages(2 * count)
    m[count, :5] = [0, t // 2 - 1, t // 2, t - 1, t + 3]         # the centred lift's boundary; a word >= t is taken mod t
    m[0, :4] = [t - 1, t // 2, t // 2 - 1, 0]
    pm = m[count:]
    a, b = S.encrypt(m[:count]), S.encrypt(pm & np.uint64(t - 1))
    idx = S.rng.choice(n, 16, replace=False)
    for i in range(r):
        a[:, :, i, idx] = S.qs[i]                                # q_i reads as 0
    d_a, d_b, d_m = native.to_device(a), native.to_device(b), native.to_device(pm)
    per = lambda f: np.stack([f(z) for z in range(count)], axis=1)

    def check(d_out, want, comps=2, what=""):
        torch.cuda.synchronize()
        assert np.array_equal(q_slots(native.to_host(d_out), comps, count, R, n), q_slots(want, comps, count, R, n)), (r, n, t, what)
        assert special_untouched(native, d_out, comps, count, R, n), (r, n, t, what)

    out = lambda comps=2: sentinel(native, comps * count * R * n)
    if "mul" in groups:
        want_rlk = M.relin_keygen(S.sk_hat, S.a, S.e)
        assert np.array_equal(native.to_host(S.d_rlk).reshape(r, 2, R, n)[:, :, :r], want_rlk[:, :, :r]), (r, n, t, "relin_keygen")
        c3 = per(lambda z: M.multiply(a[:, z], b[:, z]))
        d_c3 = out(3)
        ev.multiply(d_c3, d_a, d_b, count)
        check(d_c3, c3, 3, "multiply")
        c = per(lambda z: M.relinearize(c3[:, z], want_rlk))
        d_c = out()
        ev.relinearize(d_c, d_c3, S.d_rlk, count)
        check(d_c, c, 2, "relinearize")
        d_c = out()
        ev.multiply_relin(d_c, d_a, d_b, S.d_rlk, count)
        check(d_c, c, 2, "multiply_relin")
        for sub in (False, True):
            d_c = out()
            (ev.sub if sub else ev.add)(d_c, d_a, d_b, count)
            check(d_c, per(lambda z: M.add(a[:, z], b[:, z], sub=sub)), 2, "sub" if sub else "add")
    if "plain" in groups:
        for sub in (False, True):
            d_c = out()
            (ev.sub_plain if sub else ev.add_plain)(d_c, d_a, d_m, count)
            check(d_c, per(lambda z: M.add_plain(a[:, z], pm[z], sub=sub)), 2, "sub_plain" if sub else "add_plain")
        mhat = np.stack([M.plain_ntt(pm[z]) for z in range(count)])
        d_mhat = torch.full((count * r * n,), SENT, dtype=torch.int64, device="cuda")
        ev.plain_ntt(d_mhat, d_m, count)
        torch.cuda.synchronize()
        assert np.array_equal(native.to_host(d_mhat).reshape(count, r, n), mhat), (r, n, t, "plain_ntt")
        want = per(lambda z: M.multiply_plain_ntt(a[:, z], mhat[z]))
        d_c = out()
        ev.multiply_plain(d_c, d_a, d_m, count)
        check(d_c, want, 2, "multiply_plain")
        d_c = out()
        ev.multiply_plain_ntt(d_c, d_a, d_mhat, count, shared=False)
        check(d_c, want, 2, "multiply_plain_ntt")
        d_c = out()
        ev.multiply_plain_ntt(d_c, d_a, d_mhat[: r * n], count, shared=True)
        check(d_c, per(lambda z: M.multiply_plain_ntt(a[:, z], mhat[0])), 2, "multiply_plain_ntt shared")
    dev_keys, host_keys = {}, {}

    def key(g):
        if g not in dev_keys:
            dev_keys[g] = torch.zeros(r * 2 * R * n, dtype=torch.int64, device="cuda")
            ev.galois_keygen(dev_keys[g], S.d_sk, g, native.to_device(S.a), native.to_device(S.e))
            host_keys[g] = M.galois_keygen(S.sk_hat, g, S.a, S.e)
            torch.cuda.synchronize()
            assert np.array_equal(native.to_host(dev_keys[g]).reshape(r, 2, R, n)[:, :, :r], host_keys[g][:, :, :r]), (r, n, t, "galois_keygen", g)
        return dev_keys[g], host_keys[g]

    if "galois" in groups:
        for g in galois:
            g = 2 * n - 1 if g is None else g
            d_gk, gk = key(g)
            d_c = out()
            ev.apply_galois(d_c, d_a, d_gk, g, count)
            check(d_c, per(lambda z: M.apply_galois(a[:, z], gk, g)), 2, "apply_galois %d" % g)
    if "hoist" in groups:
        group = ev.hoist_group
        gs = [3, n + 1, 3, 2 * n - 1, 5, 25, 2 * n - 3, 1, 5][: group + 1]         # more elements than one scratch group, 3 repeated
        G = len(gs)
        assert G == group + 1 and len(set(gs)) < G
        keys = [key(g) for g in gs]
        d_gk, gks = torch.cat([k[0] for k in keys]), [k[1] for k in keys]
        hoists = [M.hoist(a[:, z]) for z in range(count)]
        d_out = sentinel(native, G * 2 * count * R * n)
        ev.apply_galois_hoisted(d_out, d_a, d_gk, gs, count)
        torch.cuda.synchronize()
        got = native.to_host(d_out).reshape(G, 2, count, R, n)
        for k, g in enumerate(gs):
            want = per(lambda z: M.hoisted(a[:, z], gks[k], g, hoists[z]))
            assert np.array_equal(got[k][:, :, :r], want[:, :, :r]), (r, n, t, "apply_galois_hoisted", k, g)
        assert np.all(got[:, :, :, R - 1] == np.uint64(SENT))
        ms = S.messages(G)
        ms[0, :5] = [0, t - 1, t // 2, t // 2 - 1, t + 3]
        d_w = torch.zeros(G * r * n, dtype=torch.int64, device="cuda")
        ev.plain_ntt(d_w, native.to_device(ms), G)
        weights = [M.plain_ntt(ms[k]) for k in range(G)]
        for d_wt, wt in ((None, None), (d_w, weights)):
            d_c = out()
            ev.galois_sum(d_c, d_a, d_gk, gs, count, weights=d_wt)
            check(d_c, per(lambda z: M.galois_sum(a[:, z], gks, gs, wt)), 2, "galois_sum %s" % ("plain" if wt is None else "weighted"))
    return group if "hoist" in groups else None


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(1, 16))
def test_every_r_at_n2048(native, oracle, gpu, r):
    """every operation, count = 3 (gridDim.z), on the first r + 1 primes of the reference demo's 16-prime set"""
    n = 2048
    qs, psis = demo_subset(n, r)
    S = Sch(native, oracle, n, qs, psis, 1024)
    group = compare(S, 3)
    if r == 1:
        assert group == 8                                         # the one r where the group is the kernels' limit, not the scratch
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(1, 16))
def test_both_correction_signs_at_every_r(native, oracle, gpu, r):
    """both sides of k_rescale<r>'s final select, sk_bq and sk_neg_bq.  The demo set's Q is far below B from r = 4 on, and no product
    on it has a negative Shenoy-Kumaresan correction.  Constant floor(Q/2) operands on 61-bit primes, where Q is about B, have both
    signs at every r (tests/test_bfv_eval_sweep_host.py asserts it): their product, every word"""
    import torch
    from ntt_cuda_amd import bfv
    n = 2048
    qs, psis = wide_subset(n, r, native.barrett_is_exact)
    ctx = bfv.BFVContext(n, qs, psis, 1024, GAMMA)
    ev = bfv.BFVEvaluator(ctx)
    M = model_of(native, oracle, ev, n, qs, psis, 1024)
    a, b = floor_half_pair(qs, n)
    d_c3 = sentinel(native, 3 * (r + 1) * n)
    ev.multiply(d_c3, native.to_device(a), native.to_device(b), 1)
    torch.cuda.synchronize()
    want = M.multiply(a[:, 0], b[:, 0])
    assert np.array_equal(q_slots(native.to_host(d_c3), 3, 1, r + 1, n), q_slots(want, 3, 1, r + 1, n)), (r, "multiply, floor(Q/2) operands")
    assert special_untouched(native, d_c3, 3, 1, r + 1, n)
    ev.close()
    ctx.close()


def primes_at(native, n, count, seed=41):
    qs = primes61(count, 1 << 31, native.barrett_is_exact, seed)
    return qs, [find_psi(q, n) for q in qs]


@pytest.mark.gpu
@pytest.mark.parametrize("n,r", [(8192, 3), (16384, 3), (32768, 15), (65536, 2)])
def test_ring_degrees(native, oracle, gpu, n, r):
    """multiply, relinearize, apply_galois; the hoisted automorphisms and their sums (galois_slot depends on log2 n) at every degree
    the hoisted tests leave out; n = 32768 is the whole 16-prime demo set; n = 65536 has no demo roots, so 61-bit primes
    = 1 (mod 2^31) found here"""
    if n == 65536:
        qs, psis = primes_at(native, n, r + 1)
    elif r == 15:
        qs, psis = demo16()
    else:
        qs, psis = demo_subset(n, r)
    S = Sch(native, oracle, n, qs, psis, 1024)
    compare(S, 1 if n >= 32768 else 2, ("mul", "galois") if n == 32768 else ("mul", "galois", "hoist"))
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["t2", "t2^31", "t2^17_config4"])
def test_values_of_t_and_61_bit_moduli(native, oracle, gpu, case):
    """t = 2 on 61-bit q_i of which two ARE the evaluator's first auxiliary candidates (it must step past them); t = 2^31 on 61-bit
    q_i = 1 (mod 2^31) -- the nearest such candidate lies 2^31 below 2^61, far under the few auxiliary primes, so that set cannot
    coincide with them and the coincidence is tested at t = 2; t = 2^17 on configs[4]'s 60-bit primes"""
    from ntt_cuda_amd import bfv
    n, r = 4096, 3
    if case == "t2^17_config4":
        n, t = 32768, 1 << 17
        qs, psis = config4()
        r = len(qs) - 1
    else:
        t = 2 if case == "t2" else 1 << 31
        qs, _ = primes_at(native, n, r + 1)
        assert all(q % (1 << 31) == 1 and q % (2 * n) == 1 and q.bit_length() == 61 for q in qs)
        if case == "t2":
            cand, _ = bfv.aux_primes(n, r)
            qs = [cand[0], qs[0], cand[2], qs[1]]                 # the special prime is excluded as well: none of the four may be reused
        psis = [find_psi(q, n) for q in qs]
    assert all(q % t == 1 for q in qs[:r])
    S = Sch(native, oracle, n, qs, psis, t)
    listed, _ = bfv.aux_primes(n, r)
    if case == "t2":
        assert set(listed) & set(qs[:r]) == {qs[0], qs[2]}
        assert S.ev.aux_primes != listed
        # the next candidates in line, in descending order
        more, _ = bfv.aux_primes(n, r + 2)
        assert S.ev.aux_primes == [b for b in more if b not in qs][: r + 1]
    assert not set(S.ev.aux_primes) & set(qs)
    compare(S, 1 if n == 32768 else 2, ("mul", "plain", "galois"))
    S.close()


@pytest.mark.gpu
def test_size_condition_on_both_sides(native, oracle, gpu):
    """fifteen 61-bit primes at n = 2^15: the largest t the documented inequality admits is accepted, satisfies the exact condition
    4 n t Q + 2 (r + 1) B < B m_sk on the primes the evaluator reports and multiplies word for word; the next t is refused"""
    from ntt_cuda_amd import bfv
    n, r = 32768, 15
    qs, psis = primes_at(native, n, r + 1)
    listed, _ = bfv.aux_primes(n, r)
    assert not set(listed) & set(qs)
    lts = [lt for lt in range(1, 32) if size_condition_bits(n, 1 << lt, qs[:r], listed)]
    t_ok, t_bad = 1 << lts[-1], 1 << (lts[-1] + 1)
    assert lts == list(range(1, lts[-1] + 1)) and t_bad <= 1 << 31 and all(q % t_bad == 1 for q in qs)
    print("largest accepted t = 2^%d, smallest rejected t = 2^%d" % (lts[-1], lts[-1] + 1))
    ctx = bfv.BFVContext(n, qs, psis, t_bad, GAMMA)
    with pytest.raises(Exception, match=r"\[-2\]"):
        bfv.BFVEvaluator(ctx)
    ctx.close()
    S = Sch(native, oracle, n, qs, psis, t_ok)
    assert S.ev.aux_primes == listed
    assert size_condition_bits(n, t_ok, qs[:r], S.ev.aux_primes) and size_condition_exact(n, t_ok, qs[:r], S.ev.aux_primes)
    compare(S, 1, ("mul",))
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 2, 4, 15])
def test_crafted_conversion_edges(native, oracle, gpu, r):
    """arbitrary words, not encryptions: the extension's r_m on and around its sign split, tensor coefficients that put t D / Q on and
    next to integers with both signs, the largest tensor coefficients, the Shenoy-Kumaresan correction of both signs, and the widest
    relinearization sums; on 61-bit primes, where Q is about B (tests/test_bfv_eval_sweep_host.py asserts that each is reached)"""
    import torch
    from ntt_cuda_amd import bfv
    n, t = 2048, 1024
    qs, psis = wide_subset(n, r, native.barrett_is_exact)
    R = r + 1
    ctx = bfv.BFVContext(n, qs, psis, t, GAMMA)
    ev = bfv.BFVEvaluator(ctx)
    M = model_of(native, oracle, ev, n, qs, psis, t)
    a, b, _ = crafted_operands(qs, t, n, 100 + r)
    count = a.shape[1]
    rng = np.random.default_rng(300 + r)
    rlk = np.stack([np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(2)]) for _ in range(r)])
    d_a, d_b, d_rlk = native.to_device(a), native.to_device(b), native.to_device(rlk)
    per = lambda f: np.stack([f(z) for z in range(count)], axis=1)

    def check(d_out, want, comps, cnt, what):
        torch.cuda.synchronize()
        got = q_slots(native.to_host(d_out), comps, cnt, R, n)
        want = q_slots(want, comps, cnt, R, n)
        for z in range(cnt):
            assert np.array_equal(got[:, z], want[:, z]), (r, what, z)
        assert special_untouched(native, d_out, comps, cnt, R, n), (r, what)

    c3 = per(lambda z: M.multiply(a[:, z], b[:, z]))
    d_c3 = sentinel(native, 3 * count * R * n)
    ev.multiply(d_c3, d_a, d_b, count)
    check(d_c3, c3, 3, count, "multiply")
    c = per(lambda z: M.relinearize(c3[:, z], rlk))
    d_c = sentinel(native, 2 * count * R * n)
    ev.relinearize(d_c, native.to_device(np.ascontiguousarray(c3)), d_rlk, count)
    check(d_c, c, 2, count, "relinearize")
    d_c = sentinel(native, 2 * count * R * n)
    ev.multiply_relin(d_c, d_a, d_b, d_rlk, count)
    check(d_c, c, 2, count, "multiply_relin")
    x3, top = crafted_relin(qs, n, 200 + r)
    for key, name in ((top, "largest key"), (rlk, "random key")):
        d_c = sentinel(native, 2 * R * n)
        ev.relinearize(d_c, native.to_device(x3), native.to_device(key), 1)
        check(d_c, M.relinearize(x3[:, 0], key).reshape(2, 1, R, n), 2, 1, "relinearize, crafted digits, " + name)
    ev.close()
    ctx.close()
