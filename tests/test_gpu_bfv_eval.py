"""GPU: the BFV evaluator (include/mi355ntt.h, "BFV evaluation") -- every output word against the CPU model
(tests/bfv_eval_model.py), round trips through the existing encrypt / decrypt drivers, batches, non-canonical inputs, the
complete relinearization key generation, a Barrett-inexact BFV object, argument errors and concurrent streams."""
import ctypes
import os

import numpy as np
import pytest

import params as P
from bfv_eval_model import EvalModel, negacyclic_mod_t

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat1_decryption_n4096.npz")
T, GAMMA = 1024, P.GAMMA61


def demo_set(n, R):
    qs = P.Q55[:R]
    return qs, [pow(w, 32768 // n, q) for w, q in zip(P.PSI55, qs)]


def config4():
    return P.Q60 + [P.Q60_SPECIAL], P.PSI60 + [P.PSI60_SPECIAL]


def demo16():
    """the reference demo's 16-prime set (demo.cu:35-36, n = 2^15, log q = 880; the special prime last), as bench.py carries it"""
    from bench import DEMO_PSI16, DEMO_Q16
    return list(DEMO_Q16), list(DEMO_PSI16)


class Scheme:
    """keys on the GPU (drivers fed with oracle-style samples), encryption of numpy messages, relinearization key from explicit samples"""

    def __init__(self, native, oracle, n, qs, psis, seed=7, exact_on_inexact_primes=False, model=True):
        import torch
        from ntt_cuda_amd import bfv
        self.native, self.oracle, self.n, self.qs, self.psis = native, oracle, n, qs, psis
        self.R, self.r = len(qs), len(qs) - 1
        self.ctx = bfv.BFVContext(n, qs, psis, T, GAMMA, exact_on_inexact_primes=exact_on_inexact_primes)
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
        self.model = EvalModel(oracle, n, qs[:-1], psis[:-1], self.ev.aux_primes, self._aux_psis(), T, native.barrett_is_exact) if model else None

    def _aux_psis(self):
        from ntt_cuda_amd import bfv
        bs, ps = bfv.aux_primes(self.n, self.r)
        if bs == self.ev.aux_primes:
            return ps
        out = []
        for b in self.ev.aux_primes:
            out.append(next(w for w in (pow(x, (b - 1) // (2 * self.n), b) for x in range(2, 1000)) if pow(w, self.n, b) == b - 1))
        return out

    def messages(self, count):
        return self.rng.integers(0, T, size=(count, self.n), dtype=np.uint64)

    def encrypt(self, m):
        """m [count][n] -> device ciphertexts [2][count][R][n] through mi355ntt_bfv_encrypt_batch"""
        count, n, R = m.shape[0], self.n, self.R
        u = np.stack([self.oracle.bfv_sample(self.qs, n, int(self.rng.integers(1 << 30)))["ternary"] for _ in range(count)])
        c = np.stack([u, u])
        e = np.stack([np.stack([self.smp["err"]() for _ in range(count)]) for _ in range(2)])
        d_c = self.native.to_device(np.ascontiguousarray(c))
        self.ctx.encrypt_batch(d_c, self.d_pk, self.native.to_device(np.ascontiguousarray(e)), self.native.to_device(m), count)
        return d_c

    def decrypt(self, d_c, count):
        import torch
        c = d_c.clone()
        self.ctx.decrypt_batch(c, self.d_sk, count)
        torch.cuda.synchronize()
        h = self.native.to_host(c).reshape(2, count, self.R, self.n)
        return h[0, :, self.R - 2, :]

    def close(self):
        self.ev.close()
        self.ctx.close()


def q_slots(x, comps, count, R, n):
    return np.asarray(x).reshape(comps, count, R, n)[:, :, : R - 1]


SENT = 0x5A5A5A5A5A5A5A5A


def sentinel(native, words):
    import torch
    return torch.full((words,), SENT, dtype=torch.int64, device="cuda")


def special_untouched(native, d, comps, count, R, n):
    h = native.to_host(d).reshape(comps, count, R, n)
    return bool(np.all(h[:, :, R - 1] == np.uint64(SENT)))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["demo4096", "config4"])
def test_every_word_matches_the_model(native, oracle, gpu, cfg):
    import torch
    n, (qs, psis) = (4096, demo_set(4096, 3)) if cfg == "demo4096" else (32768, config4())
    S = Scheme(native, oracle, n, qs, psis)
    R, r, M = S.R, S.r, S.model
    # relinearization key from explicit samples
    want_rlk = M.relin_keygen(S.sk_hat, S.a, S.e)
    got_rlk = native.to_host(S.d_rlk).reshape(r, 2, R, n)
    assert np.array_equal(got_rlk[:, :, :r], want_rlk[:, :, :r])
    m = S.messages(2)
    d_a, d_b = S.encrypt(m[:1]), S.encrypt(m[1:])
    a, b = native.to_host(d_a).reshape(2, R, n), native.to_host(d_b).reshape(2, R, n)
    d_c3 = sentinel(native, 3 * R * n)
    S.ev.multiply(d_c3, d_a, d_b)
    torch.cuda.synchronize()
    c3 = M.multiply(a, b)
    assert np.array_equal(q_slots(native.to_host(d_c3), 3, 1, R, n), q_slots(c3, 3, 1, R, n))
    assert special_untouched(native, d_c3, 3, 1, R, n)
    d_c = sentinel(native, 2 * R * n)
    S.ev.relinearize(d_c, d_c3, S.d_rlk)
    torch.cuda.synchronize()
    c = M.relinearize(c3, want_rlk)
    assert np.array_equal(q_slots(native.to_host(d_c), 2, 1, R, n), q_slots(c, 2, 1, R, n))
    assert special_untouched(native, d_c, 2, 1, R, n)
    for sub in (False, True):
        d_s = sentinel(native, 2 * R * n)
        (S.ev.sub if sub else S.ev.add)(d_s, d_a, d_b)
        torch.cuda.synchronize()
        assert np.array_equal(q_slots(native.to_host(d_s), 2, 1, R, n), q_slots(M.add(a, b, sub=sub), 2, 1, R, n))
        assert special_untouched(native, d_s, 2, 1, R, n)
    # and the fused call gives the same words as the two steps
    d_f = sentinel(native, 2 * R * n)
    S.ev.multiply_relin(d_f, d_a, d_b, S.d_rlk)
    torch.cuda.synchronize()
    assert np.array_equal(q_slots(native.to_host(d_f), 2, 1, R, n), q_slots(c, 2, 1, R, n))
    assert np.array_equal(S.decrypt(d_f, 1)[0], negacyclic_mod_t(m[0], m[1], T))
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["demo4096", "config4", "demo16"])
def test_round_trip_through_the_drivers(native, oracle, gpu, cfg):
    import torch
    if cfg == "demo4096":
        n, (qs, psis) = 4096, demo_set(4096, 3)
    elif cfg == "config4":
        n, (qs, psis) = 32768, config4()
    else:
        n, (qs, psis) = 32768, demo16()
    S = Scheme(native, oracle, n, qs, psis, model=False)
    assert len(S.ev.aux_primes) == S.r + 1
    m = S.messages(4)
    d = [S.encrypt(m[i: i + 1]) for i in range(4)]
    out = torch.empty_like(d[0])
    S.ev.multiply_relin(out, d[0], d[1], S.d_rlk)
    p01 = negacyclic_mod_t(m[0], m[1], T)
    assert np.array_equal(S.decrypt(out, 1)[0], p01)
    if cfg == "config4":
        # depth 2: (m0 m1) m2
        out2 = torch.empty_like(out)
        S.ev.multiply_relin(out2, out, d[2], S.d_rlk)
        assert np.array_equal(S.decrypt(out2, 1)[0], negacyclic_mod_t(p01, m[2], T))
        # (m0 + m1) m2 - m3
        s = torch.empty_like(out)
        S.ev.add(s, d[0], d[1])
        S.ev.multiply_relin(s, s, d[2], S.d_rlk)
        S.ev.sub(s, s, d[3])
        want = (negacyclic_mod_t((m[0] + m[1]) % T, m[2], T) + T - m[3]) % T
        assert np.array_equal(S.decrypt(s, 1)[0], want)
    S.close()


@pytest.mark.gpu
def test_batched_equals_looped(native, oracle, gpu):
    import torch
    n, (qs, psis) = 32768, config4()
    S = Scheme(native, oracle, n, qs, psis, model=False)
    R = S.R
    for count in (1, 7, 64):
        m = S.messages(2 * count)
        d_a, d_b = S.encrypt(m[:count]), S.encrypt(m[count:])
        out = torch.empty_like(d_a)
        S.ev.multiply_relin(out, d_a, d_b, S.d_rlk, count)
        ha, hb = native.to_host(d_a).reshape(2, count, R, n), native.to_host(d_b).reshape(2, count, R, n)
        scr = S.ev.scratch(1)
        loop = np.empty((2, count, R, n), dtype=np.uint64)
        for z in range(count):
            one = torch.empty(2 * R * n, dtype=torch.int64, device="cuda")
            S.ev.multiply_relin(one, native.to_device(np.ascontiguousarray(ha[:, z])), native.to_device(np.ascontiguousarray(hb[:, z])),
                                S.d_rlk, 1, scratch=scr)
            torch.cuda.synchronize()
            loop[:, z] = native.to_host(one).reshape(2, R, n)
        got = native.to_host(out).reshape(2, count, R, n)
        assert np.array_equal(got[:, :, : R - 1], loop[:, :, : R - 1]), count
        plain = S.decrypt(out, count)
        for z in range(count):
            assert np.array_equal(plain[z], negacyclic_mod_t(m[z], m[count + z], T)), (count, z)
    S.close()


@pytest.mark.gpu
def test_words_equal_to_q_read_as_zero(native, oracle, gpu):
    import torch
    n, (qs, psis) = 4096, demo_set(4096, 3)
    S = Scheme(native, oracle, n, qs, psis, model=False)
    R, r = S.R, S.r
    m = S.messages(2)
    a = native.to_host(S.encrypt(m[:1])).reshape(2, R, n)
    b = native.to_host(S.encrypt(m[1:])).reshape(2, R, n)
    idx = S.rng.choice(n, 64, replace=False)
    a0, aq = a.copy(), a.copy()
    for h in range(2):
        for i in range(r):
            a0[h, i, idx] = 0
            aq[h, i, idx] = qs[i]
    outs = []
    for x in (a0, aq):
        d_x, d_b = native.to_device(x), native.to_device(b)
        c3 = torch.zeros(3 * R * n, dtype=torch.int64, device="cuda")
        S.ev.multiply(c3, d_x, d_b)
        c = torch.zeros(2 * R * n, dtype=torch.int64, device="cuda")
        S.ev.multiply_relin(c, d_x, d_b, S.d_rlk)
        s = torch.zeros(2 * R * n, dtype=torch.int64, device="cuda")
        S.ev.add(s, d_x, d_b)
        d = torch.zeros(2 * R * n, dtype=torch.int64, device="cuda")
        S.ev.sub(d, d_b, d_x)
        torch.cuda.synchronize()
        outs.append([native.to_host(v) for v in (c3, c, s, d)])
    for u, v in zip(*outs):
        assert np.array_equal(u, v)
    # relinearize alone, on a product whose three components hold q_i in place of 0
    c3 = outs[0][0].reshape(3, R, n)
    z0, zq = c3.copy(), c3.copy()
    for h in range(3):
        for i in range(r):
            z0[h, i, idx] = 0
            zq[h, i, idx] = qs[i]
    rel = []
    for x in (z0, zq):
        c = torch.zeros(2 * R * n, dtype=torch.int64, device="cuda")
        S.ev.relinearize(c, native.to_device(x), S.d_rlk)
        torch.cuda.synchronize()
        rel.append(native.to_host(c))
    assert np.array_equal(rel[0], rel[1])
    S.close()


@pytest.mark.gpu
def test_complete_relin_keygen_decrypts(native, oracle, gpu):
    import torch
    n, (qs, psis) = 32768, config4()
    S = Scheme(native, oracle, n, qs, psis, model=False)
    rlk = torch.zeros_like(S.d_rlk)
    rnd = torch.empty(S.ev.relin_random_bytes, dtype=torch.uint8, device="cuda")
    temp = torch.empty(S.R * n, dtype=torch.int64, device="cuda")
    S.ev.relin_keygen_rns(rlk, S.d_sk, rnd, temp, nonce=12345)
    rlk2 = torch.zeros_like(S.d_rlk)
    S.ev.relin_keygen_rns(rlk2, S.d_sk, rnd, temp, nonce=12346)
    torch.cuda.synchronize()
    assert not torch.equal(rlk, rlk2)                    # the nonce matters
    # keygen_rns with the same nonce draws other samples: relinearization keys have a keystream key of their own
    sk3, pk3 = torch.empty(S.R * n, dtype=torch.int64, device="cuda"), torch.empty(2 * S.R * n, dtype=torch.int64, device="cuda")
    rnd_k = torch.empty(S.ctx.keygen_random_bytes, dtype=torch.uint8, device="cuda")
    S.ctx.keygen_rns(rnd_k, sk3, pk3, temp, nonce=12345)
    torch.cuda.synchronize()
    a0 = native.to_host(rlk).reshape(S.r, 2, S.R, n)[0, 1, : S.r]
    assert not np.array_equal(a0, native.to_host(pk3).reshape(2, S.R, n)[1, : S.r])
    m = S.messages(2)
    d_a, d_b = S.encrypt(m[:1]), S.encrypt(m[1:])
    for key in (rlk, rlk2):
        out = torch.empty_like(d_a)
        S.ev.multiply_relin(out, d_a, d_b, key)
        assert np.array_equal(S.decrypt(out, 1)[0], negacyclic_mod_t(m[0], m[1], T))
    S.close()


@pytest.mark.gpu
def test_inexact_bfv_object_multiplies_exactly(native, oracle, gpu):
    import torch
    from ntt_cuda_amd import bfv
    z = np.load(GOLD)
    n, qs, psis = int(z["n"]), [int(x) for x in z["q"]], [int(x) for x in z["psi"]]
    ctx = bfv.BFVContext(n, qs, psis, int(z["t"]), int(z["gamma"]))
    assert ctx.uses_literal_kernels
    ev = bfv.BFVEvaluator(ctx)
    R, r = len(qs), len(qs) - 1
    bs, ps = bfv.aux_primes(n, r)
    assert ev.aux_primes == bs
    M = EvalModel(oracle, n, qs[:r], psis[:r], bs, ps, int(z["t"]), native.barrett_is_exact)
    assert not all(native.barrett_is_exact(q) for q in qs[:r])
    rng = np.random.default_rng(77)
    a = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(2)])
    b = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(2)])
    d_c3 = torch.zeros(3 * R * n, dtype=torch.int64, device="cuda")
    ev.multiply(d_c3, native.to_device(a), native.to_device(b))
    torch.cuda.synchronize()
    assert np.array_equal(q_slots(native.to_host(d_c3), 3, 1, R, n), q_slots(M.multiply(a, b), 3, 1, R, n))
    ev.close()
    ctx.close()


@pytest.mark.gpu
def test_argument_errors_leave_outputs_untouched(native, oracle, gpu):
    import torch
    from ntt_cuda_amd import EINVAL, EUNSUPPORTED, lib, vp
    n, (qs, psis) = 4096, demo_set(4096, 3)
    S = Scheme(native, oracle, n, qs, psis, model=False)
    R, h = S.R, S.ev._h
    L = lib()
    m = S.messages(2)
    d_a, d_b = S.encrypt(m[:1]), S.encrypt(m[1:])
    out = sentinel(native, 3 * R * n)
    scr = S.ev.scratch(1)
    P_ = lambda t: vp(t.data_ptr())
    null = vp(0)
    st = vp(torch.cuda.current_stream().cuda_stream)
    calls = [
        (EINVAL, L.mi355ntt_bfv_multiply(None, P_(out), P_(d_a), P_(d_b), 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_multiply(h, null, P_(d_a), P_(d_b), 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_multiply(h, P_(out), null, P_(d_b), 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_multiply(h, P_(out), P_(d_a), P_(d_b), 1, null, st)),
        (EINVAL, L.mi355ntt_bfv_multiply(h, P_(out), P_(d_a), P_(d_b), 0, P_(scr), st)),
        (EUNSUPPORTED, L.mi355ntt_bfv_multiply(h, P_(out), P_(d_a), P_(d_b), 65536, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_relinearize(h, P_(out), P_(d_a), null, 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_relinearize(h, P_(out), P_(d_a), P_(S.d_rlk), 1, null, st)),
        (EINVAL, L.mi355ntt_bfv_multiply_relin(h, P_(out), P_(d_a), P_(d_b), P_(S.d_rlk), 0, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_multiply_relin(h, P_(out), P_(d_a), P_(d_b), P_(S.d_rlk), 1, null, st)),
        (EUNSUPPORTED, L.mi355ntt_bfv_multiply_relin(h, P_(out), P_(d_a), P_(d_b), P_(S.d_rlk), 70000, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_add(h, P_(out), null, P_(d_b), 1, st)),
        (EINVAL, L.mi355ntt_bfv_sub(h, P_(out), P_(d_a), P_(d_b), 0, st)),
        (EUNSUPPORTED, L.mi355ntt_bfv_add(h, P_(out), P_(d_a), P_(d_b), 65536, st)),
        (EINVAL, L.mi355ntt_bfv_relin_keygen(h, P_(out), null, P_(d_a), P_(d_b), st)),
        (EINVAL, L.mi355ntt_bfv_relin_keygen_rns(h, P_(out), P_(S.d_sk), null, P_(scr), 0, st)),
        (EINVAL, L.mi355ntt_bfv_eval_create(None, S.ctx._h)),
        (EINVAL, L.mi355ntt_bfv_eval_aux_primes(h, None)),
        (EINVAL, L.mi355ntt_bfv_aux_primes(4096, 3, None, None)),
        (EUNSUPPORTED, L.mi355ntt_bfv_aux_primes(4096, 16, (ctypes.c_ulonglong * 17)(), None)),
    ]
    for want, got in calls:
        assert got == want
    assert L.mi355ntt_bfv_eval_scratch_bytes(None, 1) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENT))
    # a parameter set outside the size condition: q_i wider than 61 bits
    from ntt_cuda_amd import bfv
    q62 = [q for q, _ in P.Q62_N4096][:3]
    w62 = [w for _, w in P.Q62_N4096][:3]
    c62 = bfv.BFVContext(4096, q62, w62, T, GAMMA)
    with pytest.raises(Exception, match=r"\[-2\]"):
        bfv.BFVEvaluator(c62)
    c62.close()
    S.close()


@pytest.mark.gpu
def test_two_streams_match_serial(native, oracle, gpu):
    import torch
    n, (qs, psis) = 32768, config4()
    S = Scheme(native, oracle, n, qs, psis, model=False)
    count = 8
    m = S.messages(4 * count)
    ins = [(S.encrypt(m[i * count:(i + 1) * count]), S.encrypt(m[(i + 2) * count:(i + 3) * count])) for i in range(2)]
    serial = []
    for a, b in ins:
        o = torch.empty_like(a)
        S.ev.multiply_relin(o, a, b, S.d_rlk, count)
        serial.append(o)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    scr = [S.ev.scratch(count), S.ev.scratch(count)]
    outs = [torch.empty_like(ins[0][0]), torch.empty_like(ins[0][0])]
    torch.cuda.synchronize()
    for _ in range(3):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                S.ev.multiply_relin(outs[i], ins[i][0], ins[i][1], S.d_rlk, count, scratch=scr[i], stream=streams[i])
    torch.cuda.synchronize()
    R = S.R
    for i in range(2):
        got = native.to_host(outs[i]).reshape(2, count, R, n)[:, :, : R - 1]
        want = native.to_host(serial[i]).reshape(2, count, R, n)[:, :, : R - 1]
        assert np.array_equal(got, want)
    S.close()


@pytest.mark.gpu
def test_per_call_scratch_follows_the_launch_stream(native, oracle, gpu):
    """stream= without scratch= and without entering the stream: the wrapper's scratch must not return to the current stream's pool
    while the call's kernels still run (allocations there, filled with garbage, would otherwise land in it)"""
    import torch
    n, (qs, psis) = 32768, config4()
    S = Scheme(native, oracle, n, qs, psis, model=False)
    count = 8
    m = S.messages(4 * count)
    ins = [(S.encrypt(m[i * count:(i + 1) * count]), S.encrypt(m[(i + 2) * count:(i + 3) * count])) for i in range(2)]
    serial = []
    for a, b in ins:
        o = torch.empty_like(a)
        S.ev.multiply_relin(o, a, b, S.d_rlk, count)
        serial.append(o)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.empty_like(ins[0][0]), torch.empty_like(ins[0][0])]
    words = S.ev.scratch_bytes(count) // 8
    for _ in range(3):
        for i in range(2):
            S.ev.multiply_relin(outs[i], ins[i][0], ins[i][1], S.d_rlk, count, stream=streams[i])
            junk = torch.full((words,), -1, dtype=torch.int64, device="cuda")      # current stream
            del junk
    torch.cuda.synchronize()
    R = S.R
    for i in range(2):
        got = native.to_host(outs[i]).reshape(2, count, R, n)[:, :, : R - 1]
        want = native.to_host(serial[i]).reshape(2, count, R, n)[:, :, : R - 1]
        assert np.array_equal(got, want)
    S.close()
