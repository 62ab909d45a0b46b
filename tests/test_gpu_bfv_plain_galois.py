"""GPU: the BFV evaluator's plaintext operations and Galois automorphisms (include/mi355ntt.h, "BFV evaluation with plaintext operands
and Galois automorphisms") -- every output word against the CPU model (tests/bfv_galois_model.py), add_plain against encryption
itself, round trips through the drivers, the complete galois key generation, a Barrett-inexact BFV object, argument errors, two
streams and a captured graph."""
import ctypes

import numpy as np
import pytest

from bfv_eval_model import negacyclic_mod_t
from bfv_galois_model import GaloisModel, automorphism
from test_gpu_bfv_eval import GOLD, SENT, T, Scheme, config4, demo16, demo_set, q_slots, sentinel, special_untouched


def scheme(native, oracle, cfg, model=True, seed=7):
    if cfg == "demo4096":
        n, (qs, psis) = 4096, demo_set(4096, 3)
    elif cfg == "config4":
        n, (qs, psis) = 32768, config4()
    else:
        n, (qs, psis) = 32768, demo16()
    S = Scheme(native, oracle, n, qs, psis, seed=seed, model=False)
    if model:
        S.model = GaloisModel(oracle, n, qs[:-1], psis[:-1], S.ev.aux_primes, S._aux_psis(), T, native.barrett_is_exact)
    return S


def galois_key(S, g):
    import torch
    gk = torch.zeros(S.r * 2 * S.R * S.n, dtype=torch.int64, device="cuda")
    S.ev.galois_keygen(gk, S.d_sk, g, S.native.to_device(S.a), S.native.to_device(S.e))
    return gk


def with_q_words(S, x, comps, count):
    """x [comps][count][R][n] host words with a few words of every Q slot replaced by q_i (which reads as 0)"""
    x = x.reshape(comps, count, S.R, S.n).copy()
    idx = S.rng.choice(S.n, 16, replace=False)
    for i in range(S.r):
        x[:, :, i, idx] = S.qs[i]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["demo4096", "config4"])
def test_every_word_matches_the_model(native, oracle, gpu, cfg):
    import torch
    S = scheme(native, oracle, cfg)
    M, R, r, n = S.model, S.R, S.r, S.n
    count = 2
    m = S.messages(2 * count)
    a = with_q_words(S, native.to_host(S.encrypt(m[:count])), 2, count)
    d_a = native.to_device(a)
    pm = m[count:].copy()
    pm[0, :5] = [0, T - 1, T // 2, T // 2 - 1, T + 3]           # the centred lift's edges; a word >= t is taken mod t
    d_m = native.to_device(pm)
    mhat = np.stack([M.plain_ntt(pm[z]) for z in range(count)])

    def check(d_out, want):
        torch.cuda.synchronize()
        assert np.array_equal(q_slots(native.to_host(d_out), 2, count, R, n), q_slots(want, 2, count, R, n))
        assert special_untouched(native, d_out, 2, count, R, n)

    for sub in (False, True):
        d_c = sentinel(native, 2 * count * R * n)
        (S.ev.sub_plain if sub else S.ev.add_plain)(d_c, d_a, d_m, count)
        check(d_c, np.stack([M.add_plain(a[:, z], pm[z], sub=sub) for z in range(count)], axis=1))
    d_mhat = torch.zeros(count * r * n, dtype=torch.int64, device="cuda")
    S.ev.plain_ntt(d_mhat, d_m, count)
    torch.cuda.synchronize()
    assert np.array_equal(native.to_host(d_mhat).reshape(count, r, n), mhat)
    want = np.stack([M.multiply_plain_ntt(a[:, z], mhat[z]) for z in range(count)], axis=1)
    d_c = sentinel(native, 2 * count * R * n)
    S.ev.multiply_plain(d_c, d_a, d_m, count)
    check(d_c, want)
    d_c = sentinel(native, 2 * count * R * n)
    S.ev.multiply_plain_ntt(d_c, d_a, d_mhat, count, shared=False)
    check(d_c, want)
    d_c = sentinel(native, 2 * count * R * n)
    S.ev.multiply_plain_ntt(d_c, d_a, d_mhat[: r * n], count, shared=True)
    check(d_c, np.stack([M.multiply_plain_ntt(a[:, z], mhat[0]) for z in range(count)], axis=1))
    for g in (3, n + 1, 2 * n - 1):
        gk = galois_key(S, g)
        want_gk = M.galois_keygen(S.sk_hat, g, S.a, S.e)
        torch.cuda.synchronize()
        assert np.array_equal(native.to_host(gk).reshape(r, 2, R, n)[:, :, :r], want_gk[:, :, :r]), g
        d_c = sentinel(native, 2 * count * R * n)
        S.ev.apply_galois(d_c, d_a, gk, g, count)
        check(d_c, np.stack([M.apply_galois(a[:, z], want_gk, g) for z in range(count)], axis=1))
    S.close()


@pytest.mark.gpu
def test_add_plain_is_encryptions_encoding(native, oracle, gpu):
    """add_plain(encrypt(u, e, 0), m) == encrypt(u, e, m) and sub_plain(encrypt(u, e, m), m) == encrypt(u, e, 0), word for word"""
    import torch
    S = scheme(native, oracle, "config4", model=False)
    R, n, count = S.R, S.n, 3
    u = np.stack([oracle.bfv_sample(S.qs, n, 90 + z)["ternary"] for z in range(count)])
    e = np.stack([np.stack([S.smp["err"]() for _ in range(count)]) for _ in range(2)])
    d_e = native.to_device(np.ascontiguousarray(e))
    m = S.messages(count)
    m[0, :4] = [0, T - 1, T // 2, T // 2 - 1]
    enc = {}
    for key, msg in (("0", np.zeros_like(m)), ("m", m)):
        d_c = native.to_device(np.ascontiguousarray(np.stack([u, u])))
        S.ctx.encrypt_batch(d_c, S.d_pk, d_e, native.to_device(msg), count)
        enc[key] = d_c
    d_m = native.to_device(m)
    added = torch.empty_like(enc["0"])
    S.ev.add_plain(added, enc["0"], d_m, count)
    back = enc["m"].clone()
    S.ev.sub_plain(back, back, d_m, count)                       # in place
    torch.cuda.synchronize()
    q = lambda d: q_slots(native.to_host(d), 2, count, R, n)
    assert np.array_equal(q(added), q(enc["m"]))
    assert np.array_equal(q(back), q(enc["0"]))
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["demo4096", "config4"])
def test_round_trips_through_the_drivers(native, oracle, gpu, cfg):
    import torch
    S = scheme(native, oracle, cfg, model=False)
    n, count = S.n, 2
    m = S.messages(2 * count)
    d_a = S.encrypt(m[:count])
    keys = {}
    for g in (3, 5, n // 2 + 1, n + 1, 2 * n - 1):
        keys[g] = galois_key(S, g)
        out = torch.empty_like(d_a)
        S.ev.apply_galois(out, d_a, keys[g], g, count)
        plain = S.decrypt(out, count)
        for z in range(count):
            assert np.array_equal(plain[z], automorphism(m[z], g, T)), (g, z)
    # a composition: tau_5 tau_3 = tau_15
    out = torch.empty_like(d_a)
    S.ev.apply_galois(out, d_a, keys[3], 3, count)
    S.ev.apply_galois(out, out, keys[5], 5, count)               # in place
    plain = S.decrypt(out, count)
    for z in range(count):
        assert np.array_equal(plain[z], automorphism(m[z], 15, T))
    out = torch.empty_like(d_a)
    S.ev.multiply_plain(out, d_a, native.to_device(m[count:]), count)
    plain = S.decrypt(out, count)
    for z in range(count):
        assert np.array_equal(plain[z], negacyclic_mod_t(m[z], m[count + z], T))
    S.close()


@pytest.mark.gpu
def test_chain_on_config4(native, oracle, gpu):
    """multiply_relin -> apply_galois -> multiply_plain_ntt (shared) -> add_plain.  Four 60-bit primes: Q / (2t) is about 2^229, and the
    DESIGN.md bounds after the chain stay near 2^110.  Two 55-bit primes would leave Q / (2t) near 2^99, below the chain's bound."""
    import torch
    S = scheme(native, oracle, "config4", model=False)
    n, r, count = S.n, S.r, 2
    m = S.messages(2 * count + 2)
    d_a, d_b = S.encrypt(m[:count]), S.encrypt(m[count:2 * count])
    g = 5
    gk = galois_key(S, g)
    x = torch.empty_like(d_a)
    S.ev.multiply_relin(x, d_a, d_b, S.d_rlk, count)
    S.ev.apply_galois(x, x, gk, g, count)
    d_mhat = torch.empty(r * n, dtype=torch.int64, device="cuda")
    S.ev.plain_ntt(d_mhat, native.to_device(m[-2:-1]), 1)
    S.ev.multiply_plain_ntt(x, x, d_mhat, count, shared=True)
    S.ev.add_plain(x, x, native.to_device(np.stack([m[-1]] * count)), count)
    plain = S.decrypt(x, count)
    for z in range(count):
        want = automorphism(negacyclic_mod_t(m[z], m[count + z], T), g, T)
        want = (negacyclic_mod_t(want, m[-2], T) + m[-1]) % T
        assert np.array_equal(plain[z], want), z
    S.close()


@pytest.mark.gpu
def test_demo16_round_trip(native, oracle, gpu):
    import torch
    S = scheme(native, oracle, "demo16", model=False)
    n = S.n
    m = S.messages(2)
    d_a = S.encrypt(m[:1])
    g = 2 * n - 1
    gk = galois_key(S, g)
    out = torch.empty_like(d_a)
    S.ev.apply_galois(out, d_a, gk, g)
    assert np.array_equal(S.decrypt(out, 1)[0], automorphism(m[0], g, T))
    del gk
    S.ev.multiply_plain(out, d_a, native.to_device(m[1:]))
    assert np.array_equal(S.decrypt(out, 1)[0], negacyclic_mod_t(m[0], m[1], T))
    S.close()


@pytest.mark.gpu
def test_complete_galois_keygen(native, oracle, gpu):
    import torch
    S = scheme(native, oracle, "config4", model=False)
    R, r, n = S.R, S.r, S.n
    gs = [3, 2 * n - 1]
    gk = torch.zeros(len(gs) * r * 2 * R * n, dtype=torch.int64, device="cuda")
    rnd = torch.empty(S.ev.galois_random_bytes(len(gs)), dtype=torch.uint8, device="cuda")
    temp = torch.empty(R * n, dtype=torch.int64, device="cuda")
    S.ev.galois_keygen_rns(gk, S.d_sk, gs, rnd, temp, nonce=4242)
    rlk = torch.zeros(r * 2 * R * n, dtype=torch.int64, device="cuda")
    rnd_r = torch.empty(S.ev.relin_random_bytes, dtype=torch.uint8, device="cuda")
    S.ev.relin_keygen_rns(rlk, S.d_sk, rnd_r, temp, nonce=4242)
    torch.cuda.synchronize()
    h = native.to_host(gk).reshape(len(gs), r, 2, R, n)
    a_halves = [h[k, :, 1, :r] for k in range(len(gs))]
    assert not np.array_equal(a_halves[0], a_halves[1])
    rl = native.to_host(rlk).reshape(r, 2, R, n)[:, 1, :r]
    assert not np.array_equal(a_halves[0], rl) and not np.array_equal(a_halves[1], rl)
    m = S.messages(1)
    d_a = S.encrypt(m)
    for k, g in enumerate(gs):
        out = torch.empty_like(d_a)
        S.ev.apply_galois(out, d_a, gk[k * r * 2 * R * n: (k + 1) * r * 2 * R * n], g)
        assert np.array_equal(S.decrypt(out, 1)[0], automorphism(m[0], g, T)), g
    S.close()


@pytest.mark.gpu
def test_inexact_bfv_object_gives_exact_words(native, oracle, gpu):
    import torch
    from ntt_cuda_amd import bfv
    z = np.load(GOLD)
    n, qs, psis, t = int(z["n"]), [int(x) for x in z["q"]], [int(x) for x in z["psi"]], int(z["t"])
    ctx = bfv.BFVContext(n, qs, psis, t, int(z["gamma"]))
    assert ctx.uses_literal_kernels
    ev = bfv.BFVEvaluator(ctx)
    R, r = len(qs), len(qs) - 1
    bs, ps = bfv.aux_primes(n, r)
    assert ev.aux_primes == bs
    M = GaloisModel(oracle, n, qs[:r], psis[:r], bs, ps, t, native.barrett_is_exact)
    assert not all(native.barrett_is_exact(q) for q in qs[:r])
    rng = np.random.default_rng(78)
    a = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(2)])
    m = rng.integers(0, t, size=(1, n), dtype=np.uint64)
    d_c = torch.zeros(2 * R * n, dtype=torch.int64, device="cuda")
    ev.multiply_plain(d_c, native.to_device(a), native.to_device(m))
    torch.cuda.synchronize()
    assert np.array_equal(q_slots(native.to_host(d_c), 2, 1, R, n), q_slots(M.multiply_plain(a, m[0]), 2, 1, R, n))
    # galois key and automorphism from explicit samples
    sk_hat = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs])
    ka = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(r)])
    ke = np.stack([np.stack([rng.integers(0, 8, size=n, dtype=np.uint64) for _ in qs]) for _ in range(r)])
    g = 3
    gk = torch.zeros(r * 2 * R * n, dtype=torch.int64, device="cuda")
    ev.galois_keygen(gk, native.to_device(sk_hat), g, native.to_device(ka), native.to_device(ke))
    ev.apply_galois(d_c, native.to_device(a), gk, g)
    torch.cuda.synchronize()
    want_gk = M.galois_keygen(sk_hat, g, ka, ke)
    assert np.array_equal(native.to_host(gk).reshape(r, 2, R, n)[:, :, :r], want_gk[:, :, :r])
    assert np.array_equal(q_slots(native.to_host(d_c), 2, 1, R, n), q_slots(M.apply_galois(a, want_gk, g), 2, 1, R, n))
    ev.close()
    ctx.close()


@pytest.mark.gpu
def test_argument_errors_leave_outputs_untouched(native, oracle, gpu):
    import torch
    from ntt_cuda_amd import EINVAL, EUNSUPPORTED, lib, vp
    S = scheme(native, oracle, "demo4096", model=False)
    R, r, n, h = S.R, S.r, S.n, S.ev._h
    L = lib()
    m = S.messages(1)
    d_a = S.encrypt(m)
    d_m = native.to_device(m)
    out = sentinel(native, 2 * R * n)
    gk = sentinel(native, 2 * r * R * n)
    scr = S.ev.scratch(1)
    P_ = lambda t: vp(t.data_ptr())
    null = vp(0)
    st = vp(torch.cuda.current_stream().cuda_stream)
    rnd = torch.empty(S.ev.galois_random_bytes(2), dtype=torch.uint8, device="cuda")
    gl = lambda *g: (ctypes.c_uint * len(g))(*g)
    calls = [
        (EINVAL, L.mi355ntt_bfv_add_plain(None, P_(out), P_(d_a), P_(d_m), 1, st)),
        (EINVAL, L.mi355ntt_bfv_add_plain(h, P_(out), P_(d_a), null, 1, st)),
        (EINVAL, L.mi355ntt_bfv_sub_plain(h, P_(out), P_(d_a), P_(d_m), 0, st)),
        (EUNSUPPORTED, L.mi355ntt_bfv_sub_plain(h, P_(out), P_(d_a), P_(d_m), 65536, st)),
        (EINVAL, L.mi355ntt_bfv_plain_ntt(h, null, P_(d_m), 1, st)),
        (EUNSUPPORTED, L.mi355ntt_bfv_plain_ntt(h, P_(out), P_(d_m), 65536, st)),
        (EINVAL, L.mi355ntt_bfv_multiply_plain(h, P_(out), P_(d_a), P_(d_m), 1, null, st)),
        (EINVAL, L.mi355ntt_bfv_multiply_plain(h, P_(out), null, P_(d_m), 1, P_(scr), st)),
        (EUNSUPPORTED, L.mi355ntt_bfv_multiply_plain(h, P_(out), P_(d_a), P_(d_m), 70000, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_multiply_plain_ntt(h, P_(out), P_(d_a), P_(d_m), 1, 2, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_multiply_plain_ntt(h, P_(out), P_(d_a), P_(d_m), 1, -1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_multiply_plain_ntt(h, P_(out), P_(d_a), P_(d_m), 0, 0, P_(scr), st)),
        (EUNSUPPORTED, L.mi355ntt_bfv_multiply_plain_ntt(h, P_(out), P_(d_a), P_(d_m), 65536, 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_multiply_plain_ntt(h, P_(out), P_(d_a), null, 1, 0, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen(h, P_(gk), P_(S.d_sk), 4, P_(d_a), P_(d_a), st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen(h, P_(gk), P_(S.d_sk), 0, P_(d_a), P_(d_a), st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen(h, P_(gk), P_(S.d_sk), 2 * n + 1, P_(d_a), P_(d_a), st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen(h, P_(gk), null, 3, P_(d_a), P_(d_a), st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen_rns(h, P_(gk), P_(S.d_sk), gl(3, 6), 2, P_(rnd), P_(scr), 0, st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen_rns(h, P_(gk), P_(S.d_sk), gl(2 * n), 1, P_(rnd), P_(scr), 0, st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen_rns(h, P_(gk), P_(S.d_sk), gl(3), 0, P_(rnd), P_(scr), 0, st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen_rns(h, P_(gk), P_(S.d_sk), None, 1, P_(rnd), P_(scr), 0, st)),
        (EINVAL, L.mi355ntt_bfv_galois_keygen_rns(h, P_(gk), P_(S.d_sk), gl(3), 1, null, P_(scr), 0, st)),
        (EINVAL, L.mi355ntt_bfv_apply_galois(h, P_(out), P_(d_a), P_(gk), 2, 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_apply_galois(h, P_(out), P_(d_a), P_(gk), 0, 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_apply_galois(h, P_(out), P_(d_a), P_(gk), 2 * n + 3, 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_apply_galois(h, P_(out), P_(d_a), null, 3, 1, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_apply_galois(h, P_(out), P_(d_a), P_(gk), 3, 1, null, st)),
        (EINVAL, L.mi355ntt_bfv_apply_galois(h, P_(out), P_(d_a), P_(gk), 3, 0, P_(scr), st)),
        (EUNSUPPORTED, L.mi355ntt_bfv_apply_galois(h, P_(out), P_(d_a), P_(gk), 3, 65536, P_(scr), st)),
        (EINVAL, L.mi355ntt_bfv_apply_galois(None, P_(out), P_(d_a), P_(gk), 3, 1, P_(scr), st)),
    ]
    for k, (want, got) in enumerate(calls):
        assert got == want, k
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENT)) and bool(torch.all(gk == SENT))
    S.close()


@pytest.mark.gpu
def test_two_streams_and_a_captured_graph(native, oracle, gpu):
    import torch
    S = scheme(native, oracle, "config4", model=False)
    R, n, count, g = S.R, S.n, 4, 5
    gk = galois_key(S, g)
    m = S.messages(2 * count)
    ins = [S.encrypt(m[:count]), S.encrypt(m[count:])]
    serial = []
    for a in ins:
        o = torch.empty_like(a)
        S.ev.apply_galois(o, a, gk, g, count)
        serial.append(o)
    torch.cuda.synchronize()
    q = lambda d: q_slots(native.to_host(d), 2, count, R, n)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    scr = [S.ev.scratch(count), S.ev.scratch(count)]
    outs = [torch.empty_like(ins[0]), torch.empty_like(ins[0])]
    torch.cuda.synchronize()
    for _ in range(3):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                S.ev.apply_galois(outs[i], ins[i], gk, g, count, scratch=scr[i], stream=streams[i])
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(q(outs[i]), q(serial[i]))
    # one capture on a single stream (a linear graph, no forked streams), replayed twice
    cap = torch.zeros_like(ins[0])
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        S.ev.apply_galois(cap, ins[0], gk, g, count, scratch=scr[0], stream=s)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(q(cap), q(serial[0]))
    cap.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(q(cap), q(serial[0]))
    del graph
    S.close()
