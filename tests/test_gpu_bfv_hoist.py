"""GPU: hoisted Galois automorphisms of the BFV evaluator (include/mi355ntt.h, "Hoisted Galois automorphisms") -- every Q-slot word of
apply_galois_hoisted and galois_sum against the CPU model (tests/bfv_hoist_model.py), more elements than one scratch group / one
inner-product launch holds, repeated elements, in-place sums, round trips through the drivers against the existing calls, the complete
key generation, the 16-prime demo set, a Barrett-inexact BFV object, argument errors, two streams and captured graphs."""
import ctypes

import numpy as np
import pytest

from bfv_eval_model import negacyclic_mod_t
from bfv_galois_model import automorphism
from bfv_hoist_model import HoistModel
from test_gpu_bfv_eval import GOLD, SENT, T, q_slots, sentinel, special_untouched
from test_gpu_bfv_plain_galois import galois_key, scheme, with_q_words


def hoist_scheme(native, oracle, cfg, model=True, seed=7):
    S = scheme(native, oracle, cfg, model=False, seed=seed)
    if model:
        S.model = HoistModel(oracle, S.n, S.qs[:-1], S.psis[:-1], S.ev.aux_primes, S._aux_psis(), T, native.barrett_is_exact)
    return S


def keys_for(S, gs, model=True):
    """device keys [G][r][2][R][n] from explicit samples (one key per distinct element, repeated where gs repeats) and the model's"""
    import torch
    dev, host = {}, {}
    for g in gs:
        if g not in dev:
            dev[g] = galois_key(S, g)
            if model:
                host[g] = S.model.galois_keygen(S.sk_hat, g, S.a, S.e)
    return torch.cat([dev[g] for g in gs]), [host[g] for g in gs] if model else None


def plain_weights(S, ms):
    import torch
    G = ms.shape[0]
    w = torch.zeros(G * S.r * S.n, dtype=torch.int64, device="cuda")
    S.ev.plain_ntt(w, S.native.to_device(ms), G)
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["demo4096", "config4"])
def test_every_word_matches_the_model(native, oracle, gpu, cfg):
    import torch
    S = hoist_scheme(native, oracle, cfg)
    M, R, r, n = S.model, S.R, S.r, S.n
    count = 2
    m = S.messages(count)
    a = with_q_words(S, native.to_host(S.encrypt(m)), 2, count)
    d_a = native.to_device(a)
    group = S.ev.hoist_group
    assert group == min(8, (max(8 * r + 4, r * r + 2 * r) + 3 * R - r * r) // (2 * r)) >= 1
    hoists = [M.hoist(a[:, z]) for z in range(count)]
    base = [3, n + 1, 2 * n - 1, 5, 3, 25, 2 * n - 3, 1]
    cases = [base[:1], [3, 3], (base * 2)[: group + 1]]              # G = 1, a repeated element, more than one scratch group
    if cfg == "demo4096":
        cases.append((base * 3)[:17])                                # more than one inner-product launch of galois_sum
    for gs in cases:
        G = len(gs)
        d_gk, gks = keys_for(S, gs)
        d_out = sentinel(native, G * 2 * count * R * n)
        S.ev.apply_galois_hoisted(d_out, d_a, d_gk, gs, count)
        torch.cuda.synchronize()
        got = native.to_host(d_out).reshape(G, 2, count, R, n)
        for k, g in enumerate(gs):
            want = np.stack([M.hoisted(a[:, z], gks[k], g, hoists[z]) for z in range(count)], axis=1)
            assert np.array_equal(got[k][:, :, :r], want[:, :, :r]), (gs, k)
        assert np.all(got[:, :, :, R - 1] == np.uint64(SENT))
        ms = S.messages(G)
        ms[0, :5] = [0, T - 1, T // 2, T // 2 - 1, T + 3]
        d_w = plain_weights(S, ms)
        weights = [M.plain_ntt(ms[k]) for k in range(G)]
        torch.cuda.synchronize()
        assert np.array_equal(native.to_host(d_w).reshape(G, r, n), np.stack(weights))
        for d_wt, wt in ((None, None), (d_w, weights)):
            d_c = sentinel(native, 2 * count * R * n)
            S.ev.galois_sum(d_c, d_a, d_gk, gs, count, weights=d_wt)
            torch.cuda.synchronize()
            want = np.stack([M.galois_sum(a[:, z], gks, gs, wt) for z in range(count)], axis=1)
            assert np.array_equal(q_slots(native.to_host(d_c), 2, count, R, n), q_slots(want, 2, count, R, n)), (gs, wt is None)
            assert special_untouched(native, d_c, 2, count, R, n)
            # in place: c aliasing a
            d_b = d_a.clone()
            S.ev.galois_sum(d_b, d_b, d_gk, gs, count, weights=d_wt)
            torch.cuda.synchronize()
            assert np.array_equal(q_slots(native.to_host(d_b), 2, count, R, n), q_slots(want, 2, count, R, n)), (gs, wt is None)
            assert np.array_equal(native.to_host(d_b).reshape(2, count, R, n)[:, :, R - 1], a[:, :, R - 1])
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["demo4096", "config4"])
def test_round_trips_against_the_existing_calls(native, oracle, gpu, cfg):
    """hoisted outputs decrypt to the plaintexts of G separate apply_galois calls; the weighted sum to the plaintext of the chain
    apply_galois -> multiply_plain_ntt (shared) -> add; odd counts (the inner products take two ciphertexts per thread)"""
    import torch
    S = hoist_scheme(native, oracle, cfg, model=False)
    R, r, n = S.R, S.r, S.n
    gs = [3, 5, n // 2 + 1, n + 1, 2 * n - 1, 5]
    G = len(gs)
    d_gk, _ = keys_for(S, gs, model=False)
    ksz = r * 2 * R * n
    for count in (1, 3):
        m = S.messages(count)
        d_a = S.encrypt(m)
        d_out = torch.empty(G * 2 * count * R * n, dtype=torch.int64, device="cuda")
        S.ev.apply_galois_hoisted(d_out, d_a, d_gk, gs, count)
        ms = S.messages(G)
        d_w = plain_weights(S, ms)
        chain, plain_sum = None, None
        for k, g in enumerate(gs):
            one = torch.empty_like(d_a)
            S.ev.apply_galois(one, d_a, d_gk[k * ksz: (k + 1) * ksz], g, count)
            sep = S.decrypt(one, count)
            hoisted = S.decrypt(d_out[k * 2 * count * R * n: (k + 1) * 2 * count * R * n], count)
            for z in range(count):
                assert np.array_equal(sep[z], automorphism(m[z], g, T)), (g, z)
                assert np.array_equal(hoisted[z], sep[z]), (g, z)
            if plain_sum is None:
                plain_sum = one.clone()
            else:
                S.ev.add(plain_sum, plain_sum, one, count)
            S.ev.multiply_plain_ntt(one, one, d_w[k * r * n: (k + 1) * r * n], count, shared=True)
            if chain is None:
                chain = one
            else:
                S.ev.add(chain, chain, one, count)
        for d_wt, ref in ((None, plain_sum), (d_w, chain)):
            d_c = torch.empty_like(d_a)
            S.ev.galois_sum(d_c, d_a, d_gk, gs, count, weights=d_wt)
            got, want = S.decrypt(d_c, count), S.decrypt(ref, count)
            for z in range(count):
                exp = np.zeros(n, dtype=np.uint64)
                for k, g in enumerate(gs):
                    tg = automorphism(m[z], g, T)
                    exp = (exp + (tg if d_wt is None else negacyclic_mod_t(ms[k], tg, T))) % T
                assert np.array_equal(want[z], exp), (d_wt is None, z)
                assert np.array_equal(got[z], want[z]), (d_wt is None, z)
    S.close()


@pytest.mark.gpu
def test_complete_keygen_and_the_demo16_set(native, oracle, gpu):
    """keys from galois_keygen_rns; r = 15 (scratch groups of 2)"""
    import torch
    for cfg, gs in (("config4", None), ("demo16", None)):
        S = hoist_scheme(native, oracle, cfg, model=False)
        R, r, n = S.R, S.r, S.n
        gs = [3, 2 * n - 1, n + 1]
        G = len(gs)
        assert cfg != "demo16" or (r == 15 and S.ev.hoist_group == 2)
        gk = torch.zeros(G * r * 2 * R * n, dtype=torch.int64, device="cuda")
        rnd = torch.empty(S.ev.galois_random_bytes(G), dtype=torch.uint8, device="cuda")
        temp = torch.empty(R * n, dtype=torch.int64, device="cuda")
        S.ev.galois_keygen_rns(gk, S.d_sk, gs, rnd, temp, nonce=9090)
        m = S.messages(1)
        d_a = S.encrypt(m)
        d_out = torch.empty(G * 2 * R * n, dtype=torch.int64, device="cuda")
        S.ev.apply_galois_hoisted(d_out, d_a, gk, gs)
        for k, g in enumerate(gs):
            assert np.array_equal(S.decrypt(d_out[k * 2 * R * n: (k + 1) * 2 * R * n], 1)[0], automorphism(m[0], g, T)), (cfg, g)
        ms = S.messages(G)
        d_w = plain_weights(S, ms)
        for d_wt in (None, d_w):
            d_c = torch.empty_like(d_a)
            S.ev.galois_sum(d_c, d_a, gk, gs, weights=d_wt)
            exp = np.zeros(n, dtype=np.uint64)
            for k, g in enumerate(gs):
                tg = automorphism(m[0], g, T)
                exp = (exp + (tg if d_wt is None else negacyclic_mod_t(ms[k], tg, T))) % T
            assert np.array_equal(S.decrypt(d_c, 1)[0], exp), (cfg, d_wt is None)
        del gk, d_out, d_w
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
    M = HoistModel(oracle, n, qs[:r], psis[:r], bs, ps, t, native.barrett_is_exact)
    assert not all(native.barrett_is_exact(q) for q in qs[:r])
    rng = np.random.default_rng(79)
    a = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(2)])
    sk_hat = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs])
    ka = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(r)])
    ke = np.stack([np.stack([rng.integers(0, 8, size=n, dtype=np.uint64) for _ in qs]) for _ in range(r)])
    gs = [3, 2 * n - 1]
    G = len(gs)
    gk = torch.zeros(G * r * 2 * R * n, dtype=torch.int64, device="cuda")
    for k, g in enumerate(gs):
        ev.galois_keygen(gk[k * r * 2 * R * n: (k + 1) * r * 2 * R * n], native.to_device(sk_hat), g, native.to_device(ka), native.to_device(ke))
    gks = [M.galois_keygen(sk_hat, g, ka, ke) for g in gs]
    ms = rng.integers(0, t, size=(G, n), dtype=np.uint64)
    d_w = torch.zeros(G * r * n, dtype=torch.int64, device="cuda")
    ev.plain_ntt(d_w, native.to_device(ms), G)
    d_a = native.to_device(a)
    d_out = sentinel(native, G * 2 * R * n)
    ev.apply_galois_hoisted(d_out, d_a, gk, gs)
    d_c = sentinel(native, 2 * R * n)
    ev.galois_sum(d_c, d_a, gk, gs, weights=d_w)
    torch.cuda.synchronize()
    got = native.to_host(d_out).reshape(G, 2, R, n)
    for k, g in enumerate(gs):
        assert np.array_equal(got[k][:, :r], M.hoisted(a, gks[k], g)[:, :r]), g
    want = M.galois_sum(a, gks, gs, [M.plain_ntt(ms[k]) for k in range(G)])
    assert np.array_equal(q_slots(native.to_host(d_c), 2, 1, R, n), q_slots(want, 2, 1, R, n))
    ev.close()
    ctx.close()


@pytest.mark.gpu
def test_argument_errors_leave_outputs_untouched(native, oracle, gpu):
    import torch
    from ntt_cuda_amd import EINVAL, lib, vp
    S = hoist_scheme(native, oracle, "demo4096", model=False)
    R, r, n, h = S.R, S.r, S.n, S.ev._h
    L = lib()
    d_a = S.encrypt(S.messages(1))
    out = sentinel(native, 2 * 2 * R * n)
    gk = sentinel(native, 2 * 2 * r * R * n)
    w = sentinel(native, 2 * r * n)
    scr = S.ev.scratch(1)
    P_ = lambda t: vp(t.data_ptr())
    null = vp(0)
    st = vp(torch.cuda.current_stream().cuda_stream)
    gl = lambda *g: (ctypes.c_uint * len(g))(*g)
    H, Sm = L.mi355ntt_bfv_apply_galois_hoisted, L.mi355ntt_bfv_galois_sum
    calls = [
        H(h, P_(out), P_(d_a), P_(gk), gl(3, 6), 2, 1, P_(scr), st),                  # even g
        H(h, P_(out), P_(d_a), P_(gk), gl(2 * n + 1, 3), 2, 1, P_(scr), st),          # g >= 2n
        H(h, P_(out), P_(d_a), P_(gk), gl(3, 0), 2, 1, P_(scr), st),
        H(h, P_(out), P_(d_a), P_(gk), gl(3), 0, 1, P_(scr), st),                     # G = 0
        H(h, P_(out), P_(d_a), P_(gk), None, 1, 1, P_(scr), st),
        H(None, P_(out), P_(d_a), P_(gk), gl(3), 1, 1, P_(scr), st),
        H(h, null, P_(d_a), P_(gk), gl(3), 1, 1, P_(scr), st),
        H(h, P_(out), null, P_(gk), gl(3), 1, 1, P_(scr), st),
        H(h, P_(out), P_(d_a), null, gl(3), 1, 1, P_(scr), st),
        H(h, P_(out), P_(d_a), P_(gk), gl(3), 1, 1, null, st),
        H(h, P_(out), P_(d_a), P_(gk), gl(3), 1, 0, P_(scr), st),                     # count = 0
        H(h, P_(out), P_(d_a), P_(gk), gl(3), 1, 65536, P_(scr), st),
        Sm(h, P_(out), P_(d_a), P_(gk), gl(3, 2 * n), 2, P_(w), 1, P_(scr), st),
        Sm(h, P_(out), P_(d_a), P_(gk), gl(2 * n + 5), 1, null, 1, P_(scr), st),
        Sm(h, P_(out), P_(d_a), P_(gk), gl(3), 0, P_(w), 1, P_(scr), st),
        Sm(h, P_(out), P_(d_a), P_(gk), None, 1, P_(w), 1, P_(scr), st),
        Sm(None, P_(out), P_(d_a), P_(gk), gl(3), 1, P_(w), 1, P_(scr), st),
        Sm(h, null, P_(d_a), P_(gk), gl(3), 1, P_(w), 1, P_(scr), st),
        Sm(h, P_(out), null, P_(gk), gl(3), 1, P_(w), 1, P_(scr), st),
        Sm(h, P_(out), P_(d_a), null, gl(3), 1, P_(w), 1, P_(scr), st),
        Sm(h, P_(out), P_(d_a), P_(gk), gl(3), 1, P_(w), 1, null, st),
        Sm(h, P_(out), P_(d_a), P_(gk), gl(3), 1, P_(w), 0, P_(scr), st),
        Sm(h, P_(out), P_(d_a), P_(gk), gl(3), 1, null, 65536, P_(scr), st),
    ]
    for k, got in enumerate(calls):
        assert got == EINVAL, k
    assert L.mi355ntt_bfv_hoist_group(None) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENT)) and bool(torch.all(gk == SENT)) and bool(torch.all(w == SENT))
    S.close()


@pytest.mark.gpu
def test_two_streams_and_captured_graphs(native, oracle, gpu):
    import torch
    S = hoist_scheme(native, oracle, "config4", model=False)
    R, r, n, count = S.R, S.r, S.n, 4
    gs = [5, 2 * n - 1, 3, n + 1, 5]                             # one more than a scratch group at r = 4
    G = len(gs)
    d_gk, _ = keys_for(S, gs, model=False)
    m = S.messages(2 * count)
    ins = [S.encrypt(m[:count]), S.encrypt(m[count:])]
    d_w = plain_weights(S, S.messages(G))
    new_h = lambda: torch.zeros(G * 2 * count * R * n, dtype=torch.int64, device="cuda")
    serial = []
    for a in ins:
        o, c = new_h(), torch.zeros_like(a)
        S.ev.apply_galois_hoisted(o, a, d_gk, gs, count)
        S.ev.galois_sum(c, a, d_gk, gs, count, weights=d_w)
        serial.append((o, c))
    torch.cuda.synchronize()
    qh = lambda d: q_slots(native.to_host(d), 2 * G, count, R, n)
    qc = lambda d: q_slots(native.to_host(d), 2, count, R, n)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    scr = [S.ev.scratch(count), S.ev.scratch(count)]
    outs = [(new_h(), torch.zeros_like(ins[0])) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                S.ev.apply_galois_hoisted(outs[i][0], ins[i], d_gk, gs, count, scratch=scr[i], stream=streams[i])
                S.ev.galois_sum(outs[i][1], ins[i], d_gk, gs, count, weights=d_w, scratch=scr[i], stream=streams[i])
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(qh(outs[i][0]), qh(serial[i][0]))
        assert np.array_equal(qc(outs[i][1]), qc(serial[i][1]))
    # one capture of each call on a single stream (a linear graph, no forked streams), replayed twice
    cap_h, cap_c = new_h(), torch.zeros_like(ins[0])
    s = torch.cuda.Stream()
    graphs = [torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()]
    torch.cuda.synchronize()
    with torch.cuda.graph(graphs[0], stream=s):
        S.ev.apply_galois_hoisted(cap_h, ins[0], d_gk, gs, count, scratch=scr[0], stream=s)
    with torch.cuda.graph(graphs[1], stream=s):
        S.ev.galois_sum(cap_c, ins[0], d_gk, gs, count, weights=d_w, scratch=scr[1], stream=s)
    for _ in range(2):
        cap_h.zero_()
        cap_c.zero_()
        graphs[0].replay()
        graphs[1].replay()
        torch.cuda.synchronize()
        assert np.array_equal(qh(cap_h), qh(serial[0][0]))
        assert np.array_equal(qc(cap_c), qc(serial[0][1]))
    del graphs
    S.close()
