"""GPU: the BFV evaluator's key, plaintext and Galois kernels on crafted words (tests/bfv_edge_inputs.py; tests/
test_bfv_galois_edges_host.py shows on the CPU that each set reaches what it was built for), every Q-slot word against the CPU model
(tests/bfv_hoist_model.py) with np.array_equal: the coefficient gather's negation of 0, q_i, 1 and q_i - 1, the 128-bit
accumulators of the inner products at their peak, -(a s + e) at 0 and at its maximum, c0 +/- E(m) on its wraps, a 30-bit prime among
61-bit ones, and a batch large enough for the large-batch transforms.  Outputs start as sentinel words, which the special prime's
slot must keep; inputs carry the sentinel there as well."""
import numpy as np
import pytest

from bfv_edge_inputs import SENT as INPUT_SENT
from bfv_edge_inputs import (SUM_ELEMS, constant_message, galois_elements, gather_set, key_set, mixed_width_set, peak_set, peak_set_unit,
                             plain_set, random_keys, sum_elements, top_keys)
from bfv_sweep_inputs import demo_subset, wide_subset
from test_gpu_bfv_eval import SENT, q_slots, sentinel, special_untouched
from test_gpu_bfv_eval_sweep import GAMMA, Sch, compare, model_of
from test_gpu_bfv_plain_galois import with_q_words

N, T = 2048, 1024
CRAFT_R = [1, 2, 4, 15]
assert INPUT_SENT == SENT                    # the inputs' special slots hold the word the outputs are checked for


class Ev:
    """an evaluator and its model on (qs, psis), no keys"""

    def __init__(self, native, oracle, qs, psis, n=N, t=T):
        from ntt_cuda_amd import bfv
        self.native, self.n, self.t, self.qs = native, n, t, list(qs)
        self.R, self.r = len(qs), len(qs) - 1
        self.ctx = bfv.BFVContext(n, qs, psis, t, GAMMA)
        self.ev = bfv.BFVEvaluator(self.ctx)
        self.model = model_of(native, oracle, self.ev, n, list(qs), list(psis), t)

    def check(self, d_out, want, comps=2, count=1, what=""):
        """every Q-slot word of a [comps][count][R][n] output; the special slot still the sentinel"""
        import torch
        torch.cuda.synchronize()
        got = q_slots(self.native.to_host(d_out), comps, count, self.R, self.n)
        assert np.array_equal(got, q_slots(want, comps, count, self.R, self.n)), (self.r, what)
        assert special_untouched(self.native, d_out, comps, count, self.R, self.n), (self.r, what)

    def out(self, comps=2, count=1):
        return sentinel(self.native, comps * count * self.R * self.n)

    def close(self):
        self.ev.close()
        self.ctx.close()


def wide(native, oracle, r):
    return Ev(native, oracle, *wide_subset(N, r, native.barrett_is_exact))


def hoisted_and_sums(E, a, keys, gs, weights, what):
    """apply_galois_hoisted and galois_sum (plain, weighted, each also in place) of the ciphertext a [2][1][R][n] with keys
    [G][r][2][R][n] for the elements gs, weights [G][r][n] as plain_ntt writes them"""
    import torch
    native, M, ev, R, r, n = E.native, E.model, E.ev, E.R, E.r, E.n
    G = len(gs)
    d_a, d_gk = native.to_device(a), native.to_device(np.ascontiguousarray(keys))
    terms = M.terms(a[:, 0], keys, gs)
    d_out = sentinel(native, G * 2 * R * n)
    ev.apply_galois_hoisted(d_out, d_a, d_gk, gs, 1)
    torch.cuda.synchronize()
    got = native.to_host(d_out).reshape(G, 2, R, n)
    for k, g in enumerate(gs):
        assert np.array_equal(got[k][:, :r], M.hoisted(a[:, 0], keys[k], g, term=terms[k])[:, :r]), (r, what, "apply_galois_hoisted", k, g)
    assert np.all(got[:, :, R - 1] == np.uint64(SENT)), (r, what)
    d_w = native.to_device(np.ascontiguousarray(weights))
    for d_wt, wt in ((None, None), (d_w, list(weights))):
        name = "%s, galois_sum %s" % (what, "plain" if wt is None else "weighted")
        want = M.galois_sum(a[:, 0], keys, gs, wt, terms=terms).reshape(2, 1, R, n)
        d_c = E.out()
        ev.galois_sum(d_c, d_a, d_gk, gs, 1, weights=d_wt)
        E.check(d_c, want, what=name)
        d_b = d_a.clone()                                                      # in place: c aliasing a
        ev.galois_sum(d_b, d_b, d_gk, gs, 1, weights=d_wt)
        E.check(d_b, want, what=name + ", in place")


def model_weights(E, ms):
    """plain_ntt of the messages ms [G][n] on the GPU, held to the model's; returns the model's [G][r][n]"""
    import torch
    G = ms.shape[0]
    d_w = torch.full((G * E.r * E.n,), SENT, dtype=torch.int64, device="cuda")
    E.ev.plain_ntt(d_w, E.native.to_device(ms), G)
    torch.cuda.synchronize()
    want = np.stack([E.model.plain_ntt(ms[k]) for k in range(G)])
    assert np.array_equal(E.native.to_host(d_w).reshape(G, E.r, E.n), want), (E.r, "plain_ntt")
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["top", "random"])
@pytest.mark.parametrize("r", CRAFT_R)
def test_gather_set(native, oracle, gpu, r, key):
    """0, q_i, 1, q_i - 1 and q_i - 2 under the coefficient gather's negation (k_galois_digits, k_hoist_finish) for the six elements of
    galois_elements, with keys of q_j - 1 in every word and with random keys"""
    E = wide(native, oracle, r)
    a = gather_set(E.qs, N, 400 + r)
    gs = galois_elements(N)
    keys = top_keys(E.qs, N, len(gs)) if key == "top" else random_keys(E.qs, N, len(gs), 410 + r)
    d_a = native.to_device(a)
    for k, g in enumerate(gs):
        d_c = E.out()
        E.ev.apply_galois(d_c, d_a, native.to_device(keys[k]), g, 1)
        E.check(d_c, E.model.apply_galois(a[:, 0], keys[k], g).reshape(2, 1, E.R, N), what="apply_galois %d, %s key" % (g, key))
    ms = np.random.default_rng(420 + r).integers(0, T, size=(len(gs), N), dtype=np.uint64)
    hoisted_and_sums(E, a, keys, gs, model_weights(E, ms), "gather set, %s key" % key)
    E.close()


def run_peak_sets(E, what):
    """group + 1 elements; at r = 1, 2 also SUM_ELEMS, more than one inner-product launch of galois_sum: P is read back at the peak"""
    qs, M = E.qs, E.model
    sizes = sorted({E.ev.hoist_group + 1, SUM_ELEMS} if E.r <= 2 else {E.ev.hoist_group + 1})
    for c, name in ((peak_set(qs, N), "peak set"), (peak_set_unit(qs, N), "unit peak set")):
        for G in sizes:
            gs = sum_elements(N, G)
            w = model_weights(E, constant_message(N, T - 1, G))
            assert all(np.all(w[:, j] == np.uint64(q - 1)) for j, q in enumerate(M.qs))
            hoisted_and_sums(E, c, top_keys(qs, N, G), gs, w, "%s, %s, G = %d" % (what, name, G))
    # the same c1 as the third component of a product: k_relin_dot's NTT-domain peak
    c = peak_set(qs, N)
    c3 = np.concatenate([c[:1], c[:1], c[1:]])
    rlk = top_keys(qs, N, 1)[0]
    d_c = E.out()
    E.ev.relinearize(d_c, E.native.to_device(c3), E.native.to_device(rlk), 1)
    E.check(d_c, M.relinearize(c3[:, 0], rlk).reshape(2, 1, E.R, N), what=what + ", relinearize at the peak")
    g = 2 * N - 1
    d_c = E.out()
    E.ev.apply_galois(d_c, E.native.to_device(c), E.native.to_device(rlk), g, 1)
    E.check(d_c, M.apply_galois(c[:, 0], rlk, g).reshape(2, 1, E.R, N), what=what + ", apply_galois at the peak")


@pytest.mark.gpu
@pytest.mark.parametrize("r", CRAFT_R)
def test_peak_sets(native, oracle, gpu, r):
    """x^0-only ciphertexts, keys and weights of q_j - 1: every NTT-domain 128-bit sum of k_hoist_dot, k_hoist_sum and k_relin_dot at
    (q_j - 1) + r (qmin - 1) (q_j - 1), k_hoist_sum's weighted chain at (q_j - 1)^2 + s, across more than one launch"""
    E = wide(native, oracle, r)
    run_peak_sets(E, "wide primes")
    E.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", CRAFT_R)
def test_key_set(native, oracle, gpu, r):
    """k_relin_key and k_galois_key with a s + e = 0 (mod q) by both routes (the `v ? q - v : 0` select) and at its maximum"""
    import torch
    E = wide(native, oracle, r)
    R, M = E.R, E.model
    for shift, g in enumerate((1, 3, 2 * N - 1)):
        sk, a, e = key_set(E.qs, N, shift)
        d_sk, d_a, d_e = native.to_device(sk), native.to_device(a), native.to_device(e)
        for name, call, want in (("relin_keygen", lambda d: E.ev.relin_keygen(d, d_sk, d_a, d_e), M.relin_keygen(sk, a, e)),
                                 ("galois_keygen", lambda d: E.ev.galois_keygen(d, d_sk, g, d_a, d_e), M.galois_keygen(sk, g, a, e))):
            d_k = sentinel(native, r * 2 * R * N)
            call(d_k)
            E.check(d_k, want.reshape(2 * r, 1, R, N), comps=2 * r, what="%s, shift %d, g = %d" % (name, shift, g))
        torch.cuda.synchronize()
        assert np.array_equal(native.to_host(d_sk).reshape(R, N), sk)                     # inputs are left as they were
    E.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", CRAFT_R)
def test_plain_set(native, oracle, gpu, r):
    """k_plain_addsub on the wraps of c0 +/- E(m), k_plain_lift on the lift's boundary; multiply_plain (k_plain_copy around the fused
    products) on the peak set's ciphertext with the plaintexts -1 and -t/2"""
    import torch
    E = wide(native, oracle, r)
    R, M, ev = E.R, E.model, E.ev
    a, m = plain_set(E.qs, N, T, 500 + r)
    d_a, d_m = native.to_device(a), native.to_device(m)
    for sub in (False, True):
        d_c = E.out()
        (ev.sub_plain if sub else ev.add_plain)(d_c, d_a, d_m, 1)
        E.check(d_c, M.add_plain(a[:, 0], m[0], sub=sub).reshape(2, 1, R, N), what="sub_plain" if sub else "add_plain")
        d_b = d_a.clone()                                                                 # in place
        (ev.sub_plain if sub else ev.add_plain)(d_b, d_b, d_m, 1)
        E.check(d_b, M.add_plain(a[:, 0], m[0], sub=sub).reshape(2, 1, R, N), what="in place")
    model_weights(E, m)
    c = peak_set(E.qs, N)
    d_c_in = native.to_device(c)
    for v in (T - 1, T // 2):
        pm = constant_message(N, v)
        mhat = model_weights(E, pm)
        want = M.multiply_plain_ntt(c[:, 0], mhat[0]).reshape(2, 1, R, N)
        d_mhat = native.to_device(mhat)
        d_c = E.out()
        ev.multiply_plain(d_c, d_c_in, native.to_device(pm), 1)
        E.check(d_c, want, what="multiply_plain %d" % v)
        for shared in (False, True):
            d_c = E.out()
            ev.multiply_plain_ntt(d_c, d_c_in, d_mhat, 1, shared=shared)
            E.check(d_c, want, what="multiply_plain_ntt %d shared=%s" % (v, shared))
    E.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small_at", [0, 2])
def test_mixed_width_moduli(native, oracle, gpu, small_at):
    """one 30-bit prime among 61-bit ones: red64 of a 61-bit digit into the small prime has a quotient of about 2^31 (every other
    tested set has primes of one width, where it is 0 or 1).  Creation accepts such a set: the size condition only gets easier"""
    qs, psis = mixed_width_set(N, T, native.barrett_is_exact, small_at)
    S = Sch(native, oracle, N, qs, psis, T)
    compare(S, 2, ("plain", "galois", "hoist"))
    S.close()
    E = Ev(native, oracle, qs, psis)
    run_peak_sets(E, "mixed widths, small prime at %d" % small_at)
    E.close()


@pytest.mark.gpu
def test_large_batch_equals_looped(native, oracle, gpu):
    """count = 151 ciphertexts at n = 2048, r = 3: every transform batch of the calls below is larger than both small-batch thresholds
    of the n = 2^11 kernels (lat_threshold<11>: 256 polynomials for plain transforms, 448 for fused products), so the large-batch
    kernels run, which the other evaluator tests (count <= 4) never reach outside multiply_relin.  The smallest batches are count r =
    453 (the lift of multiply_plain: plain, > 256; each half of its fused products: fused, > 448); the others are 2 count r = 906
    (inverse transforms, the shared fused product), count r^2 = 1359 and count r (r + 1) = 1812 (digits).  count is odd: the inner
    products take two ciphertexts per thread, 76 chunks with a last half-empty one.  Every ciphertext's words must equal those of the
    same call on that ciphertext alone (which the other tests hold to the model); three of them are held to the model here"""
    import torch
    n, r, count = N, 3, 151
    assert count * r > 448 and count % 2 == 1
    qs, psis = demo_subset(n, r)
    S = Sch(native, oracle, n, qs, psis, T)
    M, ev, R = S.model, S.ev, S.R
    m = S.messages(2 * count)
    a = with_q_words(S, S.encrypt(m[:count]), 2, count)
    pm = m[count:]
    pm[0, :5] = [0, T // 2 - 1, T // 2, T - 1, T + 3]
    d_a, d_m = native.to_device(a), native.to_device(pm).reshape(-1)
    gs = sum_elements(n, ev.hoist_group + 1)
    G = len(gs)
    a_s = np.stack([np.stack([S.rng.integers(0, q, size=n, dtype=np.uint64) for q in qs]) for _ in range(r)])
    keys = []
    for g in gs:
        d_k = torch.zeros(r * 2 * R * n, dtype=torch.int64, device="cuda")
        ev.galois_keygen(d_k, S.d_sk, g, native.to_device(a_s), native.to_device(S.e))
        keys.append(d_k)
    d_gk = torch.cat(keys)
    gk = native.to_host(d_gk).reshape(G, r, 2, R, n)
    wm = S.messages(G)
    d_w = torch.zeros(G * r * n, dtype=torch.int64, device="cuda")
    ev.plain_ntt(d_w, native.to_device(wm), G)
    d_mhat = torch.zeros(count * r * n, dtype=torch.int64, device="cuda")
    ev.plain_ntt(d_mhat, d_m, count)
    torch.cuda.synchronize()
    w, mhat = native.to_host(d_w).reshape(G, r, n), native.to_host(d_mhat).reshape(count, r, n)
    ct = 2 * R * n

    def calls(d_x, d_pm, d_pmhat, cnt, scratch):
        """name -> output [comps][cnt][R][n] of every call on the cnt ciphertexts d_x"""
        res = {}

        def run(name, fn, comps=2):
            d_o = sentinel(native, comps * cnt * R * n)
            fn(d_o)
            res[name] = d_o

        run("add_plain", lambda o: ev.add_plain(o, d_x, d_pm, cnt))
        run("multiply_plain", lambda o: ev.multiply_plain(o, d_x, d_pm, cnt, scratch=scratch))
        run("multiply_plain_ntt", lambda o: ev.multiply_plain_ntt(o, d_x, d_pmhat, cnt, shared=False, scratch=scratch))
        run("multiply_plain_ntt shared", lambda o: ev.multiply_plain_ntt(o, d_x, d_mhat[: r * n], cnt, shared=True, scratch=scratch))
        run("apply_galois", lambda o: ev.apply_galois(o, d_x, keys[0], gs[0], cnt, scratch=scratch))
        run("apply_galois_hoisted", lambda o: ev.apply_galois_hoisted(o, d_x, d_gk, gs, cnt, scratch=scratch), 2 * G)
        run("galois_sum", lambda o: ev.galois_sum(o, d_x, d_gk, gs, cnt, weights=d_w, scratch=scratch))
        torch.cuda.synchronize()
        return {k: native.to_host(v).reshape(-1, 2, cnt, R, n) for k, v in res.items()}

    got = calls(d_a, d_m, d_mhat, count, ev.scratch(count))
    for name, x in got.items():
        assert np.all(x[:, :, :, R - 1] == np.uint64(SENT)), name
    scr = ev.scratch(1)
    for z in range(count):
        one = calls(native.to_device(np.ascontiguousarray(a[:, z])), d_m[z * n: (z + 1) * n], d_mhat[z * r * n: (z + 1) * r * n], 1, scr)
        for name, x in one.items():
            assert np.array_equal(got[name][:, :, z, :r], x[:, :, 0, :r]), (name, z)
    for z in (0, count // 2, count - 1):
        c = a[:, z]
        want = {"add_plain": M.add_plain(c, pm[z]), "multiply_plain": M.multiply_plain_ntt(c, mhat[z]),
                "multiply_plain_ntt": M.multiply_plain_ntt(c, mhat[z]), "multiply_plain_ntt shared": M.multiply_plain_ntt(c, mhat[0]),
                "apply_galois": M.apply_galois(c, gk[0], gs[0]), "galois_sum": M.galois_sum(c, gk, gs, list(w))}
        hoist = M.hoist(c)
        want["apply_galois_hoisted"] = np.concatenate([M.hoisted(c, gk[k], g, hoist) for k, g in enumerate(gs)])
        assert np.array_equal(mhat[z], M.plain_ntt(pm[z])), z
        for name, x in want.items():
            assert np.array_equal(got[name][:, :, z, :r].reshape(-1, r, n), x[:, :r]), (name, z)
    S.close()
