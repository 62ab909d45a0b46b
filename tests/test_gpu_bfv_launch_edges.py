"""GPU: the BFV launch layer's element-wise kernels (kernels_bfv.hip, kernels_epi.cuh, bfv_host.cpp) at their edges.  Inputs come from
tests/bfv_launch_inputs.py (tests/test_bfv_launch_edges_host.py shows on the CPU that each reaches the branch it was built for); every
expected word comes from the oracle's literal restatement of the reference.  Every word of every buffer a driver touches is compared,
scratch slots included; the one exception is the dropped prime's c1 slot of a batch, as in tests/test_gpu_bfv_drivers.py."""
import statistics

import numpy as np
import pytest

import bfv_launch_inputs as LI
from test_bfv_launch_edges_host import literal_inputs, oracle_decrypt

M64 = LI.M64


def make_ctx(ps, **kw):
    from ntt_cuda_amd import bfv
    return bfv.BFVContext(ps.n, ps.qs, ps.psis, ps.t, ps.gamma, **kw)


def run_decrypt(native, oracle, ctx, ps, c, sk):
    import torch
    want, _ = oracle_decrypt(oracle, ps, c, sk)
    d_c, d_sk = native.to_device(c), native.to_device(sk)
    ctx.decrypt(d_c, d_sk)
    torch.cuda.synchronize()
    assert np.array_equal(native.to_host(d_c).reshape(2, ps.R, ps.n), want), ps
    assert np.array_equal(native.to_host(d_sk), sk)


def run_encrypt(native, oracle, ctx, ps, c, pk, e, m):
    import torch
    want = oracle.bfv_encrypt_core(c, pk, e, m, ps.qs, ps.psis, ps.n, ps.t).reshape(2, ps.R, ps.n)
    d_c, d_pk, d_e, d_m = (native.to_device(x) for x in (c, pk, e, m))
    ctx.encrypt(d_c, d_pk, d_e, d_m)
    torch.cuda.synchronize()
    assert np.array_equal(native.to_host(d_c).reshape(2, ps.R, ps.n), want), ps
    for d, h in ((d_pk, pk), (d_e, e), (d_m, m)):
        assert np.array_equal(native.to_host(d), h)


def keygen_inputs(oracle, ps, seed):
    w, e, _ = LI.craft_keygen(ps, seed)
    prm = oracle.Params(ps.n, ps.qs, ps.psis)
    return LI.delta_key(ps), np.stack([np.zeros_like(w), oracle.forward_batch(w, prm).reshape(ps.R, ps.n)]), e


def keygen_ntt_inputs(oracle, ps, seed):
    a_hat, e_hat, _ = LI.craft_keygen_ntt(ps, seed)
    e = oracle.inverse_batch(e_hat, oracle.Params(ps.n, ps.qs, ps.psis)).reshape(ps.R, ps.n)
    return LI.delta_key(ps), np.stack([np.zeros_like(a_hat), a_hat]), e


def run_keygen(native, oracle, ctx, ps, sk, pk, e):
    import torch
    want_sk, want_pk = oracle.bfv_keygen_core(sk, pk, e, ps.qs, ps.psis, ps.n)
    d_sk, d_pk, d_e = (native.to_device(x) for x in (sk, pk, e))
    ctx.keygen(d_sk, d_pk, d_e)
    torch.cuda.synchronize()
    assert np.array_equal(native.to_host(d_sk), want_sk), ps
    assert np.array_equal(native.to_host(d_pk), want_pk), ps
    assert np.array_equal(native.to_host(d_e), e)


# ---- 1. single drivers, crafted inputs
@pytest.mark.gpu
@pytest.mark.parametrize("driver", ["keygen", "keygen-ntt", "encrypt", "decrypt"])
@pytest.mark.parametrize("idx", range(len(LI.SINGLE_NAMES)), ids=LI.SINGLE_NAMES)
def test_single_drivers_on_crafted_inputs(native, oracle, gpu, idx, driver):
    """keygen: w + e placed in the coefficient domain (what the reference's sequence adds); keygen-ntt: a_hat + NTT(e) placed in the NTT
    domain, which is the sum k_keygen_pk0 forms on these (exact) contexts"""
    ps = LI.single_sets()[idx]
    ctx = make_ctx(ps)
    assert not ctx.uses_literal_kernels
    if driver == "decrypt":
        c, _ = LI.craft_decrypt(ps, 100 + idx)
        run_decrypt(native, oracle, ctx, ps, c, LI.identity_key(ps, ps.r))
    elif driver == "encrypt":
        c, e, m, _ = LI.craft_encrypt(ps, 200 + idx)
        run_encrypt(native, oracle, ctx, ps, c, np.ones((2, ps.R, ps.n), dtype=np.uint64), e, m)
    elif driver == "keygen-ntt":
        run_keygen(native, oracle, ctx, ps, *keygen_ntt_inputs(oracle, ps, 350 + idx))
    else:
        run_keygen(native, oracle, ctx, ps, *keygen_inputs(oracle, ps, 300 + idx))
    ctx.close()


# ---- 2. literal contexts: the reference's own sequence, and the exact kernels where the reference's result is canonical
@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(LI.LITERAL_NAMES)), ids=LI.LITERAL_NAMES)
def test_literal_contexts_against_oracle(native, oracle, gpu, idx):
    ps = LI.literal_sets()[idx]
    ctx = make_ctx(ps)
    assert ctx.uses_literal_kernels
    c, _ = LI.craft_decrypt(ps, 400 + idx)
    run_decrypt(native, oracle, ctx, ps, c, LI.identity_key(ps, ps.r))
    c, e, m, _ = LI.craft_encrypt(ps, 500 + idx)
    run_encrypt(native, oracle, ctx, ps, c, np.ones((2, ps.R, ps.n), dtype=np.uint64), e, m)
    run_keygen(native, oracle, ctx, ps, *keygen_inputs(oracle, ps, 600 + idx))
    rng = np.random.default_rng(idx)                                      # and a key that is not the identity
    sk = np.stack([LI.uniform(rng, q, ps.n) for q in ps.qs[: ps.r]])
    run_decrypt(native, oracle, ctx, ps, c, sk)
    ctx.close()
    found = literal_inputs(oracle, ps)
    ctx = make_ctx(ps, exact_on_inexact_primes=True)
    assert not ctx.uses_literal_kernels
    _, c, _ = found["decrypt"]
    run_decrypt(native, oracle, ctx, ps, c, LI.identity_key(ps, ps.r))
    _, c, e, m, _ = found["encrypt"]
    run_encrypt(native, oracle, ctx, ps, c, np.ones((2, ps.R, ps.n), dtype=np.uint64), e, m)
    _, a_hat, e, _ = found["keygen"]                                      # k_keygen_pk0 on Barrett-inexact primes in place of the reference's sequence
    run_keygen(native, oracle, ctx, ps, LI.delta_key(ps), np.stack([np.zeros_like(a_hat), a_hat]), e)
    ctx.close()


# ---- 3. pointers aligned to 8 bytes only: the V = 1 forms
def offset_view(native, a):
    """(device buffer one word longer with sentinels around the data, its [1:-1] view: 8 bytes off a 16-byte boundary)"""
    import torch
    buf = torch.full((a.size + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:-1]
    view.copy_(native.to_device(a).reshape(-1))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return buf, view


def sentinels_intact(buf):
    return int(buf[0]) == 0x5A5A5A5A5A5A5A5A and int(buf[-1]) == 0x5A5A5A5A5A5A5A5A


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["encrypt-c", "encrypt-e", "encrypt-m", "decrypt-c", "keygen-pk", "keygen-e", "keygen-sk",
                                  "literal:keygen-pk", "literal:keygen-e"])
def test_pointers_aligned_to_eight_bytes_only(native, oracle, gpu, case):
    """each operand in turn as a view one word into a longer buffer: the words of the aligned call (pinned on the oracle above, and once
    more here for the literal context), and the word in front of the view and the word behind it untouched.  k_encrypt_tail<1>,
    k_decrypt_scale<1>, k_decrypt_round<1> and k_keygen_pk0<1> (pk, sk) run on an exact context, where keygen only copies e; k_add_negate
    runs on literal contexts alone, so its V = 1 form takes pk or e of a literal set"""
    import torch
    idx = 3
    literal = case.startswith("literal:")
    ps = LI.literal_sets()[1] if literal else LI.single_sets()[idx]
    ctx = make_ctx(ps)
    assert bool(ctx.uses_literal_kernels) == literal
    driver, which = case.split(":")[-1].split("-")
    if driver == "encrypt":
        c, e, m, _ = LI.craft_encrypt(ps, 200 + idx)
        host = dict(c=c, pk=np.ones((2, ps.R, ps.n), dtype=np.uint64), e=e, m=m)
        call = lambda d: ctx.encrypt(d["c"], d["pk"], d["e"], d["m"])
    elif driver == "decrypt":
        host = dict(c=LI.craft_decrypt(ps, 100 + idx)[0], sk=LI.identity_key(ps, ps.r))
        call = lambda d: ctx.decrypt(d["c"], d["sk"])
    else:
        sk, pk, e = keygen_inputs(oracle, ps, 300 + idx)
        host = dict(sk=sk, pk=pk, e=e)
        call = lambda d: ctx.keygen(d["sk"], d["pk"], d["e"])
    aligned = {k: native.to_device(v).reshape(-1) for k, v in host.items()}
    call(aligned)
    dev = {k: native.to_device(v).reshape(-1) for k, v in host.items()}
    buf, dev[which] = offset_view(native, host[which])
    call(dev)
    torch.cuda.synchronize()
    for k in host:
        assert torch.equal(dev[k], aligned[k]), (case, k)
    assert sentinels_intact(buf), case
    if literal:
        want_sk, want_pk = oracle.bfv_keygen_core(host["sk"], host["pk"], host["e"], ps.qs, ps.psis, ps.n)
        assert np.array_equal(native.to_host(dev["pk"]), want_pk.reshape(-1)) and np.array_equal(native.to_host(dev["sk"]), want_sk.reshape(-1))
    ctx.close()


# ---- 4. (and 5., when its prime exists) the fused epilogue, every class, both kernels
_POOL = {}


def class_entry(ci):
    return LI.epi_off_set() if ci == len(LI.CLASS_NAMES) else LI.class_sets()[ci]


def class_pool(oracle, ci):
    """per class set: four crafted ciphertexts and PLAIN_POOL random ones with what the reference leaves of each under the identity key"""
    if ci not in _POOL:
        ps = class_entry(ci)[0]
        sk = LI.identity_key(ps, ps.R)
        rng = np.random.default_rng(900 + ci)
        crafted = [LI.craft_decrypt(ps, 700 + 10 * ci + j)[0] for j in range(4)]
        plain = [np.stack([np.stack([LI.uniform(rng, q, ps.n) for q in ps.qs]) for _ in range(2)]) for _ in range(LI.PLAIN_POOL)]
        _POOL[ci] = [(c, oracle_decrypt(oracle, ps, c, sk)[0]) for c in crafted], [(c, oracle_decrypt(oracle, ps, c, sk)[0]) for c in plain]
    return _POOL[ci]


def compare_batch(got, wants, R):
    for z, w in enumerate(wants):
        assert np.array_equal(got[0, z], w[0]), z
        assert np.array_equal(got[1, z, : R - 1], w[1, : R - 1]), z           # (the dropped prime's c1 slot is scratch in the batch)


@pytest.mark.gpu
@pytest.mark.parametrize("count", LI.BATCH_COUNTS)
@pytest.mark.parametrize("ci", range(len(LI.CLASS_NAMES) + 1), ids=LI.CLASS_NAMES + ("class-epi-off",))
def test_batched_decryption_every_class_both_epilogue_kernels(native, oracle, gpu, ci, count):
    """decrypt_batch at n = 2^15, R = 2 on the small-batch side (k_lat_inv_a_epi, every class), the persistent side (k_polymul15_epi where
    epi_class() holds, the two-step path elsewhere) and across the head / tail cut (bfv_launch_inputs.BATCH_COUNTS).  Crafted ciphertexts
    first, last and on both sides of the cut; the others cycle through PLAIN_POOL = 37 random ones (a period coprime to the cut, the tail
    and the batch sizes) -- every ciphertext against the oracle in full.  The last set is item 5's: a prime on which the driver must take
    the two-step path; the search (tests/test_bfv_launch_edges_host.py records its outcome) found none, and the case then has nothing to run"""
    import torch
    if class_entry(ci) is None:
        assert LI.search_epi_off_prime() == (None, LI.EPI_OFF_BUDGET)
        return
    ps, cls, _ = class_entry(ci)
    nctx = native.NTTContext(ps.n, ps.qs, ps.psis)
    assert nctx.kernel_class == cls and nctx.literal_routing == 0
    nctx.close()
    ctx = make_ctx(ps)
    crafted, plain = class_pool(oracle, ci)
    slots = LI.crafted_slots(count)
    pick = [crafted[slots.index(z)] if z in slots else plain[z % len(plain)] for z in range(count)]
    c = np.stack([np.stack([p[0][h] for p in pick]) for h in range(2)])                  # [2][count][R][n]
    d_c, d_sk = native.to_device(c), native.to_device(LI.identity_key(ps, ps.R))
    ctx.decrypt_batch(d_c, d_sk, count)
    torch.cuda.synchronize()
    compare_batch(native.to_host(d_c).reshape(2, count, ps.R, ps.n), [p[1] for p in pick], ps.R)
    if count == LI.BATCH_COUNTS[-1]:                                                     # a key that is not the identity
        sk = np.stack([LI.uniform(np.random.default_rng(ci), q, ps.n) for q in ps.qs])
        d_c, d_sk = native.to_device(c), native.to_device(sk)
        ctx.decrypt_batch(d_c, d_sk, count)
        torch.cuda.synchronize()
        got = native.to_host(d_c).reshape(2, count, ps.R, ps.n)
        for z in (0, count // 2, count - 1):
            w = oracle_decrypt(oracle, ps, np.ascontiguousarray(c[:, z]), sk)[0]
            assert np.array_equal(got[0, z], w[0]) and np.array_equal(got[1, z, : ps.r], w[1, : ps.r]), z
    ctx.close()


# ---- 6. samplers on crafted bytes
UNIFORM_WORDS = [0, 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, 1 << 63, (1 << 64) - (1 << 10), (1 << 64) - 1]
GAUSSIAN_WORDS = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF]


def sampler_sets():
    p25 = LI.small_primes()[2]
    e62 = LI.P.EDGE_PRIMES[62][0]
    return [LI.ParamSet("n2048-R2-25+62", 2048, *LI.with_roots([p25, e62], 2048), 1024, LI.P.GAMMA61), LI.single_sets()[1]]


def gaussian_real_value(words):
    """3.2 Phi^-1(d) in double precision for the float d the kernels form from each word"""
    d = words.astype(np.float32) / np.float32(4294967295.0)
    eps = np.float32(1.192092896e-07)
    d = np.where(d == 0, d + eps, np.where(d == 1, d - eps, d)).astype(np.float32)
    inv = statistics.NormalDist().inv_cdf
    return np.array([float(np.float32(3.2)) * inv(float(x)) for x in d])


def check_gaussian(got, want, words, qs):
    signed = [np.where(g > q // 2, g.astype(np.int64) - q, g.astype(np.int64)) for g, q in zip(got, qs)]
    want_signed = np.where(want[0] > qs[0] // 2, want[0].astype(np.int64) - qs[0], want[0].astype(np.int64))
    for s in signed:
        assert np.array_equal(s, signed[0])                                  # the same signed value for every prime
    real = gaussian_real_value(words)
    decided = (np.abs(real - np.rint(real)) > 1e-3) | (np.abs(real) > 19.2 + 1e-3)
    diff = signed[0] - want_signed
    bad = np.nonzero((np.abs(diff) > 1) | (decided & (diff != 0)))[0]
    assert bad.size == 0, [(hex(int(words[i])), int(signed[0][i]), int(want_signed[i]), float(real[i])) for i in bad[:8]]


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(2), ids=["R2", "R16"])
def test_samplers_on_crafted_bytes(native, oracle, gpu, si):
    import torch
    ps = sampler_sets()[si]
    n, R, qs = ps.n, ps.R, ps.qs
    assert {q.bit_length() for s in sampler_sets() for q in s.qs} >= {25, 55, 62}
    ctx = make_ctx(ps)
    rng = np.random.default_rng(40 + si)
    tern = np.concatenate([np.arange(256, dtype=np.uint8)[::-1], np.arange(256, dtype=np.uint8), rng.integers(0, 256, size=n - 512, dtype=np.uint8)])
    uni = rng.integers(0, 1 << 64, size=(R, n), dtype=np.uint64)
    for i in range(R):
        for j, p in enumerate(LI.positions(n)):
            uni[i, p] = UNIFORM_WORDS[(i + j) % len(UNIFORM_WORDS)]
    gw = [rng.integers(0, 1 << 32, size=n, dtype=np.uint32) for _ in range(3)]
    for k, g in enumerate(gw):
        for j, p in enumerate(LI.positions(n)):
            g[p] = GAUSSIAN_WORDS[(j + k) % len(GAUSSIAN_WORDS)]
    z64 = lambda *shape: torch.full(shape, -1, dtype=torch.int64, device=gpu)
    # keygen's samplers: n ternary bytes, R n uniform words, n Gaussian words
    rnd = np.concatenate([tern, uni.reshape(-1).view(np.uint8), gw[0].view(np.uint8)])
    assert ctx.keygen_random_bytes == 9 * R * n + 4 * n >= rnd.size         # (bfv_keygen.cuh:99 draws more than its samplers read)
    rnd = np.concatenate([rnd, np.zeros(ctx.keygen_random_bytes - rnd.size, dtype=np.uint8)])
    sk, pk, tmp = z64(R, n), z64(2, R, n), z64(R, n)
    ctx.sample_keygen(torch.from_numpy(rnd).to(gpu), sk, pk, tmp)
    torch.cuda.synchronize()
    want_t = oracle.sample_xq("ternary", tern, n, qs)
    assert np.array_equal(native.to_host(sk), want_t) and (want_t[:, 0] == 2).all() and (want_t[:, 255] == np.array(qs, np.uint64) - np.uint64(1)).all()
    got_u = native.to_host(pk)
    assert np.array_equal(got_u[1], oracle.sample_xq("uniform", uni.reshape(-1).view(np.uint8), n, qs))
    assert all((got_u[1, i] < np.uint64(q)).all() for i, q in enumerate(qs)) and (got_u[0] == np.uint64(M64)).all()      # (pk0 is not the sampler's)
    check_gaussian(native.to_host(tmp), oracle.sample_xq("gaussian", gw[0].view(np.uint8), n, qs), gw[0], qs)
    # encryption's sampler: n ternary bytes, n + n Gaussian words
    rnd = np.concatenate([tern, gw[1].view(np.uint8), gw[2].view(np.uint8)])
    assert rnd.size == ctx.encrypt_random_bytes
    c, e = z64(2, R, n), z64(2, R, n)
    ctx.sample_encrypt(torch.from_numpy(rnd).to(gpu), c, e)
    torch.cuda.synchronize()
    got_c, got_e = native.to_host(c), native.to_host(e)
    assert np.array_equal(got_c[0], want_t) and np.array_equal(got_c[1], want_t)
    for h in range(2):
        check_gaussian(got_e[h], oracle.sample_xq("gaussian", gw[1 + h].view(np.uint8), n, qs), gw[1 + h], qs)
    ctx.close()
