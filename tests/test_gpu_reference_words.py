"""Reference binary = oracle = library, word for word, on the GPU.

oracle/_ref/ref60, ref30 and decryption_test are the reference's own kernels built for gfx950 (`make -C oracle ref`: mechanical
translation, with the two inline-PTX functions of its uint128.h restated in oracle/ref_shim.h).  Every test sends one request
(tests/ref_words_cases.py) through one child process and compares the response with the oracle and with the library's routes for the
same operation.  No tolerance anywhere; the one non-integer step, the Gaussian sampler, is word for word between the reference binary
and the library (both call the device's normcdfinvf) and goes through check_gaussian, unchanged, against the oracle's AS241.

The port self-check comes first: if it fails the port is wrong and nothing below means anything, so every other test fails with it."""
import os
import re
import subprocess

import numpy as np
import pytest

import params as P
import ref_py as R
import ref_words_cases as C

# the three binaries and the translated decryption_test they were built from (the self-check reads its arrays) travel together
BUILT = R.available() and os.path.exists(os.path.join(R.REF_DIR, "src", "decryption_test.hip"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not BUILT, reason=R.SKIP_REASON)]

M64 = (1 << 64) - 1
_SELF = {}


def corner_operands():
    """the corner operands of tests/lazy_inputs.py (w_corners, around_multiples) for a 62-, a 60- and a 36-bit modulus, and the machine
    edges 0, 1, 2^32 +- 1, 2^63, 2^64 - 1"""
    import lazy_inputs as LZ
    vals = {0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, M64 - 1, M64}
    for q in (P.EDGE_PRIMES[62][0], P.INEXACT_PRIMES[60][0], P.INEXACT_PRIMES[36][0]):
        vals |= set(LZ.w_corners(q)) | set(LZ.around_multiples(q, 2))
    return sorted(v for v in vals if 0 <= v <= M64)


def self_check():
    """runs once per session; returns None when the port is sound, else the reason"""
    if "result" in _SELF:
        return _SELF["result"]
    _SELF["result"] = "the self-check did not finish"
    try:
        p = subprocess.run([R.DECRYPTION_TEST], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, env=dict(os.environ, **R.CHILD_ENV))
        text = p.stdout.decode("utf-8", "replace")
        assert p.returncode == 0, (p.returncode, text[-500:])
        assert "Computations are correct." in text, text[-500:]
        shown = [int(x) for x in re.search(r"\[([0-9, ]+)\]\s*$", text).group(1).replace(" ", "").strip(",").split(",")]
        assert shown == [i % 10 for i in range(10)], shown
        # the arrays the program decrypts are the committed KAT-1.  The program never prints them (the statements that would are
        # commented out in it), so they are read from the initialisers of the translated source it was built from
        kat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat1_decryption_n4096.npz"))
        with open(os.path.join(R.REF_DIR, "src", "decryption_test.hip")) as f:
            src = f.read()
        for name in ("c_host", "sk_host"):
            m = re.search(r"unsigned long long %s\[\]\s*=\s*\{\s*([0-9, \t]+)\}" % name, src)
            assert m is not None, "no initialiser of %s in oracle/_ref/src/decryption_test.hip" % name
            arr = np.array([int(x) for x in m.group(1).split(",")], dtype=np.uint64)
            assert np.array_equal(arr, kat[name].reshape(-1)), name
        # ref_shim.h on the device against Python integers
        ops = corner_operands()
        pairs = [(x, y) for x in ops for y in ops]
        quads = [(x, y, z, w) for (x, y) in pairs[::7] for (z, w) in ((0, 0), (1, 0), (0, 1), (M64, M64), (y, x), (x, y))]
        triples = [(x, y, s) for (x, y) in pairs[::5] for s in (0, 1, 23, 35, 58, 60, 63, 64)]
        mul, sub, shf = R.run(R.REF60, [R.Case(R.SELFCHECK_MUL64, 0, words=np.array(pairs, dtype=np.uint64)),
                                        R.Case(R.SELFCHECK_SUB128, 0, words=np.array(quads, dtype=np.uint64)),
                                        R.Case(R.SELFCHECK_SHIFT, 0, words=np.array(triples, dtype=np.uint64))])
        mul = mul.reshape(-1, 4)
        for (x, y), row in zip(pairs, mul):
            p_ = x * y
            assert [int(v) for v in row] == [p_ & M64, p_ >> 64, p_ & M64, p_ >> 64], (x, y)
        for (alo, ahi, blo, bhi), row in zip(quads, sub.reshape(-1, 2)):
            d = ((ahi << 64 | alo) - (bhi << 64 | blo)) % (1 << 128)
            assert [int(v) for v in row] == [d & M64, d >> 64], (alo, ahi, blo, bhi)
        # uint128.h's shift members with PTX's clamp (ref_shift.h): a 64-bit shift by 64 or more gives 0, word by word as the source
        # writes it -- `x >> s` and shiftr are the 128-bit shift for s = 1 .. 64, and for s = 0 the low word picks up `high << 64` = 0
        shr = lambda v, c: 0 if c >= 64 else v >> c
        shl = lambda v, c: 0 if c >= 64 else (v << c) & M64
        for (lo, hi, c), row in zip(triples, shf.reshape(-1, 6)):
            right = [shr(lo, c) | shl(hi, 64 - c), shr(hi, c)]
            left = [shl(lo, c), shl(hi, c) | shr(lo, 64 - c)]
            assert [int(v) for v in row] == right + right + left, (lo, hi, c)
            if 1 <= c <= 64:
                assert right == [((hi << 64 | lo) >> c) & M64, (hi << 64 | lo) >> (c + 64)]
        _SELF["result"] = None
    except Exception as exc:            # kept: every dependent test reports it
        _SELF["result"] = "%s: %s" % (type(exc).__name__, exc)
    return _SELF["result"]


@pytest.fixture
def port(gpu):
    why = self_check()
    if why is not None:
        pytest.fail("the port self-check failed, so the reference binaries prove nothing: " + why)


def test_port_self_check(gpu):
    """decryption_test prints `Computations are correct.` and the plaintext i % 10; its c_host / sk_host -- which it does not print, so
    they are parsed out of the translated source it was built from, oracle/_ref/src -- are the committed KAT-1;
    ref_shim.h's mul64 / sub128 and the shift members behind ref_shift.h equal Python integers on the corner operands, on the device."""
    assert self_check() is None, self_check()


def run_group(oracle, group):
    binary, items = group
    outs = R.run(binary, [it.case for it in items])
    for it, got in zip(items, outs):
        if it.expect is None:
            continue
        want = it.expect()
        bad = np.nonzero(got != want)[0] if got.shape == want.shape else np.array([-1])
        assert bad.size == 0, ("reference binary != oracle", it.name, bad[:8], [(hex(int(got[i])), hex(int(want[i]))) for i in bad[:4] if i >= 0])
    return items, outs


def same(got, ref, what):
    bad = np.nonzero(got.reshape(-1) != ref.reshape(-1))[0] if got.size == ref.size else np.array([-1])
    assert bad.size == 0, ("library != reference binary", what, bad[:8], [(hex(int(got.reshape(-1)[i])), hex(int(ref.reshape(-1)[i]))) for i in bad[:4] if i >= 0])


def off_by_a_word(native, table):
    """the table on the device at an address that is 8-byte but not 16-byte aligned"""
    import torch
    view = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), native.to_device(table)])[1:]
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


# ---- 2. single transforms
@pytest.mark.parametrize("n", C.SIZES)
def test_single_transforms(native, oracle, gpu, port, n):
    import torch
    items, outs = run_group(oracle, C.transforms(oracle, n))
    s = torch.cuda.current_stream()
    ctxs, tabs = {}, {}
    seen_class0 = 0
    for it, ref in zip(items, outs):
        q, psi, a, op = it.meta["q"], it.meta["psi"], it.meta["input"], it.meta["op"]
        if q not in ctxs:
            prm = oracle.Params(n, [q], [psi])
            ctxs[q] = (native.NTTContext(n, [q], [psi]), prm, native.to_device(prm.psi_tabs[0]), native.to_device(prm.psiinv_tabs[0]),
                       off_by_a_word(native, prm.psi_tabs[0]), off_by_a_word(native, prm.psiinv_tabs[0]))
            assert native.barrett_is_exact(q) == (not it.meta["inexact"]), q
        ctx, prm, d_psi, d_psiinv, l_psi, l_psiinv = ctxs[q]
        mu, k = int(prm.mu[0]), int(prm.k[0])
        d = native.to_device(a)
        getattr(ctx, op)(d)
        same(native.to_host(d), ref, (it.name, "NTTContext"))
        raw, tab, lit = (native.forwardNTT, d_psi, l_psi) if op == "forward" else (native.inverseNTT, d_psiinv, l_psiinv)
        mod, inv = native.Moduli([q], [mu], [k]), op == "inverse"
        # fast routing: the context derived from the caller's table (throughput kernels on an exact prime, the single-pass class-0
        # kernels on an inexact one), with the per-call table comparison and then on the caller's promise
        for trusted in (False, True):
            if trusted:
                assert native.raw_trust_tables(n, tab, mod, inverse=inv)
            d = native.to_device(a)
            raw(d, n, s, q, mu, k, tab)
            assert native.raw_uses_fast_kernels(n, tab, mod, inverse=inv), (it.name, trusted)
            same(native.to_host(d), ref, (it.name, "raw fast", trusted))
        # literal routing: the same table contents at an address that is not 16-byte aligned keep the call on the Algorithm-7 stage
        # kernels (include/mi355ntt.h, "Routing") -- the library's closest mirror of the reference, on exact and inexact primes alike
        assert not native.raw_uses_fast_kernels(n, lit, mod, inverse=inv), it.name
        d = native.to_device(a)
        raw(d, n, s, q, mu, k, lit)
        same(native.to_host(d), ref, (it.name, "raw literal"))
        if it.meta.get("class0") and it.meta["op"] == "forward":
            assert (ref >= np.uint64(q)).any(), it.name                  # a word no exact kernel returns
            seen_class0 += 1
    assert seen_class0 == len(C.inexact_moduli(n)) - sum(1 for q, _ in C.inexact_moduli(n) if (n, q) in C.NOT_CONSTRUCTED)
    torch.cuda.synchronize()
    for ctx, *_ in ctxs.values():
        ctx.close()
    native.raw_cache_clear()


# ---- 3. batch forms
def test_batch_forms(native, oracle, gpu, port):
    import torch
    items, outs = run_group(oracle, C.batches(oracle))
    s = torch.cuda.current_stream()
    for it, ref in zip(items, outs):
        m, op, n = it.meta, it.meta["op"], it.meta["n"]
        if op in ("forward_batch", "inverse_batch"):
            prm = oracle.Params(n, m["qs"], m["psis"])
            mod = native.Moduli(prm.q, prm.mu, prm.k)
            fwd = op == "forward_batch"
            tab = native.to_device(prm.psi_tabs if fwd else prm.psiinv_tabs)
            d = native.to_device(m["input"])
            (native.forwardNTT_batch if fwd else native.inverseNTT_batch)(d, n, tab, m["num"], m["division"], mod)
            same(native.to_host(d), ref, (it.name, "raw"))
            ctx = native.NTTContext(n, m["qs"], m["psis"])
            d = native.to_device(m["input"])
            getattr(ctx, op)(d, m["num"], m["division"])
            same(native.to_host(d), ref, (it.name, "NTTContext"))
            ctx.close()
            continue
        q, psi = m["q"], m["psi"]
        prm = oracle.Params(n, [q], [psi])
        mu, k = int(prm.mu[0]), int(prm.k[0])
        d_psi, d_psiinv = native.to_device(prm.psi_tabs[0]), native.to_device(prm.psiinv_tabs[0])
        da, db = native.to_device(m["a"]), native.to_device(m["b"])
        if op == "forward_double":
            native.forwardNTTdouble(da, db, n, s, s, q, mu, k, d_psi)
            same(np.concatenate([native.to_host(da), native.to_host(db)]), ref, it.name)
        elif op == "half_poly_mul":
            native.half_poly_mul_device(da, db, n, s, q, mu, k, d_psi, d_psiinv)
            same(native.to_host(da), ref, it.name)
        else:
            native.full_poly_mul_device(da, db, n, s, s, q, mu, k, d_psi)
            same(np.concatenate([native.to_host(da), native.to_host(db)]), ref, it.name)
    native.raw_cache_clear()


# ---- 4. pointwise and element-wise
def test_pointwise_and_elementwise(native, oracle, gpu, port):
    import torch
    items, outs = run_group(oracle, C.pointwise(oracle))
    s = torch.cuda.current_stream()
    saw_q_plus_r = False
    for it, ref in zip(items, outs):
        m, op, n = it.meta, it.meta["op"], it.meta["n"]
        if op in ("barrett_batch", "barrett_batch_3param"):
            prm = oracle.Params(n, m["qs"], [1] * len(m["qs"]), tables=False)
            mod = native.Moduli(prm.q, prm.mu, prm.k)
            da, db = native.to_device(m["a"]), native.to_device(m["b"])
            if op == "barrett_batch":
                native.barrett_batch(da, db, n, m["division"], mod, num=m["num"])
                same(native.to_host(da), ref, it.name)
            else:
                dc = torch.zeros_like(da)
                native.barrett_batch_3param(dc, da, db, n, m["division"], mod, num=m["num"])
                same(native.to_host(dc), ref, it.name)
                same(native.to_host(da), m["a"], it.name + " leaves a")
            row_q = np.array(m["qs"], dtype=np.uint64)[np.arange(m["num"]) % m["division"]][:, None]
            assert (ref.reshape(m["num"], n) >= row_q).any(), it.name
            continue
        q = m["q"]
        prm = oracle.Params(n, [q], [1], tables=False)
        mu, k = int(prm.mu[0]), int(prm.k[0])
        da, db = native.to_device(m["a"]), native.to_device(m["b"])
        if op == "barrett":
            native.barrett(da, db, q, mu, k, s)
            assert (m["noncanonical"] > 0) == (not native.barrett_is_exact(q)), q      # constructed pairs exist on every inexact prime
            if m["noncanonical"]:
                assert int((ref >= np.uint64(q)).sum()) >= m["noncanonical"], it.name  # ... and the reference leaves q + r on each
                saw_q_plus_r = True
        elif op == "barrett_int":
            native.barrett_int(da, m["scalar"], q, mu, k, s)
        elif op == "poly_add":
            native.poly_add_device(da, db, n, s, q)
            assert ref[1] == q and ref[2] == q and (ref[6:64] == np.uint64(q)).all()           # `>`: a sum equal to q stays q
        elif op == "poly_sub":
            native.poly_sub_device(da, db, n, s, q)
            assert ref[4] == 5 + q and ref[5] == 7                                               # q is added where a < b; b is never subtracted
        elif op == "poly_negate":
            native.poly_negate_device(da, n, s, q)
            assert ref[0] == 0 and (ref[64:72] == 0).all() and ref[1] == q - 1
        elif op == "poly_add_integer":
            native.poly_add_integer_device(da, m["scalar"], n, s, q)
        elif op == "poly_mul_int_t":
            native.poly_mul_int_t(da, m["scalar"], n, s, m["t"])
            assert int(ref.max()) <= ((m["t"] - 1) & 0xffffffff)                                # the reference's mask is a 32-bit `unsigned`
        else:
            raise AssertionError(op)
        same(native.to_host(da), ref, it.name)
    assert saw_q_plus_r


# ---- 5. keystream and samplers
def test_keystream_and_samplers(native, oracle, gpu, port):
    import torch
    from ntt_cuda_amd import bfv
    from test_gpu_bfv_launch_edges import check_gaussian
    binary, items, inp = C.samplers(oracle)
    items, outs = run_group(oracle, (binary, items))
    n, qs, tern, uni, gw = inp["n"], inp["qs"], inp["tern"], inp["uni"], inp["gw"]
    Rn = len(qs)
    by = {it.name: (it, out) for it, out in zip(items, outs)}
    for name, (it, ref) in by.items():
        if it.meta["op"] == "keystream":
            out = torch.full((it.meta["nbytes"],), 0xAA, dtype=torch.uint8, device=gpu)
            native.salsa20_keystream(out, it.meta["key"], 0)
            got = out.cpu().numpy()
            whole = it.meta["nbytes"] // 64 * 64
            assert np.array_equal(got[:whole], R.unpack_bytes(ref)[:whole]) and (got[whole:] == 0xAA).all(), name
    psis = [pow(P.REF_PARAMS[4096][1], 2, qs[0]),                           # a 4096-th root from the reference's 8192-th
            C.root_for(P.Q55[0], P.PSI55[0], n), C.root_for(P.EDGE_PRIMES[62][0], P.EDGE_PRIMES[62][1][32768], n)]
    assert all(pow(p, n, q) == q - 1 for p, q in zip(psis, qs))
    ctx = bfv.BFVContext(n, qs, psis, 1024, P.GAMMA61)
    z64 = lambda *shape: torch.full(shape, -1, dtype=torch.int64, device=gpu)
    rnd = np.concatenate([tern, uni.reshape(-1).view(np.uint8), gw[0].view(np.uint8)])
    rnd = np.concatenate([rnd, np.zeros(ctx.keygen_random_bytes - rnd.size, dtype=np.uint8)])
    sk, pk, tmp = z64(Rn, n), z64(2, Rn, n), z64(Rn, n)
    ctx.sample_keygen(torch.from_numpy(rnd).to(gpu), sk, pk, tmp)
    torch.cuda.synchronize()
    ref_t = by["ternary_dist_xq"][1].reshape(Rn, n)
    same(native.to_host(sk), ref_t, "ternary_dist_xq")
    assert (ref_t[:, 0] == 2).all() and (ref_t[:, 255] == np.array(qs, np.uint64) - np.uint64(1)).all()      # byte 255 gives 2, byte 0 gives q - 1
    same(native.to_host(pk)[1], by["uniform_dist_xq"][1], "uniform_dist_xq")
    ref_g = by["gaussian_dist_xq"][1].reshape(Rn, n)
    same(native.to_host(tmp), ref_g, "gaussian_dist_xq")                     # both call the device's normcdfinvf: word for word
    rnd = np.concatenate([tern, gw[1].view(np.uint8), gw[2].view(np.uint8)])
    c, e = z64(2, Rn, n), z64(2, Rn, n)
    ctx.sample_encrypt(torch.from_numpy(rnd).to(gpu), c, e)
    torch.cuda.synchronize()
    x2 = by["convert_ternary_gaussian_x2"][1]
    ref_c, ref_e = x2[:2 * Rn * n].reshape(2, Rn, n), x2[2 * Rn * n:].reshape(2, Rn, n)
    same(native.to_host(c), ref_c, "convert_ternary_gaussian_x2 c")
    same(native.to_host(e), ref_e, "convert_ternary_gaussian_x2 e")
    assert np.array_equal(ref_c[0], ref_t) and np.array_equal(ref_c[1], ref_t)
    # the oracle's AS241: every word where it differs from the reference binary is listed and goes through check_gaussian, unchanged
    for label, got, words in (("keygen", ref_g, gw[0]), ("e0", ref_e[0], gw[1]), ("e1", ref_e[1], gw[2])):
        want = oracle.sample_xq("gaussian", words.view(np.uint8), n, qs)
        differing = np.nonzero((got != want).any(axis=0))[0]
        print("gaussian %s: oracle != reference binary at" % label, [(int(i), hex(int(words[i]))) for i in differing])
        assert (got != want).mean() < 2e-3
        check_gaussian(got, want, words, qs)
    ctx.close()


# ---- 6. complete drivers
def test_complete_drivers(native, oracle, gpu, port):
    import torch
    from ntt_cuda_amd import bfv
    items, outs = run_group(oracle, C.drivers(oracle))
    gauss = C.driver_gauss_from_responses(items, outs)
    z64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=gpu)
    for it, ref in zip(items, outs):
        if it.meta["op"] != "drivers":
            continue
        n, qs, psis, t, gamma, k = (it.meta[x] for x in ("n", "qs", "psis", "t", "gamma", "constants"))
        Rn = len(qs)
        parts = dict(zip(("sk", "pk", "c_enc", "c_dec"), np.split(ref, np.cumsum([Rn * n, 2 * Rn * n, 2 * Rn * n]))))
        # oracle
        d = C.drivers_oracle(oracle, n, qs, psis, t, gamma, gauss[it.meta["set"]])
        for name in ("sk", "pk", "c_enc", "c_dec"):
            bad = np.nonzero(d[name] != parts[name])[0]
            assert bad.size == 0, ("oracle != reference binary", it.name, name, bad[:8])
        assert np.array_equal(d["plain"], d["m"])
        # library
        ctx = bfv.BFVContext(n, qs, psis, t, gamma)
        lib_k = ctx.constants()
        for name in ("inv_punctured_q", "neg_inv_q_mod_t_gamma", "prod_t_gamma_mod_q", "inv_q_last_mod_q", "qi_div_t", "base_change_matrix"):
            assert np.array_equal(lib_k[name], k[name]), name
        assert lib_k["mu_gamma"] == k["mu_gamma"]
        rnd = torch.zeros(ctx.keygen_random_bytes, dtype=torch.uint8, device=gpu)
        sk, pk, tmp = z64(Rn, n), z64(2, Rn, n), z64(Rn, n)
        ctx.keygen_rns(rnd, sk, pk, tmp, nonce=0)
        same(native.to_host(sk), parts["sk"], (it.name, "secret key"))
        same(native.to_host(pk), parts["pk"], (it.name, "public key"))
        c, e = z64(2, Rn, n), z64(2, Rn, n)
        rnd_e = torch.zeros(ctx.encrypt_random_bytes, dtype=torch.uint8, device=gpu)
        m = native.to_device(d["m"])
        ctx.encryption_rns(c, pk, rnd_e, e, m, nonce=0)
        # encryption_rns leaves the special prime's rows as its rounding step left them: compared as well, the buffer is whole
        same(native.to_host(c), parts["c_enc"], (it.name, "ciphertext"))
        got = ctx.decrypt(c, sk)
        torch.cuda.synchronize()
        same(native.to_host(c), parts["c_dec"], (it.name, "buffer after decryption"))
        assert torch.equal(got, m)
        ctx.close()


# ---- 7. the 30-bit path
@pytest.mark.parametrize("n", C.SIZES30)
def test_30bit_path(native, oracle, gpu, port, n):
    import torch
    items, outs = run_group(oracle, C.thirty(oracle, n))
    dev32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(gpu)
    host32 = lambda t_: t_.cpu().numpy().view(np.uint32)
    for it, ref in zip(items, outs):
        m, op, prm = it.meta, it.meta["op"], it.meta["prm"]
        d = dev32(m["input"])
        if op == "forward30":
            native.forward30(d, n, m["q"], prm.mu, m["bits"], dev32(prm.psi_tab), 1)
        elif op == "inverse30":
            native.inverse30(d, n, m["q"], prm.mu, m["bits"], dev32(prm.psiinv_tab), 1)
        else:
            native.barrett30(d, dev32(m["b"]), m["q"], prm.mu, m["bits"])
        torch.cuda.synchronize()
        same(host32(d), R.unpack_u32(ref), it.name)
