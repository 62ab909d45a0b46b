"""The NTT sections of the reference's BFV drivers as launch sequences on an NTTContext (Python mirror of
compat/bfv_launch.hpp; same buffer layouts and num/division arguments as bfv_keygen.cuh:129-145,
bfv_encryption.cuh:268-271, bfv_decryption.cuh:98-101 of ozgunozerk/NTT-Cuda)."""


def keygen_ntt_a(ctx, secret_key, public_key, n, q_amount, stream=None):
    """bfv_keygen.cuh:129-133: sk -> NTT(sk) in place; pk0 = INTT(pk1 (.) NTT(sk)).  public_key is [2][r][n], pk1 second."""
    ctx.forward_batch(secret_key, q_amount, q_amount, stream)
    pk = public_key.reshape(-1)
    ctx.pointwise_mul(pk[: q_amount * n], pk[q_amount * n: 2 * q_amount * n], secret_key, q_amount, q_amount, stream)
    ctx.inverse_batch(pk[: q_amount * n], q_amount, q_amount, stream)


def keygen_ntt_b(ctx, public_key, q_amount, stream=None):
    """bfv_keygen.cuh:145"""
    ctx.forward_batch(public_key, q_amount, q_amount, stream)


def encryption_ntt(ctx, c, public_key, q_amount, stream=None):
    """bfv_encryption.cuh:268-271 as one fused launch"""
    ctx.polymul_batch(c, public_key, 2 * q_amount, q_amount, stream)


def decryption_ntt(ctx, c, secret_key, n, q_amount, stream=None):
    """bfv_decryption.cuh:98-101: c1 = c[(r+1) n :], num = r, division = r + 1"""
    c1 = c.reshape(-1)[(q_amount + 1) * n:]
    ctx.polymul_batch(c1, secret_key, q_amount, q_amount + 1, stream)


class BFVContext:
    """The BFV launch layer on the GPU (C ABI section "BFV" of include/mi355ntt.h): parameter bootstrap of
    demo.cu:62-272 and keygen_rns / encryption_rns / decryption_rns after their samplers.  `q`, `psi` list all primes,
    the special one (dropped by encryption) last."""

    def __init__(self, n, q, psi, t, gamma, device=0, exact_on_inexact_primes=False):
        import ctypes
        import numpy as np
        from . import lib, _check, _np_u64, u64p, vp, CTX_EXACT_ON_INEXACT_PRIMES
        self._h = vp()
        qs, ps = _np_u64(np.atleast_1d(q)), _np_u64(np.atleast_1d(psi))
        assert qs.size == ps.size
        _check(lib().mi355ntt_bfv_create(ctypes.byref(self._h), int(n), int(qs.size), qs.ctypes.data_as(u64p),
                                         ps.ctypes.data_as(u64p), int(t), int(gamma), int(device),
                                         CTX_EXACT_ON_INEXACT_PRIMES if exact_on_inexact_primes else 0), "mi355ntt_bfv_create")
        self.n, self.num_primes, self.t, self.gamma = int(n), int(qs.size), int(t), int(gamma)
        self.device = int(device)

    def _p(self, t, polys):
        """pointer of a buffer that must hold `polys` polynomials on this object's device (the C ABI takes raw pointers)"""
        from . import _ptr_n
        return _ptr_n(t, int(polys) * self.n, self.device)

    def close(self):
        from . import lib, vp
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().mi355ntt_bfv_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def uses_literal_kernels(self):
        from . import lib
        return bool(lib().mi355ntt_ctx_uses_literal_kernels(lib().mi355ntt_bfv_ntt(self._h)))

    def constants(self):
        import numpy as np
        from . import lib, _check, u64p
        r = self.num_primes - 1
        out = dict(inv_punctured_q=np.zeros(r, np.uint64), neg_inv_q_mod_t_gamma=np.zeros(2, np.uint64),
                   prod_t_gamma_mod_q=np.zeros(r, np.uint64), inv_q_last_mod_q=np.zeros(r, np.uint64),
                   qi_div_t=np.zeros(r + 1, np.uint64), base_change_matrix=np.zeros(2 * r, np.uint64), mu_gamma=np.zeros(1, np.uint64))
        _check(lib().mi355ntt_bfv_constants(self._h, *[v.ctypes.data_as(u64p) for v in out.values()]), "mi355ntt_bfv_constants")
        out["mu_gamma"] = int(out["mu_gamma"][0])
        return out

    def keygen(self, secret_key, public_key, e, stream=None):
        from . import lib, _check, _ptr, _stream
        R = self.num_primes
        _check(lib().mi355ntt_bfv_keygen(self._h, self._p(secret_key, R), self._p(public_key, 2 * R), self._p(e, R), _stream(stream)),
               "mi355ntt_bfv_keygen")

    def encrypt(self, c, public_key, e, m, stream=None):
        from . import lib, _check, _ptr, _stream
        R = self.num_primes
        _check(lib().mi355ntt_bfv_encrypt(self._h, self._p(c, 2 * R), self._p(public_key, 2 * R), self._p(e, 2 * R), self._p(m, 1),
                                          _stream(stream)), "mi355ntt_bfv_encrypt")

    def decrypt(self, c, secret_key, stream=None):
        """In place on c; returns the view of c holding the plaintext (c + n (num_primes - 2))."""
        from . import lib, _check, _ptr, _stream
        R = self.num_primes
        _check(lib().mi355ntt_bfv_decrypt(self._h, self._p(c, 2 * R), self._p(secret_key, R - 1), _stream(stream)), "mi355ntt_bfv_decrypt")
        off = self.n * (self.num_primes - 2)
        return c.reshape(-1)[off: off + self.n]

    # ---- batches of ciphertexts, layout [2][count][num_primes][n]
    def encrypt_batch(self, c, public_key, e, m, count, stream=None):
        from . import lib, _check, _stream
        R = self.num_primes
        _check(lib().mi355ntt_bfv_encrypt_batch(self._h, self._p(c, 2 * R * count), self._p(public_key, 2 * R), self._p(e, 2 * R * count),
                                                self._p(m, count), int(count), _stream(stream)), "mi355ntt_bfv_encrypt_batch")

    def decrypt_batch(self, c, secret_key, count, stream=None):
        """In place; the plaintext of ciphertext z is c.reshape(-1)[(z R + R - 2) n : ... + n]."""
        from . import lib, _check, _stream
        R = self.num_primes
        _check(lib().mi355ntt_bfv_decrypt_batch(self._h, self._p(c, 2 * R * count), self._p(secret_key, R), int(count), _stream(stream)),
               "mi355ntt_bfv_decrypt_batch")

    # ---- samplers and the complete drivers
    @property
    def keygen_random_bytes(self):
        from . import lib
        return int(lib().mi355ntt_bfv_keygen_random_bytes(self._h))

    @property
    def encrypt_random_bytes(self):
        from . import lib
        return int(lib().mi355ntt_bfv_encrypt_random_bytes(self._h))

    def sample_keygen(self, rnd, secret_key, public_key, temp, stream=None):
        from . import lib, _check, _ptr, _byte_ptr, _stream
        _check(lib().mi355ntt_bfv_sample_keygen(self._h, _byte_ptr(rnd), _ptr(secret_key), _ptr(public_key), _ptr(temp), _stream(stream)),
               "mi355ntt_bfv_sample_keygen")

    def sample_encrypt(self, rnd, c, e, stream=None):
        from . import lib, _check, _ptr, _byte_ptr, _stream
        _check(lib().mi355ntt_bfv_sample_encrypt(self._h, _byte_ptr(rnd), _ptr(c), _ptr(e), _stream(stream)), "mi355ntt_bfv_sample_encrypt")

    def keygen_rns(self, rnd, secret_key, public_key, temp, nonce=0, stream=None):
        """keygen_rns complete (bfv_keygen.cuh:95-151): keystream (reference default key) -> samplers -> key generation"""
        from . import lib, _check, _ptr, _byte_ptr, _stream
        _check(lib().mi355ntt_bfv_keygen_rns(self._h, _byte_ptr(rnd), _ptr(secret_key), _ptr(public_key), _ptr(temp), int(nonce),
                                             _stream(stream)), "mi355ntt_bfv_keygen_rns")

    def encryption_rns(self, c, public_key, rnd, e, m, nonce=0, stream=None):
        """encryption_rns complete (bfv_encryption.cuh:223-290)"""
        from . import lib, _check, _ptr, _byte_ptr, _stream
        _check(lib().mi355ntt_bfv_encryption_rns(self._h, _ptr(c), _ptr(public_key), _byte_ptr(rnd), _ptr(e), _ptr(m), int(nonce),
                                                 _stream(stream)), "mi355ntt_bfv_encryption_rns")


def aux_primes(n, r):
    """mi355ntt_bfv_aux_primes (host only): the r + 1 primes of B_sk for ring degree n, m_sk last, and a primitive 2n-th root of each"""
    import numpy as np
    from . import lib, _check, u64p
    b, psi = np.zeros(r + 1, np.uint64), np.zeros(r + 1, np.uint64)
    _check(lib().mi355ntt_bfv_aux_primes(int(n), int(r), b.ctypes.data_as(u64p), psi.ctypes.data_as(u64p)), "mi355ntt_bfv_aux_primes")
    return [int(x) for x in b], [int(x) for x in psi]


class BFVEvaluator:
    """Homomorphic evaluation on the ciphertexts of a BFVContext (C ABI section "BFV evaluation"): add, sub, multiply (BEHZ tensor
    product and t/Q rescale), relinearize and both fused; plaintext operands (add_plain, sub_plain, plain_ntt, multiply_plain,
    multiply_plain_ntt) and Galois automorphisms (galois_keygen, galois_keygen_rns, apply_galois; many elements of one ciphertext
    batch at once: apply_galois_hoisted, galois_sum).  Plaintexts are [count][n] words
    taken mod t; a galois key is [r][2][num_primes][n].  Ciphertexts are [2][count][num_primes][n] as encrypt_batch writes them
    (count = 1: [2][num_primes][n]); the product before relinearization is [3][count][num_primes][n]; the relinearization key is
    [r][2][num_primes][n], r = num_primes - 1.  Scratch is allocated per call from torch's caching allocator, on the launch stream,
    unless passed; a caller-owned scratch buffer must not be shared by calls that may run concurrently."""

    def __init__(self, bfv):
        import ctypes
        from . import lib, _check, vp
        self._h = vp()
        _check(lib().mi355ntt_bfv_eval_create(ctypes.byref(self._h), bfv._h), "mi355ntt_bfv_eval_create")
        self.bfv = bfv                      # the C object keeps a pointer to it
        self.n, self.num_primes, self.device = bfv.n, bfv.num_primes, bfv.device
        self.r = self.num_primes - 1

    def close(self):
        from . import lib, vp
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().mi355ntt_bfv_eval_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def aux_primes(self):
        import numpy as np
        from . import lib, _check, u64p
        b = np.zeros(self.r + 1, np.uint64)
        _check(lib().mi355ntt_bfv_eval_aux_primes(self._h, b.ctypes.data_as(u64p)), "mi355ntt_bfv_eval_aux_primes")
        return [int(x) for x in b]

    def scratch_bytes(self, count=1):
        from . import lib
        return int(lib().mi355ntt_bfv_eval_scratch_bytes(self._h, int(count)))

    def scratch(self, count=1):
        """a device buffer large enough for calls with `count` ciphertexts"""
        import torch
        return torch.empty(max(1, self.scratch_bytes(count) // 8), dtype=torch.int64, device="cuda:%d" % self.device)

    def _p(self, t, polys):
        from . import _ptr_n
        return _ptr_n(t, int(polys) * self.n, self.device)

    def _ct(self, count, comps=2):
        """polynomials of a ciphertext batch [comps][count][num_primes][n]"""
        return comps * count * self.num_primes

    def _keys(self, num=1):
        """polynomials of `num` relinearization or galois keys [r][2][num_primes][n]"""
        return num * 2 * self.r * self.num_primes

    def _plain(self, count):
        """polynomials of `count` plaintexts in the NTT domain, [count][r][n]"""
        return count * self.r

    @staticmethod
    def _elems(gs):
        """(the Galois elements as a C array of unsigned, their number)"""
        import ctypes
        gs = [int(g) for g in gs]
        return (ctypes.c_uint * max(1, len(gs)))(*gs), len(gs)

    def _launch(self, fn, count, scratch, stream):
        """fn(scratch pointer, stream handle).  Without `scratch` the buffer comes from torch's caching allocator ON THE LAUNCH STREAM
        and lives until the call is enqueued: freed afterwards, it returns to that stream's pool, where only work ordered after
        the call's kernels can receive it (a buffer taken on another stream could be handed out again while they still run)."""
        import torch
        from . import _stream
        polys = self.scratch_bytes(count) // 8 // self.n
        if scratch is not None:
            return fn(self._p(scratch, polys), _stream(stream))
        s = torch.cuda.current_stream() if stream is None else stream
        if isinstance(s, int):
            s = torch.cuda.ExternalStream(s, device="cuda:%d" % self.device)
        with torch.cuda.stream(s):
            buf = self.scratch(count)
        fn(self._p(buf, polys), _stream(s))
        del buf

    def relin_keygen(self, rlk, secret_key, a, e, stream=None):
        from . import lib, _check, _stream
        R, r = self.num_primes, self.r
        _check(lib().mi355ntt_bfv_relin_keygen(self._h, self._p(rlk, self._keys()), self._p(secret_key, R), self._p(a, r * R), self._p(e, r * R),
                                               _stream(stream)), "mi355ntt_bfv_relin_keygen")

    @property
    def relin_random_bytes(self):
        return self.r * self.bfv.keygen_random_bytes

    def relin_keygen_rns(self, rlk, secret_key, rnd, temp, nonce, stream=None):
        """the complete relinearization key generation; `nonce` has no default: a fresh one per key"""
        from . import lib, _check, _byte_ptr, _stream
        R = self.num_primes
        assert rnd.numel() >= self.relin_random_bytes
        _check(lib().mi355ntt_bfv_relin_keygen_rns(self._h, self._p(rlk, self._keys()), self._p(secret_key, R), _byte_ptr(rnd), self._p(temp, R),
                                                   int(nonce), _stream(stream)), "mi355ntt_bfv_relin_keygen_rns")

    def add(self, c, a, b, count=1, stream=None):
        from . import lib, _check, _stream
        w = self._ct(count)
        _check(lib().mi355ntt_bfv_add(self._h, self._p(c, w), self._p(a, w), self._p(b, w), int(count), _stream(stream)), "mi355ntt_bfv_add")

    def sub(self, c, a, b, count=1, stream=None):
        from . import lib, _check, _stream
        w = self._ct(count)
        _check(lib().mi355ntt_bfv_sub(self._h, self._p(c, w), self._p(a, w), self._p(b, w), int(count), _stream(stream)), "mi355ntt_bfv_sub")

    def multiply(self, c3, a, b, count=1, scratch=None, stream=None):
        from . import lib, _check
        args = (self._p(c3, self._ct(count, 3)), self._p(a, self._ct(count)), self._p(b, self._ct(count)), int(count))
        self._launch(lambda scr, s: _check(lib().mi355ntt_bfv_multiply(self._h, *args, scr, s), "mi355ntt_bfv_multiply"), count, scratch, stream)

    def relinearize(self, c, c3, rlk, count=1, scratch=None, stream=None):
        from . import lib, _check
        args = (self._p(c, self._ct(count)), self._p(c3, self._ct(count, 3)), self._p(rlk, self._keys()), int(count))
        self._launch(lambda scr, s: _check(lib().mi355ntt_bfv_relinearize(self._h, *args, scr, s), "mi355ntt_bfv_relinearize"), count, scratch,
                     stream)

    def multiply_relin(self, c, a, b, rlk, count=1, scratch=None, stream=None):
        from . import lib, _check
        w = self._ct(count)
        args = (self._p(c, w), self._p(a, w), self._p(b, w), self._p(rlk, self._keys()), int(count))
        self._launch(lambda scr, s: _check(lib().mi355ntt_bfv_multiply_relin(self._h, *args, scr, s), "mi355ntt_bfv_multiply_relin"), count,
                     scratch, stream)

    def add_plain(self, c, a, m, count=1, stream=None):
        """c = (c0 + E(m), c1), E(m) encryption's encoding of m"""
        from . import lib, _check, _stream
        w = self._ct(count)
        _check(lib().mi355ntt_bfv_add_plain(self._h, self._p(c, w), self._p(a, w), self._p(m, count), int(count), _stream(stream)),
               "mi355ntt_bfv_add_plain")

    def sub_plain(self, c, a, m, count=1, stream=None):
        from . import lib, _check, _stream
        w = self._ct(count)
        _check(lib().mi355ntt_bfv_sub_plain(self._h, self._p(c, w), self._p(a, w), self._p(m, count), int(count), _stream(stream)),
               "mi355ntt_bfv_sub_plain")

    def plain_ntt(self, mhat, m, count=1, stream=None):
        """mhat [count][r][n]: the centred lift of m in the NTT domain over Q, the operand of multiply_plain_ntt"""
        from . import lib, _check, _stream
        _check(lib().mi355ntt_bfv_plain_ntt(self._h, self._p(mhat, self._plain(count)), self._p(m, count), int(count), _stream(stream)),
               "mi355ntt_bfv_plain_ntt")

    def multiply_plain(self, c, a, m, count=1, scratch=None, stream=None):
        from . import lib, _check
        w = self._ct(count)
        args = (self._p(c, w), self._p(a, w), self._p(m, count), int(count))
        self._launch(lambda scr, s: _check(lib().mi355ntt_bfv_multiply_plain(self._h, *args, scr, s), "mi355ntt_bfv_multiply_plain"), count,
                     scratch, stream)

    def multiply_plain_ntt(self, c, a, mhat, count=1, shared=False, scratch=None, stream=None):
        """shared=False: mhat [count][r][n], one plaintext per ciphertext; shared=True: mhat [r][n] for the whole batch"""
        from . import lib, _check
        w = self._ct(count)
        args = (self._p(c, w), self._p(a, w), self._p(mhat, self._plain(1 if shared else count)), int(count), 1 if shared else 0)
        self._launch(lambda scr, s: _check(lib().mi355ntt_bfv_multiply_plain_ntt(self._h, *args, scr, s), "mi355ntt_bfv_multiply_plain_ntt"),
                     count, scratch, stream)

    def galois_keygen(self, gk, secret_key, g, a, e, stream=None):
        """key for Galois element g from explicit samples (as relin_keygen)"""
        from . import lib, _check, _stream
        R, r = self.num_primes, self.r
        _check(lib().mi355ntt_bfv_galois_keygen(self._h, self._p(gk, self._keys()), self._p(secret_key, R), int(g), self._p(a, r * R),
                                                self._p(e, r * R), _stream(stream)), "mi355ntt_bfv_galois_keygen")

    def galois_random_bytes(self, num_g=1):
        return int(num_g) * self.r * self.bfv.keygen_random_bytes

    def galois_keygen_rns(self, gk, secret_key, gs, rnd, temp, nonce, stream=None):
        """the complete key generation for the elements gs, gk [len(gs)][r][2][num_primes][n]; `nonce` has no default: a fresh one per
        call"""
        from . import lib, _check, _byte_ptr, _stream
        R = self.num_primes
        arr, num = self._elems(gs)
        assert rnd.numel() >= self.galois_random_bytes(num)
        _check(lib().mi355ntt_bfv_galois_keygen_rns(self._h, self._p(gk, self._keys(num)), self._p(secret_key, R), arr, num,
                                                    _byte_ptr(rnd), self._p(temp, R), int(nonce), _stream(stream)),
               "mi355ntt_bfv_galois_keygen_rns")

    def apply_galois(self, c, a, gk, g, count=1, scratch=None, stream=None):
        """c = tau_g(a) key-switched back to s with g's key gk"""
        from . import lib, _check
        w = self._ct(count)
        args = (self._p(c, w), self._p(a, w), self._p(gk, self._keys()), int(g), int(count))
        self._launch(lambda scr, s: _check(lib().mi355ntt_bfv_apply_galois(self._h, *args, scr, s), "mi355ntt_bfv_apply_galois"), count,
                     scratch, stream)

    @property
    def hoist_group(self):
        """elements per scratch group of apply_galois_hoisted (a function of r only)"""
        from . import lib
        return int(lib().mi355ntt_bfv_hoist_group(self._h))

    def apply_galois_hoisted(self, c_out, a, gk, gs, count=1, scratch=None, stream=None):
        """c_out [len(gs)][2][count][num_primes][n]: batch k = H_{gs[k]}(a), the automorphism with the digits of a's c1 split and
        transformed once for all elements; gk [len(gs)][r][2][num_primes][n] as galois_keygen_rns writes it for gs.  c_out must not
        overlap a.  Not word for word apply_galois (another valid digit decomposition); decrypts to the same plaintext."""
        from . import lib, _check
        arr, num = self._elems(gs)
        args = (self._p(c_out, num * self._ct(count)), self._p(a, self._ct(count)), self._p(gk, self._keys(num)), arr, num, int(count))
        self._launch(lambda scr, s: _check(lib().mi355ntt_bfv_apply_galois_hoisted(self._h, *args, scr, s),
                                           "mi355ntt_bfv_apply_galois_hoisted"), count, scratch, stream)

    def galois_sum(self, c, a, gk, gs, count=1, weights=None, scratch=None, stream=None):
        """c = sum_k w_k H_{gs[k]}(a), summed in the NTT domain; weights [len(gs)][r][n] from plain_ntt(count=len(gs)), shared by the
        batch, or None for every w_k = 1.  c may alias a."""
        from . import lib, _check, vp
        arr, num = self._elems(gs)
        w = vp(0) if weights is None else self._p(weights, self._plain(num))
        args = (self._p(c, self._ct(count)), self._p(a, self._ct(count)), self._p(gk, self._keys(num)), arr, num, w, int(count))
        self._launch(lambda scr, s: _check(lib().mi355ntt_bfv_galois_sum(self._h, *args, scr, s), "mi355ntt_bfv_galois_sum"), count,
                     scratch, stream)
