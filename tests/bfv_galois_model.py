"""CPU model of the BFV evaluator's plaintext operations and Galois automorphisms (include/mi355ntt.h, "BFV evaluation with plaintext
operands and Galois automorphisms"; DESIGN.md, "Plaintext operands and Galois automorphisms").  Builds on EvalModel
(tests/bfv_eval_model.py) by import.  Exact integer arithmetic, written from the definitions:
  - tau_g(x^i) = x^(g i mod 2n), an exponent >= n flipping the sign (coefficient domain);
  - the NTT-slot permutation: slot k of the library's bit-reversed forward output holds a(psi^(2 brev(k) + 1));
  - E(m) = m floor(q_i / t) + floor((m + (t + 1) / 2) / t) per prime (encryption's encoding), m taken mod t;
  - the centred lift m~ = m - t for m >= t / 2;
  - the key switch of relinearization applied to tau_g(c1) with a key for tau_g(s).
Ciphertexts are numpy uint64 arrays [comp][R][n] with the special slot R - 1 left 0 in the outputs."""
import numpy as np

from bfv_eval_model import EvalModel, _obj


def automorphism(a, g, q):
    """tau_g of one polynomial with coefficients mod q (numpy array of n words)"""
    a = np.asarray(a, dtype=np.uint64)
    n = a.size
    i = np.arange(n, dtype=np.int64)
    e = (int(g) * i) % (2 * n)
    out = np.zeros(n, dtype=np.uint64)
    x = _obj(a) % q
    val = np.where(e >= n, (-x) % q, x)
    out[e % n] = val.astype(np.uint64)
    return out


def automorphism_int(a, g):
    """tau_g of an integer polynomial (numpy int/object array)"""
    n = len(a)
    out = np.zeros(n, dtype=object)
    for i in range(n):
        e = (int(g) * i) % (2 * n)
        out[e % n] = -a[i] if e >= n else a[i]
    return out


def slot_permutation(n, g):
    """kp with tau_g(a)^[k] = a^[kp[k]] for the library's forward order: 2 brev(kp) + 1 = g (2 brev(k) + 1) mod 2n"""
    lg = n.bit_length() - 1
    brev = np.array([int(format(k, "0%db" % lg)[::-1], 2) for k in range(n)], dtype=np.int64)
    e = (int(g) * (2 * brev + 1)) % (2 * n)
    return brev[(e - 1) // 2]


class GaloisModel(EvalModel):
    def _plain(self, m):
        return np.asarray(m, dtype=np.uint64) & np.uint64(self.t - 1)

    def encode(self, m, q):
        """encryption's E(m) mod q"""
        mi = _obj(self._plain(m))
        fix = (mi + (self.t + 1) // 2) // self.t
        return ((mi * (q // self.t) + fix) % q).astype(np.uint64)

    def add_plain(self, a, m, sub=False):
        a = self.canon(a)
        out = self._out(2)
        for i, q in enumerate(self.qs):
            e = _obj(self.encode(m, q))
            out[0, i] = ((_obj(a[0, i]) + (-e if sub else e)) % q).astype(np.uint64)
            out[1, i] = a[1, i]
        return out

    def lift(self, m):
        """the centred lift m~ as integers"""
        mi = _obj(self._plain(m))
        return np.where(mi >= self.t // 2, mi - self.t, mi)

    def plain_ntt(self, m):
        """[r][n]: m~ mod q_i, forward-transformed"""
        mt = self.lift(m)
        return np.stack([self.fwd((mt % q).astype(np.uint64), q, w) for q, w in zip(self.qs, self.psis)])

    def multiply_plain_ntt(self, a, mhat):
        a = self.canon(a)
        out = self._out(2)
        for h in range(2):
            for i, (q, w) in enumerate(zip(self.qs, self.psis)):
                prod = (_obj(self.fwd(a[h, i], q, w)) * _obj(mhat[i])) % q
                out[h, i] = self.inv(prod.astype(np.uint64), q, w)
        return out

    def multiply_plain(self, a, m):
        return self.multiply_plain_ntt(a, self.plain_ntt(m))

    def galois_keygen(self, sk_hat, g, a, e):
        """as relin_keygen with tau_g(s) (a slot permutation of the NTT-domain key) in place of s^2"""
        perm = slot_permutation(self.n, g)
        gk = np.zeros((self.r, 2, self.r + 1, self.n), dtype=np.uint64)
        for i in range(self.r):
            for j, (q, w) in enumerate(zip(self.qs, self.psis)):
                s = _obj(sk_hat[j])
                v = -(_obj(a[i][j]) * s + _obj(self.fwd(e[i][j], q, w)))
                if i == j:
                    v = v + s[perm]
                gk[i, 0, j] = (v % q).astype(np.uint64)
                gk[i, 1, j] = a[i][j]
        return gk

    def apply_galois(self, c, gk, g):
        """(tau_g(c0) + P0, P1), P the key switch of tau_g(c1): EvalModel.relinearize of (tau_g(c0), 0, tau_g(c1))"""
        c = self.canon(c)
        c3 = np.zeros((3, self.r + 1, self.n), dtype=np.uint64)
        for i, q in enumerate(self.qs):
            c3[0, i] = automorphism(c[0, i], g, q)
            c3[2, i] = automorphism(c[1, i], g, q)
        return self.relinearize(c3, gk)

    # ---- noise bounds: v the input's noise (infinity norm), rho = Q mod t (1 for every accepted parameter set)
    def bound_add_plain(self, v):
        return v + 1

    def bound_multiply_plain(self, v):
        n, t = self.n, self.t
        return (n * t // 2) * v + (self.Q % t) * n * (t - 1) // 2

    def bound_apply_galois(self, v, b_e):
        return v + self.Q % self.t + self.r * self.n * max(self.qs) * b_e
