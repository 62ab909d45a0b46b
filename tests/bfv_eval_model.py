"""CPU model of the BFV evaluator (include/mi355ntt.h, "BFV evaluation"; DESIGN.md, "BFV evaluation").

Exact integer arithmetic, written from the definitions rather than from the kernels' folded constants:
  - extension Q -> B_sk: BEHZ's fast conversion of [m~ x]_Q and small Montgomery reduction by m~ = 2^32, by its definition on the
    integer x (the result is x or x - Q), reduced mod every b_j;
  - tensor product: per prime, in the NTT domain;
  - rescale: d by centred CRT over Q u B_sk, y = floor(t d / Q) - alpha with alpha the overflow of the fast base conversion of
    [t d]_Q, the output y mod q_i;
  - relinearization: digits D_i = [d2]_{q_i}, sum_i D_i rlk_i in the NTT domain.
Transforms are the library's (bit-reversed forward output, inverse scaled by n^-1): the C oracle's where its Barrett is exact,
otherwise an exact numpy restatement (exact_forward / exact_inverse).  Ciphertexts are numpy uint64 arrays [comp][R][n] with the
special prime's slot R - 1 unused (left 0 in the outputs)."""
import numpy as np


def _bitrev_table(w, q, n):
    lg = n.bit_length() - 1
    pw = [1] * n
    for e in range(1, n):
        pw[e] = pw[e - 1] * w % q
    return [pw[int(format(i, "0%db" % lg)[::-1], 2)] for i in range(n)]


def exact_forward(a, q, psi):
    """negacyclic Cooley-Tukey, psi^bitrev table, bit-reversed output (the reference's forwardNTT order), exact"""
    n = len(a)
    tab = np.array(_bitrev_table(psi, q, n), dtype=object)
    x = np.array([int(v) for v in a], dtype=object)
    m, t = 1, n
    while m < n:
        t //= 2
        y = x.reshape(m, 2, t)
        S = tab[m:2 * m].reshape(m, 1)
        U, V = y[:, 0, :].copy(), (y[:, 1, :] * S) % q
        y[:, 0, :] = (U + V) % q
        y[:, 1, :] = (U - V) % q
        x = y.reshape(n)
        m *= 2
    return np.array([int(v) for v in x], dtype=np.uint64)


def exact_inverse(a, q, psi):
    """Gentleman-Sande with psi^-bitrev table and a halving per stage: natural-order output scaled by n^-1, exact"""
    n = len(a)
    tab = np.array(_bitrev_table(pow(psi, -1, q), q, n), dtype=object)
    inv2 = (q + 1) // 2
    x = np.array([int(v) for v in a], dtype=object)
    m, t = n, 1
    while m > 1:
        h = m // 2
        y = x.reshape(h, 2, t)
        S = tab[h:2 * h].reshape(h, 1)
        U, V = y[:, 0, :].copy(), y[:, 1, :].copy()
        y[:, 0, :] = (U + V) * inv2 % q
        y[:, 1, :] = (U - V) * S % q * inv2 % q
        x = y.reshape(n)
        t *= 2
        m = h
    return np.array([int(v) for v in x], dtype=np.uint64)


def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


class EvalModel:
    """qs, psis: the r primes of Q; bs, psis_b: the r + 1 primes of B_sk (m_sk last, as mi355ntt_bfv_eval_aux_primes lists them)"""

    def __init__(self, oracle, n, qs, psis, bs, psis_b, t, barrett_is_exact):
        self.n, self.t = int(n), int(t)
        self.qs, self.psis = [int(q) for q in qs], [int(p) for p in psis]
        self.bs, self.psis_b = [int(b) for b in bs], [int(p) for p in psis_b]
        self.r = len(self.qs)
        assert len(self.bs) == self.r + 1
        self.oracle = oracle
        self._exact = {q: bool(barrett_is_exact(q)) for q in self.qs + self.bs}
        self._prm = {}
        self.Q = 1
        for q in self.qs:
            self.Q *= q

    # ---- transforms, one polynomial mod q
    def _p(self, q, psi):
        if q not in self._prm:
            self._prm[q] = self.oracle.Params(self.n, [q], [psi])
        return self._prm[q]

    def fwd(self, a, q, psi):
        if self._exact[q]:
            return self.oracle.forward_batch(np.ascontiguousarray(a, dtype=np.uint64), self._p(q, psi)).reshape(self.n)
        return exact_forward(a, q, psi)

    def inv(self, a, q, psi):
        if self._exact[q]:
            return self.oracle.inverse_batch(np.ascontiguousarray(a, dtype=np.uint64), self._p(q, psi)).reshape(self.n)
        return exact_inverse(a, q, psi)

    # ---- integers of a residue vector
    def crt(self, res, mods, centred=False):
        M = 1
        for m in mods:
            M *= m
        x = np.zeros(self.n, dtype=object)
        for v, m in zip(res, mods):
            Mi = M // m
            x = x + (_obj(v) * pow(Mi % m, -1, m) % m) * Mi
        x = x % M
        if centred:
            x = np.where(x > M // 2, x - M, x)
        return x

    def canon(self, c):
        """words equal to q_i read as 0; [comp][R][n] -> [comp][r][n]"""
        c = np.asarray(c, dtype=np.uint64)
        return np.stack([np.stack([np.where(c[h, i] == np.uint64(q), np.uint64(0), c[h, i]) for i, q in enumerate(self.qs)])
                         for h in range(c.shape[0])])

    def _out(self, comps):
        return np.zeros((comps, self.r + 1, self.n), dtype=np.uint64)

    # ---- the operations, one ciphertext
    def add(self, a, b, sub=False):
        a, b = self.canon(a), self.canon(b)
        out = self._out(2)
        for h in range(2):
            for i, q in enumerate(self.qs):
                x = _obj(a[h, i]) + (-1 if sub else 1) * _obj(b[h, i])
                out[h, i] = (x % q).astype(np.uint64)
        return out

    def extend(self, x):
        """BEHZ Q -> B_sk with m~ = 2^32: the integer x~ = x + j Q, j in {-1, 0}, that the fast conversion of [m~ x]_Q followed by the
        small Montgomery reduction yields (x canonical in [0, Q))"""
        Q, mt = self.Q, 1 << 32
        X = self.crt(x, self.qs)
        mx = (X * mt) % Q
        conv = np.zeros(self.n, dtype=object)
        for q in self.qs:
            Qi = Q // q
            conv = conv + ((mx % q) * pow(Qi % q, -1, q) % q) * Qi
        rm = (-conv * pow(Q, -1, mt)) % mt
        rm = np.where(rm >= mt // 2, rm - mt, rm)
        return (conv + rm * Q) // mt

    def multiply(self, a, b):
        a, b = self.canon(a), self.canon(b)
        ops = [a[0], a[1], b[0], b[1]]
        ints = [self.extend(x) for x in ops]
        mods = self.qs + self.bs
        psis = self.psis + self.psis_b
        d = [[None] * len(mods) for _ in range(3)]
        for p, (m, w) in enumerate(zip(mods, psis)):
            hat = [self.fwd(ops[k][p] if p < self.r else (ints[k] % m).astype(np.uint64), m, w) for k in range(4)]
            A0, A1, B0, B1 = [_obj(h) for h in hat]
            for c, prod in enumerate([A0 * B0, A0 * B1 + A1 * B0, A1 * B1]):
                d[c][p] = self.inv((prod % m).astype(np.uint64), m, w)
        out = self._out(3)
        t, Q = self.t, self.Q
        for c in range(3):
            D = self.crt(d[c], mods, centred=True)                            # the integer tensor coefficient
            y = (t * D) // Q                                                  # floor (Python's // floors negatives)
            tdq = (t * D) % Q
            conv = np.zeros(self.n, dtype=object)
            for q in self.qs:
                Qi = Q // q
                conv = conv + ((tdq % q) * pow(Qi % q, -1, q) % q) * Qi
            alpha = (conv - tdq) // Q
            y = y - alpha
            for i, q in enumerate(self.qs):
                out[c, i] = (y % q).astype(np.uint64)
        return out

    def relinearize(self, c3, rlk):
        c3 = self.canon(c3)                                  # a word equal to q_i is the digit 0 in EVERY slot j, not only j = i
        rlk = np.asarray(rlk, dtype=np.uint64)
        out = self._out(2)
        for j, (qj, wj) in enumerate(zip(self.qs, self.psis)):
            acc = [np.zeros(self.n, dtype=object), np.zeros(self.n, dtype=object)]
            for i, qi in enumerate(self.qs):
                Dhat = _obj(self.fwd(c3[2, i] % np.uint64(qj), qj, wj))
                for h in range(2):
                    acc[h] = acc[h] + Dhat * _obj(rlk[i, h, j])
            for h in range(2):
                back = self.inv((acc[h] % qj).astype(np.uint64), qj, wj)
                out[h, j] = ((_obj(back) + _obj(c3[h, j])) % qj).astype(np.uint64)
        return out

    def relin_keygen(self, sk_hat, a, e):
        """sk_hat [R][n] NTT domain; a, e [r][R][n] (a: NTT-domain values, e: coefficient-domain residues)"""
        rlk = np.zeros((self.r, 2, self.r + 1, self.n), dtype=np.uint64)
        for i in range(self.r):
            for j, (q, w) in enumerate(zip(self.qs, self.psis)):
                s = _obj(sk_hat[j])
                v = -(_obj(a[i][j]) * s + _obj(self.fwd(e[i][j], q, w)))
                if i == j:
                    v = v + s * s
                rlk[i, 0, j] = (v % q).astype(np.uint64)
                rlk[i, 1, j] = a[i][j]
        return rlk

    # ---- measurement
    def noise(self, c, s_coeff, m):
        """max |v| of c0 + c1 s = Delta m + v (mod Q, centred), Delta = floor(Q / t); s_coeff: the secret as integers"""
        c = np.asarray(c, dtype=np.uint64)
        res = []
        for i, (q, w) in enumerate(zip(self.qs, self.psis)):
            s = (np.asarray(s_coeff, dtype=np.int64) % q).astype(np.uint64)
            prod = (_obj(self.fwd(c[1, i], q, w)) * _obj(self.fwd(s, q, w))) % q
            x = (_obj(self.inv(prod.astype(np.uint64), q, w)) + _obj(c[0, i])) % q
            res.append(x.astype(np.uint64))
        x = self.crt(res, self.qs)
        v = (x - (self.Q // self.t) * _obj(m)) % self.Q
        v = np.where(v > self.Q // 2, v - self.Q, v)
        return int(max(abs(int(z)) for z in v))

    def noise_bound(self, v1, v2, b_e):
        """DESIGN.md, "BFV evaluation": the noise after multiply + relinearize of inputs with noise v1, v2 (infinity norms),
        relinearization errors of norm <= b_e"""
        n, t, r = self.n, self.t, self.r
        K = n + 3
        rho = self.Q % t
        v3 = n * t * (v1 + v2) * (1 + K) + rho * n * t * (2 + 2 * K) + t * n * v1 * v2 // self.Q + 1 + (r + 1) * (1 + n + n * n)
        return v3 + r * n * max(self.qs) * b_e


def negacyclic_mod_t(m1, m2, t):
    """m1 * m2 mod (x^n + 1, t), exact integer convolution"""
    n = len(m1)
    full = np.convolve(np.asarray(m1, dtype=np.int64), np.asarray(m2, dtype=np.int64))
    out = full[:n].copy()
    out[: n - 1] -= full[n:]
    return (out % t).astype(np.uint64)
