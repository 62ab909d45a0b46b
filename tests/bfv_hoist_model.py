"""CPU model of the BFV evaluator's hoisted Galois automorphisms (include/mi355ntt.h, "Hoisted Galois automorphisms"; DESIGN.md,
"Hoisted Galois automorphisms and their weighted sum").  Builds on GaloisModel (tests/bfv_galois_model.py) by import.  Exact integer
arithmetic, written from the definition: with D_i = [c1]_{q_i} the digits of the INPUT's c1, lifted to every q_j by plain reduction,

    H_g(c) = ( tau_g(c0) + sum_i tau_g(D_i) gk[i][0] ,  sum_i tau_g(D_i) gk[i][1] )      mod (x^n + 1, q_j)

computed as: forward-transform the r^2 digit residues once, read them through slot_permutation(n, g), multiply-accumulate with g's
key, inverse-transform.  galois_sum adds the elements' terms in the NTT domain, each multiplied by its weight (plain_ntt's output).
Ciphertexts are numpy uint64 arrays [comp][R][n] with the special slot R - 1 left 0 in the outputs."""
import numpy as np

from bfv_eval_model import _obj
from bfv_galois_model import GaloisModel, slot_permutation


class HoistModel(GaloisModel):
    def hoist(self, c):
        """what does not depend on g: Dhat[i][j] = NTT_j([c1]_{q_i} mod q_j) and c0hat[j], as integer arrays"""
        c = self.canon(c)
        Dhat = [[_obj(self.fwd(c[1, i] % np.uint64(qj), qj, wj)) for qj, wj in zip(self.qs, self.psis)] for i in range(self.r)]
        c0hat = [_obj(self.fwd(c[0, j], qj, wj)) for j, (qj, wj) in enumerate(zip(self.qs, self.psis))]
        return Dhat, c0hat

    def _term(self, hoist, gk_k, g, j):
        """NTT-domain (acc0, acc1) of H_g for prime j, not reduced"""
        Dhat, c0hat = hoist
        perm = slot_permutation(self.n, g)
        gk_k = np.asarray(gk_k, dtype=np.uint64)
        acc = [c0hat[j][perm], np.zeros(self.n, dtype=object)]
        for i in range(self.r):
            d = Dhat[i][j][perm]
            for h in range(2):
                acc[h] = acc[h] + d * _obj(gk_k[i, h, j])
        return acc

    def terms(self, c, gks, gs):
        """[k][j]: _term of element gs[k] with its key gks[k] for prime j -- what hoisted and galois_sum of the same elements share
        (pass it to them as term / terms: the r^2 wide products per element and prime are most of the model's time)"""
        hoist = self.hoist(c)
        return [[self._term(hoist, gks[k], g, j) for j in range(self.r)] for k, g in enumerate(gs)]

    def hoisted(self, c, gk_k, g, hoist=None, term=None):
        """H_g(c) with g's key gk_k [r][2][R][n]"""
        hoist = self.hoist(c) if hoist is None and term is None else hoist
        out = self._out(2)
        for j, (q, w) in enumerate(zip(self.qs, self.psis)):
            acc = self._term(hoist, gk_k, g, j) if term is None else term[j]
            for h in range(2):
                out[h, j] = self.inv((acc[h] % q).astype(np.uint64), q, w)
        return out

    def galois_sum(self, c, gks, gs, weights=None, terms=None):
        """sum_k w_k H_{gs[k]}(c); gks [G][r][2][R][n], weights [G][r][n] (plain_ntt per element) or None for every w_k = 1"""
        hoist = self.hoist(c) if terms is None else None
        out = self._out(2)
        for j, (q, w) in enumerate(zip(self.qs, self.psis)):
            tot = [np.zeros(self.n, dtype=object), np.zeros(self.n, dtype=object)]
            for k, g in enumerate(gs):
                acc = self._term(hoist, gks[k], g, j) if terms is None else terms[k][j]
                wk = 1 if weights is None else _obj(weights[k][j])
                for h in range(2):
                    tot[h] = tot[h] + acc[h] * wk
            for h in range(2):
                out[h, j] = self.inv((tot[h] % q).astype(np.uint64), q, w)
        return out

    # ---- noise bounds: G terms, each bounded as the single operation, plus the wraps of adding G messages mod t
    # (a sum of G plaintexts below t is [sum]_t + t w with 0 <= w <= G - 1, and Delta t = -rho mod Q)
    def bound_galois_sum(self, v, b_e, G):
        return G * self.bound_apply_galois(v, b_e) + (self.Q % self.t) * (G - 1)

    def bound_galois_sum_weighted(self, v, b_e, G):
        return G * self.bound_multiply_plain(self.bound_apply_galois(v, b_e)) + (self.Q % self.t) * (G - 1)
