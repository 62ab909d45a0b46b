"""CPU: the crafted inputs of the key, plaintext and Galois edge sweep (tests/bfv_edge_inputs.py) reach what they were built to reach,
shown with Python integers and the model the GPU is compared with (tests/test_gpu_bfv_galois_edges.py does the comparison).
  - gather set: per Galois element, component and prime slot, each of 0, 1, q - 1, q, q - 2 lies on a coefficient tau_g negates and
    on one it does not.  Two elements cannot have both sides: tau_1 negates nothing, and tau_{2n-1} negates every coefficient but
    x^0, where one component of one slot holds one word -- there the slots and components rotate through the values;
  - peak sets: the model's unreduced NTT-domain accumulators (HoistModel._term) are (q_j - 1) + sum_i (c1_i mod q_j) (q_j - 1) in
    every slot, below 2^127; the second set's reduce to q_j - 1, and the weights are q_j - 1 in every word;
  - key set: a s + e = 0 (mod q) by both routes and the largest a s + e, in every prime slot of every key part;
  - plain set: all 64 pairs, c0 +/- E(m) on both sides of its wrap, m on both sides of the encoding's and the lift's boundaries;
  - mixed widths: the digit lift of the peak set into the 30-bit prime has a quotient of at least 2^30.
These are conditions on the inputs alone."""
import os
import re

import numpy as np
import pytest

from bfv_edge_inputs import (PLAIN_WORDS, SENT, SUM_ELEMS, constant_message, encode, five_values, galois_elements, gather_set, key_set,
                             key_values, mixed_width_set, negated, peak_set, peak_set_unit, plain_messages, plain_set, plain_words,
                             top_keys, widest_min)
from bfv_galois_model import automorphism
from bfv_hoist_model import HoistModel
from bfv_sweep_inputs import size_condition_bits, size_condition_exact
from test_bfv_eval_sweep_host import model_for

N, T = 2048, 1024
CRAFT_R = [1, 2, 4, 15]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def special_is_sentinel(x):
    x = np.asarray(x)
    return bool(np.all(x[..., -1, :] == np.uint64(SENT)))


@pytest.mark.parametrize("r", CRAFT_R)
def test_gather_set_has_every_value_on_both_sides(oracle, native, r):
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    a = gather_set(qs_all, N, 400 + r)
    assert a.shape == (2, 1, r + 1, N) and special_is_sentinel(a)
    canon = M.canon(a[:, 0])
    at_x0 = set()
    for g in galois_elements(N):
        neg = negated(N, g)
        for h in range(2):
            for i, q in enumerate(M.qs):
                w = a[h, 0, i]
                assert int(w.max()) <= q
                on_neg = [int(np.count_nonzero(w[neg] == np.uint64(v))) for v in five_values(q)]
                on_pos = [int(np.count_nonzero(w[~neg] == np.uint64(v))) for v in five_values(q)]
                if g == 1:
                    assert not neg.any() and min(on_pos) >= 1, (g, h, i, on_pos)
                elif g == 2 * N - 1:
                    assert np.array_equal(np.flatnonzero(~neg), [0]) and min(on_neg) >= 1, (g, h, i, on_neg)
                    assert sum(on_pos) == 1
                    at_x0.add(on_pos.index(1))
                else:
                    assert min(on_neg) >= 1 and min(on_pos) >= 1, (g, h, i, on_neg, on_pos)
                # what the model makes of them: 0 and q stay 0 under negation, 1 and q - 1 swap, q - 2 becomes 2
                out = automorphism(canon[h, i], g, q)
                src = np.arange(N)
                dst = (g * src) % (2 * N) % N
                for v, flipped in ((0, 0), (1, q - 1), (q - 1, 1), (q, 0), (q - 2, 2)):
                    sel = neg & (w == np.uint64(v))
                    assert np.all(out[dst[sel]] == np.uint64(flipped)), (g, h, i, v)
    assert len(at_x0) == min(5, r + 1)                 # tau_{2n-1}'s one fixed coefficient: slot i, component h hold value (i + h) mod 5


@pytest.mark.parametrize("r", CRAFT_R)
def test_peak_set_puts_every_accumulator_at_its_peak(oracle, native, r):
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    c = peak_set(qs_all, N)
    assert special_is_sentinel(c)
    lo = widest_min(M.qs)
    assert lo == min(M.qs)
    key = top_keys(qs_all, N, 1)[0]
    assert special_is_sentinel(key)
    hoist = M.hoist(c[:, 0])
    Dhat, c0hat = hoist
    w = M.plain_ntt(constant_message(N, T - 1)[0])
    for j, q in enumerate(M.qs):
        assert all(int(x) == q - 1 for x in c0hat[j]) and np.all(w[j] == np.uint64(q - 1))
        for i in range(r):
            assert all(int(x) == lo - 1 for x in Dhat[i][j])          # the relinearization's digits of this c1 as well
        peak = r * (lo - 1) * (q - 1)
        assert peak + (q - 1) < 1 << 127 and peak >= r * (lo - 1) ** 2
        for g in galois_elements(N):
            acc = M._term(hoist, key, g, j)
            assert all(int(x) == peak + (q - 1) for x in acc[0]), (g, j)
            assert all(int(x) == peak for x in acc[1]), (g, j)
    print("r=%d: accumulator peak = 2^%.3f" % (r, np.log2(float(r * (lo - 1) * (max(M.qs) - 1)))))


@pytest.mark.parametrize("r", CRAFT_R)
def test_unit_peak_set_reduces_to_q_minus_1(oracle, native, r):
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    c = peak_set_unit(qs_all, N)
    assert special_is_sentinel(c)
    key = top_keys(qs_all, N, 1)[0]
    hoist = M.hoist(c[:, 0])
    for j, q in enumerate(M.qs):
        for g in galois_elements(N):
            acc = M._term(hoist, key, g, j)
            for h in range(2):
                assert all(int(x) % q == q - 1 for x in acc[h]), (g, j, h)     # times the weight q - 1: (q - 1)^2 + s


def test_sum_has_more_elements_than_one_launch():
    text = open(os.path.join(ROOT, "ntt-cuda_amd", "csrc", "bfv_eval.hpp")).read()
    chunk = int(re.search(r"kHoistSumChunk\s*=\s*(\d+)", text).group(1))
    assert SUM_ELEMS > chunk


@pytest.mark.parametrize("r", CRAFT_R)
def test_key_set_reaches_zero_and_the_maximum(oracle, native, r):
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    seen = {}
    for shift in range(3):
        sk, a, e = key_set(qs_all, N, shift)
        assert special_is_sentinel(sk[None]) and special_is_sentinel(a) and special_is_sentinel(e)
        for i in range(r):
            for j, (q, w) in enumerate(zip(M.qs, M.psis)):
                ehat = M.fwd(e[i, j], q, w)
                assert np.all(ehat == ehat[0]) and int(ehat[0]) in key_values(q)           # a constant: the transform of c x^0
                pairs = {(int(x), int(y)) for x, y in zip(a[i, j], sk[j])}
                assert pairs == {(x, y) for x in key_values(q) for y in key_values(q)}, (shift, i, j)
                seen.setdefault((i, j), set()).update((x, y, int(ehat[0])) for x, y in pairs)
    for (i, j), triples in seen.items():
        q = M.qs[j]
        assert len(triples) == 27                                                           # every (a, s, e) of the three values
        v = {x * y + c for x, y, c in triples}
        assert 0 in v and q in v and max(v) == (q - 1) ** 2 + (q - 1)
        assert (0, q - 1, 0) in triples and (1, q - 1, 1) in triples and (q - 1, q - 1, q - 1) in triples


@pytest.mark.parametrize("r", CRAFT_R)
def test_plain_set_crosses_every_wrap(oracle, native, r):
    qs_all, _, M = model_for(oracle, native, N, r, T, wide=True)
    a, m = plain_set(qs_all, N, T, 500 + r)
    assert special_is_sentinel(a) and m.shape == (1, N)
    ms = plain_messages(T)
    assert ms[-1] == (1 << 64) - 1 and {x % T for x in ms} == {0, 1, T // 2 - 1, T // 2, T - 1, 3}
    for j, q in enumerate(M.qs):
        enc = M.encode(m[0], q)
        for base in (0, N - 64):
            sums, diffs = set(), set()
            for w in range(len(PLAIN_WORDS)):
                for u, mu in enumerate(ms):
                    k = base + 8 * w + u
                    E = encode(mu, q, T)
                    assert int(m[0, k]) == mu and int(enc[k]) == E                          # the model's encoding is the definition
                    assert int(a[0, 0, j, k]) == plain_words(mu, q, T)[w] <= q
                    x = int(a[0, 0, j, k]) % q
                    sums.add(x + E - q)
                    diffs.add(x - E)
            assert {-1, 0, 1} <= sums and {-1, 0, 1} <= diffs, (j, base)                    # both sides of add_mod's and sub_mod's wrap
        fix = {(mu % T + (T + 1) // 2) // T for mu in ms}
        assert fix == {0, 1}
    lift = M.lift(np.array(ms, dtype=np.uint64))
    assert [int(x) for x in lift] == [0, 1, T // 2 - 1, -(T // 2), -1, 0, 3, -1]


@pytest.mark.parametrize("small_at", [0, 2])
def test_mixed_width_lift_has_a_large_quotient(oracle, native, small_at):
    from ntt_cuda_amd import bfv
    qs, psis = mixed_width_set(N, T, native.barrett_is_exact, small_at)
    r = len(qs) - 1
    assert r == 3 and len(set(qs)) == 4
    small = qs[small_at]
    assert small.bit_length() == 30 and all(q.bit_length() == 61 for k, q in enumerate(qs) if k != small_at)
    assert all(q % (2 * N) == 1 and q % T == 1 and native.barrett_is_exact(q) for q in qs)
    bs, psis_b = bfv.aux_primes(N, r)
    assert not set(bs) & set(qs) and size_condition_bits(N, T, qs[:r], bs) and size_condition_exact(N, T, qs[:r], bs)
    M = HoistModel(oracle, N, qs[:r], psis[:r], bs, psis_b, T, native.barrett_is_exact)
    c = peak_set(qs, N)
    lo = widest_min(qs[:r])
    assert lo > small
    Dhat, _ = M.hoist(c[:, 0])
    for i, q in enumerate(qs[:r]):
        digit = int(c[1, 0, i, 0])
        assert digit == (small - 1 if i == small_at else lo - 1)
        if i != small_at:
            assert digit // small >= 1 << 30                                                 # red64's quotient in the small prime
            assert all(int(x) == digit % small for x in Dhat[i][small_at])
