// bfv_eval_arith.cuh -- what the BFV evaluator's kernel files (kernels_bfv_eval.hip, kernels_bfv_galois.hip, kernels_bfv_hoist.hip)
// share: the 64- and 128-bit reductions on an EvPrime, the word index of the dense, digit and key layouts and the NTT-slot
// permutation of a Galois element.  A kernel may use a helper only where it compiles to the same instructions as with the helper
// written out (tools/codeobj_digest.py --diff): the compiler inlines these after it has simplified the calling kernel, and the
// instruction order of several kernels moves with that.  Tried and left written out for that reason:
//   the word index helpers in k_extend<7, 10, 11>, k_rescale<every r>, k_digits, k_relin_dot, k_relin_key, k_plain_addsub,
//     k_plain_copy, k_galois_digits, k_galois_finish, k_galois_key, k_hoist_finish and k_hoist_dot's output (so there is no helper
//     for the R-strided ciphertext word: no kernel could use it);
//   the digit spread as a function: k_digits, k_galois_digits (the loop's exit test flips);
//   the coefficient gather as a function: k_galois_digits, k_hoist_finish;
//   -(a s + e) as a function: k_relin_key, k_galois_key; mac_red itself in k_relin_key.
#pragma once
#include "bfv_eval.hpp"
#include "modarith.cuh"

namespace mi355ntt {

// log2 of a power of two n (host side: launch arguments and the evaluator's size condition)
inline unsigned log2_of(unsigned n)
{
    unsigned lg = 0;
    while ((1u << lg) < n) lg++;
    return lg;
}

// ---- arithmetic ----

// x mod q for any 64-bit x: the estimate floor(x m64 / 2^64) is the quotient or up to two less (kernels_bfv.hip, reduce64)
__device__ __forceinline__ u64 red64(u64 x, const EvPrime& p)
{
    u64 r = x - mul_hi(x, p.m64) * p.q;
    r = r >= p.q ? r - p.q : r;
    return r >= p.q ? r - p.q : r;
}

// 128-bit accumulator.  Every sum here has at most r + 2 <= 17 terms, each a product of two words below 2^61: < 2^127.
struct Acc {
    u64 lo = 0, hi = 0;
    __device__ __forceinline__ void mac(u64 a, u64 b)
    {
        u64 l, h;
        mul_wide(a, b, l, h);
        lo += l;
        hi += h + (lo < l);
    }
    __device__ __forceinline__ void add(u64 a)
    {
        lo += a;
        hi += (lo < a);
    }
};

// {hi, lo} mod q: hi 2^64 by the Shoup product with 2^64 mod q (any 64-bit hi, result below 2q), lo by red64; sum below 3q < 2^64
__device__ __forceinline__ u64 red128(const Acc& a, const EvPrime& p)
{
    u64 s = shoup_mul_lazy(a.hi, p.r64, p.r64p, p.q) + red64(a.lo, p);
    s = s >= p.q ? s - p.q : s;
    return s >= p.q ? s - p.q : s;
}

// x w mod q for a constant w < q with Shoup companion wp; any 64-bit x
__device__ __forceinline__ u64 mulc(u64 x, u64 w, u64 wp, u64 q) { return csub(shoup_mul_lazy(x, w, wp, q), q); }

// a b + c mod q; a, b < 2^62, c < 2^64
__device__ __forceinline__ u64 mac_red(u64 a, u64 b, u64 c, const EvPrime& p)
{
    Acc s;
    s.mac(a, b);
    s.add(c);
    return red128(s, p);
}

// ---- layouts: the index of word k of prime j.  r = |Q|.  Every
// argument is widened by the caller, where the compiler merges the widening with the caller's other uses of the same value. ----

// the dense form [comp][count][r][n] of scratch buffers (with r + 1 for r: the B_sk side of the multiplication, and a ciphertext
// batch [comp][count][R][n], whose special slot is unused)
__device__ __forceinline__ size_t dense_word(size_t comp, size_t z, size_t j, size_t k, size_t count, size_t r, size_t n)
{
    return ((comp * count + z) * r + j) * n + k;
}

// polynomials by ciphertext or element, [count][r][n]: lifted plaintexts, weights, a staged c0
__device__ __forceinline__ size_t poly_word(size_t z, size_t j, size_t k, size_t r, size_t n) { return (z * r + j) * n + k; }

// the digits [count][r (i)][r (j)][n]: digit i of ciphertext z
__device__ __forceinline__ size_t digit_word(size_t z, size_t i, size_t j, size_t k, size_t r, size_t n)
{
    return ((z * r + i) * r + j) * n + k;
}

// a key [r (i)][2 (h)][R][n]; key e of a key set begins at part i = e r
__device__ __forceinline__ size_t key_word(size_t i, size_t h, size_t j, size_t k, size_t R, size_t n)
{
    return ((i * 2 + h) * R + j) * n + k;
}

// ---- Galois automorphism tau_g(x^i) = x^(g i mod 2n) ----

// NTT domain.  Slot k of the bit-reversed forward output holds x(psi^(2 brev(k) + 1)), so tau_g(x)'s slot k is x's slot k' with
// 2 brev(k') + 1 = g (2 brev(k) + 1) mod 2n: a permutation, no transform.  The low bits of k are the high bits of brev(k), and
// u -> g u + (g - 1) / 2 mod n keeps low bits among low bits: every aligned block of 2^b consecutive k maps onto one aligned block
// of 2^b slots, permuted inside it.  A workgroup's 256 gathered words are the 2 KiB it would read without the permutation.
__device__ __forceinline__ unsigned galois_slot(unsigned g, unsigned k, unsigned lg, unsigned n)
{
    const unsigned e = (g * (2 * (__brev(k) >> (32 - lg)) + 1)) & (2 * n - 1);
    return __brev((e - 1) >> 1) >> (32 - lg);
}

}  // namespace mi355ntt
