// bfv_eval.hpp -- the BFV evaluator (C ABI section "BFV evaluation" of include/mi355ntt.h): full-RNS multiplication in the
// BEHZ form (Bajard, Eynard, Hasan, Zucca, SAC 2016) and relinearization by RNS digits.  Shared between bfv_eval_host.cpp
// (constants, drivers) and kernels_bfv_eval.hip (the element-wise RNS steps; the transforms are the contexts' own calls).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mi355ntt.h"
#include "hostparams.hpp"

namespace mi355ntt {

constexpr unsigned kEvalMaxQ = 15;                 // r = |Q| <= 15: B_sk = r + 1 primes fills one context (MI355NTT_MAX_PRIMES)
constexpr unsigned kEvalMaxBsk = kEvalMaxQ + 1;
constexpr unsigned kEvalBlock = 256;               // threads per block of every evaluator kernel
constexpr unsigned kEvalMaxCount = 65535;          // ciphertexts per call: the kernels put the ciphertext index in gridDim.z
constexpr unsigned kHoistMaxGroup = 8;             // elements per inner-product launch of apply_galois_hoisted (r = 1 reaches it)
constexpr unsigned kHoistSumChunk = 16;            // elements per inner-product launch of galois_sum

// One modulus of the evaluator's element-wise arithmetic.  Every product is exact for q < 2^62, whatever the modulus (the
// Barrett-inexact ones of a literal BFV object included): x mod q for any 64-bit x by m64, 128-bit sums folded by 2^64 mod q.
struct EvPrime {
    u64 q;
    u64 m64;          // floor((2^64 - 1) / q)
    u64 r64, r64p;    // 2^64 mod q and its Shoup companion
};

// Per-evaluator constants (one device copy, read by every kernel through uniform loads).  Q = q_0 .. q_{r-1}, B = b_0 .. b_{r-1},
// m_sk = b_r, B_sk = B u {m_sk}, m~ = 2^32.
struct EvConsts {
    unsigned r = 0, n = 0;
    u64 t = 0;
    EvPrime q[kEvalMaxQ];
    EvPrime b[kEvalMaxBsk];
    // Q -> B_sk u {m~} with the small Montgomery reduction (BEHZ Algorithms 2 and 3)
    u64 ext_qc[kEvalMaxQ], ext_qcp[kEvalMaxQ];     // m~ (Q / q_i)^-1 mod q_i and Shoup companion
    u64 ext_mt[kEvalMaxQ];                         // (Q / q_i) mod 2^32
    u64 ext_neg_qinv_mt = 0;                       // -Q^-1 mod 2^32
    u64 ext_w[kEvalMaxQ][kEvalMaxBsk];             // (Q / q_i) m~^-1 mod b_j
    u64 ext_qm[kEvalMaxBsk], ext_neg_qm[kEvalMaxBsk];   // Q m~^-1 mod b_j and its negative
    // t x / Q fast floor Q u B_sk -> B_sk (BEHZ Algorithm 4 with t folded in)
    u64 rs_qc[kEvalMaxQ], rs_qcp[kEvalMaxQ];       // t (Q / q_i)^-1 mod q_i and Shoup companion
    u64 rs_w[kEvalMaxQ][kEvalMaxBsk];              // -q_i^-1 mod b_j
    u64 rs_tq[kEvalMaxBsk];                        // t Q^-1 mod b_j
    // Shenoy-Kumaresan B_sk -> Q (BEHZ Algorithm 5)
    u64 sk_bc[kEvalMaxQ], sk_bcp[kEvalMaxQ];       // (B / b_j)^-1 mod b_j and Shoup companion
    u64 sk_msk_w[kEvalMaxQ];                       // b_j^-1 mod m_sk
    u64 sk_neg_binv = 0;                           // -B^-1 mod m_sk
    u64 sk_w[kEvalMaxQ][kEvalMaxQ];                // (B / b_j) mod q_i, [j][i]
    u64 sk_bq[kEvalMaxQ], sk_neg_bq[kEvalMaxQ];    // B mod q_i and its negative
};

// ---- launchers (kernels_bfv_eval.hip).  Layouts: a ciphertext batch is [comp][count][R][n] (R = r + 1, special slot unused);
// the multiplication's scratch holds XQ [4][count][r][n] followed by XB [4][count][r + 1][n].
// a0/a1/b0/b1 of every ciphertext -> XQ (canonical copy) and XB (extension to B_sk)
hipError_t ev_extend(const EvConsts& h, const EvConsts* d, u64* xq, u64* xb, const u64* a, const u64* b, unsigned count, hipStream_t s);
// NTT domain, every prime of Q u B_sk: (a0, a1, b0, b1) -> (a0 b0, a0 b1 + a1 b0, a1 b1) in place in slots 0..2
hipError_t ev_tensor(const EvConsts& h, const EvConsts* d, u64* xq, u64* xb, unsigned count, hipStream_t s);
// coefficient domain: floor(t d / Q) in B_sk, then Shenoy-Kumaresan to Q, into c3 [3][count][R][n]
hipError_t ev_rescale(const EvConsts& h, const EvConsts* d, u64* c3, const u64* xq, const u64* xb, unsigned count, hipStream_t s);
// D [count][r][r][n]: D[z][i][j] = (d2 of ciphertext z mod q_i) mod q_j
hipError_t ev_digits(const EvConsts& h, const EvConsts* d, u64* D, const u64* c3, unsigned count, hipStream_t s);
// P [2][count][r][n]: P[h][z][j] = sum_i D[z][i][j] rlk[i][h][j] mod q_j (NTT domain)
hipError_t ev_relin_dot(const EvConsts& h, const EvConsts* d, u64* P, const u64* D, const u64* rlk, unsigned count, hipStream_t s);
// out[h][z][j] = x[h][z][j] +/- y[h][z][j] mod q_j for h < comps, j < r; inputs may hold q_j in place of 0.  Strides in words:
// per component and per ciphertext, for the output and each input.
struct EvView {
    u64* p;
    size_t comp_stride, ct_stride;
};
hipError_t ev_addsub(const EvConsts& h, const EvConsts* d, EvView out, EvView x, EvView y, unsigned comps, unsigned count, bool sub,
                     hipStream_t s);
// relin key i: slot 0 (holding NTT(e_i)) <- -(a_i s + NTT(e_i)) + [j == i] s^2, slot 1 = a_i untouched; rlk [r][2][R][n]
hipError_t ev_relin_key(const EvConsts& h, const EvConsts* d, u64* rlk, const u64* s_hat, hipStream_t s);

// ---- launchers (kernels_bfv_galois.hip): plaintext operands and Galois automorphisms.  A plaintext is [count][n] words taken mod t.
// out = a with c0 +/- E(m) (encryption's encoding m floor(q_j / t) + fix), c1 copied; canonical, out may alias a
hipError_t ev_plain_addsub(const EvConsts& h, const EvConsts* d, u64* out, const u64* a, const u64* m, unsigned count, bool sub,
                           hipStream_t s);
// mhat [count][r][n] = the centred lift of m (m >= t/2 -> m - t) mod q_j, coefficient domain
hipError_t ev_plain_lift(const EvConsts& h, const EvConsts* d, u64* mhat, const u64* m, unsigned count, hipStream_t s);
// canonical copy of the Q slots between a ciphertext batch [2][count][R][n] and dense [2][count][r][n] (to_dense) or back
hipError_t ev_plain_copy(const EvConsts& h, const EvConsts* d, u64* ct, u64* dense, unsigned count, bool to_dense, hipStream_t s);
// D [count][r][r][n] = the digits of tau_g(c1) (as ev_digits), T [count][r][n] = tau_g(c0); ginv = g^-1 mod 2n
hipError_t ev_galois_digits(const EvConsts& h, const EvConsts* d, u64* D, u64* T, const u64* a, unsigned ginv, unsigned count,
                            hipStream_t s);
// out [2][count][R][n]: c0 = T + P0, c1 = P1 (P [2][count][r][n] as ev_relin_dot writes it, after the inverse transform)
hipError_t ev_galois_finish(const EvConsts& h, const EvConsts* d, u64* out, const u64* T, const u64* P, unsigned count, hipStream_t s);
// galois key i: slot 0 (holding NTT(e_i)) <- -(a_i s + NTT(e_i)) + [j == i] tau_g(s), slot 1 = a_i untouched; gk [r][2][R][n]
hipError_t ev_galois_key(const EvConsts& h, const EvConsts* d, u64* gk, const u64* s_hat, unsigned g, hipStream_t s);

// ---- launchers (kernels_bfv_hoist.hip): hoisted Galois automorphisms.  Dhat [count][r][r][n] is ev_galois_digits' D with ginv = 1
// after the forward transform; the elements travel as kernel arguments (no device copy: the calls can be captured into a graph).
struct HoistElems {
    unsigned g[kHoistMaxGroup], ginv[kHoistMaxGroup];
};
struct HoistSumElems {
    unsigned g[kHoistSumChunk];
};
// P [elems][2][count][r][n]: P[e][h][z][j][k] = sum_i Dhat[z][i][j][k'] gk[e][i][h][j][k], k' the NTT-slot permutation of el.g[e]
hipError_t ev_hoist_dot(const EvConsts& h, const EvConsts* d, u64* P, const u64* D, const u64* gk, const HoistElems& el, unsigned elems,
                        unsigned count, hipStream_t s);
// P [2][count][r][n] = (first ? 0 : P) + sum_e w[e][j] (that inner product + [h == 0] That[z][j][k']); w [elems][r][n] or nullptr (all 1)
hipError_t ev_hoist_sum(const EvConsts& h, const EvConsts* d, u64* P, const u64* D, const u64* T, const u64* gk, const u64* w,
                        const HoistSumElems& el, unsigned elems, bool first, unsigned count, hipStream_t s);
// out [elems][2][count][R][n]: c0 = tau_g(a's c0) + P0 (gathered from a with el.ginv[e]), c1 = P1; P after the inverse transform
hipError_t ev_hoist_finish(const EvConsts& h, const EvConsts* d, u64* out, const u64* a, const u64* P, const HoistElems& el,
                           unsigned elems, unsigned count, hipStream_t s);

}  // namespace mi355ntt
