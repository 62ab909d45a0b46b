// kernels_bfv_galois.hip -- element-wise steps of the BFV evaluator's plaintext operations and Galois automorphisms (bfv_eval.hpp,
// DESIGN.md "Plaintext operands and Galois automorphisms").  The transforms, the fused products and the key-switch inner product are
// the contexts' calls and kernels_bfv_eval.hip's k_relin_dot; these kernels do the plaintext encoding and lift, the canonical copies
// around the fused products, the coefficient automorphism fused into the digit split, and the galois key's NTT-slot permutation.
#include "bfv_eval_arith.cuh"

namespace mi355ntt {

namespace {

// ---- c0 +/- E(m), c1 copied, every output canonical.  E(m) is encryption's encoding (k_encrypt_tail, the reference's weird_m_stuff):
// m floor(q_j / t) + fix with fix = floor((m + (t + 1) / 2) / t), m taken mod t (a mask: t is a power of two).
// grid (n / kEvalBlock, 2 r (component-major), count)
__global__ void __launch_bounds__(kEvalBlock)
k_plain_addsub(const EvConsts* __restrict__ c, u64* out, const u64* a, const u64* __restrict__ m, unsigned n, unsigned count, bool sub)
{
    const unsigned r = c->r, h = blockIdx.y / r, j = blockIdx.y % r, z = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const size_t at = (((size_t)h * count + z) * (r + 1) + j) * n + k;
    const u64 q = c->q[j].q, t = c->t;
    u64 x = a[at];
    x = x >= q ? x - q : x;
    if (h == 0) {
        const u64 mi = m[(size_t)z * n + k] & (t - 1);
        const u64 fix = mi + ((t + 1) >> 1) >= t ? 1 : 0;
        const u64 e = mi * (q / t) + fix;                      // < q: m <= t - 1
        x = sub ? sub_mod(x, e, q) : add_mod(x, e, q);
    }
    out[at] = x;
}

// ---- centred lift m~ (m >= t/2 -> m - t) of m mod t as residues: mhat [count][r][n].  grid (n / kEvalBlock, r, count)
__global__ void __launch_bounds__(kEvalBlock)
k_plain_lift(const EvConsts* __restrict__ c, u64* __restrict__ mhat, const u64* __restrict__ m, unsigned n)
{
    const unsigned r = c->r, j = blockIdx.y, z = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const u64 q = c->q[j].q, t = c->t;
    const u64 mi = m[(size_t)z * n + k] & (t - 1);
    mhat[poly_word(z, j, k, r, n)] = mi >= (t >> 1) && mi ? q - (t - mi) : mi;
}

// ---- canonical copy between the R-strided ciphertext layout [2][count][R][n] and the dense [2][count][r][n]: to_dense reads the
// ciphertext (a word equal to q_j reads as 0), otherwise the dense buffer is written back.  grid (n / kEvalBlock, 2 r, count)
__global__ void __launch_bounds__(kEvalBlock)
k_plain_copy(const EvConsts* __restrict__ c, u64* ct, u64* dense, unsigned n, unsigned count, bool to_dense)
{
    const unsigned r = c->r, h = blockIdx.y / r, j = blockIdx.y % r, z = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const size_t hz = (size_t)h * count + z;
    u64* pc = ct + (hz * (r + 1) + j) * n + k;
    u64* pd = dense + (hz * r + j) * n + k;
    if (to_dense) {
        const u64 q = c->q[j].q, x = *pc;
        *pd = x >= q ? x - q : x;
    } else {
        *pc = *pd;
    }
}

// ---- coefficient automorphism tau_g(x^i) = x^(g i mod 2n), an exponent >= n flipping the sign, as a gather: output coefficient k
// reads input coefficient i = g^-1 k mod 2n (negated when i >= n, coefficient i - n).  The strided side is the read (one word per
// output, against r digit words written per c1 word), so every write is coalesced.
//   c1 polynomial (z, i): D[z][i][j] = (tau_g(c1_i) mod q_i) mod q_j, the digit split of k_digits with the permutation fused in;
//   c0 polynomial (z, i): T[z][i] = tau_g(c0_i), canonical (staged so that the output may alias the input).
// The gather reads one 256 KiB polynomial (n = 2^15) in a scattered order: every workgroup of a polynomial should hit the same XCD's
// L2.  Workgroups are dealt round-robin over the 8 XCDs (observed, not promised: speed only), so blocks b and b + 8 share one; the
// grid is (8 * chunks, ceil(2 r / 8), count) and block x serves polynomial 8 y + x % 8 (c1 first, then c0), chunk x / 8: the
// chunks of one polynomial have equal linear block ids mod 8.  Slots past 2 r in the last group exit at once.
__global__ void __launch_bounds__(kEvalBlock)
k_galois_digits(const EvConsts* __restrict__ c, u64* __restrict__ D, u64* __restrict__ T, const u64* __restrict__ a, unsigned ginv,
                unsigned n, unsigned count)
{
    const unsigned r = c->r, z = blockIdx.z;
    const unsigned p = blockIdx.y * 8 + blockIdx.x % 8;
    if (p >= 2 * r) return;
    const bool c1 = p < r;
    const unsigned i = c1 ? p : p - r;
    const unsigned k = (blockIdx.x / 8) * kEvalBlock + threadIdx.x;
    // (k_hoist_finish has this gather too, both written out: see bfv_eval_arith.cuh)
    const unsigned src = (ginv * k) & (2 * n - 1);              // ginv k mod 2n: 2n divides 2^32, the wrap is harmless
    const u64 qi = c->q[i].q;
    u64 x = a[(((size_t)(c1 ? count : 0) + z) * (r + 1) + i) * n + (src & (n - 1))];
    x = x >= qi ? x - qi : x;
    x = src >= n && x ? qi - x : x;
    if (!c1) {
        T[((size_t)z * r + i) * n + k] = x;
        return;
    }
    u64* d = D + ((size_t)z * r + i) * r * n + k;              // (k_digits' loop, written out: see bfv_eval_arith.cuh)
    for (unsigned j = 0; j < r; j++) d[(size_t)j * n] = j == i ? x : red64(x, c->q[j]);
}

// ---- key-switch result: out c0 = T + P0 (T: the staged tau_g(c0)), c1 = P1; P [2][count][r][n].  grid (n / kEvalBlock, 2 r, count)
__global__ void __launch_bounds__(kEvalBlock)
k_galois_finish(const EvConsts* __restrict__ c, u64* __restrict__ out, const u64* __restrict__ T, const u64* __restrict__ P, unsigned n,
                unsigned count)
{
    const unsigned r = c->r, h = blockIdx.y / r, j = blockIdx.y % r, z = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const size_t dz = ((size_t)z * r + j) * n + k;
    u64 x = P[(size_t)h * count * r * n + dz];
    if (h == 0) x = add_mod(x, T[dz], c->q[j].q);
    out[(((size_t)h * count + z) * (r + 1) + j) * n + k] = x;
}

// ---- galois key i, prime j: -(a s + e) + [i == j] tau_g(s) in the NTT domain; gk [r][2][R][n], slot 0 holding NTT(e_i).  tau_g(s) is
// a permutation of s_hat's slots (galois_slot), no transform.  grid (n / kEvalBlock, r (j), r (i))
__global__ void __launch_bounds__(kEvalBlock)
k_galois_key(const EvConsts* __restrict__ c, u64* __restrict__ gk, const u64* __restrict__ s_hat, unsigned g, unsigned lg, unsigned n)
{
    const unsigned r = c->r, j = blockIdx.y, i = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const size_t R = r + 1;
    const EvPrime p = c->q[j];
    u64* k0 = gk + ((size_t)i * 2 * R + j) * n + k;
    const u64 a = k0[R * n], s = s_hat[(size_t)j * n + k];
    u64 v = mac_red(a, s, k0[0], p);                    // (-(a s + e) as k_relin_key has it, written out: see bfv_eval_arith.cuh)
    v = v ? p.q - v : 0;
    if (i == j) v = add_mod(v, s_hat[(size_t)j * n + galois_slot(g, k, lg, n)], p.q);
    k0[0] = v;
}

}  // namespace

hipError_t ev_plain_addsub(const EvConsts& h, const EvConsts* d, u64* out, const u64* a, const u64* m, unsigned count, bool sub,
                           hipStream_t s)
{
    k_plain_addsub<<<dim3(h.n / kEvalBlock, 2 * h.r, count), kEvalBlock, 0, s>>>(d, out, a, m, h.n, count, sub);
    return hipGetLastError();
}

hipError_t ev_plain_lift(const EvConsts& h, const EvConsts* d, u64* mhat, const u64* m, unsigned count, hipStream_t s)
{
    k_plain_lift<<<dim3(h.n / kEvalBlock, h.r, count), kEvalBlock, 0, s>>>(d, mhat, m, h.n);
    return hipGetLastError();
}

hipError_t ev_plain_copy(const EvConsts& h, const EvConsts* d, u64* ct, u64* dense, unsigned count, bool to_dense, hipStream_t s)
{
    k_plain_copy<<<dim3(h.n / kEvalBlock, 2 * h.r, count), kEvalBlock, 0, s>>>(d, ct, dense, h.n, count, to_dense);
    return hipGetLastError();
}

hipError_t ev_galois_digits(const EvConsts& h, const EvConsts* d, u64* D, u64* T, const u64* a, unsigned ginv, unsigned count,
                            hipStream_t s)
{
    k_galois_digits<<<dim3(8 * (h.n / kEvalBlock), (2 * h.r + 7) / 8, count), kEvalBlock, 0, s>>>(d, D, T, a, ginv, h.n, count);
    return hipGetLastError();
}

hipError_t ev_galois_finish(const EvConsts& h, const EvConsts* d, u64* out, const u64* T, const u64* P, unsigned count, hipStream_t s)
{
    k_galois_finish<<<dim3(h.n / kEvalBlock, 2 * h.r, count), kEvalBlock, 0, s>>>(d, out, T, P, h.n, count);
    return hipGetLastError();
}

hipError_t ev_galois_key(const EvConsts& h, const EvConsts* d, u64* gk, const u64* s_hat, unsigned g, hipStream_t s)
{
    k_galois_key<<<dim3(h.n / kEvalBlock, h.r, h.r), kEvalBlock, 0, s>>>(d, gk, s_hat, g, log2_of(h.n), h.n);
    return hipGetLastError();
}

}  // namespace mi355ntt
