// kernels_bfv_hoist.hip -- hoisted Galois automorphisms of the BFV evaluator (bfv_eval.hpp, DESIGN.md "Hoisted Galois automorphisms
// and their weighted sum").  The digits of the INPUT's c1 are split and forward-transformed once (k_galois_digits with g = 1 and the
// Q context's transforms); an automorphism then is a permutation of NTT slots, so every Galois element costs one permuted inner
// product with its key, not r^2 more transforms.  These kernels are that inner product -- one ciphertext batch per element
// (k_hoist_dot), or the (weighted) sum over the elements taken in the NTT domain (k_hoist_sum) -- and the hoisted form's finish.
#include "bfv_eval_arith.cuh"

namespace mi355ntt {

namespace {

// Ciphertexts per thread of the inner products.  A key word is loaded once and multiplied into this many ciphertexts' accumulators;
// the ciphertext chunk is the fastest grid dimension, so the blocks that share a key tile are dispatched back to back.
constexpr unsigned kHoistCts = 2;

// a[zt][h] += sum_i Dhat[z0 + zt][i][j][kp] key[i][h][j][k] for zt < nz (block-uniform); Dhat [count][r][r][n], key [r][2][R][n]
__device__ __forceinline__ void hoist_dot(Acc (&a)[kHoistCts][2], const u64* __restrict__ D, const u64* __restrict__ key, unsigned r,
                                          unsigned j, unsigned k, unsigned kp, unsigned n, unsigned z0, unsigned nz)
{
    const u64* kq = key + key_word(0, 0, j, k, r + 1, n);
    const u64* dq = D + digit_word(z0, 0, j, kp, r, n);
    for (unsigned i = 0; i < r; i++) {
        const u64 k0 = kq[key_word(i, 0, 0, 0, r + 1, n)], k1 = kq[key_word(i, 1, 0, 0, r + 1, n)];
#pragma unroll
        for (unsigned zt = 0; zt < kHoistCts; zt++) {
            if (zt < nz) {
                const u64 d = dq[digit_word(zt, i, 0, 0, r, n)];
                a[zt][0].mac(d, k0);
                a[zt][1].mac(d, k1);
            }
        }
    }
}

// ---- one ciphertext batch per element: P[e][h][z][j][k] = sum_i Dhat[z][i][j][k'_e] gk_e[i][h][j][k].
// grid (ceil(count / kHoistCts), n / kEvalBlock, r elems): (j, e) slowest, the ciphertext chunk fastest.
__global__ void __launch_bounds__(kEvalBlock)
k_hoist_dot(const EvConsts* __restrict__ c, u64* __restrict__ P, const u64* __restrict__ D, const u64* __restrict__ gk, HoistElems el,
            unsigned lg, unsigned n, unsigned count)
{
    const unsigned r = c->r, e = blockIdx.z / r, j = blockIdx.z % r;
    const unsigned z0 = blockIdx.x * kHoistCts, nz = min(kHoistCts, count - z0);
    const unsigned k = blockIdx.y * kEvalBlock + threadIdx.x;
    const unsigned kp = galois_slot(el.g[e], k, lg, n);
    Acc a[kHoistCts][2];
    hoist_dot(a, D, gk + key_word((size_t)e * r, 0, 0, 0, r + 1, n), r, j, k, kp, n, z0, nz);
    const EvPrime p = c->q[j];
#pragma unroll
    for (unsigned zt = 0; zt < kHoistCts; zt++) {
        if (zt < nz) {
            u64* out = P + ((((size_t)e * 2) * count + z0 + zt) * r + j) * n + k;
            out[0] = red128(a[zt][0], p);
            out[(size_t)count * r * n] = red128(a[zt][1], p);
        }
    }
}

// ---- the sum over the elements in the NTT domain: P[h][z][j][k] (+)= sum_e w_e[j][k] (sum_i Dhat[z][i][j][k'_e] gk_e[i][h][j][k]
// + [h == 0] c0hat[z][j][k'_e]).  Each element's two 128-bit sums (r products, plus one word for h = 0) are reduced once, then
// multiplied by the weight word and added to the running sum with one more reduction (w == nullptr: every weight 1, a modular add),
// so no accumulator ever holds more than r + 1 terms and P is written once per launch.  first == false continues from the P of the
// previous launch (more than kHoistSumChunk elements).  T [count][r][n] = c0hat; w [elems][r][n].
// grid (ceil(count / kHoistCts), n / kEvalBlock, r)
__global__ void __launch_bounds__(kEvalBlock)
k_hoist_sum(const EvConsts* __restrict__ c, u64* __restrict__ P, const u64* __restrict__ D, const u64* __restrict__ T,
            const u64* __restrict__ gk, const u64* __restrict__ w, HoistSumElems el, unsigned elems, bool first, unsigned lg, unsigned n,
            unsigned count)
{
    const unsigned r = c->r, j = blockIdx.z;
    const unsigned z0 = blockIdx.x * kHoistCts, nz = min(kHoistCts, count - z0);
    const unsigned k = blockIdx.y * kEvalBlock + threadIdx.x;
    const EvPrime p = c->q[j];
    u64* out = P + dense_word(0, z0, j, k, count, r, n);
    const size_t hs = (size_t)count * r * n, zs = (size_t)r * n;
    u64 s[kHoistCts][2];
#pragma unroll
    for (unsigned zt = 0; zt < kHoistCts; zt++) {
        const bool load = !first && zt < nz;
        s[zt][0] = load ? out[zt * zs] : 0;
        s[zt][1] = load ? out[hs + zt * zs] : 0;
    }
    for (unsigned e = 0; e < elems; e++) {
        const unsigned kp = galois_slot(el.g[e], k, lg, n);
        Acc a[kHoistCts][2];
#pragma unroll
        for (unsigned zt = 0; zt < kHoistCts; zt++)
            if (zt < nz) a[zt][0].add(T[poly_word(z0 + zt, j, kp, r, n)]);
        hoist_dot(a, D, gk + key_word((size_t)e * r, 0, 0, 0, r + 1, n), r, j, k, kp, n, z0, nz);
        const u64 we = w ? w[poly_word(e, j, k, r, n)] : 0;
#pragma unroll
        for (unsigned zt = 0; zt < kHoistCts; zt++) {
            if (zt < nz) {
#pragma unroll
                for (unsigned h = 0; h < 2; h++) {
                    const u64 x = red128(a[zt][h], p);
                    s[zt][h] = w ? mac_red(x, we, s[zt][h], p) : add_mod(s[zt][h], x, p.q);
                }
            }
        }
    }
#pragma unroll
    for (unsigned zt = 0; zt < kHoistCts; zt++) {
        if (zt < nz) {
            out[zt * zs] = s[zt][0];
            out[hs + zt * zs] = s[zt][1];
        }
    }
}

// ---- the hoisted form's finish: out[e] c0 = tau_g(c0) + P0, c1 = P1, into the R-strided layout.  tau_g(c0) is k_galois_digits'
// coefficient-domain gather from the input (output coefficient k reads i = g^-1 k mod 2n, negated when i >= n), fused into the add:
// the input is not staged, so out must not overlap it.  P [elems][2][count][r][n].  grid (n / kEvalBlock, elems 2 r, count)
__global__ void __launch_bounds__(kEvalBlock)
k_hoist_finish(const EvConsts* __restrict__ c, u64* __restrict__ out, const u64* __restrict__ a, const u64* __restrict__ P,
               HoistElems el, unsigned n, unsigned count)
{
    const unsigned r = c->r, e = blockIdx.y / (2 * r), h = (blockIdx.y / r) & 1, j = blockIdx.y % r, z = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const size_t ehz = ((size_t)e * 2 + h) * count + z;
    u64 x = P[(ehz * r + j) * n + k];
    if (h == 0) {
        const u64 q = c->q[j].q;
        const unsigned src = (el.ginv[e] * k) & (2 * n - 1);      // (k_galois_digits' gather, written out: see bfv_eval_arith.cuh)
        u64 v = a[((size_t)z * (r + 1) + j) * n + (src & (n - 1))];
        v = v >= q ? v - q : v;
        v = src >= n && v ? q - v : v;
        x = add_mod(x, v, q);
    }
    out[(ehz * (r + 1) + j) * n + k] = x;
}

}  // namespace

hipError_t ev_hoist_dot(const EvConsts& h, const EvConsts* d, u64* P, const u64* D, const u64* gk, const HoistElems& el, unsigned elems,
                        unsigned count, hipStream_t s)
{
    k_hoist_dot<<<dim3((count + kHoistCts - 1) / kHoistCts, h.n / kEvalBlock, h.r * elems), kEvalBlock, 0, s>>>(d, P, D, gk, el,
                                                                                                                log2_of(h.n), h.n, count);
    return hipGetLastError();
}

hipError_t ev_hoist_sum(const EvConsts& h, const EvConsts* d, u64* P, const u64* D, const u64* T, const u64* gk, const u64* w,
                        const HoistSumElems& el, unsigned elems, bool first, unsigned count, hipStream_t s)
{
    k_hoist_sum<<<dim3((count + kHoistCts - 1) / kHoistCts, h.n / kEvalBlock, h.r), kEvalBlock, 0, s>>>(d, P, D, T, gk, w, el, elems, first,
                                                                                                        log2_of(h.n), h.n, count);
    return hipGetLastError();
}

hipError_t ev_hoist_finish(const EvConsts& h, const EvConsts* d, u64* out, const u64* a, const u64* P, const HoistElems& el,
                           unsigned elems, unsigned count, hipStream_t s)
{
    k_hoist_finish<<<dim3(h.n / kEvalBlock, elems * 2 * h.r, count), kEvalBlock, 0, s>>>(d, out, a, P, el, h.n, count);
    return hipGetLastError();
}

}  // namespace mi355ntt
