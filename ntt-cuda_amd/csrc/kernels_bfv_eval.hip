// kernels_bfv_eval.hip -- element-wise RNS steps of the BFV evaluator (bfv_eval.hpp).  The transforms between them are the contexts'
// own batched calls; these kernels do the base conversions, the tensor product, the rescale, the digit spread and the
// relinearization inner product.  They are bound by 64-bit multiplies, not by memory: every per-coefficient inner product is
// summed in 128 bits and reduced once per output word.  The column kernels (extension, rescale) are instantiated per r = |Q| so that
// their per-coefficient residue vectors live in registers.
#include <utility>

#include "bfv_eval_arith.cuh"

namespace mi355ntt {

namespace {

// ---- Q -> B_sk with m~ = 2^32 (BEHZ Algorithms 2 + 3).  tmp_i = [x_i m~ (Q/q_i)^-1]_{q_i}; sum_i tmp_i (Q/q_i) = [m~ x]_Q + alpha Q,
// 0 <= alpha < r.  r_m = -(that) Q^-1 mod m~, centred, makes the sum plus r_m Q divisible by m~; the quotient is x or x - Q (|.| < Q),
// congruent to x mod Q, in every b_j.
// grid (n / kEvalBlock, 4, count): component a0, a1, b0, b1 of ciphertext z.
template <unsigned RQ>
__global__ void __launch_bounds__(kEvalBlock)
k_extend(const EvConsts* __restrict__ c, u64* __restrict__ xq, u64* __restrict__ xb, const u64* __restrict__ a,
         const u64* __restrict__ b, unsigned n, unsigned count)
{
    constexpr unsigned R = RQ + 1;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const unsigned comp = blockIdx.y, z = blockIdx.z;
    const u64* src = (comp < 2 ? a : b) + ((size_t)(comp & 1) * count + z) * R * n + k;
    u64* dq = xq + ((size_t)comp * count + z) * RQ * n + k;
    u64* db = xb + ((size_t)comp * count + z) * (RQ + 1) * n + k;
    u64 tmp[RQ];
    u64 ymt = 0;
#pragma unroll
    for (unsigned i = 0; i < RQ; i++) {
        const u64 q = c->q[i].q;
        u64 x = src[(size_t)i * n];
        x = x >= q ? x - q : x;                        // a word equal to q stands for 0
        dq[(size_t)i * n] = x;
        tmp[i] = mulc(x, c->ext_qc[i], c->ext_qcp[i], q);
        ymt += tmp[i] * c->ext_mt[i];                  // mod 2^64, of which mod 2^32 is used
    }
    const unsigned rm = (unsigned)(ymt * c->ext_neg_qinv_mt);
    const bool neg = rm >= 0x80000000u;
    const u64 mag = neg ? (u64)(0u - rm) : (u64)rm;
#pragma unroll
    for (unsigned j = 0; j <= RQ; j++) {
        Acc acc;
#pragma unroll
        for (unsigned i = 0; i < RQ; i++) acc.mac(tmp[i], c->ext_w[i][j]);
        acc.mac(mag, neg ? c->ext_neg_qm[j] : c->ext_qm[j]);
        db[(size_t)j * n] = red128(acc, c->b[j]);
    }
}

// ---- NTT-domain tensor product on every prime of Q u B_sk: slots (a0, a1, b0, b1) -> (a0 b0, a0 b1 + a1 b0, a1 b1).
// grid (n / kEvalBlock, 2 r + 1, count): prime p < r is q_p (XQ), p >= r is b_{p - r} (XB).
__global__ void __launch_bounds__(kEvalBlock)
k_tensor(const EvConsts* __restrict__ c, u64* __restrict__ xq, u64* __restrict__ xb, unsigned n, unsigned count)
{
    const unsigned r = c->r, p = blockIdx.y, z = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const bool inq = p < r;
    const unsigned np = inq ? r : r + 1, slot = inq ? p : p - r;
    const EvPrime pr = inq ? c->q[slot] : c->b[slot];
    u64* base = (inq ? xq : xb) + dense_word(0, z, slot, k, count, np, n);
    const size_t cs = (size_t)count * np * n;
    const u64 a0 = base[0], a1 = base[cs], b0 = base[2 * cs], b1 = base[3 * cs];
    Acc d0, d1, d2;
    d0.mac(a0, b0);
    d1.mac(a0, b1);
    d1.mac(a1, b0);
    d2.mac(a1, b1);
    base[0] = red128(d0, pr);
    base[cs] = red128(d1, pr);
    base[2 * cs] = red128(d2, pr);
}

// ---- coefficient domain: y = floor(t d / Q) - alpha in B_sk (BEHZ Algorithm 4, t folded into the constants), then
// Shenoy-Kumaresan B_sk -> Q (Algorithm 5): alpha_sk = (conv_B(y) - y) B^-1 mod m_sk, centred, out_i = conv_B(y)_i - alpha_sk B.
// grid (n / kEvalBlock, 3, count): component d0, d1, d2 of ciphertext z into c3 [3][count][R][n].
template <unsigned RQ>
__global__ void __launch_bounds__(kEvalBlock)
k_rescale(const EvConsts* __restrict__ c, u64* __restrict__ c3, const u64* __restrict__ xq, const u64* __restrict__ xb, unsigned n,
          unsigned count)
{
    constexpr unsigned R = RQ + 1;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const unsigned comp = blockIdx.y, z = blockIdx.z;
    const u64* sq = xq + ((size_t)comp * count + z) * RQ * n + k;
    const u64* sb = xb + ((size_t)comp * count + z) * (RQ + 1) * n + k;
    u64* out = c3 + ((size_t)comp * count + z) * R * n + k;
    u64 tmp[RQ];
#pragma unroll
    for (unsigned i = 0; i < RQ; i++) tmp[i] = mulc(sq[(size_t)i * n], c->rs_qc[i], c->rs_qcp[i], c->q[i].q);
    u64 y[RQ + 1];
#pragma unroll
    for (unsigned j = 0; j <= RQ; j++) {
        Acc acc;
        acc.mac(sb[(size_t)j * n], c->rs_tq[j]);
#pragma unroll
        for (unsigned i = 0; i < RQ; i++) acc.mac(tmp[i], c->rs_w[i][j]);
        y[j] = red128(acc, c->b[j]);
    }
    u64 tb[RQ];
    Acc am;
    am.mac(y[RQ], c->sk_neg_binv);
#pragma unroll
    for (unsigned j = 0; j < RQ; j++) {
        tb[j] = mulc(y[j], c->sk_bc[j], c->sk_bcp[j], c->b[j].q);
        am.mac(tb[j], c->sk_msk_w[j]);
    }
    const u64 msk = c->b[RQ].q;
    const u64 al = red128(am, c->b[RQ]);
    const bool neg = al > (msk >> 1);
    const u64 mag = neg ? msk - al : al;
#pragma unroll
    for (unsigned i = 0; i < RQ; i++) {
        Acc acc;
#pragma unroll
        for (unsigned j = 0; j < RQ; j++) acc.mac(tb[j], c->sk_w[j][i]);
        acc.mac(mag, neg ? c->sk_bq[i] : c->sk_neg_bq[i]);
        out[(size_t)i * n] = red128(acc, c->q[i]);
    }
}

// ---- D[z][i][j] = (d2 mod q_i) mod q_j; a word equal to q_i is the digit 0.  grid (n / kEvalBlock, r (i), count)
__global__ void __launch_bounds__(kEvalBlock)
k_digits(const EvConsts* __restrict__ c, u64* __restrict__ D, const u64* __restrict__ c3, unsigned n, unsigned count)
{
    const unsigned r = c->r, i = blockIdx.y, z = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const u64 qi = c->q[i].q;
    u64 x = c3[((size_t)2 * count + z) * (r + 1) * n + (size_t)i * n + k];
    x = x >= qi ? x - qi : x;
    u64* d = D + ((size_t)z * r + i) * r * n + k;              // (k_galois_digits has this loop too: see bfv_eval_arith.cuh)
    for (unsigned j = 0; j < r; j++) d[(size_t)j * n] = j == i ? x : red64(x, c->q[j]);
}

// ---- P[h][z][j] = sum_i D[z][i][j] rlk[i][h][j], one reduction per word.  grid (n / kEvalBlock, r (j), count)
__global__ void __launch_bounds__(kEvalBlock)
k_relin_dot(const EvConsts* __restrict__ c, u64* __restrict__ P, const u64* __restrict__ D, const u64* __restrict__ rlk, unsigned n,
            unsigned count)
{
    const unsigned r = c->r, j = blockIdx.y, z = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const size_t R = r + 1;
    Acc a0, a1;
    for (unsigned i = 0; i < r; i++) {
        const u64 d = D[(((size_t)z * r + i) * r + j) * n + k];
        a0.mac(d, rlk[((size_t)i * 2 * R + j) * n + k]);
        a1.mac(d, rlk[((size_t)i * 2 * R + R + j) * n + k]);
    }
    const EvPrime p = c->q[j];
    P[((size_t)z * r + j) * n + k] = red128(a0, p);
    P[(((size_t)count + z) * r + j) * n + k] = red128(a1, p);
}

// ---- out = x +/- y on the Q slots.  grid (n / kEvalBlock, comps r, count)
__global__ void __launch_bounds__(kEvalBlock)
k_addsub(const EvConsts* __restrict__ c, EvView out, EvView x, EvView y, unsigned n, bool sub)
{
    const unsigned r = c->r, h = blockIdx.y / r, j = blockIdx.y % r, z = blockIdx.z;
    const size_t k = (size_t)j * n + blockIdx.x * kEvalBlock + threadIdx.x;
    const u64 q = c->q[j].q;
    u64 a = x.p[h * x.comp_stride + z * x.ct_stride + k];
    u64 b = y.p[h * y.comp_stride + z * y.ct_stride + k];
    a = a >= q ? a - q : a;
    b = b >= q ? b - q : b;
    out.p[h * out.comp_stride + z * out.ct_stride + k] = sub ? sub_mod(a, b, q) : add_mod(a, b, q);
}

// ---- relin key i, prime j: -(a s + e) + [i == j] s^2 in the NTT domain.  grid (n / kEvalBlock, r (j), r (i))
__global__ void __launch_bounds__(kEvalBlock)
k_relin_key(const EvConsts* __restrict__ c, u64* __restrict__ rlk, const u64* __restrict__ s_hat, unsigned n)
{
    const unsigned r = c->r, j = blockIdx.y, i = blockIdx.z;
    const unsigned k = blockIdx.x * kEvalBlock + threadIdx.x;
    const size_t R = r + 1;
    const EvPrime p = c->q[j];
    u64* k0 = rlk + ((size_t)i * 2 * R + j) * n + k;
    const u64 a = k0[R * n], s = s_hat[(size_t)j * n + k];
    Acc acc;                                            // (mac_red, written out: through it this kernel's instructions reorder)
    acc.mac(a, s);
    acc.add(k0[0]);
    u64 v = red128(acc, p);
    v = v ? p.q - v : 0;
    if (i == j) {
        Acc ss;
        ss.mac(s, s);
        v = add_mod(v, red128(ss, p), p.q);
    }
    k0[0] = v;
}

// run f(std::integral_constant<unsigned, r>) for the runtime r in 1 .. kEvalMaxQ
template <class F, unsigned... I>
hipError_t with_r_impl(unsigned r, F&& f, std::integer_sequence<unsigned, I...>)
{
    hipError_t e = hipErrorInvalidValue;
    ((r == I + 1 ? (void)(e = f(std::integral_constant<unsigned, I + 1>{})) : (void)0), ...);
    return e;
}
template <class F>
hipError_t with_r(unsigned r, F&& f)
{
    return with_r_impl(r, f, std::make_integer_sequence<unsigned, kEvalMaxQ>{});
}

}  // namespace

hipError_t ev_extend(const EvConsts& h, const EvConsts* d, u64* xq, u64* xb, const u64* a, const u64* b, unsigned count, hipStream_t s)
{
    return with_r(h.r, [&](auto RQ) {
        k_extend<decltype(RQ)::value><<<dim3(h.n / kEvalBlock, 4, count), kEvalBlock, 0, s>>>(d, xq, xb, a, b, h.n, count);
        return hipGetLastError();
    });
}

hipError_t ev_tensor(const EvConsts& h, const EvConsts* d, u64* xq, u64* xb, unsigned count, hipStream_t s)
{
    k_tensor<<<dim3(h.n / kEvalBlock, 2 * h.r + 1, count), kEvalBlock, 0, s>>>(d, xq, xb, h.n, count);
    return hipGetLastError();
}

hipError_t ev_rescale(const EvConsts& h, const EvConsts* d, u64* c3, const u64* xq, const u64* xb, unsigned count, hipStream_t s)
{
    return with_r(h.r, [&](auto RQ) {
        k_rescale<decltype(RQ)::value><<<dim3(h.n / kEvalBlock, 3, count), kEvalBlock, 0, s>>>(d, c3, xq, xb, h.n, count);
        return hipGetLastError();
    });
}

hipError_t ev_digits(const EvConsts& h, const EvConsts* d, u64* D, const u64* c3, unsigned count, hipStream_t s)
{
    k_digits<<<dim3(h.n / kEvalBlock, h.r, count), kEvalBlock, 0, s>>>(d, D, c3, h.n, count);
    return hipGetLastError();
}

hipError_t ev_relin_dot(const EvConsts& h, const EvConsts* d, u64* P, const u64* D, const u64* rlk, unsigned count, hipStream_t s)
{
    k_relin_dot<<<dim3(h.n / kEvalBlock, h.r, count), kEvalBlock, 0, s>>>(d, P, D, rlk, h.n, count);
    return hipGetLastError();
}

hipError_t ev_addsub(const EvConsts& h, const EvConsts* d, EvView out, EvView x, EvView y, unsigned comps, unsigned count, bool sub,
                     hipStream_t s)
{
    k_addsub<<<dim3(h.n / kEvalBlock, comps * h.r, count), kEvalBlock, 0, s>>>(d, out, x, y, h.n, sub);
    return hipGetLastError();
}

hipError_t ev_relin_key(const EvConsts& h, const EvConsts* d, u64* rlk, const u64* s_hat, hipStream_t s)
{
    k_relin_key<<<dim3(h.n / kEvalBlock, h.r, h.r), kEvalBlock, 0, s>>>(d, rlk, s_hat, h.n);
    return hipGetLastError();
}

}  // namespace mi355ntt
