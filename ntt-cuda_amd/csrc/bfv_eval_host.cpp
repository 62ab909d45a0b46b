// bfv_eval_host.cpp -- the BFV evaluator (C ABI section "BFV evaluation" of include/mi355ntt.h): auxiliary prime search, BEHZ
// constants, relinearization and Galois key generation and the drivers.  Transforms run through the evaluator's two exact contexts
// (one over Q, one over B_sk); the element-wise RNS steps through kernels_bfv_eval.hip, kernels_bfv_galois.hip and
// kernels_bfv_hoist.hip.  DESIGN.md, "BFV evaluation", states the algorithm and the bounds the constants below rely on.
// EvScratch is the one description of the scratch buffer, EV_ENTER the one driver prologue.
#include "../../include/mi355ntt.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <utility>

#include "bfv.hpp"
#include "bfv_eval.hpp"
#include "bfv_eval_arith.cuh"
#include "device_scope.hpp"

using namespace mi355ntt;

namespace mi355ntt {
void record_hip_error(int e);      // capi.cpp: what mi355ntt_last_hip_error() reports
}

namespace {

// deterministic Miller-Rabin for every 64-bit n (the first twelve primes as bases suffice below 3.3e24)
bool is_prime64(u64 n)
{
    if (n < 2) return false;
    static const u64 small[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    for (u64 p : small)
        if (n % p == 0) return n == p;
    u64 d = n - 1;
    unsigned s = 0;
    while ((d & 1) == 0) {
        d >>= 1;
        s++;
    }
    for (u64 a : small) {
        u64 x = modpow(a, d, n);
        if (x == 1 || x == n - 1) continue;
        bool composite = true;
        for (unsigned i = 1; i < s && composite; i++) {
            x = mulmod(x, x, n);
            if (x == n - 1) composite = false;
        }
        if (composite) return false;
    }
    return true;
}

// the r + 1 largest primes p = 1 (mod 2n) below 2^61 on which the reference's Barrett is exact and that are not in excl[0..nexcl);
// psi: x^((p - 1) / 2n) for the first x = 2, 3, ... with psi^n = -1
int aux_primes(unsigned n, unsigned r, const u64* excl, unsigned nexcl, u64* b, u64* psi_b)
{
    if (n < 2048 || n > 65536 || (n & (n - 1)) != 0) return MI355NTT_EUNSUPPORTED;
    if (r < 1 || r > kEvalMaxQ) return MI355NTT_EUNSUPPORTED;
    const u64 step = 2ull * n;
    unsigned found = 0;
    for (u64 p = (1ull << 61) - step + 1; found < r + 1 && p > (1ull << 60); p -= step) {
        bool skip = false;
        for (unsigned i = 0; i < nexcl; i++) skip |= excl[i] == p;
        if (skip || !is_prime64(p)) continue;
        const unsigned k = bit_length(p);
        if (!barrett_single_subtraction_exact(p, k, barrett_mu(p, k))) continue;
        u64 psi = 0;
        for (u64 x = 2; x < 1000 && !psi; x++) {
            const u64 w = modpow(x, (p - 1) / step, p);
            if (modpow(w, n, p) == p - 1) psi = w;
        }
        if (!psi) continue;
        b[found] = p;
        if (psi_b) psi_b[found] = psi;
        found++;
    }
    return found == r + 1 ? MI355NTT_OK : MI355NTT_EUNSUPPORTED;
}

EvPrime ev_prime(u64 q)
{
    EvPrime e;
    e.q = q;
    e.m64 = ~0ULL / q;
    e.r64 = (u64)((((u128)1) << 64) % q);
    e.r64p = shoup(e.r64, q);
    return e;
}

u64 inv_mod_2_32(u64 a)       // a odd
{
    u64 x = a;                // Newton: each step doubles the correct low bits (3 -> 6 -> 12 -> 24 -> 48)
    for (int i = 0; i < 5; i++) x *= 2 - a * x;
    return x & 0xffffffffull;
}

// product of m[0..cnt) except m[skip] (skip = cnt: all of them), mod p
u64 prod_mod(const u64* m, unsigned cnt, unsigned skip, u64 p)
{
    u64 x = 1 % p;
    for (unsigned i = 0; i < cnt; i++)
        if (i != skip) x = mulmod(x, m[i] % p, p);
    return x;
}

void build_consts(EvConsts& c, unsigned n, unsigned r, u64 t, const u64* q, const u64* b)
{
    std::memset(&c, 0, sizeof(c));
    c.r = r;
    c.n = n;
    c.t = t;
    const u64 msk = b[r];
    for (unsigned i = 0; i < r; i++) c.q[i] = ev_prime(q[i]);
    for (unsigned j = 0; j <= r; j++) c.b[j] = ev_prime(b[j]);
    const u64 mt = 1ull << 32, mask = mt - 1;
    u64 q_mt = 1;
    for (unsigned i = 0; i < r; i++) q_mt *= q[i];
    c.ext_neg_qinv_mt = (mt - inv_mod_2_32(q_mt & mask)) & mask;
    for (unsigned i = 0; i < r; i++) {
        const u64 punct = prod_mod(q, r, i, q[i]);
        const u64 pinv = modinv(punct, q[i]);
        c.ext_qc[i] = mulmod(mt % q[i], pinv, q[i]);
        c.ext_qcp[i] = shoup(c.ext_qc[i], q[i]);
        c.rs_qc[i] = mulmod(t % q[i], pinv, q[i]);
        c.rs_qcp[i] = shoup(c.rs_qc[i], q[i]);
        u64 pm = 1;
        for (unsigned k = 0; k < r; k++)
            if (k != i) pm *= q[k];
        c.ext_mt[i] = pm & mask;
    }
    for (unsigned j = 0; j <= r; j++) {
        const u64 bj = b[j];
        const u64 mt_inv = modinv(mt % bj, bj);
        for (unsigned i = 0; i < r; i++) {
            c.ext_w[i][j] = mulmod(prod_mod(q, r, i, bj), mt_inv, bj);
            c.rs_w[i][j] = bj - modinv(q[i] % bj, bj);
        }
        const u64 qb = prod_mod(q, r, r, bj);
        c.ext_qm[j] = mulmod(qb, mt_inv, bj);
        c.ext_neg_qm[j] = c.ext_qm[j] ? bj - c.ext_qm[j] : 0;
        c.rs_tq[j] = mulmod(t % bj, modinv(qb, bj), bj);
    }
    for (unsigned j = 0; j < r; j++) {
        c.sk_bc[j] = modinv(prod_mod(b, r, j, b[j]), b[j]);
        c.sk_bcp[j] = shoup(c.sk_bc[j], b[j]);
        c.sk_msk_w[j] = modinv(b[j] % msk, msk);
        for (unsigned i = 0; i < r; i++) c.sk_w[j][i] = prod_mod(b, r, j, q[i]);
    }
    c.sk_neg_binv = msk - modinv(prod_mod(b, r, r, msk), msk);
    for (unsigned i = 0; i < r; i++) {
        c.sk_bq[i] = prod_mod(b, r, r, q[i]);
        c.sk_neg_bq[i] = c.sk_bq[i] ? q[i] - c.sk_bq[i] : 0;
    }
}

// The scratch buffer of a call on `count` ciphertexts: the offset, in words, of every region a driver uses.  One polynomial per
// ciphertext is count n words; the buffer is a work region of max(8 r + 4, r^2 + 2 r) of them, which every call but multiply_relin
// lays its regions over from offset 0, and behind it 3 (r + 1) more, where multiply_relin keeps its c3 [3][count][R][n].
struct EvScratch {
    size_t r, poly;                                  // poly = count n
    constexpr EvScratch(unsigned r_, size_t n, size_t count) : r(r_), poly(count * n) {}
    constexpr size_t work() const { return (8 * r + 4 > r * r + 2 * r ? 8 * r + 4 : r * r + 2 * r) * poly; }
    constexpr size_t total() const { return work() + 3 * (r + 1) * poly; }
    // multiply: XQ [4][count][r][n], XB [4][count][r + 1][n]
    constexpr size_t xq() const { return 0; }
    constexpr size_t xb() const { return 4 * r * poly; }
    constexpr size_t mult_end() const { return xb() + 4 * (r + 1) * poly; }
    // key switch (relinearize, apply_galois): digits D [count][r][r][n], products P [2][count][r][n]; apply_galois stages
    // T [count][r][n] = tau_g(c0) behind them
    constexpr size_t digits() const { return 0; }
    constexpr size_t products() const { return r * r * poly; }
    constexpr size_t galois_t() const { return products() + 2 * r * poly; }
    constexpr size_t galois_end() const { return galois_t() + r * poly; }
    // multiply_relin: c3 behind the work region
    constexpr size_t c3() const { return work(); }
    // multiply_plain: dense copies X [2][count][r][n], lifted plaintext mhat [count][r][n]
    constexpr size_t plain_x() const { return 0; }
    constexpr size_t plain_mhat() const { return 2 * r * poly; }
    constexpr size_t plain_end() const { return plain_mhat() + r * poly; }
    // apply_galois_hoisted: D, then P [group][2][count][r][n] for as many elements as fit behind D, at most kHoistMaxGroup
    // (r = 1: 8, 2: 6, 3: 5, 4: 4, 5 and 6: 3, 7 .. 15: 2)
    constexpr unsigned hoist_group() const
    {
        const size_t g = (EvScratch(r, 1, 1).total() - r * r) / (2 * r);       // a function of r alone
        return g < kHoistMaxGroup ? (unsigned)g : kHoistMaxGroup;
    }
    constexpr size_t hoist_end() const { return products() + hoist_group() * 2 * r * poly; }
    // galois_sum: D, T [count][r][n] = c0 (transformed with the digits in one batch), P [2][count][r][n]
    constexpr size_t sum_t() const { return r * r * poly; }
    constexpr size_t sum_p() const { return sum_t() + r * poly; }
    constexpr size_t sum_end() const { return sum_p() + 2 * r * poly; }
};

// every call's regions fit: in the work region where multiply_relin keeps c3 alive behind it, in the buffer otherwise
constexpr bool scratch_fits(unsigned r)
{
    const EvScratch L(r, 1, 1);
    return L.mult_end() <= L.work() && L.products() + 2 * r <= L.work() && L.c3() + 3 * (r + 1) == L.total() &&
           L.galois_end() <= L.total() && L.plain_end() <= L.total() && L.hoist_group() >= 1 && L.hoist_end() <= L.total() &&
           L.sum_end() <= L.total();
}
template <unsigned... I>
constexpr bool scratch_fits_all(std::integer_sequence<unsigned, I...>)
{
    return (scratch_fits(I + 1) && ...);
}
static_assert(scratch_fits_all(std::make_integer_sequence<unsigned, kEvalMaxQ>{}), "an evaluator call overruns its scratch buffer");

// The keystream key of relinearization keys: NOT keygen_rns's (32 x 0x01).  With keygen's key, relin_keygen_rns and keygen_rns called
// with the same nonce would draw key 0's uniform and error samples from keygen's bytes, and rlk_0[0] - pk[0] would be s^2 mod q_0.
const unsigned char kRelinKey[32] = {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2};

}  // namespace

struct mi355ntt_bfv_eval {
    const mi355ntt_bfv* bfv = nullptr;
    mi355ntt_ctx* ctx_q = nullptr;      // exact transforms over Q = q_0 .. q_{r-1}
    mi355ntt_ctx* ctx_b = nullptr;      // exact transforms over B_sk = b_0 .. b_{r-1}, m_sk
    int device = 0;
    unsigned n = 0, r = 0, R = 0;
    EvConsts h;
    EvConsts* d = nullptr;
};

#define EV_HIP(expr)                          \
    do {                                      \
        hipError_t e__ = (expr);              \
        if (e__ != hipSuccess) {              \
            record_hip_error((int)e__);       \
            return MI355NTT_EHIP;             \
        }                                     \
    } while (0)
#define EV_RC(expr)             \
    do {                        \
        int rc__ = (expr);      \
        if (rc__) return rc__;  \
    } while (0)
// The prologue of every driver, in the manner of capi.cpp's ON_CTX_DEVICE: EINVAL unless `ptrs_ok` (the evaluator first), then the
// call's own argument check (a return code), then the evaluator's device for the rest of the scope and the launch stream as `s`.
#define EV_ENTER(ptrs_ok, check, stream)            \
    if (!(ptrs_ok)) return MI355NTT_EINVAL;         \
    EV_RC(check);                                   \
    DeviceScope scope__(ev->device);                \
    EV_HIP(scope__.err);                            \
    const hipStream_t s = (hipStream_t)(stream);    \
    (void)s

namespace {

// argument checks as return codes: EINVAL if `bad`, and the first of two checks that fails
int ev_einval_if(bool bad) { return bad ? MI355NTT_EINVAL : MI355NTT_OK; }
int ev_first(int rc_a, int rc_b) { return rc_a ? rc_a : rc_b; }

// the checks every batched evaluator call makes before it touches memory
int ev_count_ok(unsigned count)
{
    if (count == 0) return MI355NTT_EINVAL;
    if (count > kEvalMaxCount) return MI355NTT_EUNSUPPORTED;
    return MI355NTT_OK;
}

int ev_multiply(const mi355ntt_bfv_eval* ev, u64* c3, const u64* a, const u64* b, unsigned count, u64* scratch, hipStream_t s)
{
    const unsigned r = ev->r;
    const size_t nq = (size_t)count * r, nb = (size_t)count * (r + 1);
    const EvScratch L(r, ev->n, count);
    u64* xq = scratch + L.xq();
    u64* xb = scratch + L.xb();
    EV_HIP(ev_extend(ev->h, ev->d, xq, xb, a, b, count, s));
    EV_RC(mi355ntt_forward_batch(ev->ctx_q, xq, (unsigned)(4 * nq), r, s));
    EV_RC(mi355ntt_forward_batch(ev->ctx_b, xb, (unsigned)(4 * nb), r + 1, s));
    EV_HIP(ev_tensor(ev->h, ev->d, xq, xb, count, s));
    EV_RC(mi355ntt_inverse_batch(ev->ctx_q, xq, (unsigned)(3 * nq), r, s));
    EV_RC(mi355ntt_inverse_batch(ev->ctx_b, xb, (unsigned)(3 * nb), r + 1, s));
    EV_HIP(ev_rescale(ev->h, ev->d, c3, xq, xb, count, s));
    return MI355NTT_OK;
}

// the key switch shared by relinearization and the Galois automorphisms: digits D [count][r][r][n] (coefficient domain, written by the
// caller) -> P [2][count][r][n] = INTT(sum_i NTT(D_i) key_i), key [r][2][R][n]
int ev_keyswitch(const mi355ntt_bfv_eval* ev, u64* P, u64* D, const u64* key, unsigned count, hipStream_t s)
{
    const unsigned r = ev->r;
    EV_RC(mi355ntt_forward_batch(ev->ctx_q, D, count * r * r, r, s));
    EV_HIP(ev_relin_dot(ev->h, ev->d, P, D, key, count, s));
    EV_RC(mi355ntt_inverse_batch(ev->ctx_q, P, 2 * count * r, r, s));
    return MI355NTT_OK;
}

int ev_relinearize(const mi355ntt_bfv_eval* ev, u64* c, const u64* c3, const u64* rlk, unsigned count, u64* scratch, hipStream_t s)
{
    const unsigned r = ev->r, R = ev->R, n = ev->n;
    const EvScratch L(r, n, count);
    u64* D = scratch + L.digits();
    u64* P = scratch + L.products();
    EV_HIP(ev_digits(ev->h, ev->d, D, c3, count, s));
    EV_RC(ev_keyswitch(ev, P, D, rlk, count, s));
    const size_t cs = (size_t)count * R * n;
    EV_HIP(ev_addsub(ev->h, ev->d, EvView{c, cs, (size_t)R * n}, EvView{const_cast<u64*>(c3), cs, (size_t)R * n},
                     EvView{P, (size_t)count * r * n, (size_t)r * n}, 2, count, false, s));
    return MI355NTT_OK;
}

// word offset of part i of a key [r][2][R][n] (slot 0, then slot 1); counted through a key set [keys][r][2][R][n], part i of key e
// is e r + i
size_t ev_key_part(const mi355ntt_bfv_eval* ev, size_t i) { return i * 2 * ev->R * ev->n; }

constexpr unsigned kRelin = 0;      // ev_finish_key's "Galois element" of a relinearization key (a real one is odd)

// explicit samples a, e [r][R][n] into a key: e_i into slot 0, a_i into slot 1 (coefficient domain, the Q words)
int ev_copy_samples(const mi355ntt_bfv_eval* ev, u64* key, const u64* d_a, const u64* d_e, hipStream_t s)
{
    const size_t Rn = (size_t)ev->R * ev->n, bytes = (size_t)ev->r * ev->n * sizeof(u64);
    for (unsigned i = 0; i < ev->r; i++) {
        u64* k0 = key + ev_key_part(ev, i);
        EV_HIP(hipMemcpyAsync(k0, d_e + i * Rn, bytes, hipMemcpyDeviceToDevice, s));
        EV_HIP(hipMemcpyAsync(k0 + Rn, d_a + i * Rn, bytes, hipMemcpyDeviceToDevice, s));
    }
    return MI355NTT_OK;
}

// a key's samples from r blocks of keystream at rnd, by keygen's conversions: the uniform sample lands in slot 1 (the public key's
// second half), the Gaussian one in slot 0; the ternary one in d_temp is not used
int ev_draw_samples(const mi355ntt_bfv_eval* ev, u64* key, const unsigned char* rnd, u64* d_temp, hipStream_t s)
{
    const size_t bytes = mi355ntt_bfv_keygen_random_bytes(ev->bfv);
    for (unsigned i = 0; i < ev->r; i++) {
        u64* k0 = key + ev_key_part(ev, i);
        EV_RC(mi355ntt_bfv_sample_keygen(ev->bfv, rnd + i * bytes, d_temp, k0, k0, s));
    }
    return MI355NTT_OK;
}

// slot 0 of every part holds e_i (coefficient domain), slot 1 a_i: to the NTT domain, then -(a_i s + e_i) + [j == i] s^2 for
// g == kRelin, + [j == i] tau_g(s) for a Galois element g
int ev_finish_key(const mi355ntt_bfv_eval* ev, u64* key, const u64* sk, unsigned g, hipStream_t s)
{
    for (unsigned i = 0; i < ev->r; i++) EV_RC(mi355ntt_forward_batch(ev->ctx_q, key + ev_key_part(ev, i), ev->r, ev->r, s));
    EV_HIP(g == kRelin ? ev_relin_key(ev->h, ev->d, key, sk, s) : ev_galois_key(ev->h, ev->d, key, sk, g, s));
    return MI355NTT_OK;
}

// mhat [count][r][n]: the centred lift of the plaintexts m in the NTT domain over Q
int ev_lift_ntt(const mi355ntt_bfv_eval* ev, u64* mhat, const u64* m, unsigned count, hipStream_t s)
{
    EV_HIP(ev_plain_lift(ev->h, ev->d, mhat, m, count, s));
    EV_RC(mi355ntt_forward_batch(ev->ctx_q, mhat, count * ev->r, ev->r, s));
    return MI355NTT_OK;
}

// a Galois element: odd, 1 <= g < 2n
bool ev_galois_ok(const mi355ntt_bfv_eval* ev, unsigned g) { return (g & 1) && g < 2 * ev->n; }

int ev_galois_all_ok(const mi355ntt_bfv_eval* ev, const unsigned* gs, unsigned num_g)
{
    for (unsigned k = 0; k < num_g; k++)
        if (!ev_galois_ok(ev, gs[k])) return MI355NTT_EINVAL;
    return MI355NTT_OK;
}

// g^-1 mod 2n for odd g (Newton over 2^32; 2n divides 2^32)
unsigned ev_galois_inverse(unsigned g, unsigned n)
{
    unsigned x = g;
    for (int i = 0; i < 5; i++) x *= 2 - g * x;
    return x & (2 * n - 1);
}

// the checks both hoisted calls make before they touch memory: every element odd and below 2n, 1 <= count <= kEvalMaxCount
int ev_hoist_args_ok(const mi355ntt_bfv_eval* ev, const unsigned* gs, unsigned num_g, unsigned count)
{
    if (num_g == 0 || count == 0 || count > kEvalMaxCount) return MI355NTT_EINVAL;
    return ev_galois_all_ok(ev, gs, num_g);
}

// The keystream key of Galois keys: neither keygen_rns's (32 x 0x01) nor relinearization's (32 x 0x02), for the reason kRelinKey gives.
const unsigned char kGaloisKey[32] = {3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3};

}  // namespace

extern "C" {

int mi355ntt_bfv_aux_primes(unsigned n, unsigned r, mi355ntt_u64* b, mi355ntt_u64* psi_b)
{
    if (!b) return MI355NTT_EINVAL;
    return aux_primes(n, r, nullptr, 0, b, psi_b);
}

int mi355ntt_bfv_eval_create(mi355ntt_bfv_eval** out, const mi355ntt_bfv* bfv)
{
    if (!out || !bfv) return MI355NTT_EINVAL;
    *out = nullptr;
    const BfvParams& p = bfv->p;
    const unsigned R = p.R, r = p.r, n = p.n;
    if (r < 1 || r > kEvalMaxQ) return MI355NTT_EUNSUPPORTED;
    u64 q[kMaxPrimes], psi[kMaxPrimes], b[kEvalMaxBsk], psi_b[kEvalMaxBsk];
    for (unsigned i = 0; i < R; i++) {
        EV_RC(mi355ntt_ctx_prime(bfv->ntt, i, &q[i], nullptr, nullptr, &psi[i], nullptr));
        if (i < r && q[i] >= (1ull << 61)) return MI355NTT_EUNSUPPORTED;     // 128-bit sums of r + 2 products (bfv_eval.hpp)
    }
    EV_RC(aux_primes(n, r, q, R, b, psi_b));
    // BEHZ size condition: 4 n t Q + 2 (r + 1) B < B m_sk, checked as
    // sum bits(q_i) + log2 n + log2 t + 3 <= sum (bits(b_j) - 1)
    unsigned lhs = 3, rhs = 0;
    lhs += log2_of(n) + bit_length(p.t) - 1;
    for (unsigned i = 0; i < r; i++) lhs += bit_length(q[i]);
    for (unsigned j = 0; j <= r; j++) rhs += bit_length(b[j]) - 1;
    if (lhs > rhs) return MI355NTT_EUNSUPPORTED;
    mi355ntt_bfv_eval* ev = new (std::nothrow) mi355ntt_bfv_eval();
    if (!ev) return MI355NTT_ENOMEM;
    ev->bfv = bfv;
    ev->device = mi355ntt_ctx_device(bfv->ntt);
    ev->n = n;
    ev->r = r;
    ev->R = R;
    build_consts(ev->h, n, r, p.t, q, b);
    int rc = mi355ntt_ctx_create_ex(&ev->ctx_q, n, r, q, psi, ev->device, MI355NTT_CTX_EXACT_ON_INEXACT_PRIMES);
    if (!rc) rc = mi355ntt_ctx_create_ex(&ev->ctx_b, n, r + 1, b, psi_b, ev->device, MI355NTT_CTX_EXACT_ON_INEXACT_PRIMES);
    if (!rc) {
        DeviceScope scope(ev->device);
        hipError_t e = scope.err;
        if (e == hipSuccess) e = hipMalloc(&ev->d, sizeof(EvConsts));
        if (e == hipSuccess) e = hipMemcpy(ev->d, &ev->h, sizeof(EvConsts), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            record_hip_error((int)e);
            rc = e == hipErrorOutOfMemory ? MI355NTT_ENOMEM : MI355NTT_EHIP;
        }
    }
    if (rc) {
        mi355ntt_bfv_eval_destroy(ev);
        return rc;
    }
    *out = ev;
    return MI355NTT_OK;
}

int mi355ntt_bfv_eval_destroy(mi355ntt_bfv_eval* ev)
{
    if (!ev) return MI355NTT_OK;
    {
        DeviceScope scope(ev->device);
        if (ev->d) (void)hipFree(ev->d);
    }
    if (ev->ctx_q) mi355ntt_ctx_destroy(ev->ctx_q);
    if (ev->ctx_b) mi355ntt_ctx_destroy(ev->ctx_b);
    delete ev;
    return MI355NTT_OK;
}

int mi355ntt_bfv_eval_aux_primes(const mi355ntt_bfv_eval* ev, mi355ntt_u64* b)
{
    if (!ev || !b) return MI355NTT_EINVAL;
    for (unsigned j = 0; j <= ev->r; j++) b[j] = ev->h.b[j].q;
    return MI355NTT_OK;
}

size_t mi355ntt_bfv_eval_scratch_bytes(const mi355ntt_bfv_eval* ev, unsigned count)
{
    return ev ? EvScratch(ev->r, ev->n, count).total() * sizeof(u64) : 0;
}

int mi355ntt_bfv_relin_keygen(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_rlk, const mi355ntt_u64* d_secret_key, const mi355ntt_u64* d_a,
                              const mi355ntt_u64* d_e, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_rlk && d_secret_key && d_a && d_e, MI355NTT_OK, stream);
    EV_RC(ev_copy_samples(ev, d_rlk, d_a, d_e, s));
    return ev_finish_key(ev, d_rlk, d_secret_key, kRelin, s);
}

int mi355ntt_bfv_relin_keygen_rns(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_rlk, const mi355ntt_u64* d_secret_key, void* d_in,
                                  mi355ntt_u64* d_temp, mi355ntt_u64 nonce, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_rlk && d_secret_key && d_in && d_temp, ev_einval_if(((uintptr_t)d_in & 15) != 0), stream);
    EV_RC(mi355ntt_salsa20_keystream(d_in, ev->r * mi355ntt_bfv_keygen_random_bytes(ev->bfv), kRelinKey, nonce, stream));
    EV_RC(ev_draw_samples(ev, d_rlk, static_cast<unsigned char*>(d_in), d_temp, s));
    return ev_finish_key(ev, d_rlk, d_secret_key, kRelin, s);
}

static int ev_addsub_call(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_b, unsigned count,
                          mi355ntt_stream stream, bool sub)
{
    EV_ENTER(ev && d_c && d_a && d_b, ev_count_ok(count), stream);
    const size_t cs = (size_t)count * ev->R * ev->n, zs = (size_t)ev->R * ev->n;
    EV_HIP(ev_addsub(ev->h, ev->d, EvView{d_c, cs, zs}, EvView{const_cast<u64*>(d_a), cs, zs}, EvView{const_cast<u64*>(d_b), cs, zs}, 2,
                     count, sub, s));
    return MI355NTT_OK;
}

int mi355ntt_bfv_add(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_b, unsigned count,
                     mi355ntt_stream stream)
{
    return ev_addsub_call(ev, d_c, d_a, d_b, count, stream, false);
}

int mi355ntt_bfv_sub(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_b, unsigned count,
                     mi355ntt_stream stream)
{
    return ev_addsub_call(ev, d_c, d_a, d_b, count, stream, true);
}

int mi355ntt_bfv_multiply(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c3, const mi355ntt_u64* d_a, const mi355ntt_u64* d_b,
                          unsigned count, void* d_scratch, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_c3 && d_a && d_b && d_scratch, ev_count_ok(count), stream);
    return ev_multiply(ev, d_c3, d_a, d_b, count, static_cast<u64*>(d_scratch), s);
}

int mi355ntt_bfv_relinearize(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_c3, const mi355ntt_u64* d_rlk,
                             unsigned count, void* d_scratch, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_c && d_c3 && d_rlk && d_scratch, ev_count_ok(count), stream);
    return ev_relinearize(ev, d_c, d_c3, d_rlk, count, static_cast<u64*>(d_scratch), s);
}

int mi355ntt_bfv_multiply_relin(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_b,
                                const mi355ntt_u64* d_rlk, unsigned count, void* d_scratch, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_c && d_a && d_b && d_rlk && d_scratch, ev_count_ok(count), stream);
    u64* work = static_cast<u64*>(d_scratch);
    u64* c3 = work + EvScratch(ev->r, ev->n, count).c3();
    EV_RC(ev_multiply(ev, c3, d_a, d_b, count, work, s));
    return ev_relinearize(ev, d_c, c3, d_rlk, count, work, s);
}

static int ev_plain_addsub_call(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_m,
                                unsigned count, mi355ntt_stream stream, bool sub)
{
    EV_ENTER(ev && d_c && d_a && d_m, ev_count_ok(count), stream);
    EV_HIP(ev_plain_addsub(ev->h, ev->d, d_c, d_a, d_m, count, sub, s));
    return MI355NTT_OK;
}

int mi355ntt_bfv_add_plain(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_m,
                           unsigned count, mi355ntt_stream stream)
{
    return ev_plain_addsub_call(ev, d_c, d_a, d_m, count, stream, false);
}

int mi355ntt_bfv_sub_plain(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_m,
                           unsigned count, mi355ntt_stream stream)
{
    return ev_plain_addsub_call(ev, d_c, d_a, d_m, count, stream, true);
}

int mi355ntt_bfv_plain_ntt(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_mhat, const mi355ntt_u64* d_m, unsigned count,
                           mi355ntt_stream stream)
{
    EV_ENTER(ev && d_mhat && d_m, ev_count_ok(count), stream);
    return ev_lift_ntt(ev, d_mhat, d_m, count, s);
}

namespace {

// c_h mhat for both components: canonical dense copies X [2][count][r][n] in scratch, fused products, write-back
int ev_multiply_plain(const mi355ntt_bfv_eval* ev, u64* c, const u64* a, const u64* mhat, unsigned count, bool shared, u64* X,
                      hipStream_t s)
{
    const unsigned r = ev->r;
    const unsigned half = count * r;
    EV_HIP(ev_plain_copy(ev->h, ev->d, const_cast<u64*>(a), X, count, true, s));
    if (shared) {
        EV_RC(mi355ntt_polymul_batch_shared(ev->ctx_q, X, mhat, 2 * half, r, 0, s));
    } else {
        EV_RC(mi355ntt_polymul_batch(ev->ctx_q, X, mhat, half, r, s));
        EV_RC(mi355ntt_polymul_batch(ev->ctx_q, X + (size_t)half * ev->n, mhat, half, r, s));
    }
    EV_HIP(ev_plain_copy(ev->h, ev->d, c, X, count, false, s));
    return MI355NTT_OK;
}

}  // namespace

int mi355ntt_bfv_multiply_plain(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_m,
                                unsigned count, void* d_scratch, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_c && d_a && d_m && d_scratch, ev_count_ok(count), stream);
    const EvScratch L(ev->r, ev->n, count);
    u64* X = static_cast<u64*>(d_scratch) + L.plain_x();
    u64* mhat = static_cast<u64*>(d_scratch) + L.plain_mhat();
    EV_RC(ev_lift_ntt(ev, mhat, d_m, count, s));
    return ev_multiply_plain(ev, d_c, d_a, mhat, count, false, X, s);
}

int mi355ntt_bfv_multiply_plain_ntt(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_mhat,
                                    unsigned count, int shared, void* d_scratch, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_c && d_a && d_mhat && d_scratch, ev_first(ev_einval_if(shared != 0 && shared != 1), ev_count_ok(count)),
             stream);
    u64* X = static_cast<u64*>(d_scratch) + EvScratch(ev->r, ev->n, count).plain_x();
    return ev_multiply_plain(ev, d_c, d_a, d_mhat, count, shared == 1, X, s);
}

int mi355ntt_bfv_galois_keygen(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_gk, const mi355ntt_u64* d_secret_key, unsigned g,
                               const mi355ntt_u64* d_a, const mi355ntt_u64* d_e, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_gk && d_secret_key && d_a && d_e, ev_galois_all_ok(ev, &g, 1), stream);
    EV_RC(ev_copy_samples(ev, d_gk, d_a, d_e, s));
    return ev_finish_key(ev, d_gk, d_secret_key, g, s);
}

int mi355ntt_bfv_galois_keygen_rns(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_gk, const mi355ntt_u64* d_secret_key, const unsigned* g,
                                   unsigned num_g, void* d_in, mi355ntt_u64* d_temp, mi355ntt_u64 nonce, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_gk && d_secret_key && g && d_in && d_temp && num_g != 0,
             ev_first(ev_einval_if(((uintptr_t)d_in & 15) != 0), ev_galois_all_ok(ev, g, num_g)), stream);
    const unsigned r = ev->r;
    const size_t bytes = mi355ntt_bfv_keygen_random_bytes(ev->bfv);
    EV_RC(mi355ntt_salsa20_keystream(d_in, (size_t)num_g * r * bytes, kGaloisKey, nonce, stream));
    for (unsigned k = 0; k < num_g; k++) {
        u64* gk = d_gk + ev_key_part(ev, (size_t)k * r);
        EV_RC(ev_draw_samples(ev, gk, static_cast<unsigned char*>(d_in) + (size_t)k * r * bytes, d_temp, s));
        EV_RC(ev_finish_key(ev, gk, d_secret_key, g[k], s));
    }
    return MI355NTT_OK;
}

int mi355ntt_bfv_apply_galois(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_gk,
                              unsigned g, unsigned count, void* d_scratch, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_c && d_a && d_gk && d_scratch, ev_first(ev_galois_all_ok(ev, &g, 1), ev_count_ok(count)), stream);
    const EvScratch L(ev->r, ev->n, count);
    u64* scratch = static_cast<u64*>(d_scratch);
    u64 *D = scratch + L.digits(), *P = scratch + L.products(), *T = scratch + L.galois_t();
    EV_HIP(ev_galois_digits(ev->h, ev->d, D, T, d_a, ev_galois_inverse(g, ev->n), count, s));
    EV_RC(ev_keyswitch(ev, P, D, d_gk, count, s));
    EV_HIP(ev_galois_finish(ev->h, ev->d, d_c, T, P, count, s));
    return MI355NTT_OK;
}

unsigned mi355ntt_bfv_hoist_group(const mi355ntt_bfv_eval* ev) { return ev ? EvScratch(ev->r, 1, 1).hoist_group() : 0; }

int mi355ntt_bfv_apply_galois_hoisted(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c_out, const mi355ntt_u64* d_a, const mi355ntt_u64* d_gk,
                                      const unsigned* gs, unsigned num_g, unsigned count, void* d_scratch, mi355ntt_stream stream)
{
    EV_ENTER(ev && d_c_out && d_a && d_gk && gs && d_scratch, ev_hoist_args_ok(ev, gs, num_g, count), stream);
    const EvScratch L(ev->r, ev->n, count);
    const unsigned r = ev->r, n = ev->n, group = L.hoist_group();
    const size_t R = ev->R;
    u64* D = static_cast<u64*>(d_scratch) + L.digits();
    u64* P = static_cast<u64*>(d_scratch) + L.products();
    // the digits of c1 itself (g = 1); the staged copy of c0 that comes with them lands in P's space and is not used
    EV_HIP(ev_galois_digits(ev->h, ev->d, D, P, d_a, 1, count, s));
    EV_RC(mi355ntt_forward_batch(ev->ctx_q, D, count * r * r, r, s));
    for (unsigned k0 = 0; k0 < num_g; k0 += group) {
        const unsigned elems = num_g - k0 < group ? num_g - k0 : group;
        HoistElems el = {};
        for (unsigned e = 0; e < elems; e++) {
            el.g[e] = gs[k0 + e];
            el.ginv[e] = ev_galois_inverse(gs[k0 + e], n);
        }
        EV_HIP(ev_hoist_dot(ev->h, ev->d, P, D, d_gk + ev_key_part(ev, (size_t)k0 * r), el, elems, count, s));
        EV_RC(mi355ntt_inverse_batch(ev->ctx_q, P, elems * 2 * count * r, r, s));
        EV_HIP(ev_hoist_finish(ev->h, ev->d, d_c_out + (size_t)k0 * 2 * count * R * n, d_a, P, el, elems, count, s));
    }
    return MI355NTT_OK;
}

int mi355ntt_bfv_galois_sum(const mi355ntt_bfv_eval* ev, mi355ntt_u64* d_c, const mi355ntt_u64* d_a, const mi355ntt_u64* d_gk,
                            const unsigned* gs, unsigned num_g, const mi355ntt_u64* d_weights, unsigned count, void* d_scratch,
                            mi355ntt_stream stream)
{
    EV_ENTER(ev && d_c && d_a && d_gk && gs && d_scratch, ev_hoist_args_ok(ev, gs, num_g, count), stream);
    const EvScratch L(ev->r, ev->n, count);
    const unsigned r = ev->r, n = ev->n;
    u64* scratch = static_cast<u64*>(d_scratch);
    u64 *D = scratch + L.digits(), *T = scratch + L.sum_t(), *P = scratch + L.sum_p();
    EV_HIP(ev_galois_digits(ev->h, ev->d, D, T, d_a, 1, count, s));
    EV_RC(mi355ntt_forward_batch(ev->ctx_q, D, count * r * (r + 1), r, s));
    for (unsigned k0 = 0; k0 < num_g; k0 += kHoistSumChunk) {
        const unsigned elems = num_g - k0 < kHoistSumChunk ? num_g - k0 : kHoistSumChunk;
        HoistSumElems el = {};
        for (unsigned e = 0; e < elems; e++) el.g[e] = gs[k0 + e];
        EV_HIP(ev_hoist_sum(ev->h, ev->d, P, D, T, d_gk + ev_key_part(ev, (size_t)k0 * r),
                            d_weights ? d_weights + (size_t)k0 * r * n : nullptr, el, elems, k0 == 0, count, s));
    }
    EV_RC(mi355ntt_inverse_batch(ev->ctx_q, P, 2 * count * r, r, s));
    EV_HIP(ev_plain_copy(ev->h, ev->d, d_c, P, count, false, s));
    return MI355NTT_OK;
}

}  // extern "C"
