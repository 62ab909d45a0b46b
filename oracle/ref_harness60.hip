/*
 * ref_harness60.hip -- drives the reference's own 60-bit kernels and BFV drivers (test infrastructure; ours).
 *
 * Built by `make -C oracle ref` against the translated headers under oracle/_ref/src (ref_port.py); never part of
 * the product.  It calls the reference's entry points and copies none of them: the only code here is file I/O
 * (ref_proto.h), device buffers, the caller-side bootstrap every reference program performs before its first
 * launch (twiddle tables through the reference's fillTablePsi128, the __constant__ arrays through
 * hipMemcpyToSymbol), and three tiny kernels that expose ref_shim.h's mul64 / sub128 and uint128.h's shift members (ref_shift.h)
 * for the self-check.
 *
 * Ops (RefCase::op); `a`, `b` are n-word polynomials unless said otherwise, modulus 0 is used where one is needed:
 *    0 selfcheck_mul64   in: pairs (x, y)               out: per pair lo, hi, lo', hi' (primed: c.low passed as a)
 *    1 selfcheck_sub128  in: quads (alo, ahi, blo, bhi) out: per quad lo, hi
 *    2 forwardNTT        in: a                          out: a
 *    3 inverseNTT        in: a                          out: a
 *    4 forwardNTTdouble  in: a, b (two streams)         out: a, b
 *    5 forwardNTT_batch  args: num, division  in: num polys   out: the same
 *    6 inverseNTT_batch  as 5
 *    7 barrett           in: a, b                       out: a
 *    8 barrett_batch     args: num, division  in: a[num], b[num]   out: a[num]
 *    9 barrett_batch_3param  as 8, out: c[num]
 *   10 barrett_int (through poly_mul_int)   args: b     in: a   out: a
 *   11 half_poly_mul_device   in: a, b                  out: a
 *   12 full_poly_mul_device   in: a, b                  out: a, b   (one stream for both stream arguments, see below)
 *   13 poly_add_device  14 poly_sub_device   in: a, b   out: a
 *   15 poly_negate_device                    in: a      out: a
 *   16 poly_add_integer_device  args: b      in: a      out: a
 *   17 poly_mul_int_t           args: b, t   in: a      out: a
 *   18 generate_random_default  args: nbytes            out: floor(nbytes / 64) * 8 words
 *   19 generate_random          args: nbytes            out: the same
 *   20 ternary_dist_xq   in: n bytes          out: nq * n words
 *   21 uniform_dist_xq   in: nq * n words     out: nq * n words
 *   22 gaussian_dist_xq  in: n u32            out: nq * n words
 *   23 convert_ternary_gaussian_x2   in: 9n bytes   out: c (2 nq n), e (2 nq n)
 *   24 keygen_rns -> encryption_rns -> decryption_rns
 *        args: t, gamma, mu_gamma, gamma_bits, neg_inv_q_mod_t, neg_inv_q_mod_gamma,
 *              inv_q_last_mod_q[nq-1], qi_div_t[nq], inv_punctured_q[nq-1], prod_t_gamma_mod_q[nq-1],
 *              base_change_matrix[2 (nq-1)]
 *        in: m (n words)   out: secret key (nq n), public key (2 nq n), c after encryption (2 nq n),
 *                               c after decryption (2 nq n)
 *   25 selfcheck_shift   in: triples (lo, hi, shift)   out: per triple lo, hi of `x >> shift`, of shiftr(x, shift), of `x << shift`
 *
 * full_poly_mul_device launches its pointwise product on stream2 while a's transform runs on stream1, with nothing
 * ordering the two.  The harness passes the same stream for both arguments so that the words are determined.
 * generate_random uploads only the first 24 bytes of its key; the rest is what the constant array held before (zero
 * in a fresh process, generate_random_default's bytes after a call of that).  Case order in a request is kept.
 */
#include <hip/hip_runtime.h>
#include <map>
#include <tuple>
#include <vector>

#include "ref_proto.h"

#include "helper.h"
#include "parameter.h"
#include "poly_arithmetic.cuh"
#include "distributions.cuh"
#include "bfv_keygen.cuh"
#include "bfv_encryption.cuh"
#include "bfv_decryption.cuh"

using std::vector;

__global__ void hk_mul64(const u64* in, u64* out, unsigned count)
{
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint128_t c;
    mul64(in[2 * i], in[2 * i + 1], c);
    out[4 * i] = c.low;
    out[4 * i + 1] = c.high;
    uint128_t d = in[2 * i];
    mul64(d.low, in[2 * i + 1], d);
    out[4 * i + 2] = d.low;
    out[4 * i + 3] = d.high;
}

__global__ void hk_sub128(const u64* in, u64* out, unsigned count)
{
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint128_t a, b;
    a.low = in[4 * i]; a.high = in[4 * i + 1];
    b.low = in[4 * i + 2]; b.high = in[4 * i + 3];
    sub128(a, b);
    out[2 * i] = a.low;
    out[2 * i + 1] = a.high;
}

__global__ void hk_shift(const u64* in, u64* out, unsigned count)
{
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint128_t x;
    x.low = in[3 * i]; x.high = in[3 * i + 1];
    unsigned s = (unsigned)in[3 * i + 2];
    uint128_t a = x >> s;
    uint128_t b = x;
    uint128_t::shiftr(b, s);
    uint128_t c = x << s;
    out[6 * i] = a.low; out[6 * i + 1] = a.high;
    out[6 * i + 2] = b.low; out[6 * i + 3] = b.high;
    out[6 * i + 4] = c.low; out[6 * i + 5] = c.high;
}

struct Dev {
    u64* p = nullptr;
    size_t words;
    explicit Dev(size_t w, const u64* src = nullptr) : words(w)
    {
        HIP_OK(hipMalloc(&p, (w ? w : 1) * 8));
        if (src) HIP_OK(hipMemcpy(p, src, w * 8, hipMemcpyHostToDevice));
        else HIP_OK(hipMemset(p, 0, (w ? w : 1) * 8));
    }
    void append_to(vector<u64>& out, size_t w) const
    {
        size_t at = out.size();
        out.resize(at + w);
        HIP_OK(hipMemcpy(out.data() + at, p, w * 8, hipMemcpyDeviceToHost));
    }
    ~Dev() { (void)hipFree(p); }
    Dev(const Dev&) = delete;
};

static void expect_in(const RefCase& c, size_t words)
{
    if (c.in.size() != words) REF_DIE("op %llu: %zu input words, wanted %zu", c.op, c.in.size(), words);
}
static void expect_args(const RefCase& c, size_t count)
{
    if (c.args.size() != count) REF_DIE("op %llu: %zu arguments, wanted %zu", c.op, c.args.size(), count);
}

/* q_cons / q_bit_cons / mu_cons, as every reference program uploads them before a batch launch */
static void upload_moduli(const RefCase& c)
{
    u64 q[16] = { 0 }, mu[16] = { 0 };
    unsigned k[16] = { 0 };
    for (size_t i = 0; i < c.mod.size(); i++) { q[i] = c.mod[i].q; mu[i] = c.mod[i].mu; k[i] = (unsigned)c.mod[i].qbit; }
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(q_cons), q, sizeof q));
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(mu_cons), mu, sizeof mu));
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(q_bit_cons), k, sizeof k));
}

/* twiddle tables of all moduli of a case, [nq][n] each, built by the reference's own fillTablePsi128 */
struct Tables {
    Dev psi, psiinv;
    Tables(size_t w) : psi(w), psiinv(w) {}
};
static std::map<std::tuple<u64, u64, u64>, std::pair<vector<u64>, vector<u64>>> g_table_cache;
static Tables* make_tables(const RefCase& c)
{
    size_t n = c.n;
    Tables* t = new Tables(c.mod.size() * n);
    for (size_t i = 0; i < c.mod.size(); i++) {
        const RefModulus& m = c.mod[i];
        if (!m.psi) continue;
        auto key = std::make_tuple(m.q, m.psi, (u64)n);
        auto it = g_table_cache.find(key);
        if (it == g_table_cache.end()) {
            vector<u64> f(n), b(n);
            fillTablePsi128(m.psi, m.q, modinv128(m.psi, m.q), f.data(), b.data(), (unsigned)n);
            it = g_table_cache.emplace(key, std::make_pair(f, b)).first;
        }
        HIP_OK(hipMemcpy(t->psi.p + i * n, it->second.first.data(), n * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(t->psiinv.p + i * n, it->second.second.data(), n * 8, hipMemcpyHostToDevice));
    }
    return t;
}

static void run_bfv(RefCase& c, hipStream_t* streams)
{
    const size_t n = c.n, nq = c.mod.size(), r = nq - 1;
    if (nq < 2) REF_DIE("op 24 wants at least two moduli");
    expect_in(c, n);
    expect_args(c, 6 + r + nq + r + r + 2 * r);
    const u64* a = c.args.data();
    u64 t = a[0], gamma = a[1], mu_gamma = a[2];
    unsigned gamma_bits = (unsigned)a[3];
    vector<u64> neg_inv = { a[4], a[5] };
    a += 6;
    vector<u64> inv_q_last(a, a + r); a += r;
    vector<u64> qi_div_t(a, a + nq); a += nq;
    vector<u64> inv_punct(a, a + r); a += r;
    vector<u64> prod_tg(a, a + r); a += r;
    vector<u64> bcm(a, a + 2 * r);

    vector<u64> q(nq), mu(nq);
    vector<unsigned> qbit(nq);
    for (size_t i = 0; i < nq; i++) { q[i] = c.mod[i].q; mu[i] = c.mod[i].mu; qbit[i] = (unsigned)c.mod[i].qbit; }
    u64 pad[16] = { 0 };
    memcpy(pad, inv_q_last.data(), r * 8);
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(inv_q_last_mod_q_cons), pad, sizeof pad));
    memcpy(pad, inv_punct.data(), r * 8);
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(inv_punctured_q_cons), pad, sizeof pad));
    memcpy(pad, prod_tg.data(), r * 8);
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(prod_t_gamma_mod_q_cons), pad, sizeof pad));

    Tables* tab = make_tables(c);
    size_t in_bytes = (1 + 8) * nq * n + 4 * n;
    Dev in((in_bytes + 7) / 8), sk(nq * n), pk(2 * nq * n), temp(nq * n), ct(2 * nq * n), e(2 * nq * n);
    Dev m(n, c.in.data()), d_q(nq, q.data()), d_qdt(nq, qi_div_t.data()), d_bcm(2 * r, bcm.data());
    vector<u64*> u(nq, nullptr);

    keygen_rns((unsigned char*)in.p, (int)nq, q.data(), (unsigned)n, sk.p, pk.p, streams, temp.p, mu, qbit, tab->psi.p, tab->psiinv.p);
    HIP_OK(hipDeviceSynchronize());
    sk.append_to(c.out, nq * n);
    pk.append_to(c.out, 2 * nq * n);

    encryption_rns(ct.p, pk.p, (unsigned char*)in.p, u.data(), e.p, (unsigned)n, streams, q.data(), qbit, mu, inv_q_last,
                   tab->psi.p, tab->psiinv.p, m.p, d_qdt.p, d_q.p, (unsigned)t, (int)nq);
    HIP_OK(hipDeviceSynchronize());
    ct.append_to(c.out, 2 * nq * n);

    vector<u64> output_base = { t, gamma };
    vector<unsigned> output_base_bits = { 0, gamma_bits };
    decryption_rns(ct.p, sk.p, q.data(), qbit, mu, tab->psi.p, tab->psiinv.p, (int)n, (unsigned)r, inv_punct, d_bcm.p,
                   t, gamma, mu_gamma, output_base, output_base_bits, neg_inv, gamma >> 1, prod_tg);
    HIP_OK(hipDeviceSynchronize());
    ct.append_to(c.out, 2 * nq * n);
    delete tab;
}

static void run_case(RefCase& c, hipStream_t* streams)
{
    const size_t n = c.n, nq = c.mod.size();
    hipStream_t& s1 = streams[0];
    hipStream_t& s2 = streams[1];
    if (c.op >= 2 && c.op != 25 && (n < 2048 || n > 32768 || (n & (n - 1)))) REF_DIE("op %llu: n = %zu is not a size the reference dispatches", c.op, n);
    if (c.op >= 2 && c.op != 18 && c.op != 19 && c.op != 25 && nq < 1) REF_DIE("op %llu wants a modulus", c.op);
    upload_moduli(c);
    const RefModulus m0 = nq ? c.mod[0] : RefModulus{ 0, 0, 0, 0 };

    switch (c.op) {
    case 0: {
        size_t count = c.in.size() / 2;
        expect_in(c, 2 * count);
        Dev in(2 * count, c.in.data()), out(4 * count);
        hk_mul64<<<(count + 63) / 64, 64, 0, s1>>>(in.p, out.p, (unsigned)count);
        HIP_OK(hipDeviceSynchronize());
        out.append_to(c.out, 4 * count);
        break;
    }
    case 1: {
        size_t count = c.in.size() / 4;
        expect_in(c, 4 * count);
        Dev in(4 * count, c.in.data()), out(2 * count);
        hk_sub128<<<(count + 63) / 64, 64, 0, s1>>>(in.p, out.p, (unsigned)count);
        HIP_OK(hipDeviceSynchronize());
        out.append_to(c.out, 2 * count);
        break;
    }
    case 2: case 3: {
        expect_in(c, n);
        Tables* t = make_tables(c);
        Dev a(n, c.in.data());
        if (c.op == 2) forwardNTT(a.p, (unsigned)n, s1, m0.q, m0.mu, (int)m0.qbit, t->psi.p);
        else inverseNTT(a.p, (unsigned)n, s1, m0.q, m0.mu, (int)m0.qbit, t->psiinv.p);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, n);
        delete t;
        break;
    }
    case 4: {
        expect_in(c, 2 * n);
        Tables* t = make_tables(c);
        Dev a(n, c.in.data()), b(n, c.in.data() + n);
        forwardNTTdouble(a.p, b.p, (unsigned)n, s1, s2, m0.q, m0.mu, (int)m0.qbit, t->psi.p);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, n);
        b.append_to(c.out, n);
        delete t;
        break;
    }
    case 5: case 6: {
        expect_args(c, 2);
        size_t num = c.args[0], division = c.args[1];
        if (!num || num > 4096 || !division || division > nq) REF_DIE("op %llu: num / division out of range", c.op);
        expect_in(c, num * n);
        Tables* t = make_tables(c);
        Dev a(num * n, c.in.data());
        if (c.op == 5) forwardNTT_batch(a.p, (unsigned)n, t->psi.p, (unsigned)num, (unsigned)division);
        else inverseNTT_batch(a.p, (unsigned)n, t->psiinv.p, (unsigned)num, (unsigned)division);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, num * n);
        delete t;
        break;
    }
    case 7: {
        expect_in(c, 2 * n);
        Dev a(n, c.in.data()), b(n, c.in.data() + n);
        barrett<<<n / 256, 256, 0, s1>>>(a.p, b.p, m0.q, m0.mu, (int)m0.qbit);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, n);
        break;
    }
    case 8: case 9: {
        expect_args(c, 2);
        size_t num = c.args[0], division = c.args[1];
        if (!num || num > 4096 || !division || division > nq) REF_DIE("op %llu: num / division out of range", c.op);
        expect_in(c, 2 * num * n);
        Dev a(num * n, c.in.data()), b(num * n, c.in.data() + num * n), out(num * n);
        dim3 grid((unsigned)(n / 256), (unsigned)num);
        if (c.op == 8) barrett_batch<<<grid, 256, 0, 0>>>(a.p, b.p, (unsigned)n, (unsigned)division);
        else barrett_batch_3param<<<grid, 256, 0, 0>>>(out.p, a.p, b.p, (unsigned)n, (unsigned)division);
        HIP_OK(hipDeviceSynchronize());
        (c.op == 8 ? a : out).append_to(c.out, num * n);
        break;
    }
    case 10: {
        expect_args(c, 1);
        expect_in(c, n);
        Dev a(n, c.in.data());
        poly_mul_int(a.p, c.args[0], (unsigned)n, s1, m0.q, m0.mu, (int)m0.qbit);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, n);
        break;
    }
    case 11: case 12: {
        expect_in(c, 2 * n);
        Tables* t = make_tables(c);
        Dev a(n, c.in.data()), b(n, c.in.data() + n);
        if (c.op == 11) half_poly_mul_device(a.p, b.p, (unsigned)n, s1, m0.q, m0.mu, (int)m0.qbit, t->psi.p, t->psiinv.p);
        else full_poly_mul_device(a.p, b.p, (unsigned)n, s1, s1, m0.q, m0.mu, (int)m0.qbit, t->psi.p);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, n);
        if (c.op == 12) b.append_to(c.out, n);
        delete t;
        break;
    }
    case 13: case 14: {
        expect_in(c, 2 * n);
        Dev a(n, c.in.data()), b(n, c.in.data() + n);
        if (c.op == 13) poly_add_device(a.p, b.p, (unsigned)n, s1, m0.q);
        else poly_sub_device(a.p, b.p, (unsigned)n, s1, m0.q);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, n);
        break;
    }
    case 15: case 16: case 17: {
        expect_args(c, c.op - 15);
        expect_in(c, n);
        Dev a(n, c.in.data());
        if (c.op == 15) poly_negate_device(a.p, (unsigned)n, s1, m0.q);
        else if (c.op == 16) poly_add_integer_device(a.p, c.args[0], (unsigned)n, s1, m0.q);
        else poly_mul_int_t(a.p, c.args[0], (unsigned)n, s1, c.args[1]);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, n);
        break;
    }
    case 18: case 19: {
        expect_args(c, 1);
        size_t nbytes = c.args[0];
        if (nbytes > (1u << 26)) REF_DIE("op %llu: too many bytes", c.op);
        Dev a(nbytes / 8 + 8);
        if (c.op == 18) generate_random_default((unsigned char*)a.p, (unsigned)nbytes);
        else generate_random((unsigned char*)a.p, (unsigned)nbytes, s1);
        HIP_OK(hipDeviceSynchronize());
        a.append_to(c.out, nbytes / 64 * 8);
        break;
    }
    case 20: case 21: case 22: {
        size_t want = c.op == 20 ? n / 8 : c.op == 21 ? nq * n : n / 2;
        expect_in(c, want);
        Dev in(want, c.in.data()), out(nq * n);
        unsigned grid = (unsigned)(nq * n / convertBlockSize);
        if (c.op == 20) ternary_dist_xq<<<grid, convertBlockSize, 0, 0>>>((unsigned char*)in.p, out.p, (unsigned)n, (unsigned)nq);
        else if (c.op == 21) uniform_dist_xq<<<grid, convertBlockSize, 0, 0>>>((unsigned char*)in.p, out.p, (unsigned)n, (unsigned)nq);
        else gaussian_dist_xq<<<grid, convertBlockSize, 0, 0>>>((unsigned char*)in.p, out.p, (unsigned)n, (unsigned)nq);
        HIP_OK(hipDeviceSynchronize());
        out.append_to(c.out, nq * n);
        break;
    }
    case 23: {
        expect_in(c, 9 * n / 8);
        Dev in(9 * n / 8, c.in.data()), ct(2 * nq * n), e(2 * nq * n);
        convert_ternary_gaussian_x2<<<(unsigned)(nq * n / convertBlockSize), convertBlockSize, 0, 0>>>((unsigned char*)in.p, ct.p, e.p, (unsigned)n, (int)nq);
        HIP_OK(hipDeviceSynchronize());
        ct.append_to(c.out, 2 * nq * n);
        e.append_to(c.out, 2 * nq * n);
        break;
    }
    case 24:
        run_bfv(c, streams);
        break;
    case 25: {
        size_t count = c.in.size() / 3;
        expect_in(c, 3 * count);
        Dev in(3 * count, c.in.data()), out(6 * count);
        hk_shift<<<(count + 63) / 64, 64, 0, s1>>>(in.p, out.p, (unsigned)count);
        HIP_OK(hipDeviceSynchronize());
        out.append_to(c.out, 6 * count);
        break;
    }
    default:
        REF_DIE("unknown op %llu", c.op);
    }
    HIP_OK(hipGetLastError());
}

int main(int argc, char** argv)
{
    if (argc != 3) REF_DIE("usage: %s REQUEST.bin RESPONSE.bin", argv[0]);
    vector<RefCase> cases = ref_read_request(argv[1]);
    hipStream_t streams[32];
    for (hipStream_t& s : streams) HIP_OK(hipStreamCreate(&s));
    for (RefCase& c : cases) run_case(c, streams);
    HIP_OK(hipDeviceSynchronize());
    ref_write_response(argv[2], cases);
    return 0;
}
