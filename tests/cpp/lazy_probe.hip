// lazy_probe -- the lazy modular primitives of csrc/ntt_core.cuh (and modarith.cuh) one operand tuple at a time, and the
// compile-time reduction policy as data.  Test infrastructure only (tests/test_lazy_bounds_host.py, tests/test_gpu_lazy_primitives.py).
//
//   lazy_probe policy          host only, never touches the GPU: JSON of fwd_reduce_mask, InvPolicy::mask / cmul and Lazy::TQ for
//                              LOGN = 11 .. 15 and HL = 2 .. 6, and of the (HL, NEAR) classes this program instantiates
//   lazy_probe consts Q K      host only: prime_reduction_constants(Q, K) as JSON (the function fast_tables_create calls)
//   lazy_probe run IN OUT      one element-wise kernel per record of IN, results to OUT
//
// IN (64-bit little-endian words): {MAGIC, records}, then per record {op, HL, NEAR, q, k, mu, count, arrays} followed by `arrays`
// blocks {length, words...}.  Per-tuple arrays hold `count` words.  The TWS = true forms read their twiddle through an "s" asm
// operand, so it must be wave-uniform: their w / wp arrays hold ONE entry per workgroup of kBlock tuples (ceil(count / kBlock)
// words), read at blockIdx.x.  OUT: per record `count` words (mul_wide: count low words, then count high words).
// Every thread handles one tuple, checks its index against count and stores once; all sizes are validated before any launch.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ntt-cuda_amd/csrc/ntt_core.cuh"

using namespace mi355ntt;

namespace {

constexpr u64 kMagic = 0x4c415a5950524f42ull;      // "LAZYPROB"
constexpr unsigned kBlock = 64;                    // one wave per workgroup: one (w, wp) per wave for the TWS forms
constexpr u64 kMaxCount = 1u << 20;

enum Op : int {
    OP_MUL_HI = 0, OP_MUL_WIDE, OP_BARRETT_MUL, OP_SHOUP_MUL_LAZY, OP_MUL_SHOUP2, OP_MUL_SHOUP4M, OP_MUL_SHOUP4M_TWS,
    OP_MUL_SHOUP4M_ACC, OP_MUL_SHOUP4M_ACC_TWS, OP_REDUCE_2Q, OP_REDUCE_2Q_NEAR, OP_MUL_FOLD_NEAR, OP_LIT_BARRETT_MUL,
    OP_CANON_FWD, OP_CANON_INV, OP_FUSED_MUL, OP_COUNT
};
// per-tuple arrays, per-workgroup arrays (the TWS twiddles, which come first in the record's operand order after y)
struct OpShape { int tuple_arrays, block_arrays; bool near_only, classed; };
constexpr OpShape kShape[OP_COUNT] = {
    {2, 0, false, false},   // mul_hi(a, b)
    {2, 0, false, false},   // mul_wide(a, b)
    {2, 0, false, false},   // barrett_mul(a, b)
    {3, 0, false, false},   // shoup_mul_lazy(y, w, wp)
    {3, 0, false, false},   // mul_shoup2(y, w, wp)
    {3, 0, false, false},   // mul_shoup4m<false>(y, w, wp)
    {1, 2, false, false},   // mul_shoup4m<true>(y; W, WP)
    {4, 0, false, false},   // mul_shoup4m_acc<false>(y, w, wp, base)
    {2, 2, false, false},   // mul_shoup4m_acc<true>(y, base; W, WP)
    {1, 0, false, false},   // reduce_2q(x)
    {1, 0, true, false},    // reduce_2q_near(x)
    {2, 0, true, false},    // mul_fold_near(x, b)
    {2, 0, false, false},   // lit_barrett_mul(y, w)
    {1, 0, false, true},    // canon_after_forward<HL, NEAR>(x)
    {1, 0, false, true},    // canon_after_inverse<HL, NEAR>(x)
    {2, 0, false, true},    // FusedMul<HL, NEAR>::mul(x, b)
};

// the (HL, NEAR) classes the library instantiates (dispatch_class, kernels_fast_impl.cuh; class HL_LIT and its exact primes' class 2)
struct ClassId { int hl; bool near; };
constexpr ClassId kClasses[] = {{6, true}, {5, true}, {4, true}, {3, true}, {2, true}, {6, false}, {4, false}, {3, false}, {2, false},
                                {HL_LIT, false}};

struct Args {
    const PrimeDev* p;
    const u64 *a, *b, *c, *d;      // per-tuple operands in record order
    const u64 *W, *WP;             // per-workgroup twiddles of the TWS forms
    u64* out;
    unsigned count;
};

template <int OP>
__global__ void __launch_bounds__(kBlock) k_probe(Args x)
{
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= x.count) return;
    const PrimeDev& p = *x.p;
    u64 r = 0;
    if constexpr (OP == OP_MUL_HI) r = mul_hi(x.a[i], x.b[i]);
    else if constexpr (OP == OP_BARRETT_MUL) r = barrett_mul(x.a[i], x.b[i], p.q, p.mu, p.k);
    else if constexpr (OP == OP_SHOUP_MUL_LAZY) r = shoup_mul_lazy(x.a[i], x.b[i], x.c[i], p.q);
    else if constexpr (OP == OP_MUL_SHOUP2) r = mul_shoup2(x.a[i], x.b[i], x.c[i], p.nq);
    else if constexpr (OP == OP_MUL_SHOUP4M) r = mul_shoup4m<false>(x.a[i], x.b[i], x.c[i], p.nq);
    else if constexpr (OP == OP_MUL_SHOUP4M_TWS) r = mul_shoup4m<true>(x.a[i], x.W[blockIdx.x], x.WP[blockIdx.x], p.nq);
    else if constexpr (OP == OP_MUL_SHOUP4M_ACC) r = mul_shoup4m_acc<false>(x.a[i], x.b[i], x.c[i], p.nq, x.d[i]);
    else if constexpr (OP == OP_MUL_SHOUP4M_ACC_TWS) r = mul_shoup4m_acc<true>(x.a[i], x.W[blockIdx.x], x.WP[blockIdx.x], p.nq, x.b[i]);
    else if constexpr (OP == OP_REDUCE_2Q) r = reduce_2q(x.a[i], p);
    else if constexpr (OP == OP_REDUCE_2Q_NEAR) r = reduce_2q_near(x.a[i], p);
    else if constexpr (OP == OP_MUL_FOLD_NEAR) r = mul_fold_near(x.a[i], x.b[i], p);
    else if constexpr (OP == OP_LIT_BARRETT_MUL) r = lit_barrett_mul(x.a[i], x.b[i], p);
    x.out[i] = r;
}

__global__ void __launch_bounds__(kBlock) k_probe_wide(Args x)
{
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= x.count) return;
    u64 lo, hi;
    mul_wide(x.a[i], x.b[i], lo, hi);
    const ulonglong2 r{lo, hi};
    reinterpret_cast<ulonglong2*>(x.out)[i] = r;        // (one store per thread; the host splits the pairs)
}

template <int OP, int HL, bool NEAR>
__global__ void __launch_bounds__(kBlock) k_probe_class(Args x)
{
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= x.count) return;
    const PrimeDev& p = *x.p;
    u64 r;
    if constexpr (OP == OP_CANON_FWD) r = canon_after_forward<HL, NEAR>(x.a[i], p);
    else if constexpr (OP == OP_CANON_INV) r = canon_after_inverse<HL, NEAR>(x.a[i], p);
    else r = FusedMul<HL, NEAR>::mul(x.a[i], x.b[i], p);
    x.out[i] = r;
}

template <int OP>
void launch_plain(const Args& x, unsigned blocks) { k_probe<OP><<<dim3(blocks), dim3(kBlock)>>>(x); }

template <int OP, int HL, bool NEAR>
void launch_class_one(const Args& x, unsigned blocks) { k_probe_class<OP, HL, NEAR><<<dim3(blocks), dim3(kBlock)>>>(x); }

template <int OP>
bool launch_class(int hl, bool near, const Args& x, unsigned blocks)
{
#define LAZY_PROBE_CLASS(H, N) if (hl == H && near == N) { launch_class_one<OP, H, N>(x, blocks); return true; }
    LAZY_PROBE_CLASS(6, true) LAZY_PROBE_CLASS(5, true) LAZY_PROBE_CLASS(4, true) LAZY_PROBE_CLASS(3, true) LAZY_PROBE_CLASS(2, true)
    LAZY_PROBE_CLASS(6, false) LAZY_PROBE_CLASS(4, false) LAZY_PROBE_CLASS(3, false) LAZY_PROBE_CLASS(2, false)
    LAZY_PROBE_CLASS(HL_LIT, false)
#undef LAZY_PROBE_CLASS
    return false;
}

// ---- policy -------------------------------------------------------------------------------------
template <int LOGN, int HL>
void print_policy_one(bool& first)
{
    constexpr InvPolicy<LOGN, HL> pol{};
    std::printf("%s\n  {\"logn\": %d, \"hl\": %d, \"tq\": %d, \"fwd_mask\": %u, \"inv_mask\": %u, \"cmul\": [", first ? "" : ",", LOGN, HL,
                Lazy<HL>::TQ, fwd_reduce_mask<LOGN, HL>(), pol.mask);
    for (int s = 0; s < LOGN; s++) std::printf("%s%d", s ? ", " : "", pol.cmul[s]);
    std::printf("]}");
    first = false;
}
template <int LOGN>
void print_policy_logn(bool& first)
{
    print_policy_one<LOGN, 2>(first);
    print_policy_one<LOGN, 3>(first);
    print_policy_one<LOGN, 4>(first);
    print_policy_one<LOGN, 5>(first);
    print_policy_one<LOGN, 6>(first);
}
int policy()
{
    bool first = true;
    std::printf("{\"policy\": [");
    print_policy_logn<11>(first);
    print_policy_logn<12>(first);
    print_policy_logn<13>(first);
    print_policy_logn<14>(first);
    print_policy_logn<15>(first);
    std::printf("\n ],\n \"hl_lit\": %d, \"hl_lit_exact\": %d, \"block\": %u,\n \"classes\": [", HL_LIT, HL_LIT_EXACT, kBlock);
    for (size_t i = 0; i < sizeof(kClasses) / sizeof(kClasses[0]); i++)
        std::printf("%s[%d, %s]", i ? ", " : "", kClasses[i].hl, kClasses[i].near ? "true" : "false");
    std::printf("]}\n");
    return 0;
}

int consts(const char* qs, const char* ks)
{
    const u64 q = std::strtoull(qs, nullptr, 10);
    const u32 k = (u32)std::strtoul(ks, nullptr, 10);
    if (k < 34 || k > 62 || (q >> (k - 1)) != 1) {
        std::fprintf(stderr, "lazy_probe: q must have exactly k bits, 34 <= k <= 62 (the range `run` takes)\n");
        return 2;
    }
    PrimeDev d{};
    const bool near_ok = prime_reduction_constants(d, q, k);
    std::printf("{\"nq\": %llu, \"red_sh1\": %u, \"red_sh2\": %u, \"red_c\": %u, \"delta\": %u, \"near_sh\": %u, \"near_mask\": %u, \"near_ok\": %s}\n",
                d.nq, d.red_sh1, d.red_sh2, d.red_c, d.delta, d.near_sh, d.near_mask, near_ok ? "true" : "false");
    return 0;
}

// ---- run ----------------------------------------------------------------------------------------
struct Record {
    int op, hl;
    bool near;
    u64 q, mu;
    u32 k;
    unsigned count, blocks;
    size_t arr[6];           // word offsets of the operand arrays inside the file image (tuple arrays first, then W, WP)
    size_t out_words, out_off;      // out_off: even, so that mul_wide's 16-byte stores are aligned
};

bool fail(const char* what)
{
    std::fprintf(stderr, "lazy_probe: %s\n", what);
    return false;
}

bool parse(const std::vector<u64>& f, std::vector<Record>& recs)
{
    if (f.size() < 2 || f[0] != kMagic) return fail("bad magic");
    const u64 nrec = f[1];
    if (nrec > 4096) return fail("too many records");
    size_t pos = 2;
    for (u64 r = 0; r < nrec; r++) {
        if (f.size() - pos < 8) return fail("truncated record header");
        Record R{};
        const u64 op = f[pos], hl = f[pos + 1], near = f[pos + 2], count = f[pos + 6], arrays = f[pos + 7];
        R.q = f[pos + 3];
        const u64 k = f[pos + 4];
        R.mu = f[pos + 5];
        pos += 8;
        if (op >= OP_COUNT) return fail("unknown op");
        if (near > 1) return fail("NEAR must be 0 or 1");
        if (count == 0 || count > kMaxCount) return fail("count out of range");
        if (k < 34 || k > 62 || (R.q >> (k - 1)) != 1 || !(R.q & 1)) return fail("q must be odd with exactly k bits, 34 <= k <= 62");
        const OpShape sh = kShape[op];
        if (arrays != (u64)(sh.tuple_arrays + sh.block_arrays)) return fail("wrong number of arrays for this op");
        R.op = (int)op;
        R.hl = (int)hl;
        R.near = near != 0;
        R.k = (u32)k;
        R.count = (unsigned)count;
        R.blocks = (R.count + kBlock - 1) / kBlock;
        if (op == OP_LIT_BARRETT_MUL && k > 61) return fail("lit_barrett_mul serves 34 ... 61 bits");
        if (sh.classed) {
            bool ok = false;
            for (const ClassId& c : kClasses) ok = ok || (c.hl == R.hl && c.near == R.near);
            if (!ok) return fail("(HL, NEAR) is not an instantiated class");
            if (R.hl != HL_LIT && (int)(64 - k) < R.hl) return fail("modulus too wide for this headroom class");
        }
        for (int a = 0; a < sh.tuple_arrays + sh.block_arrays; a++) {
            if (f.size() - pos < 1) return fail("truncated array header");
            const u64 len = f[pos++];
            const u64 want = a < sh.tuple_arrays ? R.count : R.blocks;
            if (len != want) return fail("array length does not match count");
            if (f.size() - pos < len) return fail("truncated array");
            R.arr[a] = pos;
            pos += len;
        }
        R.out_words = (size_t)R.count * (op == OP_MUL_WIDE ? 2 : 1);
        recs.push_back(R);
    }
    if (pos != f.size()) return fail("trailing words");
    return true;
}

#define HIP_OK(e)                                                                                     \
    do {                                                                                              \
        const hipError_t err__ = (e);                                                                 \
        if (err__ != hipSuccess) {                                                                    \
            std::fprintf(stderr, "lazy_probe: %s: %s\n", #e, hipGetErrorString(err__));               \
            return 3;                                                                                 \
        }                                                                                             \
    } while (0)

int run(const char* in, const char* outp)
{
    std::vector<u64> f;
    {
        FILE* fp = std::fopen(in, "rb");
        if (!fp) return fail("cannot open input"), 2;
        std::fseek(fp, 0, SEEK_END);
        const long bytes = std::ftell(fp);
        std::fseek(fp, 0, SEEK_SET);
        if (bytes < 16 || bytes % 8 != 0 || bytes > (1L << 30)) {
            std::fclose(fp);
            return fail("input size"), 2;
        }
        f.resize((size_t)bytes / 8);
        const size_t got = std::fread(f.data(), 8, f.size(), fp);
        std::fclose(fp);
        if (got != f.size()) return fail("short read"), 2;
    }
    std::vector<Record> recs;
    if (!parse(f, recs)) return 2;

    // host-side class checks that need the derived constants
    std::vector<PrimeDev> pd(recs.size());
    size_t total_out = 0;
    for (size_t r = 0; r < recs.size(); r++) {
        Record& R = recs[r];
        PrimeDev& d = pd[r];
        std::memset(&d, 0, sizeof(d));
        d.q = R.q;
        d.mu = R.mu;
        d.k = R.k;
        const bool near_ok = prime_reduction_constants(d, R.q, R.k);
        if ((kShape[R.op].near_only || (kShape[R.op].classed && R.near)) && !near_ok) return fail("near-2^k form on a modulus without that shape"), 2;
        recs[r].out_off = total_out;
        total_out += (R.out_words + 1) & ~(size_t)1;
    }

    u64 *d_in = nullptr, *d_out = nullptr;
    PrimeDev* d_pd = nullptr;
    HIP_OK(hipMalloc((void**)&d_in, f.size() * 8));
    HIP_OK(hipMalloc((void**)&d_out, total_out * 8));
    HIP_OK(hipMalloc((void**)&d_pd, pd.size() * sizeof(PrimeDev)));
    HIP_OK(hipMemcpy(d_in, f.data(), f.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_pd, pd.data(), pd.size() * sizeof(PrimeDev), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xee, total_out * 8));

    for (size_t r = 0; r < recs.size(); r++) {
        const Record& R = recs[r];
        const OpShape sh = kShape[R.op];
        Args x{};
        x.p = d_pd + r;
        const u64* tup[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int a = 0; a < sh.tuple_arrays; a++) tup[a] = d_in + R.arr[a];
        x.a = tup[0]; x.b = tup[1]; x.c = tup[2]; x.d = tup[3];
        if (sh.block_arrays) {
            x.W = d_in + R.arr[sh.tuple_arrays];
            x.WP = d_in + R.arr[sh.tuple_arrays + 1];
        }
        x.out = d_out + R.out_off;
        x.count = R.count;
        switch (R.op) {
        case OP_MUL_HI: launch_plain<OP_MUL_HI>(x, R.blocks); break;
        case OP_MUL_WIDE: k_probe_wide<<<dim3(R.blocks), dim3(kBlock)>>>(x); break;
        case OP_BARRETT_MUL: launch_plain<OP_BARRETT_MUL>(x, R.blocks); break;
        case OP_SHOUP_MUL_LAZY: launch_plain<OP_SHOUP_MUL_LAZY>(x, R.blocks); break;
        case OP_MUL_SHOUP2: launch_plain<OP_MUL_SHOUP2>(x, R.blocks); break;
        case OP_MUL_SHOUP4M: launch_plain<OP_MUL_SHOUP4M>(x, R.blocks); break;
        case OP_MUL_SHOUP4M_TWS: launch_plain<OP_MUL_SHOUP4M_TWS>(x, R.blocks); break;
        case OP_MUL_SHOUP4M_ACC: launch_plain<OP_MUL_SHOUP4M_ACC>(x, R.blocks); break;
        case OP_MUL_SHOUP4M_ACC_TWS: launch_plain<OP_MUL_SHOUP4M_ACC_TWS>(x, R.blocks); break;
        case OP_REDUCE_2Q: launch_plain<OP_REDUCE_2Q>(x, R.blocks); break;
        case OP_REDUCE_2Q_NEAR: launch_plain<OP_REDUCE_2Q_NEAR>(x, R.blocks); break;
        case OP_MUL_FOLD_NEAR: launch_plain<OP_MUL_FOLD_NEAR>(x, R.blocks); break;
        case OP_LIT_BARRETT_MUL: launch_plain<OP_LIT_BARRETT_MUL>(x, R.blocks); break;
        case OP_CANON_FWD: if (!launch_class<OP_CANON_FWD>(R.hl, R.near, x, R.blocks)) return 2; break;
        case OP_CANON_INV: if (!launch_class<OP_CANON_INV>(R.hl, R.near, x, R.blocks)) return 2; break;
        case OP_FUSED_MUL: if (!launch_class<OP_FUSED_MUL>(R.hl, R.near, x, R.blocks)) return 2; break;
        default: return 2;
        }
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());          // each kernel is checked before the next one starts
    }
    std::vector<u64> raw(total_out), out;
    HIP_OK(hipMemcpy(raw.data(), d_out, total_out * 8, hipMemcpyDeviceToHost));
    for (const Record& R : recs) {
        const u64* t = raw.data() + R.out_off;
        if (R.op == OP_MUL_WIDE) {               // pairs {lo, hi} -> count low words, then count high words
            for (unsigned i = 0; i < R.count; i++) out.push_back(t[2 * (size_t)i]);
            for (unsigned i = 0; i < R.count; i++) out.push_back(t[2 * (size_t)i + 1]);
        } else {
            out.insert(out.end(), t, t + R.out_words);
        }
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_pd);
    FILE* fo = std::fopen(outp, "wb");
    if (!fo) return fail("cannot open output"), 2;
    const size_t put = std::fwrite(out.data(), 8, out.size(), fo);
    if (std::fclose(fo) != 0 || put != out.size()) return fail("short write"), 2;
    std::printf("lazy_probe: %zu records, %zu words\n", recs.size(), out.size());
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "policy") return policy();
    if (argc == 4 && std::string(argv[1]) == "consts") return consts(argv[2], argv[3]);
    if (argc == 4 && std::string(argv[1]) == "run") return run(argv[2], argv[3]);
    std::fprintf(stderr, "usage: lazy_probe policy | consts Q K | run IN OUT\n");
    return 2;
}
