/*
 * ref_harness30.hip -- drives the reference's 30-bit kernels (old/ntt_30bit.cuh; test infrastructure; ours).
 *
 * Same protocol as ref_harness60.hip (ref_proto.h); 32-bit words travel two to a u64, low half first.  The tables
 * come from the reference's own fillTablePsi64.  One polynomial per case, as the reference launches them.
 *
 * Ops:   2 forwardNTT   3 inverseNTT   in: a (n u32)        out: a
 *        7 barrett_30bit               in: a, b (n u32 each) out: a
 *
 * Buffers: the reference's 30-bit forwardNTT launches twice the blocks its single-kernel stage needs at n = 8192,
 * 16384 and 32768; the surplus blocks load and store a[n .. 2n) and read twiddles up to index 3n/2.  The harness
 * therefore gives the data and both tables 2n words, zero beyond n, so that every access stays inside its buffer;
 * the surplus blocks never touch a[0 .. n), which is all that is returned.
 */
#include <hip/hip_runtime.h>
#include <vector>

#include "ref_proto.h"

#include "helper.h"
#include "parameter.h"
#include "ntt_30bit.cuh"

using std::vector;

struct Dev32 {
    unsigned* p = nullptr;
    Dev32(size_t words, const unsigned* src, size_t src_words)
    {
        HIP_OK(hipMalloc(&p, words * 4));
        HIP_OK(hipMemset(p, 0, words * 4));
        if (src) HIP_OK(hipMemcpy(p, src, src_words * 4, hipMemcpyHostToDevice));
    }
    ~Dev32() { (void)hipFree(p); }
    Dev32(const Dev32&) = delete;
};

static void run_case(RefCase& c, hipStream_t& s)
{
    const size_t n = c.n;
    if (n < 2048 || n > 65536 || (n & (n - 1))) REF_DIE("n = %zu is not a size the reference dispatches", n);
    if (c.mod.size() != 1) REF_DIE("one modulus per case");
    const RefModulus m = c.mod[0];
    if (m.q >> 32 || m.mu >> 32 || m.psi >> 32) REF_DIE("30-bit path: parameters must fit 32 bits");
    const unsigned* in = (const unsigned*)c.in.data();
    vector<unsigned> out(n);

    if (c.op == 2 || c.op == 3) {
        if (c.in.size() != n / 2) REF_DIE("op %llu wants n u32", c.op);
        vector<unsigned> f(n), b(n);
        fillTablePsi64((unsigned)m.psi, (unsigned)m.q, modpow64((unsigned)m.psi, (unsigned)m.q - 2, (unsigned)m.q), f.data(), b.data(), (unsigned)n);
        Dev32 a(2 * n, in, n), psi(2 * n, f.data(), n), psiinv(2 * n, b.data(), n);
        if (c.op == 2) forwardNTT(a.p, (unsigned)n, s, (unsigned)m.q, (unsigned)m.mu, (int)m.qbit, psi.p);
        else inverseNTT(a.p, (unsigned)n, s, (unsigned)m.q, (unsigned)m.mu, (int)m.qbit, psiinv.p);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), a.p, n * 4, hipMemcpyDeviceToHost));
    } else if (c.op == 7) {
        if (c.in.size() != n) REF_DIE("op 7 wants 2n u32");
        Dev32 a(n, in, n), b(n, in + n, n);
        barrett_30bit<<<n / 256, 256, 0, s>>>(a.p, b.p, (unsigned)m.q, (unsigned)m.mu, (int)m.qbit);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), a.p, n * 4, hipMemcpyDeviceToHost));
    } else {
        REF_DIE("unknown op %llu", c.op);
    }
    HIP_OK(hipGetLastError());
    c.out.resize(n / 2);
    memcpy(c.out.data(), out.data(), n * 4);
}

int main(int argc, char** argv)
{
    if (argc != 3) REF_DIE("usage: %s REQUEST.bin RESPONSE.bin", argv[0]);
    vector<RefCase> cases = ref_read_request(argv[1]);
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    for (RefCase& c : cases) run_case(c, s);
    HIP_OK(hipDeviceSynchronize());
    ref_write_response(argv[2], cases);
    return 0;
}
