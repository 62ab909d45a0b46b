/*
 * ref_proto.h -- request / response files of the reference harnesses (test infrastructure; ours).
 *
 * Everything is a little-endian u64.  Byte and 32-bit payloads are packed into u64 words, zero padded.
 *
 *   request :  REF_REQ_MAGIC, ncases, then per case
 *                op, n, nq, nargs, nwords,
 *                nq x (q, mu, qbit, psi)      -- psi = 0: no twiddle tables wanted for this modulus
 *                nargs scalar arguments
 *                nwords input words
 *   response:  REF_RSP_MAGIC, ncases, then per case
 *                nwords, nwords output words
 *
 * One process per invocation: `ref60 REQUEST.bin RESPONSE.bin`.  Exit status 0 only if every case ran and every
 * HIP call returned hipSuccess; the response is written only then.  oracle/ref_py.py is the Python side.
 */
#ifndef REF_PROTO_H
#define REF_PROTO_H

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef unsigned long long u64;

#define REF_REQ_MAGIC 0x3151455246455221ULL
#define REF_RSP_MAGIC 0x3150535246455221ULL

struct RefModulus { u64 q, mu, qbit, psi; };

struct RefCase {
    u64 op, n;
    std::vector<RefModulus> mod;
    std::vector<u64> args, in, out;
};

#define REF_DIE(...) do { fprintf(stderr, "ref harness: " __VA_ARGS__); fprintf(stderr, "\n"); exit(2); } while (0)
#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) REF_DIE("%s -> %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

static std::vector<RefCase> ref_read_request(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) REF_DIE("cannot open %s", path);
    fseek(f, 0, SEEK_END);
    long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 16 || bytes % 8) REF_DIE("%s: not a whole number of words", path);
    std::vector<u64> w(bytes / 8);
    if (fread(w.data(), 8, w.size(), f) != w.size()) REF_DIE("short read on %s", path);
    fclose(f);
    if (w[0] != REF_REQ_MAGIC) REF_DIE("%s: bad magic", path);
    size_t at = 2;
    std::vector<RefCase> cases(w[1]);
    for (RefCase& c : cases) {
        if (at + 5 > w.size()) REF_DIE("truncated case header");
        c.op = w[at]; c.n = w[at + 1];
        u64 nq = w[at + 2], nargs = w[at + 3], nwords = w[at + 4];
        at += 5;
        if (nq > 16 || at + 4 * nq + nargs + nwords > w.size()) REF_DIE("truncated case body");
        c.mod.resize(nq);
        for (RefModulus& m : c.mod) { m.q = w[at]; m.mu = w[at + 1]; m.qbit = w[at + 2]; m.psi = w[at + 3]; at += 4; }
        c.args.assign(w.begin() + at, w.begin() + at + nargs); at += nargs;
        c.in.assign(w.begin() + at, w.begin() + at + nwords); at += nwords;
    }
    if (at != w.size()) REF_DIE("trailing words in %s", path);
    return cases;
}

static void ref_write_response(const char* path, const std::vector<RefCase>& cases)
{
    FILE* f = fopen(path, "wb");
    if (!f) REF_DIE("cannot create %s", path);
    u64 head[2] = { REF_RSP_MAGIC, (u64)cases.size() };
    fwrite(head, 8, 2, f);
    for (const RefCase& c : cases) {
        u64 nw = c.out.size();
        fwrite(&nw, 8, 1, f);
        if (nw && fwrite(c.out.data(), 8, nw, f) != nw) REF_DIE("short write on %s", path);
    }
    if (fclose(f)) REF_DIE("close failed on %s", path);
}

#endif
