/*
 * ref_shift.h -- 64-bit shifts by a count of 64 or more, as the reference's own platform performs them (test infrastructure; ours).
 *
 * The reference's uint128.h shifts 64-bit words by run-time counts that reach 64: shiftr(x, qbit + 2) in singleBarrett at
 * qbit = 62, and `64 - shift` at shift = 0.  C++ leaves such a shift undefined.  The reference's device code gets PTX's shl / shr,
 * which clamp: a count of 64 or more gives 0, and its 62-bit Barrett is exact because of that.  gfx950's shift instructions take
 * the count modulo 64 instead, so the same source returns other words there: every word of a transform on a 62-bit modulus.
 * The port recipe (ref_port.py) therefore routes the shifts of
 * uint128.h's three shift members -- and nothing else -- through these two helpers, which clamp in device code and leave host code
 * as the host compiler makes it, as on the reference's platform.  The harness op `selfcheck_shift` checks the three members on
 * the device against Python integers.
 */
#ifndef REF_SHIFT_H
#define REF_SHIFT_H

__host__ __device__ __forceinline__ unsigned long long ref_shr64(unsigned long long x, unsigned s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return s >= 64 ? 0ull : x >> s;
#else
    return x >> s;
#endif
}

__host__ __device__ __forceinline__ unsigned long long ref_shl64(unsigned long long x, unsigned s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return s >= 64 ? 0ull : x << s;
#else
    return x << s;
#endif
}

#endif
