/*
 * ref_shim.h -- the only two FUNCTIONS of the reference's arithmetic that are ours (test infrastructure).  (ref_shift.h, next to
 * this file, is the one other place: what a 64-bit shift by a count of 64 gives.)
 *
 * The reference writes its 128-bit subtract and its 64x64->128 product in inline PTX (the last two functions of
 * its uint128.h).  PTX does not exist on gfx950, so the port recipe (ref_port.py) cuts those two definitions out
 * of the translated copy of that header and includes this file in their place.  Both are restated in plain C++
 * on unsigned __int128 with the reference's signatures; everything else under oracle/_ref/src is the reference's
 * own text after mechanical translation.  The harness op `selfcheck` runs these two on the device against Python
 * integers before any other comparison is believed.
 */
#ifndef REF_SHIM_H
#define REF_SHIM_H

/* a -= b over 128 bits, wrapping (borrow propagated from the low into the high word) */
__device__ __forceinline__ void sub128(uint128_t& a, const uint128_t& b)
{
    unsigned __int128 x = ((unsigned __int128)a.high << 64) | a.low;
    unsigned __int128 y = ((unsigned __int128)b.high << 64) | b.low;
    x -= y;
    a.low = (unsigned long long)x;
    a.high = (unsigned long long)(x >> 64);
}

/* c = a * b, all 128 bits.  a or b may alias a word of c (callers pass c.low as a): the product is formed first */
__device__ __forceinline__ void mul64(const unsigned long long& a, const unsigned long long& b, uint128_t& c)
{
    unsigned __int128 p = (unsigned __int128)a * b;
    c.low = (unsigned long long)p;
    c.high = (unsigned long long)(p >> 64);
}

#endif
