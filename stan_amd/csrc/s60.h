// s60.h -- the lossless 60-bit value stream's number format, shared by who writes it (matrix_streams.hip: k_to_s60) and who
// reads it (spmv_kernels.inc: load9).  After the Jacobi scaling every entry of an SPD matrix satisfies |a| <= 1, so the
// eleven exponent bits of an fp64 carry four that never change: an entry travels as
//   sign (1 bit) | exponent code (7 bits) | the 52 mantissa bits, unchanged
// with code 0 = +-0.0 (the sign kept) and codes 1 ... 127 = the unbiased exponents -126 ... 0 (fp64 exponent field =
// code + 896).  Encodable: a == +-0, or 2^-126 <= |a| < 2; everything else (|a| >= 2, |a| < 2^-126 with the subnormals,
// Inf, NaN) is REFUSED, and one refused entry refuses the stream for the whole matrix.  Nothing here is floating-point
// arithmetic: the decoded double is the stored double bit for bit.
// A slot's block of 64 rows x 9 entries is vals60[slot][17][64] dwords: rows 0 ... 8 the low 32 bits of the nine entries,
// rows 9 ... 16 the nine 28-bit high parts, packed back to back into eight dwords (252 of 256 bits).
// Plain C++ as well as HIP: the host-side check of this arithmetic compiles this file with a sanitizer.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define S60_FN __host__ __device__ __forceinline__
#define S60_UNROLL _Pragma("unroll")
#else
#define S60_FN inline
#define S60_UNROLL
#endif

constexpr int S60_ROWS = 17;             // dwords per entry column of a slot (fp64: 18, FIXED-48: 14)
constexpr uint32_t S60_EXP_BIAS = 896;   // fp64 exponent field = code + 896

// the bits of a double -> low dword and 28-bit high part; false: refused (the code written is +0.0)
S60_FN bool s60_encode(uint64_t bits, uint32_t *lo, uint32_t *hi28) {
    const uint32_t hw = (uint32_t)(bits >> 32), lw = (uint32_t)bits;
    const uint32_t sign = hw >> 31, ef = (hw >> 20) & 0x7ffu, mh = hw & 0xfffffu;
    if (ef == 0 && mh == 0 && lw == 0) { *lo = 0; *hi28 = sign << 27; return true; }   // +-0.0
    if (ef <= S60_EXP_BIAS || ef > S60_EXP_BIAS + 127) { *lo = 0; *hi28 = 0; return false; }
    *lo = lw;
    *hi28 = (sign << 27) | ((ef - S60_EXP_BIAS) << 20) | mh;
    return true;
}
// ... and back: one add for the exponent, one select for zero
S60_FN uint64_t s60_decode(uint32_t lo, uint32_t hi28) {
    const uint32_t rest = hi28 & 0x7ffffffu;   // code << 20 | the mantissa's high 20 bits
    const uint32_t hw = ((hi28 & 0x8000000u) << 4) | ((rest >> 20) != 0 ? rest + (S60_EXP_BIAS << 20) : 0u);
    return ((uint64_t)hw << 32) | lo;
}
// the nine high parts <-> eight dwords; entry j sits at bit 28 j of the 256 (offsets known at compile time once unrolled)
S60_FN void s60_pack_high(const uint32_t h[9], uint32_t w[8]) {
    S60_UNROLL
    for (int m = 0; m < 8; m++) w[m] = 0;
    S60_UNROLL
    for (int j = 0; j < 9; j++) {
        const int d = (28 * j) >> 5, o = (28 * j) & 31;
        w[d] |= h[j] << o;
        if (o > 4) w[d + 1] |= h[j] >> (32 - o);   // (o > 4: the part does not end inside dword d; then d + 1 <= 7)
    }
}
S60_FN uint32_t s60_high(const uint32_t w[8], int j) {
    const int d = (28 * j) >> 5, o = (28 * j) & 31;
    uint32_t h = w[d] >> o;
    if (o > 4) h |= w[d + 1] << (32 - o);
    return h & 0xfffffffu;
}
