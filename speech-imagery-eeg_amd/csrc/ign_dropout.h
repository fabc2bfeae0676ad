// Attention-dropout keep mask: ONE definition for every attention kernel (forward, dQ, dK / dV, all arithmetics), the mask-dump
// entry point ign_attn_dropout_mask and the host (tests restate it in numpy).  Usable from __device__ and host code.
//
// The keep decision for score element (batch b, head h, query i, key j) of a call is a pure function of
// (seed, b * H + h, i, j, thr): it does not depend on tile sizes, launch geometry, the kernel or the arithmetic.
//   * generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; the Random123 constants), key = the 64-bit per-call seed
//     (low word first), counter = (i >> 2, j >> 2, b * H + h, c);
//   * 4 x 4 blocks: block (i >> 2, j >> 2) takes its 16 halfwords from the two calls c = 0, 1; element (i, j) reads halfword
//     n = (i & 3) * 4 + (j & 3) -- call n >> 3, word (n & 7) >> 1, low half for even n, high half for odd n;
//   * keep <=> halfword >= thr, thr = round(p * 65536) (p_eff = thr / 65536, accurate to 2^-16); kept values are scaled by
//     s = 65536 / (65536 - thr), so the output is unbiased for the rate actually used.
// A lane of the forward / dQ kernels holds 4 consecutive keys of one query: one call per 4 elements (ign_drop_row4).  A lane of
// the dK / dV kernels holds 4 consecutive queries of one key: both calls per 4 elements (ign_drop_col4).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define IGN_DROP_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#define IGN_DROP_FN static inline
#endif

#define IGN_PHILOX_M0 0xD2511F53u
#define IGN_PHILOX_M1 0xCD9E8D57u
#define IGN_PHILOX_W0 0x9E3779B9u
#define IGN_PHILOX_W1 0xBB67AE85u

struct IgnPhilox4 { uint32_t x0, x1, x2, x3; };

// Philox4x32-10 of counter (c0, c1, c2, c3) under key (k0, k1).  The round keys depend on the seed only: in a kernel they are
// wave-uniform (scalar registers); the per-lane work is two 32x32 -> 64-bit products and four XORs per round.
IGN_DROP_FN IgnPhilox4 ign_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)IGN_PHILOX_M0 * c0, p1 = (uint64_t)IGN_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += IGN_PHILOX_W0; k1 += IGN_PHILOX_W1;
    }
    IgnPhilox4 o = {c0, c1, c2, c3};
    return o;
}

// thr = round(p * 65536) (p * 65536 is exact in fp32; rintf rounds half to even); the caller rejects p outside [0, 1) and
// thr == 65536
IGN_DROP_FN uint32_t ign_dropout_threshold(float p) { return (uint32_t)rintf(p * 65536.0f); }
// s = 65536 / (65536 - thr), one correctly rounded fp32 division (computed on the host and passed to the kernels)
IGN_DROP_FN float ign_dropout_scale(uint32_t thr) { return 65536.0f / (float)(65536u - thr); }

IGN_DROP_FN uint32_t ign_drop_keep2(uint32_t w, uint32_t thr) {       // bit 0: low halfword kept, bit 1: high halfword kept
    return (uint32_t)((w & 0xffffu) >= thr) | ((uint32_t)((w >> 16) >= thr) << 1);
}

// keep bits of keys j4 .. j4 + 3 (j4 % 4 == 0) of query i: bit t <-> key j4 + t.  One Philox call.
IGN_DROP_FN uint32_t ign_drop_row4(uint64_t seed, uint32_t bh, uint32_t i, uint32_t j4, uint32_t thr) {
    const IgnPhilox4 x = ign_philox4x32_10(i >> 2, j4 >> 2, bh, (i >> 1) & 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const bool odd = i & 1u;                                              // halfwords 4 (i & 1) .. +3 of the call
    return ign_drop_keep2(odd ? x.x2 : x.x0, thr) | (ign_drop_keep2(odd ? x.x3 : x.x1, thr) << 2);
}

// keep bits of queries i4 .. i4 + 3 (i4 % 4 == 0) of key j: bit t <-> query i4 + t.  Two Philox calls.
IGN_DROP_FN uint32_t ign_drop_col4(uint64_t seed, uint32_t bh, uint32_t i4, uint32_t j, uint32_t thr) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const IgnPhilox4 x = ign_philox4x32_10(i4 >> 2, j >> 2, bh, 0u, k0, k1);
    const IgnPhilox4 y = ign_philox4x32_10(i4 >> 2, j >> 2, bh, 1u, k0, k1);
    const bool hiw = j & 2u;                                              // word (j & 3) >> 1 of each row's pair
    const uint32_t sh = (j & 1u) * 16u;
    const uint32_t u0 = ((hiw ? x.x1 : x.x0) >> sh) & 0xffffu, u1 = ((hiw ? x.x3 : x.x2) >> sh) & 0xffffu;
    const uint32_t u2 = ((hiw ? y.x1 : y.x0) >> sh) & 0xffffu, u3 = ((hiw ? y.x3 : y.x2) >> sh) & 0xffffu;
    return (uint32_t)(u0 >= thr) | ((uint32_t)(u1 >= thr) << 1) | ((uint32_t)(u2 >= thr) << 2) | ((uint32_t)(u3 >= thr) << 3);
}

// one element (the definition the two helpers above implement)
IGN_DROP_FN bool ign_drop_keep(uint64_t seed, uint32_t bh, uint32_t i, uint32_t j, uint32_t thr) {
    return (ign_drop_row4(seed, bh, i, j & ~3u, thr) >> (j & 3u)) & 1u;
}
