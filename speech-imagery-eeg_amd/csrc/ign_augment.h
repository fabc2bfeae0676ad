// Training augmentation of a (B, T, C) fp32 batch: ONE definition of every random decision, for the kernel (ign_augment.hip), host
// code and the numpy restatement (utils/augment.py) that the tests compare against.  Usable from __device__ and host code.
//
// Sample b has len_b time steps of data (len_b = T without lengths; clamped to 0..T) and padding behind them.  With n = len_b:
//   out[b,t,c] = keepC[b,c] * keepT[b,t] * (a[b,c] * x[b, (t - s_b) mod n, c] + sigma * n[b,t,c])    for t <  n
//   out[b,t,c] = x[b,t,c]                                                                         for t >= n  (no noise)
// keepC / keepT are selections (a dropped value is +0, nothing is rescaled); the products and the sum are separate fp32 roundings
// (the library is built with -ffp-contract=off and this header holds no fmaf), and sigma == 0 skips the noise term altogether, so a
// float32 restatement is bitwise equal whenever sigma == 0.
//
// Every draw is Philox4x32-10 (ign_dropout.h) under key = the 64-bit per-call seed (low word first).  The last counter word is a
// tag per kind of draw and every transform reads a word of its own, so a draw is a pure function of (seed, b), (seed, b, c) or
// (seed, b, t, c): it does not depend on launch geometry, on B, or on which transforms are on.
//   per sample   counter (b, 0, 0, IGN_AUG_TAG_SAMPLE) -> words x0, x1, x2
//     shift      S = min(floor(shift * n), n - 1) (fp32 product), s_b = x0 mod (2 S + 1) - S, uniform in [-S, S].  Modulo bias:
//                a value is favoured by at most (2 S + 1) / 2^32, below 2^-20 for T < 2048 (any series this project trains on).
//     time mask  one span: M = min(floor(time_mask * n), n), length m = x1 mod (M + 1), start = x2 mod (n - m + 1);
//                keepT[b,t] = 0 for start <= t < start + m.  The span never leaves [0, n).
//   per channel  counter (b, c, 0, IGN_AUG_TAG_CHANNEL) -> words x0, x1
//     amplitude  a[b,c] = 1 + scale * (2 u - 1), u = (x0 >> 8) * 2^-24 (24-bit uniform, exact in fp32; 2 u - 1 is exact too).
//                scale < 1 keeps a > 0.  The shapelet expert's instance norm cancels a per-channel gain: this term is there for
//                the FCN / ResNet / EEG-CNN / Transformer side.
//     electrode  keepC[b,c] <=> (x1 & 0xffff) >= thr, thr = round(p * 65536): the rule of ign_dropout_threshold.
//   noise        counter (e >> 2, 0, b, IGN_AUG_TAG_NOISE), e = t * C + c the flat index inside the sample: one call serves the
//                four consecutive flat indices of a quad (quads may straddle rows).  Box-Muller on 24-bit uniforms:
//                u1 = ((w0 >> 8) + 1) * 2^-24 in (0, 1], u2 = (w1 >> 8) * 2^-24 in [0, 1), r = sqrtf(-2 logf(u1)), th = 2 pi u2,
//                (r cos(th), r sin(th)) from one sincosf; words (x0, x1) give elements 0, 1 of the quad and (x2, x3) elements 2, 3.  The
//                precise logf / sqrtf / sincosf, not the fast intrinsics.  |n| <= sqrt(48 ln 2) = 5.77 (u1 >= 2^-24).
// Edge cases: n = 0 copies the row through; n = 1 forces S = M = 0 (both rates are below 1).
#pragma once
#include "ign_dropout.h"

#define IGN_AUG_TAG_SAMPLE  0u
#define IGN_AUG_TAG_CHANNEL 1u
#define IGN_AUG_TAG_NOISE   2u
#define IGN_AUG_TWO_PI      6.28318530717958647692f

// what one sample draws: the shift as a forward rotation sh = s_b mod n in [0, n), and the masked span [m0, m1)
struct IgnAugSample { int sh, m0, m1; };

IGN_DROP_FN IgnAugSample ign_aug_sample(uint64_t seed, uint32_t b, int n, float shift, float time_mask) {
    IgnAugSample o = {0, 0, 0};
    if (n < 1) return o;
    const IgnPhilox4 x = ign_philox4x32_10(b, 0u, 0u, IGN_AUG_TAG_SAMPLE, (uint32_t)seed, (uint32_t)(seed >> 32));
    int S = (int)floorf(shift * (float)n), M = (int)floorf(time_mask * (float)n);
    S = S < n - 1 ? S : n - 1;
    M = M < n ? M : n;
    const int s = (int)(x.x0 % (uint32_t)(2 * S + 1)) - S;
    o.sh = s < 0 ? s + n : s;
    const int m = (int)(x.x1 % (uint32_t)(M + 1));
    o.m0 = (int)(x.x2 % (uint32_t)(n - m + 1));
    o.m1 = o.m0 + m;
    return o;
}

// what one (sample, channel) draws: the gain a[b,c] and whether the electrode is kept
struct IgnAugChannel { float a; bool keep; };

IGN_DROP_FN IgnAugChannel ign_aug_channel(uint64_t seed, uint32_t b, uint32_t c, float scale, uint32_t chan_thr) {
    const IgnPhilox4 x = ign_philox4x32_10(b, c, 0u, IGN_AUG_TAG_CHANNEL, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u = (float)(x.x0 >> 8) * 0x1p-24f;
    const float d = 2.0f * u - 1.0f;
    IgnAugChannel o;
    o.a = 1.0f + scale * d;
    o.keep = (x.x1 & 0xffffu) >= chan_thr;
    return o;
}

IGN_DROP_FN void ign_aug_box_muller(uint32_t w0, uint32_t w1, float* n0, float* n1) {
    const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(w1 >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    const float th = IGN_AUG_TWO_PI * u2;
    float sn, cs;
    sincosf(th, &sn, &cs);
    *n0 = r * cs;
    *n1 = r * sn;
}

// the four standard normals of quad q (flat indices 4 q .. 4 q + 3) of sample b
IGN_DROP_FN void ign_aug_noise4(uint64_t seed, uint32_t b, uint32_t q, float n[4]) {
    const IgnPhilox4 x = ign_philox4x32_10(q, 0u, b, IGN_AUG_TAG_NOISE, (uint32_t)seed, (uint32_t)(seed >> 32));
    ign_aug_box_muller(x.x0, x.x1, &n[0], &n[1]);
    ign_aug_box_muller(x.x2, x.x3, &n[2], &n[3]);
}

// one element (the definition the kernel implements): xs = x[b, (t - s_b) mod n, c] for t < n
IGN_DROP_FN float ign_aug_apply(float xs, float a, bool keep, float sigma, float noise) {
    float v = a * xs;
    if (sigma != 0.0f) {
        const float z = sigma * noise;
        v = v + z;
    }
    return keep ? v : 0.0f;
}
