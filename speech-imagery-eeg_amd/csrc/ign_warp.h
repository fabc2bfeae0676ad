// Time, magnitude and window warping of a (B, T, C) fp32 training batch: ONE definition of the map, for the kernel (ign_warp.hip),
// host code (ign_warp_map) and the numpy restatement (utils/warp.py) that the tests compare against.  Usable from __device__ and
// host code.  The library is built with -ffp-contract=off and this header holds no fmaf and none of expf / logf / sinf: every
// product, sum and quotient below is one fp32 rounding (the quotients IEEE-correct), so a float32 restatement is bitwise equal.
//
// Sample b has n = len_b time steps of data (T without lengths; clamped to 0..T) and padding behind them.  K = knots interior knots
// (1..8), seg = K + 1; control points i = 0 .. K + 1 sit at equal spacing over [0, n - 1] (knot coordinate u = t * seg / (n - 1)).
//
// Draws: Philox4x32-10 (ign_dropout.h) under key = the 64-bit per-call seed (low word first), last counter word IGN_WARP_TAG = 3
// (0..2 are ign_augment.h's; the attention dropout's counters carry a head index in word 2 and 0 / 1 in word 3).
//   counter (b, 0, 0, 3) -> x0, x1, x2: the sample is warped iff (x0 >> 8) * 2^-24 < prob, else copied bit for bit;
//                                        x1 = window start draw; x2 & 1 = window factor (0 -> 0.5, 1 -> 2)
//   speed knot i: word i & 3 of counter (b, 1 + (i >> 2), 0, 3);  gain knot i: word i & 3 of counter (b, 4 + (i >> 2), 0, 3)
//   u = (word >> 8) * 2^-24;  v_i = 1 + twarp * (2 u - 1);  m_i = 1 + mwarp * (2 u - 1).  Rates lie in [0, 1): v_i, m_i > 0.
// A draw is a pure function of (seed, b): not of c, B, the launch geometry, or which of the three transforms are on.
//
// Window map (wwarp = R > 0, only when n >= 3): Lw = min(max(floor(R * n), 2), n - 1), a = x1 mod (n - Lw + 1), c = 0.5 or 2,
//   Iw(t) = t + (c - 1) * clamp(t - a, 0, Lw)   (multiples of 0.5 below 2^22: exact),   pos(t) = (Iw(t) * (n - 1)) / Iw(n - 1);
//   otherwise pos(t) = t.  The window [a, a + Lw) is stretched (c = 2) or compressed (c = 0.5) and the whole rescaled to [0, n - 1].
// Smooth map (twarp > 0): the speed is piecewise linear through (i, v_i); C_0 = 0, C_{i+1} = C_i + 0.5 * (v_i + v_{i+1}) summed in
//   order; for a position p: u = (p * seg) / (n - 1), i = min(floor(u), K), f = u - i,
//   I = C_i + (f * v_i + (f * f) * (0.5 * (v_{i+1} - v_i))),   smooth(p) = (I * (n - 1)) / C_seg;   otherwise smooth(p) = p.
// Composite: phi(t) = min(max(smooth(pos(t)), 0), n - 1) for t < n - 1 and phi(n - 1) = n - 1 by definition.  The clamp is applied
//   whichever transforms are on: pos(n - 2) may round one ulp above n - 1.  Rounding is monotone and every step above is a
//   non-decreasing function of t up to roundings that are far below the step of its argument (|f| steps by >= 0.5 seg / (n - 1),
//   v_i >= 0.01 at twarp = 0.99), so phi is non-decreasing; tests/test_warp_host.py checks it over the cases.
// Resampling: i0 = min(floor(phi), n - 2), w = phi - i0, y = (w == 0) ? x[i0] : x[i0] + w * (x[i0 + 1] - x[i0])  (w == 0 is a copy: a
//   non-finite neighbour does not leak).
// Gain (mwarp > 0): u = (t * seg) / (n - 1) from the integer OUTPUT step t, i = min(floor(u), K), f = u - i,
//   g(t) = m_i + f * (m_{i+1} - m_i); one curve per sample, shared by all channels; out = g * y.  mwarp == 0: no multiplication.
// Edge cases: n < 2 copies the row; t >= n is copied through; a sample not warped by prob, and any call with all three rates 0, is
//   an exact copy with no arithmetic.  IGN_WARP_MAX_T keeps t * seg (seg <= 9) and Iw (<= 2 t) exact in fp32.
#pragma once
#include "ign_dropout.h"

#define IGN_WARP_TAG       3u
#ifndef IGN_WARP_MAX_KNOTS            // also in include/ign_abi.h
#define IGN_WARP_MAX_KNOTS 8
#define IGN_WARP_MAX_T     (1 << 20)
#endif
#define IGN_WARP_MAX_CTRL  (IGN_WARP_MAX_KNOTS + 2)

// what one sample draws: whether it is warped at all, and its window [a, a + Lw) with factor c (Lw = 0: no window map)
struct IgnWarpSample { bool on; int a, Lw; float c; };

IGN_DROP_FN IgnWarpSample ign_warp_sample(uint64_t seed, uint32_t b, int n, float wwarp, float prob) {
    IgnWarpSample o = {false, 0, 0, 1.0f};
    if (n < 2) return o;
    const IgnPhilox4 x = ign_philox4x32_10(b, 0u, 0u, IGN_WARP_TAG, (uint32_t)seed, (uint32_t)(seed >> 32));
    o.on = (float)(x.x0 >> 8) * 0x1p-24f < prob;
    if (wwarp > 0.0f && n >= 3) {
        int Lw = (int)floorf(wwarp * (float)n);
        Lw = Lw > 2 ? Lw : 2;
        Lw = Lw < n - 1 ? Lw : n - 1;
        o.Lw = Lw;
        o.a = (int)(x.x1 % (uint32_t)(n - Lw + 1));
        o.c = (x.x2 & 1u) ? 2.0f : 0.5f;
    }
    return o;
}

// control value i (0 .. knots + 1) of the speed curve (first = 1) or the gain curve (first = 4): 1 + rate * (2 u - 1)
IGN_DROP_FN float ign_warp_knot(uint64_t seed, uint32_t b, int i, uint32_t first, float rate) {
    const IgnPhilox4 x = ign_philox4x32_10(b, first + ((uint32_t)i >> 2), 0u, IGN_WARP_TAG, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t k = (uint32_t)i & 3u;
    const uint32_t word = k == 0u ? x.x0 : k == 1u ? x.x1 : k == 2u ? x.x2 : x.x3;
    const float u = (float)(word >> 8) * 0x1p-24f;
    const float d = 2.0f * u - 1.0f;
    return 1.0f + rate * d;
}

IGN_DROP_FN float ign_warp_window_integral(float t, const IgnWarpSample s) {
    float d = t - (float)s.a;
    d = d > 0.0f ? d : 0.0f;
    d = d < (float)s.Lw ? d : (float)s.Lw;
    return t + (s.c - 1.0f) * d;
}

// pos(t) of the integer step t (n >= 2)
IGN_DROP_FN float ign_warp_pos(int t, int n, const IgnWarpSample s) {
    if (s.Lw == 0) return (float)t;
    const float last = (float)(n - 1);
    return (ign_warp_window_integral((float)t, s) * last) / ign_warp_window_integral(last, s);
}

// knot coordinate of position p: segment i = min(floor(u), K) and f = u - i
IGN_DROP_FN void ign_warp_segment(float p, int n, int knots, int* i, float* f) {
    const float u = (p * (float)(knots + 1)) / (float)(n - 1);
    int k = (int)floorf(u);
    k = k < knots ? k : knots;
    *i = k;
    *f = u - (float)k;
}

// smooth(p): v holds the knots + 2 speed values (no dynamic indexing of a local array: the running sum is scanned)
IGN_DROP_FN float ign_warp_smooth(float p, int n, int knots, const float* v) {
    int i;
    float f;
    ign_warp_segment(p, n, knots, &i, &f);
    float acc = 0.0f, Ci = 0.0f;
    for (int j = 0; j <= knots; ++j) {
        if (j == i) Ci = acc;
        acc = acc + 0.5f * (v[j] + v[j + 1]);
    }
    const float v0 = v[i], v1 = v[i + 1];
    const float I = Ci + (f * v0 + (f * f) * (0.5f * (v1 - v0)));
    return (I * (float)(n - 1)) / acc;
}

// what one output row t < n of a warped sample (n >= 2) needs: the source rows i0, i0 + 1, the weight w and the gain g
struct IgnWarpRow { int i0; float w, g; };

IGN_DROP_FN float ign_warp_phi(int t, int n, const IgnWarpSample s, int knots, float twarp, const float* v) {
    const float last = (float)(n - 1);
    if (t >= n - 1) return last;
    float p = ign_warp_pos(t, n, s);
    if (twarp > 0.0f) p = ign_warp_smooth(p, n, knots, v);
    p = p > 0.0f ? p : 0.0f;
    return p < last ? p : last;
}

IGN_DROP_FN float ign_warp_gain(int t, int n, int knots, const float* m) {
    int i;
    float f;
    ign_warp_segment((float)t, n, knots, &i, &f);
    const float m0 = m[i], m1 = m[i + 1];
    return m0 + f * (m1 - m0);
}

IGN_DROP_FN IgnWarpRow ign_warp_row(int t, int n, const IgnWarpSample s, int knots, float twarp, float mwarp, const float* v,
                                    const float* m) {
    IgnWarpRow o;
    const float phi = ign_warp_phi(t, n, s, knots, twarp, v);
    int i0 = (int)floorf(phi);
    i0 = i0 < n - 2 ? i0 : n - 2;
    o.i0 = i0;
    o.w = phi - (float)i0;
    o.g = mwarp > 0.0f ? ign_warp_gain(t, n, knots, m) : 1.0f;
    return o;
}

// one element (the definition the kernel implements): x0 = x[b, i0, c], x1 = x[b, i0 + 1, c]
IGN_DROP_FN float ign_warp_apply(float x0, float x1, float w, float g, bool gain) {
    float y = x0;
    if (w != 0.0f) {
        const float d = x1 - x0;
        y = x0 + w * d;
    }
    return gain ? g * y : y;
}
