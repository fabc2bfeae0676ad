// Evidence maps: the class logit laid out over time and electrodes.  ONE definition of the arithmetic, for the kernels
// (ign_evidence.hip) and the numpy restatement (utils/evidence.py: evidence_rule, cam_spread_rule) that the tests compare against
// bit for bit.  Usable from __device__ and host code.  The library is built with -ffp-contract=off and this header holds no fmaf:
// every product and sum below is one fp32 rounding.
//
// Shapelet expert (linear head, eval mode): sbm_logit[b,n] = sum_f W[n,f] * p[b,f], feature f = col0_g + k * C + c, matched on
// electrode c over the samples [t[b,f] * stride_g, t[b,f] * stride_g + L_g).  Its share of the logit is spread evenly over that
// window:
//   v[b,f]       = fl(fl(W[n_b,f] * p[b,f]) * invL_g),   invL_g = float32(1) / float32(L_g) from the host
//   E_sbm[b,s,c] = sum of v[b,f] over the features of electrode c with 0 <= t[b,f] < Tw_g whose window covers s,
//                  g ascending, then k ascending, starting from 0.0f; a term that does not cover s is not added (adding 0.0f
//                  instead is the same bits: the running sum starts at +0 and never becomes -0);
//                  times scale[b] once, at the end, when a per-sample scale is given.
// t = -1 (--mask_padding: the sample is shorter than the shapelet) contributes nothing; so does any t outside [0, Tw_g): device data
// is never trusted as an index bound.  A window is kept as (start, len) with len = 0 for "no window": s is covered iff
// (unsigned)(s - start) < (unsigned)len.
//
// FCN expert: cam[b,t] on block 3's axis (ign_bn_relu_cam_fwd; checked against float64, not bit for bit) is spread evenly over the
// R = k1 + k2 + k3 - 2 input samples it saw, T = Tl + R - 1:
//   E_dnn[b,s] = fl(invR * sum_{t = max(0, s-R+1)}^{min(s, Tl-1)} cam[b,t]),  t ascending, starting from 0.0f, invR from the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IGN_EV_FN __host__ __device__ static inline
#else
#define IGN_EV_FN static inline
#endif

// one feature's window on its electrode and its value per covered sample
struct IgnEvTerm { int start, len; float v; };

IGN_EV_FN IgnEvTerm ign_evidence_term(float w, float p, int t, int stride, int L, int Tw, float invL) {
    IgnEvTerm o;
    const bool ok = t >= 0 && t < Tw;
    o.start = ok ? t * stride : 0;
    o.len = ok ? L : 0;
    o.v = (w * p) * invL;
    return o;
}

IGN_EV_FN bool ign_evidence_covers(int s, int start, int len) { return (unsigned)(s - start) < (unsigned)len; }

// the running sum after one more term (see above: adding 0.0f where the window does not cover s changes no bit)
IGN_EV_FN float ign_evidence_add(float acc, int s, int start, int len, float v) {
    return acc + (ign_evidence_covers(s, start, len) ? v : 0.0f);
}

// E_dnn[b,s] from one sample's cam row
IGN_EV_FN float ign_cam_spread_at(const float* cam_row, int s, int Tl, int R, float invR) {
    const int lo = s - R + 1 > 0 ? s - R + 1 : 0, hi = s < Tl - 1 ? s : Tl - 1;
    float acc = 0.0f;
    for (int t = lo; t <= hi; ++t) acc = acc + cam_row[t];
    return invR * acc;
}
