// Mixup / CutMix of the training batch (run.py --mix) in ONE out-of-place pass over the (B, T, C) batch: sample b is blended with its
// partner p = (b + roll) mod B, or -- inside the sample's CutMix span -- replaced by it.  The draws (roll, lam, span) are made on the
// host (utils/mix.py:mix_draws) and arrive as device arrays; the kernel only applies them.
//
// Memory-bound: two reads and one write of the batch, no workspace, no atomics, bitwise repeatable.  The layout is ign_augment_btc's:
// a block owns MIX_CHUNK consecutive flat (t, c) indices of one sample, a lane owns the quad e0 .. e0 + 3 (e0 % 4 == 0).  Rows are
// 4-byte aligned only (C = 122, odd T * C), so a quad goes through a 4-byte-aligned 16-byte vector type, which the compiler turns
// into one dwordx4 access (global memory takes those at dword alignment); the tail of the sample takes the element path.  The
// per-sample scalars (length, lam, span) are block-uniform; the span and the data / padding boundary are compares on the flat index
// per element, not separate paths.  A sample with lam == 1 and an empty span, and every quad of the padding, is a copy that never
// reads the partner: 1 * x + 0 * x_p would turn an infinite partner into NaN.
#include <cstdint>
#include "ign_btc.h"

constexpr int MIX_THREADS = 256;
constexpr int MIX_QUADS = 4;                                   // quads per lane
constexpr int MIX_CHUNK = MIX_THREADS * MIX_QUADS * 4;         // flat indices per block

struct __attribute__((packed, aligned(4))) MixQuad { float v[4]; };

struct MixArgs {
    const float* x;
    float* out;
    const int32_t* len;   // (B) or null
    const float* lam;     // (B)
    const int32_t* span;  // (B, 2) = (start, m) or null
    int roll, B, T, C, nchunk;
};

// one element: the partner inside the span, the blend elsewhere (a copy at lam == 1), the sample itself in the padding
__device__ __forceinline__ float mix_apply(float xv, float pv, int e, int n, int s0, int s1, float lam, float om, bool blend) {
    if (e >= n) return xv;
    if (e >= s0 && e < s1) return pv;
    return blend ? lam * xv + om * pv : xv;
}

__global__ void __launch_bounds__(MIX_THREADS) mix_kernel(const MixArgs a) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.nchunk;
    const int chunk = blockIdx.x - b * a.nchunk;
    const int C = a.C, TC = a.T * C;
    const int len = IGN_BTC_LEN(a.len, b, a.T);
    const int n = len * C;                                        // flat indices of data; padding from there to TC
    int start = 0, m = 0;
    if (a.span) {
        start = min(max(a.span[2 * b], 0), len);
        m = min(max(a.span[2 * b + 1], 0), len - start);
    }
    const int s0 = start * C, s1 = (start + m) * C;               // the span in flat indices, inside [0, n]
    const float lam = a.lam[b], om = 1.f - lam;
    const bool blend = lam != 1.f;
    const bool copy = !blend && s0 == s1;                         // block-uniform: the partner is never read
    int p = b + a.roll;
    if (p >= a.B) p -= a.B;                                       // roll in [0, B)
    const float* xb = a.x + (size_t)b * TC;
    const float* pb = a.x + (size_t)p * TC;
    float* ob = a.out + (size_t)b * TC;
#pragma unroll
    for (int u = 0; u < MIX_QUADS; ++u) {
        const int e0 = chunk * MIX_CHUNK + (u * MIX_THREADS + tid) * 4;
        if (e0 >= TC) break;                                      // e0 grows with u
        if (e0 + 3 < TC) {
            const MixQuad q = *reinterpret_cast<const MixQuad*>(xb + e0);
            if (copy || e0 >= n) {                                // nothing to mix: copied through
                *reinterpret_cast<MixQuad*>(ob + e0) = q;
                continue;
            }
            const MixQuad r = *reinterpret_cast<const MixQuad*>(pb + e0);
            MixQuad o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.v[k] = mix_apply(q.v[k], r.v[k], e0 + k, n, s0, s1, lam, om, blend);
            *reinterpret_cast<MixQuad*>(ob + e0) = o;
        } else {
            for (int e = e0; e < TC; ++e) {
                const float xv = xb[e];
                ob[e] = (copy || e >= n) ? xv : mix_apply(xv, pb[e], e, n, s0, s1, lam, om, blend);
            }
        }
    }
}

extern "C" int ign_mix_btc(const float* x, float* out, const int32_t* len_b, const float* lam_b, const int32_t* span_b2, int roll,
                           int B, int T, int C, void* stream) {
    static const char* who = "ign_mix_btc";
    if (const int rc = ign_btc_check(who, x, out, B, T, C)) return rc;
    if (!lam_b || roll < 0 || roll >= B) {
        ign_set_error("%s: null lam_b, or roll=%d outside [0, B) with B=%d", who, roll, B);
        return IGN_E_ARG;
    }
    const long long nchunk = ((long long)T * C + MIX_CHUNK - 1) / MIX_CHUNK;
    if (const int rc = ign_btc_grid_check(who, B, T, C, nchunk)) return rc;
    MixArgs a;
    a.x = x; a.out = out; a.len = len_b; a.lam = lam_b; a.span = span_b2; a.roll = roll; a.B = B; a.T = T; a.C = C;
    a.nchunk = (int)nchunk;
    {
        IgnScopedTimer tm("mix", (hipStream_t)stream);
        hipLaunchKernelGGL(mix_kernel, dim3((unsigned)(B * nchunk)), dim3(MIX_THREADS), 0, (hipStream_t)stream, a);
    }
    return ign_check_launch("mix_kernel");
}
