// Training augmentation (run.py --augment): circular shift, per-channel gain, Gaussian noise, electrode dropout and one masked time
// span per sample, in ONE out-of-place pass over the (B, T, C) batch.  The rule -- every random decision -- is ign_augment.h.
//
// Memory-bound without noise: one read and one write of the batch, no workspace, no atomics, bitwise repeatable.  A block owns
// AUG_CHUNK consecutive flat (t, c) indices of one sample; a lane owns the quad e0 .. e0 + 3 (e0 % 4 == 0), which is also the noise
// rule's quad: one Philox call and two Box-Muller pairs per lane and trip.  A shift moves whole rows of C floats, so the source of a
// quad is the same flat array rotated by sh * C: contiguous except for the one quad that crosses the seam and the one that
// crosses the end of the data.  Source and destination of a quad are 4-byte aligned only (C = 122, any shift, any T * C): both
// go through a 4-byte-aligned 16-byte vector type, which the compiler turns into one dwordx4 access (global memory takes those at
// dword alignment); the seam, the data / padding boundary and the tail of the sample take the element path.
// Per-sample draws are block-uniform (one Philox call per lane, the same in every lane); per-(b, c) draws are taken once per
// block into LDS, and only when the gain or the electrode dropout is on.  The noise path is a separate instantiation: with
// sigma == 0 no Philox call, logarithm, square root or sine is issued per element.
#include "ign_btc.h"
#include "ign_augment.h"

constexpr int AUG_THREADS = 256;
constexpr int AUG_QUADS = 4;                                   // quads per lane
constexpr int AUG_CHUNK = AUG_THREADS * AUG_QUADS * 4;         // flat indices per block
constexpr int AUG_CMAX = 8192;                                 // channels whose gain / keep table fits 64 KB of LDS

struct __attribute__((packed, aligned(4))) AugQuad { float v[4]; };

struct AugArgs {
    const float* x;
    float* out;
    const int32_t* len;   // (B) or null
    int T, C, nchunk;
    unsigned long long seed;
    float shift, scale, sigma, time_mask;
    unsigned chan_thr;
};

template <bool NOISE>
__global__ void __launch_bounds__(AUG_THREADS) augment_kernel(const AugArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.nchunk;
    const int chunk = blockIdx.x - b * a.nchunk;
    const int C = a.C, TC = a.T * C;
    const int len = IGN_BTC_LEN(a.len, b, a.T);
    const int n = len * C;                                        // flat indices of data; padding from there to TC
    const IgnAugSample sp = ign_aug_sample(a.seed, (uint32_t)b, len, a.shift, a.time_mask);
    const int shc = sp.sh * C;                                    // in [0, n)
    const bool per_channel = a.scale != 0.f || a.chan_thr != 0u;  // block-uniform
    float* gain = lds;
    float* keep = lds + C;
    if (per_channel) {
        for (int c = tid; c < C; c += AUG_THREADS) {
            const IgnAugChannel ch = ign_aug_channel(a.seed, (uint32_t)b, (uint32_t)c, a.scale, a.chan_thr);
            gain[c] = ch.a;
            keep[c] = ch.keep ? 1.f : 0.f;
        }
        __syncthreads();
    }
    const float* xb = a.x + (size_t)b * TC;
    float* ob = a.out + (size_t)b * TC;
#pragma unroll
    for (int u = 0; u < AUG_QUADS; ++u) {
        const int e0 = chunk * AUG_CHUNK + (u * AUG_THREADS + tid) * 4;
        if (e0 >= TC) break;                                      // e0 grows with u
        float v[4];
        const bool whole = e0 + 3 < TC;
        if (whole && e0 >= n) {                                   // padding: copied through
            *reinterpret_cast<AugQuad*>(ob + e0) = *reinterpret_cast<const AugQuad*>(xb + e0);
            continue;
        }
        if (whole && e0 + 3 < n && (e0 >= shc || e0 + 3 < shc)) { // data, source contiguous: not across the seam
            const int s0 = e0 - shc + (e0 < shc ? n : 0);
            const AugQuad q = *reinterpret_cast<const AugQuad*>(xb + s0);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = q.v[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = e0 + k;
                const int s = e < n ? e - shc + (e < shc ? n : 0) : e;
                v[k] = e < TC ? xb[s] : 0.f;
            }
        }
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (NOISE) ign_aug_noise4(a.seed, (uint32_t)b, (uint32_t)(e0 >> 2), nz);
        int t = (int)((unsigned)e0 / (unsigned)C), c = e0 - t * C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e0 + k < n) {                                     // data; beyond n the loaded value is the output
                const bool kp = !(t >= sp.m0 && t < sp.m1) && (!per_channel || keep[c] != 0.f);
                v[k] = ign_aug_apply(v[k], per_channel ? gain[c] : 1.0f, kp, NOISE ? a.sigma : 0.f, nz[k]);
            }
            if (++c == C) { c = 0; ++t; }
        }
        if (whole) {
            AugQuad q;
#pragma unroll
            for (int k = 0; k < 4; ++k) q.v[k] = v[k];
            *reinterpret_cast<AugQuad*>(ob + e0) = q;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < TC) ob[e0 + k] = v[k];
        }
    }
}

extern "C" int ign_augment_btc(const float* x, float* out, const int32_t* len_b, int B, int T, int C, unsigned long long seed,
                               float shift, float scale, float sigma, unsigned chan_thr, float time_mask, void* stream) {
    static const char* who = "ign_augment_btc";
    if (C > AUG_CMAX) {                                           // ahead of the overlap rule, whose span grows with C
        ign_set_error("%s: C=%d above %d channels", who, C, AUG_CMAX);
        return IGN_E_TOOBIG;
    }
    if (const int rc = ign_btc_check(who, x, out, B, T, C)) return rc;
    if (!ign_rate_ok(shift) || !ign_rate_ok(scale) || !ign_rate_ok(time_mask) || chan_thr >= 65536u) {
        ign_set_error("%s: shift=%g scale=%g time_mask=%g must lie in [0, 1) and chan_thr=%u below 65536", who, (double)shift,
                      (double)scale, (double)time_mask, chan_thr);
        return IGN_E_ARG;
    }
    if (!(sigma >= 0.f) || sigma > 3.0e38f) {
        ign_set_error("%s: sigma=%g must be finite and non-negative", who, (double)sigma);
        return IGN_E_ARG;
    }
    const long long nchunk = ((long long)T * C + AUG_CHUNK - 1) / AUG_CHUNK;
    if (const int rc = ign_btc_grid_check(who, B, T, C, nchunk)) return rc;
    AugArgs a;
    a.x = x; a.out = out; a.len = len_b; a.T = T; a.C = C; a.nchunk = (int)nchunk; a.seed = seed;
    a.shift = shift; a.scale = scale; a.sigma = sigma; a.time_mask = time_mask; a.chan_thr = chan_thr;
    const size_t lds = (scale != 0.f || chan_thr != 0u) ? (size_t)C * 2 * sizeof(float) : 0;
    const dim3 grid((unsigned)(B * nchunk)), block(AUG_THREADS);
    {
        IgnScopedTimer tm("augment", (hipStream_t)stream);
        if (sigma != 0.f) hipLaunchKernelGGL(augment_kernel<true>, grid, block, lds, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(augment_kernel<false>, grid, block, lds, (hipStream_t)stream, a);
    }
    return ign_check_launch("augment_kernel");
}
