// Time, magnitude and window warping of the training batch (run.py --warp): every sample of a (B, T, C) batch is resampled along
// time through its own monotone map phi_b(t) and scaled by its own smooth gain curve g_b(t), in ONE out-of-place pass.  The rule --
// every draw and every rounding -- is ign_warp.h.
//
// Memory-bound: one read of two neighbouring source rows per output row (the second is the first of the next output row or close
// to it: L2 serves most of it) and one write, no workspace, no atomics, bitwise repeatable.  A block owns `rows` consecutive
// output rows of one sample.  phi(t), the source row, the weight and the gain are per output ROW, not per element: the first
// K + 2 lanes draw the two knot tables into LDS, then one lane per row of the tile works its row record out into LDS, and the pass
// over the tile reads it back (a broadcast).  Lanes run along c, the contiguous axis: a row is C / VEC units of VEC floats, VEC = 4
// where C % 4 == 0 and both buffers are 16-byte aligned, 2 likewise for 8 bytes (C = 122), else 1; the block is LX x (256 / LX)
// lanes with LX the smallest power of two that holds a row's units (at most 256), so for a short row a wave carries several rows.
// A tile of the padding, a sample that is not warped and a call with every rate 0 take the copy path: no LDS, no arithmetic.
#include <cstdint>
#include "ign_btc.h"
#include "ign_warp.h"

constexpr int WARP_THREADS = 256;
constexpr int WARP_MAX_ROWS = WARP_THREADS;                    // one lane per row record
constexpr int WARP_TILE_ELEMS = 4096;                          // floats per block, about

struct WarpArgs {
    const float* x;
    float* out;
    const int32_t* len;   // (B) or null
    int T, C, rows, ntile, lx_log2;
    unsigned long long seed;
    float twarp, mwarp, wwarp, prob;
    int knots;
};

template <int VEC> struct WarpVec;
template <> struct WarpVec<1> { float v[1]; };
template <> struct __attribute__((aligned(8))) WarpVec<2> { float v[2]; };
template <> struct __attribute__((aligned(16))) WarpVec<4> { float v[4]; };

template <int VEC>
__global__ void __launch_bounds__(WARP_THREADS) warp_kernel(const WarpArgs a) {
    typedef WarpVec<VEC> Vec;
    __shared__ float s_v[IGN_WARP_MAX_CTRL], s_m[IGN_WARP_MAX_CTRL];
    __shared__ int s_i0[WARP_MAX_ROWS];
    __shared__ float s_w[WARP_MAX_ROWS], s_g[WARP_MAX_ROWS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.ntile;
    const int r0 = (blockIdx.x - b * a.ntile) * a.rows;
    const int nr = min(a.rows, a.T - r0);                          // rows of this tile, >= 1
    const int C = a.C, U = C / VEC;
    const int n = IGN_BTC_LEN(a.len, b, a.T);
    const bool rates = a.twarp > 0.f || a.mwarp > 0.f || a.wwarp > 0.f;
    IgnWarpSample sp = {false, 0, 0, 1.0f};
    if (rates && r0 < n) sp = ign_warp_sample(a.seed, (uint32_t)b, n, a.wwarp, a.prob);      // block-uniform; false for n < 2
    const bool warped = sp.on;
    const bool gain = a.mwarp > 0.f;
    if (warped) {
        if (tid < a.knots + 2) {
            s_v[tid] = a.twarp > 0.f ? ign_warp_knot(a.seed, (uint32_t)b, tid, 1u, a.twarp) : 1.0f;
            s_m[tid] = gain ? ign_warp_knot(a.seed, (uint32_t)b, tid, 4u, a.mwarp) : 1.0f;
        }
        __syncthreads();
        if (tid < nr) {
            const int t = r0 + tid;
            IgnWarpRow row = {t, 0.0f, 1.0f};
            if (t < n) row = ign_warp_row(t, n, sp, a.knots, a.twarp, a.mwarp, s_v, s_m);
            s_i0[tid] = t < n ? row.i0 : -1;                      // -1: a row of the padding, copied through
            s_w[tid] = row.w;
            s_g[tid] = row.g;
        }
        __syncthreads();
    }
    const int lx = tid & ((1 << a.lx_log2) - 1), ly = tid >> a.lx_log2, ny = WARP_THREADS >> a.lx_log2, nx = 1 << a.lx_log2;
    const float* xb = a.x + (size_t)b * a.T * C;
    float* ob = a.out + ((size_t)b * a.T + r0) * C;
    for (int r = ly; r < nr; r += ny) {
        const int i0 = warped ? s_i0[r] : -1;
        float* orow = ob + (size_t)r * C;
        if (i0 < 0) {
            const float* src = xb + (size_t)(r0 + r) * C;
            for (int u = lx; u < U; u += nx) reinterpret_cast<Vec*>(orow)[u] = reinterpret_cast<const Vec*>(src)[u];
            continue;
        }
        const float w = s_w[r], g = s_g[r];
        const float* src = xb + (size_t)i0 * C;                   // rows i0 and i0 + 1 <= n - 1 hold data
        for (int u = lx; u < U; u += nx) {
            const Vec q0 = reinterpret_cast<const Vec*>(src)[u];
            Vec o = q0;
            if (w != 0.f) {                                       // wave-uniform within a row
                const Vec q1 = reinterpret_cast<const Vec*>(src + C)[u];
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = ign_warp_apply(q0.v[k], q1.v[k], w, g, gain);
            } else if (gain) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = g * q0.v[k];
            }
            reinterpret_cast<Vec*>(orow)[u] = o;
        }
    }
}

static int warp_check_rule(const char* who, float twarp, float mwarp, float wwarp, int knots, float prob) {
    if (!ign_rate_ok(twarp) || !ign_rate_ok(mwarp) || !ign_rate_ok(wwarp)) {
        ign_set_error("%s: twarp=%g mwarp=%g wwarp=%g must lie in [0, 1)", who, (double)twarp, (double)mwarp, (double)wwarp);
        return IGN_E_ARG;
    }
    if (knots < 1 || knots > IGN_WARP_MAX_KNOTS || !(prob > 0.f && prob <= 1.f)) {
        ign_set_error("%s: knots=%d outside 1..%d, or prob=%g outside (0, 1]", who, knots, IGN_WARP_MAX_KNOTS, (double)prob);
        return IGN_E_ARG;
    }
    return 0;
}

extern "C" int ign_warp_map(unsigned long long seed, int b, int n, float twarp, float mwarp, float wwarp, int knots, float prob,
                            float* phi_n, float* gain_n) {
    static const char* who = "ign_warp_map";
    if (!phi_n || b < 0 || n < 0) {
        ign_set_error("%s: null phi_n or negative b=%d / n=%d", who, b, n);
        return IGN_E_ARG;
    }
    if (const int rc = warp_check_rule(who, twarp, mwarp, wwarp, knots, prob)) return rc;
    if (n > IGN_WARP_MAX_T) {
        ign_set_error("%s: n=%d above IGN_WARP_MAX_T=%d", who, n, IGN_WARP_MAX_T);
        return IGN_E_TOOBIG;
    }
    const bool rates = twarp > 0.f || mwarp > 0.f || wwarp > 0.f;
    IgnWarpSample sp = {false, 0, 0, 1.0f};
    if (rates) sp = ign_warp_sample(seed, (uint32_t)b, n, wwarp, prob);
    float v[IGN_WARP_MAX_CTRL], m[IGN_WARP_MAX_CTRL];
    for (int i = 0; i < knots + 2; ++i) {
        v[i] = sp.on && twarp > 0.f ? ign_warp_knot(seed, (uint32_t)b, i, 1u, twarp) : 1.0f;
        m[i] = sp.on && mwarp > 0.f ? ign_warp_knot(seed, (uint32_t)b, i, 4u, mwarp) : 1.0f;
    }
    for (int t = 0; t < n; ++t) {
        IgnWarpRow row = {t, 0.0f, 1.0f};
        if (sp.on) row = ign_warp_row(t, n, sp, knots, twarp, mwarp, v, m);
        phi_n[t] = (float)row.i0 + row.w;                          // exact: phi itself
        if (gain_n) gain_n[t] = row.g;
    }
    return 0;
}

extern "C" int ign_warp_btc(const float* x, float* out, const int32_t* len_b, int B, int T, int C, unsigned long long seed,
                            float twarp, float mwarp, float wwarp, int knots, float prob, void* stream) {
    static const char* who = "ign_warp_btc";
    if (const int rc = ign_btc_check(who, x, out, B, T, C)) return rc;
    if (const int rc = warp_check_rule(who, twarp, mwarp, wwarp, knots, prob)) return rc;
    if (T > IGN_WARP_MAX_T) {
        ign_set_error("%s: T=%d above IGN_WARP_MAX_T=%d", who, T, IGN_WARP_MAX_T);
        return IGN_E_TOOBIG;
    }
    int rows = WARP_TILE_ELEMS / C;
    rows = rows < 1 ? 1 : rows > WARP_MAX_ROWS ? WARP_MAX_ROWS : rows;
    rows = rows < T ? rows : T;
    const long long ntile = ((long long)T + rows - 1) / rows;
    if (const int rc = ign_btc_grid_check(who, B, T, C, ntile)) return rc;
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
    const int vec = (C % 4 == 0 && ((xa | oa) & 15) == 0) ? 4 : (C % 2 == 0 && ((xa | oa) & 7) == 0) ? 2 : 1;
    const int U = C / vec;
    int lx_log2 = 0;
    while ((1 << lx_log2) < U && (1 << lx_log2) < WARP_THREADS) ++lx_log2;
    WarpArgs a;
    a.x = x; a.out = out; a.len = len_b; a.T = T; a.C = C; a.rows = rows; a.ntile = (int)ntile; a.lx_log2 = lx_log2; a.seed = seed;
    a.twarp = twarp; a.mwarp = mwarp; a.wwarp = wwarp; a.prob = prob; a.knots = knots;
    const dim3 grid((unsigned)(B * ntile)), block(WARP_THREADS);
    {
        IgnScopedTimer tm("warp", (hipStream_t)stream);
        if (vec == 4) hipLaunchKernelGGL(warp_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
        else if (vec == 2) hipLaunchKernelGGL(warp_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(warp_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
    }
    return ign_check_launch("warp_kernel");
}
