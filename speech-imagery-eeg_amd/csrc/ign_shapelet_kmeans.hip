// Sliding k-means over the training windows: one Lloyd step of the shapelet initialisation (utils/shapelet_init.py).
//
// The distance of shapelet (k, c) reads channel c only, so the windows xn[b, c, t*stride : t*stride+L] over all (b, t) are
// clustered per channel into the K centroids w[:, c, :].  One step over a batch is three launches:
//   km_assign_kernel  the forward's mapping (ign_shapelet_fwd.h): one wave per (b, c) row, the row staged in LDS, lane <-> TT
//                     consecutive windows, w[k,c,j] wave-uniform through the scalar cache, shapelets in tiles of 5 / 2 / 1.  The
//                     distance is the direct mean (x - w)^2 (no expansion: cancellation); a running (min, arg-min) over the K tiles
//                     takes the place of the forward's reduction over t (strict <: lowest k on ties).  Per row it writes the
//                     assignment of every window, the count of every cluster and the sum of the minima.
//   km_accum_kernel   the weight-gradient pass's mapping: lane <-> shapelet position j, block <-> (channel, batch slice, j tile,
//                     K tile); for every window of the slice the wave-uniform assignment selects the accumulator that takes
//                     x[t*stride + j].  One partial (nbs, K, C, L) per batch slice, summed in (b, t) order.
//   km_reduce_kernel  partials over the slices, per-row counts and minima over the batch, each by ONE thread in ascending order,
//                     written (accumulate = 0) or added (1) to sums / counts / inertia.
// No atomics anywhere: every output element has one writer and a fixed summation order, so a step is bitwise repeatable.
// km_update_kernel: w = sums / counts where counts > 0; an empty cluster keeps its centroid bit for bit.
#include "ign_common.h"
#include <algorithm>

namespace {

struct KmAssignArgs {
    const float* xn;        // (B,C,T)
    const float* w;         // (K,C,L)
    int32_t* assign;        // (B,C,Tw)
    int32_t* cnt_part;      // (B,C,K)
    float* inert_part;      // (B,C)
    int B, C, T, K, L, Tw, stride;
    int npass;              // passes of 64*TT windows per row
    int xs_len;             // floats of LDS (multiple of 4)
    float invL;
};

typedef const __attribute__((address_space(4))) float* km_cfloat_p;

// KT shapelets k0 .. k0+KT-1 against the TT windows of this lane: squared differences accumulated over j, then the running
// (min, arg-min) update in ascending k
template <int TT, int KT>
__device__ __forceinline__ void km_tile(const float* xl, km_cfloat_p wk, const size_t wks, const int L, const int k0,
                                        const float invL, float (&best)[TT], int (&arg)[TT]) {
    constexpr int J = 4;
    float acc[KT][TT];
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[k][t] = 0.f;
    float xw[TT + J - 1];
#pragma unroll
    for (int i = 0; i < TT - 1; ++i) xw[i] = xl[i];
    int j0 = 0;
    for (; j0 + J <= L; j0 += J) {
#pragma unroll
        for (int jj = 0; jj < J; ++jj) xw[TT - 1 + jj] = xl[j0 + TT - 1 + jj];
#pragma unroll
        for (int jj = 0; jj < J; ++jj)
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const float wv = wk[k * wks + j0 + jj];             // wave-uniform: scalar load, SGPR operand
#pragma unroll
                for (int t = 0; t < TT; ++t) {
                    const float df = xw[t + jj] - wv;
                    acc[k][t] = fmaf(df, df, acc[k][t]);
                }
            }
#pragma unroll
        for (int i = 0; i < TT - 1; ++i) xw[i] = xw[i + J];
    }
    for (; j0 < L; ++j0) {                                          // L % J tail
        xw[TT - 1] = xl[j0 + TT - 1];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const float wv = wk[k * wks + j0];
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                const float df = xw[t] - wv;
                acc[k][t] = fmaf(df, df, acc[k][t]);
            }
        }
#pragma unroll
        for (int i = 0; i < TT - 1; ++i) xw[i] = xw[i + 1];
    }
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            const float d = acc[k][t] * invL;
            if (d < best[t]) { best[t] = d; arg[t] = k0 + k; }
        }
}

template <int TT>
__global__ void __launch_bounds__(64) km_assign_kernel(const KmAssignArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int lane = threadIdx.x;
    const size_t rowi = blockIdx.x;                                 // b*C + c
    const int c = (int)(rowi % (size_t)a.C);
    {
        const float* row = a.xn + rowi * a.T;
        for (int i = lane; i < a.xs_len; i += 64) xs[i] = (i < a.T) ? row[i] : 0.f;
    }
    __syncthreads();

    const size_t wks = (size_t)a.C * a.L;
    const km_cfloat_p wc = (km_cfloat_p)(uintptr_t)(a.w + (size_t)c * a.L);
    int32_t* arow = a.assign + rowi * a.Tw;
    int32_t* cp = a.cnt_part + rowi * a.K;
    float inert = 0.f;

    for (int pass = 0; pass < a.npass; ++pass) {
        const int tl = (pass * 64 + lane) * TT;                     // first window of this lane; past Tw only in the last pass
        const float* xl = xs + tl * a.stride;                       // stride != 1 only with TT == 1; stays inside xs_len
        float best[TT];
        int arg[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) { best[t] = INFINITY; arg[t] = 0; }
        int k0 = 0;
        for (; k0 + 5 <= a.K; k0 += 5) km_tile<TT, 5>(xl, wc + k0 * wks, wks, a.L, k0, a.invL, best, arg);
        for (; k0 + 2 <= a.K; k0 += 2) km_tile<TT, 2>(xl, wc + k0 * wks, wks, a.L, k0, a.invL, best, arg);
        for (; k0 < a.K; ++k0) km_tile<TT, 1>(xl, wc + k0 * wks, wks, a.L, k0, a.invL, best, arg);

        const int nvalid = min(TT, max(0, a.Tw - tl));
#pragma unroll
        for (int t = 0; t < TT; ++t)
            if (t < nvalid) {
                inert += best[t];
                arow[tl + t] = arg[t];
            }
        // cluster sizes of this row: wave-wide population counts; lane 0 owns the row's K counters across the passes
        for (int k = 0; k < a.K; ++k) {
            int n = 0;
#pragma unroll
            for (int t = 0; t < TT; ++t) n += __popcll(__ballot(t < nvalid && arg[t] == k));
            if (lane == 0) cp[k] = (pass ? cp[k] : 0) + n;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) inert += __shfl_xor(inert, m);  // butterfly: the same tree every run
    if (lane == 0) a.inert_part[rowi] = inert;
}

constexpr int KM_XS = 3072;     // floats of x staged per chunk of windows (and the most windows per chunk)
constexpr int KM_KT = 8;        // most clusters per accumulate block (the kernel is instantiated for 1 .. KM_KT)

struct KmAccArgs {
    const float* xn;        // (B,C,T)
    const int32_t* assign;  // (B,C,Tw)
    float* part;            // (nbs,K,C,L)
    int B, C, T, K, L, Tw, stride;
    int rps;                // batch rows per slice
    int njt;                // tiles of blockDim.x shapelet positions
    int tc;                 // windows per staged chunk: (tc-1)*stride + blockDim.x <= KM_XS, tc <= KM_XS
};

template <int KT>
__global__ void __launch_bounds__(256) km_accum_kernel(const KmAccArgs a) {
    __shared__ float xs[KM_XS];
    __shared__ int asg[KM_XS];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int c = blockIdx.x, s = blockIdx.y;
    const int jt = blockIdx.z % a.njt, kt = blockIdx.z / a.njt;
    const int j0 = jt * nth, j = j0 + tid, k0 = kt * KT;
    float acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = 0.f;

    const int b_hi = min(a.B, (s + 1) * a.rps);
    for (int b = s * a.rps; b < b_hi; ++b) {
        const size_t rowi = (size_t)b * a.C + c;
        const float* row = a.xn + rowi * a.T;
        const int32_t* arow = a.assign + rowi * a.Tw;
        for (int t0 = 0; t0 < a.Tw; t0 += a.tc) {
            const int n = min(a.tc, a.Tw - t0);
            const int len = (n - 1) * a.stride + nth;               // <= KM_XS by the choice of tc
            const int g0 = t0 * a.stride + j0;
            for (int i = tid; i < len; i += nth) xs[i] = (g0 + i < a.T) ? row[g0 + i] : 0.f;
            for (int i = tid; i < n; i += nth) asg[i] = arow[t0 + i] - k0;
            __syncthreads();
#pragma unroll 4
            for (int t = 0; t < n; ++t) {
                const int av = asg[t];                               // same address in every lane: a broadcast read
                const float xv = xs[t * a.stride + tid];
#pragma unroll
                for (int k = 0; k < KT; ++k) acc[k] += (av == k) ? xv : 0.f;
            }
            __syncthreads();
        }
    }
    if (j < a.L)
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k0 + k < a.K) a.part[(((size_t)s * a.K + k0 + k) * a.C + c) * a.L + j] = acc[k];
}

struct KmReduceArgs {
    const float* part;          // (nbs,K,C,L)
    const int32_t* cnt_part;    // (B,C,K)
    const float* inert_part;    // (B,C)
    float* sums;                // (K,C,L)
    int32_t* counts;            // (K,C)
    float* inertia;             // (C)
    size_t n;                   // K*C*L
    int B, C, K, nbs, accumulate;
};

__global__ void __launch_bounds__(256) km_reduce_kernel(const KmReduceArgs a) {
    const size_t total = a.n + (size_t)a.K * a.C + a.C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        if (i < a.n) {
            float v = 0.f;
            for (int s = 0; s < a.nbs; ++s) v += a.part[(size_t)s * a.n + i];
            a.sums[i] = a.accumulate ? a.sums[i] + v : v;
        } else if (i < a.n + (size_t)a.K * a.C) {
            const int kc = (int)(i - a.n), k = kc / a.C, c = kc - k * a.C;
            int v = 0;
            for (int b = 0; b < a.B; ++b) v += a.cnt_part[((size_t)b * a.C + c) * a.K + k];
            a.counts[kc] = a.accumulate ? a.counts[kc] + v : v;
        } else {
            const int c = (int)(i - a.n - (size_t)a.K * a.C);
            double v = 0.0;
            for (int b = 0; b < a.B; ++b) v += (double)a.inert_part[(size_t)b * a.C + c];
            a.inertia[c] = a.accumulate ? a.inertia[c] + (float)v : (float)v;
        }
    }
}

__global__ void __launch_bounds__(256) km_update_kernel(float* w, const float* sums, const int32_t* counts, size_t n, int L) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int cnt = counts[i / (size_t)L];
        if (cnt > 0) w[i] = sums[i] / (float)cnt;
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct KmPlan {
    int Tw, TT, npass, xs_len, rps, nbs, threads, njt, nkt, kt, tc;
    size_t lds, off_cnt, off_inert, off_part, bytes;
};

// the launch plan of one step; the domain is the forward's (any B, C, T; 1 <= L <= T; stride, K >= 1; rows within its LDS staging)
int km_plan(const char* who, int B, int C, int T, int K, int L, int stride, KmPlan* p) {
    if (B <= 0 || C <= 0 || T <= 0 || K <= 0 || L <= 0 || stride <= 0 || L > T) {
        if (who) ign_set_error("%s: bad dimensions B=%d C=%d T=%d K=%d L=%d stride=%d", who, B, C, T, K, L, stride);
        return IGN_E_ARG;
    }
    if ((size_t)B * C > 0x7fffffffull) {
        if (who) ign_set_error("%s: B*C = %zu rows exceed the grid limit", who, (size_t)B * C);
        return IGN_E_ARG;
    }
    p->Tw = (T - L) / stride + 1;
    // windows per lane: the power of two that covers the row in one pass, at most 8; strided windows do not slide: TT = 1
    int TT = 1;
    if (stride == 1)
        while (TT < 8 && 64 * TT < p->Tw) TT *= 2;
    p->TT = TT;
    p->npass = (p->Tw + 64 * TT - 1) / (64 * TT);
    const size_t xs_len = (((size_t)p->npass * 64 * TT - 1) * stride + (TT - 1) + L + 3) & ~(size_t)3;
    p->lds = xs_len * 4;
    if (p->lds > 160 * 1024) {           // the forward's row limit (the whole LDS of a CU)
        if (who) ign_set_error("%s: a row needs %zu bytes of LDS staging (T=%d L=%d stride=%d)", who, p->lds, T, L, stride);
        return IGN_E_TOOBIG;
    }
    p->xs_len = (int)xs_len;
    // batch slices of 4 rows (more when the partials would pass 256 MB or the grid's y limit), as the weight-gradient pass
    int rps = 4;
    while (((size_t)((B + rps - 1) / rps) * K * C * L * 4 > ((size_t)256 << 20) || (B + rps - 1) / rps > 65535) && rps < B) rps *= 2;
    p->rps = rps;
    p->nbs = (B + rps - 1) / rps;
    // accumulate blocks: the shapelet positions in equal tiles of at most 256 lanes (whole waves), the clusters in equal tiles of
    // at most KM_KT -- L = 300 runs 2 x 192 lanes instead of 2 x 256, K = 5 five select-adds per sample instead of eight
    p->njt = (L + 255) / 256;
    p->threads = (((L + p->njt - 1) / p->njt + 63) / 64) * 64;
    p->nkt = (K + KM_KT - 1) / KM_KT;
    p->kt = (K + p->nkt - 1) / p->nkt;
    if ((size_t)p->njt * p->nkt > 65535) {
        if (who) ign_set_error("%s: K=%d L=%d need %zu accumulate tiles per slice (limit 65535)", who, K, L, (size_t)p->njt * p->nkt);
        return IGN_E_TOOBIG;
    }
    p->tc = std::max(1, std::min(p->Tw, (KM_XS - p->threads) / stride + 1));
    p->off_cnt = align256((size_t)B * C * p->Tw * 4);
    p->off_inert = p->off_cnt + align256((size_t)B * C * K * 4);
    p->off_part = p->off_inert + align256((size_t)B * C * 4);
    p->bytes = p->off_part + align256((size_t)p->nbs * K * C * L * 4);
    return 0;
}

template <int TT>
void km_launch_assign(const KmAssignArgs& a, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&km_assign_kernel<TT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
    hipLaunchKernelGGL((km_assign_kernel<TT>), dim3((unsigned)((size_t)a.B * a.C)), dim3(64), lds, s, a);
}

template <int KT>
void km_launch_accum(const KmAccArgs& c, const KmPlan& p, hipStream_t s) {
    hipLaunchKernelGGL((km_accum_kernel<KT>), dim3((unsigned)c.C, (unsigned)p.nbs, (unsigned)(p.njt * p.nkt)), dim3(p.threads), 0, s, c);
}

unsigned km_flat_grid(size_t n) { return (unsigned)std::min<size_t>(2048, (n + 255) / 256); }

}  // namespace

extern "C" size_t ign_shapelet_kmeans_workspace_bytes(int B, int C, int T, int K, int L, int stride) {
    KmPlan p;
    if (km_plan(nullptr, B, C, T, K, L, stride, &p)) return 0;
    return p.bytes;
}

extern "C" int ign_shapelet_kmeans_step(const float* xn_bct, const float* w_kcl, int32_t* assign, float* sums_kcl, int32_t* counts_kc,
                                        float* inertia_c, void* workspace, int accumulate, int B, int C, int T, int K, int L,
                                        int stride, void* stream) {
    static const char* who = "ign_shapelet_kmeans_step";
    KmPlan p;
    int rc;
    if ((rc = km_plan(who, B, C, T, K, L, stride, &p))) return rc;
    if (!xn_bct || !w_kcl || !sums_kcl || !counts_kc || !inertia_c || !workspace) {
        ign_set_error("%s: null pointer argument (only assign may be null)", who);
        return IGN_E_ARG;
    }
    if (accumulate != 0 && accumulate != 1) {
        ign_set_error("%s: accumulate=%d is neither 0 nor 1", who, accumulate);
        return IGN_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    KmAssignArgs a;
    a.xn = xn_bct; a.w = w_kcl; a.assign = assign ? assign : (int32_t*)ws;
    a.cnt_part = (int32_t*)(ws + p.off_cnt); a.inert_part = (float*)(ws + p.off_inert);
    a.B = B; a.C = C; a.T = T; a.K = K; a.L = L; a.Tw = p.Tw; a.stride = stride; a.npass = p.npass; a.xs_len = p.xs_len;
    a.invL = 1.0f / (float)L;
    {
        IgnScopedTimer tm("kmeans_assign", s);
        switch (p.TT) {
            case 1: km_launch_assign<1>(a, p.lds, s); break;
            case 2: km_launch_assign<2>(a, p.lds, s); break;
            case 4: km_launch_assign<4>(a, p.lds, s); break;
            default: km_launch_assign<8>(a, p.lds, s); break;
        }
    }
    if ((rc = ign_check_launch("km_assign_kernel"))) return rc;

    KmAccArgs c;
    c.xn = xn_bct; c.assign = a.assign; c.part = (float*)(ws + p.off_part);
    c.B = B; c.C = C; c.T = T; c.K = K; c.L = L; c.Tw = p.Tw; c.stride = stride; c.rps = p.rps; c.njt = p.njt; c.tc = p.tc;
    {
        IgnScopedTimer tm("kmeans_accum", s);
        switch (p.kt) {
            case 1: km_launch_accum<1>(c, p, s); break;
            case 2: km_launch_accum<2>(c, p, s); break;
            case 3: km_launch_accum<3>(c, p, s); break;
            case 4: km_launch_accum<4>(c, p, s); break;
            case 5: km_launch_accum<5>(c, p, s); break;
            case 6: km_launch_accum<6>(c, p, s); break;
            case 7: km_launch_accum<7>(c, p, s); break;
            default: km_launch_accum<8>(c, p, s); break;
        }
    }
    if ((rc = ign_check_launch("km_accum_kernel"))) return rc;

    KmReduceArgs r;
    r.part = c.part; r.cnt_part = a.cnt_part; r.inert_part = a.inert_part; r.sums = sums_kcl; r.counts = counts_kc;
    r.inertia = inertia_c; r.n = (size_t)K * C * L; r.B = B; r.C = C; r.K = K; r.nbs = p.nbs; r.accumulate = accumulate;
    {
        IgnScopedTimer tm("kmeans_reduce", s);
        hipLaunchKernelGGL(km_reduce_kernel, dim3(km_flat_grid(r.n + (size_t)K * C + C)), dim3(256), 0, s, r);
    }
    return ign_check_launch("km_reduce_kernel");
}

extern "C" int ign_shapelet_kmeans_update(float* w_kcl, const float* sums_kcl, const int32_t* counts_kc, int K, int C, int L,
                                          void* stream) {
    static const char* who = "ign_shapelet_kmeans_update";
    if (K <= 0 || C <= 0 || L <= 0) {
        ign_set_error("%s: bad dimensions K=%d C=%d L=%d", who, K, C, L);
        return IGN_E_ARG;
    }
    if (!w_kcl || !sums_kcl || !counts_kc) {
        ign_set_error("%s: null pointer argument", who);
        return IGN_E_ARG;
    }
    const size_t n = (size_t)K * C * L;
    hipLaunchKernelGGL(km_update_kernel, dim3(km_flat_grid(n)), dim3(256), 0, (hipStream_t)stream, w_kcl, sums_kcl, counts_kc, n, L);
    return ign_check_launch("km_update_kernel");
}
