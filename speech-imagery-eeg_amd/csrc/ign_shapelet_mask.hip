// Variable-length series (--mask_padding): the two passes that make the shapelet expert treat sample b of a zero-padded batch
// as if it had been given alone, truncated to its own length n_b = len_b[b] (UEA's collate pads at the end, so the keep-mask is
// a length).  Neither the forward nor the two backward kernels change:
//   ign_instnorm_fwd_len   mean / unbiased std over x[b, :n_b, c] only, xn[b, c, t >= n_b] = 0 -- the twin of ign_instnorm_fwd;
//   ign_shapelet_regate    runs AFTER the unchanged forward.  Window t of group g is valid for sample b iff t < Tw_b =
//                          (n_b - L) / stride + 1 (0 if n_b < L); a valid window reads x[b, :n_b] only, so its saved distance is
//                          already that of the truncated problem.  Per (b, c, k) row of d_save the pass recomputes P, Dmin, t*, Z, mu
//                          from the first Tw_b distances (the formulas of the forward's epilogue, ign_shapelet_fwd.h) and overwrites
//                          the others with 1e18f, the value the forward itself gives to slots past the end of a row: with it the
//                          backward's coefficient (ign_shapelet_bwd.h) is exactly 0 -- RBF: p = exp(-(eps d)^2) = 0 multiplies it;
//                          LTS: exp(dmin - d) = 0, and on a row without any window P = 0 makes the upstream factor P (1 - P) zero.
// Memory-bound: one sweep over d_save (the LTS second sweep re-reads a row of a few KB that the same wave has just pulled into
// the cache) and a partial write.  One wave per row, lanes along t (coalesced), any Tw (the lanes loop); the 64 partial results
// are merged by the forward's DPP reductions in a fixed order: no atomics, bitwise repeatable.
#include "ign_shapelet_fwd.h"

#define IGN_NO_WINDOW 1e18f            // ops.NO_WINDOW: Dmin of a feature without a valid window, and d_save of an invalid window

// ---------------------------------------------------------------------------------------------------- instance norm
// Tiling of instnorm_kernel (ign_instnorm.hip): a block owns (b, CT channels), stages the n_b x CT tile in LDS (pitch CT+1), one
// wave per channel takes mean and unbiased variance in two sweeps and writes the (c, t) line: normalised below n_b, 0 from there on.
__global__ void __launch_bounds__(1024) instnorm_len_kernel(const float* __restrict__ x, const int32_t* __restrict__ len_b,
                                                           float* __restrict__ xn, int B, int T, int C, int CT, float eps) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int pitch = CT + 1;
    const int nct = (C + CT - 1) / CT;
    const int b = blockIdx.x / nct;
    const int c0 = (blockIdx.x - b * nct) * CT;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int n = min(max(len_b[b], 0), T);                       // device data: clamped, never trusted as an index bound
    const float* xb = x + (size_t)b * T * C;
    for (int i0 = tid; i0 < n * CT; i0 += 8 * nthr) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = i0 + u * nthr;
            const int t = idx / CT, cc = idx - t * CT;
            v[u] = (idx < n * CT && c0 + cc < C) ? xb[(size_t)t * C + c0 + cc] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = i0 + u * nthr;
            const int t = idx / CT, cc = idx - t * CT;
            if (idx < n * CT) tile[t * pitch + cc] = v[u];
        }
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int cc = wave; cc < CT; cc += (nthr >> 6)) {
        const int c = c0 + cc;
        if (c >= C) break;
        float* on = xn + ((size_t)b * C + c) * T;
        if (n < 2) {                                              // no unbiased std of fewer than two samples: the row is 0
            for (int t = lane; t < T; t += 64) on[t] = 0.f;
            continue;
        }
        float s = 0.f;
        for (int t = lane; t < n; t += 64) s += tile[t * pitch + cc];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mean = s / (float)n;
        float v = 0.f;
        for (int t = lane; t < n; t += 64) {
            const float dv = tile[t * pitch + cc] - mean;
            v = fmaf(dv, dv, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        const float denom = sqrtf(v / (float)(n - 1)) + eps;      // torch.std: unbiased; eps outside the sqrt
        for (int t = lane; t < T; t += 64) on[t] = (t < n) ? (tile[t * pitch + cc] - mean) / denom : 0.f;
    }
}

extern "C" int ign_instnorm_fwd_len(const float* x_btc, const int32_t* len_b, float* xn_bct, int B, int T, int C, float eps,
                                    void* stream) {
    static const char* who = "ign_instnorm_fwd_len";
    if (!x_btc || !len_b || !xn_bct || B <= 0 || T <= 0 || C <= 0) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d T=%d C=%d)", who, B, T, C);
        return IGN_E_ARG;
    }
    int CT = 32;                                                  // the tile rule of ign_instnorm_fwd
    while (CT > 1 && (size_t)T * (CT + 1) * 4 > 150 * 1024) CT >>= 1;
    const size_t lds = (size_t)T * (CT + 1) * 4;
    const int threads = lds > 64 * 1024 ? 1024 : 256;
    if (lds > 160 * 1024) {
        ign_set_error("%s: T=%d does not fit the LDS tile", who, T);
        return IGN_E_TOOBIG;
    }
    const int nct = (C + CT - 1) / CT;
    if ((long long)B * nct > 0x7fffffffLL) {
        ign_set_error("%s: B=%d C=%d needs more blocks than a grid has", who, B, C);
        return IGN_E_TOOBIG;
    }
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)instnorm_len_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    IgnScopedTimer tm("instnorm_len", (hipStream_t)stream);
    hipLaunchKernelGGL(instnorm_len_kernel, dim3((unsigned)B * nct), dim3(threads), lds, (hipStream_t)stream, x_btc, len_b, xn_bct,
                       B, T, C, CT, eps);
    return ign_check_launch("instnorm_len_kernel");
}

// ---------------------------------------------------------------------------------------------------- regate
struct ShpRegateArgs {
    float* d;             // (B,C,K,Tw) in / out
    const int32_t* len;   // (B)
    const float* thr;     // (K,C) or null
    float* p_out;         // (B,ld) + col0
    float* dmin_out;      // (B,ld) + col0
    int32_t* tstar;       // (B,K,C)
    float* zmu;           // (B,K,C,2)
    int B, C, T, K, L, Tw, stride, ld, col0, gate;
    long long rows;       // B*C*K
    float eps;
};

constexpr int REGATE_WAVES = 4;        // rows per block: waves share nothing (no LDS, no barrier)
constexpr int REGATE_U = 4;            // loads in flight per lane and trip of the row loop

__global__ void __launch_bounds__(64 * REGATE_WAVES) shp_regate_kernel(const ShpRegateArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * REGATE_WAVES + wave;
    if (row >= a.rows) return;                                    // wave-uniform: the DPP merges below run with every lane on
    const int ck = a.C * a.K;
    const int b = (int)(row / ck);
    const int r = (int)(row - (long long)b * ck);
    const int c = r / a.K, k = r - c * a.K;
    const int n = min(max(a.len[b], 0), a.T);                     // device data: clamped, so Tw_b <= Tw whatever it holds
    const int Twb = (n >= a.L) ? (n - a.L) / a.stride + 1 : 0;
    float* d = a.d + (size_t)row * a.Tw;

    float best = -INFINITY, rd = INFINITY, Z = 0.f, M = 0.f;
    int idx = 0x7fffffff;
    if (a.gate == GATE_RBF) {
        for (int t0 = lane; t0 < Twb; t0 += 64 * REGATE_U) {
            float dv[REGATE_U];
#pragma unroll
            for (int u = 0; u < REGATE_U; ++u) dv[u] = (t0 + 64 * u < Twb) ? d[t0 + 64 * u] : 0.f;
#pragma unroll
            for (int u = 0; u < REGATE_U; ++u) {
                const int t = t0 + 64 * u;
                if (t < Twb) {
                    const float uu = a.eps * dv[u];
                    const float p = __expf(-(uu * uu));
                    const float e = __expf(p);
                    Z += e;
                    M = fmaf(e, p, M);
                    if (p > best) { best = p; idx = t; }           // ascending t per lane: the first index stays on ties
                    rd = fminf(rd, dv[u]);
                }
            }
        }
    } else {
        // sweep 1: row minimum and its first index (best holds -d, so that the arg-max merge below is the arg-min)
        for (int t0 = lane; t0 < Twb; t0 += 64 * REGATE_U) {
            float dv[REGATE_U];
#pragma unroll
            for (int u = 0; u < REGATE_U; ++u) dv[u] = (t0 + 64 * u < Twb) ? d[t0 + 64 * u] : 0.f;
#pragma unroll
            for (int u = 0; u < REGATE_U; ++u) {
                const int t = t0 + 64 * u;
                if (t < Twb && -dv[u] > best) { best = -dv[u]; idx = t; }
            }
        }
    }
    for (int t = Twb + lane; t < a.Tw; t += 64) d[t] = IGN_NO_WINDOW;     // what the backward reads for an invalid window

    // ---- merge the 64 lanes (results in lane 63), first index on ties
    IGN_ARGMAX_STEP(DPP_QP_XOR1, 0xf);
    IGN_ARGMAX_STEP(DPP_QP_XOR2, 0xf);
    IGN_ARGMAX_STEP(DPP_HALF_MIRROR, 0xf);
    IGN_ARGMAX_STEP(DPP_MIRROR, 0xf);
    IGN_ARGMAX_STEP(DPP_BCAST15, 0xa);
    IGN_ARGMAX_STEP(DPP_BCAST31, 0xc);
    float dmin;
    if (a.gate == GATE_RBF) {
        dmin = wave_min_l63(rd);
    } else {
        dmin = -wave_bcast_l63(best);                             // every lane: the sums below are stabilised by the row minimum
        // sweep 2: soft-min sums; the valid part of the row is untouched by the fill above
        for (int t0 = lane; t0 < Twb; t0 += 64 * REGATE_U) {
            float dv[REGATE_U];
#pragma unroll
            for (int u = 0; u < REGATE_U; ++u) dv[u] = (t0 + 64 * u < Twb) ? d[t0 + 64 * u] : 0.f;
#pragma unroll
            for (int u = 0; u < REGATE_U; ++u) {
                if (t0 + 64 * u < Twb) {
                    const float e = __expf(dmin - dv[u]);
                    Z += e;
                    M = fmaf(e, dv[u], M);
                }
            }
        }
    }
    Z = wave_sum_l63(Z);
    M = wave_sum_l63(M);
    if (lane == 63) {
        const size_t col = (size_t)b * a.ld + a.col0 + (size_t)k * a.C + c;
        const size_t sidx = ((size_t)b * a.K + k) * a.C + c;
        if (Twb == 0) {                                           // no valid window: the feature is off and carries no gradient
            a.p_out[col] = 0.f;
            a.dmin_out[col] = IGN_NO_WINDOW;
            a.tstar[sidx] = -1;
            a.zmu[2 * sidx] = 1.f;
            a.zmu[2 * sidx + 1] = 0.f;
        } else {
            float pout = best;                                    // RBF: p[t*]
            if (a.gate == GATE_LTS) pout = 1.f / (1.f + __expf(-(a.thr[(size_t)k * a.C + c] - dmin)));
            a.p_out[col] = pout;
            a.dmin_out[col] = dmin;
            a.tstar[sidx] = idx;
            a.zmu[2 * sidx] = Z;
            a.zmu[2 * sidx + 1] = M / Z;
        }
    }
}

static int plan_regate(const char* who, float* d_save, const int32_t* len_b, const float* thr_kc, float* p_out, float* dmin_out, int ld,
                       int col0, int32_t* tstar, float* zmu, int B, int C, int T, int K, int L, int stride, float eps, int mode,
                       ShpRegateArgs* a) {
    if ((mode & ~0x3f) != 0 || (mode & 0xf) > IGN_DIST_PEARS) {   // the forward's range
        ign_set_error("%s: unknown mode 0x%x", who, mode);
        return IGN_E_ARG;
    }
    const int gate = (mode & IGN_GATE_LTS) ? GATE_LTS : GATE_RBF;
    if (B <= 0 || C <= 0 || T <= 0 || K <= 0 || L <= 0 || stride <= 0 || L > T) {
        ign_set_error("%s: bad dimensions B=%d C=%d T=%d K=%d L=%d stride=%d", who, B, C, T, K, L, stride);
        return IGN_E_ARG;
    }
    if (!d_save) {
        ign_set_error("%s: d_save is required (run the forward with d_save, then this pass)", who);
        return IGN_E_ARG;
    }
    if (!len_b || !p_out || !dmin_out || !tstar || !zmu || (gate == GATE_LTS && !thr_kc)) {
        ign_set_error("%s: null pointer argument", who);
        return IGN_E_ARG;
    }
    if (ld < col0 + K * C || col0 < 0) {
        ign_set_error("%s: output row pitch ld=%d too small for col0=%d + K*C=%d", who, ld, col0, K * C);
        return IGN_E_ARG;
    }
    const long long rows = (long long)B * C * K;
    if ((long long)C * K > 0x7fffffffLL || (rows + REGATE_WAVES - 1) / REGATE_WAVES > 0x7fffffffLL) {
        ign_set_error("%s: B*C*K=%lld rows need more blocks than a grid has", who, rows);
        return IGN_E_TOOBIG;
    }
    a->d = d_save; a->len = len_b; a->thr = thr_kc; a->p_out = p_out; a->dmin_out = dmin_out; a->tstar = tstar; a->zmu = zmu;
    a->B = B; a->C = C; a->T = T; a->K = K; a->L = L; a->Tw = (T - L) / stride + 1; a->stride = stride; a->ld = ld; a->col0 = col0;
    a->gate = gate; a->rows = rows; a->eps = eps;
    return 0;
}

static int launch_regate(const ShpRegateArgs& a, void* stream) {
    {
        IgnScopedTimer tm("shp_regate", (hipStream_t)stream);
        hipLaunchKernelGGL(shp_regate_kernel, dim3((unsigned)((a.rows + REGATE_WAVES - 1) / REGATE_WAVES)), dim3(64 * REGATE_WAVES), 0,
                           (hipStream_t)stream, a);
    }
    return ign_check_launch("shp_regate_kernel");
}

extern "C" int ign_shapelet_regate(float* d_save, const int32_t* len_b, const float* thr_kc, float* p_out, float* dmin_out, int ld,
                                   int col0, int32_t* tstar, float* zmu, int B, int C, int T, int K, int L, int stride, float eps,
                                   int mode, void* stream) {
    ShpRegateArgs a;
    int rc;
    if ((rc = plan_regate("ign_shapelet_regate", d_save, len_b, thr_kc, p_out, dmin_out, ld, col0, tstar, zmu, B, C, T, K, L, stride,
                          eps, mode, &a))) return rc;
    return launch_regate(a, stream);
}

extern "C" int ign_shapelet_regate_bank(int G, float* const* d_save, const int32_t* len_b, const float* const* thr_kc, float* p_out,
                                        float* dmin_out, int ld, const int* col0, int32_t* const* tstar, float* const* zmu, int B,
                                        int C, int T, const int* K, const int* L, const int* stride, float eps, int mode,
                                        void* stream) {
    static const char* who = "ign_shapelet_regate_bank";
    if (G <= 0 || G > SHP_MAX_GROUPS || !d_save || !col0 || !tstar || !zmu || !K || !L || !stride) {
        ign_set_error("%s: G=%d outside 1..%d or null table", who, G, SHP_MAX_GROUPS);
        return IGN_E_ARG;
    }
    ShpRegateArgs a[SHP_MAX_GROUPS];
    int rc;
    for (int g = 0; g < G; ++g)          // validate every group before the first launch
        if ((rc = plan_regate(who, d_save[g], len_b, thr_kc ? thr_kc[g] : nullptr, p_out, dmin_out, ld, col0[g], tstar[g], zmu[g], B, C,
                              T, K[g], L[g], stride[g], eps, mode, &a[g]))) return rc;
    for (int g = 0; g < G; ++g)
        if ((rc = launch_regate(a[g], stream))) return rc;
    return 0;
}
