// Shapelet backward w.r.t. the INPUT (dloss/dxn): the third sliding pass, with the output on the sample axis.
//
//   gxn[b,c,s] (+)= sum_k sum_{(t,j): t*stride + j = s}  dl/dd[b,t,k,c] * dd/dx
//       L1 : dd/dx = sign(x[b,c,s] - w[k,c,j]) / L          MSE: dd/dx = 2 (x[b,c,s] - w[k,c,j]) / L
// dl/dd is the coefficient the weight pass (ign_shapelet_bwd.h) forms from the saved distances d_t, the row statistics
// {t*, Z, mu} and the upstream gradient of the gate output; shp_dldd below restates it term by term.
//
// Mapping (fp32 VALU bound, the same E = B*C*K*Tw*L element-ops as the weight pass; plain C++: compare, select, add).
//   * a block owns a tile of SHP_BWDX_TILE samples of one (b, c) row; a wave owns 64*SPL consecutive samples, lane <-> sample
//     s = wave_base + i*64 + lane: x[s] and its accumulator stay in registers for the whole pass, and every output sample is
//     written by exactly one lane -- no cross-lane reduction, no float atomics, a fixed summation order;
//   * a sample s = q*stride + r meets shapelet position j = r + m*stride in window t = q - m.  Per stage of `kb` shapelets and
//     per chunk of `mc` offsets m the block stages w[k,c, m0*stride : (m0+mc)*stride) and A[k][t] = dl/dd * (1 or 2)/L for
//     every window the tile can meet (zero outside [0, Tw)) in LDS; the inner step reads w as a broadcast (stride 1) and
//     A[q - m] from consecutive addresses in consecutive lanes;
//   * stride 1: offsets no sample of the wave can meet (m > s or s - m >= Tw for all of them) are skipped wave-uniformly;
//   * a shapelet longer than one chunk is walked chunk by chunk (any L <= T), A being recomputed per chunk.
// The G groups of a bank run one after another on the stream; the first overwrites gxn, the others add to it.
#include "ign_common.h"
#include <algorithm>

// dl/dd_t of one window from its saved distance: RBF gate exp(-(eps d)^2) under the straight-through max, or the LTS
// straight-through soft-min under sigmoid(thr - min_d) (gm = -g P (1 - P)).  Same terms, same order as shp_bwd_kernel.
__device__ __forceinline__ float shp_dldd(int gate, float d1, int t, int ts, float gv, float invZ, float mu, float gm, float dmin,
                                          float eps, float two_eps2) {
    const float hard = (t == ts) ? 1.f : 0.f;
    if (gate == GATE_RBF) {
        const float uu = eps * d1;
        const float pp = __expf(-(uu * uu));
        const float e = __expf(pp);
        const float coef = gv * (hard + e * invZ * (pp - mu));
        return coef * (-two_eps2 * d1 * pp);
    }
    const float sft = __expf(dmin - d1) * invZ;
    return gm * (hard + sft * (mu - d1));
}

// TIE (IGN_TIE_EXACT, L1 only): the step adds av where x > w, subtracts it where x < w and adds nothing where x == w.
template <int DIST, bool S1, bool TIE = false>
__global__ void __launch_bounds__(SHP_BWDX_THREADS) shp_bwdx_kernel(const ShpBwdXArgs a) {
    constexpr int SPL = SHP_BWDX_SPL, TILE = SHP_BWDX_TILE, NT = SHP_BWDX_THREADS;
    static_assert(!TIE || DIST == DIST_L1, "the exact-tie variant exists for L1 only");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int stride = S1 ? 1 : a.stride;
    const int wlen = a.mc * stride;
    float* ws = smem;                        // [kb][wlen]   w[k,c, m0*stride + i]
    float* As = ws + a.kb * wlen;            // [kb][na]     A[k][tlo + u]
    float* Par = As + a.kb * a.na;           // [kb][8]      per-shapelet scalars of this row

    const int tile = (int)(blockIdx.x % (unsigned)a.ntile);
    const size_t rowi = blockIdx.x / (unsigned)a.ntile;                // b*C + c
    const int c = (int)(rowi % (size_t)a.C), b = (int)(rowi / (size_t)a.C);
    const int s0 = tile * TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sw0 = s0 + wave * 64 * SPL;
    const float* row = a.xn + rowi * a.T;

    float x[SPL], acc[SPL];
    int q[SPL], r[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        const int s = sw0 + i * 64 + lane;
        x[i] = (s < a.T) ? row[s] : 0.f;
        q[i] = S1 ? s : s / stride;
        r[i] = S1 ? 0 : s - q[i] * stride;
        acc[i] = 0.f;
    }
    // offsets m that a sample range [lo, hi] can meet: window t = q - m must lie in [0, Tw)
    const int qmin = s0 / stride, qmax = (s0 + TILE - 1) / stride;
    const int mlo_b = max(0, qmin - (a.Tw - 1)), mhi_b = min(a.M - 1, qmax);
    const int mlo_w = max(0, sw0 / stride - (a.Tw - 1)), mhi_w = min(a.M - 1, (sw0 + 64 * SPL - 1) / stride);
    const float two_eps2 = 2.f * a.eps * a.eps;
    const float ascale = (DIST == DIST_L1) ? a.invL : 2.f * a.invL;

    for (int k0 = 0; k0 < a.K; k0 += a.kb) {
        const int kcount = min(a.kb, a.K - k0);
        bool first = true;
        for (int m0 = (mlo_b / a.mc) * a.mc; m0 <= mhi_b; m0 += a.mc) {      // block-uniform
            __syncthreads();                     // previous chunk fully consumed
            if (first && tid < kcount) {
                const int k = k0 + tid;
                const size_t sidx = ((size_t)b * a.K + k) * a.C + c;
                const size_t col = (size_t)b * a.ld + a.col0 + (size_t)k * a.C + c;
                const float gv = a.g[col];
                float gm = 0.f, dmin = 0.f;
                if (a.gate == GATE_LTS) {
                    const float P = a.p[col];
                    gm = -gv * P * (1.f - P);       // dP/dm = -sigma'(thr - m)
                    dmin = a.dmin[col];
                }
                float* pr = Par + tid * 8;
                pr[0] = gv; pr[1] = __int_as_float(a.tstar[sidx]); pr[2] = 1.f / a.zmu[2 * sidx]; pr[3] = a.zmu[2 * sidx + 1];
                pr[4] = gm; pr[5] = dmin;
            }
            first = false;
            for (int kk = 0; kk < kcount; ++kk) {
                const float* wk = a.w + ((size_t)(k0 + kk) * a.C + c) * a.L;
                for (int i = tid; i < wlen; i += NT) {
                    const int j = m0 * stride + i;
                    ws[kk * wlen + i] = (j < a.L) ? wk[j] : 0.f;
                }
            }
            __syncthreads();
            const int tlo = qmin - (m0 + a.mc - 1);
            for (int kk = 0; kk < kcount; ++kk) {
                const float* pr = Par + kk * 8;
                const float gv = pr[0], invZ = pr[2], mu = pr[3], gm = pr[4], dmin = pr[5];
                const int ts = __float_as_int(pr[1]);
                const float* dk = a.d + (rowi * a.K + (size_t)(k0 + kk)) * a.Tw;
                for (int u = tid; u < a.na; u += NT) {
                    const int t = tlo + u;
                    float A = 0.f;
                    if (t >= 0 && t < a.Tw)
                        A = ascale * shp_dldd(a.gate, dk[t], t, ts, gv, invZ, mu, gm, dmin, a.eps, two_eps2);
                    As[kk * a.na + u] = A;
                }
            }
            __syncthreads();

            const int ma = max(m0, mlo_w), mb = min(m0 + a.mc - 1, mhi_w);    // wave-uniform
            for (int kk = 0; kk < kcount; ++kk) {
                const float* wsk = ws + kk * wlen;
                const float* ab[SPL];
#pragma unroll
                for (int i = 0; i < SPL; ++i) ab[i] = As + kk * a.na + (q[i] - qmin) + (a.mc - 1);
#pragma unroll 4
                for (int m = ma; m <= mb; ++m) {
                    const int mm = m - m0;
                    if (S1) {
                        const float wj = wsk[mm];
#pragma unroll
                        for (int i = 0; i < SPL; ++i) {
                            const float av = ab[i][-mm];
                            if (TIE)                  acc[i] += (x[i] > wj) ? av : (x[i] < wj) ? -av : 0.f;
                            else if (DIST == DIST_L1) acc[i] += (x[i] > wj) ? av : -av;
                            else                      acc[i] = fmaf(av, x[i] - wj, acc[i]);
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < SPL; ++i) {
                            const int jl = r[i] + mm * stride;                  // < wlen; position j = m0*stride + jl
                            const float wj = wsk[jl];
                            const float av = (m0 * stride + jl < a.L) ? ab[i][-mm] : 0.f;
                            if (TIE)                  acc[i] += (x[i] > wj) ? av : (x[i] < wj) ? -av : 0.f;
                            else if (DIST == DIST_L1) acc[i] += (x[i] > wj) ? av : -av;
                            else                      acc[i] = fmaf(av, x[i] - wj, acc[i]);
                        }
                    }
                }
            }
        }
    }

    float* out = a.gx + rowi * a.T;
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        const int s = sw0 + i * 64 + lane;
        if (s < a.T) out[s] = a.accumulate ? out[s] + acc[i] : acc[i];
    }
}

// kb shapelets per stage, mc offsets per chunk: <= 512 shapelet positions and <= TILE + 512 window coefficients per shapelet,
// two shapelets per stage -> <= 17 KB of LDS per 4-wave block (8 blocks per CU).
size_t ign_bwdx_plan(ShpBwdXArgs* a) {
    a->ntile = (a->T + SHP_BWDX_TILE - 1) / SHP_BWDX_TILE;
    a->M = (a->L + a->stride - 1) / a->stride;
    a->mc = std::min(a->M, std::max(1, 512 / a->stride));
    a->na = (((SHP_BWDX_TILE - 1) / a->stride + 1 + a->mc) + 3) & ~3;
    a->kb = std::min(a->K, 2);
    return ((size_t)a->kb * ((size_t)a->mc * a->stride + a->na + 8)) * sizeof(float);
}

int ign_launch_bwdx(const ShpBwdXArgs& a, int dist, bool tie_exact, size_t lds, hipStream_t s) {
    const dim3 grid((unsigned)((size_t)a.B * a.C * a.ntile)), block(SHP_BWDX_THREADS);
    IgnScopedTimer tm("shp_bwd_x", s);
    if (dist == DIST_L1 && tie_exact) {
        if (a.stride == 1) hipLaunchKernelGGL((shp_bwdx_kernel<DIST_L1, true, true>), grid, block, lds, s, a);
        else               hipLaunchKernelGGL((shp_bwdx_kernel<DIST_L1, false, true>), grid, block, lds, s, a);
    } else if (dist == DIST_L1) {
        if (a.stride == 1) hipLaunchKernelGGL((shp_bwdx_kernel<DIST_L1, true>), grid, block, lds, s, a);
        else               hipLaunchKernelGGL((shp_bwdx_kernel<DIST_L1, false>), grid, block, lds, s, a);
    } else {
        if (a.stride == 1) hipLaunchKernelGGL((shp_bwdx_kernel<DIST_MSE, true>), grid, block, lds, s, a);
        else               hipLaunchKernelGGL((shp_bwdx_kernel<DIST_MSE, false>), grid, block, lds, s, a);
    }
    return ign_check_launch("shp_bwdx_kernel");
}
