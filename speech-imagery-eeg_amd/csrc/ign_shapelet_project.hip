// Shapelet projection (utils/shapelet_project.py, run.py --shapelet_project): snap every shapelet of a length group to the nearest
// window of the training set, streamed batch by batch.  The expensive half -- the sliding distance of every shapelet to every
// window, its minimum per sample and the window that attains it -- is the shapelet forward (ign_shapelet_fwd.h, ign_shapelet_mask.hip);
// this pass runs behind it on its (B, ld) outputs dmin / tstar and adds the reduction over the samples and the gather of the winner.
// One launch, a block owns 64 consecutive features f = k*C + c of the group:
//   scan    lane <-> feature, so a row of dmin / tstar is read coalesced; wave s of the block walks the s-th contiguous slice of
//           the batch in ascending b with a strict < (first index on ties; a NaN or +inf never wins; tstar outside 0 .. Tw-1 is no
//           candidate, so device data is never trusted as an address);
//   merge   wave 0 takes the slices' results from LDS in ascending s (still the lowest b on ties), compares with the running best
//           (strict <: the earlier batch keeps a tie) and writes best_d / best_src -- one writer per element;
//   gather  the waves share the block's replaced features; the 64 lanes of a wave copy the L floats of one winner, coalesced.
// No atomics, no workspace, a fixed order: bitwise repeatable.  The pass reads 8 bytes per (sample, feature) and moves at most
// K*C*L floats: tiny beside the forward that produced its input.
#include "ign_common.h"

namespace {

constexpr int PROJ_SLICES = 8;         // waves per block = slices of the batch scanned side by side

struct ShpProjectArgs {
    const float* xn;        // (B,C,T)
    const float* dmin;      // (B,ld) + col0
    const int32_t* tstar;   // (B,ld) + col0
    float* best_d;          // (K,C)
    int32_t* best_src;      // (K,C,2)
    float* cand;            // (K,C,L)
    int B, C, T, KC, L, Tw, stride, ld, col0, sample0, accumulate;
    int rps;                // batch rows per slice
};

__global__ void __launch_bounds__(64 * PROJ_SLICES) shp_project_kernel(const ShpProjectArgs a) {
    __shared__ float s_d[PROJ_SLICES][64];
    __shared__ int s_b[PROJ_SLICES][64];
    __shared__ int s_t[PROJ_SLICES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f0 = blockIdx.x * 64, f = f0 + lane;

    float bd = INFINITY;
    int bb = -1, bt = -1;
    if (f < a.KC) {
        const int b_lo = wave * a.rps, b_hi = min(a.B, b_lo + a.rps);
        const size_t col = (size_t)a.col0 + f;
#pragma unroll 4
        for (int b = b_lo; b < b_hi; ++b) {
            const size_t i = (size_t)b * a.ld + col;
            const float d = a.dmin[i];
            const int t = a.tstar[i];
            if (t >= 0 && t < a.Tw && d < bd) { bd = d; bb = b; bt = t; }
        }
    }
    s_d[wave][lane] = bd;
    s_b[wave][lane] = bb;
    s_t[wave][lane] = bt;
    __syncthreads();

    if (wave == 0) {
        for (int s = 1; s < PROJ_SLICES; ++s) {
            const float d = s_d[s][lane];
            if (d < bd) { bd = d; bb = s_b[s][lane]; bt = s_t[s][lane]; }
        }
        if (f < a.KC) {
            const bool take = bb >= 0 && (!a.accumulate || bd < a.best_d[f]);
            if (take) {
                a.best_d[f] = bd;
                a.best_src[2 * (size_t)f] = a.sample0 + bb;
                a.best_src[2 * (size_t)f + 1] = bt;
            } else {
                if (!a.accumulate) {                               // a first batch without a candidate
                    a.best_d[f] = INFINITY;
                    a.best_src[2 * (size_t)f] = -1;
                    a.best_src[2 * (size_t)f + 1] = -1;
                }
                bb = -1;
            }
        }
        s_b[0][lane] = bb;                                          // >= 0: this feature's row of cand is replaced
        s_t[0][lane] = bt;
    }
    __syncthreads();

    const int nf = min(64, a.KC - f0);
    for (int i = wave; i < nf; i += PROJ_SLICES) {
        const int b = s_b[0][i];                                    // wave-uniform
        if (b < 0) continue;
        const int c = (f0 + i) % a.C;
        const float* src = a.xn + ((size_t)b * a.C + c) * a.T + (size_t)s_t[0][i] * a.stride;     // t < Tw: the window ends inside the row
        float* dst = a.cand + (size_t)(f0 + i) * a.L;
        for (int l = lane; l < a.L; l += 64) dst[l] = src[l];
    }
}

int plan_project(const char* who, const float* xn, const float* dmin, const int32_t* tstar, int ld, int col0, int sample0,
                 float* best_d, int32_t* best_src, float* cand, int accumulate, int B, int C, int T, int K, int L, int stride,
                 ShpProjectArgs* a) {
    if (B <= 0 || C <= 0 || T <= 0 || K <= 0 || L <= 0 || stride <= 0 || L > T) {
        ign_set_error("%s: bad dimensions B=%d C=%d T=%d K=%d L=%d stride=%d", who, B, C, T, K, L, stride);
        return IGN_E_ARG;
    }
    if (!xn || !dmin || !tstar || !best_d || !best_src || !cand) {
        ign_set_error("%s: null pointer argument", who);
        return IGN_E_ARG;
    }
    if ((long long)K * C > 0x7fffffffLL - 64) {
        ign_set_error("%s: K*C = %lld features exceed the index range", who, (long long)K * C);
        return IGN_E_ARG;
    }
    if (col0 < 0 || (long long)ld < (long long)col0 + (long long)K * C) {
        ign_set_error("%s: row pitch ld=%d too small for col0=%d + K*C=%d", who, ld, col0, K * C);
        return IGN_E_ARG;
    }
    if (accumulate != 0 && accumulate != 1) {
        ign_set_error("%s: accumulate=%d is neither 0 nor 1", who, accumulate);
        return IGN_E_ARG;
    }
    if (sample0 < 0 || (long long)sample0 + B > 0x7fffffffLL) {
        ign_set_error("%s: sample0=%d with B=%d leaves the int32 range of a sample ordinal", who, sample0, B);
        return IGN_E_ARG;
    }
    a->xn = xn; a->dmin = dmin; a->tstar = tstar; a->best_d = best_d; a->best_src = best_src; a->cand = cand;
    a->B = B; a->C = C; a->T = T; a->KC = K * C; a->L = L; a->Tw = (T - L) / stride + 1; a->stride = stride; a->ld = ld; a->col0 = col0;
    a->sample0 = sample0; a->accumulate = accumulate; a->rps = (B + PROJ_SLICES - 1) / PROJ_SLICES;
    return 0;
}

int launch_project(const ShpProjectArgs& a, void* stream) {
    {
        IgnScopedTimer tm("shp_project", (hipStream_t)stream);
        hipLaunchKernelGGL(shp_project_kernel, dim3((unsigned)((a.KC + 63) / 64)), dim3(64 * PROJ_SLICES), 0, (hipStream_t)stream, a);
    }
    return ign_check_launch("shp_project_kernel");
}

}  // namespace

extern "C" int ign_shapelet_project_step(const float* xn_bct, const float* dmin, const int32_t* tstar, int ld, int col0, int sample0,
                                         float* best_d_kc, int32_t* best_src_kc2, float* cand_kcl, int accumulate, int B, int C,
                                         int T, int K, int L, int stride, void* stream) {
    ShpProjectArgs a;
    int rc;
    if ((rc = plan_project("ign_shapelet_project_step", xn_bct, dmin, tstar, ld, col0, sample0, best_d_kc, best_src_kc2, cand_kcl,
                           accumulate, B, C, T, K, L, stride, &a))) return rc;
    return launch_project(a, stream);
}

extern "C" int ign_shapelet_project_step_bank(const float* xn_bct, const float* dmin, const int32_t* tstar, int ld, int G,
                                              const int* col0, int sample0, float* const* best_d_kc, int32_t* const* best_src_kc2,
                                              float* const* cand_kcl, int accumulate, int B, int C, int T, const int* K, const int* L,
                                              const int* stride, void* stream) {
    static const char* who = "ign_shapelet_project_step_bank";
    if (G <= 0 || G > SHP_MAX_GROUPS || !col0 || !best_d_kc || !best_src_kc2 || !cand_kcl || !K || !L || !stride) {
        ign_set_error("%s: G=%d outside 1..%d or null table", who, G, SHP_MAX_GROUPS);
        return IGN_E_ARG;
    }
    ShpProjectArgs a[SHP_MAX_GROUPS];
    int rc;
    for (int g = 0; g < G; ++g)          // validate every group before the first launch
        if ((rc = plan_project(who, xn_bct, dmin, tstar, ld, col0[g], sample0, best_d_kc[g], best_src_kc2[g], cand_kcl[g], accumulate, B,
                               C, T, K[g], L[g], stride[g], &a[g]))) return rc;
    for (int g = 0; g < G; ++g)
        if ((rc = launch_project(a[g], stream))) return rc;
    return 0;
}
