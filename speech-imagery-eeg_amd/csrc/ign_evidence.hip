// Evidence maps (utils/evidence.py, run.py --evidence): the logit of one class per sample laid out over time and electrodes, from what
// the forward already produced.  The rule -- every rounding -- is ign_evidence.h.
//
// evidence_kernel: a gather, no atomics, no workspace, every element of out (B,T,C) written once.  Write-bound on paper (one (B,T,C)
// write against (B,ld) reads); what it executes per element is sum K compare-select-adds, because the rule fixes the order of the
// sum.  A block owns one sample, EV_TILE = 64 consecutive time rows and LX = 4 R electrodes, R the template parameter: lanes run
// along c, the contiguous axis of p, t, W and out, and a lane keeps R rows (tile row ly + j * NY, NY = 64 / R) of its electrode in
// registers.  The (start, len, value) terms of the block's electrodes are formed once per block into LDS, [feature][lane] so that a
// wave reads consecutive words, EV_LDS_TERMS at a time: any sum K runs as ceil(sum K * LX / EV_LDS_TERMS) chunks of the same loop.
//
// bn_relu_cam_kernel: read-bound, one 16-byte read of y_last per lane and step.  A block owns one sample and CAM_ROWS time rows; a
// row is covered by lpr = the smallest power of two >= Cl / 4 lanes (at most a wave), so a wave carries 64 / lpr rows, and the sum
// over c is a lane's fma chain followed by a butterfly over those lanes: a fixed order, bitwise repeatable.
#include <cstdint>
#include "ign_common.h"
#include "ign_evidence.h"

constexpr int EV_THREADS = 256;
constexpr int EV_TILE = 64;                 // time rows per block
constexpr int EV_LDS_TERMS = 2048;          // terms staged at a time: 24 KB of LDS

struct EvArgs {
    const float* p;          // (B,ld)
    const int32_t* t;        // (B,ld)
    const float* W;          // (N,ld)
    const int32_t* target;   // (B)
    const float* scale;      // (B) or null
    float* out;              // (B,T,C)
    int T, C, N, ld, G, ntile, nfeat;
    int K[SHP_MAX_GROUPS], L[SHP_MAX_GROUPS], stride[SHP_MAX_GROUPS], col0[SHP_MAX_GROUPS], Tw[SHP_MAX_GROUPS];
    float invL[SHP_MAX_GROUPS];
};

template <int R>
__global__ void __launch_bounds__(EV_THREADS) evidence_kernel(const EvArgs a) {
    constexpr int NY = EV_TILE / R, LX = EV_THREADS / NY, FCH = EV_LDS_TERMS / LX;
    __shared__ int s_start[EV_LDS_TERMS], s_len[EV_LDS_TERMS];
    __shared__ float s_v[EV_LDS_TERMS];
    __shared__ int s_K[SHP_MAX_GROUPS], s_L[SHP_MAX_GROUPS], s_stride[SHP_MAX_GROUPS], s_col0[SHP_MAX_GROUPS], s_Tw[SHP_MAX_GROUPS];
    __shared__ float s_invL[SHP_MAX_GROUPS];
    const int tid = threadIdx.x, lx = tid % LX, ly = tid / LX;
    const int b = blockIdx.x / a.ntile;
    const int r0 = (blockIdx.x - b * a.ntile) * EV_TILE;
    const int c0 = blockIdx.y * LX, c = c0 + lx;
    const int C = a.C, G = a.G;
    const int n = a.target[b];
    const bool tgt_ok = n >= 0 && n < a.N;                        // device data: checked, never trusted as an index bound
    if (tid < SHP_MAX_GROUPS) {                                   // the group tables, indexed per thread below
        s_K[tid] = a.K[tid]; s_L[tid] = a.L[tid]; s_stride[tid] = a.stride[tid]; s_col0[tid] = a.col0[tid]; s_Tw[tid] = a.Tw[tid];
        s_invL[tid] = a.invL[tid];
    }
    const float* pb = a.p + (size_t)b * a.ld;
    const int32_t* tb = a.t + (size_t)b * a.ld;
    const float* wn = a.W + (size_t)(tgt_ok ? n : 0) * a.ld;
    float acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = 0.0f;
    for (int f0 = 0; f0 < a.nfeat; f0 += FCH) {
        const int nf = min(FCH, a.nfeat - f0);
        __syncthreads();                                          // the tables are in place / the previous chunk is consumed
        for (int i = tid; i < nf * LX; i += EV_THREADS) {
            const int cc = c0 + (i % LX);
            int g = 0, k = f0 + i / LX;                           // the feature's group: g, k ascending is the rule's order
            while (g < G - 1 && k >= s_K[g]) k -= s_K[g++];
            IgnEvTerm term = {0, 0, 0.0f};
            if (cc < C && tgt_ok) {
                const int col = s_col0[g] + k * C + cc;
                term = ign_evidence_term(wn[col], pb[col], tb[col], s_stride[g], s_L[g], s_Tw[g], s_invL[g]);
            }
            s_start[i] = term.start;
            s_len[i] = term.len;
            s_v[i] = term.v;
        }
        __syncthreads();
        for (int f = 0; f < nf; ++f) {
            const int st = s_start[f * LX + lx], ln = s_len[f * LX + lx];
            const float v = s_v[f * LX + lx];
#pragma unroll
            for (int j = 0; j < R; ++j) acc[j] = ign_evidence_add(acc[j], r0 + ly + j * NY, st, ln, v);
        }
    }
    if (c >= C) return;
    const bool scaled = a.scale != nullptr;
    const float sc = scaled ? a.scale[b] : 1.0f;
    float* ob = a.out + ((size_t)b * a.T + r0) * C + c;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int r = ly + j * NY;
        if (r0 + r < a.T) ob[(size_t)r * C] = scaled ? acc[j] * sc : acc[j];
    }
}

template <int R>
static void evidence_launch(const EvArgs& a, int B, hipStream_t s) {
    constexpr int LX = EV_THREADS / (EV_TILE / R);
    const dim3 grid((unsigned)(B * a.ntile), (unsigned)((a.C + LX - 1) / LX)), block(EV_THREADS);
    hipLaunchKernelGGL(evidence_kernel<R>, grid, block, 0, s, a);
}

extern "C" int ign_shapelet_evidence_bank(const float* p, const int32_t* t, const float* W, const int32_t* target, const float* scale,
                                          int ld, int G, const int* K, const int* L, const int* stride, const int* col0,
                                          const float* invL, float* out, int B, int T, int C, int N, void* stream) {
    static const char* who = "ign_shapelet_evidence_bank";
    if (!p || !t || !W || !target || !out || !K || !L || !stride || !col0 || !invL || B < 1 || T < 1 || C < 1 || N < 1) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d T=%d C=%d N=%d)", who, B, T, C, N);
        return IGN_E_ARG;
    }
    if (G < 1 || G > SHP_MAX_GROUPS) {
        ign_set_error("%s: G=%d outside 1..%d", who, G, SHP_MAX_GROUPS);
        return IGN_E_ARG;
    }
    EvArgs a = {};
    long long col = 0, nfeat = 0;
    for (int g = 0; g < G; ++g) {
        if (K[g] < 1 || L[g] < 1 || L[g] > T || stride[g] < 1) {
            ign_set_error("%s: group %d: K=%d L=%d stride=%d with T=%d", who, g, K[g], L[g], stride[g], T);
            return IGN_E_ARG;
        }
        if (col0[g] != col) {
            ign_set_error("%s: group %d starts at column %d, the groups before it end at %lld", who, g, col0[g], col);
            return IGN_E_ARG;
        }
        col += (long long)K[g] * C;
        nfeat += K[g];
        if (col > 0x7fff0000LL) {
            ign_set_error("%s: more than 2^31 - 65536 feature columns", who);
            return IGN_E_TOOBIG;
        }
        a.K[g] = K[g]; a.L[g] = L[g]; a.stride[g] = stride[g]; a.col0[g] = col0[g]; a.invL[g] = invL[g];
        a.Tw[g] = (T - L[g]) / stride[g] + 1;
    }
    if (col != ld) {
        ign_set_error("%s: ld=%d, the groups hold %lld columns", who, ld, col);
        return IGN_E_ARG;
    }
    const long long ntile = ((long long)T + EV_TILE - 1) / EV_TILE;
    if ((long long)T * C > 0x7fff0000LL || (long long)B * ntile > 0x7fffffffLL || (C + 3) / 4 > 65535) {
        ign_set_error("%s: B=%d T=%d C=%d does not fit 32-bit indices or a grid", who, B, T, C);
        return IGN_E_TOOBIG;
    }
    a.p = p; a.t = t; a.W = W; a.target = target; a.scale = scale; a.out = out;
    a.T = T; a.C = C; a.N = N; a.ld = ld; a.G = G; a.ntile = (int)ntile; a.nfeat = (int)nfeat;
    hipStream_t s = (hipStream_t)stream;
    {
        IgnScopedTimer tm("evidence", s);
        if (C <= 4) evidence_launch<1>(a, B, s);
        else if (C <= 8) evidence_launch<2>(a, B, s);
        else if (C <= 16) evidence_launch<4>(a, B, s);
        else if (C <= 32) evidence_launch<8>(a, B, s);
        else if (C <= 64) evidence_launch<16>(a, B, s);
        else if (C <= 128) evidence_launch<32>(a, B, s);
        else evidence_launch<64>(a, B, s);
    }
    return ign_check_launch("evidence_kernel");
}

// ---------------------------------------------------------------- FCN expert: class activation map on block 3's axis
constexpr int CAM_THREADS = 256;
constexpr int CAM_ROWS = 64;                // time rows per block

__global__ void __launch_bounds__(CAM_THREADS) bn_relu_cam_kernel(const float* __restrict__ y, const float* __restrict__ a,
                                                                  const float* __restrict__ b, const float* __restrict__ W,
                                                                  const int32_t* __restrict__ target, const float* __restrict__ scale,
                                                                  float* __restrict__ cam, int Tl, int Cl, int N, int ntile,
                                                                  int lpr_log2, float invT) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lpr = 1 << lpr_log2, rpw = 64 >> lpr_log2;         // lanes per row, rows per wave
    const int li = lane & (lpr - 1), rsub = lane >> lpr_log2;
    const int bi = blockIdx.x / ntile;
    const int r0 = (blockIdx.x - bi * ntile) * CAM_ROWS;
    const int n = target[bi];
    const bool tgt_ok = n >= 0 && n < N;
    const int c4n = Cl >> 2;
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    const float4* w4 = reinterpret_cast<const float4*>(W + (size_t)(tgt_ok ? n : 0) * Cl);
    const bool one = c4n <= lpr;                                  // a lane sees one channel quad: its coefficients stay in registers
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 av = zero4, bv = zero4, wv = zero4;
    if (one && li < c4n) { av = a4[li]; bv = b4[li]; wv = w4[li]; }
    const float sc = scale ? scale[bi] : 1.0f;
    for (int q = wave * rpw + rsub; q < CAM_ROWS; q += (CAM_THREADS / 64) * rpw) {       // wave-uniform trip count
        const int t = r0 + q;
        float s = 0.0f;
        if (t < Tl && tgt_ok) {
            const float4* y4 = reinterpret_cast<const float4*>(y + ((size_t)bi * Tl + t) * Cl);
            for (int c4 = li; c4 < c4n; c4 += lpr) {
                if (!one) { av = a4[c4]; bv = b4[c4]; wv = w4[c4]; }
                const float4 yv = y4[c4];
                s = fmaf(wv.x, fmaxf(fmaf(av.x, yv.x, bv.x), 0.f), s);
                s = fmaf(wv.y, fmaxf(fmaf(av.y, yv.y, bv.y), 0.f), s);
                s = fmaf(wv.z, fmaxf(fmaf(av.z, yv.z, bv.z), 0.f), s);
                s = fmaf(wv.w, fmaxf(fmaf(av.w, yv.w, bv.w), 0.f), s);
            }
        }
        for (int o = lpr >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (li == 0 && t < Tl) {
            s = s * invT;
            cam[(size_t)bi * Tl + t] = scale ? s * sc : s;
        }
    }
}

extern "C" int ign_bn_relu_cam_fwd(const float* y_last, const float* a, const float* b, const float* head_w, const int32_t* target,
                                   const float* scale, float* cam, int B, int Tl, int Cl, int N, void* stream) {
    static const char* who = "ign_bn_relu_cam_fwd";
    if (!y_last || !a || !b || !head_w || !target || !cam || B < 1 || Tl < 1 || N < 1) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d Tl=%d N=%d)", who, B, Tl, N);
        return IGN_E_ARG;
    }
    if (Cl < 4 || Cl % 4 || Cl > 1024) {
        ign_set_error("%s: Cl=%d must be a multiple of 4 in 4..1024", who, Cl);
        return IGN_E_ARG;
    }
    if ((((uintptr_t)y_last | (uintptr_t)a | (uintptr_t)b | (uintptr_t)head_w) & 15) != 0) {
        ign_set_error("%s: y_last, a, b and head_w must be 16-byte aligned", who);
        return IGN_E_ARG;
    }
    const long long ntile = ((long long)Tl + CAM_ROWS - 1) / CAM_ROWS;
    if ((long long)B * ntile > 0x7fffffffLL) {
        ign_set_error("%s: B=%d Tl=%d needs more blocks than a grid has", who, B, Tl);
        return IGN_E_TOOBIG;
    }
    int lpr_log2 = 0;
    while ((1 << lpr_log2) < Cl / 4 && lpr_log2 < 6) ++lpr_log2;
    {
        IgnScopedTimer tm("bn_relu_cam", (hipStream_t)stream);
        hipLaunchKernelGGL(bn_relu_cam_kernel, dim3((unsigned)(B * ntile)), dim3(CAM_THREADS), 0, (hipStream_t)stream, y_last, a, b,
                           head_w, target, scale, cam, Tl, Cl, N, (int)ntile, lpr_log2, 1.0f / (float)Tl);
    }
    return ign_check_launch("bn_relu_cam_kernel");
}

// ---------------------------------------------------------------- cam on the input axis
__global__ void __launch_bounds__(256) cam_spread_kernel(const float* __restrict__ cam, float* __restrict__ out, long long total,
                                                         int Tl, int T, int R, float invR) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long bi = i / T;
    const int s = (int)(i - bi * T);
    out[i] = ign_cam_spread_at(cam + bi * Tl, s, Tl, R, invR);
}

extern "C" int ign_cam_spread(const float* cam, float* out, int B, int Tl, int R, float invR, void* stream) {
    static const char* who = "ign_cam_spread";
    if (!cam || !out || B < 1 || Tl < 1 || R < 1) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d Tl=%d R=%d)", who, B, Tl, R);
        return IGN_E_ARG;
    }
    const long long T = (long long)Tl + R - 1, total = (long long)B * T;
    if (T > 0x7fff0000LL || (total + 255) / 256 > 0x7fffffffLL) {
        ign_set_error("%s: B=%d Tl=%d R=%d does not fit a grid", who, B, Tl, R);
        return IGN_E_TOOBIG;
    }
    {
        IgnScopedTimer tm("cam_spread", (hipStream_t)stream);
        hipLaunchKernelGGL(cam_spread_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cam, out, total,
                           Tl, (int)T, R, invR);
    }
    return ign_check_launch("cam_spread_kernel");
}
