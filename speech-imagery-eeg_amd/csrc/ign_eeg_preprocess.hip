// On-device EEG preprocessing in front of the standardisation (run.py --eeg_preprocess; ops.eeg_filterbank, ops.eeg_preprocess; the numpy
// restatement is utils/eeg_filter.py:filterbank_numpy): raw (B, Cin, Tin) recordings -> nb <= 8 zero-phase FIR filters of one common
// length M, decimate by q, crop / zero-pad every band to (Tout, Cout), per-row standardise over the valid part, transpose to the
// loader's (B, Tout, nb * Cout), band-major.  A single band is the bank of one: ign_eeg_preprocess_* forward to the same launcher with
// nb = 1 and no quadrature taps, so there is one pass-1 kernel, one transpose and one set of checks.
//
//   x~      the row extended by R = (M-1)/2 samples on each side: zeros, or the reflection about the end samples (numpy 'reflect')
//   a_j[n]  = sum_k H[j][k] * x~[n*q + R - k],  n < Td = ceil(Tin / q)         a centred convolution: no delay
//   f_j     = a_j, or with quadrature taps G  sqrtf(fmaf(a_j, a_j, b_j * b_j)),  b_j the same sum over G[j]
//   out     = (f_j[t] - mean) / (std + eps) over t < Tv = min(Td, Tout), unbiased std in two sweeps; exact zeros elsewhere
//
// In reflect mode the row is filtered as x - x[0]: a constant is a fixed point of reflect-extended filtering up to the factor sum(h)
// and the standardisation removes it, so the value is the same while the fp32 products no longer carry the 1e4 uV offset.  The
// envelope needs that pivot (reflect mode only): it keeps the recording's offset, which the standardisation could not remove from
// under a square root, out of a_j.  With a single tap (R = 0) nothing is extended and no pivot is taken: the pass is then the
// arithmetic of ign_standardise_nct_to_btc, in its order, so taps {1} without cropping give that kernel's output bit for bit (an
// identity spec is the default path).
//
// pass 1, one 256-thread workgroup per (b, c < min(Cin, Cout)) row.  The extended row X[i] = x~[i - R] is staged in LDS once, split by
// phase, Xp[m] = X[m*q + p], so that the decimated convolution becomes q plain correlations (the polyphase form)
//       f[n] = sum_p sum_i h[2R - p - i*q] * Xp[n + i]
// in which every lane reads one phase array at n + const; then every band's taps run over it.  A lane owns EP_J = 5 consecutive
// outputs and walks the sub-taps in blocks of EP_U = 8: 12 LDS values feed 40 fmaf (80 with the quadrature accumulators), and the
// lane stride of 5 dwords is conflict-free on the 32 banks (4 would be 4-way).  The taps are wave-uniform scalar loads.  f stays in
// LDS for the two statistics sweeps, which wave 0 runs in the order of std_rowstats_kernel (lane-strided sums, then the butterfly:
// fixed order, no atomics), and leaves standardised as one coalesced line of the workspace, rows (b, j, c).  The tap walk, the
// statistics and the output line do not depend on nb, so block j of a bank is the one-band result for H[j] bit for bit.
// pass 2, the 64 (t) x 32 (c) LDS transpose of std_apply_transpose_kernel with Tv / Cv as the source extent of every band and
// Tout / nb * Cout as the destination's: padding rows and extra channels are written as zeros, 128-byte writes along c.
//
// LDS of pass 1: q * Lp + Tv floats with Lp = ceil((Tin + 2R) / q) + EP_J - 1  (20 KB at Tin = 2000, M = 1023, q = 1; 17 KB at
// Tin = 1651, M = 1023), whatever nb; rows beyond 64 KB are refused (IGN_E_TOOBIG).  No thread reads outside [0, Tin) of its row: the
// staging loop is the only reader of x and maps every extended index into the row or to a literal zero.
#include "ign_common.h"

namespace {
constexpr int EP_THREADS = 256, EP_J = 5, EP_U = 8;
constexpr size_t EP_LDS_MAX = 64 * 1024;

struct EpPlan {
    int R, Td, Tv, Cv, Lp;
    size_t lds;
};

EpPlan ep_plan(int Cin, int Tin, int M, int q, int Cout, int Tout) {
    EpPlan p;
    p.R = (M - 1) / 2;
    p.Td = (Tin + q - 1) / q;
    p.Tv = p.Td < Tout ? p.Td : Tout;
    p.Cv = Cin < Cout ? Cin : Cout;
    p.Lp = (Tin + 2 * p.R + q - 1) / q + EP_J - 1;
    p.lds = ((size_t)q * p.Lp + (size_t)(p.Tv > 0 ? p.Tv : 0)) * sizeof(float);
    return p;
}

}  // namespace

// The three steps of pass 1 (always inlined: one arithmetic, one order).
// ep_stage_row: the extended row, phase-split: coalesced reads of the row itself, halo indices folded back into [0, Tin) or left
// zero; the tail of every phase array (what the last lane's spare outputs touch) is zero.  The caller's barrier follows.
__device__ __forceinline__ void ep_stage_row(const float* __restrict__ xr, float* xp, int Tin, int R, int next, int q, int Lp,
                                             int reflect, float pivot, int tid) {
    for (int i = tid; i < next; i += EP_THREADS) {
        int src = i - R;
        float v = 0.f;
        if (reflect) {
            if (src < 0) src = -src;                   // R <= Tin - 1: one fold is enough on either side
            if (src >= Tin) src = 2 * (Tin - 1) - src;
            v = xr[src] - pivot;
        } else if (src >= 0 && src < Tin) {
            v = xr[src];
        }
        const int m = i / q;
        xp[(i - m * q) * Lp + m] = v;
    }
    for (int s = tid; s < q * Lp; s += EP_THREADS) {
        const int p = s / Lp, m = s - p * Lp;
        if (m * q + p >= next) xp[s] = 0.f;
    }
}

// ep_filter_row: f[0..Tv-1] of one tap set into fs, EP_J outputs per lane, sub-taps in blocks of EP_U.  With QUAD a second
// accumulator set runs the quadrature taps hq over the same LDS values and fs gets sqrtf(fmaf(a, a, b * b)).  Reads xp, writes fs.
template <bool QUAD>
__device__ __forceinline__ void ep_filter_row(const float* xp, float* fs, const float* __restrict__ h, const float* __restrict__ hq,
                                              int q, int R2, int Lp, int Tv, int tid) {
    const int wave0 = __builtin_amdgcn_readfirstlane(tid & ~63);
    for (int base = 0; base < Tv; base += EP_THREADS * EP_J) {
        if (base + wave0 * EP_J >= Tv) continue;       // a wave without outputs in this sweep (wave-uniform)
        const int n0 = base + tid * EP_J;
        const int nr = n0 < Tv ? n0 : 0;               // spare lanes recompute the first outputs and store nothing
        float acc[EP_J], bcc[EP_J];
#pragma unroll
        for (int j = 0; j < EP_J; ++j) acc[j] = bcc[j] = 0.f;
        for (int p = 0; p < q && p <= R2; ++p) {
            const float* xq = xp + p * Lp + nr;
            const float* g = h + (R2 - p);             // sub-tap i of phase p is g[-i * q]
            const float* gq = QUAD ? hq + (R2 - p) : nullptr;
            const int np = (R2 - p) / q + 1;
            int i0 = 0;
            for (; i0 + EP_U <= np; i0 += EP_U) {
                float v[EP_U + EP_J - 1];
#pragma unroll
                for (int u = 0; u < EP_U + EP_J - 1; ++u) v[u] = xq[i0 + u];
#pragma unroll
                for (int u = 0; u < EP_U; ++u) {
                    const float hv = g[-(i0 + u) * q];
#pragma unroll
                    for (int j = 0; j < EP_J; ++j) acc[j] = fmaf(hv, v[u + j], acc[j]);
                    if (QUAD) {
                        const float qv = gq[-(i0 + u) * q];
#pragma unroll
                        for (int j = 0; j < EP_J; ++j) bcc[j] = fmaf(qv, v[u + j], bcc[j]);
                    }
                }
            }
            for (; i0 < np; ++i0) {
                const float hv = g[-i0 * q];
#pragma unroll
                for (int j = 0; j < EP_J; ++j) acc[j] = fmaf(hv, xq[i0 + j], acc[j]);
                if (QUAD) {
                    const float qv = gq[-i0 * q];
#pragma unroll
                    for (int j = 0; j < EP_J; ++j) bcc[j] = fmaf(qv, xq[i0 + j], bcc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < EP_J; ++j)
            if (n0 + j < Tv) fs[n0 + j] = QUAD ? sqrtf(fmaf(acc[j], acc[j], bcc[j] * bcc[j])) : acc[j];
    }
}

// ep_row_stats: mean and unbiased standard deviation in two sweeps over LDS (no E[x^2] - E[x]^2), by wave 0 in
// std_rowstats_kernel's order; stat = {mean, 1 / (std + eps)}.  Between the caller's two barriers.
__device__ __forceinline__ void ep_row_stats(const float* fs, float* stat, int Tv, float eps, int tid) {
    if (tid < 64) {
        float s = 0.f;
        for (int t = tid; t < Tv; t += 64) s += fs[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mu = s / (float)Tv;
        float v = 0.f;
        for (int t = tid; t < Tv; t += 64) {
            const float dv = fs[t] - mu;
            v = fmaf(dv, dv, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (tid == 0) {
            stat[0] = mu;
            stat[1] = 1.f / (sqrtf(v / (float)(Tv - 1)) + eps);                        // ddof = 1, eps outside the sqrt
        }
    }
}

// Pass 1: the row is staged once, then every band's taps run over it.  Three barriers per band:
//   A  after the tap walk: fs of band j is complete before wave 0 sums it;
//   B  after the statistics: stat of band j is visible before the line is written out;
//   C  at the head of band j + 1: every thread has read fs of band j (its part of the output line) before any lane overwrites it
//      with band j + 1.  stat needs no barrier of its own: wave 0 writes band j + 1's after A of that band, which every thread
//      reaches only after it has read band j's.  xp is read-only after the staging barrier.
// Rows of the workspace are (b, j, c): band-major inside a sample, as the output's channels are.
// At most 80 scalar registers: a CU then holds 8 of these workgroups; left alone the band loop takes 91 and the CU holds 7.
template <bool QUAD>
__global__ void __launch_bounds__(EP_THREADS) __attribute__((amdgpu_num_sgpr(80)))
eeg_filterbank_kernel(const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ hq, float* __restrict__ ws,
                      int Cin, int Tin, int M, int nb, int q, int reflect, int Cv, int Tv, int Lp, float eps) {
    extern __shared__ __attribute__((aligned(16))) float ep_lds[];
    __shared__ float stat[2];
    float* xp = ep_lds;
    float* fs = ep_lds + (size_t)q * Lp;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / Cv, c = blockIdx.x - b * Cv;
    const float* xr = x + ((size_t)b * Cin + c) * Tin;
    const int R2 = M - 1, R = R2 >> 1, next = Tin + R2;
    const float pivot = (reflect && R > 0) ? xr[0] : 0.f;

    ep_stage_row(xr, xp, Tin, R, next, q, Lp, reflect, pivot, tid);
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        if (j > 0) __syncthreads();                                                    // C
        ep_filter_row<QUAD>(xp, fs, h + (size_t)j * M, QUAD ? hq + (size_t)j * M : nullptr, q, R2, Lp, Tv, tid);
        __syncthreads();                                                               // A
        ep_row_stats(fs, stat, Tv, eps, tid);
        __syncthreads();                                                               // B
        const float mean = stat[0], rstd = stat[1];
        float* wr = ws + (((size_t)b * nb + j) * Cv + c) * Tv;
        for (int t = tid; t < Tv; t += EP_THREADS) wr[t] = (fs[t] - mean) * rstd;
    }
}

// ws (B, nb, Cv, Tv) -> out (B, Tout, nb * Cout), band-major: destination channel cd = j * Cout + c; a 32-channel tile may
// straddle band blocks, so a wave finds the pair (j, c) of the first of its eight channels (at most nb - 1 <= 7 subtractions: cheaper
// than an integer division, and none at nb = 1) and steps it along them.  The pair is wave-uniform: the source row's address stays in
// scalar registers.
__global__ void __launch_bounds__(256) eeg_bank_transpose_kernel(const float* __restrict__ ws, float* __restrict__ out, int nb, int Cv,
                                                                 int Tv, int Cout, int Tout) {
    __shared__ float tile[32][65];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Ctot = nb * Cout, t = t0 + lane;
    int j = 0, c = c0 + w * 8;
    while (c >= Cout && j + 1 < nb) {                  // beyond the last band (a tile's tail) c stays >= Cout >= Cv: zeros
        c -= Cout;
        ++j;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int cc = w * 8 + i;
        tile[cc][lane] = (c0 + cc < Ctot && c < Cv && t < Tv) ? ws[(((size_t)b * nb + j) * Cv + c) * Tv + t] : 0.f;
        if (++c == Cout) {                             // valid for any Cout >= 1: checked at every step
            c = 0;
            ++j;
        }
    }
    __syncthreads();
    const int cc = threadIdx.x & 31, tr = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int tl = tr * 8 + i, t = t0 + tl, cd = c0 + cc;
        if (t < Tout && cd < Ctot) out[((size_t)b * Tout + t) * Ctot + cd] = tile[cc][tl];
    }
}

// The shape checks that the workspace size and the launch share, in the order the refusal tables of the tests fix.
static bool ep_check(const char* who, int B, int Cin, int Tin, int M, int nb, int q, int Cout, int Tout) {
    if (nb < 1 || nb > IGN_EEG_MAX_BANDS) {
        ign_set_error("%s: nb=%d bands outside 1..%d", who, nb, IGN_EEG_MAX_BANDS);
        return false;
    }
    if (B <= 0 || Cin <= 0 || Tin <= 0 || Cout <= 0 || Tout <= 0) {
        ign_set_error("%s: non-positive dimension (B=%d Cin=%d Tin=%d Cout=%d Tout=%d)", who, B, Cin, Tin, Cout, Tout);
        return false;
    }
    if (M < 1 || (M & 1) == 0 || M > IGN_EEG_MAX_TAPS) {
        ign_set_error("%s: M=%d taps; the centred filter needs an odd count in 1..%d", who, M, IGN_EEG_MAX_TAPS);
        return false;
    }
    if (q < 1 || q > IGN_EEG_MAX_DECIMATE) {
        ign_set_error("%s: decimation factor q=%d outside 1..%d", who, q, IGN_EEG_MAX_DECIMATE);
        return false;
    }
    return true;
}

static size_t ep_ws_bytes(const char* who, int B, int Cin, int Tin, int M, int nb, int q, int Cout, int Tout) {
    if (!ep_check(who, B, Cin, Tin, M, nb, q, Cout, Tout)) return 0;
    const EpPlan p = ep_plan(Cin, Tin, M, q, Cout, Tout);
    return (size_t)B * nb * p.Cv * p.Tv * sizeof(float);
}

// Every check and both launches; `who` names the entry point in the error texts, `label` the timer's row.
static int ep_launch(const char* who, const char* label, const float* x, const float* taps, const float* quad, float* out, float* ws,
                     int B, int Cin, int Tin, int M, int nb, int q, int edge, int Cout, int Tout, float eps, void* stream) {
    if (!x || !taps || !out || !ws) {
        ign_set_error("%s: null pointer", who);
        return IGN_E_ARG;
    }
    if (!ep_check(who, B, Cin, Tin, M, nb, q, Cout, Tout)) return IGN_E_ARG;
    if (edge != IGN_EDGE_REFLECT && edge != IGN_EDGE_ZERO) {
        ign_set_error("%s: edge=%d is neither IGN_EDGE_REFLECT nor IGN_EDGE_ZERO", who, edge);
        return IGN_E_ARG;
    }
    if (edge == IGN_EDGE_REFLECT && (M - 1) / 2 >= Tin) {
        ign_set_error("%s: reflect extension by R=%d needs a row of at least R+1 samples, Tin=%d", who, (M - 1) / 2, Tin);
        return IGN_E_ARG;
    }
    if (quad && edge == IGN_EDGE_ZERO) {
        ign_set_error("%s: quadrature taps (envelope) with IGN_EDGE_ZERO: without the reflect pivot the recording's offset enters "
                      "the square root", who);
        return IGN_E_ARG;
    }
    if (quad && M == 1) {
        ign_set_error("%s: quadrature taps (envelope) with M=1: a single tap has no quadrature pair", who);
        return IGN_E_ARG;
    }
    const EpPlan p = ep_plan(Cin, Tin, M, q, Cout, Tout);
    if (p.Tv < 2) {
        ign_set_error("%s: Tv = min(ceil(Tin/q), Tout) = %d; the unbiased std needs Tv >= 2 (Tin=%d q=%d Tout=%d)", who, p.Tv, Tin, q,
                      Tout);
        return IGN_E_ARG;
    }
    if (p.lds > EP_LDS_MAX) {
        ign_set_error("%s: a row of Tin=%d with M=%d taps needs %zu bytes of LDS, more than %zu", who, Tin, M, p.lds, EP_LDS_MAX);
        return IGN_E_TOOBIG;
    }
    if (B > 65535 || (long long)B * p.Cv > 0x7fffffffLL) {
        ign_set_error("%s: B=%d exceeds the launch grid (65535 samples per call)", who, B);
        return IGN_E_TOOBIG;
    }
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm(label, s);
    const auto pass1 = quad ? eeg_filterbank_kernel<true> : eeg_filterbank_kernel<false>;
    hipLaunchKernelGGL(pass1, dim3((unsigned)(B * p.Cv)), dim3(EP_THREADS), p.lds, s, x, taps, quad, ws, Cin, Tin, M, nb, q,
                       edge == IGN_EDGE_REFLECT ? 1 : 0, p.Cv, p.Tv, p.Lp, eps);
    int rc;
    if ((rc = ign_check_launch("eeg_filterbank_kernel"))) return rc;
    hipLaunchKernelGGL(eeg_bank_transpose_kernel, dim3((Tout + 63) / 64, (nb * Cout + 31) / 32, B), dim3(256), 0, s, ws, out, nb, p.Cv,
                       p.Tv, Cout, Tout);
    return ign_check_launch("eeg_bank_transpose_kernel");
}

extern "C" size_t ign_eeg_preprocess_ws_bytes(int B, int Cin, int Tin, int M, int q, int Cout, int Tout) {
    return ep_ws_bytes("ign_eeg_preprocess_ws_bytes", B, Cin, Tin, M, 1, q, Cout, Tout);
}

extern "C" int ign_eeg_preprocess_nct_to_btc(const float* x_nct, const float* taps, float* out_btc, float* ws, int B, int Cin, int Tin,
                                             int M, int q, int edge, int Cout, int Tout, float eps, void* stream) {
    return ep_launch("ign_eeg_preprocess_nct_to_btc", "eeg_preprocess", x_nct, taps, nullptr, out_btc, ws, B, Cin, Tin, M, 1, q, edge,
                     Cout, Tout, eps, stream);
}

extern "C" size_t ign_eeg_filterbank_ws_bytes(int B, int Cin, int Tin, int M, int nb, int q, int Cout, int Tout) {
    return ep_ws_bytes("ign_eeg_filterbank_ws_bytes", B, Cin, Tin, M, nb, q, Cout, Tout);
}

extern "C" int ign_eeg_filterbank_nct_to_btc(const float* x_nct, const float* taps, const float* quad, float* out_btc, float* ws,
                                             int B, int Cin, int Tin, int M, int nb, int q, int edge, int Cout, int Tout, float eps,
                                             void* stream) {
    return ep_launch("ign_eeg_filterbank_nct_to_btc", "eeg_filterbank", x_nct, taps, quad, out_btc, ws, B, Cin, Tin, M, nb, q, edge,
                     Cout, Tout, eps, stream);
}
