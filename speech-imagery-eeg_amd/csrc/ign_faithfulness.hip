// Faithfulness curves (utils/faithfulness.py, run.py --faithfulness): rank the (time, electrode) cells of every sample by a score map
// and replace the top k of them by a baseline.  Two passes, both exact and bitwise defined; the rule is utils/faithfulness.py
// (rank_rule, perturb_rule), which the kernels equal bit for bit.
//
//   key(v)   = the artifact stage's order-preserving uint32 of a float (art_key, csrc/ign_eeg_artifact.hip), restated below;
//   order    : element i precedes i' iff key_i > key_i', or the keys are equal and i < i';
//   threshold: (key, flat index) of the k-th element in that order; k = 0 gives (0xffffffff, -1);
//   selected : i < n_b and (key_i > thr_key or (key_i == thr_key and i <= thr_idx)) -- elementwise, no scan in the apply pass.
//
// rank_threshold_kernel: one workgroup per sample, all nk thresholds in one launch.  The order above is the descending order of the
// composite word  w_i = key_i << ibits | (~i & (2^ibits - 1)),  ibits = the bit length of n - 1 rounded up to whole bytes: the
// composites of a sample are distinct, so its k-th largest names one element.  An 8-bit radix select finds it, most significant byte
// first: a pass histograms the byte of every element that still matches the bytes chosen so far, a wave per requested k then scans
// its 256 counters from the top, picks the byte that holds rank r and lowers r by what lies above it.  The first pass has one
// histogram (every k starts from the empty prefix), the later ones one per k: RT_MAX_K * 256 integer counters in LDS.  The four key
// passes are followed by ibits / 8 passes over the index bits, which is where tied keys are cut at the lowest indices.  Integer LDS
// atomics only, so the counts -- and the result -- do not depend on the order of arrival; no workspace; a sample never reads another
// sample's data.  Lanes of a wave that add to the same counter (a constant map, the leading byte of similar floats) are counted with
// one ballot and one atomic.  Every __syncthreads() sits in block-uniform control flow: n, npass and nk are the same in every thread.
//
// perturb_kernel: ign_mix_btc's layout -- a block owns PT_CHUNK consecutive flat (t, c) indices of one sample, a lane a quad through a
// 4-byte-aligned 16-byte vector type; one read of x and of the score, one write of out.
#include <cstdint>
#include "ign_common.h"

constexpr int RT_THREADS = 1024;
constexpr int RT_WAVES = RT_THREADS / IGN_WAVE;
constexpr int RT_UNROLL = 4;                                   // elements per thread and trip
constexpr int RT_TRIP = RT_THREADS * RT_UNROLL;                // elements per trip of the block
constexpr int RT_MAX_K = IGN_RANK_MAX_K;
constexpr int RT_BINS = 256;

__device__ __forceinline__ unsigned faith_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// add 1 to hist[bin] for every lane with `on`; the lanes of a wave that share one bin cost one atomic
__device__ __forceinline__ void rt_count(int* hist, bool on, int bin) {
    const unsigned long long m = __ballot(on);
    if (m == 0ull) return;                                      // wave-uniform
    const int first = __shfl(bin, __ffsll((long long)m) - 1, IGN_WAVE);
    const unsigned long long same = __ballot(on && bin == first);
    if (same == m) {                                            // wave-uniform
        if ((int)(threadIdx.x & (IGN_WAVE - 1)) == __ffsll((long long)m) - 1) atomicAdd(&hist[first], __popcll(m));
    } else if (on) {
        atomicAdd(&hist[bin], 1);
    }
}

// the byte that holds rank r (1-based, from the top) of one 256-counter histogram, found by a whole wave: -> the byte in every lane,
// r lowered by the count above it.  1 <= r <= the histogram's total.
__device__ __forceinline__ int rt_pick(const int* hist, int& r) {
    const int lane = threadIdx.x & (IGN_WAVE - 1);
    const int top = RT_BINS - 1 - 4 * lane;                     // this lane's bins: top, top - 1, top - 2, top - 3
    const int c0 = hist[top], c1 = hist[top - 1], c2 = hist[top - 2], c3 = hist[top - 3];
    const int s = c0 + c1 + c2 + c3;
    int incl = s;
#pragma unroll
    for (int o = 1; o < IGN_WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o, IGN_WAVE);
        if (lane >= o) incl += up;
    }
    const int excl = incl - s;
    const bool mine = excl < r && r <= incl;                    // exactly one lane
    int digit = 0, above = 0;
    if (mine) {
        const int q = r - excl;                                 // 1 .. s
        if (q <= c0) { digit = top; above = excl; }
        else if (q <= c0 + c1) { digit = top - 1; above = excl + c0; }
        else if (q <= c0 + c1 + c2) { digit = top - 2; above = excl + c0 + c1; }
        else { digit = top - 3; above = excl + c0 + c1 + c2; }
    }
    const int src = __ffsll((long long)__ballot(mine)) - 1;
    digit = __shfl(digit, src, IGN_WAVE);
    above = __shfl(above, src, IGN_WAVE);
    r -= above;
    return digit;
}

__global__ void __launch_bounds__(RT_THREADS) rank_threshold_kernel(const float* __restrict__ score, const int32_t* __restrict__ k_bj,
                                                                    const int32_t* __restrict__ len_b, int32_t* __restrict__ thr_key,
                                                                    int32_t* __restrict__ thr_idx, int T, int Cs, int nk) {
    __shared__ int s_hist[RT_MAX_K * RT_BINS];
    __shared__ unsigned long long s_prefix[RT_MAX_K];           // the bytes chosen so far, right-aligned
    __shared__ int s_r[RT_MAX_K];                               // rank left inside the prefix; 0: k = 0, nothing to find
    const int tid = threadIdx.x, lane = tid & (IGN_WAVE - 1), wave = tid / IGN_WAVE;
    const int b = blockIdx.x;
    const int len = len_b ? min(max(len_b[b], 0), T) : T;       // device data: clamped, never trusted as an index bound
    const int n = len * Cs;                                     // < 2^31, checked on the host
    const float* sb = score + (size_t)b * T * Cs;
    const int nbits = n > 1 ? 32 - __clz(n - 1) : 0;
    const int ibits = (nbits + 7) & ~7;                         // 0, 8, 16, 24 or 32
    const unsigned long long imask = (1ull << ibits) - 1ull;
    const int npass = 4 + ibits / 8;
    if (tid < nk) {
        s_r[tid] = min(max(k_bj[(size_t)b * nk + tid], 0), n);
        s_prefix[tid] = 0ull;
    }
    for (int pass = 0; pass < npass; ++pass) {                  // block-uniform trip count
        const int shift = 8 * (npass - 1 - pass);               // the byte this pass decides
        const int nh = pass == 0 ? 1 : nk;
        for (int i = tid; i < nh * RT_BINS; i += RT_THREADS) s_hist[i] = 0;
        __syncthreads();                                        // counters cleared; s_r / s_prefix of the pass before in place
        for (int base = 0; base < n; base += RT_TRIP) {
            unsigned long long w[RT_UNROLL];
            bool in[RT_UNROLL];
#pragma unroll
            for (int u = 0; u < RT_UNROLL; ++u) {
                const int i = base + u * RT_THREADS + tid;      // base + 4095 at most: no overflow below 2^31 - 4096 (host check)
                in[u] = i < n;
                const float v = in[u] ? sb[i] : 0.0f;
                w[u] = ((unsigned long long)faith_key(v) << ibits) | (~(unsigned long long)(unsigned)i & imask);
            }
            if (pass == 0) {
#pragma unroll
                for (int u = 0; u < RT_UNROLL; ++u) rt_count(s_hist, in[u], (int)(w[u] >> shift) & 0xff);
            } else {
                for (int j = 0; j < nk; ++j) {                  // block-uniform
                    const int r = s_r[j];
                    if (r == 0) continue;                       // block-uniform: k = 0
                    const unsigned long long pre = s_prefix[j];
#pragma unroll
                    for (int u = 0; u < RT_UNROLL; ++u)
                        rt_count(s_hist + j * RT_BINS, in[u] && (w[u] >> (shift + 8)) == pre, (int)(w[u] >> shift) & 0xff);
                }
            }
        }
        __syncthreads();                                        // the counts are complete
        for (int j = wave; j < nk; j += RT_WAVES) {             // a wave per k, no barrier inside
            int r = s_r[j];
            if (r == 0) continue;                               // wave-uniform
            const int digit = rt_pick(s_hist + (pass == 0 ? 0 : j * RT_BINS), r);
            if (lane == 0) {
                s_prefix[j] = (s_prefix[j] << 8) | (unsigned long long)digit;
                s_r[j] = r;                                     // >= 1: the rank inside the longer prefix
            }
        }
        __syncthreads();                                        // before the counters are cleared and the prefixes read again
    }
    if (tid < nk) {
        const bool none = s_r[tid] == 0;
        const unsigned long long w = s_prefix[tid];
        thr_key[(size_t)b * nk + tid] = none ? (int32_t)0xffffffffu : (int32_t)(unsigned)(w >> ibits);
        thr_idx[(size_t)b * nk + tid] = none ? -1 : (int32_t)(~w & imask);
    }
}

extern "C" int ign_rank_threshold(const float* score_bts, const int32_t* k_bj, const int32_t* len_b, int32_t* thr_key_bj,
                                  int32_t* thr_idx_bj, int B, int T, int Cs, int nk, void* stream) {
    static const char* who = "ign_rank_threshold";
    if (!score_bts || !k_bj || !thr_key_bj || !thr_idx_bj || B < 1 || T < 1 || Cs < 1) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d T=%d Cs=%d)", who, B, T, Cs);
        return IGN_E_ARG;
    }
    if (nk < 1 || nk > RT_MAX_K) {
        ign_set_error("%s: nk=%d outside 1..%d (IGN_RANK_MAX_K)", who, nk, RT_MAX_K);
        return IGN_E_ARG;
    }
    if ((long long)T * Cs > 0x7fff0000LL) {
        ign_set_error("%s: T*Cs=%lld does not fit a 32-bit index", who, (long long)T * Cs);
        return IGN_E_TOOBIG;
    }
    {
        IgnScopedTimer tm("rank_threshold", (hipStream_t)stream);
        hipLaunchKernelGGL(rank_threshold_kernel, dim3((unsigned)B), dim3(RT_THREADS), 0, (hipStream_t)stream, score_bts, k_bj, len_b,
                           thr_key_bj, thr_idx_bj, T, Cs, nk);
    }
    return ign_check_launch("rank_threshold_kernel");
}

// ---------------------------------------------------------------- the perturbation
constexpr int PT_THREADS = 256;
constexpr int PT_QUADS = 4;                                    // quads per lane
constexpr int PT_CHUNK = PT_THREADS * PT_QUADS * 4;            // flat indices per block

struct __attribute__((packed, aligned(4))) PtQuad { unsigned v[4]; };

struct PtArgs {
    const unsigned* x;        // (B,T,C), as bits
    const float* score;       // (B,T,Cs)
    const int32_t* thr_key;   // (B,nk)
    const int32_t* thr_idx;   // (B,nk)
    const unsigned* fill;     // (B,C) as bits, or null: 0.0f
    const int32_t* len;       // (B) or null
    unsigned* out;
    int j, nk, insert, T, C, nchunk;
};

__device__ __forceinline__ bool pt_selected(float s, int i, unsigned tkey, int tidx) {
    const unsigned key = faith_key(s);
    return key > tkey || (key == tkey && i <= tidx);
}

// PER_CELL: Cs == C, the score of flat index e is score[e]; else Cs == 1, the score of time step e / C
template <bool PER_CELL>
__global__ void __launch_bounds__(PT_THREADS) perturb_kernel(const PtArgs a) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.nchunk;
    const int chunk = blockIdx.x - b * a.nchunk;
    const int C = a.C, TC = a.T * C;
    const int len = a.len ? min(max(a.len[b], 0), a.T) : a.T;   // device data: clamped, never trusted as an index bound
    const int n = len * C;                                       // flat indices of data; padding from there to TC
    const unsigned tkey = (unsigned)a.thr_key[(size_t)b * a.nk + a.j];
    const int tidx = a.thr_idx[(size_t)b * a.nk + a.j];
    const bool insert = a.insert != 0;
    const unsigned* xb = a.x + (size_t)b * TC;
    const float* sb = a.score + (size_t)b * (PER_CELL ? TC : a.T);
    const unsigned* fb = a.fill ? a.fill + (size_t)b * C : nullptr;
    unsigned* ob = a.out + (size_t)b * TC;
#pragma unroll
    for (int u = 0; u < PT_QUADS; ++u) {
        const int e0 = chunk * PT_CHUNK + (u * PT_THREADS + tid) * 4;
        if (e0 >= TC) break;                                     // e0 grows with u
        const int cnt = min(4, TC - e0);
        if (e0 >= n) {                                           // padding: copied through
            if (cnt == 4) *reinterpret_cast<PtQuad*>(ob + e0) = *reinterpret_cast<const PtQuad*>(xb + e0);
            else for (int k = 0; k < cnt; ++k) ob[e0 + k] = xb[e0 + k];
            continue;
        }
        int t = e0 / C, c = e0 - t * C;
        PtQuad q, o;
        float s[4];
        if (cnt == 4) {
            q = *reinterpret_cast<const PtQuad*>(xb + e0);
            if (PER_CELL) {
                const PtQuad sq = *reinterpret_cast<const PtQuad*>(sb + e0);
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = __uint_as_float(sq.v[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                q.v[k] = k < cnt ? xb[e0 + k] : 0u;
                if (PER_CELL) s[k] = k < cnt ? sb[e0 + k] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = e0 + k;
            unsigned v = q.v[k];
            if (e < n) {                                         // e < n <= TC: inside the sample's data
                const int i = PER_CELL ? e : t;
                const float sv = PER_CELL ? s[k] : sb[t];
                if (pt_selected(sv, i, tkey, tidx) != insert) v = fb ? fb[c] : 0u;
            }
            o.v[k] = v;
            if (++c == C) { c = 0; ++t; }
        }
        if (cnt == 4) {
            *reinterpret_cast<PtQuad*>(ob + e0) = o;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) ob[e0 + k] = o.v[k];
        }
    }
}

extern "C" int ign_perturb_btc(const float* x_btc, const float* score_bts, const int32_t* thr_key_bj, const int32_t* thr_idx_bj, int j,
                               int nk, const float* fill_bc, const int32_t* len_b, float* out_btc, int insert, int B, int T, int C,
                               int Cs, void* stream) {
    static const char* who = "ign_perturb_btc";
    if (!x_btc || !score_bts || !thr_key_bj || !thr_idx_bj || !out_btc || B < 1 || T < 1 || C < 1 || Cs < 1) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d T=%d C=%d Cs=%d)", who, B, T, C, Cs);
        return IGN_E_ARG;
    }
    if (Cs != 1 && Cs != C) {
        ign_set_error("%s: Cs=%d must be 1 (a score per time step) or C=%d (a score per cell)", who, Cs, C);
        return IGN_E_ARG;
    }
    if (nk < 1 || nk > RT_MAX_K) {
        ign_set_error("%s: nk=%d outside 1..%d (IGN_RANK_MAX_K)", who, nk, RT_MAX_K);
        return IGN_E_ARG;
    }
    if (j < 0 || j >= nk) {
        ign_set_error("%s: j=%d outside [0, nk) with nk=%d", who, j, nk);
        return IGN_E_ARG;
    }
    const long long TC = (long long)T * C;
    if (TC > 0x7fff0000LL) {
        ign_set_error("%s: T*C=%lld does not fit a 32-bit index", who, TC);
        return IGN_E_TOOBIG;
    }
    const long long nchunk = (TC + PT_CHUNK - 1) / PT_CHUNK;
    if ((long long)B * nchunk > 0x7fffffffLL) {
        ign_set_error("%s: B=%d T=%d C=%d needs more blocks than a grid has", who, B, T, C);
        return IGN_E_TOOBIG;
    }
    const uintptr_t xa = (uintptr_t)x_btc, oa = (uintptr_t)out_btc, bytes = (uintptr_t)B * (uintptr_t)TC * sizeof(float);
    if ((xa <= oa ? oa - xa : xa - oa) < bytes) {
        ign_set_error("%s: out of place only (the curve perturbs the same batch once per fraction): x and out overlap", who);
        return IGN_E_ARG;
    }
    PtArgs a;
    a.x = reinterpret_cast<const unsigned*>(x_btc); a.score = score_bts; a.thr_key = thr_key_bj; a.thr_idx = thr_idx_bj;
    a.fill = reinterpret_cast<const unsigned*>(fill_bc); a.len = len_b; a.out = reinterpret_cast<unsigned*>(out_btc);
    a.j = j; a.nk = nk; a.insert = insert; a.T = T; a.C = C; a.nchunk = (int)nchunk;
    {
        IgnScopedTimer tm("perturb", (hipStream_t)stream);
        const dim3 grid((unsigned)(B * nchunk)), block(PT_THREADS);
        if (Cs == C) hipLaunchKernelGGL(perturb_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(perturb_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    }
    return ign_check_launch("perturb_kernel");
}
