// Artifact stage in front of the spatial filter (run.py --eeg_artifact; ops.eeg_artifact; the rule is stated once in numpy in
// utils/eeg_artifact.py:artifact_numpy): robust row statistics, a verdict per electrode, a clamp of the good rows and the repair of
// the bad ones from the good ones, on the raw (B, C, T) batch.
//
//   m_c = med(x[c]);  s_c = med(|x[c] - m_c|)            med = the LOWER median, the element of rank (n-1)/2; a row with a non-finite
//                                                        sample has no statistics: flag 3, (0, 0)
//   ref = med(s_c over the finite rows);  flat: s_c <= fl(F ref);  noisy: s_c > fl(N ref);  no good row left: every bad one is 4
//   good rows:  r = fl(fl(K 1.4826f) s_c);  y = x < fl(m_c - r) ? fl(m_c - r) : x > fl(m_c + r) ? fl(m_c + r) : x
//   bad row c:  y[c,t] = (sum_j w[c,j] fl(y[j,t] - m_j)) / (sum_j w[c,j]),  j over the good rows, ascending, one fmaf chain
//
// The median is a SELECT, not a sort: floats map to unsigned keys of the same order, and the key of rank k is the largest v with
// #{key < v} <= k, built from the top bit down -- 32 counting passes over the row, each pass one compare per element, a ballot
// and a scalar population count per 64 elements.  The result is an element of the row, whatever the ties; no data movement, no
// atomics.  Rows of up to ART_WAVE_ROW = 2048 samples (CHISCO's 1651) are held in registers, one WAVE per row and four rows per
// workgroup: up to 32 keys per lane, padded with the largest key, the count of a pass lives in a scalar register and nothing
// meets at a barrier.  Longer rows, up to the limit, are staged in LDS, one workgroup per row, with one barrier per pass for the
// four waves' counts (two alternating slots).  For the two medians of a row that is 64 compares per element; a 2048-wide
// bitonic network reads and writes every element 132 times.
//
// Three launches per batch: the statistics (one workgroup per row), the verdicts (one workgroup per sample; the same select over
// at most 1024 scales) and the apply pass over tiles of (all C, TS samples): the clamped good rows of a tile go to `out` and,
// centred, through LDS, where every repaired electrode of the tile reads them.  No workspace beyond stats / flags, a fixed order
// everywhere: two calls give the same bits, a sample's output depends on that sample alone.
#include "ign_common.h"

namespace {

constexpr int ART_THREADS = 256;
constexpr int ART_WAVES = ART_THREADS / IGN_WAVE;
constexpr int ART_WAVE_ROW = 2048;                                      // rows up to here are held in registers, one wave per row
constexpr int ART_RED = 2 * ART_WAVES;                                  // ints behind the keys: the waves' counts, two slots
constexpr float ART_MAD_TO_SIGMA = 1.4826f;

// float -> unsigned of the same order (-0 sorts below +0; the callers take the sign of a zero median away)
__device__ __forceinline__ unsigned art_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float art_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the key of rank k (0-based) among keys[0..n): the largest v with #{key < v} <= k.  Every thread of the block calls it and gets the
// same value; `keys` is complete before the call (a barrier behind its last write) and is only read.
__device__ unsigned art_select(const unsigned* keys, int n, int k, int* red) {
    const int lane = threadIdx.x & (IGN_WAVE - 1), wave = threadIdx.x / IGN_WAVE;
    unsigned v = 0;
    for (int b = 31; b >= 0; --b) {
        const unsigned cand = v | (1u << b);
        int cnt = 0;
        for (int base = wave * IGN_WAVE; base < n; base += ART_THREADS) {         // a wave-uniform trip count
            const int i = base + lane;
            const bool lt = i < n && keys[i] < cand;
            cnt += __popcll(__ballot(lt));
        }
        int* r = red + (b & 1) * ART_WAVES;
        if (lane == 0) r[wave] = cnt;
        __syncthreads();
        if (r[0] + r[1] + r[2] + r[3] <= k) v = cand;
    }
    return v;
}

// rows of at most 64 * NPL samples: one wave per row, the keys in registers (index j * 64 + lane), pads = the largest key
template <int NPL>
__device__ __forceinline__ unsigned art_select_reg(const unsigned (&key)[NPL], int k) {
    unsigned v = 0;
    for (int b = 31; b >= 0; --b) {
        const unsigned cand = v | (1u << b);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < NPL; ++j) cnt += __popcll(__ballot(key[j] < cand));
        if (cnt <= k) v = cand;
    }
    return v;
}

template <int NPL>
__global__ __launch_bounds__(ART_THREADS) void eeg_artifact_stats_wave_kernel(const float* __restrict__ x, float* __restrict__ stats,
                                                                              unsigned char* __restrict__ flags, int T, long long rows) {
    const int lane = threadIdx.x & (IGN_WAVE - 1);
    const long long row = (long long)blockIdx.x * ART_WAVES + threadIdx.x / IGN_WAVE;
    if (row >= rows) return;                           // a whole wave leaves; there is no barrier in this kernel
    const float* xr = x + (size_t)row * T;
    unsigned key[NPL];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int i = j * IGN_WAVE + lane;
        const float v = i < T ? xr[i] : 0.0f;
        bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
        key[j] = i < T ? art_key(v) : 0xffffffffu;     // the key of no finite float
    }
    if (__ballot(bad) != 0ull) {
        if (lane == 0) {
            stats[2 * row] = 0.0f;
            stats[2 * row + 1] = 0.0f;
            flags[row] = 3;
        }
        return;
    }
    const int k = (T - 1) / 2;
    const float m = __fadd_rn(art_unkey(art_select_reg<NPL>(key, k)), 0.0f);      // -0 -> +0
#pragma unroll
    for (int j = 0; j < NPL; ++j)
        if (j * IGN_WAVE + lane < T) key[j] = __float_as_uint(fabsf(__fsub_rn(art_unkey(key[j]), m)));   // >= 0: in order as they are
    const float s = __uint_as_float(art_select_reg<NPL>(key, k));
    if (lane == 0) {
        stats[2 * row] = m;
        stats[2 * row + 1] = s;
        flags[row] = 0;
    }
}

template <int NPL>
void art_launch_wave(const float* x, float* stats, unsigned char* flags, int T, long long rows, hipStream_t s) {
    const unsigned grid = (unsigned)((rows + ART_WAVES - 1) / ART_WAVES);
    hipLaunchKernelGGL(eeg_artifact_stats_wave_kernel<NPL>, dim3(grid), dim3(ART_THREADS), 0, s, x, stats, flags, T, rows);
}

__global__ __launch_bounds__(ART_THREADS) void eeg_artifact_stats_kernel(const float* __restrict__ x, float* __restrict__ stats,
                                                                         unsigned char* __restrict__ flags, int T) {
    extern __shared__ unsigned art_lds[];
    unsigned* keys = art_lds;                          // T keys
    int* red = (int*)(art_lds + T);                    // ART_RED ints
    const size_t row = blockIdx.x;
    const float* xr = x + row * (size_t)T;
    int bad = 0;
    for (int i = threadIdx.x; i < T; i += ART_THREADS) {
        const float v = xr[i];
        bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
        keys[i] = art_key(v);
    }
    if (__syncthreads_or(bad)) {                       // the same answer in every thread
        if (threadIdx.x == 0) {
            stats[2 * row] = 0.0f;
            stats[2 * row + 1] = 0.0f;
            flags[row] = 3;
        }
        return;
    }
    const int k = (T - 1) / 2;
    const float m = __fadd_rn(art_unkey(art_select(keys, T, k, red)), 0.0f);      // -0 -> +0
    for (int i = threadIdx.x; i < T; i += ART_THREADS)                            // a thread rewrites the keys it wrote
        keys[i] = __float_as_uint(fabsf(__fsub_rn(art_unkey(keys[i]), m)));       // >= 0: the bits are in order as they are
    __syncthreads();
    const float s = __uint_as_float(art_select(keys, T, k, red));
    if (threadIdx.x == 0) {
        stats[2 * row] = m;
        stats[2 * row + 1] = s;
        flags[row] = 0;
    }
}

__device__ __forceinline__ int art_code(unsigned char flag, float s, float thr_flat, float thr_noisy, bool on_flat, bool on_noisy) {
    if (flag) return 3;
    if (on_flat && s <= thr_flat) return 1;
    if (on_noisy && s > thr_noisy) return 2;
    return 0;
}

// one workgroup per sample, C <= IGN_EEG_ARTIFACT_MAX_CHANNELS
__global__ __launch_bounds__(ART_THREADS) void eeg_artifact_verdict_kernel(const float* __restrict__ stats,
                                                                           const unsigned char* __restrict__ flags,
                                                                           unsigned char* __restrict__ verdict, int C, float flat,
                                                                           float noisy) {
    __shared__ unsigned keys[IGN_EEG_ARTIFACT_MAX_CHANNELS];
    __shared__ int red[ART_RED];
    const size_t base = (size_t)blockIdx.x * C;
    int nf = 0;
    for (int c0 = 0; c0 < C; c0 += ART_THREADS) {
        const int c = c0 + threadIdx.x;
        bool fin = false;
        if (c < C) {
            fin = flags[base + c] == 0;
            keys[c] = fin ? __float_as_uint(stats[2 * (base + c) + 1]) : 0xffffffffu;       // s >= 0; the others sort last
        }
        nf += __syncthreads_count(fin);
    }
    float ref = 0.0f;
    if (nf > 0) ref = __uint_as_float(art_select(keys, C, (nf - 1) / 2, red));
    const bool on_flat = flat > 0.0f, on_noisy = noisy > 0.0f;
    const float thr_flat = __fmul_rn(flat, ref), thr_noisy = __fmul_rn(noisy, ref);
    int ngood = 0;
    for (int c0 = 0; c0 < C; c0 += ART_THREADS) {
        const int c = c0 + threadIdx.x;
        const bool good = c < C && art_code(flags[base + c], stats[2 * (base + c) + 1], thr_flat, thr_noisy, on_flat, on_noisy) == 0;
        ngood += __syncthreads_count(good);
    }
    for (int c = threadIdx.x; c < C; c += ART_THREADS) {
        const int code = art_code(flags[base + c], stats[2 * (base + c) + 1], thr_flat, thr_noisy, on_flat, on_noisy);
        verdict[base + c] = (unsigned char)((code && ngood == 0) ? 4 : code);
    }
}

// tile = (all C, TS samples) of one sample; TS a power of two <= 64, thread = (tx = sample of the tile, ty = row class mod R)
__global__ __launch_bounds__(ART_THREADS) void eeg_artifact_apply_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                                         const unsigned char* __restrict__ flags,
                                                                         const unsigned char* __restrict__ verdict,
                                                                         const float* __restrict__ w, float* __restrict__ out, int C,
                                                                         int T, int TS, int ntile, float clip) {
    extern __shared__ float art_tile[];                // C * TS floats: fl(y - m) of the good rows; 2 C floats (m, s); C verdict bytes
    float* st = art_tile + (size_t)C * TS;
    unsigned char* vs = (unsigned char*)(st + 2 * (size_t)C);
    const int b = blockIdx.x / ntile, t0 = (blockIdx.x - b * ntile) * TS;
    const int tx = threadIdx.x & (TS - 1), ty = threadIdx.x / TS, R = ART_THREADS / TS;
    const size_t rows = (size_t)b * C;
    for (int c = threadIdx.x; c < C; c += ART_THREADS) vs[c] = verdict[rows + c];
    for (int i = threadIdx.x; i < 2 * C; i += ART_THREADS) st[i] = stats[2 * rows + i];
    __syncthreads();
    const int t = t0 + tx;
    const bool inb = t < T;
    const bool on_clip = clip > 0.0f;
    const float kr = __fmul_rn(clip, ART_MAD_TO_SIGMA);
    constexpr int DEPTH = 4;                           // rows in flight per thread: the loads of four rows leave before the first is used
    for (int c0 = ty; c0 < C; c0 += DEPTH * R) {
        float xs[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const int c = c0 + u * R;
            xs[u] = (c < C && inb) ? x[(rows + c) * (size_t)T + t] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const int c = c0 + u * R;
            if (c >= C) break;
            const int code = vs[c];
            if (code >= 1 && code <= 3) continue;      // repaired below
            const size_t idx = (rows + c) * (size_t)T + t;
            if (code == 4 && flags[rows + c] != 0) {   // nothing finite to clamp
                if (inb) out[idx] = 0.0f;
                continue;
            }
            const float m = st[2 * c], sc = st[2 * c + 1];
            const float xv = inb ? xs[u] : m;
            float y = xv;
            if (on_clip) {
                const float r = __fmul_rn(kr, sc);
                const float lo = __fsub_rn(m, r), hi = __fadd_rn(m, r);
                y = xv < lo ? lo : (xv > hi ? hi : xv);
            }
            if (inb) out[idx] = y;
            if (code == 0) art_tile[c * TS + tx] = __fsub_rn(y, m);
        }
    }
    __syncthreads();
    int nth = 0;                                       // the bad rows of the sample go round the row classes
    for (int c = 0; c < C; ++c) {
        const int code = vs[c];
        if (code < 1 || code > 3) continue;
        const bool mine = (nth % R) == ty;
        ++nth;
        if (!mine) continue;
        const float* wr = w ? w + (size_t)c * C : nullptr;
        float acc = 0.0f;
        double ws = 0.0;                               // the weights' sum, rounded once
        for (int j = 0; j < C; ++j) {
            if (j == c || vs[j] != 0) continue;
            const float wj = wr ? wr[j] : 1.0f;
            acc = fmaf(wj, art_tile[j * TS + tx], acc);
            ws += (double)wj;
        }
        if (!(ws > 0.0)) {                             // no good neighbour with a positive weight: the mean of the good rows
            acc = 0.0f;
            ws = 0.0;
            for (int j = 0; j < C; ++j) {
                if (j == c || vs[j] != 0) continue;
                acc += art_tile[j * TS + tx];
                ws += 1.0;
            }
        }
        if (inb) out[(rows + c) * (size_t)T + t] = __fdiv_rn(acc, (float)ws);
    }
}

int art_tile_span(int C) { return C <= 256 ? 64 : C <= 512 ? 32 : 16; }

}  // namespace

// what a row costs when it is staged; rows of up to ART_WAVE_ROW samples are held in registers and the launch asks for none
extern "C" size_t ign_eeg_artifact_lds_bytes(int T) {
    if (T <= 0 || T > IGN_EEG_ARTIFACT_MAX_ROW) return 0;
    return ((size_t)T + ART_RED) * sizeof(unsigned);
}

extern "C" int ign_eeg_artifact_stats_nct(const float* x_nct, float* stats, unsigned char* flags, int B, int C, int T, void* stream) {
    static const char* who = "ign_eeg_artifact_stats_nct";
    if (!x_nct || !stats || !flags) {
        ign_set_error("%s: null pointer (x, stats or flags)", who);
        return IGN_E_ARG;
    }
    if (B <= 0 || C <= 0 || T <= 0) {
        ign_set_error("%s: non-positive dimension (B=%d C=%d T=%d)", who, B, C, T);
        return IGN_E_ARG;
    }
    if (T > IGN_EEG_ARTIFACT_MAX_ROW) {
        ign_set_error("%s: a row of T=%d samples is beyond the %d that are staged in LDS", who, T, IGN_EEG_ARTIFACT_MAX_ROW);
        return IGN_E_TOOBIG;
    }
    if (C > IGN_EEG_ARTIFACT_MAX_CHANNELS) {           // the apply pass would refuse the sample: refuse it before the first launch
        ign_set_error("%s: C=%d electrodes are beyond the %d of the verdict pass", who, C, IGN_EEG_ARTIFACT_MAX_CHANNELS);
        return IGN_E_TOOBIG;
    }
    const long long rows = (long long)B * C;
    if (rows > 0x7fffffffLL) {
        ign_set_error("%s: B*C=%lld rows exceed the launch grid", who, rows);
        return IGN_E_TOOBIG;
    }
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("eeg_artifact_stats", s);
    if (T <= ART_WAVE_ROW) {                           // the keys of a row in registers: the smallest instantiation that holds them
        const int npl = (T + IGN_WAVE - 1) / IGN_WAVE;
        if (npl <= 4) art_launch_wave<4>(x_nct, stats, flags, T, rows, s);
        else if (npl <= 8) art_launch_wave<8>(x_nct, stats, flags, T, rows, s);
        else if (npl <= 16) art_launch_wave<16>(x_nct, stats, flags, T, rows, s);
        else if (npl <= 20) art_launch_wave<20>(x_nct, stats, flags, T, rows, s);
        else if (npl <= 24) art_launch_wave<24>(x_nct, stats, flags, T, rows, s);
        else if (npl <= 28) art_launch_wave<28>(x_nct, stats, flags, T, rows, s);
        else art_launch_wave<32>(x_nct, stats, flags, T, rows, s);
        return ign_check_launch("eeg_artifact_stats_wave_kernel");
    }
    const size_t lds = ign_eeg_artifact_lds_bytes(T);
    if (lds > 64 * 1024)      // the longest rows: a CU of gfx950 has 160 KB of LDS, the default cap is 64
        (void)hipFuncSetAttribute((const void*)eeg_artifact_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(eeg_artifact_stats_kernel, dim3((unsigned)rows), dim3(ART_THREADS), lds, s, x_nct, stats, flags, T);
    return ign_check_launch("eeg_artifact_stats_kernel");
}

extern "C" int ign_eeg_artifact_apply_nct(const float* x_nct, const float* stats, const unsigned char* flags, const float* w,
                                          float* out_nct, unsigned char* verdict, int B, int C, int T, float clip, float flat,
                                          float noisy, void* stream) {
    static const char* who = "ign_eeg_artifact_apply_nct";
    if (!x_nct || !stats || !flags || !out_nct || !verdict) {
        ign_set_error("%s: null pointer (x, stats, flags, out or verdict)", who);
        return IGN_E_ARG;
    }
    if (B <= 0 || C <= 0 || T <= 0) {
        ign_set_error("%s: non-positive dimension (B=%d C=%d T=%d)", who, B, C, T);
        return IGN_E_ARG;
    }
    if (T > IGN_EEG_ARTIFACT_MAX_ROW) {
        ign_set_error("%s: a row of T=%d samples is beyond the %d of the statistics pass", who, T, IGN_EEG_ARTIFACT_MAX_ROW);
        return IGN_E_TOOBIG;
    }
    if (C > IGN_EEG_ARTIFACT_MAX_CHANNELS) {
        ign_set_error("%s: C=%d electrodes are beyond the %d of the verdict pass", who, C, IGN_EEG_ARTIFACT_MAX_CHANNELS);
        return IGN_E_TOOBIG;
    }
    const int TS = art_tile_span(C);
    const int ntile = (T + TS - 1) / TS;
    if ((long long)B * C > 0x7fffffffLL || (long long)B * ntile > 0x7fffffffLL) {
        ign_set_error("%s: B*C=%lld rows exceed the launch grid", who, (long long)B * C);
        return IGN_E_TOOBIG;
    }
    // NaN compares false: a non-finite threshold is an absent key
    const float k = clip > 0.0f ? clip : 0.0f, f = flat > 0.0f ? flat : 0.0f, n = noisy > 0.0f ? noisy : 0.0f;
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("eeg_artifact_apply", s);
    hipLaunchKernelGGL(eeg_artifact_verdict_kernel, dim3((unsigned)B), dim3(ART_THREADS), 0, s, stats, flags, verdict, C, f, n);
    int rc = ign_check_launch("eeg_artifact_verdict_kernel");
    if (rc) return rc;
    const size_t lds = ((size_t)C * TS + 2 * (size_t)C) * sizeof(float) + (((size_t)C + 3) & ~(size_t)3);     // <= 64 KB + 9 KB
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)eeg_artifact_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(eeg_artifact_apply_kernel, dim3((unsigned)((long long)B * ntile)), dim3(ART_THREADS), lds, s, x_nct, stats,
                       flags, verdict, w, out_nct, C, T, TS, ntile, k);
    return ign_check_launch("eeg_artifact_apply_kernel");
}
