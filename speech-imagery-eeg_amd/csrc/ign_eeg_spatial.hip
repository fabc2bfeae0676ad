// Spatial filter stage in front of every other EEG stage (run.py --eeg_spatial; ops.eeg_spatial, ops.eeg_gram; the numpy restatement
// is utils/eeg_spatial.py:spatial_numpy / gram_numpy): one small matrix per group of samples applied across the electrodes of the
// raw (B, Cin, T) batch -- a re-reference, a montage or unmixing matrix, a per-subject whitening (Euclidean alignment) are all
//
//   g = gid[b] (0 without gid)        p[c] = x[b,c,0]        xc[c,t] = x[b,c,t] - p[c]
//   a[s,t]   = fmaf chain over c = 0 .. Cin-1 ascending of W[g,s,c] * xc[c,t], from 0
//   P[s]     = the same chain of W[g,s,c] * p[c]
//   y[b,s,t] = a[s,t] + P[s]
//
// The pivot p is the FIR kernel's (ign_eeg_preprocess.hip): recordings carry offsets of 1e4 uV over a signal of tens of uV, and
// without it every partial sum of the chain rounds at the offset's ulp.  With it everything that varies along t is computed at the
// signal's scale and the offset enters once per row, as the constant P[s] that every later stage removes.
//
// Both products run on v_mfma_f32_32x32x2_f32 in the layout of ign_sbm_bilinear.hip: a 256-thread block owns a 64 (rows) x 64*NACC
// (columns) tile, its 4 waves sit 2 x 2 with NACC 32x32 accumulators each, k advances in staged tiles of 32 (A[k][row], B[k][col] in
// LDS, pitch + 1, the next tile's global loads in flight while this one is multiplied).  On gfx950 the instruction accumulates its
// two k in ascending order in fp32 fused multiply-adds, so the accumulator IS the chain above; rows, columns and k beyond the
// operands are staged as literal zeros (fmaf(0, 0, acc) leaves acc alone) and never read or written in memory.
//
//   apply   A = W[g] (row s, k = c: k-contiguous), B = x[b] - p (k = c, column t: coalesced along t, subtracted as it is staged);
//           tile 64 x 128, grid (tiles of one sample, B).  p sits in LDS for the whole block, P[s] is a scalar chain by the block's
//           first 64 threads, added in the epilogue.  A sample whose gid is outside [0, G) gets zeros and reads nothing.
//   gram    z = (x - p) - m,  m[c] = (sum_t (x[c,t] - p[c])) / T  (a kernel of its own: one wave per row, lane-strided sums then the
//           butterfly);  A = B = z[b] (row / column = electrode, k = t), tile 64 x 64, upper triangle of tiles only, one (b, tile)
//           per block into a per-sample workspace;  a second kernel sums every group's samples in ascending b, reading element
//           (min(i,j), max(i,j)) for both (i,j) and (j,i): gram[g] is symmetric bit for bit, empty groups are zeros, count[g] is
//           written beside it.  No atomics anywhere: two calls give the same bits, and a sample's share does not depend on B.
#include "ign_common.h"

namespace {

typedef float sp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int SP_MT = 64;                 // output rows per block
constexpr int SP_KT = 32;                 // k per staged tile
constexpr int SP_THREADS = 256;
constexpr int SP_APITCH = SP_MT + 1;

__device__ __forceinline__ int sp_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__host__ __device__ __forceinline__ int sp_cdiv(long long a, int b) { return (int)((a + b - 1) / b); }

// thread t's e-th staged element of a KT x COLS tile: (kl, column offset).  KMAJOR: consecutive columns are consecutive in memory
// (threads walk the column); otherwise consecutive k are (threads walk k and the LDS store transposes).
template <bool KMAJOR, int COLS>
__device__ __forceinline__ void sp_stage_pos(int t, int e, int& kl, int& cl) {
    if (KMAJOR) { cl = t % COLS; kl = t / COLS + e * (SP_THREADS / COLS); }
    else        { kl = t % SP_KT; cl = t / SP_KT + e * (SP_THREADS / SP_KT); }
}

template <class L, int COLS, int E>
__device__ __forceinline__ void sp_stage_load(const L& ld, int kt, int c0, float (&r)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        int kl, cl;
        sp_stage_pos<L::KMAJOR, COLS>(threadIdx.x, e, kl, cl);
        r[e] = ld(kt * SP_KT + kl, cl, c0 + cl);
    }
}

template <class L, int COLS, int E>
__device__ __forceinline__ void sp_stage_store(float* s, const float (&r)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        int kl, cl;
        sp_stage_pos<L::KMAJOR, COLS>(threadIdx.x, e, kl, cl);
        s[kl * (COLS + 1) + cl] = r[e];
    }
}

// acc[c] = A[rows m0 + 32 wm ..][k] * B[k][cols n0 + 32 NACC wn + 32 c ..] over the k tiles 0 .. nk - 1.  A loader is called as
// ld(k, local column, global column) and returns 0 outside its operand.
template <int NACC, class LA, class LB>
__device__ __forceinline__ void sp_mainloop(const LA& la, const LB& lb, int nk, int m0, int n0, float* As, float* Bs,
                                            sp_f32x16 (&acc)[NACC]) {
    constexpr int NT = 64 * NACC, BPITCH = NT + 1;
    constexpr int AE = SP_KT * SP_MT / SP_THREADS, BE = SP_KT * NT / SP_THREADS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int h = lane >> 5, l32 = lane & 31;
#pragma unroll
    for (int c = 0; c < NACC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    float ra[AE], rb[BE];
    sp_stage_load<LA, SP_MT>(la, 0, m0, ra);
    sp_stage_load<LB, NT>(lb, 0, n0, rb);
    for (int kt = 0; kt < nk; ++kt) {
        sp_stage_store<LA, SP_MT>(As, ra);
        sp_stage_store<LB, NT>(Bs, rb);
        __syncthreads();
        if (kt + 1 < nk) {
            sp_stage_load<LA, SP_MT>(la, kt + 1, m0, ra);
            sp_stage_load<LB, NT>(lb, kt + 1, n0, rb);
        }
        const float* a = As + h * SP_APITCH + 32 * wm + l32;
        const float* b = Bs + h * BPITCH + 32 * NACC * wn + l32;
#pragma unroll
        for (int s = 0; s < SP_KT / 2; ++s) {
            const float av = a[2 * s * SP_APITCH];
#pragma unroll
            for (int c = 0; c < NACC; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[2 * s * BPITCH + 32 * c], acc[c], 0, 0, 0);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------- apply
constexpr int AP_NACC = 2, AP_NT = 64 * AP_NACC;

// A: W[g] (Cs, Cin) as A[k = c][row = s]
struct LdApplyA {
    static constexpr bool KMAJOR = false;
    const float* w; int Cs, Cin;
    __device__ float operator()(int k, int, int s) const { return (s < Cs && k < Cin) ? w[(size_t)s * Cin + k] : 0.f; }
};
// B: x[b] (Cin, T) minus the row's pivot (LDS) as B[k = c][col = t]
struct LdApplyB {
    static constexpr bool KMAJOR = true;
    const float* x; const float* piv; int Cin, T;
    __device__ float operator()(int k, int, int t) const { return (k < Cin && t < T) ? x[(size_t)k * T + t] - piv[k] : 0.f; }
};

__global__ __launch_bounds__(SP_THREADS) void eeg_spatial_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const int* __restrict__ gid, float* __restrict__ out, int Cin, int T,
                                                                 int Cs, int G) {
    __shared__ float As[SP_KT * SP_APITCH];
    __shared__ float Bs[SP_KT * (AP_NT + 1)];
    __shared__ float piv[IGN_EEG_SPATIAL_MAX_CHANNELS];
    __shared__ float Ps[SP_MT];
    const int b = blockIdx.y;
    const int nst = sp_cdiv(Cs, SP_MT);
    const int st = blockIdx.x % nst, tt = blockIdx.x / nst;
    const int m0 = st * SP_MT, n0 = tt * AP_NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int h = lane >> 5, l32 = lane & 31;
    float* ob = out + (size_t)b * Cs * T;
    const int g = gid ? gid[b] : 0;
    if (g < 0 || g >= G) {                           // block-uniform: zeros for this sample, nothing read
        for (int e = threadIdx.x; e < SP_MT * AP_NT; e += SP_THREADS) {
            const int s = m0 + e / AP_NT, t = n0 + e % AP_NT;
            if (s < Cs && t < T) ob[(size_t)s * T + t] = 0.f;
        }
        return;
    }
    const float* xb = x + (size_t)b * Cin * T;
    const float* wg = w + (size_t)g * Cs * Cin;
    for (int c = threadIdx.x; c < Cin; c += SP_THREADS) piv[c] = xb[(size_t)c * T];
    __syncthreads();
    if (threadIdx.x < SP_MT) {                       // P[s]: the chain over the pivots
        const int s = m0 + threadIdx.x;
        float acc = 0.f;
        if (s < Cs)
            for (int c = 0; c < Cin; ++c) acc = fmaf(wg[(size_t)s * Cin + c], piv[c], acc);
        Ps[threadIdx.x] = acc;
    }
    sp_f32x16 acc[AP_NACC];
    sp_mainloop<AP_NACC>(LdApplyA{wg, Cs, Cin}, LdApplyB{xb, piv, Cin, T}, sp_cdiv(Cin, SP_KT), m0, n0, As, Bs, acc);
    // the main loop's barriers have published Ps
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * wm + sp_acc_row(r, h);
        const int s = m0 + row;
        const float pr = Ps[row];
#pragma unroll
        for (int c = 0; c < AP_NACC; ++c) {
            const int t = n0 + 32 * AP_NACC * wn + 32 * c + l32;
            if (s < Cs && t < T) ob[(size_t)s * T + t] = acc[c][r] + pr;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------- gram
constexpr int GR_NT = 64;

// ws layout: mean (B * C) then the per-sample partial Grams (B, C, C); only elements of upper-triangle tiles are ever written or read
__global__ __launch_bounds__(SP_THREADS) void eeg_gram_mean_kernel(const float* __restrict__ x, float* __restrict__ mean, long long rows,
                                                                   int T) {
    const long long row = (long long)blockIdx.x * (SP_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                         // wave-uniform
    const int lane = threadIdx.x & 63;
    const float* xr = x + (size_t)row * T;
    const float p = xr[0];
    float s = 0.f;
    for (int t = lane; t < T; t += 64) s += xr[t] - p;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) mean[row] = s / (float)T;
}

// z[b] rows e0 .. e0 + 63 as an operand [k = t][col = electrode]: ((x - pivot) - mean), pivot and mean from LDS by local column
struct LdGram {
    static constexpr bool KMAJOR = false;
    const float* x; const float* piv; const float* mu; int C, T;
    __device__ float operator()(int k, int cl, int e) const {
        return (e < C && k < T) ? (x[(size_t)e * T + k] - piv[cl]) - mu[cl] : 0.f;
    }
};

// tile index -> (it, jt) with it <= jt < n, rows of the triangle in order
__device__ __forceinline__ void gr_tile(int tile, int n, int& it, int& jt) {
    it = 0;
    while (tile >= n - it) { tile -= n - it; ++it; }
    jt = it + tile;
}

__global__ __launch_bounds__(SP_THREADS) void eeg_gram_part_kernel(const float* __restrict__ x, const int* __restrict__ gid,
                                                                   const float* __restrict__ mean, float* __restrict__ part, int C,
                                                                   int T, int G) {
    __shared__ float As[SP_KT * SP_APITCH];
    __shared__ float Bs[SP_KT * (GR_NT + 1)];
    __shared__ float piv[2][SP_MT], mu[2][SP_MT];
    const int b = blockIdx.y;
    const int g = gid ? gid[b] : 0;
    if (g < 0 || g >= G) return;                     // belongs to no group: its partial is never read
    int it, jt;
    gr_tile(blockIdx.x, sp_cdiv(C, SP_MT), it, jt);
    const int m0 = it * SP_MT, n0 = jt * GR_NT;
    const float* xb = x + (size_t)b * C * T;
    if (threadIdx.x < 2 * SP_MT) {
        const int side = threadIdx.x / SP_MT, l = threadIdx.x % SP_MT;
        const int e = (side ? n0 : m0) + l;
        piv[side][l] = e < C ? xb[(size_t)e * T] : 0.f;
        mu[side][l] = e < C ? mean[(size_t)b * C + e] : 0.f;
    }
    __syncthreads();
    sp_f32x16 acc[1];
    sp_mainloop<1>(LdGram{xb, piv[0], mu[0], C, T}, LdGram{xb, piv[1], mu[1], C, T}, sp_cdiv(T, SP_KT), m0, n0, As, Bs, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int h = lane >> 5, l32 = lane & 31;
    float* pb = part + (size_t)b * C * C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = m0 + 32 * wm + sp_acc_row(r, h);
        const int j = n0 + 32 * wn + l32;
        if (i < C && j < C) pb[(size_t)i * C + j] = acc[0][r];
    }
}

// gram[g,i,j] = sum over b with gid[b] == g, ascending, of part[b][min(i,j)][max(i,j)]; count[g] by the first G threads
__global__ __launch_bounds__(SP_THREADS) void eeg_gram_reduce_kernel(const float* __restrict__ part, const int* __restrict__ gid,
                                                                     float* __restrict__ gram, int* __restrict__ count, int B, int C,
                                                                     int G) {
    const long long e = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    const long long CC = (long long)C * C;
    if (e < G) {
        int n = 0;
        for (int b = 0; b < B; ++b) n += (gid ? gid[b] : 0) == (int)e;
        count[e] = n;
    }
    if (e >= CC * G) return;
    const int g = (int)(e / CC);
    const int ij = (int)(e - (long long)g * CC);
    const int i = ij / C, j = ij - i * C;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const float* p = part + (size_t)lo * C + hi;
    float s = 0.f;
    for (int b = 0; b < B; ++b)
        if ((gid ? gid[b] : 0) == g) s += p[(size_t)b * CC];
    gram[e] = s;
}

bool sp_dims(const char* who, const char* name, int v, int limit) {
    if (v > limit) {
        ign_set_error("%s: %s=%d is beyond the limit of %d", who, name, v, limit);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int ign_eeg_spatial_nct(const float* x_nct, const float* w_gsc, const int* gid, float* out_nst, int B, int Cin, int T,
                                   int Cs, int G, void* stream) {
    static const char* who = "ign_eeg_spatial_nct";
    if (!x_nct || !w_gsc || !out_nst) {
        ign_set_error("%s: null pointer (x, w or out)", who);
        return IGN_E_ARG;
    }
    if (B <= 0 || Cin <= 0 || T <= 0 || Cs <= 0 || G <= 0) {
        ign_set_error("%s: non-positive dimension (B=%d Cin=%d T=%d Cs=%d G=%d)", who, B, Cin, T, Cs, G);
        return IGN_E_ARG;
    }
    if (B > 65535) {
        ign_set_error("%s: B=%d exceeds the launch grid (65535 samples per call)", who, B);
        return IGN_E_TOOBIG;
    }
    if (!sp_dims(who, "Cin", Cin, IGN_EEG_SPATIAL_MAX_CHANNELS) || !sp_dims(who, "Cs", Cs, IGN_EEG_SPATIAL_MAX_CHANNELS) ||
        !sp_dims(who, "G", G, IGN_EEG_SPATIAL_MAX_GROUPS))
        return IGN_E_TOOBIG;
    const long long tiles = (long long)sp_cdiv(Cs, SP_MT) * sp_cdiv(T, AP_NT);
    if (tiles > 0x7fffffffLL) {
        ign_set_error("%s: T=%d exceeds the launch grid", who, T);
        return IGN_E_TOOBIG;
    }
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("eeg_spatial", s);
    hipLaunchKernelGGL(eeg_spatial_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(SP_THREADS), 0, s, x_nct, w_gsc, gid, out_nst, Cin,
                       T, Cs, G);
    return ign_check_launch("eeg_spatial_kernel");
}

static bool gram_check(const char* who, int B, int C, int T, int G, int* rc) {
    if (B <= 0 || C <= 0 || T <= 0 || G <= 0) {
        ign_set_error("%s: non-positive dimension (B=%d C=%d T=%d G=%d)", who, B, C, T, G);
        *rc = IGN_E_ARG;
        return false;
    }
    if (B > 65535) {
        ign_set_error("%s: B=%d exceeds the launch grid (65535 samples per call)", who, B);
        *rc = IGN_E_TOOBIG;
        return false;
    }
    if (!sp_dims(who, "C", C, IGN_EEG_SPATIAL_MAX_CHANNELS) || !sp_dims(who, "G", G, IGN_EEG_SPATIAL_MAX_GROUPS)) {
        *rc = IGN_E_TOOBIG;
        return false;
    }
    return true;
}

extern "C" size_t ign_eeg_gram_ws_bytes(int B, int C, int T, int G) {
    int rc;
    if (!gram_check("ign_eeg_gram_ws_bytes", B, C, T, G, &rc)) return 0;
    return ((size_t)B * C + (size_t)B * C * C) * sizeof(float);
}

extern "C" int ign_eeg_gram_nct(const float* x_nct, const int* gid, float* gram_gcc, int* count_g, float* ws, int B, int C, int T, int G,
                                void* stream) {
    static const char* who = "ign_eeg_gram_nct";
    if (!x_nct || !gram_gcc || !count_g || !ws) {
        ign_set_error("%s: null pointer (x, gram, count or ws)", who);
        return IGN_E_ARG;
    }
    int rc = 0;
    if (!gram_check(who, B, C, T, G, &rc)) return rc;
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("eeg_gram", s);
    float* mean = ws;
    float* part = ws + (size_t)B * C;
    const long long rows = (long long)B * C;
    hipLaunchKernelGGL(eeg_gram_mean_kernel, dim3((unsigned)sp_cdiv(rows, SP_THREADS / 64)), dim3(SP_THREADS), 0, s, x_nct, mean, rows, T);
    if ((rc = ign_check_launch("eeg_gram_mean_kernel"))) return rc;
    const int n = sp_cdiv(C, SP_MT);
    hipLaunchKernelGGL(eeg_gram_part_kernel, dim3((unsigned)(n * (n + 1) / 2), (unsigned)B), dim3(SP_THREADS), 0, s, x_nct, gid, mean,
                       part, C, T, G);
    if ((rc = ign_check_launch("eeg_gram_part_kernel"))) return rc;
    const long long elems = (long long)G * C * C;
    hipLaunchKernelGGL(eeg_gram_reduce_kernel, dim3((unsigned)sp_cdiv(elems, SP_THREADS)), dim3(SP_THREADS), 0, s, part, gid, gram_gcc,
                       count_g, B, C, G);
    return ign_check_launch("eeg_gram_reduce_kernel");
}
