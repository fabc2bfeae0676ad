// SBM bilinear head (sbm_cls='bilinear', IGN/model/Shapelet.py:170-177, 199-205): the bilinear term of
//   out = output_layer(drop(p)) + output_bilinear(drop(p), drop(p))
// as three exact-fp32 GEMMs on v_mfma_f32_32x32x2_f32.  With inputs u, v (B,F) and weight W (N,F,F), no bias:
//   forward   T_n = U W_n (B x F, K = F)           out[b,n] = sum_j T_n[b,j] V[b,j]   (row dot in the epilogue)
//   dU        dU = sum_n (g_n . V) W_n^T            N NT GEMMs (one per class, K = F), g scaled on the operand load;
//                                                   the N partials are summed in class order by a second kernel
//   dV        dV = sum_n g_n . T_n                  elementwise from the saved T, in the dU kernel's (b, i) tiles
//   dW        dW_n = (g_n . U)^T V                  TN GEMM over K = B
// nn.Bilinear's autograd instead writes a (B,F,F) temporary per class for dU (_trilinear backward).
//
// Layout: one 256-thread block computes a 64 x 128 output tile (rows x columns); its 4 waves sit 2 x 2, each wave owns
// 32 rows x 64 columns as two 32x32 accumulators that share the A fragment.  K advances in tiles of 32: both operands are
// staged k-major in LDS (A[k][row], B[k][col], pitch +1 so the transposing stores of k-contiguous operands are
// conflict-free), the next tile's global loads are in flight while the current one is multiplied.  Out-of-range rows,
// columns and k are staged as zeros, so any B, F, N >= 1 works.  Blocks are numbered so that each XCD gets a contiguous
// run of tiles with the row tile fastest: the row tiles that read the same W tile land on the same L2.
// Reductions are fixed-order (butterfly within a wave, then a per-tile partial summed in tile order by a second kernel):
// no float atomics, results are bitwise reproducible.  Memory: T (B,N,F) when a backward follows, B*N*ceil(F/128) partial
// row dots in the forward and the N per-class partials of dU (B*N*F) in the backward; nothing of size F^2 besides W and dW.
#include "ign_common.h"

namespace {

typedef float bl_f32x16 __attribute__((ext_vector_type(16)));

constexpr int BL_MT = 64;                 // output rows per block
constexpr int BL_NT = 128;                // output columns per block
constexpr int BL_KT = 32;                 // k per staged tile
constexpr int BL_THREADS = 256;
constexpr int BL_APITCH = BL_MT + 1;      // floats per staged k row of A
constexpr int BL_BPITCH = BL_NT + 1;      // floats per staged k row of B
constexpr int BL_AE = BL_KT * BL_MT / BL_THREADS;   // A elements staged per thread (8)
constexpr int BL_BE = BL_KT * BL_NT / BL_THREADS;   // B elements staged per thread (16)
constexpr int BL_XCD = 8;

__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__host__ __device__ __forceinline__ int cdiv(long long a, int b) { return (int)((a + b - 1) / b); }

// tile index of this block: blocks are dealt round-robin to the XCDs, so block l runs on XCD l % 8; give XCD x the
// contiguous tile range [x * per, (x + 1) * per).  The grid is padded to a multiple of 8; padding blocks return.
__device__ __forceinline__ int bl_tile() {
    const int per = gridDim.x / BL_XCD;
    return (blockIdx.x % BL_XCD) * per + blockIdx.x / BL_XCD;
}

// Operand loaders: element (k, col) of a K x cols operand, zero outside.  kt is the k tile, kl the k inside it, c the
// global column (row of the output for A).  KMAJOR: consecutive columns are consecutive in memory (threads walk the
// column); otherwise consecutive k are (threads walk k and the LDS store transposes).

// forward A: U (B,F) as A[k = i][row = b]
struct LdFwdA {
    static constexpr bool KMAJOR = false;
    const float* u; int B, F;
    __device__ float operator()(int kt, int kl, int c) const {
        const int k = kt * BL_KT + kl;
        return (c < B && k < F) ? u[(long long)c * F + k] : 0.f;
    }
};
// forward B: W_n (F,F) as B[k = i][col = j]
struct LdFwdB {
    static constexpr bool KMAJOR = true;
    const float* w; int F;
    __device__ float operator()(int kt, int kl, int c) const {
        const int k = kt * BL_KT + kl;
        return (c < F && k < F) ? w[(long long)k * F + c] : 0.f;
    }
};
// dU A: g_n . V as A[k = (n, j)][row = b]; k tiles run over j inside n
struct LdDuA {
    static constexpr bool KMAJOR = false;
    const float* v; const float* g; int B, F, N, nkj;
    __device__ float operator()(int kt, int kl, int c) const {
        const int n = kt / nkj;
        const int j = (kt - n * nkj) * BL_KT + kl;
        return (c < B && j < F) ? g[(long long)c * N + n] * v[(long long)c * F + j] : 0.f;
    }
};
// dU B: W_n^T as B[k = (n, j)][col = i] = W[n][i][j]
struct LdDuB {
    static constexpr bool KMAJOR = false;
    const float* w; int F, nkj;
    __device__ float operator()(int kt, int kl, int c) const {
        const int n = kt / nkj;
        const int j = (kt - n * nkj) * BL_KT + kl;
        return (c < F && j < F) ? w[((long long)n * F + c) * F + j] : 0.f;
    }
};
// dW A: g_n . U as A[k = b][row = i]
struct LdDwA {
    static constexpr bool KMAJOR = true;
    const float* u; const float* g; int B, F, N, n;
    __device__ float operator()(int kt, int kl, int c) const {
        const int b = kt * BL_KT + kl;
        return (c < F && b < B) ? g[(long long)b * N + n] * u[(long long)b * F + c] : 0.f;
    }
};
// dW B: V as B[k = b][col = j]
struct LdDwB {
    static constexpr bool KMAJOR = true;
    const float* v; int B, F;
    __device__ float operator()(int kt, int kl, int c) const {
        const int b = kt * BL_KT + kl;
        return (c < F && b < B) ? v[(long long)b * F + c] : 0.f;
    }
};

// thread t's e-th staged element of a KT x COLS tile: (kl, column offset)
template <bool KMAJOR, int COLS>
__device__ __forceinline__ void stage_pos(int t, int e, int& kl, int& cl) {
    if (KMAJOR) { cl = t % COLS; kl = t / COLS + e * (BL_THREADS / COLS); }
    else        { kl = t % BL_KT; cl = t / BL_KT + e * (BL_THREADS / BL_KT); }
}

template <class L, int COLS, int E>
__device__ __forceinline__ void stage_load(const L& ld, int kt, int c0, float (&r)[E]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        int kl, cl;
        stage_pos<L::KMAJOR, COLS>(t, e, kl, cl);
        r[e] = ld(kt, kl, c0 + cl);
    }
}

template <class L, int COLS, int PITCH, int E>
__device__ __forceinline__ void stage_store(float* s, const float (&r)[E]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        int kl, cl;
        stage_pos<L::KMAJOR, COLS>(t, e, kl, cl);
        s[kl * PITCH + cl] = r[e];
    }
}

// acc[0..1] = A[rows m0 + 32 wm ..][k] * B[k][cols n0 + 64 wn + 32 c ..] over the k tiles kt0 .. kt0 + nk - 1
template <class LA, class LB>
__device__ __forceinline__ void bl_mainloop(const LA& la, const LB& lb, int kt0, int nk, int m0, int n0, float* As, float* Bs,
                                            bl_f32x16 (&acc)[2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int h = lane >> 5, l32 = lane & 31;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    if (nk <= 0) return;
    float ra[BL_AE], rb[BL_BE];
    stage_load<LA, BL_MT>(la, kt0, m0, ra);
    stage_load<LB, BL_NT>(lb, kt0, n0, rb);
    for (int kt = 0; kt < nk; ++kt) {
        stage_store<LA, BL_MT, BL_APITCH>(As, ra);
        stage_store<LB, BL_NT, BL_BPITCH>(Bs, rb);
        __syncthreads();
        if (kt + 1 < nk) {
            stage_load<LA, BL_MT>(la, kt0 + kt + 1, m0, ra);
            stage_load<LB, BL_NT>(lb, kt0 + kt + 1, n0, rb);
        }
        const float* a = As + h * BL_APITCH + 32 * wm + l32;
        const float* b = Bs + h * BL_BPITCH + 64 * wn + l32;
#pragma unroll
        for (int s = 0; s < BL_KT / 2; ++s) {
            const float av = a[2 * s * BL_APITCH];
            const float b0 = b[2 * s * BL_BPITCH];
            const float b1 = b[2 * s * BL_BPITCH + 32];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
// tile = (row tile of b, column tile of j, class n), b fastest.  Writes T (when t_out) and the tile's partial row dots
// part[(n * njt + jt) * B + b] = sum_{j in tile} T[b,n,j] V[b,j].
__global__ __launch_bounds__(BL_THREADS) void sbm_bilinear_fwd_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                      const float* __restrict__ w, float* __restrict__ t_out,
                                                                      float* __restrict__ part, int B, int F, int N) {
    __shared__ float As[BL_KT * BL_APITCH];
    __shared__ float Bs[BL_KT * BL_BPITCH];
    __shared__ float red[2][BL_MT];
    const int nbt = cdiv(B, BL_MT), njt = cdiv(F, BL_NT);
    const int tile = bl_tile();
    if (tile >= nbt * njt * N) return;
    const int bt = tile % nbt, jt = (tile / nbt) % njt, n = tile / (nbt * njt);
    const int m0 = bt * BL_MT, n0 = jt * BL_NT;
    bl_f32x16 acc[2];
    bl_mainloop(LdFwdA{u, B, F}, LdFwdB{w + (long long)n * F * F, F}, 0, cdiv(F, BL_KT), m0, n0, As, Bs, acc);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int h = lane >> 5, l32 = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = 32 * wm + acc_row(r, h);
        const int b = m0 + row;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int j = n0 + 64 * wn + 32 * c + l32;
            if (b < B && j < F) {
                const float tv = acc[c][r];
                if (t_out) t_out[((long long)b * N + n) * F + j] = tv;
                dot = fmaf(tv, v[(long long)b * F + j], dot);
            }
        }
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) dot += __shfl_xor(dot, o);
        if (l32 == 0) red[wn][row] = dot;
    }
    __syncthreads();
    if (threadIdx.x < BL_MT) {
        const int b = m0 + threadIdx.x;
        if (b < B) part[((long long)n * njt + jt) * B + b] = red[0][threadIdx.x] + red[1][threadIdx.x];
    }
}

// out[b,n] = sum over column tiles (in order) of the partial row dots
__global__ __launch_bounds__(BL_THREADS) void sbm_bilinear_rowdot_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                         int B, int N, int njt) {
    const long long e = (long long)blockIdx.x * BL_THREADS + threadIdx.x;
    if (e >= (long long)B * N) return;
    const int n = (int)(e / B), b = (int)(e - (long long)n * B);
    const float* p = part + (long long)n * njt * B + b;
    float s = 0.f;
    for (int jt = 0; jt < njt; ++jt) s += p[(long long)jt * B];
    out[(long long)b * N + n] = s;
}

// ---------------------------------------------------------------------------------------------------------------- backward
// tile = (row tile of b, column tile of i, class n), b fastest.  gu (nullable): class n's share of the dU tile, written to gu
// itself when N == 1, else to part[(n * B + b) * F + i].  gv (nullable): dV[b, i] = sum_n g[b,n] T[b,n,i] over the same
// rectangle, by the class-0 blocks.
__global__ __launch_bounds__(BL_THREADS) void sbm_bilinear_dgrad_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                        const float* __restrict__ w, const float* __restrict__ t_save,
                                                                        const float* __restrict__ gout, float* __restrict__ gu,
                                                                        float* __restrict__ gv, float* __restrict__ part, int B,
                                                                        int F, int N) {
    __shared__ float As[BL_KT * BL_APITCH];
    __shared__ float Bs[BL_KT * BL_BPITCH];
    const int nbt = cdiv(B, BL_MT), nit = cdiv(F, BL_NT);
    const int tile = bl_tile();
    if (tile >= nbt * nit * N) return;
    const int bt = tile % nbt, it = (tile / nbt) % nit, n = tile / (nbt * nit);
    const int m0 = bt * BL_MT, n0 = it * BL_NT;
    if (gu) {
        const int nkj = cdiv(F, BL_KT);
        float* dst = N == 1 ? gu : part + (long long)n * B * F;
        bl_f32x16 acc[2];
        bl_mainloop(LdDuA{v, gout, B, F, N, nkj}, LdDuB{w, F, nkj}, n * nkj, nkj, m0, n0, As, Bs, acc);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int wm = wave & 1, wn = wave >> 1;
        const int h = lane >> 5, l32 = lane & 31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int b = m0 + 32 * wm + acc_row(r, h);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int i = n0 + 64 * wn + 32 * c + l32;
                if (b < B && i < F) dst[(long long)b * F + i] = acc[c][r];
            }
        }
    }
    if (gv && n == 0) {
        for (int e = threadIdx.x; e < BL_MT * BL_NT; e += BL_THREADS) {
            const int b = m0 + e / BL_NT, j = n0 + e % BL_NT;
            if (b >= B || j >= F) continue;
            float s = 0.f;
            for (int n = 0; n < N; ++n) s = fmaf(gout[(long long)b * N + n], t_save[((long long)b * N + n) * F + j], s);
            gv[(long long)b * F + j] = s;
        }
    }
}

// gu[e] = sum_n part[n * B * F + e], classes in order
__global__ __launch_bounds__(BL_THREADS) void sbm_bilinear_dgrad_reduce_kernel(const float* __restrict__ part,
                                                                               float* __restrict__ gu, long long BF, int N) {
    const long long e = (long long)blockIdx.x * BL_THREADS + threadIdx.x;
    if (e >= BF) return;
    float s = part[e];
    for (int n = 1; n < N; ++n) s += part[(long long)n * BF + e];
    gu[e] = s;
}

// tile = (row tile of i, column tile of j, class n), i fastest.  gw[n][i][j] = sum_b g[b,n] U[b,i] V[b,j]
__global__ __launch_bounds__(BL_THREADS) void sbm_bilinear_wgrad_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                        const float* __restrict__ gout, float* __restrict__ gw,
                                                                        int B, int F, int N) {
    __shared__ float As[BL_KT * BL_APITCH];
    __shared__ float Bs[BL_KT * BL_BPITCH];
    const int nit = cdiv(F, BL_MT), njt = cdiv(F, BL_NT);
    const int tile = bl_tile();
    if (tile >= nit * njt * N) return;
    const int it = tile % nit, jt = (tile / nit) % njt, n = tile / (nit * njt);
    const int m0 = it * BL_MT, n0 = jt * BL_NT;
    bl_f32x16 acc[2];
    bl_mainloop(LdDwA{u, gout, B, F, N, n}, LdDwB{v, B, F}, 0, cdiv(B, BL_KT), m0, n0, As, Bs, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int h = lane >> 5, l32 = lane & 31;
    float* g = gw + (long long)n * F * F;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = m0 + 32 * wm + acc_row(r, h);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int j = n0 + 64 * wn + 32 * c + l32;
            if (i < F && j < F) g[(long long)i * F + j] = acc[c][r];
        }
    }
}

// blocks for `tiles` tiles, padded to a multiple of the XCD count (bl_tile)
long long bl_grid(long long tiles) { return (tiles + BL_XCD - 1) / BL_XCD * BL_XCD; }

bool bl_check(const char* who, const float* u, const float* v, const float* w, int B, int F, int N) {
    if (!u || !v || !w) { ign_set_error("%s: null pointer (u, v or w)", who); return false; }
    if (B < 1 || F < 1 || N < 1) { ign_set_error("%s: bad dimensions B=%d F=%d N=%d", who, B, F, N); return false; }
    const long long fwd_tiles = ((long long)B + BL_MT - 1) / BL_MT * ((F + BL_NT - 1) / BL_NT) * N;
    const long long w_tiles = (long long)((F + BL_MT - 1) / BL_MT) * ((F + BL_NT - 1) / BL_NT) * N;
    if (bl_grid(fwd_tiles) > 0x7fffffffLL || bl_grid(w_tiles) > 0x7fffffffLL || (long long)B * N > 0x7fffffffLL) {
        ign_set_error("%s: bad dimensions B=%d F=%d N=%d (grid too large)", who, B, F, N);
        return false;
    }
    return true;
}

}  // namespace

extern "C" size_t ign_sbm_bilinear_workspace_bytes(int B, int F, int N) {
    if (B < 1 || F < 1 || N < 1) return 0;
    const size_t fwd = (size_t)B * N * cdiv(F, BL_NT);                 // partial row dots
    const size_t bwd = N > 1 ? (size_t)B * N * F : 0;                   // per-class partials of dU
    return (fwd > bwd ? fwd : bwd) * sizeof(float);
}

extern "C" int ign_sbm_bilinear_fwd(const float* u, const float* v, const float* w, float* out, float* t_save, void* workspace,
                                    int B, int F, int N, void* stream) {
    static const char* who = "ign_sbm_bilinear_fwd";
    if (!bl_check(who, u, v, w, B, F, N)) return IGN_E_ARG;
    if (!out) { ign_set_error("%s: null pointer (out)", who); return IGN_E_ARG; }
    if (!workspace) { ign_set_error("%s: null workspace", who); return IGN_E_ARG; }
    const int nbt = cdiv(B, BL_MT), njt = cdiv(F, BL_NT);
    float* part = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("sbm_bilinear", s);
    hipLaunchKernelGGL(sbm_bilinear_fwd_kernel, dim3((unsigned)bl_grid((long long)nbt * njt * N)), dim3(BL_THREADS), 0, s, u, v, w,
                       t_save, part, B, F, N);
    int rc = ign_check_launch("sbm_bilinear_fwd_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(sbm_bilinear_rowdot_kernel, dim3(cdiv((long long)B * N, BL_THREADS)), dim3(BL_THREADS), 0, s, part, out, B, N,
                       njt);
    return ign_check_launch("sbm_bilinear_rowdot_kernel");
}

extern "C" int ign_sbm_bilinear_bwd(const float* u, const float* v, const float* w, const float* t_save, const float* gout, float* gu,
                                    float* gv, float* gw, void* workspace, int B, int F, int N, void* stream) {
    static const char* who = "ign_sbm_bilinear_bwd";
    if (!bl_check(who, u, v, w, B, F, N)) return IGN_E_ARG;
    if (!gout) { ign_set_error("%s: null pointer (gout)", who); return IGN_E_ARG; }
    if (gu && N > 1 && !workspace) { ign_set_error("%s: null workspace (needed for gu when N > 1)", who); return IGN_E_ARG; }
    if (gv && !t_save) { ign_set_error("%s: null pointer (t_save, needed for gv)", who); return IGN_E_ARG; }
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("sbm_bilinear", s);
    int rc = 0;
    if (gu || gv) {
        const long long tiles = (long long)cdiv(B, BL_MT) * cdiv(F, BL_NT) * N;
        float* part = (float*)workspace;
        hipLaunchKernelGGL(sbm_bilinear_dgrad_kernel, dim3((unsigned)bl_grid(tiles)), dim3(BL_THREADS), 0, s, u, v, w, t_save, gout,
                           gu, gv, part, B, F, N);
        if ((rc = ign_check_launch("sbm_bilinear_dgrad_kernel"))) return rc;
        if (gu && N > 1) {
            const long long BF = (long long)B * F;
            hipLaunchKernelGGL(sbm_bilinear_dgrad_reduce_kernel, dim3(cdiv(BF, BL_THREADS)), dim3(BL_THREADS), 0, s, part, gu, BF, N);
            if ((rc = ign_check_launch("sbm_bilinear_dgrad_reduce_kernel"))) return rc;
        }
    }
    if (gw) {
        const long long tiles = (long long)cdiv(F, BL_MT) * cdiv(F, BL_NT) * N;
        hipLaunchKernelGGL(sbm_bilinear_wgrad_kernel, dim3((unsigned)bl_grid(tiles)), dim3(BL_THREADS), 0, s, u, v, gout, gw, B, F,
                           N);
        rc = ign_check_launch("sbm_bilinear_wgrad_kernel");
    }
    return rc;
}
