// CRPS loss tail of the regression task (IGN/exp/experiment_regression.py:59-76, :159-169) in one launch per loss call.
//
//   p = softmax(z) over N bins, F_j = sum_{i<=j} p_i, H_j = [edge_j >= y] (compared in float64), row loss sum_j (F_j - H_j)^2,
//   loss = batch mean of the row losses.
//   gradient per row: r_j = F_j - H_j; q_i = (2/B) sum_{j>=i} r_j (reverse scan); dz_k = p_k (q_k - sum_i p_i q_i).
//
// InterpGN tail: out = gini_gate(sbm, dnn) with gate_fwd_kernel's arithmetic (bitwise the same out / eta), loss =
// CRPS(out) + reg + beta*CRPS(sbm), and both logit gradients through the gate (the derivative ign_loss_kernel uses).
//
// One block of CRPS_THREADS threads, one thread per row (rows base + threadIdx.x of each tile).  Up to CRPS_NREG classes a
// row lives in registers (loops fully unrolled, guarded by n < N); wider rows are read from global memory and the gradient
// buffer doubles as the row's scratch.  Each row's losses go to LDS at its row index and one thread adds them in ascending
// row order, so the batch mean does not depend on scheduling and two calls are bitwise identical.  No allocation, no host
// sync: the launch can be captured.
#include "ign_common.h"

constexpr int CRPS_THREADS = 1024, CRPS_NREG = 16;

// a row held in registers (NR > 0) or addressed in global memory (NR == 0)
template <int NR> struct RowBuf {
    float v[NR];
    __device__ __forceinline__ float& operator[](int n) { return v[n]; }
};
template <> struct RowBuf<0> {
    float* p;
    __device__ __forceinline__ float& operator[](int n) { return p[n]; }
};

// class loops: fully unrolled over the NR register slots (guarded), or a runtime loop over N
template <int NR> constexpr int kUnroll = NR ? NR : 1;
#define CRPS_FOR(n) _Pragma("unroll kUnroll<NR>") for (int n = 0; n < (NR ? NR : N); ++n) if (NR == 0 || n < N)
#define CRPS_FOR_REV(n) _Pragma("unroll kUnroll<NR>") for (int n = (NR ? NR : N) - 1; n >= 0; --n) if (NR == 0 || n < N)

// Row CRPS of softmax(z) against the step CDF of y; g <- d(batch-mean loss)/dz (2/B folded in).  Returns sum_j (F_j - H_j)^2.
// z and g may not alias.
template <int NR>
__device__ __forceinline__ float crps_row(RowBuf<NR>& z, RowBuf<NR>& g, const double* __restrict__ edges, double y, int N,
                                          float twoInvB) {
    float mx = -INFINITY;
    CRPS_FOR(n) mx = fmaxf(mx, z[n]);
    float Z = 0.f;
    CRPS_FOR(n) Z += expf(z[n] - mx);
    float F = 0.f, sq = 0.f;
    CRPS_FOR(j) {
        F += expf(z[j] - mx) / Z;
        const float r = F - (edges[j] >= y ? 1.f : 0.f);
        sq += r * r;
        g[j] = r;
    }
    float acc = 0.f, dot = 0.f;
    CRPS_FOR_REV(i) {
        acc += g[i];
        const float q = twoInvB * acc;
        g[i] = q;
        dot += (expf(z[i] - mx) / Z) * q;
    }
    CRPS_FOR(k) g[k] = (expf(z[k] - mx) / Z) * (g[k] - dot);
    return sq;
}

template <int NR>
__device__ __forceinline__ void load_row(RowBuf<NR>& r, const float* src, int N) {
    CRPS_FOR(n) r[n] = src[n];
}
template <>
__device__ __forceinline__ void load_row<0>(RowBuf<0>&, const float*, int) {}

template <int NR>
__device__ __forceinline__ void store_row(RowBuf<NR>& r, float* dst, int N) {
    CRPS_FOR(n) dst[n] = r[n];
}
template <>
__device__ __forceinline__ void store_row<0>(RowBuf<0>&, float*, int) {}

// rows of one tile; the caller's LDS `part` receives each row's loss(es) at the row's index, then thread 0 adds them in order
__device__ __forceinline__ void add_in_row_order(const float* part, int rows, float& tot) {
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < rows; ++i) tot += part[i];
    __syncthreads();
}

template <int NR>
__global__ void __launch_bounds__(CRPS_THREADS) crps_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                            const double* __restrict__ edges, float* __restrict__ loss_out,
                                                            float* grad, int B, int N) {
    __shared__ float part[CRPS_THREADS];
    float tot = 0.f;                                   // meaningful in thread 0
    const float invB = 1.f / (float)B, twoInvB = 2.f * invB;
    for (int base = 0; base < B; base += CRPS_THREADS) {
        const int rows = min(CRPS_THREADS, B - base);
        const int b = base + (int)threadIdx.x;
        if (b < B) {
            const long long o = (long long)b * N;
            RowBuf<NR> z, g;
            if constexpr (NR == 0) {
                z.p = const_cast<float*>(logits + o);
                g.p = grad + o;
            }
            load_row<NR>(z, logits + o, N);
            part[threadIdx.x] = crps_row<NR>(z, g, edges, (double)target[b], N, twoInvB);
            store_row<NR>(g, grad + o, N);
        }
        add_in_row_order(part, rows, tot);
    }
    if (threadIdx.x == 0) loss_out[0] = tot * invB;
}

template <int NR>
__global__ void __launch_bounds__(CRPS_THREADS) ign_crps_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                                const float* __restrict__ target, const double* __restrict__ edges,
                                                                const float* __restrict__ reg, float* out, float* __restrict__ eta_out,
                                                                float* __restrict__ loss3, float* gs, float* gd, int B, int N,
                                                                float beta) {
    __shared__ float part[2][CRPS_THREADS];
    float tot_o = 0.f, tot_s = 0.f;
    const float invB = 1.f / (float)B, twoInvB = 2.f * invB;
    for (int base = 0; base < B; base += CRPS_THREADS) {
        const int rows = min(CRPS_THREADS, B - base);
        const int b = base + (int)threadIdx.x;
        if (b < B) {
            const long long o = (long long)b * N;
            const float* sr = s + o;
            const float* dr = d + o;
            RowBuf<NR> sv, ov, go, gsv;
            if constexpr (NR == 0) {
                sv.p = const_cast<float*>(sr);
                ov.p = out + o;
                go.p = gd + o;
                gsv.p = gs + o;
            }
            load_row<NR>(sv, sr, N);
            // gini gate: gate_fwd_kernel's arithmetic, in the same order
            float mx = -INFINITY;
            CRPS_FOR(n) mx = fmaxf(mx, sv[n]);
            float z = 0.f, z2 = 0.f;
            CRPS_FOR(n) {
                const float e = expf(sv[n] - mx);
                z += e;
                z2 += e * e;
            }
            const float eta = ((float)N * (z2 / (z * z)) - 1.f) / (float)(N - 1);
            eta_out[b] = eta;
            CRPS_FOR(n) ov[n] = eta * sv[n] + (1.f - eta) * dr[n];
            store_row<NR>(ov, out + o, N);
            const double y = (double)target[b];
            part[0][threadIdx.x] = crps_row<NR>(ov, go, edges, y, N, twoInvB);      // go = dCRPS(out)/dout
            part[1][threadIdx.x] = crps_row<NR>(sv, gsv, edges, y, N, twoInvB);     // gsv = dCRPS(sbm)/dsbm
            // through the gate (gate_bwd_kernel / ign_loss_kernel): ds = eta*go + c*q*(q - G) + beta*gsv, dd = (1 - eta)*go
            const float G = z2 / (z * z);
            float dot = 0.f;
            CRPS_FOR(n) dot += go[n] * (sv[n] - dr[n]);
            const float c = 2.f * (float)N / (float)(N - 1) * dot;
            CRPS_FOR(n) {
                const float qn = expf(sv[n] - mx) / z;
                const float g_o = go[n];
                gs[o + n] = eta * g_o + c * qn * (qn - G) + beta * gsv[n];
                gd[o + n] = (1.f - eta) * g_o;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < rows; ++i) { tot_o += part[0][i]; tot_s += part[1][i]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss3[0] = tot_o * invB;
        loss3[1] = tot_s * invB;
        loss3[2] = tot_o * invB + beta * (tot_s * invB) + (reg ? reg[0] : 0.f);     // + info.loss.mean()
    }
}

#undef CRPS_FOR
#undef CRPS_FOR_REV

static bool crps_dims_ok(const char* name, int B, int N) {
    if (B <= 0 || N < 2 || N > IGN_HEAD_NMAX) {
        ign_set_error("%s: bad dimension (B=%d N=%d; B >= 1, 2 <= N <= %d)", name, B, N, IGN_HEAD_NMAX);
        return false;
    }
    return true;
}

extern "C" int ign_crps_fwd_bwd(const float* logits, const float* target, const double* edges, float* loss_out, float* grad,
                                int B, int N, void* stream) {
    if (!logits || !target || !edges || !loss_out || !grad) {
        ign_set_error("ign_crps_fwd_bwd: null pointer");
        return IGN_E_ARG;
    }
    if (!crps_dims_ok("ign_crps_fwd_bwd", B, N)) return IGN_E_ARG;
    if (N <= CRPS_NREG) {
        hipLaunchKernelGGL(crps_kernel<CRPS_NREG>, dim3(1), dim3(CRPS_THREADS), 0, (hipStream_t)stream, logits, target, edges,
                           loss_out, grad, B, N);
        return ign_check_launch("crps_kernel");
    }
    hipLaunchKernelGGL(crps_kernel<0>, dim3(1), dim3(CRPS_THREADS), 0, (hipStream_t)stream, logits, target, edges, loss_out, grad,
                       B, N);
    return ign_check_launch("crps_kernel");
}

extern "C" int ign_loss_crps_fwd_bwd_reg(const float* sbm, const float* dnn, const float* target, const double* edges,
                                         const float* reg, float* out, float* eta, float* loss3, float* gsbm, float* gdnn, int B,
                                         int N, float beta, void* stream) {
    if (!sbm || !dnn || !target || !edges || !out || !eta || !loss3 || !gsbm || !gdnn) {
        ign_set_error("ign_loss_crps_fwd_bwd_reg: null pointer");
        return IGN_E_ARG;
    }
    if (!crps_dims_ok("ign_loss_crps_fwd_bwd_reg", B, N)) return IGN_E_ARG;
    if (N <= CRPS_NREG) {
        hipLaunchKernelGGL(ign_crps_kernel<CRPS_NREG>, dim3(1), dim3(CRPS_THREADS), 0, (hipStream_t)stream, sbm, dnn, target, edges,
                           reg, out, eta, loss3, gsbm, gdnn, B, N, beta);
        return ign_check_launch("ign_crps_kernel");
    }
    hipLaunchKernelGGL(ign_crps_kernel<0>, dim3(1), dim3(CRPS_THREADS), 0, (hipStream_t)stream, sbm, dnn, target, edges, reg, out,
                       eta, loss3, gsbm, gdnn, B, N, beta);
    return ign_check_launch("ign_crps_kernel");
}
