// The loss tail of the training step, one launch per call, single-block kernels of a few microseconds: the gini gate
// (IGN/model/InterpGN.py:44-52), the fused classification tail (IGN/exp/experiment_classification.py:320-329) and the CRPS tails of
// the regression task (IGN/exp/experiment_regression.py:59-76, :159-169).
//  * gini gate  q = softmax(s); G = sum q^2; eta = (N G - 1)/(N-1); [eta > gating_value -> 1]; out = eta s + (1 - eta) d
//    backward   d eta / d s_j = (2N/(N-1)) q_j (q_j - G); ds = eta*gout + (sum_n gout_n (s_n - d_n)) * deta/ds; dd = (1 - eta)*gout
//    Written ONCE, in the gate_* helpers, for every kernel of this file: the fused tails' mixture and eta are bitwise ign_gate_fwd's
//    because they are the same source expressions (-ffp-contract=off).  A helper must keep its operation order and association.
//  * CE tail    loss = CE(gate(s, d), y) + beta*CE(s, y) [+ reg] (batch means) and both logit gradients: one thread per row up to
//    16 classes (ign_loss_kernel), one wave per row above (ign_loss_wide_kernel).  With class weights and / or label smoothing:
//    ign_loss_w_kernel / ign_loss_w_wide_kernel, the same two layouts behind an entry point of their own.  With two labels per
//    row and a per-row share of the first (mixup / CutMix, run.py --mix): ign_loss_mix_kernel / ign_loss_mix_wide_kernel.
//  * CRPS       p = softmax(z), F_j = sum_{i<=j} p_i, H_j = [edge_j >= y] (in float64); loss = mean_b sum_j (F_j - H_j)^2; per row
//    r_j = F_j - H_j, q_i = (2/B) sum_{j>=i} r_j, dz_k = p_k (q_k - sum_i p_i q_i).  InterpGN's tail: CRPS in place of CE above.
// The tails stay separate kernels: ign_loss_kernel adds the row terms per thread (rows t, t + 256, ...) and then over the threads,
// the others in ascending row order, and the wide kernel's row sums are butterflies -- different roundings, so merging changes bits.
#include "ign_common.h"

// ------------------------------------------------------------------------------------------------ the gate rule
__device__ __forceinline__ float gate_G(float z, float z2) { return z2 / (z * z); }         // sum softmax^2 from sum e, sum e^2
__device__ __forceinline__ float gate_eta(int N, float G) { return ((float)N * G - 1.f) / (float)(N - 1); }
// the test-time `gating_value`: eta above it snaps to 1 (the hard branch; it has no gradient through eta)
__device__ __forceinline__ bool gate_snap(float& eta, float thr, int use_thr) {
    const bool hard = use_thr && eta > thr;
    if (hard) eta = 1.f;
    return hard;
}
__device__ __forceinline__ float gate_mix(float eta, float s, float d) { return eta * s + (1.f - eta) * d; }
// c of d eta/d s_j * dot = c q_j (q_j - G), with dot = sum_n gout_n (s_n - d_n) [+ geta]
__device__ __forceinline__ float gate_coef(int N, float dot) { return 2.f * (float)N / (float)(N - 1) * dot; }
__device__ __forceinline__ float gate_ds(float eta, float go, float c, float q, float G) { return eta * go + c * q * (q - G); }
__device__ __forceinline__ float gate_dd(float eta, float go) { return (1.f - eta) * go; }

// ------------------------------------------------------------------------------------------------ rows
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
#define ROW_FOR(n) _Pragma("unroll kUnroll<NR>") for (int n = 0; n < (NR ? NR : N); ++n) if (NR == 0 || n < N)
#define ROW_FOR_REV(n) _Pragma("unroll kUnroll<NR>") for (int n = (NR ? NR : N) - 1; n >= 0; --n) if (NR == 0 || n < N)

// Softmax statistics of a row its thread holds whole (a RowBuf, a register array or a pointer): the max, then z = sum e and
// z2 = sum e^2 in class order, e_n = exp(row_n - max); `e` (nullable) keeps the e_n.
template <int NR, class Row>
__device__ __forceinline__ void row_stats(Row& row, int N, float& mx, float& z, float& z2, float* e = nullptr) {
    mx = -INFINITY;
    ROW_FOR(n) mx = fmaxf(mx, row[n]);
    z = z2 = 0.f;
    ROW_FOR(n) {
        const float en = expf(row[n] - mx);
        if (e) e[n] = en;
        z += en;
        z2 += en * en;
    }
}

template <int NR>
__device__ __forceinline__ void load_row(RowBuf<NR>& r, const float* src, int N) {
    ROW_FOR(n) r[n] = src[n];
}
template <>
__device__ __forceinline__ void load_row<0>(RowBuf<0>&, const float*, int) {}

template <int NR>
__device__ __forceinline__ void store_row(RowBuf<NR>& r, float* dst, int N) {
    ROW_FOR(n) dst[n] = r[n];
}
template <>
__device__ __forceinline__ void store_row<0>(RowBuf<0>&, float*, int) {}

// ------------------------------------------------------------------------------------------------ batch means
// rows of one tile: the caller's LDS `part` received each row's K loss terms at the row's index, thread 0 adds them in ascending row
// order into its `tot` -- the batch mean does not depend on scheduling and two calls are bitwise identical
template <int K, int P>
__device__ __forceinline__ void add_in_row_order(const float (&part)[K][P], int rows, float (&tot)[K]) {
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < rows; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) tot[k] += part[k][i];
    __syncthreads();
}

// what a gated tail reports, from the batch sums of its two criteria: {crit(out), crit(sbm), crit(out) + beta*crit(sbm) + reg}
// (`reg` nullable: + info.loss.mean(), exp:325-329)
__device__ __forceinline__ void write_loss3(float* __restrict__ loss3, float sum_o, float sum_s, float invB, float beta,
                                            const float* __restrict__ reg) {
    loss3[0] = sum_o * invB;
    loss3[1] = sum_s * invB;
    loss3[2] = sum_o * invB + beta * (sum_s * invB) + (reg ? reg[0] : 0.f);
}

// ------------------------------------------------------------------------------------------------ gini gate
__global__ void __launch_bounds__(256) gate_fwd_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                       float* __restrict__ out, float* __restrict__ eta_out, int B, int N,
                                                       float thr, int use_thr) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float* sr = s + (long long)b * N;
    float mx, z, z2;
    row_stats<0>(sr, N, mx, z, z2);
    float eta = gate_eta(N, gate_G(z, z2));
    gate_snap(eta, thr, use_thr);
    eta_out[b] = eta;
    for (int n = 0; n < N; ++n) out[(long long)b * N + n] = gate_mix(eta, sr[n], d[(long long)b * N + n]);
}

__global__ void __launch_bounds__(256) gate_bwd_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                       const float* __restrict__ gout, const float* __restrict__ geta,
                                                       float* __restrict__ gs, float* __restrict__ gd, int B, int N,
                                                       float thr, int use_thr) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float* sr = s + (long long)b * N;
    const float* dr = d + (long long)b * N;
    const float* gr = gout + (long long)b * N;
    float mx, z, z2;
    row_stats<0>(sr, N, mx, z, z2);
    float dot = geta ? geta[b] : 0.f;
    for (int n = 0; n < N; ++n) dot += gr[n] * (sr[n] - dr[n]);
    const float G = gate_G(z, z2);
    float eta = gate_eta(N, G);
    float c = gate_coef(N, dot);
    if (gate_snap(eta, thr, use_thr)) c = 0.f;
    for (int n = 0; n < N; ++n) {
        const float q = expf(sr[n] - mx) / z;
        gs[(long long)b * N + n] = gate_ds(eta, gr[n], c, q, G);
        gd[(long long)b * N + n] = gate_dd(eta, gr[n]);
    }
}

// ------------------------------------------------------------------------------------------------ fused training-loss tail
// IGN's per-step loss tail, IGN/exp/experiment_classification.py:320-329 + IGN/model/InterpGN.py:44-52, in ONE launch:
//   out = eta*s + (1-eta)*d (gini gate);  loss = CE(out, y) + beta*CE(s, y)  (batch means);  and the gradients of that
//   loss w.r.t. both experts' logits -- what torch spends ~40 softmax / nll / mean / add kernels (forward + backward) on,
//   all of them serialised between the last forward kernel and the first backward kernel.
// One block; thread <-> rows b, b+256, ...; the two CE sums are reduced through LDS in thread order (deterministic).
constexpr int LOSS_NMAX = 16;
__global__ void __launch_bounds__(256) ign_loss_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                       const long long* __restrict__ y, float* __restrict__ out,
                                                       float* __restrict__ eta_out, float* __restrict__ loss2,
                                                       float* __restrict__ gs, float* __restrict__ gd, int B, int N, float beta,
                                                       const float* __restrict__ reg) {
    __shared__ float red[2][256];
    float ce_o = 0.f, ce_s = 0.f;
    const float invB = 1.f / (float)B;
    for (int b = threadIdx.x; b < B; b += 256) {
        float sv[LOSS_NMAX], ov[LOSS_NMAX], q[LOSS_NMAX];
        const float* sr = s + (long long)b * N;
        const float* dr = d + (long long)b * N;
        const int yb = (int)y[b];
        for (int n = 0; n < N; ++n) sv[n] = sr[n];
        float mx, z, z2;
        row_stats<0>(sv, N, mx, z, z2, q);
        const float G = gate_G(z, z2);
        const float eta = gate_eta(N, G);
        eta_out[b] = eta;
        const float lse_s = mx + logf(z);
        ce_s += lse_s - sv[yb];
        float mo = -INFINITY;
        for (int n = 0; n < N; ++n) {
            ov[n] = gate_mix(eta, sv[n], dr[n]);
            out[(long long)b * N + n] = ov[n];
            mo = fmaxf(mo, ov[n]);
        }
        float zo = 0.f;
        for (int n = 0; n < N; ++n) zo += expf(ov[n] - mo);
        ce_o += mo + logf(zo) - ov[yb];
        // gradients: g_out = (softmax(out) - onehot)/B ; through the gate ; + beta*(softmax(s) - onehot)/B
        float dot = 0.f;
        float go[LOSS_NMAX];
        for (int n = 0; n < N; ++n) {
            go[n] = (expf(ov[n] - mo) / zo - (n == yb ? 1.f : 0.f)) * invB;
            dot += go[n] * (sv[n] - dr[n]);
        }
        const float c = gate_coef(N, dot);
        for (int n = 0; n < N; ++n) {
            const float qn = q[n] / z;
            gs[(long long)b * N + n] = gate_ds(eta, go[n], c, qn, G) + beta * (qn - (n == yb ? 1.f : 0.f)) * invB;
            gd[(long long)b * N + n] = gate_dd(eta, go[n]);
        }
    }
    red[0][threadIdx.x] = ce_o;
    red[1][threadIdx.x] = ce_s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b2 = 0.f;
        for (int i = 0; i < 256; ++i) { a += red[0][i]; b2 += red[1][i]; }
        write_loss3(loss2, a, b2, invB, beta, reg);
    }
}

// The same loss tail for 16 < N <= IGN_HEAD_NMAX: one block of 16 waves, one wave per row (rows w, w + 16, ...), the lanes cover
// the classes in chunks of 64 and every row-wide max / sum is a butterfly over the wave (each lane ends with the same value), so
// its sums are not bitwise ign_loss_kernel's or the gate kernels'.  Each row's two CE terms go to LDS at their row index; one
// thread adds them in ascending row order (LOSS_TILE rows at a time), so the batch mean does not depend on how the waves were
// scheduled.
constexpr int LOSS_WAVES = 16, LOSS_TILE = 1024, LOSS_KMAX = IGN_HEAD_NMAX / 64;
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ void __launch_bounds__(LOSS_WAVES * 64) ign_loss_wide_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                                        const long long* __restrict__ y, float* __restrict__ out,
                                                                        float* __restrict__ eta_out, float* __restrict__ loss2,
                                                                        float* __restrict__ gs, float* __restrict__ gd, int B, int N,
                                                                        float beta, const float* __restrict__ reg) {
    __shared__ float ce[2][LOSS_TILE];
    float tot[2] = {0.f, 0.f};                         // {CE(out), CE(s)} batch sums, meaningful in thread 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float invB = 1.f / (float)B;
    for (int base = 0; base < B; base += LOSS_TILE) {
        const int rows = min(LOSS_TILE, B - base);
        for (int r = wave; r < rows; r += LOSS_WAVES) {
            const int b = base + r;
            const float* sr = s + (long long)b * N;
            const float* dr = d + (long long)b * N;
            const int yb = (int)y[b];
            float sv[LOSS_KMAX], dv[LOSS_KMAX], q[LOSS_KMAX], ov[LOSS_KMAX], eo[LOSS_KMAX];
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                const int n = k * 64 + lane;
                sv[k] = n < N ? sr[n] : -INFINITY;
                dv[k] = n < N ? dr[n] : 0.f;
                mx = fmaxf(mx, sv[k]);
            }
            mx = wave_max(mx);
            float z = 0.f, z2 = 0.f;
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                q[k] = k * 64 + lane < N ? expf(sv[k] - mx) : 0.f;
                z += q[k];
                z2 += q[k] * q[k];
            }
            z = wave_sum(z);
            z2 = wave_sum(z2);
            const float G = gate_G(z, z2);
            const float eta = gate_eta(N, G);
            if (lane == 0) eta_out[b] = eta;
            float mo = -INFINITY, s_y = 0.f, o_y = 0.f;
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                const int n = k * 64 + lane;
                ov[k] = gate_mix(eta, sv[k], dv[k]);
                if (n < N) {
                    out[(long long)b * N + n] = ov[k];
                    mo = fmaxf(mo, ov[k]);
                }
                if (n == yb) { s_y = sv[k]; o_y = ov[k]; }
            }
            mo = wave_max(mo);
            s_y = wave_sum(s_y);                  // exactly one lane holds the label's logits, the others add zeros
            o_y = wave_sum(o_y);
            float zo = 0.f;
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                eo[k] = k * 64 + lane < N ? expf(ov[k] - mo) : 0.f;
                zo += eo[k];
            }
            zo = wave_sum(zo);
            // gradients: g_out = (softmax(out) - onehot)/B ; through the gate ; + beta*(softmax(s) - onehot)/B
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                const int n = k * 64 + lane;
                eo[k] = (eo[k] / zo - (n == yb ? 1.f : 0.f)) * invB;          // go
                if (n < N) dot += eo[k] * (sv[k] - dv[k]);
            }
            dot = wave_sum(dot);
            const float c = gate_coef(N, dot);
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                const int n = k * 64 + lane;
                if (n < N) {
                    const float qn = q[k] / z;
                    gs[(long long)b * N + n] = gate_ds(eta, eo[k], c, qn, G) + beta * (qn - (n == yb ? 1.f : 0.f)) * invB;
                    gd[(long long)b * N + n] = gate_dd(eta, eo[k]);
                }
            }
            if (lane == 0) {
                ce[0][r] = mo + logf(zo) - o_y;
                ce[1][r] = mx + logf(z) - s_y;
            }
        }
        add_in_row_order(ce, rows, tot);
    }
    if (threadIdx.x == 0) write_loss3(loss2, tot[0], tot[1], invB, beta, reg);
}

// ------------------------------------------------------------------------------------------------ weighted, label-smoothed CE tail
// The same tail under F.cross_entropy(z, y, weight=w, label_smoothing=eps, reduction='mean'), for both criteria.  With p = softmax(z),
// D = sum_b w[y_b], W = sum_n w_n:
//   CEw        = sum_b [ (1-eps) w[y_b] (lse_b - z[b,y_b]) + (eps/N) sum_n w_n (lse_b - z[b,n]) ] / D
//   dCEw/dz_bn = ( (1-eps) w[y_b] (p_n - [n = y_b]) + (eps/N) (p_n W - w_n) ) / D
// Separate kernels, so the unweighted ones above keep their bits; the gate is the same gate_* expressions in the same order.
// D and W come from a pre-pass inside the launch (cew_prepass): no atomics, the same bits every call.
struct CeW {
    float keep, smooth, W, invD;       // 1 - eps, eps/N, sum_n w_n, 1 / sum_b w[y_b]
};
__device__ __forceinline__ int cew_label(long long y, int N) { return (int)(y < 0 ? 0 : y >= N ? N - 1 : y); }   // device data: clamped
// one logit's gradient; wy = w[y_b], wn = w_n, hit = [n == y_b]
__device__ __forceinline__ float cew_grad(const CeW& k, float wy, float p, float wn, bool hit) {
    return (k.keep * wy * (p - (hit ? 1.f : 0.f)) + k.smooth * (p * k.W - wn)) * k.invD;
}
// one row's loss term before the division by D; nll = lse - z_y, smo = sum_n w_n (lse - z_n)
__device__ __forceinline__ float cew_term(const CeW& k, float wy, float nll, float smo) { return k.keep * wy * nll + k.smooth * smo; }

// Stages the class weights (null = ones) in the caller's LDS `wl` and returns {1 - eps, eps/N, W, 1/D} to every thread.  W is summed
// in class order; D per thread over its rows t, t + blockDim, ... in ascending order, then over the threads in thread order (`red`:
// blockDim floats of LDS, free again on return).
__device__ __forceinline__ CeW cew_prepass(const float* __restrict__ cw, const long long* __restrict__ y, int B, int N, float eps,
                                           float* wl, float* red) {
    __shared__ float dw[2];
    const int T = (int)blockDim.x;
    for (int n = threadIdx.x; n < N; n += T) wl[n] = cw ? cw[n] : 1.f;
    __syncthreads();
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += T) part += wl[cew_label(y[b], N)];
    red[threadIdx.x] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        float D = 0.f, W = 0.f;
        for (int i = 0; i < min(T, B); ++i) D += red[i];               // threads past the last row hold zeros
        for (int n = 0; n < N; ++n) W += wl[n];
        dw[0] = D;
        dw[1] = W;
    }
    __syncthreads();
    return CeW{1.f - eps, eps / (float)N, dw[1], 1.f / dw[0]};
}

// N <= 16: ign_loss_kernel's layout (thread <-> rows b, b + 256, ...; the two sums reduced through LDS in thread order)
__global__ void __launch_bounds__(256) ign_loss_w_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                         const long long* __restrict__ y, const float* __restrict__ cw,
                                                         float* __restrict__ out, float* __restrict__ eta_out,
                                                         float* __restrict__ loss3, float* __restrict__ gs, float* __restrict__ gd,
                                                         int B, int N, float beta, float eps, const float* __restrict__ reg) {
    __shared__ float red[2][256];
    __shared__ float wl[LOSS_NMAX];
    const CeW k = cew_prepass(cw, y, B, N, eps, wl, red[0]);
    float ce_o = 0.f, ce_s = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        float sv[LOSS_NMAX], ov[LOSS_NMAX], q[LOSS_NMAX];
        const float* sr = s + (long long)b * N;
        const float* dr = d + (long long)b * N;
        const int yb = cew_label(y[b], N);
        const float wy = wl[yb];
        for (int n = 0; n < N; ++n) sv[n] = sr[n];
        float mx, z, z2;
        row_stats<0>(sv, N, mx, z, z2, q);
        const float G = gate_G(z, z2);
        const float eta = gate_eta(N, G);
        eta_out[b] = eta;
        const float lse_s = mx + logf(z);
        float mo = -INFINITY;
        for (int n = 0; n < N; ++n) {
            ov[n] = gate_mix(eta, sv[n], dr[n]);
            out[(long long)b * N + n] = ov[n];
            mo = fmaxf(mo, ov[n]);
        }
        float zo = 0.f;
        for (int n = 0; n < N; ++n) zo += expf(ov[n] - mo);
        const float lse_o = mo + logf(zo);
        float smo_s = 0.f, smo_o = 0.f;
        for (int n = 0; n < N; ++n) {
            smo_s += wl[n] * (lse_s - sv[n]);
            smo_o += wl[n] * (lse_o - ov[n]);
        }
        ce_s += cew_term(k, wy, lse_s - sv[yb], smo_s);
        ce_o += cew_term(k, wy, lse_o - ov[yb], smo_o);
        // gradients: g_out = dCEw(out)/dout ; through the gate ; + beta * dCEw(s)/ds
        float dot = 0.f;
        float go[LOSS_NMAX];
        for (int n = 0; n < N; ++n) {
            go[n] = cew_grad(k, wy, expf(ov[n] - mo) / zo, wl[n], n == yb);
            dot += go[n] * (sv[n] - dr[n]);
        }
        const float c = gate_coef(N, dot);
        for (int n = 0; n < N; ++n) {
            const float qn = q[n] / z;
            gs[(long long)b * N + n] = gate_ds(eta, go[n], c, qn, G) + beta * cew_grad(k, wy, qn, wl[n], n == yb);
            gd[(long long)b * N + n] = gate_dd(eta, go[n]);
        }
    }
    red[0][threadIdx.x] = ce_o;
    red[1][threadIdx.x] = ce_s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b2 = 0.f;
        for (int i = 0; i < 256; ++i) { a += red[0][i]; b2 += red[1][i]; }
        write_loss3(loss3, a, b2, k.invD, beta, reg);
    }
}

// 16 < N <= IGN_HEAD_NMAX: ign_loss_wide_kernel's layout (one wave per row, lanes over the classes in chunks of 64, row sums by
// butterfly, the rows' loss terms added in ascending row order)
__global__ void __launch_bounds__(LOSS_WAVES * 64) ign_loss_w_wide_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                                          const long long* __restrict__ y,
                                                                          const float* __restrict__ cw, float* __restrict__ out,
                                                                          float* __restrict__ eta_out, float* __restrict__ loss3,
                                                                          float* __restrict__ gs, float* __restrict__ gd, int B, int N,
                                                                          float beta, float eps, const float* __restrict__ reg) {
    __shared__ float ce[2][LOSS_TILE];
    __shared__ float wl[IGN_HEAD_NMAX];
    static_assert(LOSS_TILE >= LOSS_WAVES * 64, "cew_prepass borrows one row of `ce` for its per-thread sums");
    const CeW k = cew_prepass(cw, y, B, N, eps, wl, ce[0]);
    float tot[2] = {0.f, 0.f};                         // {CEw(out), CEw(s)} batch sums before / D, meaningful in thread 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < B; base += LOSS_TILE) {
        const int rows = min(LOSS_TILE, B - base);
        for (int r = wave; r < rows; r += LOSS_WAVES) {
            const int b = base + r;
            const float* sr = s + (long long)b * N;
            const float* dr = d + (long long)b * N;
            const int yb = cew_label(y[b], N);
            const float wy = wl[yb];
            float sv[LOSS_KMAX], dv[LOSS_KMAX], q[LOSS_KMAX], ov[LOSS_KMAX], eo[LOSS_KMAX], wv[LOSS_KMAX];
            float mx = -INFINITY;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                const int n = kk * 64 + lane;
                sv[kk] = n < N ? sr[n] : -INFINITY;
                dv[kk] = n < N ? dr[n] : 0.f;
                wv[kk] = n < N ? wl[n] : 0.f;
                mx = fmaxf(mx, sv[kk]);
            }
            mx = wave_max(mx);
            float z = 0.f, z2 = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                q[kk] = kk * 64 + lane < N ? expf(sv[kk] - mx) : 0.f;
                z += q[kk];
                z2 += q[kk] * q[kk];
            }
            z = wave_sum(z);
            z2 = wave_sum(z2);
            const float G = gate_G(z, z2);
            const float eta = gate_eta(N, G);
            if (lane == 0) eta_out[b] = eta;
            float mo = -INFINITY, s_y = 0.f, o_y = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                const int n = kk * 64 + lane;
                ov[kk] = gate_mix(eta, sv[kk], dv[kk]);
                if (n < N) {
                    out[(long long)b * N + n] = ov[kk];
                    mo = fmaxf(mo, ov[kk]);
                }
                if (n == yb) { s_y = sv[kk]; o_y = ov[kk]; }
            }
            mo = wave_max(mo);
            s_y = wave_sum(s_y);                  // exactly one lane holds the label's logits, the others add zeros
            o_y = wave_sum(o_y);
            float zo = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                eo[kk] = kk * 64 + lane < N ? expf(ov[kk] - mo) : 0.f;
                zo += eo[kk];
            }
            zo = wave_sum(zo);
            const float lse_s = mx + logf(z), lse_o = mo + logf(zo);
            float smo_s = 0.f, smo_o = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk)
                if (kk * 64 + lane < N) {         // the padding lanes hold -inf logits
                    smo_s += wv[kk] * (lse_s - sv[kk]);
                    smo_o += wv[kk] * (lse_o - ov[kk]);
                }
            smo_s = wave_sum(smo_s);
            smo_o = wave_sum(smo_o);
            // gradients: g_out = dCEw(out)/dout ; through the gate ; + beta * dCEw(s)/ds
            float dot = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                const int n = kk * 64 + lane;
                eo[kk] = cew_grad(k, wy, eo[kk] / zo, wv[kk], n == yb);          // go
                if (n < N) dot += eo[kk] * (sv[kk] - dv[kk]);
            }
            dot = wave_sum(dot);
            const float c = gate_coef(N, dot);
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                const int n = kk * 64 + lane;
                if (n < N) {
                    const float qn = q[kk] / z;
                    gs[(long long)b * N + n] = gate_ds(eta, eo[kk], c, qn, G) + beta * cew_grad(k, wy, qn, wv[kk], n == yb);
                    gd[(long long)b * N + n] = gate_dd(eta, eo[kk]);
                }
            }
            if (lane == 0) {
                ce[0][r] = cew_term(k, wy, lse_o - o_y, smo_o);
                ce[1][r] = cew_term(k, wy, lse_s - s_y, smo_s);
            }
        }
        add_in_row_order(ce, rows, tot);
    }
    if (threadIdx.x == 0) write_loss3(loss3, tot[0], tot[1], k.invD, beta, reg);
}

// ------------------------------------------------------------------------------------------------ soft-label (mixup / CutMix) CE tail
// The weighted tail with two labels per row, ya_b and yb_b, and the share lam_b of the first (run.py --mix).  With a_b = lam_b w[ya_b],
// c_b = (1 - lam_b) w[yb_b], D = sum_b (a_b + c_b), W = sum_n w_n:
//   CEm        = sum_b [ (1-eps) (a_b (lse_b - z[b,ya_b]) + c_b (lse_b - z[b,yb_b])) + (eps/N) sum_n w_n (lse_b - z[b,n]) ] / D
//   dCEm/dz_bn = ( (1-eps) (a_b (p_n - [n = ya_b]) + c_b (p_n - [n = yb_b])) + (eps/N) (p_n W - w_n) ) / D
// lam == 1 everywhere is CEw.  Separate kernels again, so the tails above keep their bits; the gate is the same gate_* expressions
// in the same order, the two layouts are those of ign_loss_w_kernel / ign_loss_w_wide_kernel, and D and W come from a pre-pass
// inside the launch (cem_prepass), summed in cew_prepass's order.
struct CeMRow {
    int ya, yb;
    float a, c;                        // lam w[ya], (1 - lam) w[yb]
};
__device__ __forceinline__ float cem_lam(float lam) { return fminf(fmaxf(lam, 0.f), 1.f); }   // device data: clamped (NaN -> 0)
__device__ __forceinline__ CeMRow cem_row(const long long* __restrict__ ya, const long long* __restrict__ yb,
                                          const float* __restrict__ lam, int b, int N, const float* wl) {
    CeMRow r;
    r.ya = cew_label(ya[b], N);
    r.yb = cew_label(yb[b], N);
    const float l = cem_lam(lam[b]);
    r.a = l * wl[r.ya];
    r.c = (1.f - l) * wl[r.yb];
    return r;
}
__device__ __forceinline__ float cem_grad(const CeW& k, const CeMRow& r, float p, float wn, int n) {
    return (k.keep * (r.a * (p - (n == r.ya ? 1.f : 0.f)) + r.c * (p - (n == r.yb ? 1.f : 0.f))) + k.smooth * (p * k.W - wn)) * k.invD;
}
// one row's loss term before the division by D; nll_a = lse - z_ya, nll_b = lse - z_yb, smo = sum_n w_n (lse - z_n)
__device__ __forceinline__ float cem_term(const CeW& k, const CeMRow& r, float nll_a, float nll_b, float smo) {
    return k.keep * (r.a * nll_a + r.c * nll_b) + k.smooth * smo;
}

// cew_prepass with D = sum_b (a_b + c_b): per thread over its rows t, t + blockDim, ... in ascending order, then over the threads in
// thread order; W in class order.  `red`: blockDim floats of LDS, free again on return.
__device__ __forceinline__ CeW cem_prepass(const float* __restrict__ cw, const long long* __restrict__ ya,
                                           const long long* __restrict__ yb, const float* __restrict__ lam, int B, int N, float eps,
                                           float* wl, float* red) {
    __shared__ float dw[2];
    const int T = (int)blockDim.x;
    for (int n = threadIdx.x; n < N; n += T) wl[n] = cw ? cw[n] : 1.f;
    __syncthreads();
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += T) {
        const CeMRow r = cem_row(ya, yb, lam, b, N, wl);
        part += r.a + r.c;
    }
    red[threadIdx.x] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        float D = 0.f, W = 0.f;
        for (int i = 0; i < min(T, B); ++i) D += red[i];               // threads past the last row hold zeros
        for (int n = 0; n < N; ++n) W += wl[n];
        dw[0] = D;
        dw[1] = W;
    }
    __syncthreads();
    return CeW{1.f - eps, eps / (float)N, dw[1], 1.f / dw[0]};
}

// N <= 16: ign_loss_kernel's layout (thread <-> rows b, b + 256, ...; the two sums reduced through LDS in thread order)
__global__ void __launch_bounds__(256) ign_loss_mix_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                           const long long* __restrict__ ya, const long long* __restrict__ yb,
                                                           const float* __restrict__ lam, const float* __restrict__ cw,
                                                           float* __restrict__ out, float* __restrict__ eta_out,
                                                           float* __restrict__ loss3, float* __restrict__ gs, float* __restrict__ gd,
                                                           int B, int N, float beta, float eps, const float* __restrict__ reg) {
    __shared__ float red[2][256];
    __shared__ float wl[LOSS_NMAX];
    const CeW k = cem_prepass(cw, ya, yb, lam, B, N, eps, wl, red[0]);
    float ce_o = 0.f, ce_s = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        float sv[LOSS_NMAX], ov[LOSS_NMAX], q[LOSS_NMAX];
        const float* sr = s + (long long)b * N;
        const float* dr = d + (long long)b * N;
        const CeMRow r = cem_row(ya, yb, lam, b, N, wl);
        for (int n = 0; n < N; ++n) sv[n] = sr[n];
        float mx, z, z2;
        row_stats<0>(sv, N, mx, z, z2, q);
        const float G = gate_G(z, z2);
        const float eta = gate_eta(N, G);
        eta_out[b] = eta;
        const float lse_s = mx + logf(z);
        float mo = -INFINITY;
        for (int n = 0; n < N; ++n) {
            ov[n] = gate_mix(eta, sv[n], dr[n]);
            out[(long long)b * N + n] = ov[n];
            mo = fmaxf(mo, ov[n]);
        }
        float zo = 0.f;
        for (int n = 0; n < N; ++n) zo += expf(ov[n] - mo);
        const float lse_o = mo + logf(zo);
        float smo_s = 0.f, smo_o = 0.f;
        for (int n = 0; n < N; ++n) {
            smo_s += wl[n] * (lse_s - sv[n]);
            smo_o += wl[n] * (lse_o - ov[n]);
        }
        ce_s += cem_term(k, r, lse_s - sv[r.ya], lse_s - sv[r.yb], smo_s);
        ce_o += cem_term(k, r, lse_o - ov[r.ya], lse_o - ov[r.yb], smo_o);
        // gradients: g_out = dCEm(out)/dout ; through the gate ; + beta * dCEm(s)/ds
        float dot = 0.f;
        float go[LOSS_NMAX];
        for (int n = 0; n < N; ++n) {
            go[n] = cem_grad(k, r, expf(ov[n] - mo) / zo, wl[n], n);
            dot += go[n] * (sv[n] - dr[n]);
        }
        const float c = gate_coef(N, dot);
        for (int n = 0; n < N; ++n) {
            const float qn = q[n] / z;
            gs[(long long)b * N + n] = gate_ds(eta, go[n], c, qn, G) + beta * cem_grad(k, r, qn, wl[n], n);
            gd[(long long)b * N + n] = gate_dd(eta, go[n]);
        }
    }
    red[0][threadIdx.x] = ce_o;
    red[1][threadIdx.x] = ce_s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b2 = 0.f;
        for (int i = 0; i < 256; ++i) { a += red[0][i]; b2 += red[1][i]; }
        write_loss3(loss3, a, b2, k.invD, beta, reg);
    }
}

// 16 < N <= IGN_HEAD_NMAX: ign_loss_wide_kernel's layout (one wave per row, lanes over the classes in chunks of 64, row sums by
// butterfly, the rows' loss terms added in ascending row order)
__global__ void __launch_bounds__(LOSS_WAVES * 64) ign_loss_mix_wide_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                                            const long long* __restrict__ ya,
                                                                            const long long* __restrict__ yb,
                                                                            const float* __restrict__ lam,
                                                                            const float* __restrict__ cw, float* __restrict__ out,
                                                                            float* __restrict__ eta_out, float* __restrict__ loss3,
                                                                            float* __restrict__ gs, float* __restrict__ gd, int B,
                                                                            int N, float beta, float eps,
                                                                            const float* __restrict__ reg) {
    __shared__ float ce[2][LOSS_TILE];
    __shared__ float wl[IGN_HEAD_NMAX];
    static_assert(LOSS_TILE >= LOSS_WAVES * 64, "cem_prepass borrows one row of `ce` for its per-thread sums");
    const CeW k = cem_prepass(cw, ya, yb, lam, B, N, eps, wl, ce[0]);
    float tot[2] = {0.f, 0.f};                         // {CEm(out), CEm(s)} batch sums before / D, meaningful in thread 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < B; base += LOSS_TILE) {
        const int rows = min(LOSS_TILE, B - base);
        for (int r = wave; r < rows; r += LOSS_WAVES) {
            const int b = base + r;
            const float* sr = s + (long long)b * N;
            const float* dr = d + (long long)b * N;
            const CeMRow row = cem_row(ya, yb, lam, b, N, wl);
            float sv[LOSS_KMAX], dv[LOSS_KMAX], q[LOSS_KMAX], ov[LOSS_KMAX], eo[LOSS_KMAX], wv[LOSS_KMAX];
            float mx = -INFINITY;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                const int n = kk * 64 + lane;
                sv[kk] = n < N ? sr[n] : -INFINITY;
                dv[kk] = n < N ? dr[n] : 0.f;
                wv[kk] = n < N ? wl[n] : 0.f;
                mx = fmaxf(mx, sv[kk]);
            }
            mx = wave_max(mx);
            float z = 0.f, z2 = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                q[kk] = kk * 64 + lane < N ? expf(sv[kk] - mx) : 0.f;
                z += q[kk];
                z2 += q[kk] * q[kk];
            }
            z = wave_sum(z);
            z2 = wave_sum(z2);
            const float G = gate_G(z, z2);
            const float eta = gate_eta(N, G);
            if (lane == 0) eta_out[b] = eta;
            float mo = -INFINITY, s_ya = 0.f, o_ya = 0.f, s_yb = 0.f, o_yb = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                const int n = kk * 64 + lane;
                ov[kk] = gate_mix(eta, sv[kk], dv[kk]);
                if (n < N) {
                    out[(long long)b * N + n] = ov[kk];
                    mo = fmaxf(mo, ov[kk]);
                }
                if (n == row.ya) { s_ya = sv[kk]; o_ya = ov[kk]; }
                if (n == row.yb) { s_yb = sv[kk]; o_yb = ov[kk]; }
            }
            mo = wave_max(mo);
            s_ya = wave_sum(s_ya);                // exactly one lane holds a label's logits, the others add zeros
            o_ya = wave_sum(o_ya);
            s_yb = wave_sum(s_yb);
            o_yb = wave_sum(o_yb);
            float zo = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                eo[kk] = kk * 64 + lane < N ? expf(ov[kk] - mo) : 0.f;
                zo += eo[kk];
            }
            zo = wave_sum(zo);
            const float lse_s = mx + logf(z), lse_o = mo + logf(zo);
            float smo_s = 0.f, smo_o = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk)
                if (kk * 64 + lane < N) {         // the padding lanes hold -inf logits
                    smo_s += wv[kk] * (lse_s - sv[kk]);
                    smo_o += wv[kk] * (lse_o - ov[kk]);
                }
            smo_s = wave_sum(smo_s);
            smo_o = wave_sum(smo_o);
            // gradients: g_out = dCEm(out)/dout ; through the gate ; + beta * dCEm(s)/ds
            float dot = 0.f;
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                const int n = kk * 64 + lane;
                eo[kk] = cem_grad(k, row, eo[kk] / zo, wv[kk], n);               // go
                if (n < N) dot += eo[kk] * (sv[kk] - dv[kk]);
            }
            dot = wave_sum(dot);
            const float c = gate_coef(N, dot);
#pragma unroll
            for (int kk = 0; kk < LOSS_KMAX; ++kk) {
                const int n = kk * 64 + lane;
                if (n < N) {
                    const float qn = q[kk] / z;
                    gs[(long long)b * N + n] = gate_ds(eta, eo[kk], c, qn, G) + beta * cem_grad(k, row, qn, wv[kk], n);
                    gd[(long long)b * N + n] = gate_dd(eta, eo[kk]);
                }
            }
            if (lane == 0) {
                ce[0][r] = cem_term(k, row, lse_o - o_ya, lse_o - o_yb, smo_o);
                ce[1][r] = cem_term(k, row, lse_s - s_ya, lse_s - s_yb, smo_s);
            }
        }
        add_in_row_order(ce, rows, tot);
    }
    if (threadIdx.x == 0) write_loss3(loss3, tot[0], tot[1], k.invD, beta, reg);
}

// ------------------------------------------------------------------------------------------------ CRPS tails
// One block of CRPS_THREADS threads, one thread per row (rows base + threadIdx.x of each tile).  Up to CRPS_NREG classes a
// row lives in registers (loops fully unrolled, guarded by n < N); wider rows are read from global memory and the gradient
// buffer doubles as the row's scratch.
// Row CRPS of softmax(z) against the step CDF of y; g <- d(batch-mean loss)/dz (2/B folded in).  Returns sum_j (F_j - H_j)^2.
// z and g may not alias.
template <int NR>
__device__ __forceinline__ float crps_row(RowBuf<NR>& z, RowBuf<NR>& g, const double* __restrict__ edges, double y, int N,
                                          float twoInvB) {
    float mx = -INFINITY;
    ROW_FOR(n) mx = fmaxf(mx, z[n]);
    float Z = 0.f;
    ROW_FOR(n) Z += expf(z[n] - mx);
    float F = 0.f, sq = 0.f;
    ROW_FOR(j) {
        F += expf(z[j] - mx) / Z;
        const float r = F - (edges[j] >= y ? 1.f : 0.f);
        sq += r * r;
        g[j] = r;
    }
    float acc = 0.f, dot = 0.f;
    ROW_FOR_REV(i) {
        acc += g[i];
        const float q = twoInvB * acc;
        g[i] = q;
        dot += (expf(z[i] - mx) / Z) * q;
    }
    ROW_FOR(k) g[k] = (expf(z[k] - mx) / Z) * (g[k] - dot);
    return sq;
}

template <int NR>
__global__ void __launch_bounds__(CRPS_THREADS) crps_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                            const double* __restrict__ edges, float* __restrict__ loss_out,
                                                            float* grad, int B, int N) {
    __shared__ float part[1][CRPS_THREADS];
    float tot[1] = {0.f};                              // meaningful in thread 0
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
            part[0][threadIdx.x] = crps_row<NR>(z, g, edges, (double)target[b], N, twoInvB);
            store_row<NR>(g, grad + o, N);
        }
        add_in_row_order(part, rows, tot);
    }
    if (threadIdx.x == 0) loss_out[0] = tot[0] * invB;
}

template <int NR>
__global__ void __launch_bounds__(CRPS_THREADS) ign_crps_kernel(const float* __restrict__ s, const float* __restrict__ d,
                                                                const float* __restrict__ target, const double* __restrict__ edges,
                                                                const float* __restrict__ reg, float* out, float* __restrict__ eta_out,
                                                                float* __restrict__ loss3, float* gs, float* gd, int B, int N,
                                                                float beta) {
    __shared__ float part[2][CRPS_THREADS];
    float tot[2] = {0.f, 0.f};                         // {CRPS(out), CRPS(sbm)} batch sums, meaningful in thread 0
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
            float mx, z, z2;
            row_stats<NR>(sv, N, mx, z, z2);
            const float G = gate_G(z, z2);
            const float eta = gate_eta(N, G);
            eta_out[b] = eta;
            ROW_FOR(n) ov[n] = gate_mix(eta, sv[n], dr[n]);
            store_row<NR>(ov, out + o, N);
            const double y = (double)target[b];
            // the sbm row first: its max and exponentials are row_stats', so none of them has to stay live across the other row
            // (with the mixture's row first the register row instantiation spills at 1024 threads)
            part[1][threadIdx.x] = crps_row<NR>(sv, gsv, edges, y, N, twoInvB);     // gsv = dCRPS(sbm)/dsbm
            part[0][threadIdx.x] = crps_row<NR>(ov, go, edges, y, N, twoInvB);      // go = dCRPS(out)/dout
            // through the gate: ds = eta*go + c*q*(q - G) + beta*gsv, dd = (1 - eta)*go
            float dot = 0.f;
            ROW_FOR(n) dot += go[n] * (sv[n] - dr[n]);
            const float c = gate_coef(N, dot);
            ROW_FOR(n) {
                const float qn = expf(sv[n] - mx) / z;
                const float g_o = go[n];
                gs[o + n] = gate_ds(eta, g_o, c, qn, G) + beta * gsv[n];
                gd[o + n] = gate_dd(eta, g_o);
            }
        }
        add_in_row_order(part, rows, tot);
    }
    if (threadIdx.x == 0) write_loss3(loss3, tot[0], tot[1], invB, beta, reg);
}

#undef ROW_FOR
#undef ROW_FOR_REV

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ign_gate_fwd(const float* sbm, const float* dnn, float* out, float* eta, int B, int N, float gating_value,
                            int use_gating_value, void* stream) {
    if (!sbm || !dnn || !out || !eta || B <= 0 || N < 2) {
        ign_set_error("ign_gate_fwd: null pointer or bad dimension (B=%d N=%d)", B, N);
        return IGN_E_ARG;
    }
    hipLaunchKernelGGL(gate_fwd_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, sbm, dnn, out, eta, B, N,
                       gating_value, use_gating_value);
    return ign_check_launch("gate_fwd_kernel");
}

extern "C" int ign_gate_bwd(const float* sbm, const float* dnn, const float* gout, const float* geta, float* gsbm,
                            float* gdnn, int B, int N, float gating_value, int use_gating_value, void* stream) {
    if (!sbm || !dnn || !gout || !gsbm || !gdnn || B <= 0 || N < 2) {
        ign_set_error("ign_gate_bwd: null pointer or bad dimension (B=%d N=%d)", B, N);
        return IGN_E_ARG;
    }
    hipLaunchKernelGGL(gate_bwd_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, sbm, dnn, gout, geta, gsbm,
                       gdnn, B, N, gating_value, use_gating_value);
    return ign_check_launch("gate_bwd_kernel");
}

extern "C" int ign_loss_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const float* reg, float* out,
                                    float* eta, float* loss2, float* gsbm, float* gdnn, int B, int N, float beta, void* stream) {
    if (!sbm || !dnn || !labels || !out || !eta || !loss2 || !gsbm || !gdnn || B <= 0 || N < 2) {
        ign_set_error("ign_loss_fwd_bwd: null pointer or bad dimension (B=%d N=%d, N <= %d)", B, N, IGN_HEAD_NMAX);
        return IGN_E_ARG;
    }
    if (N > IGN_HEAD_NMAX) { ign_set_error("ign_loss_fwd_bwd: N=%d classes > %d", N, IGN_HEAD_NMAX); return IGN_E_UNSUP; }
    const bool wide = N > LOSS_NMAX;
    hipLaunchKernelGGL(wide ? ign_loss_wide_kernel : ign_loss_kernel, dim3(1), dim3(wide ? LOSS_WAVES * 64 : 256), 0,
                       (hipStream_t)stream, sbm, dnn, labels, out, eta, loss2, gsbm, gdnn, B, N, beta, reg);
    return ign_check_launch(wide ? "ign_loss_wide_kernel" : "ign_loss_kernel");
}

extern "C" int ign_loss_fwd_bwd(const float* sbm, const float* dnn, const long long* labels, float* out, float* eta, float* loss2,
                                float* gsbm, float* gdnn, int B, int N, float beta, void* stream) {
    return ign_loss_fwd_bwd_reg(sbm, dnn, labels, nullptr, out, eta, loss2, gsbm, gdnn, B, N, beta, stream);
}

extern "C" int ign_loss_w_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const float* class_w,
                                      const float* reg, float* out, float* eta, float* loss3, float* gsbm, float* gdnn, int B, int N,
                                      float beta, float label_smoothing, void* stream) {
    if (!sbm || !dnn || !labels || !out || !eta || !loss3 || !gsbm || !gdnn || B <= 0 || N < 2) {
        ign_set_error("ign_loss_w_fwd_bwd_reg: null pointer or bad dimension (B=%d N=%d, N <= %d)", B, N, IGN_HEAD_NMAX);
        return IGN_E_ARG;
    }
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) {
        ign_set_error("ign_loss_w_fwd_bwd_reg: label_smoothing=%g outside [0, 1)", (double)label_smoothing);
        return IGN_E_ARG;
    }
    if (N > IGN_HEAD_NMAX) { ign_set_error("ign_loss_w_fwd_bwd_reg: N=%d classes > %d", N, IGN_HEAD_NMAX); return IGN_E_UNSUP; }
    const bool wide = N > LOSS_NMAX;
    {
        IgnScopedTimer tm("loss_w", (hipStream_t)stream);
        hipLaunchKernelGGL(wide ? ign_loss_w_wide_kernel : ign_loss_w_kernel, dim3(1), dim3(wide ? LOSS_WAVES * 64 : 256), 0,
                           (hipStream_t)stream, sbm, dnn, labels, class_w, out, eta, loss3, gsbm, gdnn, B, N, beta, label_smoothing,
                           reg);
    }
    return ign_check_launch(wide ? "ign_loss_w_wide_kernel" : "ign_loss_w_kernel");
}

extern "C" int ign_loss_mix_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const long long* labels_b,
                                        const float* lam_b, const float* class_w, const float* reg, float* out, float* eta,
                                        float* loss3, float* gsbm, float* gdnn, int B, int N, float beta, float label_smoothing,
                                        void* stream) {
    if (!sbm || !dnn || !labels || !labels_b || !lam_b || !out || !eta || !loss3 || !gsbm || !gdnn || B <= 0 || N < 2) {
        ign_set_error("ign_loss_mix_fwd_bwd_reg: null pointer or bad dimension (B=%d N=%d, N <= %d)", B, N, IGN_HEAD_NMAX);
        return IGN_E_ARG;
    }
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) {
        ign_set_error("ign_loss_mix_fwd_bwd_reg: label_smoothing=%g outside [0, 1)", (double)label_smoothing);
        return IGN_E_ARG;
    }
    if (N > IGN_HEAD_NMAX) { ign_set_error("ign_loss_mix_fwd_bwd_reg: N=%d classes > %d", N, IGN_HEAD_NMAX); return IGN_E_UNSUP; }
    const bool wide = N > LOSS_NMAX;
    {
        IgnScopedTimer tm("loss_mix", (hipStream_t)stream);
        hipLaunchKernelGGL(wide ? ign_loss_mix_wide_kernel : ign_loss_mix_kernel, dim3(1), dim3(wide ? LOSS_WAVES * 64 : 256), 0,
                           (hipStream_t)stream, sbm, dnn, labels, labels_b, lam_b, class_w, out, eta, loss3, gsbm, gdnn, B, N, beta,
                           label_smoothing, reg);
    }
    return ign_check_launch(wide ? "ign_loss_mix_wide_kernel" : "ign_loss_mix_kernel");
}

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
    hipLaunchKernelGGL(N <= CRPS_NREG ? crps_kernel<CRPS_NREG> : crps_kernel<0>, dim3(1), dim3(CRPS_THREADS), 0, (hipStream_t)stream,
                       logits, target, edges, loss_out, grad, B, N);
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
    hipLaunchKernelGGL(N <= CRPS_NREG ? ign_crps_kernel<CRPS_NREG> : ign_crps_kernel<0>, dim3(1), dim3(CRPS_THREADS), 0,
                       (hipStream_t)stream, sbm, dnn, target, edges, reg, out, eta, loss3, gsbm, gdnn, B, N, beta);
    return ign_check_launch("ign_crps_kernel");
}
