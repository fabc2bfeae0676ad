// Expert-head GEMMs and the two SBM regularisers: the small HBM-bound pieces of the training step.  (The gini gate and the fused
// loss tails are in ign_loss.hip; Adam, the gradient gather and clipping on the flat buffers are in ign_optim.hip.)
//
//  * head GEMM  out[b,n] = sum_f X[b,f] W[n,f] (+ bias[n])  with N = number of classes (2..IGN_HEAD_NMAX = 256; above 16 in
//    16-class chunks, one extra grid dimension, same launch count) -- "skinny":
//    IGN/model/Shapelet.py:171,200 (SBM head, F = G*K*C = 2440), IGN/model/Transformer.py:72,109 (F = T*d = 512000),
//    IGN/model/FullyConvNet.py:50,58.  N is far too small for an MFMA tile to pay (a 32x32 tile would be >90 % padding)
//    and the op moves 4*(B*F + N*F) bytes for 2*B*F*N flops (intensity ~N/2 flop/byte): HBM/L2 bound, so it is a
//    coalesced float4 streaming kernel with N accumulators per thread and a block reduction.
#include "ign_common.h"

constexpr int HEAD_NMAX = 16;

// ------------------------------------------------------------------------------------------------ head forward
// One block per row; 256 threads, or 1024 for long rows (the Transformer's 512 000-feature head: one 256-thread block per CU
// kept four loads per lane in flight and ran at 0.7 TB/s).
// WIDE (N > 16): blockIdx.y = 16-class chunk; each chunk runs the N <= 16 arithmetic on its classes n0 .. n0 + 15 (the row of X
// is re-read per chunk, from L2).  The N <= 16 instantiation is the single-chunk kernel (n0 = 0, one grid row).
template <bool WIDE>
__global__ void __launch_bounds__(1024) head_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        int B, int F, int N, long long ldx) {
    __shared__ float red[16][HEAD_NMAX];
    const int b = blockIdx.x;
    const int n0 = WIDE ? blockIdx.y * HEAD_NMAX : 0;
    const int nc = WIDE ? min(N - n0, HEAD_NMAX) : N;         // classes of this chunk
    const float* x = X + (long long)b * ldx;
    const float* Wc = W + (long long)n0 * F;
    float acc[HEAD_NMAX];
#pragma unroll
    for (int n = 0; n < HEAD_NMAX; ++n) acc[n] = 0.f;
    const int F4 = F & ~3;
    const int nthr = blockDim.x;
    for (int f = threadIdx.x * 4; f < F4; f += nthr * 4) {
        const float4 xv = *reinterpret_cast<const float4*>(x + f);
#pragma unroll
        for (int n = 0; n < HEAD_NMAX; ++n)
            if (n < nc) {
                const float4 wv = *reinterpret_cast<const float4*>(Wc + (long long)n * F + f);
                acc[n] += xv.x * wv.x + xv.y * wv.y + xv.z * wv.z + xv.w * wv.w;
            }
    }
    for (int f = F4 + threadIdx.x; f < F; f += nthr)
#pragma unroll
        for (int n = 0; n < HEAD_NMAX; ++n)
            if (n < nc) acc[n] += x[f] * Wc[(long long)n * F + f];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < HEAD_NMAX; ++n) {
        float v = acc[n];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][n] = v;
    }
    __syncthreads();
    if (threadIdx.x < nc) {
        const int n = threadIdx.x;
        float t = 0.f;
        for (int w = 0; w < (nthr >> 6); ++w) t += red[w][n];          // fixed order
        out[(long long)b * N + n0 + n] = t + (bias ? bias[n0 + n] : 0.f);
    }
}

// gX[b,f] = sum_n g[b,n] W[n,f].  WIDE: the thread walks the 16-class chunks in ascending order into one accumulator -- the
// order of a single N-loop, so the sum does not depend on the chunking.
template <bool WIDE>
__device__ __forceinline__ void head_bwd_x_body(const float* __restrict__ g, const float* __restrict__ W,
                                                float* __restrict__ gX, int B, int F, int N, long long ldx, int bx, int b) {
    const int f = (bx * 256 + threadIdx.x) * 4;
    if (f >= F) return;
    float gn[HEAD_NMAX];
    if constexpr (!WIDE) {
#pragma unroll
        for (int n = 0; n < HEAD_NMAX; ++n) gn[n] = n < N ? g[(long long)b * N + n] : 0.f;
    }
    if (f + 3 < F) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        const int nch = WIDE ? (N + HEAD_NMAX - 1) / HEAD_NMAX : 1;
        for (int c = 0; c < nch; ++c) {
            const int n0 = c * HEAD_NMAX, nc = WIDE ? min(N - n0, HEAD_NMAX) : N;
            if constexpr (WIDE) {
#pragma unroll
                for (int n = 0; n < HEAD_NMAX; ++n) gn[n] = n < nc ? g[(long long)b * N + n0 + n] : 0.f;
            }
#pragma unroll
            for (int n = 0; n < HEAD_NMAX; ++n)
                if (n < nc) {
                    const float4 wv = *reinterpret_cast<const float4*>(W + (long long)(n0 + n) * F + f);
                    r.x += gn[n] * wv.x; r.y += gn[n] * wv.y; r.z += gn[n] * wv.z; r.w += gn[n] * wv.w;
                }
        }
        *reinterpret_cast<float4*>(gX + (long long)b * ldx + f) = r;
    } else {                                         // (unreachable while F % 4 == 0 is required)
        for (int ff = f; ff < F; ++ff) {
            float r = 0.f;
            for (int n = 0; n < N; ++n) r += (WIDE ? g[(long long)b * N + n] : gn[n]) * W[(long long)n * F + ff];
            gX[(long long)b * ldx + ff] = r;
        }
    }
}

template <bool WIDE>
__global__ void __launch_bounds__(256) head_bwd_x_kernel(const float* __restrict__ g, const float* __restrict__ W,
                                                         float* __restrict__ gX, int B, int F, int N, long long ldx) {
    head_bwd_x_body<WIDE>(g, W, gX, B, F, N, ldx, blockIdx.x, blockIdx.y);
}

// gW[n,f] = sum_b g[b,n] X[b,f];  gbias[n] = sum_b g[b,n].
// Block = 32 consecutive f x 8 batch groups: each thread sums its group's rows in ascending order, the 8 partials are
// combined in fixed order through LDS (deterministic).  32 f per block keeps F/32 blocks in flight (F=2440: 77 blocks;
// a 256-f-per-block version ran 10 blocks and took 125 us of a 17.9 ms step).
// `add` / `add_scale` (both nullable): gW += add_scale[0] * add -- a gradient of the same tensor that does not depend on the batch
// (the L1 regulariser of the SBM head, IGN/model/Shapelet.py:219) rides on this store instead of an accumulate kernel.
// `bx` = the block's 32-f slice, `n0` = its first class.  WIDE: the block covers classes n0 .. n0 + 15 and stages only those
// columns of g (B x 16 floats, whatever N), so the LDS budget does not grow with N; f-slice 0 of each chunk writes its gbias.
template <bool WIDE>
__device__ __forceinline__ void head_bwd_w_body(const float* __restrict__ g, const float* __restrict__ X,
                                                float* __restrict__ gW, float* __restrict__ gbias, int B, int F,
                                                int N, long long ldx, const float* __restrict__ add,
                                                const float* __restrict__ add_scale, const int bx, const int n0) {
    extern __shared__ float sm[];               // g copy [B*gsn], then partials [8][HEAD_NMAX][32]
    const int gsn = WIDE ? HEAD_NMAX : N;       // row pitch of the g copy
    const int nc = WIDE ? min(N - n0, HEAD_NMAX) : N;
    float* gs = sm;
    float* part = sm + B * gsn;
    if (WIDE) {
        for (int i = threadIdx.x; i < B * HEAD_NMAX; i += 256) {
            const int b = i / HEAD_NMAX, n = i % HEAD_NMAX;
            gs[i] = n < nc ? g[(long long)b * N + n0 + n] : 0.f;
        }
    } else {
        for (int i = threadIdx.x; i < B * N; i += 256) gs[i] = g[i];
    }
    __syncthreads();
    if (gbias && bx == 0 && threadIdx.x < nc) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += gs[b * gsn + threadIdx.x];
        gbias[n0 + threadIdx.x] = s;
    }
    const int fl = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int f = bx * 32 + fl;
    const int per = (B + 7) / 8;
    const int b0 = grp * per, b1 = min(B, b0 + per);
    float acc[HEAD_NMAX];
#pragma unroll
    for (int n = 0; n < HEAD_NMAX; ++n) acc[n] = 0.f;
    if (f < F)
        for (int b = b0; b < b1; ++b) {
            const float xv = X[(long long)b * ldx + f];
#pragma unroll
            for (int n = 0; n < HEAD_NMAX; ++n)
                if (n < nc) acc[n] = fmaf(gs[b * gsn + n], xv, acc[n]);
        }
#pragma unroll
    for (int n = 0; n < HEAD_NMAX; ++n)
        if (n < nc) part[(grp * HEAD_NMAX + n) * 32 + fl] = acc[n];
    __syncthreads();
    for (int i = threadIdx.x; i < nc * 32; i += 256) {
        const int n = i >> 5, ff = i & 31;
        if (bx * 32 + ff < F) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) s += part[(q * HEAD_NMAX + n) * 32 + ff];
            const long long o = (long long)(n0 + n) * F + bx * 32 + ff;
            if (add) s += (add_scale ? add_scale[0] : 1.f) * add[o];
            gW[o] = s;
        }
    }
}

// grid (F/32 slices[, 16-class chunks])
template <bool WIDE>
__global__ void __launch_bounds__(256) head_bwd_w_kernel(const float* __restrict__ g, const float* __restrict__ X,
                                                         float* __restrict__ gW, float* __restrict__ gbias, int B, int F,
                                                         int N, long long ldx, const float* __restrict__ add,
                                                         const float* __restrict__ add_scale) {
    head_bwd_w_body<WIDE>(g, X, gW, gbias, B, F, N, ldx, add, add_scale, blockIdx.x, WIDE ? blockIdx.y * HEAD_NMAX : 0);
}

// both gradients in ONE launch: blocks [0, nwb) play head_bwd_w_kernel's role, the rest head_bwd_x_kernel's ((nxb, B) grid
// flattened) -- block-uniform branch, the two halves touch disjoint outputs.  WIDE: nwb = (F/32 slices) x (16-class chunks),
// slice-fastest.
template <bool WIDE>
__global__ void __launch_bounds__(256) head_bwd_xw_kernel(const float* __restrict__ g, const float* __restrict__ X,
                                                          const float* __restrict__ W, float* __restrict__ gX,
                                                          float* __restrict__ gW, float* __restrict__ gbias, int B, int F, int N,
                                                          long long ldx, const float* __restrict__ add,
                                                          const float* __restrict__ add_scale, int nwb, int nxb) {
    const int blk = blockIdx.x;
    if (blk < nwb) {
        const int nfb = WIDE ? (F + 31) / 32 : nwb;
        const int c = WIDE ? blk / nfb : 0;
        head_bwd_w_body<WIDE>(g, X, gW, gbias, B, F, N, ldx, add, add_scale, blk - c * nfb, c * HEAD_NMAX);
    } else {
        const int r = blk - nwb;
        head_bwd_x_body<WIDE>(g, W, gX, B, F, N, ldx, r % nxb, r / nxb);
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ign_head_fwd(const float* X, const float* W, const float* bias, float* out, int B, int F, int N,
                            long long ldx, void* stream) {
    if (!X || !W || !out || B <= 0 || F <= 0 || N <= 0 || ldx < F) {
        ign_set_error("ign_head_fwd: null pointer or bad dimension (B=%d F=%d N=%d ldx=%lld)", B, F, N, ldx);
        return IGN_E_ARG;
    }
    if (N > IGN_HEAD_NMAX) { ign_set_error("ign_head_fwd: N=%d classes > %d", N, IGN_HEAD_NMAX); return IGN_E_UNSUP; }
    if ((ldx & 3) || ((uintptr_t)X & 15) || ((uintptr_t)W & 15) || (F & 3)) {
        ign_set_error("ign_head_fwd: X/W must be 16-byte aligned with F and ldx multiples of 4 (F=%d ldx=%lld)", F, ldx);
        return IGN_E_ARG;
    }
    IgnScopedTimer tm("head_fwd", (hipStream_t)stream);
    const dim3 blk(F >= 32768 ? 1024 : 256);
    if (N <= HEAD_NMAX)
        hipLaunchKernelGGL(head_fwd_kernel<false>, dim3(B), blk, 0, (hipStream_t)stream, X, W, bias, out, B, F, N, ldx);
    else
        hipLaunchKernelGGL(head_fwd_kernel<true>, dim3(B, (N + HEAD_NMAX - 1) / HEAD_NMAX), blk, 0, (hipStream_t)stream, X, W, bias,
                           out, B, F, N, ldx);
    return ign_check_launch("head_fwd_kernel");
}

extern "C" int ign_head_bwd(const float* g, const float* X, const float* W, float* gX, float* gW, float* gbias, int B,
                            int F, int N, long long ldx, void* stream) {
    return ign_head_bwd_acc(g, X, W, gX, gW, gbias, nullptr, nullptr, B, F, N, ldx, stream);
}

extern "C" int ign_head_bwd_acc(const float* g, const float* X, const float* W, float* gX, float* gW, float* gbias,
                                const float* gW_add, const float* add_scale_dev, int B, int F, int N, long long ldx, void* stream) {
    if (!g || !X || !W || B <= 0 || F <= 0 || N <= 0 || ldx < F) {
        ign_set_error("ign_head_bwd: null pointer or bad dimension");
        return IGN_E_ARG;
    }
    if (N > IGN_HEAD_NMAX) { ign_set_error("ign_head_bwd: N=%d classes > %d", N, IGN_HEAD_NMAX); return IGN_E_UNSUP; }
    if ((ldx & 3) || (F & 3) || ((uintptr_t)W & 15) || (gX && ((uintptr_t)gX & 15))) {
        ign_set_error("ign_head_bwd: W/gX must be 16-byte aligned with F and ldx multiples of 4");
        return IGN_E_ARG;
    }
    // the weight gradient stages g in LDS: all of it for N <= 16, one 16-class chunk of it (B x 16) above
    const bool wide = N > HEAD_NMAX;
    const int gsn = wide ? HEAD_NMAX : N, nch = (N + HEAD_NMAX - 1) / HEAD_NMAX;
    if ((size_t)B * gsn * 4 > 40 * 1024) { ign_set_error("ign_head_bwd: B*N=%d too large for the LDS copy of g", B * gsn); return IGN_E_TOOBIG; }
    const size_t lds = ((size_t)B * gsn + 8 * HEAD_NMAX * 32) * 4;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (gX && gW) {
        const int nfb = (F + 31) / 32, nxb = (F / 4 + 255) / 256;
        IgnScopedTimer tm("head_bwd_xw", s);
        if (!wide)
            hipLaunchKernelGGL(head_bwd_xw_kernel<false>, dim3((unsigned)(nfb + nxb * B)), dim3(256), lds, s, g, X, W, gX, gW, gbias, B,
                               F, N, ldx, gW_add, add_scale_dev, nfb, nxb);
        else
            hipLaunchKernelGGL(head_bwd_xw_kernel<true>, dim3((unsigned)(nfb * nch + nxb * B)), dim3(256), lds, s, g, X, W, gX, gW,
                               gbias, B, F, N, ldx, gW_add, add_scale_dev, nfb * nch, nxb);
        return ign_check_launch("head_bwd_xw_kernel");
    }
    if (gX) {
        IgnScopedTimer tm("head_bwd_x", s);
        if (!wide)
            hipLaunchKernelGGL(head_bwd_x_kernel<false>, dim3((F / 4 + 255) / 256, B), dim3(256), 0, s, g, W, gX, B, F, N, ldx);
        else
            hipLaunchKernelGGL(head_bwd_x_kernel<true>, dim3((F / 4 + 255) / 256, B), dim3(256), 0, s, g, W, gX, B, F, N, ldx);
        if ((rc = ign_check_launch("head_bwd_x_kernel"))) return rc;
    }
    if (gW) {
        IgnScopedTimer tm("head_bwd_w", s);
        if (!wide)
            hipLaunchKernelGGL(head_bwd_w_kernel<false>, dim3((F + 31) / 32), dim3(256), lds, s, g, X, gW, gbias, B, F, N, ldx, gW_add,
                               add_scale_dev);
        else
            hipLaunchKernelGGL(head_bwd_w_kernel<true>, dim3((F + 31) / 32, nch), dim3(256), lds, s, g, X, gW, gbias, B, F, N, ldx,
                               gW_add, add_scale_dev);
        if ((rc = ign_check_launch("head_bwd_w_kernel"))) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ shapelet diversity
// loss = mean_{c,i,j} exp(-|| w[i,c,:] - w[j,c,:] + 1e-6 ||_2) (1 - delta_ij)      IGN/model/Shapelet.py:223-230
// (nn.PairwiseDistance(p=2): the eps is added to the DIFFERENCE, so d_ij != d_ji in the last bits -- both are kept).
// One block per channel: pass 1 reduces the K*K squared distances into LDS, pass 2 forms the loss partial and the
// gradient of the (unit-weighted) loss w.r.t. w.  Replaces ~25 tiny elementwise / reduction launches per group.
constexpr int DIV_KMAX = 16;

// one block = one channel c of one group; thread 0 returns the loss partial (already times `scale`), gw receives scale * gradient
__device__ __forceinline__ float diversity_block(const float* __restrict__ w, float* __restrict__ gw, int K, int C, int L, int c,
                                                 float eps, float scale) {
    __shared__ float D2[DIV_KMAX][DIV_KMAX];        // D2[i][j] = sum_l (w_i - w_j + eps)^2
    __shared__ float Ew[DIV_KMAX][DIV_KMAX];        // exp(-D_ij) / D_ij   (0 on the diagonal)
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t cs = (size_t)C * L;                 // stride between shapelets
    const float* wc = w + (size_t)c * L;
    for (int i = 0; i < K; ++i)
        for (int j = i + 1; j < K; ++j) {
            float a = 0.f, b = 0.f;
            for (int l = tid; l < L; l += 256) {
                const float dl = wc[i * cs + l] - wc[j * cs + l];
                a = fmaf(dl + eps, dl + eps, a);
                b = fmaf(eps - dl, eps - dl, b);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
            __syncthreads();
            if (lane == 0) red[wave] = a;
            __syncthreads();
            const float ta = red[0] + red[1] + red[2] + red[3];
            __syncthreads();
            if (lane == 0) red[wave] = b;
            __syncthreads();
            const float tb = red[0] + red[1] + red[2] + red[3];
            if (tid == 0) { D2[i][j] = ta; D2[j][i] = tb; }
        }
    __syncthreads();
    const float norm = 1.f / ((float)C * K * K);
    if (tid < K * K) {
        const int i = tid / K, j = tid % K;
        float e = 0.f, ew = 0.f;
        if (i != j) {
            const float d = sqrtf(D2[i][j]);
            e = expf(-d);
            ew = e / d;
        }
        Ew[i][j] = ew;
        D2[i][j] = e;                                // reuse as e_ij for the loss sum below
    }
    __syncthreads();
    float lossp = 0.f;
    if (tid == 0) {
        float s = 0.f;
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) s += D2[i][j];
        lossp = s * norm * scale;
    }
    // d e_ij / d w_i[l] = -e_ij (dl + eps) / D_ij ;  d e_ji / d w_i[l] = +e_ji (eps - dl) / D_ji   (dl = w_i[l] - w_j[l])
    for (int l = tid; l < L; l += 256)
        for (int i = 0; i < K; ++i) {
            const float wi = wc[i * cs + l];
            float g = 0.f;
            for (int j = 0; j < K; ++j)
                if (j != i) {
                    const float dl = wi - wc[j * cs + l];
                    g += -Ew[i][j] * (dl + eps) + Ew[j][i] * (eps - dl);
                }
            gw[i * cs + (size_t)c * L + l] = g * norm * scale;
        }
    return lossp;
}

__global__ void __launch_bounds__(256) diversity_kernel(const float* __restrict__ w, float* __restrict__ loss_part,
                                                        float* __restrict__ gw, int K, int C, int L, float eps) {
    const float lp = diversity_block(w, gw, K, C, L, blockIdx.x, eps, 1.f);
    if (threadIdx.x == 0) loss_part[blockIdx.x] = lp;
}

// ------------------------------------------------------------------------------------------------ both SBM regularisers, one launch
// loss = lambda_reg * mean |W| + lambda_div * sum_g diversity_g   (ShapeBottleneckModel.loss, IGN/model/Shapelet.py:217-230) with
// the gradient of every term -- the value does not depend on the batch, so forward and backward are one launch; the consumers
// (head weight gradient, shapelet gradient reduction) add `upstream * gradient` in their own epilogues.
//   blocks [0, G*C): channel c of group g (diversity_block);  blocks [G*C, G*C + nwb): 1024 elements of W each.
// Every block leaves one partial; the block that draws the last ticket adds them up in a fixed order (thread-strided sums, then
// a fixed tree), so the result is bitwise reproducible although the arrival order is not.  Cross-block visibility follows the
// producer / consumer recipe of the MI355X guide (agent-scope release before the ticket, acquire after it, sc1 loads).
constexpr int REG_GMAX = 8;
constexpr int REG_TICKET_WORD = 0, REG_PARTS_WORD = 4;      // workspace words: [ticket, 3 spare, nblk partials]
struct RegTable {
    const float* w[REG_GMAX];
    float* gw[REG_GMAX];
    int K[REG_GMAX], L[REG_GMAX];
};
__global__ void __launch_bounds__(256) sbm_reg_kernel(const RegTable t, int G, int C, const float* __restrict__ W,
                                                      float* __restrict__ gWreg, long long nW, int nwb, float lam_reg, float lam_div,
                                                      float eps, float* __restrict__ parts, unsigned int* __restrict__ ticket,
                                                      float* __restrict__ loss_out) {
    __shared__ float red[256];
    __shared__ int is_last;
    const int blk = blockIdx.x, tid = threadIdx.x;
    const int nblk = G * C + nwb;
    float lp = 0.f;
    if (blk < G * C) {
        const int g = blk / C, c = blk - g * C;
        lp = diversity_block(t.w[g], t.gw[g], t.K[g], C, t.L[g], c, eps, lam_div);
    } else {
        // lambda_reg * mean |W|: gradient lambda_reg * sign(W) / numel (sign(0) = 0, as aten::sgn)
        const long long i0 = (long long)(blk - G * C) * 1024 + tid * 4;
        const float sc = lam_reg / (float)nW;
        float a = 0.f;
        for (int u = 0; u < 4; ++u) {
            const long long i = i0 + u;
            if (i < nW) {
                const float v = W[i];
                a += fabsf(v);
                gWreg[i] = v > 0.f ? sc : (v < 0.f ? -sc : 0.f);
            }
        }
        red[tid] = a;
        __syncthreads();
        if (tid == 0) {
            float sacc = 0.f;
            for (int i = 0; i < 256; ++i) sacc += red[i];
            lp = sacc * sc;
        }
    }
    if (tid == 0) {
        __hip_atomic_store(parts + blk, lp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (old == (unsigned int)(nblk - 1));
        if (is_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!is_last) return;
    float a = 0.f;
    for (int i = tid; i < nblk; i += 256) a += __hip_atomic_load(parts + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    red[tid] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        loss_out[0] = red[0];
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch on this stream
    }
}

extern "C" size_t ign_sbm_reg_workspace_bytes(int G, int C, long long nW) {
    if (G < 0 || G > REG_GMAX || C <= 0 || nW < 0) return 0;
    return (size_t)(G * C + (nW + 1023) / 1024 + 4) * sizeof(float);
}

extern "C" int ign_sbm_reg_fwd_bwd(const float* W, float* gW_reg, long long nW, float lambda_reg, int G, const float* const* w_kcl,
                                   float* const* gw_kcl, const int* K, const int* L, int C, float lambda_div, float eps,
                                   float* loss_out, void* workspace, void* stream) {
    static const char* who = "ign_sbm_reg_fwd_bwd";
    if (!loss_out || !workspace || G < 0 || G > REG_GMAX || C <= 0 || nW < 0 || (nW > 0 && (!W || !gW_reg)) ||
        (G > 0 && (!w_kcl || !gw_kcl || !K || !L))) {
        ign_set_error("%s: null pointer or bad dimension (G=%d C=%d nW=%lld)", who, G, C, nW);
        return IGN_E_ARG;
    }
    RegTable t;
    for (int g = 0; g < G; ++g) {
        if (!w_kcl[g] || !gw_kcl[g] || K[g] <= 0 || L[g] <= 0) { ign_set_error("%s: group %d: null pointer or bad K / L", who, g); return IGN_E_ARG; }
        if (K[g] > DIV_KMAX) { ign_set_error("%s: K=%d > %d shapelets per group", who, K[g], DIV_KMAX); return IGN_E_UNSUP; }
        t.w[g] = w_kcl[g]; t.gw[g] = gw_kcl[g]; t.K[g] = K[g]; t.L[g] = L[g];
    }
    const int nwb = (int)((nW + 1023) / 1024);
    const int nblk = G * C + nwb;
    if (nblk <= 0) { ign_set_error("%s: nothing to do", who); return IGN_E_ARG; }
    // The caller zero-fills the workspace ONCE; the kernel re-arms it.  The ticket is word REG_TICKET_WORD whatever nblk is, so calls
    // of different sizes may follow each other on one buffer (behind the partials it would sit on a stale partial of a larger call).
    unsigned int* ticket = (unsigned int*)workspace + REG_TICKET_WORD;
    float* parts = (float*)workspace + REG_PARTS_WORD;
    IgnScopedTimer tm("sbm_reg", (hipStream_t)stream);
    hipLaunchKernelGGL(sbm_reg_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, t, G, C, W, gW_reg, nW, nwb, lambda_reg,
                       lambda_div, eps, parts, ticket, loss_out);
    return ign_check_launch("sbm_reg_kernel");
}

extern "C" int ign_diversity_fwd_bwd(const float* w_kcl, float* loss_part_c, float* gw_kcl, int K, int C, int L, float eps,
                                     void* stream) {
    if (!w_kcl || !loss_part_c || !gw_kcl || K <= 0 || C <= 0 || L <= 0) {
        ign_set_error("ign_diversity_fwd_bwd: null pointer or bad dimension (K=%d C=%d L=%d)", K, C, L);
        return IGN_E_ARG;
    }
    if (K > DIV_KMAX) { ign_set_error("ign_diversity_fwd_bwd: K=%d > %d shapelets per group", K, DIV_KMAX); return IGN_E_UNSUP; }
    IgnScopedTimer tm("diversity", (hipStream_t)stream);
    hipLaunchKernelGGL(diversity_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, w_kcl, loss_part_c, gw_kcl, K, C, L, eps);
    return ign_check_launch("diversity_kernel");
}
