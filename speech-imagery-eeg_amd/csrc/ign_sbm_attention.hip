// SBM attention head (sbm_cls='attention', IGN/model/Shapelet.py:117-131, 201-205) as fused kernels: the (B,F,F) scores and
// probabilities of the torch composition are never stored.
//
//   q_i = x_i a + Pq_i,  k_j = x_j c + Pk_j   (Pq = bq + pos, Pk = bk + pos; a / c the 16-wide q / k projection weights)
//   o_i = sum_j softmax_j(tau q_i.k_j) x_j
// The 16-term dot product factorises:  q_i.k_j = gamma x_i x_j + x_i u_j + w_i x_j + M_ij  with gamma = a.c, u_j = a.Pk_j,
// w_i = Pq_i.c and M = Pq Pk^T, which is the same for every sample.  A thread owns one row (i, or j in the column kernel) of NB
// samples, so each M element it computes (16 FMAs) serves NB samples; everything per sample is three FMAs and the softmax.
// Scores are kept in base-2 units: kappa = tau log2(e) is folded into Pq, gamma, u and w, so exp is one v_exp_f32; the saved
// lse is base-2 as well (lse2 = m + log2 l) and only the backward of this file reads it.
//
// Layout (deterministic, no float atomics):
//   fwd        block = (64 rows i, a chunk of 32 samples), loops over j in LDS tiles of 64;  online softmax per 8 j.
//   bwd row    same blocking; dx (q side) -> dx, and per chunk: dPq contraction (F,16), dw (F), dgamma (one per block).
//   bwd col    block = (64 columns j, a chunk of 32 samples), loops over i; dx += (k side) + (v side), per chunk dPk (F,16), du (F).
//   reduce     16 rows per block: sums the chunk partials in chunk order, writes dpos, leaves 4x16 partials per block.
//   final      one block: bias and projection-weight gradients from those partials in block order.
// With E = tau g_i P_ij (x_j - o_i) the gradient of the raw dot product (the kernels accumulate it without tau and scale once):
//   dx_i += sum_j E_ij (gamma x_j + u_j)   dx_j += sum_i E_ij (gamma x_i + w_i) + sum_i P_ij g_i
//   dw_i = sum_{b,j} E x_j   du_j = sum_{b,i} E x_i   dgamma = sum E x_i x_j
//   dPq_i = sum_j (sum_b E_ij) Pk_j + dw_i c    dPk_j = sum_i (sum_b E_ij) Pq_i + du_j a
//   da = dgamma c + sum_j du_j Pk_j   dc = dgamma a + sum_i dw_i Pq_i   dbq = sum dPq   dbk = sum dPk   dpos = dPq + dPk
// Memory: the saved o / lse (B,F) and, in the backward, 2 F*16 + 2 F floats per chunk of 32 samples.
#include "ign_common.h"
#include <math.h>

namespace {

constexpr int SA_D = 16;          // attention width (SelfAttention(dim_feature, 16))
constexpr int SA_NB = 8;          // samples per thread
constexpr int SA_WAVES = 4;       // waves per block, each on its own NB samples
constexpr int SA_BC = SA_NB * SA_WAVES;   // samples per chunk (block)
constexpr int SA_ROWS = 64;       // rows (i or j) per block: one per lane
constexpr int SA_T = 64;          // staged rows of the other side per LDS tile
constexpr int SA_SUB = 8;         // rows per inner step (one M-tile column per lane)
constexpr float SA_LN2 = 0.69314718055994530942f;
constexpr float SA_LOG2E = 1.44269504088896340736f;

__device__ __forceinline__ float sa_exp2(float v) { return __builtin_amdgcn_exp2f(v); }

__device__ __forceinline__ float dot16(const float* __restrict__ p, const float* __restrict__ s) {
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < SA_D; ++d) acc = fmaf(p[d], s[d], acc);
    return acc;
}

// M'-element of one register row r (16 floats) against the staged row `t` (16 floats, LDS), plus its mask
__device__ __forceinline__ float m_elem(const float* __restrict__ r, const float* __restrict__ t, float mask) {
    const float4* t4 = reinterpret_cast<const float4*>(t);
    float acc = mask;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = t4[q];
        acc = fmaf(r[4 * q + 0], v.x, acc);
        acc = fmaf(r[4 * q + 1], v.y, acc);
        acc = fmaf(r[4 * q + 2], v.z, acc);
        acc = fmaf(r[4 * q + 3], v.w, acc);
    }
    return acc;
}

__device__ __forceinline__ void axpy16(float* __restrict__ acc, float e, const float* __restrict__ t) {
    const float4* t4 = reinterpret_cast<const float4*>(t);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = t4[q];
        acc[4 * q + 0] = fmaf(e, v.x, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(e, v.y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(e, v.z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(e, v.w, acc[4 * q + 3]);
    }
}

struct SaParams {
    const float* wq;    // (16)  q_proj.weight[:,0]
    const float* bq;    // (16)
    const float* wk;    // (16)  k_proj.weight[:,0]
    const float* bk;    // (16)
    const float* pos;   // (>=F, 16)
};

// Stage the "key side" of a tile for the forward / row kernels: Pk rows (unscaled), u'_j = kappa a.Pk_j and the mask,
// then x_j and A'_j = gamma' x_j + u'_j of the block's samples ([j][sample] so a wave reads its NB samples as float4s).
struct KeyTile {
    float pk[SA_T * SA_D];
    float xs[SA_T * SA_BC];
    float as[SA_T * SA_BC];
    float us[SA_T];
    float mask[SA_T];
};

static_assert(offsetof(KeyTile, as) == offsetof(KeyTile, xs) + SA_T * SA_BC * sizeof(float) &&
              2 * SA_T * SA_BC >= SA_WAVES * SA_ROWS * SA_D && SA_T * SA_D >= 2 * SA_WAVES * SA_ROWS,
              "the row kernel's end-of-block reduction reuses xs + as and pk");

__device__ void stage_keys(KeyTile& t, const SaParams& P, const float* __restrict__ x, long long ldx, int B, int F, int b0,
                           int j0, float kappa, float gam, const float* a) {
    const int tid = threadIdx.x;
    for (int idx = tid; idx < SA_T * SA_D; idx += blockDim.x) {
        const int jj = idx >> 4, d = idx & 15, j = j0 + jj;
        t.pk[idx] = j < F ? P.bk[d] + P.pos[(long long)j * SA_D + d] : 0.f;
    }
    __syncthreads();
    if (tid < SA_T) {
        const int j = j0 + tid;
        t.us[tid] = kappa * dot16(a, &t.pk[tid * SA_D]);
        t.mask[tid] = j < F ? 0.f : -INFINITY;
    }
    __syncthreads();
    for (int idx = tid; idx < SA_T * SA_BC; idx += blockDim.x) {
        const int b = idx / SA_T, jj = idx - b * SA_T, j = j0 + jj, bg = b0 + b;
        const float xv = (j < F && bg < B) ? x[(long long)bg * ldx + j] : 0.f;
        t.xs[jj * SA_BC + b] = xv;
        t.as[jj * SA_BC + b] = fmaf(gam, xv, t.us[jj]);
    }
    __syncthreads();
}

__device__ __forceinline__ void load_a_c(const SaParams& P, float* a, float* c, float& gam_raw) {
#pragma unroll
    for (int d = 0; d < SA_D; ++d) { a[d] = P.wq[d]; c[d] = P.wk[d]; }
    gam_raw = dot16(a, c);
}

// -------------------------------------------------------------------------------------------------------------- forward
__global__ void __launch_bounds__(256) sbm_attn_fwd_kernel(const float* __restrict__ x, long long ldx, const SaParams P,
                                                           float* __restrict__ out, float* __restrict__ lse, int B, int F,
                                                           float kappa) {
    __shared__ __attribute__((aligned(16))) KeyTile t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * SA_ROWS + lane;
    const int b0 = blockIdx.y * SA_BC, bw = b0 + wave * SA_NB;
    float a[SA_D], c[SA_D], gam;
    load_a_c(P, a, c, gam);
    gam *= kappa;
    const bool iv = i < F;
    float pq[SA_D];
#pragma unroll
    for (int d = 0; d < SA_D; ++d) pq[d] = iv ? kappa * (P.bq[d] + P.pos[(long long)i * SA_D + d]) : 0.f;
    const float wi = dot16(pq, c);
    float xi[SA_NB], m[SA_NB], l[SA_NB], o[SA_NB];
#pragma unroll
    for (int b = 0; b < SA_NB; ++b) {
        xi[b] = (iv && bw + b < B) ? x[(long long)(bw + b) * ldx + i] : 0.f;
        m[b] = -INFINITY; l[b] = 0.f; o[b] = 0.f;
    }
    for (int j0 = 0; j0 < F; j0 += SA_T) {
        __syncthreads();                                    // the previous tile is consumed
        stage_keys(t, P, x, ldx, B, F, b0, j0, kappa, gam, a);
        const int nj = min(SA_T, F - j0);
        for (int jt = 0; jt < nj; jt += SA_SUB) {
            float mt[SA_SUB];
#pragma unroll
            for (int s = 0; s < SA_SUB; ++s) mt[s] = m_elem(pq, &t.pk[(jt + s) * SA_D], t.mask[jt + s]);
#pragma unroll
            for (int h = 0; h < SA_NB / 4; ++h) {
                float sc[4][SA_SUB], xv[4][SA_SUB];
#pragma unroll
                for (int s = 0; s < SA_SUB; ++s) {
                    const float4 x4 = *reinterpret_cast<const float4*>(&t.xs[(jt + s) * SA_BC + wave * SA_NB + 4 * h]);
                    const float4 a4 = *reinterpret_cast<const float4*>(&t.as[(jt + s) * SA_BC + wave * SA_NB + 4 * h]);
                    xv[0][s] = x4.x; xv[1][s] = x4.y; xv[2][s] = x4.z; xv[3][s] = x4.w;
                    sc[0][s] = fmaf(xi[4 * h + 0], a4.x, fmaf(wi, x4.x, mt[s]));
                    sc[1][s] = fmaf(xi[4 * h + 1], a4.y, fmaf(wi, x4.y, mt[s]));
                    sc[2][s] = fmaf(xi[4 * h + 2], a4.z, fmaf(wi, x4.z, mt[s]));
                    sc[3][s] = fmaf(xi[4 * h + 3], a4.w, fmaf(wi, x4.w, mt[s]));
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int b = 4 * h + r;
                    float mx = sc[r][0];
#pragma unroll
                    for (int s = 1; s < SA_SUB; ++s) mx = fmaxf(mx, sc[r][s]);
                    const float mn = fmaxf(m[b], mx);      // finite: the first step of a row holds j = 0
                    const float al = sa_exp2(m[b] - mn);
                    float lb = l[b] * al, ob = o[b] * al;
#pragma unroll
                    for (int s = 0; s < SA_SUB; ++s) {
                        const float p = sa_exp2(sc[r][s] - mn);
                        lb += p;
                        ob = fmaf(p, xv[r][s], ob);
                    }
                    m[b] = mn; l[b] = lb; o[b] = ob;
                }
            }
        }
    }
    if (!iv) return;
#pragma unroll
    for (int b = 0; b < SA_NB; ++b) {
        if (bw + b >= B) break;
        const long long e = (long long)(bw + b) * F + i;
        out[e] = o[b] / l[b];
        if (lse) lse[e] = m[b] + log2f(l[b]);
    }
}

// ------------------------------------------------------------------------------------------------------ backward, rows i
__global__ void __launch_bounds__(256) sbm_attn_bwd_row_kernel(const float* __restrict__ x, long long ldx, const SaParams P,
                                                               const float* __restrict__ out, const float* __restrict__ lse,
                                                               const float* __restrict__ gout, float* __restrict__ dx,
                                                               float* __restrict__ part_pq, float* __restrict__ part_w,
                                                               float* __restrict__ part_gam, int B, int F, float kappa,
                                                               float tau) {
    __shared__ __attribute__((aligned(16))) KeyTile t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * SA_ROWS + lane;
    const int b0 = blockIdx.y * SA_BC, bw = b0 + wave * SA_NB;
    float a[SA_D], c[SA_D], gam;
    load_a_c(P, a, c, gam);
    gam *= kappa;
    const bool iv = i < F;
    float pq[SA_D];
#pragma unroll
    for (int d = 0; d < SA_D; ++d) pq[d] = iv ? kappa * (P.bq[d] + P.pos[(long long)i * SA_D + d]) : 0.f;
    const float wi = dot16(pq, c);
    float xi[SA_NB], oi[SA_NB], gi[SA_NB], li[SA_NB], dxq[SA_NB], rx[SA_NB], acc[SA_D];
#pragma unroll
    for (int b = 0; b < SA_NB; ++b) {
        const bool v = iv && bw + b < B;
        const long long e = (long long)(bw + b) * F + i;
        xi[b] = v ? x[(long long)(bw + b) * ldx + i] : 0.f;
        oi[b] = v ? out[e] : 0.f;
        gi[b] = v ? gout[e] : 0.f;
        li[b] = v ? lse[e] : INFINITY;                      // P = 0 on a padded (sample, row)
        dxq[b] = 0.f; rx[b] = 0.f;
    }
#pragma unroll
    for (int d = 0; d < SA_D; ++d) acc[d] = 0.f;
    for (int j0 = 0; j0 < F; j0 += SA_T) {
        __syncthreads();
        stage_keys(t, P, x, ldx, B, F, b0, j0, kappa, gam, a);
        const int nj = min(SA_T, F - j0);
        for (int jt = 0; jt < nj; jt += SA_SUB) {
            float mt[SA_SUB], es[SA_SUB];
#pragma unroll
            for (int s = 0; s < SA_SUB; ++s) { mt[s] = m_elem(pq, &t.pk[(jt + s) * SA_D], t.mask[jt + s]); es[s] = 0.f; }
#pragma unroll
            for (int h = 0; h < SA_NB / 4; ++h) {
#pragma unroll
                for (int s = 0; s < SA_SUB; ++s) {
                    const float4 x4 = *reinterpret_cast<const float4*>(&t.xs[(jt + s) * SA_BC + wave * SA_NB + 4 * h]);
                    const float4 a4 = *reinterpret_cast<const float4*>(&t.as[(jt + s) * SA_BC + wave * SA_NB + 4 * h]);
                    const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
                    const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int b = 4 * h + r;
                        const float sc = fmaf(xi[b], av[r], fmaf(wi, xv[r], mt[s]));
                        const float pg = sa_exp2(sc - li[b]) * gi[b];
                        const float e = pg * (xv[r] - oi[b]);
                        dxq[b] = fmaf(e, av[r], dxq[b]);
                        rx[b] = fmaf(e, xv[r], rx[b]);
                        es[s] += e;
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < SA_SUB; ++s) axpy16(acc, es[s], &t.pk[(jt + s) * SA_D]);
        }
    }
    // dx (q side); the column kernel adds the k and v sides
    float rsum = 0.f, gsum = 0.f;
#pragma unroll
    for (int b = 0; b < SA_NB; ++b) {
        if (iv && bw + b < B) dx[(long long)(bw + b) * F + i] = SA_LN2 * dxq[b];
        rsum += rx[b];
        gsum = fmaf(xi[b], rx[b], gsum);
    }
    // per-chunk partials, summed over the four waves in a fixed order
    __syncthreads();
    float* red = t.xs;                                      // 4 waves x 64 rows x 16: xs and as, which are adjacent
    float* red_w = t.pk;                                    // 4 x 64
    float* red_g = t.pk + SA_WAVES * SA_ROWS;               // 256
#pragma unroll
    for (int d = 0; d < SA_D; ++d) red[(wave * SA_ROWS + lane) * SA_D + d] = acc[d];
    red_w[wave * SA_ROWS + lane] = rsum;
    red_g[threadIdx.x] = gsum;
    __syncthreads();
    const long long chF = (long long)blockIdx.y * F;
    for (int idx = threadIdx.x; idx < SA_ROWS * SA_D; idx += blockDim.x) {
        const int r = idx >> 4, d = idx & 15, ii = blockIdx.x * SA_ROWS + r;
        if (ii < F) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < SA_WAVES; ++w) v += red[(w * SA_ROWS + r) * SA_D + d];
            part_pq[(chF + ii) * SA_D + d] = tau * v;
        }
    }
    if (threadIdx.x < SA_ROWS && blockIdx.x * SA_ROWS + (int)threadIdx.x < F) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < SA_WAVES; ++w) v += red_w[w * SA_ROWS + threadIdx.x];
        part_w[chF + blockIdx.x * SA_ROWS + threadIdx.x] = tau * v;
    }
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < o) red_g[threadIdx.x] += red_g[threadIdx.x + o];
    }
    if (threadIdx.x == 0) part_gam[(long long)blockIdx.y * gridDim.x + blockIdx.x] = tau * red_g[0];
}

// --------------------------------------------------------------------------------------------------- backward, columns j
struct QueryTile {
    float pq[SA_T * SA_D];      // kappa Pq_i
    float xs[SA_T * SA_BC];     // x_i
    float bs[SA_T * SA_BC];     // B'_i = gamma' x_i + w'_i
    float ls[SA_T * SA_BC];     // lse2 (+inf on padding)
    float os[SA_T * SA_BC];     // o_i
    float gs[SA_T * SA_BC];     // g_i
    float ws[SA_T];             // w'_i = kappa Pq_i.c
    float mask[SA_T];
};

static_assert(offsetof(QueryTile, bs) == offsetof(QueryTile, xs) + SA_T * SA_BC * sizeof(float) &&
              2 * SA_T * SA_BC >= SA_WAVES * SA_ROWS * SA_D, "the column kernel's end-of-block reduction reuses xs + bs");

__global__ void __launch_bounds__(256) sbm_attn_bwd_col_kernel(const float* __restrict__ x, long long ldx, const SaParams P,
                                                               const float* __restrict__ out, const float* __restrict__ lse,
                                                               const float* __restrict__ gout, float* __restrict__ dx,
                                                               float* __restrict__ part_pk, float* __restrict__ part_u, int B,
                                                               int F, float kappa, float tau) {
    __shared__ __attribute__((aligned(16))) QueryTile t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x * SA_ROWS + lane;
    const int b0 = blockIdx.y * SA_BC, bw = b0 + wave * SA_NB;
    float a[SA_D], c[SA_D], gam;
    load_a_c(P, a, c, gam);
    gam *= kappa;
    const bool jv = j < F;
    float pk[SA_D];
#pragma unroll
    for (int d = 0; d < SA_D; ++d) pk[d] = jv ? P.bk[d] + P.pos[(long long)j * SA_D + d] : 0.f;
    const float uj = kappa * dot16(a, pk);
    float xj[SA_NB], dxk[SA_NB], dv[SA_NB], du[SA_NB], acc[SA_D];
#pragma unroll
    for (int b = 0; b < SA_NB; ++b) {
        xj[b] = (jv && bw + b < B) ? x[(long long)(bw + b) * ldx + j] : 0.f;
        dxk[b] = 0.f; dv[b] = 0.f; du[b] = 0.f;
    }
#pragma unroll
    for (int d = 0; d < SA_D; ++d) acc[d] = 0.f;
    for (int i0 = 0; i0 < F; i0 += SA_T) {
        __syncthreads();
        for (int idx = tid; idx < SA_T * SA_D; idx += blockDim.x) {
            const int ii = idx >> 4, d = idx & 15, i = i0 + ii;
            t.pq[idx] = i < F ? kappa * (P.bq[d] + P.pos[(long long)i * SA_D + d]) : 0.f;
        }
        __syncthreads();
        if (tid < SA_T) {
            t.ws[tid] = dot16(&t.pq[tid * SA_D], c);
            t.mask[tid] = i0 + tid < F ? 0.f : -INFINITY;
        }
        __syncthreads();
        for (int idx = tid; idx < SA_T * SA_BC; idx += blockDim.x) {
            const int b = idx / SA_T, ii = idx - b * SA_T, i = i0 + ii, bg = b0 + b;
            const bool v = i < F && bg < B;
            const long long e = (long long)bg * F + i;
            const float xv = v ? x[(long long)bg * ldx + i] : 0.f;
            const int s = ii * SA_BC + b;
            t.xs[s] = xv;
            t.bs[s] = fmaf(gam, xv, t.ws[ii]);
            t.ls[s] = v ? lse[e] : INFINITY;
            t.os[s] = v ? out[e] : 0.f;
            t.gs[s] = v ? gout[e] : 0.f;
        }
        __syncthreads();
        const int ni = min(SA_T, F - i0);
#pragma unroll 2
        for (int ii = 0; ii < ni; ++ii) {
            const float mt = m_elem(pk, &t.pq[ii * SA_D], t.mask[ii]);
            float es = 0.f;
#pragma unroll
            for (int h = 0; h < SA_NB / 4; ++h) {
                const int o4 = ii * SA_BC + wave * SA_NB + 4 * h;
                const float4 x4 = *reinterpret_cast<const float4*>(&t.xs[o4]);
                const float4 b4 = *reinterpret_cast<const float4*>(&t.bs[o4]);
                const float4 l4 = *reinterpret_cast<const float4*>(&t.ls[o4]);
                const float4 q4 = *reinterpret_cast<const float4*>(&t.os[o4]);
                const float4 g4 = *reinterpret_cast<const float4*>(&t.gs[o4]);
                const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
                const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, ov[4] = {q4.x, q4.y, q4.z, q4.w};
                const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int b = 4 * h + r;
                    const float sc = fmaf(xv[r], uj, fmaf(xj[b], bv[r], mt));
                    const float pg = sa_exp2(sc - lv[r]) * gv[r];
                    dv[b] += pg;
                    const float e = pg * (xj[b] - ov[r]);
                    dxk[b] = fmaf(e, bv[r], dxk[b]);
                    du[b] = fmaf(e, xv[r], du[b]);
                    es += e;
                }
            }
            axpy16(acc, es, &t.pq[ii * SA_D]);
        }
    }
    float usum = 0.f;
#pragma unroll
    for (int b = 0; b < SA_NB; ++b) {
        if (jv && bw + b < B) {
            const long long e = (long long)(bw + b) * F + j;
            dx[e] = dx[e] + fmaf(SA_LN2, dxk[b], dv[b]);   // the row kernel wrote the q side (same stream, earlier launch)
        }
        usum += du[b];
    }
    __syncthreads();
    float* red = t.xs;                                      // 4 x 64 x 16: xs and bs, which are adjacent
    float* red_u = t.ls;
#pragma unroll
    for (int d = 0; d < SA_D; ++d) red[(wave * SA_ROWS + lane) * SA_D + d] = acc[d];
    red_u[wave * SA_ROWS + lane] = usum;
    __syncthreads();
    const long long chF = (long long)blockIdx.y * F;
    for (int idx = tid; idx < SA_ROWS * SA_D; idx += blockDim.x) {
        const int r = idx >> 4, d = idx & 15, jj = blockIdx.x * SA_ROWS + r;
        if (jj < F) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < SA_WAVES; ++w) v += red[(w * SA_ROWS + r) * SA_D + d];
            part_pk[(chF + jj) * SA_D + d] = SA_LN2 * v;       // tau / kappa: the staged Pq rows carry kappa
        }
    }
    if (tid < SA_ROWS && blockIdx.x * SA_ROWS + tid < F) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < SA_WAVES; ++w) v += red_u[w * SA_ROWS + tid];
        part_u[chF + blockIdx.x * SA_ROWS + tid] = tau * v;
    }
}

// ------------------------------------------------------------------------------------------------ backward, reductions
constexpr int SA_RROWS = 16;    // rows per reduce block (x 16 widths = 256 threads)

__global__ void __launch_bounds__(256) sbm_attn_bwd_reduce_kernel(const SaParams P, const float* __restrict__ part_pq,
                                                                  const float* __restrict__ part_pk,
                                                                  const float* __restrict__ part_w,
                                                                  const float* __restrict__ part_u, float* __restrict__ gpos,
                                                                  float* __restrict__ part2, int F, int nch) {
    __shared__ float red[4][SA_RROWS][SA_D];
    const int r = threadIdx.x >> 4, d = threadIdx.x & 15, i = blockIdx.x * SA_RROWS + r;
    float q = 0.f, k = 0.f, ua = 0.f, wc = 0.f;
    if (i < F) {
        float dw = 0.f, du = 0.f, sq = 0.f, sk = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            const long long row = (long long)ch * F + i;
            dw += part_w[row];
            du += part_u[row];
            sq += part_pq[row * SA_D + d];
            sk += part_pk[row * SA_D + d];
        }
        const float pos = P.pos[(long long)i * SA_D + d];
        q = fmaf(dw, P.wk[d], sq);                         // dPq_i = contraction + dw_i c
        k = fmaf(du, P.wq[d], sk);                         // dPk_i = contraction + du_i a
        gpos[(long long)i * SA_D + d] = q + k;
        ua = du * (P.bk[d] + pos);                         // du_j Pk_j  -> da
        wc = dw * (P.bq[d] + pos);                         // dw_i Pq_i  -> dc
    }
    red[0][r][d] = q; red[1][r][d] = k; red[2][r][d] = ua; red[3][r][d] = wc;
    __syncthreads();
    if (threadIdx.x < 4 * SA_D) {
        const int qi = threadIdx.x >> 4, dd = threadIdx.x & 15;
        float v = 0.f;
        for (int rr = 0; rr < SA_RROWS; ++rr) v += red[qi][rr][dd];
        part2[(long long)blockIdx.x * 4 * SA_D + threadIdx.x] = v;
    }
}

__global__ void __launch_bounds__(256) sbm_attn_bwd_final_kernel(const SaParams P, const float* __restrict__ part2, int nred,
                                                                 const float* __restrict__ part_gam, int ngam,
                                                                 float* __restrict__ gwq, float* __restrict__ gbq,
                                                                 float* __restrict__ gwk, float* __restrict__ gbk) {
    __shared__ float sums[4 * SA_D];
    __shared__ float red[256];
    const int tid = threadIdx.x;
    float g = 0.f;
    for (int n = tid; n < ngam; n += 256) g += part_gam[n];
    red[tid] = g;
    if (tid < 4 * SA_D) {
        float v = 0.f;
        for (int n = 0; n < nred; ++n) v += part2[(long long)n * 4 * SA_D + tid];
        sums[tid] = v;
    }
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) red[tid] += red[tid + o];
    }
    __syncthreads();
    if (tid < SA_D) {
        const float dgam = red[0];
        gbq[tid] = sums[tid];
        gbk[tid] = sums[SA_D + tid];
        gwq[tid] = fmaf(dgam, P.wk[tid], sums[2 * SA_D + tid]);   // da = dgamma c + sum_j du_j Pk_j
        gwk[tid] = fmaf(dgam, P.wq[tid], sums[3 * SA_D + tid]);   // dc = dgamma a + sum_i dw_i Pq_i
    }
}

int sa_nch(int B) { return (B + SA_BC - 1) / SA_BC; }
int sa_nrow_blocks(int F) { return (F + SA_ROWS - 1) / SA_ROWS; }
int sa_nred_blocks(int F) { return (F + SA_RROWS - 1) / SA_RROWS; }

bool sa_check(const char* who, const float* x, long long ldx, const SaParams& P, int B, int F, int D, float scale) {
    if (!x || !P.wq || !P.bq || !P.wk || !P.bk || !P.pos) {
        ign_set_error("%s: null pointer", who);
        return false;
    }
    if (B < 1 || F < 1 || ldx < F) {
        ign_set_error("%s: bad dimensions (B=%d F=%d ldx=%lld; need B, F >= 1 and ldx >= F)", who, B, F, ldx);
        return false;
    }
    if (!(scale > 0.f) || !isfinite(scale)) {
        ign_set_error("%s: scale = %g must be positive and finite", who, (double)scale);
        return false;
    }
    return true;
}

}  // namespace

extern "C" size_t ign_sbm_attn_workspace_bytes(int B, int F) {
    if (B < 1 || F < 1) return 0;
    const size_t nch = (size_t)sa_nch(B);
    const size_t floats = nch * (size_t)F * (2 * SA_D + 2) + nch * (size_t)sa_nrow_blocks(F) + (size_t)sa_nred_blocks(F) * 4 * SA_D;
    return floats * sizeof(float);
}

extern "C" int ign_sbm_attn_fwd(const float* x, long long ldx, const float* wq, const float* bq, const float* wk, const float* bk,
                                const float* pos, float* out, float* lse, int B, int F, int D, float scale, void* stream) {
    static const char* who = "ign_sbm_attn_fwd";
    const SaParams P{wq, bq, wk, bk, pos};
    if (!sa_check(who, x, ldx, P, B, F, D, scale)) return IGN_E_ARG;
    if (!out) { ign_set_error("%s: null pointer (out)", who); return IGN_E_ARG; }
    if (D != SA_D) { ign_set_error("%s: D=%d: only the 16-wide head of SelfAttention is implemented", who, D); return IGN_E_UNSUP; }
    IgnScopedTimer tm("sbm_attn", (hipStream_t)stream);
    hipLaunchKernelGGL(sbm_attn_fwd_kernel, dim3(sa_nrow_blocks(F), sa_nch(B)), dim3(256), 0, (hipStream_t)stream, x, ldx, P, out,
                       lse, B, F, scale * SA_LOG2E);
    return ign_check_launch("sbm_attn_fwd_kernel");
}

extern "C" int ign_sbm_attn_bwd(const float* x, long long ldx, const float* wq, const float* bq, const float* wk, const float* bk,
                                const float* pos, const float* out, const float* lse, const float* gout, float* gx, float* gwq,
                                float* gbq, float* gwk, float* gbk, float* gpos, void* workspace, int B, int F, int D, float scale,
                                void* stream) {
    static const char* who = "ign_sbm_attn_bwd";
    const SaParams P{wq, bq, wk, bk, pos};
    if (!sa_check(who, x, ldx, P, B, F, D, scale)) return IGN_E_ARG;
    if (!out || !lse || !gout || !gx || !gwq || !gbq || !gwk || !gbk || !gpos || !workspace) {
        ign_set_error("%s: null pointer (saved, gradient or workspace)", who);
        return IGN_E_ARG;
    }
    if (D != SA_D) { ign_set_error("%s: D=%d: only the 16-wide head of SelfAttention is implemented", who, D); return IGN_E_UNSUP; }
    const int nch = sa_nch(B), nrb = sa_nrow_blocks(F), nred = sa_nred_blocks(F);
    float* part_pq = (float*)workspace;
    float* part_pk = part_pq + (size_t)nch * F * SA_D;
    float* part_w = part_pk + (size_t)nch * F * SA_D;
    float* part_u = part_w + (size_t)nch * F;
    float* part_gam = part_u + (size_t)nch * F;
    float* part2 = part_gam + (size_t)nch * nrb;
    const float kappa = scale * SA_LOG2E;
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("sbm_attn", s);
    hipLaunchKernelGGL(sbm_attn_bwd_row_kernel, dim3(nrb, nch), dim3(256), 0, s, x, ldx, P, out, lse, gout, gx, part_pq, part_w,
                       part_gam, B, F, kappa, scale);
    int rc = ign_check_launch("sbm_attn_bwd_row_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(sbm_attn_bwd_col_kernel, dim3(nrb, nch), dim3(256), 0, s, x, ldx, P, out, lse, gout, gx, part_pk, part_u, B,
                       F, kappa, scale);
    if ((rc = ign_check_launch("sbm_attn_bwd_col_kernel"))) return rc;
    hipLaunchKernelGGL(sbm_attn_bwd_reduce_kernel, dim3(nred), dim3(256), 0, s, P, part_pq, part_pk, part_w, part_u, gpos, part2, F,
                       nch);
    if ((rc = ign_check_launch("sbm_attn_bwd_reduce_kernel"))) return rc;
    hipLaunchKernelGGL(sbm_attn_bwd_final_kernel, dim3(1), dim3(256), 0, s, P, part2, nred, part_gam, nch * nrb, gwq, gbq, gwk, gbk);
    return ign_check_launch("sbm_attn_bwd_final_kernel");
}
