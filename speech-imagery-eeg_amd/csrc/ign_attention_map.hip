// Attention map  A = dropout(softmax(scale * Q K^T))  as a (B, H, L, S) fp32 tensor: the `attn` that FullAttention returns with
// output_attention=True (IGN/layers/SelfAttention_Family.py:56-75).  The fused forward kernels never store the scores; they save
// the row log-sum-exp.  This kernel recomputes each 32 x 32 score tile with the arithmetic that produced that lse (fp32 MFMA, the
// three-plane bf16 split, bf16 rounding, or the two-plane fp16 split with the forward's power-of-two operand scales),
// turns it into probabilities exp(s - lse), applies the call's keep mask (ign_dropout.h) and writes the tile.
//
// It is a pure write stream (8.19 GB per layer at B 256, H 8, L = S = 1000), so the tile is oriented for the store: S = Q K^T with
// the queries on the accumulator rows and the key on the lane (the orientation of attn_bwd_dkdv_kernel).  Accumulator register r
// of lane (c = lane&31, h = lane>>5) holds query row (r&3) + 8(r>>2) + 4h, key column c: one store per register writes two
// 128-byte row segments, the shape plain stores run at full rate with.  Block = 4 waves x 32 queries; the block's K tiles are
// staged in LDS (split into planes while they are staged, as in the forward) and every wave runs over all keys.
#include "ign_common.h"
#include "ign_dropout.h"
#include "ign_attn_split.h"

struct AttnMapArgs {
    const float *q, *k, *lse;                // q (B,L,H,E), k (B,S,H,E) with element strides sb, sl; head stride E; lse (B,H,L)
    float* attn;                             // (B,H,L,S) contiguous
    long long q_sb, q_sl, k_sb, k_sl;
    int L, S, H;
    float scale;
    const float *bq, *bk;                    // h3: device-side bounds of |q|, |k| (the forward's)
    unsigned long long seed;                 // DROPOUT instantiations: per-call seed, keep threshold, 1 / (1 - p_eff)
    unsigned thr;
    float dscale;
};

constexpr int MAP_KT = 64;                   // keys staged per LDS tile

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

template <int E, int MATH, bool DROPOUT>
__global__ void __launch_bounds__(256) attn_map_kernel(const AttnMapArgs a) {
    constexpr bool F32 = MATH == IGN_ATTN_MATH_F32;
    constexpr int NP = MATH == IGN_ATTN_MATH_X6 ? 3 : (MATH == IGN_ATTN_MATH_H3 ? 2 : 1);
    constexpr int EH = E / 2, NS = E / 16, V4 = E / 4;
    constexpr int PF = E + 4;                                     // fp32 tile pitch (the fp32 forward's)
    constexpr int PK = E + 8, KPLANE = MAP_KT * PK;               // 16-bit plane pitch (the split forward's)
    __shared__ __attribute__((aligned(16))) float smem[F32 ? MAP_KT * PF : NP * KPLANE / 2];
    __bf16* Ks = reinterpret_cast<__bf16*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y, bh = b * a.H + head;
    const int q0 = blockIdx.x * 128 + wave * 32;                  // the wave's 32 queries = the tile's rows
    const long long qrow = q0 + l31 < a.L ? q0 + l31 : a.L - 1;   // this lane's query in the A operand

    // Q operand, as the forward forms it: fp32 (scale folded in), or the split planes of q * scale * log2(e) (* sq for h3)
    const float sc2u = a.scale * 1.44269504088896341f;
    const float sq = (NP == 2) ? pow2_scale_v(*a.bq * fabsf(sc2u)) : 1.f;
    const float sk = (NP == 2) ? pow2_scale_v(*a.bk) : 1.f;
    const float us = (NP == 2) ? 1.f / (sq * sk) : 1.f;
    float Qf[F32 ? EH : 1];
    bf16x8 Qp[3][F32 ? 1 : NS];
    const float* qp = a.q + b * a.q_sb + qrow * a.q_sl + head * E;
    if constexpr (F32) {
#pragma unroll
        for (int kk = 0; kk < EH; kk += 4) {
            const float4 t = *reinterpret_cast<const float4*>(qp + h * EH + kk);
            Qf[kk] = t.x * a.scale; Qf[kk + 1] = t.y * a.scale; Qf[kk + 2] = t.z * a.scale; Qf[kk + 3] = t.w * a.scale;
        }
    } else {
        const float sc2 = sc2u * sq;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float4 t0 = *reinterpret_cast<const float4*>(qp + 8 * h + 16 * s);
            const float4 t1 = *reinterpret_cast<const float4*>(qp + 8 * h + 16 * s + 4);
            const float t[8] = {t0.x * sc2, t0.y * sc2, t0.z * sc2, t0.w * sc2, t1.x * sc2, t1.y * sc2, t1.z * sc2, t1.w * sc2};
            splitN_x8<NP>(t, Qp[0][s], Qp[1][s], Qp[2][s]);
        }
    }
    // lse of this lane's 16 rows (base 2 for the split arithmetics, whose scores are in base 2)
    float lr[16];
    const float* lse_b = a.lse + (long long)bh * a.L;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = q0 + acc_row(r, h);
        lr[r] = lse_b[i < a.L ? i : a.L - 1] * (F32 ? 1.f : 1.44269504088896341f);
    }

    const float* kbase = a.k + b * a.k_sb + head * E;
    float* const orow = a.attn + ((long long)bh * a.L + q0 + 4 * h) * a.S;   // row q0 + 4h; register r adds (r&3) + 8(r>>2) rows
    for (int kt0 = 0; kt0 < a.S; kt0 += MAP_KT) {
        __syncthreads();                                          // every wave is done with the previous tile
        for (int i = threadIdx.x; i < MAP_KT * V4; i += 256) {
            const int r = i / V4, c4 = (i - r * V4) * 4;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kt0 + r < a.S) t = *reinterpret_cast<const float4*>(kbase + (long long)(kt0 + r) * a.k_sl + c4);
            if constexpr (F32) {
                *reinterpret_cast<float4*>(smem + r * PF + c4) = t;
            } else {
                if constexpr (NP == 2) t = make_float4(t.x * sk, t.y * sk, t.z * sk, t.w * sk);
                splitN_store4<NP>(t, Ks + r * PK + c4, KPLANE);
            }
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < MAP_KT / 32; ++sub) {
            const int kb = kt0 + sub * 32;
            if (kb >= a.S) break;                                 // wave-uniform
            // S tile: A = Q (row = query), B = K (column = key): the forward's products with the operands swapped
            f32x16 acc, acc2;
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc2[r] = 0.f; }
            if constexpr (F32) {
                const float* kr = smem + (sub * 32 + l31) * PF + h * EH;
#pragma unroll
                for (int kk = 0; kk < EH; kk += 4) {
                    const float4 kv = *reinterpret_cast<const float4*>(kr + kk);
                    acc = MFMA32(Qf[kk], kv.x, acc);
                    acc = MFMA32(Qf[kk + 1], kv.y, acc);
                    acc = MFMA32(Qf[kk + 2], kv.z, acc);
                    acc = MFMA32(Qf[kk + 3], kv.w, acc);
                }
            } else {
                const __bf16* kr = Ks + (sub * 32 + l31) * PK + 8 * h;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(kr + 16 * s);
                    if constexpr (NP == 3) {
                        const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(kr + KPLANE + 16 * s);
                        const bf16x8 k2 = *reinterpret_cast<const bf16x8*>(kr + 2 * KPLANE + 16 * s);
                        acc = MFMA16(Qp[0][s], k2, acc);
                        acc2 = MFMA16(Qp[2][s], k0, acc2);
                        acc = MFMA16(Qp[1][s], k1, acc);
                        acc2 = MFMA16(Qp[0][s], k1, acc2);
                        acc = MFMA16(Qp[1][s], k0, acc);
                        acc2 = MFMA16(Qp[0][s], k0, acc2);
                    } else if constexpr (NP == 2) {
                        const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(kr + KPLANE + 16 * s);
                        acc = MFMA16(Qp[0][s], k1, acc);
                        acc2 = MFMA16(Qp[1][s], k0, acc2);
                        if (s & 1) acc2 = MFMA16(Qp[0][s], k0, acc2);
                        else acc = MFMA16(Qp[0][s], k0, acc);
                    } else {
                        if (s & 1) acc2 = MFMA16(Qp[0][s], k0, acc2);
                        else acc = MFMA16(Qp[0][s], k0, acc);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] += acc2[r];
            }
            // P = exp(s - lse); h3: the accumulators hold sq sk S, un-scaled inside the exp2 as in the backward
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if constexpr (F32) acc[r] = __expf(acc[r] - lr[r]);
                else if constexpr (NP == 2) acc[r] = __builtin_amdgcn_exp2f(fmaf(acc[r], us, -lr[r]));
                else acc[r] = __builtin_amdgcn_exp2f(acc[r] - lr[r]);
            }
            if constexpr (DROPOUT) {
                // The lanes of a quad hold keys j4 .. j4 + 3; registers 4g .. 4g + 3 hold queries 8g + 4h + 0 .. 3.  Lane t of the
                // quad evaluates query 8g + 4h + t (ign_drop_row4: one Philox call per 4 x 4 block and lane, as the forward), the quad
                // exchanges the nibbles, and bit 4t + u of w[g >> 1] >> 16 (g & 1) is query t, key j4 + u.
                const int t4 = l31 & 3;
                const uint32_t j4 = (uint32_t)(kb + (l31 & ~3));
                uint32_t w[2];
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2) {
                    const uint32_t lo = ign_drop_row4(a.seed, bh, q0 + 16 * g2 + 4 * h + t4, j4, a.thr);
                    const uint32_t hi = ign_drop_row4(a.seed, bh, q0 + 16 * g2 + 8 + 4 * h + t4, j4, a.thr);
                    uint32_t x = (lo << (4 * t4)) | (hi << (16 + 4 * t4));
                    x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false);    // quad_perm [1, 0, 3, 2]
                    x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, false);    // quad_perm [2, 3, 0, 1]
                    w[g2] = x >> (l31 & 3);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int g = r >> 2, t = r & 3;
                    const bool keep = (w[g >> 1] >> (16 * (g & 1) + 4 * t)) & 1u;
                    acc[r] = keep ? acc[r] * a.dscale : 0.f;
                }
            }
            const int j = kb + l31;
            if (j < a.S) {
                float* op = orow + j;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (q0 + acc_row(r, h) < a.L) op[(long long)((r & 3) + 8 * (r >> 2)) * a.S] = acc[r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ C ABI (include/ign_abi.h)
template <int MATH, bool DROPOUT>
static void map_launch(int E, dim3 grid, hipStream_t s, const AttnMapArgs& a) {
    switch (E) {
        case 16: hipLaunchKernelGGL((attn_map_kernel<16, MATH, DROPOUT>), grid, dim3(256), 0, s, a); break;
        case 32: hipLaunchKernelGGL((attn_map_kernel<32, MATH, DROPOUT>), grid, dim3(256), 0, s, a); break;
        case 64: hipLaunchKernelGGL((attn_map_kernel<64, MATH, DROPOUT>), grid, dim3(256), 0, s, a); break;
        default:
            if constexpr (MATH == IGN_ATTN_MATH_F32 || MATH == IGN_ATTN_MATH_X6)      // BF16 / H3: E <= 64 (checked)
                hipLaunchKernelGGL((attn_map_kernel<128, MATH, DROPOUT>), grid, dim3(256), 0, s, a);
            break;
    }
}

template <bool DROPOUT>
static void map_launch_math(int math, int E, dim3 grid, hipStream_t s, const AttnMapArgs& a) {
    switch (math) {
        case IGN_ATTN_MATH_F32: map_launch<IGN_ATTN_MATH_F32, DROPOUT>(E, grid, s, a); break;
        case IGN_ATTN_MATH_X6: map_launch<IGN_ATTN_MATH_X6, DROPOUT>(E, grid, s, a); break;
        case IGN_ATTN_MATH_BF16: map_launch<IGN_ATTN_MATH_BF16, DROPOUT>(E, grid, s, a); break;
        default: map_launch<IGN_ATTN_MATH_H3, DROPOUT>(E, grid, s, a); break;
    }
}

extern "C" int ign_attn_probs(const float* q, const float* k, const float* lse, float* attn, int B, int L, int S, int H, int E,
                              long long q_sb, long long q_sl, long long k_sb, long long k_sl, float scale, void* stream, int math,
                              const float* bq, const float* bk, float p, unsigned long long seed) {
    static const char* who = "ign_attn_probs";
    if (!q || !k || !lse || !attn || ((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)lse & 3) || ((uintptr_t)attn & 3)) {
        ign_set_error("%s: a pointer is null or misaligned (q, k: 16 bytes; lse, attn: 4 bytes)", who);
        return IGN_E_ARG;
    }
    if (B <= 0 || L <= 0 || S <= 0 || H <= 0 || H > 65535 || B > 65535) {
        ign_set_error("%s: bad dimensions B=%d L=%d S=%d H=%d", who, B, L, S, H);
        return IGN_E_ARG;
    }
    if (E != 16 && E != 32 && E != 64 && E != 128) {
        ign_set_error("%s: head dimension E=%d not instantiated (16, 32, 64, 128)", who, E);
        return IGN_E_UNSUP;
    }
    if (math < IGN_ATTN_MATH_F32 || math > IGN_ATTN_MATH_H3) { ign_set_error("%s: unknown arithmetic %d", who, math); return IGN_E_ARG; }
    if ((math == IGN_ATTN_MATH_H3 || math == IGN_ATTN_MATH_BF16) && E > 64) {
        ign_set_error("%s: E=%d > 64 with the %s arithmetic", who, E, math == IGN_ATTN_MATH_H3 ? "h3" : "bf16");
        return IGN_E_UNSUP;
    }
    if (math == IGN_ATTN_MATH_H3 && (!bq || !bk)) { ign_set_error("%s: null operand bound", who); return IGN_E_ARG; }
    const long long st[4] = {q_sb, q_sl, k_sb, k_sl};
    for (int i = 0; i < 4; ++i)
        if (st[i] <= 0 || (st[i] & 3)) {
            ign_set_error("%s: stride %d = %lld must be a positive multiple of 4 elements", who, i, st[i]);
            return IGN_E_ARG;
        }
    if (!(p >= 0.f && p < 1.f)) { ign_set_error("%s: dropout p = %g outside [0, 1)", who, (double)p); return IGN_E_ARG; }
    const unsigned thr = ign_dropout_threshold(p);
    if (thr >= 65536u) { ign_set_error("%s: dropout p = %g rounds to a keep rate of 0 (p = thr / 65536)", who, (double)p); return IGN_E_ARG; }
    AttnMapArgs a = {};
    a.q = q; a.k = k; a.lse = lse; a.attn = attn;
    a.q_sb = q_sb; a.q_sl = q_sl; a.k_sb = k_sb; a.k_sl = k_sl;
    a.L = L; a.S = S; a.H = H; a.scale = scale;
    a.bq = bq; a.bk = bk;
    a.seed = seed; a.thr = thr; a.dscale = ign_dropout_scale(thr);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((L + 127) / 128, H, B);
    IgnScopedTimer tm("attn_probs", s);
    if (thr) map_launch_math<true>(math, E, grid, s, a);
    else map_launch_math<false>(math, E, grid, s, a);
    return ign_check_launch("attn_map_kernel");
}
