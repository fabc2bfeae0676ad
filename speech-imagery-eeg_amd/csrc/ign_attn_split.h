// Split-operand helpers of the attention kernels on the 16-bit matrix cores (ign_attention_x6.hip, ign_attention_map.hip): operand
// vector types, the MFMA of a plane pair, the power-of-two operand scales of the h3 arithmetic and the fp32 -> 1 / 2 / 3-plane
// splits.  Every kernel that must reproduce the forward's scores (the attention-map kernel) uses these definitions.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// ---- NP = 2: two fp16 planes of power-of-two-scaled operands, THREE products (include/ign_abi.h, "h3").  Scales come from
// device-side magnitude bounds (pow2_scale); scores are un-scaled inside the exp2 (an FMA instead of a subtraction), the
// probabilities (<= 1) are split after a multiplication by 2^14, products of bounds give hard bounds for derived operands
// (|dS| <= 2 E max|dO| max|V|).  The planes are 16-bit slots of the same LDS / register layouts as the bf16 planes.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <int NP>
__device__ __forceinline__ f32x16 mfma16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    if constexpr (NP == 2)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
#define MFMA16(a, b, c) mfma16<NP>((a), (b), (c))
__device__ __forceinline__ float pow2_scale_v(float b) {      // 2^e with 2^13 <= b 2^e < 2^14 (1 for zero / non-finite b)
    if (!(b > 0.f) || !(b < INFINITY)) return 1.f;
    int e;
    (void)frexpf(b, &e);
    e = 14 - e;
    e = e < -60 ? -60 : (e > 60 ? 60 : e);
    return ldexpf(1.f, e);
}
__device__ __forceinline__ void split2h_pair(f32x2 v, f16x2& x0, f16x2& x1) {
    x0 = __builtin_convertvector(v, f16x2);
    x1 = __builtin_convertvector(v - __builtin_convertvector(x0, f32x2), f16x2);
}

__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// x = x0 + x1 + x2 (bf16, round to nearest; the residuals are exact fp32 subtractions) for a pair of values
__device__ __forceinline__ void split3_pair(f32x2 v, bf16x2& x0, bf16x2& x1, bf16x2& x2) {
    x0 = __builtin_convertvector(v, bf16x2);
    f32x2 r = v - __builtin_convertvector(x0, f32x2);
    x1 = __builtin_convertvector(r, bf16x2);
    r -= __builtin_convertvector(x1, f32x2);
    x2 = __builtin_convertvector(r, bf16x2);
}
// eight values -> one bf16x8 MFMA operand per plane.  NP = 3: the exact three-way split (six products, fp32 accuracy);
// NP = 1: the values rounded to bf16 (one product: the arithmetic of the reference's bf16-autocast mode); p1, p2 stay unused.
template <int NP>
__device__ __forceinline__ void splitN_x8(const float (&t)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
    if constexpr (NP == 2) {
        f16x2 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split2h_pair(f32x2{t[2 * i], t[2 * i + 1]}, a[i], b[i]);
        p0 = __builtin_bit_cast(bf16x8, __builtin_shufflevector(__builtin_shufflevector(a[0], a[1], 0, 1, 2, 3),
                                                                __builtin_shufflevector(a[2], a[3], 0, 1, 2, 3), 0, 1, 2, 3, 4, 5, 6, 7));
        p1 = __builtin_bit_cast(bf16x8, __builtin_shufflevector(__builtin_shufflevector(b[0], b[1], 0, 1, 2, 3),
                                                                __builtin_shufflevector(b[2], b[3], 0, 1, 2, 3), 0, 1, 2, 3, 4, 5, 6, 7));
        p2 = p0;
        return;
    }
    if constexpr (NP == 1) {
        bf16x2 a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = __builtin_convertvector(f32x2{t[2 * i], t[2 * i + 1]}, bf16x2);
        p0 = __builtin_shufflevector(__builtin_shufflevector(a[0], a[1], 0, 1, 2, 3), __builtin_shufflevector(a[2], a[3], 0, 1, 2, 3),
                                     0, 1, 2, 3, 4, 5, 6, 7);
        p1 = p0; p2 = p0;
        return;
    }
    bf16x2 a[4], b[4], c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split3_pair(f32x2{t[2 * i], t[2 * i + 1]}, a[i], b[i], c[i]);
    p0 = __builtin_shufflevector(__builtin_shufflevector(a[0], a[1], 0, 1, 2, 3), __builtin_shufflevector(a[2], a[3], 0, 1, 2, 3),
                                 0, 1, 2, 3, 4, 5, 6, 7);
    p1 = __builtin_shufflevector(__builtin_shufflevector(b[0], b[1], 0, 1, 2, 3), __builtin_shufflevector(b[2], b[3], 0, 1, 2, 3),
                                 0, 1, 2, 3, 4, 5, 6, 7);
    p2 = __builtin_shufflevector(__builtin_shufflevector(c[0], c[1], 0, 1, 2, 3), __builtin_shufflevector(c[2], c[3], 0, 1, 2, 3),
                                 0, 1, 2, 3, 4, 5, 6, 7);
}

// four values -> NP LDS planes `plane` elements apart (8-byte stores)
template <int NP>
__device__ __forceinline__ void splitN_store4(const float4 t, __bf16* d, int plane) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    if constexpr (NP == 2) {
        typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
        f16x2 a0, a1, b0, b1;
        split2h_pair(f32x2{t.x, t.y}, a0, a1);
        split2h_pair(f32x2{t.z, t.w}, b0, b1);
        _Float16* dh = reinterpret_cast<_Float16*>(d);
        *reinterpret_cast<f16x4*>(dh) = __builtin_shufflevector(a0, b0, 0, 1, 2, 3);
        *reinterpret_cast<f16x4*>(dh + plane) = __builtin_shufflevector(a1, b1, 0, 1, 2, 3);
        return;
    }
    if constexpr (NP == 1) {
        const bf16x2 a = __builtin_convertvector(f32x2{t.x, t.y}, bf16x2), b = __builtin_convertvector(f32x2{t.z, t.w}, bf16x2);
        *reinterpret_cast<bf16x4*>(d) = __builtin_shufflevector(a, b, 0, 1, 2, 3);
        return;
    }
    bf16x2 a0, a1, a2, b0, b1, b2;
    split3_pair(f32x2{t.x, t.y}, a0, a1, a2);
    split3_pair(f32x2{t.z, t.w}, b0, b1, b2);
    *reinterpret_cast<bf16x4*>(d) = __builtin_shufflevector(a0, b0, 0, 1, 2, 3);
    *reinterpret_cast<bf16x4*>(d + plane) = __builtin_shufflevector(a1, b1, 0, 1, 2, 3);
    *reinterpret_cast<bf16x4*>(d + 2 * plane) = __builtin_shufflevector(a2, b2, 0, 1, 2, 3);
}
