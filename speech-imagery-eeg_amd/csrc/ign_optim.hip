// Everything that works on the flat parameter / gradient / moment buffers of the training step: the Adam update, the gather of
// per-parameter gradients into the flat bucket, the gradient norm with its clip coefficient, and the in-place scale.
//
//  * Adam       one launch over the flat buffers (torch.optim.Adam semantics, IGN/exp/experiment_classification.py:136,338): one
//    element rule (adam_element), one kernel (adam_kernel<CLIP, DEV>), one launcher (adam_launch) behind the four ign_adam_step*
//    entry points.
//  * AdamW      the same element rule behind ign_adamw_step_dev (adamw_kernel<CLIP>): decoupled weight decay under a per-chunk mask,
//    the learning rate of a per-step schedule and the EMA decay computed on the device by the scheduled tick (ign_sched.h), the
//    EMA of the parameters (ign_ema_update) and the in-place exchange of two flat buffers (ign_swap_flat).
#include "ign_common.h"
#include "ign_sched.h"

// ------------------------------------------------------------------------------------------------ Adam
// The update of one element; `step` = lr / bias_correction1, `bc2_sqrt` = sqrt(bias_correction2).
__device__ __forceinline__ void adam_element(float& p, const float g, float& m, float& v, const float b1, const float b2,
                                             const float step, const float bc2_sqrt, const float eps) {
    m = b1 * m + (1.f - b1) * g;
    v = b2 * v + (1.f - b2) * g * g;
    p -= step * m / (sqrtf(v) / bc2_sqrt + eps);
}

// Four elements per lane as one 16-byte access per buffer; the lane that holds the end of the buffer walks its 1..3 elements alone.
// CLIP: the gradient is read as g * coef[0], the clip coefficient ign_grad_norm_clip left on the device -- clipping costs no pass
// over the gradients and no write to them.
// DEV: the bias corrections come from bc_dev[0..1], where adam_tick_kernel left them (the graph-capturable step), not from the
// arguments bc1 / bc2_sqrt.
template <bool CLIP, bool DEV>
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long long n, float lr, float b1, float b2,
                                                   float eps, float bc1, float bc2_sqrt, const float* __restrict__ coef,
                                                   const float* __restrict__ bc_dev) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (DEV) { bc1 = bc_dev[0]; bc2_sqrt = bc_dev[1]; }
    const float step = lr / bc1;
    const float c = CLIP ? coef[0] : 1.f;
    if (i + 3 < n) {
        float4 pv = *reinterpret_cast<float4*>(p + i);
        float4 gv = *reinterpret_cast<const float4*>(g + i);
        if (CLIP) { gv.x *= c; gv.y *= c; gv.z *= c; gv.w *= c; }
        float4 mv = *reinterpret_cast<float4*>(m + i);
        float4 vv = *reinterpret_cast<float4*>(v + i);
        adam_element(pv.x, gv.x, mv.x, vv.x, b1, b2, step, bc2_sqrt, eps);
        adam_element(pv.y, gv.y, mv.y, vv.y, b1, b2, step, bc2_sqrt, eps);
        adam_element(pv.z, gv.z, mv.z, vv.z, b1, b2, step, bc2_sqrt, eps);
        adam_element(pv.w, gv.w, mv.w, vv.w, b1, b2, step, bc2_sqrt, eps);
        *reinterpret_cast<float4*>(p + i) = pv;
        *reinterpret_cast<float4*>(m + i) = mv;
        *reinterpret_cast<float4*>(v + i) = vv;
    } else {
        for (long long j = i; j < n; ++j) {
            float pv = p[j], gv = CLIP ? g[j] * c : g[j], mv = m[j], vv = v[j];
            adam_element(pv, gv, mv, vv, b1, b2, step, bc2_sqrt, eps);
            p[j] = pv; m[j] = mv; v[j] = vv;
        }
    }
}

// Graph-capturable Adam: the step count lives on the device, so a captured launch sequence stays valid when replayed.
__global__ void adam_tick_kernel(int* __restrict__ step_dev, float* __restrict__ bc_dev, float b1, float b2) {
    const int step = ++(*step_dev);
    bc_dev[0] = (float)(1.0 - pow((double)b1, (double)step));
    bc_dev[1] = (float)sqrt(1.0 - pow((double)b2, (double)step));
}

// ------------------------------------------------------------------------------------------------ AdamW, schedule, EMA
// The scheduled tick: adam_tick_kernel's count and bias corrections (the same expressions, the same bits), plus the learning rate
// and the EMA decay of this step by the rule of ign_sched.h -> hp = [bc1, bc2_sqrt, lr_t, d_t].  The schedule's parameters are
// kernel arguments that never change over a run, so one captured launch serves all of it.
__global__ void sched_tick_kernel(int* __restrict__ step_dev, float* __restrict__ hp, float b1, float b2, int kind, double base,
                                  int warmup, double min_lr, long long total, double ema) {
    const int step = ++(*step_dev);
    hp[0] = (float)(1.0 - pow((double)b1, (double)step));
    hp[1] = (float)sqrt(1.0 - pow((double)b2, (double)step));
    hp[2] = ign_sched_lr_at(kind, base, warmup, min_lr, total, step);
    hp[3] = ign_ema_decay_at(ema, step);
}

// adam_kernel's layout and element rule with the step's learning rate and bias corrections read from hp (sched_tick_kernel) and
// decoupled weight decay in front of the update: p *= 1 - lr_t * wd where mask[chunk of 64 floats] != 0 (null mask: everywhere;
// wd == 0: no multiply at all, so an undecayed element takes adam_element's path alone).  A lane's four elements start at a
// multiple of four and so never straddle a chunk.
template <bool CLIP>
__global__ void __launch_bounds__(256) adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long long n, float b1, float b2, float eps, float wd,
                                                    const unsigned char* __restrict__ mask, const float* __restrict__ hp,
                                                    const float* __restrict__ coef) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float bc1 = hp[0], bc2_sqrt = hp[1], lr = hp[2];
    const float step = lr / bc1;
    const float c = CLIP ? coef[0] : 1.f;
    const bool decay = wd != 0.f && (!mask || mask[i >> 6]);
    const float keep = 1.f - lr * wd;
    if (i + 3 < n) {
        float4 pv = *reinterpret_cast<float4*>(p + i);
        float4 gv = *reinterpret_cast<const float4*>(g + i);
        if (CLIP) { gv.x *= c; gv.y *= c; gv.z *= c; gv.w *= c; }
        float4 mv = *reinterpret_cast<float4*>(m + i);
        float4 vv = *reinterpret_cast<float4*>(v + i);
        if (decay) { pv.x *= keep; pv.y *= keep; pv.z *= keep; pv.w *= keep; }
        adam_element(pv.x, gv.x, mv.x, vv.x, b1, b2, step, bc2_sqrt, eps);
        adam_element(pv.y, gv.y, mv.y, vv.y, b1, b2, step, bc2_sqrt, eps);
        adam_element(pv.z, gv.z, mv.z, vv.z, b1, b2, step, bc2_sqrt, eps);
        adam_element(pv.w, gv.w, mv.w, vv.w, b1, b2, step, bc2_sqrt, eps);
        *reinterpret_cast<float4*>(p + i) = pv;
        *reinterpret_cast<float4*>(m + i) = mv;
        *reinterpret_cast<float4*>(v + i) = vv;
    } else {
        for (long long j = i; j < n; ++j) {
            float pv = p[j], gv = CLIP ? g[j] * c : g[j], mv = m[j], vv = v[j];
            if (decay) pv *= keep;
            adam_element(pv, gv, mv, vv, b1, b2, step, bc2_sqrt, eps);
            p[j] = pv; m[j] = mv; v[j] = vv;
        }
    }
}

// ema += (1 - d_t) * (p - ema), d_t = hp[3]: p == ema adds (1 - d_t) * 0 = 0, the average keeps its bits.
__global__ void __launch_bounds__(256) ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long long n,
                                                  const float* __restrict__ hp) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float w = 1.f - hp[3];
    if (i + 3 < n) {
        float4 e = *reinterpret_cast<float4*>(ema + i);
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        e.x += w * (q.x - e.x); e.y += w * (q.y - e.y); e.z += w * (q.z - e.z); e.w += w * (q.w - e.w);
        *reinterpret_cast<float4*>(ema + i) = e;
    } else {
        for (long long j = i; j < n; ++j) ema[j] += w * (p[j] - ema[j]);
    }
}

// a <-> b in place: every lane holds its own elements of both in registers between the loads and the stores.
__global__ void __launch_bounds__(256) swap_flat_kernel(float* __restrict__ a, float* __restrict__ b, long long n) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 3 < n) {
        const float4 x = *reinterpret_cast<float4*>(a + i);
        const float4 y = *reinterpret_cast<float4*>(b + i);
        *reinterpret_cast<float4*>(a + i) = y;
        *reinterpret_cast<float4*>(b + i) = x;
    } else {
        for (long long j = i; j < n; ++j) { const float x = a[j]; a[j] = b[j]; b[j] = x; }
    }
}

// ------------------------------------------------------------------------------------------------ gather
// Gather per-parameter gradient tensors into the flat bucket in ONE launch (instead of one accumulate kernel per parameter):
// blockIdx.y = table entry, blockIdx.x strides over its elements.
constexpr int GATHER_MAX = 96;
struct GatherTable {
    const float* src[GATHER_MAX];
    long long off[GATHER_MAX];
    long long n[GATHER_MAX];
};
// ACC: add into the slots (gradient accumulation over micro-batches: the extra cost is one read of each slot).
template <bool ACC>
__global__ void __launch_bounds__(256) gather_flat_kernel(const GatherTable t, float* __restrict__ flat) {
    const int e = blockIdx.y;
    const float* __restrict__ src = t.src[e];
    float* __restrict__ dst = flat + t.off[e];
    const long long n = t.n[e];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        dst[i] = ACC ? dst[i] + src[i] : src[i];
}

// ------------------------------------------------------------------------------------------------ gradient norm / clipping
// Global L2 norm of the flat gradient buffer and the clip_grad_norm_ coefficient, in ONE launch with a fixed summation order:
//   stage 1  block b sums the squares of the contiguous slice [b*NORM_SLICE, (b+1)*NORM_SLICE): four 16-byte loads per lane (all
//            issued before the first use), a lane sum in load order, a butterfly over the wave, the four wave sums through LDS in
//            wave order -> part[b].  A pure HBM read: 20 VGPRs, so every CU holds its 8 blocks and the grid (256 blocks at 4 MB,
//            2048 at 32 MB) keeps all of them busy.
//   stage 2  the block that takes the last ticket of an integer counter (agent-scope release before the ticket, acquire after it)
//            adds the partials: lane t the contiguous run [t*per, (t+1)*per) in index order, in double, then the same butterfly /
//            LDS order.  WHICH block does this depends on scheduling; WHAT it computes does not -- no float atomics, bitwise
//            repeatable.  It hands the counter back at zero, so the workspace is zero-filled once, not per call.
// Non-finite values get no special case: an inf makes the norm inf and the coefficient 0 (inf * 0 = NaN in that element, like
// torch's in-place multiply), a NaN makes both NaN (`c > 1 ? 1 : c` keeps a NaN, as torch.clamp(max=1) does).
constexpr int NORM_SLICE = 4096;                 // floats per stage-1 block = 256 lanes x 4 loads x 4 floats
constexpr int NORM_HDR = 4;                      // floats in front of the partials: [0] = the ticket counter, 16-byte padding
__global__ void __launch_bounds__(256) grad_norm_kernel(const float* __restrict__ g, long long n, float max_norm,
                                                        float* __restrict__ out2, float* __restrict__ ws, int nparts) {
    __shared__ float red[4];
    __shared__ double red2[4];
    __shared__ int last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * NORM_SLICE;
    const long long end = min(n, base + NORM_SLICE);
    float4 x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = base + (long long)(k * 256 + tid) * 4;
        x[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i + 3 < end) x[k] = *reinterpret_cast<const float4*>(g + i);
        else {                                   // ragged tail of the buffer: zeros add nothing
            if (i < end) x[k].x = g[i];
            if (i + 1 < end) x[k].y = g[i + 1];
            if (i + 2 < end) x[k].z = g[i + 2];
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (x[k].x * x[k].x + x[k].y * x[k].y) + (x[k].z * x[k].z + x[k].w * x[k].w);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    unsigned int* ticket = reinterpret_cast<unsigned int*>(ws);
    float* part = ws + NORM_HDR;
    if (tid == 0) {
        __hip_atomic_store(part + blockIdx.x, ((red[0] + red[1]) + red[2]) + red[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();                         // release: the partial is visible device-wide before the ticket is drawn
        last = atomicAdd(ticket, 1u) == (unsigned int)(nparts - 1);
    }
    __syncthreads();
    if (!last) return;
    __threadfence();                             // acquire: every other block's partial
    const int per = (nparts + 255) / 256;
    double t = 0.0;
    for (int j = tid * per; j < min(nparts, (tid + 1) * per); ++j)
        t += (double)__hip_atomic_load(part + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) red2[wave] = t;
    __syncthreads();
    if (tid == 0) {
        const float norm = (float)sqrt(((red2[0] + red2[1]) + red2[2]) + red2[3]);
        const float c = max_norm / (norm + 1e-6f);
        out2[0] = norm;
        out2[1] = c > 1.f ? 1.f : c;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next call on this stream
    }
}

__global__ void __launch_bounds__(256) scale_flat_kernel(float* __restrict__ g, long long n, const float* __restrict__ coef) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float c = coef[0];
    if (i + 3 < n) {
        float4 v = *reinterpret_cast<float4*>(g + i);
        v.x *= c; v.y *= c; v.z *= c; v.w *= c;
        *reinterpret_cast<float4*>(g + i) = v;
    } else {
        for (long long j = i; j < n; ++j) g[j] *= c;
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
// The launcher of all four Adam entry points.  Device-count form (step_dev / bc_dev given): adam_tick_kernel advances the count and
// leaves the bias corrections in bc_dev, the update reads them there.  Host-count form: they are computed here from `step`.
static int adam_launch(const char* who, float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                       float beta2, float eps, int step, int* step_dev, float* bc_dev, const float* coef_dev, void* stream) {
    const bool dev = step_dev || bc_dev;
    if (!p || !g || !m || !v || n <= 0 || (dev ? !step_dev || !bc_dev : step <= 0)) {
        ign_set_error("%s: null pointer, n <= 0 or step <= 0", who);
        return IGN_E_ARG;
    }
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) {
        ign_set_error("%s: buffers must be 16-byte aligned", who);
        return IGN_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    float bc1 = 0.f, bc2_sqrt = 0.f;
    if (dev) {
        hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, s, step_dev, bc_dev, beta1, beta2);
        int rc;
        if ((rc = ign_check_launch("adam_tick_kernel"))) return rc;
    } else {
        bc1 = (float)(1.0 - pow((double)beta1, step));
        bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, step));
    }
    IgnScopedTimer tm("adam", s);
    const auto kernel = dev ? (coef_dev ? adam_kernel<true, true> : adam_kernel<false, true>)
                            : (coef_dev ? adam_kernel<true, false> : adam_kernel<false, false>);
    const long long blocks = (n / 4 + 256) / 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, g, m, v, n, lr, beta1, beta2, eps, bc1, bc2_sqrt, coef_dev,
                       (const float*)bc_dev);
    return ign_check_launch("adam_kernel");
}

extern "C" int ign_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                             float eps, int step, void* stream) {
    return adam_launch("ign_adam_step", p, g, m, v, n, lr, beta1, beta2, eps, step, nullptr, nullptr, nullptr, stream);
}

extern "C" int ign_adam_step_clip(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                                  float eps, int step, const float* coef_dev, void* stream) {
    return adam_launch("ign_adam_step_clip", p, g, m, v, n, lr, beta1, beta2, eps, step, nullptr, nullptr, coef_dev, stream);
}

extern "C" int ign_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                                 float eps, int* step_dev, float* bc_dev, void* stream) {
    return adam_launch("ign_adam_step_dev", p, g, m, v, n, lr, beta1, beta2, eps, 0, step_dev, bc_dev, nullptr, stream);
}

extern "C" int ign_adam_step_clip_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                                      float eps, int* step_dev, float* bc_dev, const float* coef_dev, void* stream) {
    return adam_launch("ign_adam_step_clip_dev", p, g, m, v, n, lr, beta1, beta2, eps, 0, step_dev, bc_dev, coef_dev, stream);
}

extern "C" float ign_sched_lr(int kind, double base_lr, int warmup, double min_lr, long long total_steps, long long step) {
    return ign_sched_lr_at(kind, base_lr, warmup, min_lr, total_steps, step);
}

extern "C" int ign_adamw_step_dev(float* p, const float* g, float* m, float* v, long long n, float beta1, float beta2, float eps,
                                  float weight_decay, const unsigned char* decay_mask, int sched_kind, double base_lr, int warmup,
                                  double min_lr, long long total_steps, double ema_decay, int* step_dev, float* hp_dev,
                                  const float* coef_dev, void* stream) {
    if (!p || !g || !m || !v || !step_dev || !hp_dev || n <= 0) {
        ign_set_error("ign_adamw_step_dev: null pointer or n <= 0");
        return IGN_E_ARG;
    }
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) {
        ign_set_error("ign_adamw_step_dev: buffers must be 16-byte aligned");
        return IGN_E_ARG;
    }
    if (!ign_sched_valid(sched_kind, base_lr, warmup, min_lr, total_steps) || !(weight_decay >= 0.f) ||
        !(ema_decay >= 0.0 && ema_decay < 1.0)) {
        ign_set_error("ign_adamw_step_dev: schedule kind %d, base_lr %g, warmup %d, min_lr %g, total_steps %lld, weight_decay %g or "
                      "ema_decay %g out of range", sched_kind, base_lr, warmup, min_lr, total_steps, (double)weight_decay, ema_decay);
        return IGN_E_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sched_tick_kernel, dim3(1), dim3(1), 0, s, step_dev, hp_dev, beta1, beta2, sched_kind, base_lr, warmup, min_lr,
                       total_steps, ema_decay);
    int rc;
    if ((rc = ign_check_launch("sched_tick_kernel"))) return rc;
    IgnScopedTimer tm("adamw", s);
    const long long blocks = (n / 4 + 256) / 256;
    hipLaunchKernelGGL(coef_dev ? adamw_kernel<true> : adamw_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, p, g, m, v, n,
                       beta1, beta2, eps, weight_decay, decay_mask, (const float*)hp_dev, coef_dev);
    return ign_check_launch("adamw_kernel");
}

extern "C" int ign_ema_update(float* ema, const float* p, long long n, const float* hp_dev, void* stream) {
    if (!ema || !p || !hp_dev || n <= 0) {
        ign_set_error("ign_ema_update: null pointer or n <= 0");
        return IGN_E_ARG;
    }
    if (((uintptr_t)ema | (uintptr_t)p) & 15) {
        ign_set_error("ign_ema_update: ema and p must be 16-byte aligned");
        return IGN_E_ARG;
    }
    IgnScopedTimer tm("ema", (hipStream_t)stream);
    const long long blocks = (n / 4 + 256) / 256;
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ema, p, n, hp_dev);
    return ign_check_launch("ema_kernel");
}

extern "C" int ign_swap_flat(float* a, float* b, long long n, void* stream) {
    if (!a || !b || n <= 0) {
        ign_set_error("ign_swap_flat: null pointer or n <= 0");
        return IGN_E_ARG;
    }
    if (((uintptr_t)a | (uintptr_t)b) & 15) {
        ign_set_error("ign_swap_flat: a and b must be 16-byte aligned");
        return IGN_E_ARG;
    }
    if (a < b ? a + n > b : b + n > a) {
        ign_set_error("ign_swap_flat: a and b overlap");
        return IGN_E_ARG;
    }
    IgnScopedTimer tm("swap_flat", (hipStream_t)stream);
    const long long blocks = (n / 4 + 256) / 256;
    hipLaunchKernelGGL(swap_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, n);
    return ign_check_launch("swap_flat_kernel");
}

static int gather_flat(const char* who, bool acc, const void* const* src, const long long* off, const long long* n, int count,
                       float* flat, void* stream) {
    if (!src || !off || !n || !flat || count < 0) {
        ign_set_error("%s: null pointer or negative count", who);
        return IGN_E_ARG;
    }
    for (int base = 0; base < count; base += GATHER_MAX) {
        GatherTable t;
        const int m = count - base < GATHER_MAX ? count - base : GATHER_MAX;
        long long big = 1;
        for (int i = 0; i < m; ++i) {
            t.src[i] = (const float*)src[base + i]; t.off[i] = off[base + i]; t.n[i] = n[base + i];
            if (!t.src[i] || t.n[i] < 0) { ign_set_error("%s: entry %d is null / negative", who, base + i); return IGN_E_ARG; }
            if (t.n[i] > big) big = t.n[i];
        }
        const long long bx = (big + 256 * 8 - 1) / (256 * 8);            // ~8 elements per thread for the largest entry
        const dim3 grid((unsigned)(bx < 1 ? 1 : (bx > 1024 ? 1024 : bx)), (unsigned)m);
        if (acc) {
            IgnScopedTimer tm("gather_acc", (hipStream_t)stream);
            hipLaunchKernelGGL(gather_flat_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, t, flat);
        } else {
            hipLaunchKernelGGL(gather_flat_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, t, flat);
        }
        int rc;
        if ((rc = ign_check_launch("gather_flat_kernel"))) return rc;
    }
    return 0;
}

extern "C" int ign_gather_flat(const void* const* src, const long long* off, const long long* n, int count, float* flat,
                               void* stream) {
    return gather_flat("ign_gather_flat", false, src, off, n, count, flat, stream);
}

extern "C" int ign_gather_flat_acc(const void* const* src, const long long* off, const long long* n, int count, float* flat,
                                   void* stream) {
    return gather_flat("ign_gather_flat_acc", true, src, off, n, count, flat, stream);
}

extern "C" size_t ign_grad_norm_workspace_bytes(long long n) {
    if (n <= 0) return 0;
    return (size_t)(NORM_HDR + (n + NORM_SLICE - 1) / NORM_SLICE) * sizeof(float);
}

extern "C" int ign_grad_norm_clip(const float* g, long long n, float max_norm, float* out2, void* workspace, void* stream) {
    if (!g || !out2 || !workspace || n <= 0) {
        ign_set_error("ign_grad_norm_clip: null pointer or n <= 0");
        return IGN_E_ARG;
    }
    if (((uintptr_t)g | (uintptr_t)workspace) & 15) {
        ign_set_error("ign_grad_norm_clip: g and workspace must be 16-byte aligned");
        return IGN_E_ARG;
    }
    const long long nparts = (n + NORM_SLICE - 1) / NORM_SLICE;
    if (nparts > 0x7fffffffLL) { ign_set_error("ign_grad_norm_clip: n=%lld too large", n); return IGN_E_TOOBIG; }
    IgnScopedTimer tm("grad_norm", (hipStream_t)stream);
    hipLaunchKernelGGL(grad_norm_kernel, dim3((unsigned)nparts), dim3(256), 0, (hipStream_t)stream, g, n, max_norm, out2,
                       (float*)workspace, (int)nparts);
    return ign_check_launch("grad_norm_kernel");
}

extern "C" int ign_scale_flat(float* g, long long n, const float* coef_dev, void* stream) {
    if (!g || !coef_dev || n <= 0) {
        ign_set_error("ign_scale_flat: null pointer or n <= 0");
        return IGN_E_ARG;
    }
    if ((uintptr_t)g & 15) {
        ign_set_error("ign_scale_flat: g must be 16-byte aligned");
        return IGN_E_ARG;
    }
    IgnScopedTimer tm("scale_flat", (hipStream_t)stream);
    const long long blocks = (n / 4 + 256) / 256;
    hipLaunchKernelGGL(scale_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, n, coef_dev);
    return ign_check_launch("scale_flat_kernel");
}
