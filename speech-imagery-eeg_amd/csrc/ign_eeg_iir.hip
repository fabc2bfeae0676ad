// Zero-phase IIR stage between the spatial filter and the FIR / standardisation stages (run.py --eeg_iir; ops.eeg_iir; the rule is
// stated once in numpy float64 in utils/eeg_iir.py:iir_numpy): a cascade of second-order sections run forward and backward along
// time over every (b, c) row of the raw (B, C, T) batch -- scipy.signal.sosfiltfilt(sos, x, padtype='odd', padlen=P).
//
//   p  = x[0];  u = double(x) - double(p)
//   ue = [-u[P] .. -u[1],  u[0..T),  2u[T-1]-u[T-2] .. 2u[T-1]-u[T-1-P]]                          N = T + 2P samples
//   section k, state (s1, s2):   y = b0*v + s1;   s1 = (b1*v - a1*y) + s2;   s2 = b2*v - a2*y
//   forward: states start at zi_k * ue[0];  backward: the same cascade over the reversed forward output, from zi_k * (its first)
//   out[t] = float( back[P+t] + g0*p )
//
// Every value between the load of x and the store of out is a double: the poles of a 0.5 Hz high-pass at 500 Hz sit at radius 0.996
// and a float recurrence is 4.7e-5 of the row's scale away from this one.
//
// One wave per row, one row per block.  The extended row lives in LDS as doubles (8 N bytes; the staging loop is the only reader of x
// and reads [0, T) only).  Lane l owns the chunk [l*Lc, min((l+1)*Lc, N)) with Lc = ceil(N / 64) rounded up to odd: a lane stride of
// 2 Lc dwords is conflict-free for 8-byte LDS accesses.  The state update is affine in the state, s' = A s + B v, so per section and
// direction
//   (a) every lane runs its chunk from a zero state and keeps the end state e_l;
//   (b) M = A^Lc, the transition of a full chunk, comes from two homogeneous runs, and M^2, M^4 .. M^32 from squaring it (once per
//       section, by lane k, before the loop);
//   (c) the start states c_0 = zi_k * first, c_{l+1} = M c_l + e_l, i.e. c_l = sum_{i<=l} M^(l-i) f_i with f = (c_0, e_0, e_1, ..),
//       come from an inclusive scan across the lanes in six fixed steps, f_l += M^(2^j) f_(l-2^j);
//   (d) every lane runs its chunk again from c_l and overwrites it in place.
// Measured on the host in numpy float64, this evaluation is within 6e-12 of the row's scale of the sequential rule (carries resolved
// one lane after the other: 4e-13; the tests allow 1e-9), and the scan replaces 63 dependent steps per section and direction, which
// took more time than (a) and (d) together.  The backward direction is the same code with the index reversed.  A lane reads and
// writes its own chunk only, so the wave meets at three points: after the staging, between the directions (`first` of the backward
// run is the last lane's sample), before the store.  No workspace, no atomics, a fixed order: a row's result depends on that row
// and the table alone.
#include "ign_common.h"

namespace {

constexpr int IIR_WAVE = 64;
constexpr int IIR_SCAN_STEPS = 6;                                       // log2(IIR_WAVE)
// doubles behind the staged row: M^(2^j), j = 0..5, per section, row-major 2 x 2
constexpr int IIR_EXTRA = IGN_EEG_IIR_MAX_SECTIONS * IIR_SCAN_STEPS * 4;

__host__ __device__ __forceinline__ int iir_chunk(int N) { return ((N + IIR_WAVE - 1) / IIR_WAVE) | 1; }

struct IirCoef {
    double b0, b1, b2, a1, a2;
};

// one step of a section; the products that feed a subtraction are fused into it (one rounding fewer than the rule's wording, far
// inside the order-of-evaluation distance)
__device__ __forceinline__ double iir_step(double v, const IirCoef& c, double& s1, double& s2) {
    const double y = fma(c.b0, v, s1);
    s1 = fma(-c.a1, y, c.b1 * v) + s2;
    s2 = fma(-c.a2, y, c.b2 * v);
    return y;
}

// the section over buf[base + step * i], i in [0, len), from the state (s1, s2); WRITE: the output replaces the input.  Four samples
// at a time with the next four already in flight, so the recurrence does not wait for LDS at every step; every access stays inside
// the lane's own chunk.
template <bool WRITE>
__device__ __forceinline__ void iir_run(double* buf, int base, int step, int len, const IirCoef& c, double& s1, double& s2) {
    int i = 0;
    if (len >= 4) {
        double v0 = buf[base], v1 = buf[base + step], v2 = buf[base + 2 * step], v3 = buf[base + 3 * step];
        for (; i + 4 <= len; i += 4) {
            const int j = base + step * i;
            double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0;
            if (i + 8 <= len) {
                w0 = buf[j + 4 * step];
                w1 = buf[j + 5 * step];
                w2 = buf[j + 6 * step];
                w3 = buf[j + 7 * step];
            }
            const double y0 = iir_step(v0, c, s1, s2);
            const double y1 = iir_step(v1, c, s1, s2);
            const double y2 = iir_step(v2, c, s1, s2);
            const double y3 = iir_step(v3, c, s1, s2);
            if (WRITE) {
                buf[j] = y0;
                buf[j + step] = y1;
                buf[j + 2 * step] = y2;
                buf[j + 3 * step] = y3;
            }
            v0 = w0;
            v1 = w1;
            v2 = w2;
            v3 = w3;
        }
    }
    for (; i < len; ++i) {
        const int j = base + step * i;
        const double y = iir_step(buf[j], c, s1, s2);
        if (WRITE) buf[j] = y;
    }
}

__global__ __launch_bounds__(IIR_WAVE) void eeg_iir_kernel(const float* __restrict__ x, const double* __restrict__ coef,
                                                           float* __restrict__ out, int T, int ns, int P, double g0) {
    extern __shared__ double iir_lds[];
    const int N = T + 2 * P;
    double* buf = iir_lds;                             // N doubles: the extended row, filtered in place
    double* Msh = iir_lds + N;                         // IIR_EXTRA doubles
    const int lane = threadIdx.x;
    const size_t row = blockIdx.x;
    const float* xr = x + row * (size_t)T;
    const double p = (double)xr[0];
    const int Lc = iir_chunk(N);

    const double ulast = (double)xr[T - 1] - p;
    for (int i = lane; i < N; i += IIR_WAVE) {
        double v;
        if (i < P) v = -((double)xr[P - i] - p);                                   // P - i in [1, P], P < T
        else if (i < P + T) v = (double)xr[i - P] - p;
        else v = 2.0 * ulast - ((double)xr[T - 2 - (i - P - T)] - p);              // T - 2 - k, k in [0, P): down to T - 1 - P >= 0
        buf[i] = v;
    }
    if (lane < ns) {                                   // (b) M = A^Lc by columns: the homogeneous runs from (1, 0) and from (0, 1)
        const double a1 = coef[lane * 8 + 3], a2 = coef[lane * 8 + 4];
        double m00 = 1.0, m10 = 0.0, m01 = 0.0, m11 = 1.0;
        for (int i = 0; i < Lc; ++i) {
            double t = fma(-a1, m00, m10);
            m10 = -a2 * m00;
            m00 = t;
            t = fma(-a1, m01, m11);
            m11 = -a2 * m01;
            m01 = t;
        }
        double* mk = Msh + lane * IIR_SCAN_STEPS * 4;
        for (int j = 0; j < IIR_SCAN_STEPS; ++j) {
            mk[4 * j] = m00;
            mk[4 * j + 1] = m01;
            mk[4 * j + 2] = m10;
            mk[4 * j + 3] = m11;
            const double q00 = fma(m00, m00, m01 * m10), q01 = fma(m00, m01, m01 * m11);
            const double q10 = fma(m10, m00, m11 * m10), q11 = fma(m10, m01, m11 * m11);
            m00 = q00;
            m01 = q01;
            m10 = q10;
            m11 = q11;
        }
    }
    __syncthreads();

    const int nl = (N + Lc - 1) / Lc;                  // lanes with a chunk; all but the last are full
    const int lo = lane * Lc;
    const int len = lane < nl ? (N - lo < Lc ? N - lo : Lc) : 0;

    for (int dir = 0; dir < 2; ++dir) {
        const int base = dir ? N - 1 - lo : lo, step = dir ? -1 : 1;
        const double first = buf[dir ? N - 1 : 0];
        __syncthreads();                               // every lane holds `first` before its owner overwrites it
        for (int k = 0; k < ns; ++k) {
            const double* ck = coef + k * 8;
            const IirCoef c = {ck[0], ck[1], ck[2], ck[3], ck[4]};
            double e1 = 0.0, e2 = 0.0;
            iir_run<false>(buf, base, step, len, c, e1, e2);                                                  // (a)
            double f1 = __shfl_up(e1, 1, IIR_WAVE), f2 = __shfl_up(e2, 1, IIR_WAVE);                          // (c)
            if (lane == 0) {
                f1 = ck[5] * first;
                f2 = ck[6] * first;
            }
            const double* mk = Msh + k * IIR_SCAN_STEPS * 4;
            for (int j = 0; (1 << j) < nl; ++j) {
                const int d = 1 << j;
                const double t1 = __shfl_up(f1, d, IIR_WAVE), t2 = __shfl_up(f2, d, IIR_WAVE);
                const double m00 = mk[4 * j], m01 = mk[4 * j + 1], m10 = mk[4 * j + 2], m11 = mk[4 * j + 3];
                if (lane >= d) {
                    f1 = fma(m00, t1, fma(m01, t2, f1));
                    f2 = fma(m10, t1, fma(m11, t2, f2));
                }
            }
            iir_run<true>(buf, base, step, len, c, f1, f2);                                                   // (d)
        }
        __syncthreads();                               // the chunks of this direction are complete
    }
    const double g0p = g0 * p;
    float* orow = out + row * (size_t)T;
    for (int t = lane; t < T; t += IIR_WAVE) orow[t] = (float)(buf[P + t] + g0p);
}

// shared argument check; LDS bytes of a row, 0 with *rc set on a refusal
size_t iir_plan(const char* who, int T, int P, int* rc) {
    *rc = 0;
    if (T <= 0 || P < 0 || P >= T) {
        ign_set_error("%s: the pad length P=%d must lie in [0, T) with T=%d", who, P, T);
        *rc = IGN_E_ARG;
        return 0;
    }
    const long long N = (long long)T + 2LL * P;
    if (N > IGN_EEG_IIR_MAX_ROW) {
        ign_set_error("%s: a row of T + 2P = %lld samples is beyond the %d that fit the LDS staging budget", who, N, IGN_EEG_IIR_MAX_ROW);
        *rc = IGN_E_TOOBIG;
        return 0;
    }
    return (size_t)(N + IIR_EXTRA) * sizeof(double);
}

}  // namespace

extern "C" size_t ign_eeg_iir_lds_bytes(int T, int P) {
    int rc;
    return iir_plan("ign_eeg_iir_lds_bytes", T, P, &rc);
}

extern "C" int ign_eeg_iir_nct(const float* x_nct, const double* coef, float* out_nct, int B, int C, int T, int ns, int P, double g0,
                               void* stream) {
    static const char* who = "ign_eeg_iir_nct";
    if (!x_nct || !coef || !out_nct) {
        ign_set_error("%s: null pointer (x, coef or out)", who);
        return IGN_E_ARG;
    }
    if (B <= 0 || C <= 0 || T <= 0) {
        ign_set_error("%s: non-positive dimension (B=%d C=%d T=%d)", who, B, C, T);
        return IGN_E_ARG;
    }
    if (ns < 1 || ns > IGN_EEG_IIR_MAX_SECTIONS) {
        ign_set_error("%s: ns=%d sections outside 1..%d", who, ns, IGN_EEG_IIR_MAX_SECTIONS);
        return IGN_E_ARG;
    }
    int rc = 0;
    const size_t lds = iir_plan(who, T, P, &rc);
    if (rc) return rc;
    const long long rows = (long long)B * C;
    if (rows > 0x7fffffffLL) {
        ign_set_error("%s: B*C=%lld rows exceed the launch grid", who, rows);
        return IGN_E_TOOBIG;
    }
    if (lds > 64 * 1024)      // the longest rows: a CU of gfx950 has 160 KB of LDS, the default cap is 64
        (void)hipFuncSetAttribute((const void*)eeg_iir_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("eeg_iir", s);
    hipLaunchKernelGGL(eeg_iir_kernel, dim3((unsigned)rows), dim3(IIR_WAVE), lds, s, x_nct, coef, out_nct, T, ns, P, g0);
    return ign_check_launch("eeg_iir_kernel");
}
