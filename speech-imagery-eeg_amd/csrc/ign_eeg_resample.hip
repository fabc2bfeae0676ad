// Rational resampling stage between the IIR stage and the FIR / standardisation stages (run.py --eeg_resample; ops.eeg_resample; the
// rule is stated once in numpy float64 in utils/eeg_resample.py:resample_numpy): every (b, c) row of the raw (B, C, Tin) batch goes
// from Tin to Tout = ceil(Tin * up / down) samples through a polyphase Kaiser-windowed low-pass -- scipy.signal.resample_poly.
//
//   p  = x[0];  u = x - p;  ue = u extended by R = Lp samples on both sides (reflect, or zeros)
//   n in [0, Tout):  a = n*down + hl;  khi = a div up;  r = a mod up
//   out[n] = p + sum_{i < Lp} tab[r][i] * ue[khi - i]                       one fmaf chain, i ascending
//
// tab (up, Lp) holds the fp32 taps by phase, tab[r][i] = h[r + i*up], zero past the last tap.  The pivot p re-enters with gain 1: the
// phases' DC gains differ by 1e-4, which would print a ripple of the recording's offset onto the signal.
//
// One workgroup per row.  The extended row (Tin + 2R floats; the staging loop is the only reader of x and reads [0, Tin) only) and
// the phase table sit in LDS.  Lane <-> output n: neighbouring outputs read different phases, so the table's row stride is Lp | 1 --
// odd: r steps by down mod up from lane to lane (61 at 64/125, odd, so 32 lanes hold 32 different r mod 32), and with an odd stride
// r*stride + i then falls on 32 different banks; lanes that share a phase read one address, which is a broadcast.  The row
// reads of neighbouring lanes are down/up apart: two lanes per bank at 64/125 and at 1/2.  khi and r cost one integer division per
// output; the chain is Lp fmaf with two LDS reads each.  No workspace, no atomics, a fixed order: a row's result depends on that row
// and the table alone.
//
// Bounds (with the launcher's checks: Lp = ceil((2hl+1)/up), Tout = ceil(Tin*up/down)): a <= Tin*up - 1 + hl, so
// khi <= Tin + (hl-1) div up <= Tin + Lp - 1 and the highest index read, khi + R, is below Tin + 2R; the lowest is
// khi - (Lp-1) + R >= 1.  a stays an int: Tin*up < 16384 * 8192 by the LDS and table limits, hl <= 4096.
#include "ign_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr size_t RS_MAX_LDS = 64 * 1024;

__host__ __device__ __forceinline__ int rs_stride(int Lp) { return Lp | 1; }

__global__ __launch_bounds__(RS_THREADS) void eeg_resample_kernel(const float* __restrict__ x, const float* __restrict__ tab,
                                                                  float* __restrict__ out, int Tin, int Tout, int up, int down, int hl,
                                                                  int Lp, int edge) {
    extern __shared__ float rs_lds[];
    const int R = Lp, N = Tin + 2 * R, ts = rs_stride(Lp);
    float* ue = rs_lds;                                // N floats: the pivoted, extended row
    float* tl = rs_lds + N;                            // up * ts floats: the phase table, rows padded to an odd stride
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const float* xr = x + row * (size_t)Tin;
    const float p = xr[0];

    for (int j = tid; j < N; j += RS_THREADS) {
        const int s = j - R;
        float v = 0.f;
        if (s >= 0 && s < Tin) v = xr[s] - p;
        else if (edge == IGN_EDGE_REFLECT) v = xr[s < 0 ? -s : 2 * (Tin - 1) - s] - p;      // R < Tin: [1, R] and [Tin-1-R, Tin-2]
        ue[j] = v;
    }
    for (int j = tid; j < up * Lp; j += RS_THREADS) {
        const int r = j / Lp;
        tl[r * ts + (j - r * Lp)] = tab[j];
    }
    __syncthreads();

    float* orow = out + row * (size_t)Tout;
    for (int n = tid; n < Tout; n += RS_THREADS) {
        const int a = n * down + hl;
        const int khi = a / up, r = a - khi * up;
        const float* t = tl + r * ts;
        const float* u = ue + khi + R;
        float acc = 0.f;
        for (int i = 0; i < Lp; ++i) acc = fmaf(t[i], u[-i], acc);
        orow[n] = acc + p;
    }
}

int rs_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// the checks the byte count and the launcher share; LDS bytes of a row plus the table, 0 with *rc set on a refusal
size_t rs_plan(const char* who, int Tin, int up, int Lp, int* rc) {
    *rc = 0;
    if (Tin <= 0 || up <= 0 || Lp <= 0) {
        ign_set_error("%s: non-positive Tin=%d, up=%d or Lp=%d", who, Tin, up, Lp);
        *rc = IGN_E_ARG;
        return 0;
    }
    const long long table = (long long)up * Lp;
    if (table > IGN_EEG_RESAMPLE_MAX_TABLE) {
        ign_set_error("%s: a phase table of up*Lp = %d*%d = %lld floats is beyond IGN_EEG_RESAMPLE_MAX_TABLE = %d", who, up, Lp, table,
                      IGN_EEG_RESAMPLE_MAX_TABLE);
        *rc = IGN_E_TOOBIG;
        return 0;
    }
    const long long bytes = 4LL * ((long long)Tin + 2LL * Lp + (long long)up * rs_stride(Lp));
    if (bytes > (long long)RS_MAX_LDS) {
        ign_set_error("%s: a row of Tin=%d samples extended by 2*%d plus a %d x %d table is %lld bytes of LDS, beyond %zu", who, Tin, Lp,
                      up, Lp, bytes, RS_MAX_LDS);
        *rc = IGN_E_TOOBIG;
        return 0;
    }
    return (size_t)bytes;
}

}  // namespace

extern "C" size_t ign_eeg_resample_lds_bytes(int Tin, int up, int Lp) {
    int rc;
    return rs_plan("ign_eeg_resample_lds_bytes", Tin, up, Lp, &rc);
}

extern "C" int ign_eeg_resample_nct(const float* x_nct, const float* tab, float* out_nct, int B, int C, int Tin, int Tout, int up,
                                    int down, int hl, int Lp, int edge, void* stream) {
    static const char* who = "ign_eeg_resample_nct";
    if (!x_nct || !tab || !out_nct) {
        ign_set_error("%s: null pointer (x, tab or out)", who);
        return IGN_E_ARG;
    }
    if (B <= 0 || C <= 0 || Tin <= 0 || Tout <= 0 || up <= 0 || down <= 0 || hl < 0 || Lp <= 0) {
        ign_set_error("%s: non-positive dimension (B=%d C=%d Tin=%d Tout=%d up=%d down=%d hl=%d Lp=%d)", who, B, C, Tin, Tout, up, down,
                      hl, Lp);
        return IGN_E_ARG;
    }
    if (rs_gcd(up, down) != 1) {
        ign_set_error("%s: up/down = %d/%d is not in lowest terms", who, up, down);
        return IGN_E_ARG;
    }
    if ((2LL * hl + 1 + up - 1) / up != Lp) {
        ign_set_error("%s: Lp=%d is not ceil((2*hl+1)/up) = %lld for hl=%d, up=%d", who, Lp, (2LL * hl + 1 + up - 1) / up, hl, up);
        return IGN_E_ARG;
    }
    const long long want = ((long long)Tin * up + down - 1) / down;
    if (want != Tout) {
        ign_set_error("%s: Tout=%d is not ceil(Tin*up/down) = %lld for Tin=%d, %d/%d", who, Tout, want, Tin, up, down);
        return IGN_E_ARG;
    }
    if (edge != IGN_EDGE_REFLECT && edge != IGN_EDGE_ZERO) {
        ign_set_error("%s: edge=%d is neither IGN_EDGE_REFLECT nor IGN_EDGE_ZERO", who, edge);
        return IGN_E_ARG;
    }
    if (edge == IGN_EDGE_REFLECT && Lp >= Tin) {
        ign_set_error("%s: a reflect extension by R=%d samples needs rows of more than R samples, got Tin=%d", who, Lp, Tin);
        return IGN_E_ARG;
    }
    int rc = 0;
    const size_t lds = rs_plan(who, Tin, up, Lp, &rc);
    if (rc) return rc;
    const long long rows = (long long)B * C;
    if (rows > 0x7fffffffLL) {
        ign_set_error("%s: B*C=%lld rows exceed the launch grid", who, rows);
        return IGN_E_TOOBIG;
    }
    hipStream_t s = (hipStream_t)stream;
    IgnScopedTimer tm("eeg_resample", s);
    hipLaunchKernelGGL(eeg_resample_kernel, dim3((unsigned)rows), dim3(RS_THREADS), lds, s, x_nct, tab, out_nct, Tin, Tout, up, down,
                       hl, Lp, edge);
    return ign_check_launch("eeg_resample_kernel");
}
