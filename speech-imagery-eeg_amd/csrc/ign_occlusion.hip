// Occlusion maps (utils/occlusion.py, run.py --occlusion): hide a window of time on a group of electrodes, run the model, record how far
// the class score falls, and lay the falls back over the cells that were hidden.  Two passes, both exact and bitwise defined; the rule is
// utils/occlusion.py (occlude_rule, spread_rule), which the kernels equal bit for bit.
//
//   grid     : W <= T steps per window, S <= W steps between windows, nt = ceil((T - W) / S) + 1 windows -- the HOST's numbers, the
//              same for every sample; patch p = i * G + g hides window i on the electrodes c with gid[c] == g;
//   hidden   : gid[c] == g(p) and i(p) * S <= t < min(i(p) * S + W, n_b), n_b = clamp(len_b, 0, T);
//   covering : the windows over step t are i = max(0, ceil((t - W + 1) / S)) .. min(nt - 1, t / S): at least one, at most ceil(W / S).
//
// occlude_kernel: perturb_kernel's layout (csrc/ign_faithfulness.hip) -- a block owns OC_CHUNK consecutive flat (t, c) indices of one
// sample, a lane a quad through a 4-byte-aligned 16-byte vector type.  A quad of x, its fill values and its group ids are read once
// into registers, then the Pc copies are written with a select each: one read and Pc writes of the batch.
//
// spread_kernel: a gather -- a lane owns a cell and adds the drops of the windows over its step in ascending order, each one float
// add (the file is compiled with -ffp-contract=off), then multiplies by the host's 1 / count.  No atomics, no workspace; a sample
// reads its own drops only.
#include <cstdint>
#include "ign_common.h"

constexpr int OC_THREADS = 256;
constexpr int OC_QUADS = 4;                                    // quads per lane
constexpr int OC_CHUNK = OC_THREADS * OC_QUADS * 4;            // flat indices per block
constexpr long long OC_INDEX_LIMIT = 0x7fff0000LL;             // 2^31 - 65536

struct __attribute__((packed, aligned(4))) OcQuad { unsigned v[4]; };

struct OcArgs {
    const unsigned* x;        // (B,T,C), as bits
    const unsigned* fill;     // (B,C) as bits, or null: 0.0f
    const int32_t* len;       // (B) or null
    const int32_t* gid;       // (C)
    unsigned* out;            // (B*Pc,T,C)
    int p0, Pc, G, W, S, T, C, nchunk;
};

__global__ void __launch_bounds__(OC_THREADS) occlude_kernel(const OcArgs a) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.nchunk;
    const int chunk = blockIdx.x - b * a.nchunk;
    const int C = a.C, TC = a.T * C, G = a.G;
    const int len = a.len ? min(max(a.len[b], 0), a.T) : a.T;   // device data: clamped, never trusted as an index bound
    const unsigned* xb = a.x + (size_t)b * TC;
    const unsigned* fb = a.fill ? a.fill + (size_t)b * C : nullptr;
    unsigned* ob = a.out + (size_t)b * a.Pc * TC;               // the sample's Pc copies, TC apart
    const int i0 = a.p0 / G, g0 = a.p0 - i0 * G;                // block-uniform
#pragma unroll
    for (int u = 0; u < OC_QUADS; ++u) {
        const int e0 = chunk * OC_CHUNK + (u * OC_THREADS + tid) * 4;
        if (e0 >= TC) break;                                     // e0 grows with u
        const int cnt = min(4, TC - e0);
        OcQuad q;
        unsigned f[4];
        int g[4], t[4];
        if (cnt == 4) q = *reinterpret_cast<const OcQuad*>(xb + e0);
        int tt = e0 / C, c = e0 - tt * C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = k < cnt;                             // c < C always: the loads below stay inside (C) and (B,C)
            if (cnt != 4) q.v[k] = in ? xb[e0 + k] : 0u;
            f[k] = fb ? fb[c] : 0u;
            g[k] = in ? a.gid[c] : -1;                           // -1: no group, the lane's spare slots are never selected
            t[k] = tt;
            if (++c == C) { c = 0; ++tt; }
        }
        int i = i0, gp = g0;
        for (int p = 0; p < a.Pc; ++p) {                         // block-uniform trip count
            const int lo = i * a.S, hi = min(lo + a.W, len);     // lo + W <= 2T: no overflow
            OcQuad o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.v[k] = (g[k] == gp && t[k] >= lo && t[k] < hi) ? f[k] : q.v[k];
            unsigned* dst = ob + (size_t)p * TC + e0;
            if (cnt == 4) {
                *reinterpret_cast<OcQuad*>(dst) = o;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) dst[k] = o.v[k];
            }
            if (++gp == G) { gp = 0; ++i; }
        }
    }
}

// what both entry points ask of the grid -> 0, or IGN_E_ARG with the reason set
static int oc_check_grid(const char* who, int G, int W, int S, int nt, int T) {
    if (G < 1) {
        ign_set_error("%s: G=%d electrode groups, need at least one", who, G);
        return IGN_E_ARG;
    }
    if (S < 1 || S > W || W > T) {
        ign_set_error("%s: need 1 <= S <= W <= T, got S=%d W=%d T=%d (a stride above the window leaves steps uncovered)", who, S, W, T);
        return IGN_E_ARG;
    }
    const int want = (T - W + S - 1) / S + 1;
    if (nt != want) {
        ign_set_error("%s: nt=%d, but T=%d W=%d S=%d give ceil((T - W) / S) + 1 = %d windows", who, nt, T, W, S, want);
        return IGN_E_ARG;
    }
    return 0;
}

extern "C" int ign_occlude_btc(const float* x_btc, const float* fill_bc, const int32_t* len_b, const int32_t* gid_c, float* out, int p0,
                               int Pc, int G, int W, int S, int nt, int B, int T, int C, void* stream) {
    static const char* who = "ign_occlude_btc";
    if (!x_btc || !gid_c || !out || B < 1 || T < 1 || C < 1) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d T=%d C=%d)", who, B, T, C);
        return IGN_E_ARG;
    }
    if (const int rc = oc_check_grid(who, G, W, S, nt, T)) return rc;
    if (p0 < 0 || Pc < 1 || (long long)p0 + Pc > (long long)nt * G) {
        ign_set_error("%s: patches p0=%d .. p0+Pc-1 with Pc=%d outside [0, nt*G) = [0, %lld)", who, p0, Pc, (long long)nt * G);
        return IGN_E_ARG;
    }
    const long long TC = (long long)T * C;
    if (TC >= OC_INDEX_LIMIT || (long long)B * Pc >= OC_INDEX_LIMIT || (long long)B * Pc * TC >= OC_INDEX_LIMIT) {
        ign_set_error("%s: B*Pc*T*C = %d*%d*%lld does not fit a 32-bit index", who, B, Pc, TC);
        return IGN_E_TOOBIG;
    }
    const long long nchunk = (TC + OC_CHUNK - 1) / OC_CHUNK;   // B * nchunk <= B * TC: fits a grid
    const uintptr_t xa = (uintptr_t)x_btc, oa = (uintptr_t)out, xbytes = (uintptr_t)B * (uintptr_t)TC * sizeof(float);
    const uintptr_t obytes = xbytes * (uintptr_t)Pc;
    if (xa < oa ? oa - xa < xbytes : xa - oa < obytes) {
        ign_set_error("%s: out of place only (Pc copies are written from one read of x): x and out overlap", who);
        return IGN_E_ARG;
    }
    OcArgs a;
    a.x = reinterpret_cast<const unsigned*>(x_btc); a.fill = reinterpret_cast<const unsigned*>(fill_bc); a.len = len_b; a.gid = gid_c;
    a.out = reinterpret_cast<unsigned*>(out);
    a.p0 = p0; a.Pc = Pc; a.G = G; a.W = W; a.S = S; a.T = T; a.C = C; a.nchunk = (int)nchunk;
    {
        IgnScopedTimer tm("occlude", (hipStream_t)stream);
        hipLaunchKernelGGL(occlude_kernel, dim3((unsigned)(B * nchunk)), dim3(OC_THREADS), 0, (hipStream_t)stream, a);
    }
    return ign_check_launch("occlude_kernel");
}

// ---------------------------------------------------------------- the gather back
constexpr int SP_THREADS = 256;

__global__ void __launch_bounds__(SP_THREADS) spread_kernel(const float* __restrict__ drop, const int32_t* __restrict__ gid,
                                                            const int32_t* __restrict__ len_b, const float* __restrict__ inv_k,
                                                            float* __restrict__ out, int G, int W, int S, int nt, int T, int C,
                                                            int nchunk) {
    const int b = blockIdx.x / nchunk;
    const int e = (blockIdx.x - b * nchunk) * SP_THREADS + threadIdx.x;
    const int TC = T * C;
    if (e >= TC) return;
    const int len = len_b ? min(max(len_b[b], 0), T) : T;       // device data: clamped, never trusted as an index bound
    const int t = e / C, c = e - t * C;
    float m = 0.0f;
    if (t < len) {
        const int g = min(max(gid[c], 0), G - 1);                // the caller checked gid; clamped all the same before it indexes
        const int lo = t - W + 1 > 0 ? (t - W + S) / S : 0;      // ceil((t - W + 1) / S)
        const int hi = min(nt - 1, t / S);                       // lo <= hi, hi - lo + 1 <= ceil(W / S) (the host checked the grid)
        const float* db = drop + (size_t)b * nt * G + g;
        float s = db[(size_t)lo * G];
        for (int i = lo + 1; i <= hi; ++i) s += db[(size_t)i * G];
        m = s * inv_k[hi - lo + 1];
    }
    out[(size_t)b * TC + e] = m;
}

extern "C" int ign_occlusion_spread(const float* drop_bp, const int32_t* gid_c, const int32_t* len_b, const float* inv_k, float* out_btc,
                                    int G, int W, int S, int nt, int B, int T, int C, void* stream) {
    static const char* who = "ign_occlusion_spread";
    if (!drop_bp || !gid_c || !inv_k || !out_btc || B < 1 || T < 1 || C < 1) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d T=%d C=%d)", who, B, T, C);
        return IGN_E_ARG;
    }
    if (const int rc = oc_check_grid(who, G, W, S, nt, T)) return rc;
    if ((W + S - 1) / S > IGN_OCC_MAX_COVER) {
        ign_set_error("%s: W=%d S=%d put ceil(W / S) = %d windows over a step, more than %d (IGN_OCC_MAX_COVER)", who, W, S,
                      (W + S - 1) / S, IGN_OCC_MAX_COVER);
        return IGN_E_ARG;
    }
    const long long TC = (long long)T * C;
    if (TC >= OC_INDEX_LIMIT) {
        ign_set_error("%s: T*C=%lld does not fit a 32-bit index", who, TC);
        return IGN_E_TOOBIG;
    }
    const long long nchunk = (TC + SP_THREADS - 1) / SP_THREADS;
    if ((long long)B * nchunk > 0x7fffffffLL || (long long)nt * G >= OC_INDEX_LIMIT) {
        ign_set_error("%s: B=%d T=%d C=%d nt*G=%lld needs more blocks than a grid has", who, B, T, C, (long long)nt * G);
        return IGN_E_TOOBIG;
    }
    {
        IgnScopedTimer tm("occlusion_spread", (hipStream_t)stream);
        hipLaunchKernelGGL(spread_kernel, dim3((unsigned)(B * nchunk)), dim3(SP_THREADS), 0, (hipStream_t)stream, drop_bp, gid_c, len_b,
                           inv_k, out_btc, G, W, S, nt, T, C, (int)nchunk);
    }
    return ign_check_launch("spread_kernel");
}
