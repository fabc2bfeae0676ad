// The loss tail of the training step, one launch per call, single-block kernels of a few microseconds: the gini gate
// (IGN/model/InterpGN.py:44-52), the fused classification tail (IGN/exp/experiment_classification.py:320-329) and the CRPS tails of
// the regression task (IGN/exp/experiment_regression.py:59-76, :159-169).
//  * gini gate  q = softmax(s); G = sum q^2; eta = (N G - 1)/(N-1); [eta > gating_value -> 1]; out = eta s + (1 - eta) d
//    backward   d eta / d s_j = (2N/(N-1)) q_j (q_j - G); ds = eta*gout + (sum_n gout_n (s_n - d_n)) * deta/ds; dd = (1 - eta)*gout
//    Written ONCE, in the gate_* helpers, for every kernel of this file: the fused tails' mixture and eta are bitwise ign_gate_fwd's
//    because they are the same source expressions (-ffp-contract=off).  A helper must keep its operation order and association.
//  * CE tail    loss = CE(gate(s, d), y) + beta*CE(s, y) [+ reg] (batch means) and both logit gradients.  Shared by every call: the
//    row's softmax statistics, the gate, the mixture's softmax, the gradients through the gate, the reduction of the rows' loss terms
//    and write_loss3 -- two kernel templates, one per layout.  A label RULE (PlainRule, WeightedRule, SoftRule; one per entry point,
//    passed by value) is what the cross-entropies differ in: how a row's labels and weights are read, the loss-term and the gradient
//    expression, the divisor (1/B or 1/D), and whether class weights are staged and the smoothing sums taken.  The plain rule stages
//    nothing, makes no pre-pass and adds no barrier: its instantiations read and compute what the unweighted tail always did.
//  * CRPS       p = softmax(z), F_j = sum_{i<=j} p_i, H_j = [edge_j >= y] (in float64); loss = mean_b sum_j (F_j - H_j)^2; per row
//    r_j = F_j - H_j, q_i = (2/B) sum_{j>=i} r_j, dz_k = p_k (q_k - sum_i p_i q_i).  InterpGN's tail: CRPS in place of CE above.
// What stays separate, because the summation orders differ and merging would change bits: the two CE layouts -- one thread per row up
// to 16 classes (ign_loss_kernel: row terms added per thread over rows t, t + 256, ..., then over the threads), one wave per row above
// (ign_loss_wide_kernel: row sums are butterflies, row terms added in ascending row order) -- and the CRPS tails (ascending row order,
// rows in registers or global memory).  The three rules share a layout and a summation order exactly, so they share the kernels; they
// are not folded into one another (plain is not weighted with w = 1, eps = 0; weighted is not soft with lam = 1): those are other
// expressions with other roundings.  tests/golden/loss_tail_bits.json pins every output bit of the CE tail.
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
// Two layouts (ign_loss_kernel, ign_loss_wide_kernel), each written once over a label rule.  With p = softmax(z), lse = log sum e^z:
//  * PlainRule     F.cross_entropy(z, y):                               CE = sum_b (lse_b - z[b,y_b]) / B,  dCE/dz_bn = (p_n - [n = y_b]) / B
//  * WeightedRule  F.cross_entropy(z, y, weight=w, label_smoothing=eps); D = sum_b w[y_b], W = sum_n w_n:
//      CEw        = sum_b [ (1-eps) w[y_b] (lse_b - z[b,y_b]) + (eps/N) sum_n w_n (lse_b - z[b,n]) ] / D
//      dCEw/dz_bn = ( (1-eps) w[y_b] (p_n - [n = y_b]) + (eps/N) (p_n W - w_n) ) / D
//  * SoftRule      the same with two labels per row, ya_b and yb_b, and the share lam_b of the first (mixup / CutMix, run.py --mix);
//    a_b = lam_b w[ya_b], c_b = (1 - lam_b) w[yb_b], D = sum_b (a_b + c_b):
//      CEm        = sum_b [ (1-eps) (a_b (lse_b - z[b,ya_b]) + c_b (lse_b - z[b,yb_b])) + (eps/N) sum_n w_n (lse_b - z[b,n]) ] / D
//      dCEm/dz_bn = ( (1-eps) (a_b (p_n - [n = ya_b]) + c_b (p_n - [n = yb_b])) + (eps/N) (p_n W - w_n) ) / D
//    lam == 1 everywhere is CEw in value, not in bits: keep * (a * nll + 0) and keep * wy * nll associate differently.
constexpr int LOSS_NMAX = 16;                          // widest row of the thread-per-row layout

struct CeW {
    float keep, smooth, W, invD;       // 1 - eps, eps/N, sum_n w_n, 1 / D
};
__device__ __forceinline__ int cew_label(long long y, int N) { return (int)(y < 0 ? 0 : y >= N ? N - 1 : y); }   // device data: clamped
// one logit's gradient; wy = w[y_b], wn = w_n, hit = [n == y_b]
__device__ __forceinline__ float cew_grad(const CeW& k, float wy, float p, float wn, bool hit) {
    return (k.keep * wy * (p - (hit ? 1.f : 0.f)) + k.smooth * (p * k.W - wn)) * k.invD;
}
// one row's loss term before the division by D; nll = lse - z_y, smo = sum_n w_n (lse - z_n)
__device__ __forceinline__ float cew_term(const CeW& k, float wy, float nll, float smo) { return k.keep * wy * nll + k.smooth * smo; }

struct CeMRow {
    int y[2];
    float a, c;                        // lam w[ya], (1 - lam) w[yb]
};
__device__ __forceinline__ float cem_lam(float lam) { return fminf(fmaxf(lam, 0.f), 1.f); }   // device data: clamped (NaN -> 0)
__device__ __forceinline__ CeMRow cem_row(const long long* __restrict__ ya, const long long* __restrict__ yb,
                                          const float* __restrict__ lam, int b, int N, const float* wl) {
    CeMRow r;
    r.y[0] = cew_label(ya[b], N);
    r.y[1] = cew_label(yb[b], N);
    const float l = cem_lam(lam[b]);
    r.a = l * wl[r.y[0]];
    r.c = (1.f - l) * wl[r.y[1]];
    return r;
}
__device__ __forceinline__ float cem_grad(const CeW& k, const CeMRow& r, float p, float wn, int n) {
    return (k.keep * (r.a * (p - (n == r.y[0] ? 1.f : 0.f)) + r.c * (p - (n == r.y[1] ? 1.f : 0.f))) + k.smooth * (p * k.W - wn)) * k.invD;
}
// one row's loss term before the division by D; nll_a = lse - z_ya, nll_b = lse - z_yb, smo = sum_n w_n (lse - z_n)
__device__ __forceinline__ float cem_term(const CeW& k, const CeMRow& r, float nll_a, float nll_b, float smo) {
    return k.keep * (r.a * nll_a + r.c * nll_b) + k.smooth * smo;
}

// The pre-pass of a rule with class weights, inside the launch (no atomics, the same bits every call): stages the weights (null =
// ones) in the caller's LDS `wl` and returns {1 - eps, eps/N, W, 1/D} to every thread.  W is summed in class order; D = sum_b
// rule.row_weight(b) per thread over its rows t, t + blockDim, ... in ascending order, then over the threads in thread order (`red`:
// blockDim floats of LDS, free again on return).
template <class Rule>
__device__ __forceinline__ CeW ce_prepass(const Rule& rule, int B, int N, float* wl, float* red) {
    __shared__ float dw[2];
    const int T = (int)blockDim.x;
    for (int n = threadIdx.x; n < N; n += T) wl[n] = rule.cw ? rule.cw[n] : 1.f;
    __syncthreads();
    float part = 0.f;
    for (int b = threadIdx.x; b < B; b += T) part += rule.row_weight(b, N, wl);
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
    return CeW{1.f - rule.eps, rule.eps / (float)N, dw[1], 1.f / dw[0]};
}

// A label rule: what the three cross-entropies do differently, handed to the kernel by value.  Its pointers and eps come from the
// entry point; begin() fills the rest on the device before the first row.  kLabels labels per row (Row::y); kWeights: class weights
// are staged in LDS (`wl`, else null and `wn` unused) and the smoothing sums `smo` are taken.  term(): a row's loss term from nll[j]
// = lse - z[y_j]; grad(): lead * d(batch loss)/dz_n at softmax value p, `lead` being 1 or beta (a product with 1.f is exact);
// inv(): the divisor handed to write_loss3.  The names are the entry point's in ign_last_error, its IgnScopedTimer label (null:
// untimed) and what ign_check_launch reports for the two layouts.
struct PlainRule {
    static constexpr bool kWeights = false;
    static constexpr int kLabels = 1;
    static constexpr const char *kEntry = "ign_loss_fwd_bwd", *kTimer = nullptr, *kNarrow = "ign_loss_kernel", *kWide = "ign_loss_wide_kernel";
    struct Row { int y[1]; };
    const long long* __restrict__ labels;
    float invB;
    bool pointers_ok() const { return labels; }
    __device__ __forceinline__ void begin(int B, int, float*, float*) { invB = 1.f / (float)B; }
    __device__ __forceinline__ Row row(int b, int, const float*) const { return Row{{(int)labels[b]}}; }   // not clamped
    __device__ __forceinline__ float term(const Row&, const float (&nll)[1], float) const { return nll[0]; }
    __device__ __forceinline__ float grad(float lead, const Row& r, float p, float, int n) const {
        return lead * (p - (n == r.y[0] ? 1.f : 0.f)) * invB;
    }
    __device__ __forceinline__ float inv() const { return invB; }
};

struct WeightedRule {
    static constexpr bool kWeights = true;
    static constexpr int kLabels = 1;
    static constexpr const char *kEntry = "ign_loss_w_fwd_bwd_reg", *kTimer = "loss_w", *kNarrow = "ign_loss_w_kernel",
                                *kWide = "ign_loss_w_wide_kernel";
    struct Row { int y[1]; float wy; };
    const long long* __restrict__ labels;
    const float* __restrict__ cw;
    float eps;
    CeW k;
    bool pointers_ok() const { return labels; }
    __device__ __forceinline__ float row_weight(int b, int N, const float* wl) const { return wl[cew_label(labels[b], N)]; }
    __device__ __forceinline__ void begin(int B, int N, float* wl, float* red) { k = ce_prepass(*this, B, N, wl, red); }
    __device__ __forceinline__ Row row(int b, int N, const float* wl) const {
        const int y = cew_label(labels[b], N);
        return Row{{y}, wl[y]};
    }
    __device__ __forceinline__ float term(const Row& r, const float (&nll)[1], float smo) const { return cew_term(k, r.wy, nll[0], smo); }
    __device__ __forceinline__ float grad(float lead, const Row& r, float p, float wn, int n) const {
        return lead * cew_grad(k, r.wy, p, wn, n == r.y[0]);
    }
    __device__ __forceinline__ float inv() const { return k.invD; }
};

struct SoftRule {
    static constexpr bool kWeights = true;
    static constexpr int kLabels = 2;
    static constexpr const char *kEntry = "ign_loss_mix_fwd_bwd_reg", *kTimer = "loss_mix", *kNarrow = "ign_loss_mix_kernel",
                                *kWide = "ign_loss_mix_wide_kernel";
    using Row = CeMRow;
    const long long* __restrict__ labels;
    const long long* __restrict__ labels_b;
    const float* __restrict__ lam;
    const float* __restrict__ cw;
    float eps;
    CeW k;
    bool pointers_ok() const { return labels && labels_b && lam; }
    __device__ __forceinline__ float row_weight(int b, int N, const float* wl) const {
        const CeMRow r = row(b, N, wl);
        return r.a + r.c;
    }
    __device__ __forceinline__ void begin(int B, int N, float* wl, float* red) { k = ce_prepass(*this, B, N, wl, red); }
    __device__ __forceinline__ Row row(int b, int N, const float* wl) const { return cem_row(labels, labels_b, lam, b, N, wl); }
    __device__ __forceinline__ float term(const Row& r, const float (&nll)[2], float smo) const { return cem_term(k, r, nll[0], nll[1], smo); }
    __device__ __forceinline__ float grad(float lead, const Row& r, float p, float wn, int n) const { return lead * cem_grad(k, r, p, wn, n); }
    __device__ __forceinline__ float inv() const { return k.invD; }
};

// the rule's class weights in LDS: NW floats, or nothing
template <class Rule, int NW>
__device__ __forceinline__ float* class_weights_lds() {
    if constexpr (Rule::kWeights) {
        __shared__ float wl[NW];
        return wl;
    } else {
        return nullptr;
    }
}

// N <= LOSS_NMAX.  One block; thread <-> rows b, b+256, ...; the two CE sums are reduced through LDS in thread order (deterministic).
template <class Rule>
__global__ void __launch_bounds__(256) ign_loss_kernel(const float* __restrict__ s, const float* __restrict__ d, Rule rule,
                                                       float* __restrict__ out, float* __restrict__ eta_out,
                                                       float* __restrict__ loss3, float* __restrict__ gs, float* __restrict__ gd,
                                                       int B, int N, float beta, const float* __restrict__ reg) {
    __shared__ float red[2][256];
    float* wl = class_weights_lds<Rule, LOSS_NMAX>();
    rule.begin(B, N, wl, red[0]);
    float ce_o = 0.f, ce_s = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        float sv[LOSS_NMAX], ov[LOSS_NMAX], q[LOSS_NMAX];
        const float* sr = s + (long long)b * N;
        const float* dr = d + (long long)b * N;
        const typename Rule::Row row = rule.row(b, N, wl);
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
        if constexpr (Rule::kWeights)
            for (int n = 0; n < N; ++n) {
                smo_s += wl[n] * (lse_s - sv[n]);
                smo_o += wl[n] * (lse_o - ov[n]);
            }
        float nll_s[Rule::kLabels], nll_o[Rule::kLabels];
#pragma unroll
        for (int j = 0; j < Rule::kLabels; ++j) {
            nll_s[j] = lse_s - sv[row.y[j]];
            nll_o[j] = lse_o - ov[row.y[j]];
        }
        ce_s += rule.term(row, nll_s, smo_s);
        ce_o += rule.term(row, nll_o, smo_o);
        // gradients: g_out = dCE(out)/dout ; through the gate ; + beta * dCE(s)/ds
        float dot = 0.f;
        float go[LOSS_NMAX];
        for (int n = 0; n < N; ++n) {
            go[n] = rule.grad(1.f, row, expf(ov[n] - mo) / zo, Rule::kWeights ? wl[n] : 0.f, n);
            dot += go[n] * (sv[n] - dr[n]);
        }
        const float c = gate_coef(N, dot);
        for (int n = 0; n < N; ++n) {
            const float qn = q[n] / z;
            gs[(long long)b * N + n] = gate_ds(eta, go[n], c, qn, G) + rule.grad(beta, row, qn, Rule::kWeights ? wl[n] : 0.f, n);
            gd[(long long)b * N + n] = gate_dd(eta, go[n]);
        }
    }
    red[0][threadIdx.x] = ce_o;
    red[1][threadIdx.x] = ce_s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b2 = 0.f;
        for (int i = 0; i < 256; ++i) { a += red[0][i]; b2 += red[1][i]; }
        write_loss3(loss3, a, b2, rule.inv(), beta, reg);
    }
}

// LOSS_NMAX < N <= IGN_HEAD_NMAX: one block of 16 waves, one wave per row (rows w, w + 16, ...), the lanes cover the classes in
// chunks of 64 and every row-wide max / sum is a butterfly over the wave (each lane ends with the same value), so its sums are not
// bitwise ign_loss_kernel's or the gate kernels'.  Each row's two CE terms go to LDS at their row index; one thread adds them in
// ascending row order (LOSS_TILE rows at a time), so the batch mean does not depend on how the waves were scheduled.
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
template <class Rule>
__global__ void __launch_bounds__(LOSS_WAVES * 64) ign_loss_wide_kernel(const float* __restrict__ s, const float* __restrict__ d, Rule rule,
                                                                        float* __restrict__ out, float* __restrict__ eta_out,
                                                                        float* __restrict__ loss3, float* __restrict__ gs,
                                                                        float* __restrict__ gd, int B, int N, float beta,
                                                                        const float* __restrict__ reg) {
    __shared__ float ce[2][LOSS_TILE];
    static_assert(LOSS_TILE >= LOSS_WAVES * 64, "ce_prepass borrows one row of `ce` for its per-thread sums");
    float* wl = class_weights_lds<Rule, IGN_HEAD_NMAX>();
    rule.begin(B, N, wl, ce[0]);
    float tot[2] = {0.f, 0.f};                         // {CE(out), CE(s)} batch sums before the division, meaningful in thread 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < B; base += LOSS_TILE) {
        const int rows = min(LOSS_TILE, B - base);
        for (int r = wave; r < rows; r += LOSS_WAVES) {
            const int b = base + r;
            const float* sr = s + (long long)b * N;
            const float* dr = d + (long long)b * N;
            const typename Rule::Row row = rule.row(b, N, wl);
            float sv[LOSS_KMAX], dv[LOSS_KMAX], q[LOSS_KMAX], ov[LOSS_KMAX], eo[LOSS_KMAX], wv[LOSS_KMAX];
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                const int n = k * 64 + lane;
                sv[k] = n < N ? sr[n] : -INFINITY;
                dv[k] = n < N ? dr[n] : 0.f;
                wv[k] = Rule::kWeights && n < N ? wl[n] : 0.f;
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
            float mo = -INFINITY, s_y[Rule::kLabels] = {}, o_y[Rule::kLabels] = {};
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                const int n = k * 64 + lane;
                ov[k] = gate_mix(eta, sv[k], dv[k]);
                if (n < N) {
                    out[(long long)b * N + n] = ov[k];
                    mo = fmaxf(mo, ov[k]);
                }
#pragma unroll
                for (int j = 0; j < Rule::kLabels; ++j)
                    if (n == row.y[j]) { s_y[j] = sv[k]; o_y[j] = ov[k]; }
            }
            mo = wave_max(mo);
#pragma unroll
            for (int j = 0; j < Rule::kLabels; ++j) {
                s_y[j] = wave_sum(s_y[j]);        // exactly one lane holds a label's logits, the others add zeros
                o_y[j] = wave_sum(o_y[j]);
            }
            float zo = 0.f;
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                eo[k] = k * 64 + lane < N ? expf(ov[k] - mo) : 0.f;
                zo += eo[k];
            }
            zo = wave_sum(zo);
            const float lse_s = mx + logf(z), lse_o = mo + logf(zo);
            float smo_s = 0.f, smo_o = 0.f;
            if constexpr (Rule::kWeights) {
#pragma unroll
                for (int k = 0; k < LOSS_KMAX; ++k)
                    if (k * 64 + lane < N) {      // the padding lanes hold -inf logits
                        smo_s += wv[k] * (lse_s - sv[k]);
                        smo_o += wv[k] * (lse_o - ov[k]);
                    }
                smo_s = wave_sum(smo_s);
                smo_o = wave_sum(smo_o);
            }
            // gradients: g_out = dCE(out)/dout ; through the gate ; + beta * dCE(s)/ds
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                const int n = k * 64 + lane;
                eo[k] = rule.grad(1.f, row, eo[k] / zo, wv[k], n);               // go
                if (n < N) dot += eo[k] * (sv[k] - dv[k]);
            }
            dot = wave_sum(dot);
            const float c = gate_coef(N, dot);
#pragma unroll
            for (int k = 0; k < LOSS_KMAX; ++k) {
                const int n = k * 64 + lane;
                if (n < N) {
                    const float qn = q[k] / z;
                    gs[(long long)b * N + n] = gate_ds(eta, eo[k], c, qn, G) + rule.grad(beta, row, qn, wv[k], n);
                    gd[(long long)b * N + n] = gate_dd(eta, eo[k]);
                }
            }
            if (lane == 0) {
                float nll_s[Rule::kLabels], nll_o[Rule::kLabels];
#pragma unroll
                for (int j = 0; j < Rule::kLabels; ++j) {
                    nll_s[j] = lse_s - s_y[j];
                    nll_o[j] = lse_o - o_y[j];
                }
                ce[0][r] = rule.term(row, nll_o, smo_o);
                ce[1][r] = rule.term(row, nll_s, smo_s);
            }
        }
        add_in_row_order(ce, rows, tot);
    }
    if (threadIdx.x == 0) write_loss3(loss3, tot[0], tot[1], rule.inv(), beta, reg);
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

// The one launcher of the CE tail: the checks, the layout choice, the launch.
template <class Rule>
static int ce_tail_launch(const float* sbm, const float* dnn, Rule rule, const float* reg, float* out, float* eta, float* loss3,
                          float* gsbm, float* gdnn, int B, int N, float beta, void* stream) {
    if (!sbm || !dnn || !rule.pointers_ok() || !out || !eta || !loss3 || !gsbm || !gdnn || B <= 0 || N < 2) {
        ign_set_error("%s: null pointer or bad dimension (B=%d N=%d, N <= %d)", Rule::kEntry, B, N, IGN_HEAD_NMAX);
        return IGN_E_ARG;
    }
    if constexpr (Rule::kWeights)
        if (!(rule.eps >= 0.f && rule.eps < 1.f)) {
            ign_set_error("%s: label_smoothing=%g outside [0, 1)", Rule::kEntry, (double)rule.eps);
            return IGN_E_ARG;
        }
    if (N > IGN_HEAD_NMAX) { ign_set_error("%s: N=%d classes > %d", Rule::kEntry, N, IGN_HEAD_NMAX); return IGN_E_UNSUP; }
    const bool wide = N > LOSS_NMAX;
    auto launch = [&] {
        hipLaunchKernelGGL(wide ? ign_loss_wide_kernel<Rule> : ign_loss_kernel<Rule>, dim3(1), dim3(wide ? LOSS_WAVES * 64 : 256), 0,
                           (hipStream_t)stream, sbm, dnn, rule, out, eta, loss3, gsbm, gdnn, B, N, beta, reg);
    };
    if (Rule::kTimer) {
        IgnScopedTimer tm(Rule::kTimer, (hipStream_t)stream);
        launch();
    } else {
        launch();
    }
    return ign_check_launch(wide ? Rule::kWide : Rule::kNarrow);
}

extern "C" int ign_loss_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const float* reg, float* out,
                                    float* eta, float* loss2, float* gsbm, float* gdnn, int B, int N, float beta, void* stream) {
    return ce_tail_launch(sbm, dnn, PlainRule{labels, 0.f}, reg, out, eta, loss2, gsbm, gdnn, B, N, beta, stream);
}

extern "C" int ign_loss_fwd_bwd(const float* sbm, const float* dnn, const long long* labels, float* out, float* eta, float* loss2,
                                float* gsbm, float* gdnn, int B, int N, float beta, void* stream) {
    return ign_loss_fwd_bwd_reg(sbm, dnn, labels, nullptr, out, eta, loss2, gsbm, gdnn, B, N, beta, stream);
}

extern "C" int ign_loss_w_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const float* class_w,
                                      const float* reg, float* out, float* eta, float* loss3, float* gsbm, float* gdnn, int B, int N,
                                      float beta, float label_smoothing, void* stream) {
    return ce_tail_launch(sbm, dnn, WeightedRule{labels, class_w, label_smoothing, {}}, reg, out, eta, loss3, gsbm, gdnn, B, N, beta,
                          stream);
}

extern "C" int ign_loss_mix_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const long long* labels_b,
                                        const float* lam_b, const float* class_w, const float* reg, float* out, float* eta,
                                        float* loss3, float* gsbm, float* gdnn, int B, int N, float beta, float label_smoothing,
                                        void* stream) {
    return ce_tail_launch(sbm, dnn, SoftRule{labels, labels_b, lam_b, class_w, label_smoothing, {}}, reg, out, eta, loss3, gsbm, gdnn, B,
                          N, beta, stream);
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
