/* ign_abi.h -- C ABI of libign_hip.so: the MI355X (gfx950) hot path of the Interpretability-Gated-Network.
 *
 * The reference (001camellia/Speech-Imagery-EEG, IGN/ = InterpretGatedNetwork/) has no FFI: its hot path is a
 * chain of PyTorch eager ops inside Python modules.  Each entry point below replaces one such chain; the
 * reference lines it stands in for are cited per function.  Binding side: INTEGRATION.md (ctypes).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (contiguous fp32 unless noted); the library never
 *    allocates or frees device memory; its only mutable state is the optional timing registry (ign_timing_*);
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); kernels are enqueued and the call
 *    returns immediately;
 *  - return 0 on success; IGN_E_* (<0) on argument errors (nothing was launched); -(hipError_t) on a launch error;
 *    ign_last_error() gives a human-readable reason for the calling thread;
 *  - `workspace` buffers are caller-provided, sized by the matching *_workspace_bytes().
 */
#ifndef IGN_ABI_H
#define IGN_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGN_ABI_VERSION 1

#define IGN_E_ARG      (-1001)  /* bad pointer / dimension                                */
#define IGN_E_UNSUP    (-1002)  /* combination not implemented (see message)              */
#define IGN_E_TOOBIG   (-1003)  /* a row does not fit the LDS staging budget              */

/* Largest class count N of the class-head GEMMs (ign_head_*) and the fused loss tail (ign_loss_*); above it they return
 * IGN_E_UNSUP.  N <= 16 runs the single-pass kernels; wider heads run in 16-class chunks with the same launch count.      */
#define IGN_HEAD_NMAX  256

/* distance / gate selectors: `mode` = IGN_DIST_* | IGN_GATE_*                                           */
#define IGN_DIST_L1    0   /* mean |x-w|      IGN/model/Shapelet.py:74 ("euclidean", the default)        */
#define IGN_DIST_MSE   1   /* mean (x-w)^2    IGN/model/Shapelet.py:24-40 (memory_efficient branch)      */
#define IGN_DIST_COS   2   /* 1 - cos         IGN/model/Shapelet.py:64-66                                */
#define IGN_DIST_PEARS 3   /* 1 - pearson     IGN/model/Shapelet.py:67-69,11-19                          */
#define IGN_GATE_RBF   0x00 /* exp(-(eps d)^2) + straight-through max   IGN/model/Shapelet.py:77-84      */
#define IGN_GATE_LTS   0x10 /* straight-through soft-min + sigmoid(thr - min_d)  Shapelet.py:105-111     */
#define IGN_TIE_EXACT  0x20 /* opt-in: L1 backward passes use sign(0) = 0 at x == w, as aten::sgn (see below) */

int         ign_abi_version(void);
const char* ign_last_error(void);

/* Instance normalisation fused with the (B,T,C) -> (B,C,T) transpose.
 * Replaces IGN/model/Shapelet.py:186-187  (rearrange 'b t c -> b c t'; (x-mean_T)/(std_T(unbiased)+eps)).
 * xt_bct (nullable) additionally receives the un-normalised transpose (input of the FCN expert,
 * IGN/model/FullyConvNet.py:53).                                                                        */
int ign_instnorm_fwd(const float* x_btc, float* xn_bct, float* xt_bct, int B, int T, int C, float eps,
                     void* stream);
/* Same pass, additionally max |x| of the raw input as an atomic maximum into *amax_slot (caller zeroes it): the magnitude bound
 * of the FCN expert's first fp16 GEMM operand (ign_clconv_fwd_h3), taken where the batch is staged anyway instead of by a
 * separate ign_absmax pass when both experts run on one stream.                                                              */
int ign_instnorm_fwd_amax(const float* x_btc, float* xn_bct, float* xt_bct, int B, int T, int C, float eps, float* amax_slot,
                          void* stream);

/* Plain (B,T,C) -> (B,C,T) transpose of a batch: what `x.permute(0, 2, 1)` means for a consumer that needs electrodes-first rows
 * (the EEG-CNN baseline, IGN/model/eegcnn.py:134, fed from the time-first item contract of IGN/data_factory/uea.py).           */
int ign_transpose_btc_to_bct(const float* x_btc, float* out_bct, int B, int T, int C, void* stream);

/* On-GPU input pipeline of the CHISCO loader: raw (B,C,T) recordings -> standardised (B,T,C) batches.
 * Replaces, per batch, Normalizer('per_sample_std') of IGN/data_factory/eeg.py:332-367 (per sample and channel over time:
 * (x - mean) / (std(ddof=1) + eps)) and the (C,T) -> (T,C) item transpose that IGN/data_factory/uea.py:7-42 batches.
 * stats_ws: B*C*2 floats of workspace (mean, 1/(std+eps) per row).                                                    */
int ign_standardise_nct_to_btc(const float* x_nct, float* out_btc, float* stats_ws, int B, int C, int T, float eps,
                               void* stream);

/* EEG preprocessing in front of the standardisation (csrc/ign_eeg_preprocess.hip; run.py --eeg_preprocess; numpy restatement
 * utils/eeg_filter.py:filterbank_numpy): raw (B,Cin,Tin) recordings -> nb centred FIR filters of one common length, decimate by q,
 * crop / zero-pad every band to (Tout,Cout), standardise, transpose -> out (B,Tout,nb*Cout).  What the reference's loader does on the
 * CPU with scipy.signal.decimate(ftype='fir', zero_phase=True) and its channel / time fitting (IGN/data_factory/eeg_processor.py:
 * 258-381), here for a whole batch and several bands in front of the per-sample statistics.  One rule, one launcher; the four entry
 * points below differ only in what they fix.
 *   taps (nb,M) and optional quadrature taps quad (nb,M), fp32 on the DEVICE, M odd, R = (M-1)/2;  x~ = the row extended by R
 *   samples: zeros (IGN_EDGE_ZERO) or mirrored about the end samples, x~[-i] = x[i], x~[Tin-1+i] = x[Tin-1-i] (IGN_EDGE_REFLECT,
 *   numpy pad 'reflect'; needs R <= Tin-1).  Per band j and row (b, c < min(Cin,Cout)):
 *   a_j[n] = sum_k taps[j,k] * x~[n*q + R - k],  n < Td = ceil(Tin/q)   (a convolution, centred: zero-phase for symmetric taps)
 *   quad == NULL:  f_j = a_j;   else  b_j[n] = the same sum with quad[j,k],  f_j[n] = sqrtf(fmaf(a_j[n], a_j[n], b_j[n] * b_j[n]))
 *   Tv = min(Td, Tout); mean and unbiased std of f_j[0..Tv-1] in two sweeps;
 *   out[b,t,j*Cout+c] = (f_j[t] - mean) / (std + eps) for t < Tv; exactly 0 for Tv <= t < Tout and for Cin <= c < Cout.
 * out is BAND-MAJOR: channel j*Cout + c is electrode c of band j; every band block is cropped / zero-padded to Cout electrodes on its
 * own.  The extended row is staged once per (b,c) and every band runs over it with the same tap walk, so block j does not depend on
 * the other bands: without quad it is the bank of one for taps[j], bit for bit.
 * In reflect mode with M > 1 the kernel filters x - x[b,c,0] (a constant passes reflect-extended filtering up to the factor
 * sum(taps[j]) and the standardisation removes it): the same value, without the recording's offset in the fp32 products.  M = 1
 * extends nothing and takes no pivot; the statistics run in ign_standardise_nct_to_btc's order, so nb = 1, taps {1} with Cout = Cin,
 * Tout = Tin give that entry point's output bit for bit.  Fixed summation order, no atomics: two calls give the same bits.  Nothing
 * outside [0,Tin) of a row is read; taps longer than the row are legal in zero mode.
 * ws: ign_eeg_filterbank_ws_bytes() bytes (B * nb * min(Cin,Cout) * Tv floats; 0 for arguments the launcher refuses).
 * IGN_E_ARG: null pointer, nb outside 1..IGN_EEG_MAX_BANDS, non-positive dimension, M even or > IGN_EEG_MAX_TAPS, q outside
 * 1..IGN_EEG_MAX_DECIMATE, unknown edge, reflect with R >= Tin, quad with IGN_EDGE_ZERO (without the pivot the recording's offset
 * times sum(taps[j]) enters the square root and the standardisation cannot remove it), quad with M == 1, Tv < 2.  IGN_E_TOOBIG: a row
 * whose phase-split image and filtered copy exceed 64 KB of LDS ((Tin + M - 1 + q*4 + Tv) floats, whatever nb), or B > 65535.
 * Nothing is launched on an error; the error text names the entry point that was called.                                      */
#define IGN_EDGE_REFLECT     0
#define IGN_EDGE_ZERO        1
#define IGN_EEG_MAX_TAPS     1023
#define IGN_EEG_MAX_DECIMATE 16
/* One band: the bank of one.  taps (M); the same as the entry points below with nb = 1 and quad = NULL, out (B,Tout,Cout),
 * ws B * min(Cin,Cout) * Tv floats.                                                                                            */
size_t ign_eeg_preprocess_ws_bytes(int B, int Cin, int Tin, int M, int q, int Cout, int Tout);
int ign_eeg_preprocess_nct_to_btc(const float* x_nct, const float* taps, float* out_btc, float* ws, int B, int Cin, int Tin, int M,
                                  int q, int edge, int Cout, int Tout, float eps, void* stream);

/* The rule above in full (run.py --eeg_preprocess bank=... / envelope; ops.eeg_filterbank).                                    */
#define IGN_EEG_MAX_BANDS 8
size_t ign_eeg_filterbank_ws_bytes(int B, int Cin, int Tin, int M, int nb, int q, int Cout, int Tout);
int ign_eeg_filterbank_nct_to_btc(const float* x_nct, const float* taps, const float* quad, float* out_btc, float* ws, int B, int Cin,
                                  int Tin, int M, int nb, int q, int edge, int Cout, int Tout, float eps, void* stream);

/* Spatial filter stage in front of all of the above (csrc/ign_eeg_spatial.hip; run.py --eeg_spatial; ops.eeg_spatial / ops.eeg_gram;
 * numpy restatement utils/eeg_spatial.py:spatial_numpy / gram_numpy): one (Cs,Cin) matrix per group of samples applied across the
 * electrodes of the raw batch -- a common average reference, a montage / unmixing matrix computed offline, the per-subject
 * whitening of Euclidean alignment (He & Wu 2020).  x (B,Cin,T) fp32 raw, w (G,Cs,Cin) fp32, gid (B) int32 or NULL (group 0),
 * out (B,Cs,T) in the input's layout, so ign_standardise_nct_to_btc or the filter bank run on it unchanged.  With g = gid[b]:
 *   p[c] = x[b,c,0];  xc[c,t] = x[b,c,t] - p[c];
 *   a[s,t] = fmaf chain over c = 0..Cin-1 ascending of w[g,s,c] * xc[c,t], from 0;  P[s] = the same chain of w[g,s,c] * p[c];
 *   out[b,s,t] = a[s,t] + P[s]
 * The pivot keeps the recording's offset (1e4 uV over tens of uV of signal) out of the chain's partial sums: it enters once per
 * row, as a constant that the standardisation removes.  The chain runs on v_mfma_f32_32x32x2_f32 (exact fp32 on gfx950, k in
 * ascending order; Cin is padded with zeros, which leaves the bits alone).  A gid outside [0,G) writes zeros for that sample and
 * reads nothing out of bounds.  No atomics, fixed order: two calls give the same bits, and sample b's output does not depend on B or
 * on its position in the batch.  Nothing beyond Cs, T and Cin is read or written.
 * IGN_E_ARG: null x / w / out, non-positive dimension.  IGN_E_TOOBIG: B > 65535, Cin or Cs > IGN_EEG_SPATIAL_MAX_CHANNELS,
 * G > IGN_EEG_SPATIAL_MAX_GROUPS.  Nothing is launched on an error.                                                             */
#define IGN_EEG_SPATIAL_MAX_CHANNELS 512
#define IGN_EEG_SPATIAL_MAX_GROUPS   64
int ign_eeg_spatial_nct(const float* x_nct, const float* w_gsc, const int* gid, float* out_nst, int B, int Cin, int T, int Cs, int G,
                        void* stream);

/* Per-group Gram matrix of a (B,C,T) fp32 batch (the spatial stage's own output while an alignment is fitted):
 *   xc = x - x[..,:1];  m[c] = (sum_t xc[c,t]) / T;  z = xc - m
 *   gram[g,i,j] = sum over b with gid[b] == g, ascending, of sum_t z[b,i,t] * z[b,j,t];   count[g] = number of such b
 * Every element of gram (G,C,C) and count (G) is OVERWRITTEN (zeros for an empty group; a gid outside [0,G) belongs to no group);
 * the host accumulates batches in float64.  Same matrix cores; only the upper triangle of 64 x 64 tiles is computed, per sample,
 * into ws, and summed in ascending b with element (j,i) read from (i,j): gram[g] is symmetric bit for bit.  No atomics.
 * ws: ign_eeg_gram_ws_bytes() bytes (B*C + B*C*C floats; 0 for arguments the launcher refuses).
 * IGN_E_ARG: null x / gram / count / ws, non-positive dimension.  IGN_E_TOOBIG: B > 65535, C > IGN_EEG_SPATIAL_MAX_CHANNELS,
 * G > IGN_EEG_SPATIAL_MAX_GROUPS.  Nothing is launched on an error.                                                             */
size_t ign_eeg_gram_ws_bytes(int B, int C, int T, int G);
int ign_eeg_gram_nct(const float* x_nct, const int* gid, float* gram_gcc, int* count_g, float* ws, int B, int C, int T, int G,
                     void* stream);

/* Zero-phase IIR stage behind the spatial filter and in front of the FIR / standardisation stages (csrc/ign_eeg_iir.hip; run.py
 * --eeg_iir; ops.eeg_iir; the rule in numpy float64: utils/eeg_iir.py:iir_numpy): a cascade of ns second-order sections applied
 * forward and backward along time to every (b,c) row -- scipy.signal.sosfiltfilt(sos, x, padtype='odd', padlen=P) -- for what FIR
 * filters cannot do inside a trial: a 0.5 Hz high-pass, a 50 Hz notch 1-2 Hz wide.  x (B,C,T) fp32 raw, out (B,C,T) fp32,
 * coef (ns,8) DOUBLE on the device, rows (b0, b1, b2, a1, a2, zi1, zi2, 0) with a0 = 1 (utils/eeg_iir.py:section_table), g0 the
 * squared DC gain of the cascade.  Per row:
 *   p = x[0];  u = double(x) - double(p);  ue = the odd extension of u by P samples on both sides (N = T + 2P)
 *   section k, state (s1,s2):  y = b0*v + s1;  s1 = (b1*v - a1*y) + s2;  s2 = b2*v - a2*y
 *   forward from the states zi_k * ue[0], then the same cascade over the reversed result from zi_k * (its first sample)
 *   out[t] = float(back[P+t] + g0*p)
 * All arithmetic between the load and the store is double.  One wave per row, the extended row staged as doubles in LDS
 * (ign_eeg_iir_lds_bytes(); 0 for arguments the launcher refuses), 64 chunks whose start states come from a fixed six-step scan across
 * the lanes (within 2e-11 of the row's scale of the sequential evaluation): no workspace, no atomics, two calls give the same bits,
 * and a row's output does not depend on B, C or its position.  x is read inside [0,T) only.
 * IGN_E_ARG: null x / coef / out, non-positive dimension, ns outside 1..IGN_EEG_IIR_MAX_SECTIONS, P < 0, P >= T.
 * IGN_E_TOOBIG: T + 2P > IGN_EEG_IIR_MAX_ROW (64 KB of doubles), B*C beyond the launch grid.  Nothing is launched on an error.   */
#define IGN_EEG_IIR_MAX_SECTIONS 8
#define IGN_EEG_IIR_MAX_ROW      8192
size_t ign_eeg_iir_lds_bytes(int T, int P);
int ign_eeg_iir_nct(const float* x_nct, const double* coef, float* out_nct, int B, int C, int T, int ns, int P, double g0, void* stream);

/* Rational resampling stage behind the IIR stage and in front of the FIR / standardisation stages (csrc/ign_eeg_resample.hip; run.py
 * --eeg_resample; ops.eeg_resample; the rule in numpy float64: utils/eeg_resample.py:resample_numpy): every (b,c) row goes from Tin to
 * Tout = ceil(Tin*up/down) samples through the polyphase Kaiser-windowed low-pass that scipy.signal.resample_poly designs.
 * x (B,C,Tin) fp32 raw, out (B,C,Tout) fp32, up/down in lowest terms, tab (up,Lp) fp32 on the device: tab[r][i] = h[r + i*up] of the
 * 2*hl+1 taps h (DC gain up), zero past the last tap, Lp = ceil((2*hl+1)/up) (utils/eeg_resample.py:design_taps, phase_table).  Per row:
 *   p = x[0];  u = x - p;  ue = u extended by R = Lp samples on both sides: mirrored about the end samples (IGN_EDGE_REFLECT) or zeros
 *   (IGN_EDGE_ZERO: out - p is scipy.signal.resample_poly(u, up, down))
 *   n in [0,Tout):  a = n*down + hl;  khi = a div up;  r = a mod up
 *   out[n] = p + sum_{i<Lp} tab[r][i] * ue[khi - i]        one fmaf chain, i ascending
 * The pivot p re-enters with gain exactly 1, not with the phase's DC gain sum_i tab[r][i] (which differs from 1 by up to 1.4e-4 at
 * 64/125 and would print a ripple of the recording's offset onto the signal): a constant row gives p bit for bit.
 * One workgroup per row; the extended row and the table (row stride Lp|1) are staged in LDS (ign_eeg_resample_lds_bytes(); 0 for
 * arguments the launcher refuses).  One launch, no workspace, no atomics, two calls give the same bits, a row's output does not depend
 * on B, C or its position; x is read inside [0,Tin) only and every element of out is written.
 * IGN_E_ARG: null x / tab / out, non-positive dimension, up/down not in lowest terms, Lp != ceil((2*hl+1)/up),
 * Tout != ceil(Tin*up/down), unknown edge, reflect with R >= Tin.  IGN_E_TOOBIG: up*Lp > IGN_EEG_RESAMPLE_MAX_TABLE, a row plus table
 * over 64 KB of LDS, B*C beyond the launch grid.  Nothing is launched on an error.                                                     */
#define IGN_EEG_RESAMPLE_MAX_TABLE 8192
size_t ign_eeg_resample_lds_bytes(int Tin, int up, int Lp);
int ign_eeg_resample_nct(const float* x_nct, const float* tab, float* out_nct, int B, int C, int Tin, int Tout, int up, int down, int hl,
                         int Lp, int edge, void* stream);

/* Artifact stage in FRONT of the spatial filter (csrc/ign_eeg_artifact.hip; run.py --eeg_artifact; ops.eeg_artifact; the rule in
 * numpy: utils/eeg_artifact.py:artifact_numpy): robust row statistics, a verdict per electrode, a clamp of the good rows, the bad
 * rows rebuilt from the good ones.  x (B,C,T) fp32 raw, out (B,C,T) fp32, stats (B,C,2) fp32 (m, s), flags (B,C) u8 (0, or 3 for a
 * row with a non-finite sample), verdict (B,C) u8: 0 good, 1 flat, 2 noisy, 3 non-finite, 4 unrepaired; w (C,C) fp32 non-negative
 * neighbour weights on the device, or NULL: all ones (the diagonal is never read).  med = the LOWER median, the element of rank
 * (n-1)/2.  Per sample:
 *   m_c = med(x[c]) (+0 for -0);  s_c = med(|x[c] - m_c|), each difference rounded once;  a non-finite row: flag 3, stats (0,0)
 *   ref = med(s_c over the finite rows);  flat: s_c <= fl(flat*ref);  noisy: s_c > fl(noisy*ref);  no good row left: every bad row
 *   gets 4 and is clamped only (a non-finite one: zeros)
 *   good rows, clip > 0:  r = fl(fl(clip*1.4826f)*s_c);  lo = fl(m_c - r);  hi = fl(m_c + r);  y = x < lo ? lo : x > hi ? hi : x
 *   bad row c:  y[c,t] = (sum_j w[c,j]*fl(y[j,t] - m_j)) / (sum_j w[c,j]),  j over the good rows ascending, j != c, one fmaf chain;
 *   the weights' sum is rounded once; without a good j of positive weight: all ones over the good rows
 * A non-positive clip, flat or noisy means the key is absent.  ign_eeg_artifact_stats_nct is one launch: the row as ordered keys and the
 * rank element found by a bitwise select (32 counting passes), exact whatever the ties -- rows of up to 2048 samples in registers, one
 * wave per row, no LDS; longer rows staged in LDS, one workgroup per row (ign_eeg_artifact_lds_bytes(): what a row of T samples costs
 * when it is staged; 0 for a T the launcher refuses).  ign_eeg_artifact_apply_nct is two launches: the verdicts (one workgroup per sample), then tiles of
 * (all C, 16..64 samples) whose clamped good rows go through LDS.  No atomics, no workspace beyond stats / flags, two calls give the
 * same bits; every element of stats, flags, out and verdict is written; a row's statistics do not depend on B, C or its position, a
 * sample's output not on B or its position.
 * IGN_E_ARG: null x / stats / flags / out / verdict, non-positive dimension.  IGN_E_TOOBIG: T > IGN_EEG_ARTIFACT_MAX_ROW,
 * C > IGN_EEG_ARTIFACT_MAX_CHANNELS, B*C beyond the launch grid.  Nothing is launched on an error.                                  */
#define IGN_EEG_ARTIFACT_MAX_ROW      16384
#define IGN_EEG_ARTIFACT_MAX_CHANNELS 1024
size_t ign_eeg_artifact_lds_bytes(int T);
int ign_eeg_artifact_stats_nct(const float* x_nct, float* stats, unsigned char* flags, int B, int C, int T, void* stream);
int ign_eeg_artifact_apply_nct(const float* x_nct, const float* stats, const unsigned char* flags, const float* w, float* out_nct,
                               unsigned char* verdict, int B, int C, int T, float clip, float flat, float noisy, void* stream);

/* Shapelet transform of ONE length group: sliding-window distance + gate, never materialising (B,Tw,K,C,L).
 * Replaces IGN/model/Shapelet.py:60-84 (GATE_RBF) / :96-111 (GATE_LTS).   Tw = (T-L)/stride + 1.
 *   xn_bct   (B,C,T)    normalised input
 *   w_kcl    (K,C,L)    shapelets            thr_kc (K,C) LTS thresholds (NULL for RBF)
 *   p_out    row-major (B, ld) ; this group writes columns [col0 + k*C + c]     (max_p / sigmoid gate)
 *   dmin_out same indexing                                                       (min_t d)
 *   tstar    (B,K,C) int32  arg-max_t p  (RBF) / arg-min_t d (LTS); first index on ties (torch.argmax)
 *   zmu      (B,K,C,2)      {Z, mu}: RBF Z=sum_t exp(p_t), mu=sum_t softmax_t(p) p_t ;
 *                           LTS Z=sum_t exp(-(d_t-dmin)), mu=sum_t softmin_t(d) d_t      (for backward)
 *   d_save   (B,C,K,Tw)     every window distance, kept for the backward (NULL: not saved)
 *   xstat_save (B,C,Tw)     cosine / pearson only (else NULL): |x_win| resp. sqrt(sum (x_win-mean)^2), for the backward
 * IGN_DIST_PEARS expects w_kcl already CENTRED over its last axis (w - mean_j w; the caller's autograd projects the
 * gradient back), so that <x_win, w_c> equals the reference's centred numerator (Shapelet.py:11-19).               */
int ign_shapelet_fwd(const float* xn_bct, const float* w_kcl, const float* thr_kc,
                     float* p_out, float* dmin_out, int ld, int col0,
                     int32_t* tstar, float* zmu, float* d_save, float* xstat_save,
                     int B, int C, int T, int K, int L, int stride, float eps, int mode, void* stream);

/* All G (<= 8) length groups of a bank -- the loop over `self.shapelets` of IGN/model/Shapelet.py:190-196 -- in one call: the
 * per-group arguments of ign_shapelet_fwd as tables of G entries (host arrays; the outputs share p_out / dmin_out / ld).  Every
 * group is validated before the first launch; results are bitwise those of G ign_shapelet_fwd calls.                         */
int ign_shapelet_fwd_bank(const float* xn_bct, int G, const float* const* w_kcl, const float* const* thr_kc, float* p_out,
                          float* dmin_out, int ld, const int* col0, int32_t* const* tstar, float* const* zmu,
                          float* const* d_save, float* const* xstat_save, int B, int C, int T, const int* K, const int* L,
                          const int* stride, float eps, int mode, void* stream);

/* Backward of the above w.r.t. the shapelets (autograd of Shapelet.py:60-84 / :96-111; closed form in
 * SURVEY.md App. A).  g_out is dloss/dp_out with the same (ld, col0) indexing as p_out.
 *   gw_kcl (K,C,L) receives dloss/dw (overwritten, deterministic: fixed-order two-stage reduction over B)
 *   workspace: ign_shapelet_bwd_workspace_bytes() bytes.
 * Gradients w.r.t. the input are not produced here (the training loop's inputs are data: IGN/exp/experiment_classification.py:315);
 * ign_shapelet_bwd_input below is the separate pass for them.
 * LTS: dloss/dthr is a (B,KC) elementwise reduction the caller forms from g_out and p_out.
 * sign(0) convention (IGN_DIST_L1 only).  The reference differentiates |x - w| with aten::sgn, sign(0) = 0
 * (IGN/model/Shapelet.py:74).  The kernel accumulates P_j = sum_{t: x > w} A_t and returns 2 P_j - sum_t A_t, which counts an
 * element with x[b,c,t+j] == w[k,c,j] (bit-equal floats) as sign = -1.  Hence, exactly,
 *     gw_kcl[k,c,j] = reference[k,c,j] - sum_{(b,t): x[b,c,t*stride+j] == w[k,c,j]} A[b,k,c,t],   A = -(dloss/dd[b,t,k,c]) / L,
 * and the two agree wherever no sample is bit-equal to the weight it is compared with (always, for weights that an
 * optimiser has moved; a shapelet initialised as a copy of an input window is the reachable exception -- and with the RBF gate
 * a perfect-match window has d = 0, dp/dd = 0, so A = 0 there).  Forward outputs are unaffected.  Pinned by the reference
 * fixtures tests/golden/shapelet_tie_{l1,lts}.npz: tests/test_gpu_shapelet.py::test_exact_ties_differ_from_sgn0_by_exactly_
 * the_documented_term asserts this identity (and nothing else) at 1e-4.  Other distances have no kink (MSE: the factor x - w
 * is 0 at a tie; cosine / pearson: smooth).
 * IGN_TIE_EXACT (mode bit 0x20, opt-in) selects separate IGN_DIST_L1 instantiations that add A where x > w, subtract it where
 * x < w and add nothing where x == w: such an element contributes 0 to gw_kcl, as aten::sgn does, so gw_kcl equals the
 * reference on the tie fixtures too.  Same staging, same fixed-order reduction, same workspace size, bitwise repeatable;
 * slower than the default (two compares per element).  The forward ignores the bit; with MSE / cosine / pearson it is accepted
 * and changes nothing (same kernels, same bits).
 * stride > 1 (IGN/model/Shapelet.py:162: int(log2 L) once seq_len >= 3000 -- run_uea.sh's MotorImagery, EigenWorms) is
 * served by a generic-step kernel; shapelets longer than 2048 positions are split over several blocks.  Rows up to
 * T ~ 40 000 fit the forward's LDS staging (160 KB per CU); beyond that both calls return IGN_E_TOOBIG.             */
size_t ign_shapelet_bwd_workspace_bytes(int B, int C, int T, int K, int L, int stride, int mode);
/* The launch plan ign_shapelet_bwd derives from the shape, for inspection (host code only, nothing is launched; no mode: every
 * distance and gate shares the plan).  out receives IGN_SHAPELET_BWD_PLAN_FIELDS ints:
 *   JJ (shapelet positions per lane), cpk (position chunks per shapelet), kb (shapelets per block), nkt (shapelet tiles),
 *   threads (per block), tc (window positions staged per chunk), xs_len (floats of the staged x chunk), nbs (batch slices =
 *   partials to reduce), njt (blocks per long strided shapelet), LDS bytes per block.
 * Returns 0, IGN_E_ARG for bad dimensions or a null out, or the plan's refusal (IGN_E_TOOBIG: stride 1 and L > 4096, or more
 * than 64 KB of LDS) -- the code ign_shapelet_bwd returns for the same shape; out is left untouched on an error.                */
#define IGN_SHAPELET_BWD_PLAN_FIELDS 10
int ign_shapelet_bwd_plan(int B, int C, int T, int K, int L, int stride, int* out);
int ign_shapelet_bwd(const float* xn_bct, const float* w_kcl, const float* g_out, const float* p_out,
                     const float* dmin_out, int ld, int col0,
                     const int32_t* tstar, const float* zmu, const float* d_save,
                     const float* xstat_save, const float* wnorm_kc /* (K,C) sqrt(sum_j w^2): cosine / pearson, else NULL */,
                     float* gw_kcl, void* workspace,
                     int B, int C, int T, int K, int L, int stride, float eps, int mode, void* stream);

/* Backward of every group of a bank in one call (the per-group arguments of ign_shapelet_bwd as tables of G <= 8 host entries):
 * G backward launches, then ONE reduction launch over all groups that also adds add_scale_dev[0] * gw_add[g] into group g's
 * result (gw_add / add_scale_dev nullable) -- the batch-independent gradient of the diversity regulariser
 * (ign_sbm_reg_fwd_bwd), so that a parameter with two gradient sources needs no accumulate kernel.  Every group is validated
 * before the first launch; with nothing added the results are bitwise those of G ign_shapelet_bwd calls (B <= 256).
 * workspace: ign_shapelet_bwd_bank_workspace_bytes() bytes.                                                              */
size_t ign_shapelet_bwd_bank_workspace_bytes(int G, int B, int C, int T, const int* K, const int* L, const int* stride, int mode);
int ign_shapelet_bwd_bank(const float* xn_bct, int G, const float* const* w_kcl, const float* g_out, const float* p_out,
                          const float* dmin_out, int ld, const int* col0, const int32_t* const* tstar, const float* const* zmu,
                          const float* const* d_save, const float* const* xstat_save, const float* const* wnorm_kc,
                          float* const* gw_kcl, const float* const* gw_add, const float* add_scale_dev, void* workspace,
                          int B, int C, int T, const int* K, const int* L, const int* stride, float eps, int mode, void* stream);

/* Backward of ign_shapelet_fwd w.r.t. the INPUT (saliency, a learnable front-end, input-space regularisers): with dloss/dd the
 * coefficient ign_shapelet_bwd forms from g_out and the saved d_save / zmu / tstar / p_out / dmin_out,
 *     gxn_bct[b,c,s] (+)= sum_k sum_{(t,j): t*stride + j = s} dloss/dd[b,t,k,c] * dd/dx,
 *     IGN_DIST_L1: dd/dx = sign(x[b,c,s] - w[k,c,j]) / L        IGN_DIST_MSE: dd/dx = 2 (x[b,c,s] - w[k,c,j]) / L.
 * gxn_bct (B,C,T) is overwritten when accumulate == 0 and added to otherwise; samples no window covers receive 0.  Every
 * output sample is summed by one lane in a fixed order (k, then j ascending) and written once: no float atomics, no
 * workspace, bitwise reproducible.  Arguments and saved tensors as ign_shapelet_bwd; any stride >= 1, any L <= T (long
 * shapelets are walked in chunks); rows beyond the forward's LDS staging limit return the forward's IGN_E_TOOBIG.
 * IGN_DIST_COS / IGN_DIST_PEARS: IGN_E_ARG (input gradients exist for L1 and MSE only).  Nothing is launched on an error.
 * sign(0) convention (IGN_DIST_L1 only): as for gw_kcl above, an element with x[b,c,s] == w[k,c,j] (bit-equal floats) counts
 * as sign(x - w) = -1, where the reference's aten::sgn gives 0.  Hence, exactly,
 *     gxn_bct[b,c,s] = reference[b,c,s] - sum_{(k,t,j): t*stride + j = s, x[b,c,s] == w[k,c,j]} dloss/dd[b,t,k,c] / L,
 * so the tie terms of gw_kcl and gxn_bct stay negatives of each other, as every other term is.  MSE has no kink.
 * With IGN_TIE_EXACT in `mode` an element with x[b,c,s] == w[k,c,j] contributes 0 to gxn_bct as well (a separate L1
 * instantiation: compare both ways, add nothing at a tie), as aten::sgn does, so gxn_bct equals the reference.             */
int ign_shapelet_bwd_input(const float* xn_bct, const float* w_kcl, const float* g_out, const float* p_out,
                           const float* dmin_out, int ld, int col0, const int32_t* tstar, const float* zmu,
                           const float* d_save, float* gxn_bct, int accumulate,
                           int B, int C, int T, int K, int L, int stride, float eps, int mode, void* stream);
/* Every group of a bank (tables of G <= 8 host entries, as ign_shapelet_bwd_bank): G launches one after another on `stream`,
 * the first overwriting gxn_bct and the others adding to it, so the result is bitwise that of G ign_shapelet_bwd_input calls
 * with accumulate = 0, 1, 1, ...  Every group is validated before the first launch.                                         */
int ign_shapelet_bwd_input_bank(const float* xn_bct, int G, const float* const* w_kcl, const float* g_out, const float* p_out,
                                const float* dmin_out, int ld, const int* col0, const int32_t* const* tstar,
                                const float* const* zmu, const float* const* d_save, float* gxn_bct,
                                int B, int C, int T, const int* K, const int* L, const int* stride, float eps, int mode,
                                void* stream);

/* Shapelet initialisation from data: one Lloyd (k-means) step of one length group over a batch (csrc/ign_shapelet_kmeans.hip).
 * The distance of shapelet (k, c) reads channel c only, so every channel clusters its own windows
 * xn[b, c, t*stride : t*stride+L], over all (b, t < Tw), into the K centroids w_kcl[:, c, :]:
 *   d[k] = (1/L) sum_j (x[t*stride+j] - w[k,c,j])^2   (direct differences, fp32),   a = argmin_k d[k]   (lowest k on ties)
 *   sums_kcl[k,c,j] (+)= sum_{(b,t): a = k} x[b,c,t*stride+j]      counts_kc[k,c] (+)= #{(b,t): a = k}   (int32, exact)
 *   inertia_c[c]    (+)= sum_{(b,t)} min_k d[k]                    assign (B,C,Tw) int32, nullable: a of every window
 * accumulate = 0 overwrites sums / counts / inertia, 1 adds to them (a training set streamed batch by batch into one set of
 * sums).  No atomics: per-slice partials and per-row counts are summed in a fixed order, so the outputs are bitwise repeatable.
 * Domain: the forward's -- any B, C, T; 1 <= L <= T; stride, K >= 1; rows beyond its LDS staging return IGN_E_TOOBIG.  Nothing
 * is launched on an error.  workspace: ign_shapelet_kmeans_workspace_bytes() bytes (0 for arguments outside the domain), no
 * initialisation needed.
 * ign_shapelet_kmeans_update: w_kcl[k,c,:] = sums_kcl[k,c,:] / counts_kc[k,c] where counts_kc[k,c] > 0; an empty cluster keeps
 * its centroid bit for bit.  A cluster of one window becomes an exact copy of that window (the x == w case of IGN_TIE_EXACT).  */
size_t ign_shapelet_kmeans_workspace_bytes(int B, int C, int T, int K, int L, int stride);
int ign_shapelet_kmeans_step(const float* xn_bct, const float* w_kcl, int32_t* assign, float* sums_kcl, int32_t* counts_kc,
                             float* inertia_c, void* workspace, int accumulate, int B, int C, int T, int K, int L, int stride,
                             void* stream);
int ign_shapelet_kmeans_update(float* w_kcl, const float* sums_kcl, const int32_t* counts_kc, int K, int C, int L, void* stream);

/* Backward of ign_instnorm_fwd: gxn_bct (B,C,T) = dloss/dxn -> gx_btc (B,T,C) = dloss/dx in the loader's layout.  With
 * y = (x - mu) / (sigma + eps), sigma the unbiased std over T:
 *     gx_j = [ g_j - mean_T(g) - y_j * (sum_i g_i y_i) / (T - 1) * (sigma + eps) / sigma ] / (sigma + eps).
 * mu and sigma are recomputed from x_btc with the forward's two-pass scheme (the forward saves no statistics).  A constant
 * row (sigma == 0), where the reference's autograd yields NaN, receives gx = 0 for every sample of that row.  T >= 2; the
 * LDS tile limit of ign_instnorm_fwd applies (IGN_E_TOOBIG beyond it).                                                      */
int ign_instnorm_bwd(const float* x_btc, const float* gxn_bct, float* gx_btc, int B, int T, int C, float eps, void* stream);

/* Variable-length series (csrc/ign_shapelet_mask.hip; run.py --mask_padding).  A ragged batch arrives zero-padded at the end to
 * (B,T,C) with len_b (B) int32 on the DEVICE: n_b = len_b[b] samples of row b are data (clamped to 0..T by the kernels).  The two
 * passes below make the shapelet expert compute, for every sample, what it computes for that sample alone truncated to n_b.
 *
 * ign_instnorm_fwd_len: the length-aware twin of ign_instnorm_fwd.  Mean and unbiased std over x[b, :n_b, c]; (x - mean)/(std + eps)
 * for t < n_b and exactly 0 for t >= n_b; n_b < 2: the whole row is 0.  No raw transpose and no amax (callers that need them call
 * ign_instnorm_fwd on the padded batch).  Tile limit of ign_instnorm_fwd (IGN_E_TOOBIG beyond it).                               */
int ign_instnorm_fwd_len(const float* x_btc, const int32_t* len_b, float* xn_bct, int B, int T, int C, float eps, void* stream);

/* ign_shapelet_regate: runs AFTER ign_shapelet_fwd of the same group on xn_bct of ign_instnorm_fwd_len, on that call's outputs
 * (same ld / col0 / K / L / stride / eps / mode; d_save is REQUIRED).  Sample b has Tw_b = (n_b - L)/stride + 1 valid windows
 * (0 if n_b < L).  Per (b,c,k) row the pass recomputes p_out, dmin_out, tstar and zmu from d_save[.., t < Tw_b] with the forward's
 * formulas (RBF: Z = sum exp(p_t), mu = sum exp(p_t) p_t / Z, p_out = max p; LTS: Z = sum exp(dmin - d_t), mu = sum e_t d_t / Z,
 * p_out = sigmoid(thr - dmin); first index on ties) and overwrites d_save[.., t >= Tw_b] with 1e18f, the forward's value for
 * slots past the end of a row, for which the coefficient of ign_shapelet_bwd / ign_shapelet_bwd_input is exactly 0 -- those
 * kernels then yield the sum over samples of the gradients of the truncated problems, unchanged.
 * Tw_b = 0: p_out = 0, dmin_out = 1e18f, tstar = -1, zmu = {1, 0}; the feature receives and sends no gradient.
 * One wave per row, fixed-order reductions, no atomics: bitwise repeatable.  Any Tw.  The dist bits and IGN_TIE_EXACT of `mode` are
 * validated and otherwise unused (the pass reads distances, whatever produced them).  Nothing is launched on an error.
 * ign_shapelet_regate_bank: every group of a bank (tables of G <= 8 host entries, as ign_shapelet_fwd_bank), each validated before
 * the first launch.                                                                                                              */
int ign_shapelet_regate(float* d_save, const int32_t* len_b, const float* thr_kc, float* p_out, float* dmin_out, int ld, int col0,
                        int32_t* tstar, float* zmu, int B, int C, int T, int K, int L, int stride, float eps, int mode,
                        void* stream);
int ign_shapelet_regate_bank(int G, float* const* d_save, const int32_t* len_b, const float* const* thr_kc, float* p_out,
                             float* dmin_out, int ld, const int* col0, int32_t* const* tstar, float* const* zmu, int B, int C, int T,
                             const int* K, const int* L, const int* stride, float eps, int mode, void* stream);

/* Shapelet projection (csrc/ign_shapelet_project.hip; run.py --shapelet_project): every shapelet of one length group is snapped
 * to the nearest window of a training set that is streamed batch by batch.  Runs AFTER the shapelet forward of a batch, on its
 * outputs: dmin and tstar are (B, ld), column col0 + k*C + c -- the minimum distance per sample and feature and the index of its
 * window (the layout of ign_shapelet_fwd's dmin_out, and of the (B,K,C) tstar tables of a bank concatenated along the features).
 * Per (k, c):
 *   candidates  the samples b with 0 <= tstar < Tw = (T - L)/stride + 1 (ign_shapelet_regate gives a sample shorter than the
 *               shapelet tstar = -1: it never takes part; an index past Tw is never used as an address either);
 *   j           the candidate with the smallest dmin, the lowest b on ties; strict <, so a NaN (or +inf) never wins;
 *   the running best is replaced if accumulate == 0, or if dmin[j] < best_d_kc[k,c] strictly (an earlier batch wins a tie, i.e.
 *   the lowest global sample index).  On replacement: best_d_kc[k,c] = dmin[j], best_src_kc2[k,c] = (sample0 + j, tstar[j]),
 *   cand_kcl[k,c,:] = xn_bct[j, c, tstar[j]*stride : +L], copied bit for bit.
 *   accumulate == 0 and no candidate: best_d = +inf, src = (-1, -1), the cand row is left untouched.
 * No atomics, no workspace, a fixed order: bitwise repeatable.  Any B, C, K; 1 <= L <= T; stride >= 1; sample0 >= 0.  Nothing is
 * launched on an error.
 * ign_shapelet_project_step_bank: every group of a bank (tables of G <= 8 host entries, as ign_shapelet_fwd_bank; dmin / tstar /
 * ld shared), each validated before the first launch.                                                                            */
int ign_shapelet_project_step(const float* xn_bct, const float* dmin, const int32_t* tstar, int ld, int col0, int sample0,
                              float* best_d_kc, int32_t* best_src_kc2, float* cand_kcl, int accumulate, int B, int C, int T, int K,
                              int L, int stride, void* stream);
int ign_shapelet_project_step_bank(const float* xn_bct, const float* dmin, const int32_t* tstar, int ld, int G, const int* col0,
                                   int sample0, float* const* best_d_kc, int32_t* const* best_src_kc2, float* const* cand_kcl,
                                   int accumulate, int B, int C, int T, const int* K, const int* L, const int* stride, void* stream);

/* Augmentation (csrc/ign_augment.hip; run.py --augment): the training batch x (B,T,C) -> out (B,T,C), one launch, out of place
 * (x == out or overlapping buffers: IGN_E_ARG), no workspace, no atomics, bitwise repeatable.  len_b (B) int32 on the DEVICE
 * or NULL (every sample has T steps); n = len_b[b] clamped to 0..T.
 *   out[b,t,c] = keepC[b,c] * keepT[b,t] * (a[b,c] * x[b, (t - s_b) mod n, c] + sigma * n[b,t,c])   for t <  n
 *   out[b,t,c] = x[b,t,c]                                                                          for t >= n (padding: no noise)
 * The rule (csrc/ign_augment.h, the one definition the kernel, host code and the numpy restatement utils/augment.py share): every
 * draw is Philox4x32-10 (Random123 constants) under key = seed (low word first); the last counter word tags the kind of draw and
 * every transform reads its own word, so a draw depends on (seed, b), (seed, b, c) or (seed, b, t, c) only -- not on the launch
 * geometry, on B, or on which transforms are on.
 *   per sample, counter (b, 0, 0, 0) -> x0, x1, x2:
 *     shift      S = min(floor(shift * n), n - 1), s_b = x0 mod (2 S + 1) - S (modulo bias below (2 S + 1) / 2^32 < 2^-20 up to
 *                T = 2047);
 *     time mask  M = min(floor(time_mask * n), n), m = x1 mod (M + 1), start = x2 mod (n - m + 1), keepT = 0 in [start, start + m);
 *   per channel, counter (b, c, 0, 1) -> x0, x1:
 *     gain       a = 1 + scale * (2 u - 1), u = (x0 >> 8) * 2^-24.  The SBM's instance norm cancels a per-channel gain; the term is
 *                for the FCN / ResNet / EEG-CNN / Transformer side;
 *     electrode  keepC <=> (x1 & 0xffff) >= chan_thr, chan_thr = round(p * 65536) as for attention dropout; nothing is rescaled;
 *   noise, counter (e >> 2, 0, b, 2) with e = t * C + c: four consecutive flat indices share a call; Box-Muller on
 *     u1 = ((w0 >> 8) + 1) * 2^-24, u2 = (w1 >> 8) * 2^-24 with the precise logf / sqrtf / sincosf: (x0, x1) -> elements 0, 1 of the
 *     quad, (x2, x3) -> elements 2, 3.  sigma == 0 skips the noise path; the other terms are separate fp32 roundings (no fma), so a
 *     float32 restatement is then bitwise equal.
 * n = 0 copies the row; n = 1 forces S = M = 0.  shift, scale, time_mask in [0, 1), chan_thr < 65536, sigma finite and >= 0, T >= 1,
 * else IGN_E_ARG; C > 8192 or T * C >= 2^31 - 65536: IGN_E_TOOBIG.  Nothing is launched on an error.                              */
int ign_augment_btc(const float* x_btc, float* out_btc, const int32_t* len_b, int B, int T, int C, unsigned long long seed,
                    float shift, float scale, float sigma, unsigned chan_thr, float time_mask, void* stream);

/* Mixup / CutMix of the training batch (csrc/ign_mix.hip; run.py --mix): x (B,T,C) -> out (B,T,C), one launch, out of place
 * (x == out or overlapping buffers: IGN_E_ARG), no workspace, no atomics, bitwise repeatable.  Sample b is mixed with its partner
 * p = (b + roll) mod B.  len_b (B) int32 on the DEVICE or NULL (every sample has T steps), n = len_b[b] clamped to 0..T; lam_b (B)
 * float32 and span_b2 (B,2) int32 = (start_b, m_b) (NULL: every span is empty) on the DEVICE:
 *   out[b,t,c] = x[p,t,c]                                       for start_b <= t < start_b + m_b, t < n   (CutMix span)
 *   out[b,t,c] = lam_b * x[b,t,c] + (1 - lam_b) * x[p,t,c]      for the other t < n                       (mixup)
 *   out[b,t,c] = x[b,t,c]                                       for t >= n                                (padding copied through)
 * The partner is read at the same t whatever its own length (its padding is zero by the loader's contract).  1 - lam_b, the two
 * products and the sum are separate fp32 roundings (no fma): a float32 restatement (utils/mix.py:mix_reference) is bitwise equal.
 * lam_b == 1 copies x[b,t,c] (not 1*x + 0*x_p: the partner may hold inf / NaN).  The draws (roll, lam, span) are the host's:
 * utils/mix.py:mix_draws.  roll outside [0, B), T < 1, a null pointer: IGN_E_ARG; T * C >= 2^31 - 65536: IGN_E_TOOBIG.  Nothing is
 * launched on an error.                                                                                                          */
int ign_mix_btc(const float* x_btc, float* out_btc, const int32_t* len_b, const float* lam_b, const int32_t* span_b2, int roll,
                int B, int T, int C, void* stream);

/* Time, magnitude and window warping of the training batch (csrc/ign_warp.hip; run.py --warp): x (B,T,C) -> out (B,T,C), one launch,
 * out of place (x == out or overlapping buffers: IGN_E_ARG), no workspace, no atomics, every element of out written once, bitwise
 * repeatable.  len_b (B) int32 on the DEVICE or NULL (every sample has T steps); n = len_b[b] clamped to 0..T.
 *   out[b,t,c] = g_b(t) * y,  y = (w == 0) ? x[b,i0,c] : x[b,i0,c] + w * (x[b,i0+1,c] - x[b,i0,c])       for t <  n
 *                i0 = min(floor(phi_b(t)), n - 2),  w = phi_b(t) - i0   (mwarp == 0: no multiplication)
 *   out[b,t,c] = x[b,t,c]                                                                              for t >= n (padding)
 * The rule (csrc/ign_warp.h, the one definition the kernel, ign_warp_map and the numpy restatement utils/warp.py share; every product,
 * sum and quotient is one fp32 rounding, no fma, so the restatement is bitwise equal).  K = knots, seg = K + 1, control points
 * i = 0 .. K + 1 at equal spacing over [0, n - 1].  Draws: Philox4x32-10 under key = seed (low word first), last counter word 3:
 *   counter (b, 0, 0, 3) -> x0, x1, x2: warped iff (x0 >> 8) * 2^-24 < prob (else the sample is copied bit for bit); x1 the window
 *     start; x2 & 1 the window factor (0 -> 0.5, 1 -> 2);
 *   speed knot i = word i & 3 of counter (b, 1 + (i >> 2), 0, 3), gain knot i likewise of (b, 4 + (i >> 2), 0, 3);
 *     u = (word >> 8) * 2^-24, v_i = 1 + twarp * (2 u - 1), m_i = 1 + mwarp * (2 u - 1): positive for rates in [0, 1).
 *   window map (wwarp = R > 0 and n >= 3): Lw = min(max(floor(R * n), 2), n - 1), a = x1 mod (n - Lw + 1), c = 0.5 or 2,
 *     Iw(t) = t + (c - 1) * clamp(t - a, 0, Lw) (exact), pos(t) = (Iw(t) * (n - 1)) / Iw(n - 1); else pos(t) = t;
 *   smooth map (twarp > 0): C_0 = 0, C_{i+1} = C_i + 0.5 * (v_i + v_{i+1}) in order; u = (p * seg) / (n - 1), i = min(floor(u), K),
 *     f = u - i, I = C_i + (f * v_i + (f * f) * (0.5 * (v_{i+1} - v_i))), smooth(p) = (I * (n - 1)) / C_seg; else smooth(p) = p;
 *   phi(t) = min(max(smooth(pos(t)), 0), n - 1) for t < n - 1 (the clamp whichever transforms are on) and phi(n - 1) = n - 1;
 *   gain (mwarp > 0): i, f as above from the integer output step t, g(t) = m_i + f * (m_{i+1} - m_i), one curve for all channels.
 * The map and the gain depend on (seed, b, n) only: not on c, B, the launch geometry, or which of the other transforms are on.
 * n < 2 copies the row; a sample not warped by prob and a call with all three rates 0 are exact copies (still one launch).
 * twarp, mwarp, wwarp outside [0, 1), knots outside 1..IGN_WARP_MAX_KNOTS, prob outside (0, 1], T < 1, a null x / out: IGN_E_ARG;
 * T > IGN_WARP_MAX_T (t * seg and Iw stay exact in fp32) or T * C >= 2^31 - 65536: IGN_E_TOOBIG.  Nothing is launched on an error.
 * ign_warp_map: HOST only, nothing is launched and no pointer is a device pointer -- the header's rule for sample b of length n,
 * for inspection and tests: phi_n (n) and, unless NULL, gain_n (n) host arrays; an unwarped sample gives phi(t) = t, gain 1.
 * Refusals as above (n < 0 or b < 0: IGN_E_ARG; n > IGN_WARP_MAX_T: IGN_E_TOOBIG).                                               */
#define IGN_WARP_MAX_KNOTS 8
#define IGN_WARP_MAX_T     (1 << 20)
int ign_warp_btc(const float* x_btc, float* out_btc, const int32_t* len_b, int B, int T, int C, unsigned long long seed,
                 float twarp, float mwarp, float wwarp, int knots, float prob, void* stream);
int ign_warp_map(unsigned long long seed, int b, int n, float twarp, float mwarp, float wwarp, int knots, float prob,
                 float* phi_n, float* gain_n);

/* Evidence maps (csrc/ign_evidence.hip, rule: csrc/ign_evidence.h; utils/evidence.py, run.py --evidence): the logit of class
 * n_b = target[b] laid out over the input, from what the forward already produced.  No workspace, no atomics, every output element
 * written exactly once (zeros included), bitwise repeatable.  target (B) int32 and scale (B) float32 (NULL: no scaling) on the DEVICE.
 *
 * ign_shapelet_evidence_bank: the linear-head shapelet expert.  p, t (B,ld) = P and Tstar of the bank forward, W (N,ld) the head's
 *   weight, feature f = col0[g] + k*C + c, window [t*stride_g, t*stride_g + L_g) on electrode c.  out (B,T,C):
 *     out[b,s,c] = scale[b] * sum over g, then k ascending, of fl(fl(W[n_b,f] * p[b,f]) * invL[g]) where the window covers s,
 *   summed from 0.0f, one fp32 rounding per operation (no fma); invL[g] = 1.0f / L[g] is the HOST's.  A feature with t outside
 *   [0, Tw_g), Tw_g = (T - L_g) / stride_g + 1, (t = -1: no window under --mask_padding) and a sample whose target lies outside
 *   [0, N) contribute nothing.  Host tables K, L, stride, col0, invL of G groups.  G outside 1..8, col0 / ld that do not tile the
 *   row as col0[g+1] = col0[g] + K[g]*C with ld the total, L[g] outside 1..T, stride < 1, a null pointer: IGN_E_ARG;
 *   T*C >= 2^31 - 65536: IGN_E_TOOBIG.  Nothing is launched on an error.
 * ign_bn_relu_cam_fwd: the FCN expert, on block 3's time axis.  y_last (B,Tl,Cl) the raw output of the last convolution, a, b (Cl)
 *   the BatchNorm affine, head_w (N,Cl):  cam[b,t] = scale[b] * (1/Tl) * sum_c head_w[n_b,c] * relu(fma(a_c, y, b_c)), so that
 *   sum_t cam[b,t] + bias[n_b] is the expert's logit.  One read of y_last; the sum over c runs in a fixed order inside a wave.
 *   Cl % 4 == 0, Cl <= 1024 as the other ign_bn_* entry points; a target outside [0, N) gives a zero row.
 * ign_cam_spread: cam (B,Tl) -> out (B,T), T = Tl + R - 1, each cam[b,t] spread evenly over the R input samples it saw:
 *     out[b,s] = fl(invR * sum_{t = max(0, s-R+1)}^{min(s, Tl-1)} cam[b,t]),  t ascending from 0.0f, invR = 1.0f / R the HOST's.
 *   R < 1 or Tl < 1: IGN_E_ARG.                                                                                                 */
int ign_shapelet_evidence_bank(const float* p, const int32_t* t, const float* W, const int32_t* target, const float* scale, int ld,
                               int G, const int* K, const int* L, const int* stride, const int* col0, const float* invL, float* out,
                               int B, int T, int C, int N, void* stream);
int ign_bn_relu_cam_fwd(const float* y_last, const float* a, const float* b, const float* head_w, const int32_t* target,
                        const float* scale, float* cam, int B, int Tl, int Cl, int N, void* stream);
int ign_cam_spread(const float* cam, float* out, int B, int Tl, int R, float invR, void* stream);

/* Faithfulness curves (csrc/ign_faithfulness.hip; rule: utils/faithfulness.py rank_rule / perturb_rule; run.py --faithfulness): rank
 * the cells of every sample by a score map and replace the top k by a baseline -- the deletion / insertion test of an explanation.
 * score (B,T,Cs) float32, Cs == C (a score per cell) or Cs == 1 (a score per time step, applied to every electrode); flat index
 * i = t*Cs + c; sample b has n_b = clamp(len_b[b], 0, T) * Cs valid scores (len_b NULL: T * Cs).  All arrays on the DEVICE.
 *   key(v): u = bits(v); sign set: ~u, else u | 0x80000000 -- a total order on bit patterns (-0 below +0, positive NaNs above +inf,
 *           nothing special-cased).  Element i precedes i' iff key_i > key_i', or the keys are equal and i < i'.
 *   selected(b, i, j): i < n_b and (key_i > thr_key[b,j] or (key_i == thr_key[b,j] and i <= thr_idx[b,j])).
 * ign_rank_threshold: k (B,nk) int32, clamped to [0, n_b] on the device -> thr_key, thr_idx (B,nk) int32 (thr_key holds the uint32
 *   key's bits): key and flat index of the k-th element in the order above, so that exactly min(k, n_b) elements are selected and
 *   the sets of ascending k are nested; k = 0 gives (0xffffffff, -1).  One workgroup per sample, an 8-bit radix select over the
 *   key then over the index bits among tied keys, integer LDS counters only: no workspace, no float atomics, bitwise repeatable, a
 *   sample's result independent of the batch around it.  nk outside 1..IGN_RANK_MAX_K, a null pointer (len_b may be), a
 *   non-positive dimension: IGN_E_ARG; T*Cs >= 2^31 - 65536: IGN_E_TOOBIG.
 * ign_perturb_btc: x (B,T,C) -> out (B,T,C), out of place (overlapping buffers: IGN_E_ARG): for t < len_b, out[b,t,c] = fill[b,c]
 *   (fill (B,C), NULL: 0.0f) where selected(b, t*Cs + (Cs == C ? c : 0), j) != (insert != 0), elsewhere -- and for t >= len_b -- the
 *   bits of x[b,t,c].  j is a HOST integer: the launch can be captured.  One read of x and score, one write of out.  Cs not in
 *   {1, C}, nk outside 1..IGN_RANK_MAX_K, j outside [0, nk), a null x / score / thr_key / thr_idx / out, a non-positive dimension:
 *   IGN_E_ARG; T*C >= 2^31 - 65536: IGN_E_TOOBIG.
 * Nothing is launched on an error.  Timing labels rank_threshold, perturb.                                                        */
#define IGN_RANK_MAX_K 32
int ign_rank_threshold(const float* score_bts, const int32_t* k_bj, const int32_t* len_b, int32_t* thr_key_bj, int32_t* thr_idx_bj,
                       int B, int T, int Cs, int nk, void* stream);
int ign_perturb_btc(const float* x_btc, const float* score_bts, const int32_t* thr_key_bj, const int32_t* thr_idx_bj, int j, int nk,
                    const float* fill_bc, const int32_t* len_b, float* out_btc, int insert, int B, int T, int C, int Cs, void* stream);

/* Occlusion maps (csrc/ign_occlusion.hip; rule: utils/occlusion.py occlude_rule / spread_rule; run.py --occlusion): hide a window of
 * time on a group of electrodes, run the model on the copies, lay the falls of the class score back over the hidden cells -- an
 * attribution that needs a forward pass only, for every model.  The time grid is the HOST's and the same for every sample: windows of
 * W steps every S steps, 1 <= S <= W <= T, nt = ceil((T - W) / S) + 1 of them; gid (C) int32 in [0, G) names each electrode's group;
 * patch p = i * G + g hides window i on group g; sample b has n_b = clamp(len_b[b], 0, T) steps (len_b NULL: T).  Arrays on the DEVICE.
 *   hidden(b, p, t, c): gid[c] == g(p) and i(p) * S <= t < min(i(p) * S + W, n_b).
 * ign_occlude_btc: x (B,T,C) -> out (B*Pc,T,C), row b*Pc + q the copy of sample b under patch p0 + q: the bits of fill[b,c] (fill
 *   (B,C), NULL: 0.0f) where hidden, elsewhere the bits of x[b,t,c].  One read of x, Pc writes; out of place (overlapping buffers:
 *   IGN_E_ARG); every scalar is a HOST integer: the launch can be captured.  p0 < 0, Pc < 1, p0 + Pc > nt*G: IGN_E_ARG;
 *   B*Pc*T*C >= 2^31 - 65536: IGN_E_TOOBIG.  A gid outside [0, G) matches no patch.
 * ign_occlusion_spread: drop (B, nt*G) -> out (B,T,C): for t < n_b
 *     out[b,t,c] = fl(fl(sum_i drop[b, i*G + gid[c]]) * inv_k[cnt]),  i = max(0, ceil((t-W+1)/S)) .. min(nt-1, t/S) ascending, each
 *   addition one float add starting from the first term, cnt their number, inv_k (ceil(W/S) + 1) the HOST's table inv_k[k] = 1.0f / k
 *   (inv_k[0] unused); for t >= n_b, +0.0f.  A gather, a lane per cell: no atomics, no workspace, bitwise repeatable, a sample's map
 *   independent of the batch around it.  ceil(W/S) > IGN_OCC_MAX_COVER: IGN_E_ARG.  gid is the caller's to check; a value outside
 *   [0, G) is clamped before it indexes.
 * Both: a null pointer (fill_bc and len_b may be), a non-positive dimension, G < 1, S < 1, S > W, W > T, nt not the grid's value:
 *   IGN_E_ARG; T*C >= 2^31 - 65536: IGN_E_TOOBIG.  Nothing is launched on an error.  Timing labels occlude, occlusion_spread.   */
#define IGN_OCC_MAX_COVER 64
int ign_occlude_btc(const float* x_btc, const float* fill_bc, const int32_t* len_b, const int32_t* gid_c, float* out, int p0, int Pc,
                    int G, int W, int S, int nt, int B, int T, int C, void* stream);
int ign_occlusion_spread(const float* drop_bp, const int32_t* gid_c, const int32_t* len_b, const float* inv_k, float* out_btc, int G,
                         int W, int S, int nt, int B, int T, int C, void* stream);

/* Fused attention core softmax(scale * Q K^T) V, exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32), scores never
 * materialised.  Replaces IGN/layers/SelfAttention_Family.py:56-75 (FullAttention: no mask; dropout 0 here -- dropout p > 0
 * is ign_attn_*_dropout below) and the attention inside nn.TransformerEncoderLayer of IGN/model/eegcnn.py:219-228.
 *   q (B,L,H,E), k/v (B,S,H,E): unit stride over E, stride E over H; *_sb / *_sl are the ELEMENT strides of the
 *   batch and sequence axes (multiples of 4), so packed qkv projections can be passed without a copy.
 *   out (B,L,H,E) contiguous; lse (B,H,L) log-sum-exp of the scaled scores (saved for the backward).
 *   E in {16, 32, 64, 128}; all pointers 16-byte aligned.                                                          */
int ign_attn_fwd(const float* q, const float* k, const float* v, float* out, float* lse,
                 int B, int L, int S, int H, int E,
                 long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                 float scale, void* stream);
/* Backward: gq (B,L,H,E), gk/gv (B,S,H,E) contiguous outputs (overwritten); gout (B,L,H,E) contiguous;
 * delta_ws: B*H*L floats of workspace.  dQ recomputes the scores instead of using float atomics: deterministic.  */
/* The forward on the bf16 matrix cores at fp32 accuracy (split-bf16 products as in ign_clconv_*_x6; K / V tiles are split while
 * they are staged, Q and P in registers).  Same arguments, outputs and saved statistics as ign_attn_fwd, so ign_attn_bwd follows
 * either.                                                                                                                   */
int ign_attn_fwd_x6(const float* q, const float* k, const float* v, float* out, float* lse, int B, int L, int S, int H, int E,
                    long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                    float scale, void* stream);
int ign_attn_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout,
                 float* gq, float* gk, float* gv, float* delta_ws,
                 int B, int L, int S, int H, int E,
                 long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                 float scale, void* stream);
/* The backward in split-bf16 form: delta, then dV, dK (key blocks, each recomputing S) and dQ (query blocks) as three kernels;
 * same arguments and results as ign_attn_bwd (gradients bitwise reproducible, no atomics).  E <= 64 runs without register
 * spills; E = 128 is accepted but slower than ign_attn_bwd.                                                                */
int ign_attn_bwd_x6(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout,
                 float* gq, float* gk, float* gv, float* delta_ws,
                 int B, int L, int S, int H, int E,
                 long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                 float scale, void* stream);
/* Both with ONE product per MFMA step on operands rounded to bf16 (Q, K, V, P, dO, dS; fp32 accumulation and softmax): what the
 * reference's default bf16-autocast mode computes for the two attention matmuls.  Same arguments and outputs.             */
int ign_attn_fwd_bf16(const float* q, const float* k, const float* v, float* out, float* lse, int B, int L, int S, int H, int E,
                    long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                    float scale, void* stream);
int ign_attn_bwd_bf16(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout,
                 float* gq, float* gk, float* gv, float* delta_ws,
                 int B, int L, int S, int H, int E,
                 long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                 float scale, void* stream);
/* ign_attn_bwd_x6 (bf16 = 0) / ign_attn_bwd_bf16 (bf16 = 1) writing gq / gk / gv with the caller's batch and sequence strides
 * (elements, multiples of 4; head stride E): the three gradients can land in ONE packed (B, L, 3, H, E) buffer -- the gradient of
 * a fused q/k/v projection -- without a gather pass.                                                                      */
int ign_attn_bwd_x6_strided(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout,
                 float* gq, float* gk, float* gv, float* delta_ws,
                 int B, int L, int S, int H, int E,
                 long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                 float scale, void* stream,
                            long long g_sb, long long g_sl, int bf16);

/* The attention core on two fp16 planes / three products per element pair (the "h3" arithmetic described at ign_clconv_fwd_h3;
 * E <= 64): Q, K, V, dO are scaled by powers of two from the device-side bounds bq / bk / bv / bgo (upper bounds of their maxima),
 * scores are un-scaled inside the exp2, probabilities (<= 1) are split after a multiplication by 2^14, the score gradient by its
 * hard bound 2 E max|dO| max|V|.  Same results as ign_attn_fwd_x6 / ign_attn_bwd_x6 at the fp32 rounding level.  g_sb = g_sl = 0:
 * contiguous gradients, else the strided outputs of ign_attn_bwd_x6_strided.                                                  */
int ign_attn_fwd_h3(const float* q, const float* k, const float* v, float* out, float* lse,
                    int B, int L, int S, int H, int E,
                    long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                    float scale, void* stream, const float* bq, const float* bk, const float* bv);
int ign_attn_bwd_h3(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout,
                    float* gq, float* gk, float* gv, float* delta_ws,
                    int B, int L, int S, int H, int E,
                    long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                    float scale, void* stream, long long g_sb, long long g_sl,
                    const float* bq, const float* bk, const float* bv, const float* bgo,
                    float* g_amax /* nullable: max over |gq|, |gk|, |gv| as an atomic maximum (caller zeroes) -- the bound of
                                     the packed gradient for the projection's backward GEMMs */);

/* Attention dropout: A = dropout(softmax(scale Q K^T)) as in IGN/layers/SelfAttention_Family.py:56-75 and the self_attn of
 * nn.TransformerEncoderLayer (IGN/model/eegcnn.py:219-228), inside the fused kernels (the DROPOUT instantiations of all six).
 * Keep mask (csrc/ign_dropout.h, the one definition every kernel and ign_attn_dropout_mask evaluate): the decision for score
 * element (b, h, i, j) is a pure function of (seed, b*H + h, i, j, p) -- independent of tiles, launch geometry, kernel and
 * arithmetic.  Philox4x32-10 (Random123 constants), key = seed (low word first), counter = (i>>2, j>>2, b*H + h, c); the 4x4
 * block (i>>2, j>>2) takes its 16 halfwords from the calls c = 0, 1 and element (i, j) reads halfword n = (i&3)*4 + (j&3):
 * call n>>3, word (n&7)>>1, low half for even n.  keep <=> halfword >= thr, thr = round(p * 65536) (p_eff = thr / 65536); kept
 * values are scaled by s = 65536 / (65536 - thr) (fp32).  p in [0, 1) with thr < 65536, else IGN_E_ARG.
 *   forward:  O = (Z o P) V s, P = softmax(scale Q K^T); lse stays the statistic of the UN-dropped softmax; s is folded into the
 *             final normalisation, so P <= 1 still holds for the h3 split;
 *   backward: dV = (Z o P)^T dO s; dP = dO V^T; dS = P o (Z o dP s - D), D = rowsum(dO o O) as without dropout.
 *   h3: the score-gradient bound grows to 2 E max|dO| max|V| s; a bound of the output is max|v| s (not max|v|).
 * Arguments: those of ign_attn_fwd / ign_attn_bwd_h3, plus `math` (IGN_ATTN_MATH_*; bq / bk / bv / bgo / g_amax are read for H3
 * only and may be null otherwise; BF16 and H3 need E <= 64), g_sb / g_sl (0, 0: contiguous gradients; else the strided
 * gradients of ign_attn_bwd_x6_strided -- not with F32), and p, seed.  The backward regenerates the mask from (p, seed): pass
 * the forward's values.                                                                                                       */
#define IGN_ATTN_MATH_F32  0   /* fp32 MFMA (ign_attn_fwd / ign_attn_bwd)                                          */
#define IGN_ATTN_MATH_X6   1   /* three bf16 planes, six products (ign_attn_fwd_x6 / ign_attn_bwd_x6)            */
#define IGN_ATTN_MATH_BF16 2   /* one bf16 product: the autocast arithmetic (ign_attn_fwd_bf16 / _bwd_bf16)       */
#define IGN_ATTN_MATH_H3   3   /* two fp16 planes, three products (ign_attn_fwd_h3 / ign_attn_bwd_h3)             */
int ign_attn_fwd_dropout(const float* q, const float* k, const float* v, float* out, float* lse,
                         int B, int L, int S, int H, int E,
                         long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                         float scale, void* stream, int math, const float* bq, const float* bk, const float* bv,
                         float p, unsigned long long seed);
int ign_attn_bwd_dropout(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout,
                         float* gq, float* gk, float* gv, float* delta_ws,
                         int B, int L, int S, int H, int E,
                         long long q_sb, long long q_sl, long long k_sb, long long k_sl, long long v_sb, long long v_sl,
                         float scale, void* stream, int math, long long g_sb, long long g_sl,
                         const float* bq, const float* bk, const float* bv, const float* bgo, float* g_amax,
                         float p, unsigned long long seed);
/* The (B, H, L, S) keep mask of one call as bytes (1 = kept), through the same device function as the kernels: test and
 * debugging infrastructure.                                                                                                   */
int ign_attn_dropout_mask(unsigned char* keep, int B, int H, int L, int S, float p, unsigned long long seed, void* stream);

/* Attention map: A = dropout(softmax(scale Q K^T)), the (B, H, L, S) `attn` of IGN/layers/SelfAttention_Family.py:56-75 with
 * output_attention=True, recomputed from q, k and the lse a forward call saved:
 *   attn[((b H + h) L + i) S + j] = exp(scale s_ij - lse[b, h, i]) * keep(b, h, i, j) * s      (fp32, contiguous, 64-bit offsets)
 * s_ij is the score in the arithmetic `math` (IGN_ATTN_MATH_*, as ign_attn_fwd_dropout; BF16 and H3 need E <= 64; bq / bk are
 * read for H3 only, and must be the forward's bounds: the h3 operand scales come from them).  Pass the forward's q, k, scale,
 * math, p and seed: keep and s are the mask and scale of ign_dropout.h above, so the map is the one the forward applied
 * (p = 0: no mask, s = 1).  With the fp32-accurate arithmetics (F32, X6, H3) a row sums to s * (kept mass) at fp32 rounding;
 * BF16 rounds q and k to bf16 exactly as the forward does.  q, k: the layouts and strides of ign_attn_fwd (16-byte aligned).
 * Errors before any launch: a null pointer, bad dimensions or strides, p outside [0, 1), an unknown `math`, H3 without bounds
 * -> IGN_E_ARG; E not in {16, 32, 64, 128}, or E > 64 with BF16 / H3 -> IGN_E_UNSUP.  No gradient flows through the map.     */
int ign_attn_probs(const float* q, const float* k, const float* lse, float* attn,
                   int B, int L, int S, int H, int E,
                   long long q_sb, long long q_sl, long long k_sb, long long k_sl,
                   float scale, void* stream, int math, const float* bq, const float* bk,
                   float p, unsigned long long seed);

/* Skinny expert-head GEMM  out[b,n] = sum_f X[b,f] W[n,f] (+ bias[n]),  N <= IGN_HEAD_NMAX classes, F % 4 == 0, row pitch ldx.
 * Replaces nn.Linear at IGN/model/Shapelet.py:171,200 (SBM head), IGN/model/Transformer.py:72,109,
 * IGN/model/FullyConvNet.py:50,58.  Backward: gX (B,ldx) and/or gW (N,F), gbias (N) (any may be NULL); sums over the
 * batch run in ascending order, gX sums the classes in ascending order (deterministic).  One launch per call at any N
 * (N > 16: 16-class chunks as an extra grid dimension).  gW stages g in LDS: B*N <= 10240 for N <= 16, B <= 640 above
 * (IGN_E_TOOBIG otherwise, whichever outputs are asked for).  gbias is written by the weight-gradient blocks: with gW NULL it
 * is not touched.                                                                                                          */
int ign_head_fwd(const float* X, const float* W, const float* bias, float* out, int B, int F, int N, long long ldx,
                 void* stream);
int ign_head_bwd(const float* g_out, const float* X, const float* W, float* gX, float* gW, float* gbias,
                 int B, int F, int N, long long ldx, void* stream);
/* The same with gW += add_scale_dev[0] * gW_add (both nullable; add_scale_dev NULL = 1): a batch-independent gradient of W --
 * the L1 regulariser mean|W| of IGN/model/Shapelet.py:219 -- lands in the same store instead of an accumulate kernel.   */
int ign_head_bwd_acc(const float* g_out, const float* X, const float* W, float* gX, float* gW, float* gbias,
                     const float* gW_add, const float* add_scale_dev, int B, int F, int N, long long ldx, void* stream);

/* Gini-index gate of the two experts, forward and backward.  Replaces IGN/model/InterpGN.py:44-52:
 * eta = (N*sum softmax(sbm)^2 - 1)/(N-1); if use_gating_value and eta > gating_value: eta = 1 (test time);
 * out = eta*sbm + (1-eta)*dnn.   out (B,N), eta (B).  Backward: geta (B) may be NULL.                              */
int ign_gate_fwd(const float* sbm, const float* dnn, float* out, float* eta, int B, int N, float gating_value,
                 int use_gating_value, void* stream);
int ign_gate_bwd(const float* sbm, const float* dnn, const float* gout, const float* geta, float* gsbm, float* gdnn,
                 int B, int N, float gating_value, int use_gating_value, void* stream);

/* IGN's training-loss tail in one launch: gini gate + CE(mixture, y) + beta*CE(sbm, y) (batch means) and the gradients of
 * that sum w.r.t. both experts' logits.  Replaces IGN/exp/experiment_classification.py:320-329 (the two F.cross_entropy
 * terms) together with IGN/model/InterpGN.py:44-52 and their autograd.  labels: int64 (B), values in [0, N).
 * out (B,N), eta (B), loss2 = {CE(out,y), CE(sbm,y), their beta-weighted sum}, gsbm / gdnn (B,N) = d(CE(out,y) + beta*CE(sbm,y)) / d logits.
 * 2 <= N <= IGN_HEAD_NMAX; one block, one launch at any N (N > 16: one wave per row, per-row losses summed in row order).   */
int ign_loss_fwd_bwd(const float* sbm, const float* dnn, const long long* labels, float* out, float* eta, float* loss2,
                     float* gsbm, float* gdnn, int B, int N, float beta, void* stream);
/* The same with the model's regulariser value added to loss2[2] on the device (`reg`: one float, nullable): the whole training
 * loss CE(out,y) + info.loss.mean() + beta*CE(sbm,y) of IGN/exp/experiment_classification.py:325-329 in one launch.        */
int ign_loss_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const float* reg, float* out, float* eta,
                         float* loss2, float* gsbm, float* gdnn, int B, int N, float beta, void* stream);
/* The same tail under F.cross_entropy(z, y, weight=class_w, label_smoothing=eps, reduction='mean') for BOTH criteria, in one
 * launch.  class_w: (N) positive finite floats, nullable = all ones; 0 <= label_smoothing < 1.  With D = sum_b w[y_b],
 * W = sum_n w_n, p = softmax(z), lp = log p:
 *   CEw = (1-eps) sum_b w[y_b] (-lp[b,y_b]) / D + (eps/N) sum_b sum_n w_n (-lp[b,n]) / D
 *   dCEw/dz[b,n] = ( (1-eps) w[y_b] (p_n - [n = y_b]) + (eps/N) (p_n W - w_n) ) / D
 * loss3 = {CEw(out), CEw(sbm), CEw(out) + beta*CEw(sbm) + reg[0]}; gsbm / gdnn through the gate as above.  D and W are summed
 * inside the launch in a fixed order (no atomics: two calls agree bitwise); up to 16 classes out / eta are bitwise
 * ign_gate_fwd's.  Labels outside [0, N) are clamped into it.  Limits and error codes as ign_loss_fwd_bwd_reg.            */
int ign_loss_w_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const float* class_w, const float* reg,
                           float* out, float* eta, float* loss3, float* gsbm, float* gdnn, int B, int N, float beta,
                           float label_smoothing, void* stream);
/* The weighted tail with TWO labels per row and a per-row share lam_b of the first (run.py --mix: mixup / CutMix), in one launch.
 * labels (ya) / labels_b (yb): int64 (B); lam_b: float32 (B) in [0, 1] (clamped into it); class_w nullable = all ones;
 * 0 <= label_smoothing < 1.  With p = softmax(z), lp = log p, W = sum_n w_n, a_b = lam_b w[ya_b], c_b = (1 - lam_b) w[yb_b]:
 *   D   = sum_b (a_b + c_b)
 *   CEm = [ (1-eps) sum_b ( a_b (-lp[b,ya_b]) + c_b (-lp[b,yb_b]) ) + (eps/N) sum_b sum_n w_n (-lp[b,n]) ] / D
 *   dCEm/dz[b,n] = [ (1-eps) ( a_b (p_n - [n = ya_b]) + c_b (p_n - [n = yb_b]) ) + (eps/N) (p_n W - w_n) ] / D
 * loss3 = {CEm(out), CEm(sbm), CEm(out) + beta*CEm(sbm) + reg[0]}; gsbm / gdnn through the gate as above.  lam == 1 everywhere is
 * ign_loss_w_fwd_bwd_reg's criterion; without class weights CEm = mean_b [lam_b CE(z_b, ya_b) + (1 - lam_b) CE(z_b, yb_b)].
 * D and W are summed inside the launch in a fixed order (no atomics: two calls agree bitwise); up to 16 classes out / eta are
 * bitwise ign_gate_fwd's.  Labels outside [0, N) are clamped into it.  Limits and error codes as ign_loss_w_fwd_bwd_reg.         */
int ign_loss_mix_fwd_bwd_reg(const float* sbm, const float* dnn, const long long* labels, const long long* labels_b,
                             const float* lam_b, const float* class_w, const float* reg, float* out, float* eta, float* loss3,
                             float* gsbm, float* gdnn, int B, int N, float beta, float label_smoothing, void* stream);

/* Regression loss tail (IGN/exp/experiment_regression.py:59-76): CRPS of the softmax CDF over N bins against the step CDF
 * H_j = [edges[j] >= target] (compared in float64; edges may hold +-inf, a target on an edge counts as >=), batch mean, and
 * its gradient w.r.t. the logits, in one launch.  logits / grad (B,N) fp32, target (B) fp32, edges (N) fp64, loss_out (1).
 * 2 <= N <= IGN_HEAD_NMAX, any B >= 1; one block, per-row losses summed in row order (bitwise repeatable); no allocation.  */
int ign_crps_fwd_bwd(const float* logits, const float* target, const double* edges, float* loss_out, float* grad,
                     int B, int N, void* stream);
/* InterpGN's regression tail in one launch (IGN/exp/experiment_regression.py:159-169): out / eta = the gini gate of
 * ign_gate_fwd (bitwise the same), loss3 = {CRPS(out), CRPS(sbm), CRPS(out) + beta*CRPS(sbm) + reg[0]} (`reg` nullable),
 * gsbm / gdnn = d(CRPS(out) + beta*CRPS(sbm)) / d logits through the gate.  Limits and order as ign_crps_fwd_bwd.          */
int ign_loss_crps_fwd_bwd_reg(const float* sbm, const float* dnn, const float* target, const double* edges, const float* reg,
                              float* out, float* eta, float* loss3, float* gsbm, float* gdnn, int B, int N, float beta,
                              void* stream);

/* Shapelet diversity regulariser of one length group, forward and gradient in one launch.
 * Replaces IGN/model/Shapelet.py:223-230:  mean_{c,i,j} exp(-||w[i,c,:] - w[j,c,:] + eps||_2) (1 - delta_ij), eps = 1e-6.
 * loss_part_c (C): per-channel partial sums (their sum is the group's loss); gw_kcl (K,C,L): d loss / d w.  K <= 16.  */
int ign_diversity_fwd_bwd(const float* w_kcl, float* loss_part_c, float* gw_kcl, int K, int C, int L, float eps,
                          void* stream);

/* Both regularisers of the shapelet bottleneck model -- ShapeBottleneckModel.loss(), IGN/model/Shapelet.py:217-230 -- value and
 * gradients in ONE launch:  loss_out[0] = lambda_reg * mean|W| + lambda_div * sum_g diversity_g  (G = 0 skips the diversity
 * term, as the reference does for lambda_div <= 0);  gW_reg (nW) = lambda_reg * sign(W) / nW (sign(0) = 0);  gw_kcl[g] (K,C,L) =
 * lambda_div * d diversity_g / d w.  Per-block partials are combined in a fixed order by the block that finishes last (bitwise
 * reproducible).  workspace: ign_sbm_reg_workspace_bytes() bytes, ZERO-FILLED ONCE by the caller and then owned by one stream;
 * never written by anyone else.  Layout: word 0 is the ticket counter (0 between calls: the kernel re-arms it), words 1 .. 3 are
 * spare, the partials start at word 4.  Because the ticket does not move with the number of blocks, a buffer sized for the largest
 * configuration serves calls of ANY smaller (G, C, nW) in any order -- each call writes its loss.  G <= 8, K <= 16.          */
size_t ign_sbm_reg_workspace_bytes(int G, int C, long long nW);
int ign_sbm_reg_fwd_bwd(const float* W, float* gW_reg, long long nW, float lambda_reg, int G, const float* const* w_kcl,
                        float* const* gw_kcl, const int* K, const int* L, int C, float lambda_div, float eps, float* loss_out,
                        void* workspace, void* stream);

/* SBM attention head (sbm_cls='attention'; IGN/model/Shapelet.py:117-131, 201-205) without its (B,F,F) scores:
 *   q_i = x_i wq + bq + pos_i,  k_j = x_j wk + bk + pos_j,  out_i = sum_j softmax_j(scale q_i.k_j) x_j   (D = 16 wide q / k)
 * x (B,F) with row pitch ldx >= F; wq / wk the (D,1) projection weights, bq / bk (D), pos (>= F, D); out (B,F) contiguous.
 * lse (B,F): base-2 log-sum-exp of the scaled scores, written when not NULL and read only by ign_sbm_attn_bwd.
 * Backward: gout (B,F) contiguous; writes gx (B,F) and the parameter gradients gwq / gbq / gwk / gbk (D) and gpos (F,D) (rows
 * of pos past F are not touched).  workspace: ign_sbm_attn_workspace_bytes(B, F) bytes, no initialisation needed.
 * Any B, F >= 1; fp32 only; fixed-order reductions, no float atomics: bitwise reproducible.  D must be 16.                */
size_t ign_sbm_attn_workspace_bytes(int B, int F);
int ign_sbm_attn_fwd(const float* x, long long ldx, const float* wq, const float* bq, const float* wk, const float* bk,
                     const float* pos, float* out, float* lse, int B, int F, int D, float scale, void* stream);
int ign_sbm_attn_bwd(const float* x, long long ldx, const float* wq, const float* bq, const float* wk, const float* bk,
                     const float* pos, const float* out, const float* lse, const float* gout, float* gx, float* gwq, float* gbq,
                     float* gwk, float* gbk, float* gpos, void* workspace, int B, int F, int D, float scale, void* stream);

/* SBM bilinear head (sbm_cls='bilinear'; IGN/model/Shapelet.py:170-177, 199-205): the nn.Bilinear term, no bias,
 *   out[b,n] = sum_{i,j} u[b,i] w[n,i,j] v[b,j]
 * as exact-fp32 matrix-core GEMMs.  u, v (B,F), w (N,F,F), out (B,N), all contiguous.  Forward: T_n = u w_n and the row
 * dot with v; t_save (B,N,F) receives T when not NULL (the backward's gv needs it).  Backward with gout (B,N):
 * gu = sum_n (gout_n . v) w_n^T, gv = sum_n gout_n . T_n (needs t_save), gw_n = (gout_n . u)^T v; each of gu / gv / gw may
 * be NULL and is then not computed.  workspace: ign_sbm_bilinear_workspace_bytes(B, F, N) bytes, no initialisation needed:
 * B*N floats per 128 columns of F (forward row-dot partials), or B*N*F (the backward's per-class partials of gu) if more;
 * the backward needs it only for gu with N > 1.
 * Any B, F, N >= 1; fixed-order reductions, no float atomics: bitwise reproducible.  No F*F or B*F*F temporary.        */
size_t ign_sbm_bilinear_workspace_bytes(int B, int F, int N);
int ign_sbm_bilinear_fwd(const float* u, const float* v, const float* w, float* out, float* t_save, void* workspace, int B, int F,
                         int N, void* stream);
int ign_sbm_bilinear_bwd(const float* u, const float* v, const float* w, const float* t_save, const float* gout, float* gu,
                         float* gv, float* gw, void* workspace, int B, int F, int N, void* stream);

/* One Adam step over flat buffers (torch.optim.Adam semantics, no weight decay / amsgrad): replaces the per-tensor
 * optimizer.step() of IGN/exp/experiment_classification.py:338.  `step` is the 1-based step count; all four buffers
 * 16-byte aligned.                                                                                                    */
int ign_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                  float beta1, float beta2, float eps, int step, void* stream);

/* Copy `count` gradient tensors (src[i], n[i] floats) to flat + off[i] in one launch: the flat gradient bucket of the
 * data-parallel step is filled by one kernel instead of one accumulate kernel per parameter.  src / off / n are HOST arrays. */
int ign_gather_flat(const void* const* src, const long long* off, const long long* n, int count, float* flat, void* stream);

/* The same step with the step count kept on the device (*step_dev is incremented, bc_dev[2] receives the bias
 * corrections): nothing host-side changes between steps, so the launch sequence can be captured into a hipGraph.  All
 * four buffers 16-byte aligned.                                                                                       */
int ign_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                      float beta1, float beta2, float eps, int* step_dev, float* bc_dev, void* stream);

/* Gradient clipping on the flat gradient buffer (torch.nn.utils.clip_grad_norm_, IGN/exp/experiment_classification.py:336-337).
 * ign_grad_norm_clip: out2[0] = ||g||_2 over the n floats of g (the zero padding between parameter slots adds nothing),
 * out2[1] = min(1, max_norm / (out2[0] + 1e-6)), the coefficient clip_grad_norm_ multiplies the gradients by.  One launch and no
 * host synchronisation: every block sums the squares of a fixed contiguous slice of 4096 floats (16-byte loads, wave butterfly,
 * waves in order through LDS) into one partial; the block that finishes last adds the partials in index order (in double).  No
 * float atomics: the result is bitwise repeatable and independent of how the launch was scheduled.  Non-finite values get no
 * special case -- an inf gradient gives the coefficient 0 (inf * 0 = NaN in that element), a NaN gradient a NaN coefficient, as
 * in torch.  g and workspace 16-byte aligned.  workspace: ign_grad_norm_workspace_bytes(n) bytes, ZERO-FILLED ONCE before the
 * first call (it holds an integer ticket counter that every call hands back at zero); calls that share a workspace must be
 * ordered on one stream.                                                                                                      */
size_t ign_grad_norm_workspace_bytes(long long n);
int ign_grad_norm_clip(const float* g, long long n, float max_norm, float* out2, void* workspace, void* stream);

/* ign_adam_step / ign_adam_step_dev reading grad[i] * coef_dev[0] (coef_dev = out2 + 1 of ign_grad_norm_clip): clipping folded
 * into the optimizer, no extra pass over the gradients and no write to them.  coef_dev == NULL: exactly ign_adam_step /
 * ign_adam_step_dev (same kernels, same bits).  Both: all four buffers 16-byte aligned.                                       */
int ign_adam_step_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                       float beta1, float beta2, float eps, int step, const float* coef_dev, void* stream);
int ign_adam_step_clip_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                           float beta1, float beta2, float eps, int* step_dev, float* bc_dev, const float* coef_dev,
                           void* stream);

/* g[i] *= coef_dev[0] in place, i < n (g 16-byte aligned): for callers that want the gradients themselves clipped, the
 * stand-alone clip_grad_norm_ contract.                                                                                      */
int ign_scale_flat(float* g, long long n, const float* coef_dev, void* stream);

/* ign_gather_flat that ADDS src[i] into flat + off[i] instead of overwriting: gradient accumulation over micro-batches in one
 * launch per micro-step (one extra read of each slot) instead of one accumulate kernel per parameter.                        */
int ign_gather_flat_acc(const void* const* src, const long long* off, const long long* n, int count, float* flat, void* stream);

/* AdamW with a per-step learning-rate schedule and an EMA of the parameters, on the flat buffers (csrc/ign_sched.h holds the rule).
 * Optimizer step s = 1, 2, ...; W = warmup, M = min_lr, S = total_steps:
 *   s < W: lr = base_lr * s / W;   IGN_SCHED_CONSTANT (0), s >= W: lr = base_lr;
 *   IGN_SCHED_COSINE (1), s >= W: lr = M + (base_lr - M) * 0.5 * (1 + cos(pi * t / T)), t = min(s - W, T), T = max(1, S - W);
 *   EMA decay d = min(ema_decay, (1 + s) / (10 + s));   all in double, rounded to float once.
 * ign_sched_lr: the learning rate of step `step` by that rule, on the host (no device, no stream): for logging and tests.       */
float ign_sched_lr(int sched_kind, double base_lr, int warmup, double min_lr, long long total_steps, long long step);

/* One AdamW step with the count on the device (graph-capturable, like ign_adam_step_dev): a tick kernel increments *step_dev and
 * leaves hp_dev[4] = [bias_correction1, sqrt(bias_correction2), lr of this step, EMA decay of this step]; the update kernel reads
 * them there, applies param *= 1 - lr * weight_decay where decay_mask says so and then the Adam update of ign_adam_step (same
 * element rule).  decay_mask: one byte per 64-float chunk of the buffers, ceil(n / 64) bytes ON THE DEVICE, non-zero = decay;
 * NULL = decay every element.  weight_decay == 0 skips the multiply.  coef_dev: the clip coefficient of ign_grad_norm_clip
 * (grad is read as grad * coef_dev[0]) or NULL for no clipping.  The schedule arguments must not change over a captured run.
 * With weight_decay 0, IGN_SCHED_CONSTANT and warmup 0 the parameters and moments are bit for bit those of ign_adam_step_dev /
 * ign_adam_step_clip_dev at lr = (float)base_lr.  All four buffers 16-byte aligned; arguments out of range: IGN_E_ARG.          */
int ign_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float beta1, float beta2,
                       float eps, float weight_decay, const unsigned char* decay_mask, int sched_kind, double base_lr, int warmup,
                       double min_lr, long long total_steps, double ema_decay, int* step_dev, float* hp_dev, const float* coef_dev,
                       void* stream);

/* ema[i] += (1 - hp_dev[3]) * (param[i] - ema[i]), i < n: the exponential moving average of the parameters with the decay the
 * tick of ign_adamw_step_dev left on the device.  param == ema (in value) leaves ema unchanged to the bit.  A launch of its own so
 * that it can follow whatever rewrites the parameters after the optimizer (the --pos_weight clamp).  Both 16-byte aligned.     */
int ign_ema_update(float* ema, const float* param, long long n, const float* hp_dev, void* stream);

/* Exchange the n floats of a and b in place, one launch, no temporary (a and b 16-byte aligned, not overlapping): the averaged
 * weights go into the parameter buffer for validation and back out without any pointer changing.                             */
int ign_swap_flat(float* a, float* b, long long n, void* stream);

/* EEG-CNN block 1 without its (B,F1,C,T) intermediate (1 GB at B=256) -- see csrc/ign_eegcnn.hip for the algebra.
 * Replaces the BatchNorm-1 batch statistics of IGN/model/eegcnn.py:90-91 (block1_conv1 -> block1_bn1):
 *   y1[r,f,t] = sum_j w1[f,j] xpad[r, t+j]   (rows r = (b,c); 'same' zero padding, pad_left on the left)
 *   fwd:  m2[f]   = sum_{r,t} (y1 - mu[f])^2                     (mu = the batch mean, supplied by the caller)
 *   bwd:  g[f,j]  = sum_{r,t} (y1 - mu[f]) xpad[r, t+j]          (= 1/2 d m2[f] / d w1[f,j])
 * x (rows,T), w1 (F1,k1), mu (F1); workspace: ign_conv1_sumsq_workspace_bytes().  Deterministic reductions.       */
size_t ign_conv1_sumsq_workspace_bytes(int rows, int F1, int k1);
int ign_conv1_sumsq_fwd(const float* x, const float* w1, const float* mu, float* m2, void* workspace,
                        int rows, int T, int F1, int k1, int pad_left, void* stream);
int ign_conv1_sumsq_bwd(const float* x, const float* w1, const float* mu, float* g_fj, void* workspace,
                        int rows, int T, int F1, int k1, int pad_left, void* stream);

/* LayerNorm over the last dimension of an (R, D) matrix (nn.LayerNorm semantics: biased variance, eps inside the sqrt), forward
 * and backward; D % 4 == 0, D <= 4096 (backward: D <= 2048).  fwd saves mean / rstd (R each).  bwd: gx and, when not NULL,
 * dgamma / dbeta (fixed-order two-pass reduction: reproducible); part = ign_layernorm_parts(R, D) * 2 * D floats of workspace.
 * Replaces IGN/layers/Transformer_EncDec.py:36-37,48,76-77, the norms of nn.TransformerEncoderLayer in IGN/model/eegcnn.py:219-228
 * and IGN/model/TimesNet.py:197.                                                                                          */
long long ign_layernorm_parts(long long R, int D);
int ign_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long long R, int D,
                      float eps, void* stream);
/* y = LayerNorm(x + res) in one pass: the residual connection of a post-norm encoder layer (IGN/layers/Transformer_EncDec.py:
 * 36-37,48; nn.TransformerEncoderLayer of IGN/model/eegcnn.py:219-228) in front of its LayerNorm.  `sum` (R, D) receives x + res,
 * the tensor ign_layernorm_bwd takes as `x`; its gx is the gradient of both addends.                                          */
int ign_layernorm_res_fwd(const float* x, const float* res, float* sum, const float* gamma, const float* beta, float* y,
                          float* mean, float* rstd, long long R, int D, float eps, void* stream);
int ign_layernorm_bwd(const float* x, const float* gy, const float* gamma, const float* mean, const float* rstd, float* gx,
                      float* dgamma, float* dbeta, float* part, long long R, int D, void* stream);
/* ign_layernorm_bwd that also takes max |gx| as an atomic maximum into *amax_slot (caller zeroes): the magnitude bound of dL/dx
 * for the fp16 GEMMs of the dense layer behind (ign_clconv_fwd_h3 / ign_linear_wgrad_h3), where gx is produced anyway.           */
int ign_layernorm_bwd_amax(const float* x, const float* gy, const float* gamma, const float* mean, const float* rstd, float* gx,
                           float* dgamma, float* dbeta, float* part, float* amax_slot, long long R, int D, void* stream);
/* Lag sums C[d] = sum_rows sum_u x[row][u] x[row][u+d], d < K <= 128 -- with edge terms from the first / last k-1 samples of
 * each row they give the window Gram matrix G[j,j'] = sum x_pad[t+j] x_pad[t+j'] and BatchNorm-1's batch variance of
 * IGN/model/eegcnn.py:90-91 as the quadratic form w1^T G w1 (gradient 2 G w1): K*T FMA per row for all filters, no backward
 * pass over the data.  part: (ign_autocorr_parts(rows), K) partial sums, added up by the caller in double.                   */
long long ign_autocorr_parts(int rows);
int ign_autocorr_fwd(const float* x_rows, float* part, int rows, int T, int K, void* stream);
/* The edge terms of that Gram matrix: per row only the first / last k-1 samples of the zero-padded row xp (left pad pad_left)
 * enter.  part: (ign_edge_lagprod_parts(rows), 2, 124, 128) floats, [b][0][s][d] = sum over the block's rows of xp[s] xp[s+d]
 * (head, s + d < k-1), [b][1][s][d] = the same at xp[T+s] (tail); summed over b by the caller in double.  k <= 125.  Column
 * d = 127 (never a lag) carries the plain column sums of the same samples: [b][0][s][127] = sum xp[s], [b][1][s][127] = sum
 * xp[T+s] -- what the zero padding removes from the per-tap sums behind BatchNorm-1's batch MEAN (ign_bn1_gram).                */
long long ign_edge_lagprod_parts(int rows);
int ign_edge_lagprod_fwd(const float* x_rows, float* part, int rows, int T, int k, int pad_left, void* stream);
/* BatchNorm-1 of the EEG-CNN block (IGN/model/eegcnn.py:90-91: batch statistics of the (B, F1, C, T) temporal convolution that is
 * never formed) from data statistics, in three small launches instead of ~45 float64 library kernels (cumsum / flip / cat /
 * gather / einsum and their autograd):
 *   ign_bn1_data_stats  x (rows, T) -> the window Gram matrix G (k, k) and the per-tap sums S (k), float64, in four launches and no
 *                     library call: lag sums + row sums (ign_autocorr_sum_fwd), edge terms + column sums of the first / last k-1
 *                     samples (ign_edge_lagprod_fwd), their per-block partials summed in float64, and the assembly
 *                        G[j][j+d] = C[d] - sum_{s<j} Dh[s][d] - sum_{s>=j} Dt[s][d],  S[j] = total - (samples tap j never sees).
 *                     workspace: ign_bn1_data_stats_workspace_bytes.  IGN_E_UNSUP for rows longer than 1024 samples.
 *   ign_bn1_fold_fwd  per filter f: mu = w_f . S / n, var = w_f^T G w_f / n - mu^2, a = gamma_f / sqrt(var + eps), b = beta_f - a mu;
 *                     outputs alpha[f D + i] = a, cshift[f D + i] = b * rs[f D + i] (rs = row sums of the depthwise weights: the
 *                     affine map of BatchNorm-1 as it enters the fused BatchNorm-2 op), updates the running statistics
 *                     (nullable) with `momentum`, saves G w_f, mu, var, 1/sqrt for the backward
 *   ign_bn1_fold_bwd  gradients of w1 (F1, k), gamma, beta and rs from those of alpha / cshift (closed form: d mu = S / n,
 *                     d var = 2 G w / n - 2 mu S / n).
 * k <= 125, F1 * D <= 4096.                                                                                                    */
size_t ign_bn1_data_stats_workspace_bytes(int rows, int T, int k);
int ign_bn1_data_stats(const float* x_rows, int rows, int T, int k, int pad_left, void* workspace, double* G, double* S, void* stream);
/* ign_autocorr_fwd restricted to its register-tiled kernel (T <= 1024), which then also returns the plain sum of each block's rows:
 * rowsum_part[p], p < *used_parts = partial rows actually written (later rows of `part` are not touched).                         */
int ign_autocorr_sum_fwd(const float* x_rows, float* part, float* rowsum_part, int rows, int T, int K, int* used_parts, void* stream);
int ign_bn1_fold_fwd(const float* w1, const float* gamma, const float* beta, const float* rs, const double* G, const double* S,
                     double n, float eps, float momentum, float* running_mean, float* running_var, float* alpha, float* cshift,
                     double* saved /* (F1, k + 4) */, int F1, int k, int Dm, void* stream);
int ign_bn1_fold_bwd(const float* g_alpha, const float* g_cshift, const float* w1, const float* gamma, const float* rs,
                     const double* S, const double* saved, double n, float* g_w1, float* g_gamma, float* g_beta, float* g_rs,
                     int F1, int k, int Dm, void* stream);
/* Depthwise (per-channel) 1-D convolution over time, zero 'same' padding: y[b,c,t] = sum_j w[c,j] xpad[b,c,t+j].
 * Replaces the temporal convolutions of IGN/model/eegcnn.py:67 (after the channel contraction) and :78 (block2_conv1).
 * flip=1 correlates with the reversed filter (gradient w.r.t. x: call with dy and pad_left = k-1-pad_left).
 * bwd_weight: dw[c,j] = sum_{b,t} dy[b,c,t] xpad[b,c,t+j]  (workspace: ign_dwconv1d_bwd_weight_workspace_bytes()). */
int ign_dwconv1d_fwd(const float* x, const float* w, float* y, int B, int C, int T, int k, int pad_left, int flip,
                     void* stream);
size_t ign_dwconv1d_bwd_weight_workspace_bytes(int B, int C, int k);
int ign_dwconv1d_bwd_weight(const float* x, const float* dy, float* dw, void* workspace, int B, int C, int T, int k,
                            int pad_left, void* stream);

/* EEG-CNN block, the ops around the depthwise temporal convolutions (IGN/model/eegcnn.py:67-108), (B, channels, T) layout.
 * Channel contraction u[b,o,t] = sum_c W[o,c] x[b,c,t]: the depthwise SPATIAL conv (eegcnn.py:71,92; Conv2d(F1, D*F1, (C,1),
 * groups=F1) applied after the temporal conv commutes with it, see csrc/ign_eegcnn.hip) and the POINTWISE conv (:79,100).
 *   wt_ci64: W^T zero-padded to (Ci, 64) floats (Co <= 64, Ci <= 128).  The input gradient is the same call with W in place of
 *   W^T; bwd_weight: dW[o,c] = sum_{b,t} du[b,o,t] x[b,c,t] (workspace: ign_chan_contract_bwd_weight_workspace_bytes()).     */
int ign_chan_contract_fwd(const float* x_bct, const float* wt_ci64, float* u_bot, int B, int Ci, int Co, int T, void* stream);
size_t ign_chan_contract_bwd_weight_workspace_bytes(int B, int Ci, int Co, int T);
int ign_chan_contract_bwd_weight(const float* du_bot, const float* x_bct, float* dw_oc, void* workspace, int B, int Ci, int Co,
                                 int T, void* stream);

/* BatchNorm2d with batch statistics + ELU + AvgPool2d((1,P)) as one op (eegcnn.py:72-74,93-95 / :80-82,101-103).
 *   ign_chan_stats: sums_c2 (C,2) DOUBLES = per-channel sum v, sum v^2 over (b,t)  (workspace: ign_chan_stats_workspace_bytes()).
 *   ign_affine_elu_pool_fwd: out[b,c,tp] = mean_{i<P} ELU(scale[c] v[b,c,tp P+i] + shift[c]); the caller folds BatchNorm (and the
 *     affine map in front of it) into scale / shift; Tp = T / P.
 *   backward: ign_bn_elu_pool_bwd_sums -> (C,2) doubles S1 = sum dz, S2 = sum dz (v - mean[c]) with dz = ELU'(.) dout / P;
 *     ign_bn_elu_pool_bwd_apply: dv = ka[c] dz + kb[c] + kc[c] v (the BatchNorm backward as three per-channel coefficients).
 *   ign_bn_fold_fwd / _bwd: the per-channel algebra between the two passes in one launch each -- forward: moments of v, the
 *     affine map y = alpha v + c in front of the BatchNorm (NULL: identity), gamma, beta -> scale / shift of the apply pass,
 *     fold_c2 (C,2) doubles {mean_v, r = rsqrt(alpha^2 var_v + eps)} kept for the backward, and the nn.BatchNorm running-statistics
 *     update (momentum, unbiased variance; NULL pointers: skipped); backward: (S1, S2) -> ka / kb / kc and dgamma, dbeta, dalpha. */
size_t ign_chan_stats_workspace_bytes(int B, int C);
int ign_chan_stats(const float* v_bct, double* sums_c2, void* workspace, int B, int C, int T, void* stream);
int ign_affine_elu_pool_fwd(const float* v_bct, const float* scale_c, const float* shift_c, float* out, int B, int C, int T, int P,
                            void* stream);
int ign_bn_elu_pool_bwd_sums(const float* v_bct, const float* dout, const float* scale_c, const float* shift_c, const float* mean_c,
                             double* sums_c2, void* workspace, int B, int C, int T, int P, void* stream);
int ign_bn_elu_pool_bwd_apply(const float* v_bct, const float* dout, const float* scale_c, const float* shift_c, const float* ka_c,
                              const float* kb_c, const float* kc_c, float* dv_bct, int B, int C, int T, int P, void* stream);
int ign_bn_fold_fwd(const double* sums_c2, const float* alpha_c, const float* cshift_c, const float* gamma_c, const float* beta_c,
                    float* scale_c, float* shift_c, double* fold_c2, float* running_mean, float* running_var, int C, long long n,
                    float eps, float momentum, void* stream);
int ign_bn_fold_bwd(const double* sums_c2, const double* fold_c2, const float* alpha_c, const float* gamma_c, float* ka_c, float* kb_c,
                    float* kc_c, float* dgamma_c, float* dbeta_c, float* dalpha_c, int C, long long n, float eps, void* stream);

/* ---- FCN expert: channels-last 1-D convolution as an implicit GEMM on the fp32 matrix cores, BatchNorm + ReLU
 * folded into the GEMM prologues / epilogues (csrc/ign_clconv_{f32,x6}.hip, ign_bn.hip).  Replaces IGN/model/FullyConvNet.py:31-59
 * (3 x [Conv1d -> BatchNorm1d -> ReLU] -> AdaptiveAvgPool1d) and its autograd.  Activations are (B, T, C) row-major
 * (the loader's layout); a 'valid' convolution: Tout = Tin - k + 1.  All sums are fixed-order (deterministic).
 *
 * ign_clconv_pack_weights: w (Co,Ci,k) [torch Conv1d layout] -> wt_fwd (Co, k*Ci) with kk = j*Ci + ci, and (if not
 *   NULL) wt_dgrad (Ci, k*Co) with kk = jj*Co + co holding w[co][ci][k-1-jj].
 * ign_clconv_fwd: y[b,t,co] = bias[co] + sum_{j,ci} in[b,t+j,ci] w[co,ci,j], where in = x, or relu(pro_a[ci]*x + pro_b[ci])
 *   when pro_a/pro_b are given (the BatchNorm affine + ReLU of the block below, applied while staging).
 *   stat_part (ign_clconv_mtiles(B*Tout), 2, Co), nullable: per-tile sum_y and sum_y^2 for this block's BatchNorm.
 * ign_clconv_dgrad: given dyp (B, Tout + 2(k-1), Co) = dL/dy zero-padded by k-1 rows on both sides of every sample,
 *   computes dL/dz[b,t,ci] (z = this conv's input = relu(a_in*y_in + b_in)) and, in the epilogue, the ReLU-masked
 *   g_in = dL/dz * [a_in*y_in + b_in > 0] (B,Tin,Ci) plus stat_part (ign_clconv_mtiles(B*Tin), 2, Ci) = per-tile
 *   sum g_in and sum g_in*(y_in - mean_in)*invstd_in   (BatchNorm backward sums of the block below).
 * ign_clconv_wgrad: dw[co,ci,j] = sum_{b,t} dy[b,t,co] in[b,t+j,ci]  (in as for fwd; dy rows are read from a buffer
 *   padded by dy_pad rows per side).  Co % 4 == 0.  workspace: ign_clconv_wgrad_workspace_bytes().                  */
long long ign_clconv_mtiles(long long M);
int ign_clconv_pack_weights(const float* w_oik, float* wt_fwd, float* wt_dgrad, int Co, int Ci, int k, void* stream);
int ign_clconv_fwd(const float* x, const float* wt_fwd, const float* bias, const float* pro_a, const float* pro_b,
                   float* y, float* stat_part, int B, int Tin, int Ci, int Co, int k, void* stream);
int ign_clconv_dgrad(const float* dyp, const float* wt_dgrad, const float* y_in, const float* a_in, const float* b_in,
                     const float* mean_in, const float* invstd_in, float* g_in, float* stat_part,
                     int B, int Tin, int Ci, int Co, int k, void* stream);
/* ign_clconv_dgrad_input: the data gradient of a convolution whose input is RAW DATA (the expert's first block: no BatchNorm / ReLU
 *   below it), gx[b,t,ci] = sum_{jj,co} dyp[b,t+jj,co] w[co,ci,k-1-jj]  (gx (B,Tin,Ci); dyp, wt_dgrad as for ign_clconv_dgrad).
 *   Plain epilogue: no bias, no mask, no partial sums, nothing written outside gx.  Any Ci >= 1 (the channel count of the data:
 *   122, 6, 3, 1 -- ragged n-tiles store per column), Co % 4 == 0.  Fixed-order sums, no atomics: bitwise repeatable.  The _x6 /
 *   _bf16 / _h3 forms (declared with their siblings below) take the packed transposed weights of their arithmetic, k <= 16;
 *   _h3 the bounds of |dL/dy| and |W|.  Timed under "clconv_dgrad_input".  What the saliency of the gated mixture runs
 *   (utils/saliency.py, explain="gated" / "dnn"); the reference gets it from autograd through nn.Conv1d (IGN/model/FullyConvNet.py:32). */
int ign_clconv_dgrad_input(const float* dyp, const float* wt_dgrad, float* gx, int B, int Tin, int Ci, int Co, int k, void* stream);
/* Split-bf16 ("x6") variants of fwd / dgrad: the same maths at fp32 rounding-level accuracy on the bf16 matrix cores.
 * gfx950 executes fp32-input MFMA at the fp32 vector rate; here every fp32 operand is split exactly into three bf16 terms
 * and the six partial products of weight >= 2^-16 are accumulated in fp32 (v_mfma_f32_32x32x16_bf16): 2.7x the fp32-MFMA
 * throughput, error vs float64 at the level of fp32 accumulation (tests/test_gpu_fcn.py).  The weights arrive pre-split:
 * ign_clconv_pack_weights_x3 writes wt3_fwd (ign_clconv_x3_elems(Co, Ci, k) bf16) and, if not NULL, wt3_dgrad
 * (ign_clconv_x3_elems(Ci, Co, k) bf16) in step-block-major order: the 3 planes x 128 rows x 16 channels that one (n-tile,
 * 16-channel chunk, tap) step of the kernel consumes are one contiguous 12 KB block (zero in padded rows / channels).  Activations stay fp32 in HBM
 * and are split while they are staged into LDS -- once per (128 + k - 1)-row span and 16-channel chunk, shared by all k taps.
 * The x6 kernels tile every sample separately: stat_part has ign_clconv_x6_mtiles(B, Tout) [fwd] resp. (B, Tin) [dgrad]
 * rows.  k <= 16.                                                                                                       */
int ign_clconv_kpad(int C);                          /* channels rounded up to 16 */
long long ign_clconv_x3_elems(int rows, int chans, int k);   /* bf16 elements of a packed set: fwd (Co, Ci, k), dgrad (Ci, Co, k) */
long long ign_clconv_x6_mtiles(int B, int rows);     /* rows of stat_part for the x6 kernels: B * ceil(rows / 128) */
int ign_clconv_pack_weights_x3(const float* w_oik, void* wt3_fwd, void* wt3_dgrad, int Co, int Ci, int k, void* stream);
int ign_clconv_fwd_x6(const float* x, const void* wt3_fwd, const float* bias, const float* pro_a, const float* pro_b,
                      float* y, float* stat_part, int B, int Tin, int Ci, int Co, int k, void* stream);
int ign_clconv_dgrad_x6(const float* dyp, const void* wt3_dgrad, const float* y_in, const float* a_in, const float* b_in,
                        const float* mean_in, const float* invstd_in, float* g_in, float* stat_part,
                        int B, int Tin, int Ci, int Co, int k, void* stream);
int ign_clconv_dgrad_input_x6(const float* dyp, const void* wt3_dgrad, float* gx, int B, int Tin, int Ci, int Co, int k, void* stream);
/* Weight gradient on the bf16 matrix cores (same split): operands staged row-major and read with the transposing LDS read
 * ds_read_b64_tr_b16; one staged input span serves all k taps.  k in {2, 3, 5, 8} (the FCN expert's kernels), Co % 4 == 0;
 * k = 1 (a Linear layer over the B*Tin rows; needs Ci % 4 == 0, dy_pad == 0, no prologue) runs 128 x 128 tiles instead.
 * Same arguments and result as ign_clconv_wgrad.                                                                        */
size_t ign_clconv_wgrad_x6_workspace_bytes(int B, int Tin, int Ci, int Co, int k);
int ign_clconv_wgrad_x6(const float* dyp, int dy_pad, const float* x, const float* pro_a, const float* pro_b,
                        float* dw_oik, void* workspace, int B, int Tin, int Ci, int Co, int k, void* stream);
/* Deferred reduction: ign_clconv_wgrad_x6 / _bf16 called with dw_oik == NULL (k > 1) leave their ign_clconv_wgrad_x6_nsplit()
 * partial slabs in `workspace`; ign_clconv_wgrad_reduce_multi then reduces up to 8 layers in ONE launch (same ascending-order
 * sums as the per-layer reduction: identical bits).  Tables are host arrays.                                                  */
int ign_clconv_wgrad_x6_nsplit(int B, int Tin, int Ci, int Co, int k);
int ign_clconv_wgrad_reduce_multi(int n, const void* const* part, float* const* dw_oik, const int* nsplit, const int* Co,
                                  const int* Ci, const int* k, void* stream);
/* ign_clconv_pack_weights_x3 for up to 8 layers in ONE launch; counters[l] (nullable table / entries): an int64 device counter
 * incremented by one -- nn.BatchNorm1d.num_batches_tracked of the BatchNorm behind layer l in training mode
 * (IGN/model/FullyConvNet.py:31-50 builds Conv1d + BatchNorm1d pairs).                                                       */
int ign_clconv_pack_weights_x3_multi(int n, const float* const* w_oik, void* const* wt3_fwd, void* const* wt3_dgrad,
                                     const int* Co, const int* Ci, const int* k, long long* const* counters, void* stream);

/* ---- Two-plane fp16 GEMMs ("h3"): fp32 accuracy from THREE products per element pair instead of six.
 * Every fp32 operand x of a GEMM is first multiplied by a power of two s (exact) chosen from an upper bound of the tensor's
 * magnitude so that 2^13 <= bound * s < 2^14, then split into two fp16 terms h0 = fp16(s x), h1 = fp16(s x - h0) (the residual
 * is an exact fp32 subtraction), and the products a0 b0 + a0 b1 + a1 b0 are accumulated in fp32 by v_mfma_f32_32x32x16_f16; the
 * epilogue multiplies by 1 / (s_a s_b) (exact).  What is dropped is O(2^-22 |a b|) per product -- at the level of the fp32
 * accumulation error of a K ~ 1000 reduction; measured against float64 the results are as close as the six-product bf16 kernels
 * and the fp32-MFMA kernels (tests/test_gpu_fcn.py runs every case on all three).  Without the scaling fp16's narrow exponent
 * range would lose the second term of small operands (gradients of 1e-5: 5e-4 relative error); with it the absolute error of
 * an element is <= 2^-22 of the tensor's bound.  Bounds are device scalars (`slots`: 4 floats per layer, see ign_fcn_scan):
 *   weights        max |W|                       -- ign_fcn_scan, from the parameters
 *   layer input    l = 0: max |x| (ign_absmax);  l > 0: max_c(|gamma_c| sqrt(R - 1) + |beta_c|) of the BatchNorm in front, a HARD
 *                  bound of relu(gamma yhat + beta): a value standardised with the batch's own statistics over R rows cannot
 *                  exceed sqrt(R - 1) (training mode only; eval mode keeps the bf16 kernels)
 *   dL/dy          max |dL/dy|, taken by ign_bn_bwd_apply_amax as it writes the tensor (integer atomicMax on the bit patterns of
 *                  non-negative floats: exact and order-independent, so results stay bitwise reproducible)
 * Supported magnitudes: the scale exponent is clamped to +-60, i.e. bounds from 2^-46 (1.4e-14; below it the operand loses
 * precision gradually and finally reads as zero -- gradients of that size no longer move an fp32 weight) to 2^74 (1.9e22; a
 * tensor beyond it overflows fp16 and the result is NaN, as loudly as the diverged run that produced it).  A bound of 0 or a
 * non-finite bound selects scale 1.  A bound should BE an upper bound; the scaled bound lies in [2^13, 2^14) and fp16 reaches
 * 65504, so an element up to 3.9 times the bound is still split exactly like any other (the host side relies on a factor 1.13 of
 * this headroom where dL/du of a GELU inherits the bound of dL/dy), an element beyond 4 times the bound overflows to infinity.
 * Replaces the same reference lines as ign_clconv_fwd / _dgrad / _wgrad (IGN/model/FullyConvNet.py:31-59 and its autograd).   */
int ign_absmax(const float* x, long long n, float* slot /* max'ed into, caller zeroes */, void* stream);
/* ... of up to 16 tensors in one launch (a model's dense-layer weights once per step): slots[i] = max |x[i][0..count[i])|.     */
int ign_absmax_multi(int n, const float* const* x, const long long* count, float* const* slots, void* stream);
/* ign_fcn_scan also clears `zero[0..nzero)` (nullable / 0): the identically-zero gradients of the convolution biases in front of
 * a batch-statistics BatchNorm are views of that buffer, so the backward needs no fill launch.                               */
int ign_fcn_scan(int nl, const float* const* w, const long long* nw, const float* const* gamma_prev, const float* const* beta_prev,
                 const int* C_prev, const long long* R_prev, float* slots /* (nl, 4): written */, float* zero, long long nzero,
                 void* stream);
int ign_clconv_pack_weights_h2_multi(int n, const float* const* w_oik, void* const* wt_fwd, void* const* wt_dgrad, const int* Co,
                                     const int* Ci, const int* k, long long* const* counters, const float* const* w_bounds,
                                     void* stream);
int ign_clconv_fwd_h3(const float* x, const void* wt_h2, const float* bias, const float* pro_a, const float* pro_b, float* y,
                      float* stat_part, const float* bound_in, const float* bound_w, int B, int Tin, int Ci, int Co, int k,
                      void* stream);
/* the same, additionally max'ing max |y| into the device float amax_out (nullable; the caller zeroes it): the magnitude bound of
 * the output for the next GEMM that consumes it -- taken in the epilogue instead of by a pass over the tensor (ign_absmax)     */
int ign_clconv_fwd_h3_amax(const float* x, const void* wt_h2, const float* bias, const float* pro_a, const float* pro_b, float* y,
                           float* stat_part, const float* bound_in, const float* bound_w, float* amax_out, int B, int Tin, int Ci,
                           int Co, int k, void* stream);
/* du = (g W) * gelu'(u) in ONE GEMM: the input gradient of the feed-forward's second dense layer z = gelu(u) W^T + b
 * (IGN/layers/Transformer_EncDec.py:46-47) THROUGH the activation -- the exact-GELU derivative Phi(u) + u phi(u) is applied in the
 * epilogue, so dL/dy is never written and aten::gelu_backward's three passes over the (rows, d_ff) tensors disappear.  g (M, Co),
 * wd_h2 = the packed TRANSPOSED weight (as for the input gradient via ign_clconv_fwd_h3), u / du (M, Ci); Ci % 256 == 0,
 * Co % 4 == 0; amax_out nullable (max |du|).  f16x3 arithmetic only (IGN_E_UNSUP otherwise: callers keep the two-kernel route).  */
int ign_linear_dgrad_gelu_h3(const float* g, const void* wd_h2, const float* u, float* du, const float* bound_g, const float* bound_w,
                             float* amax_out, long long M, int Co, int Ci, void* stream);
int ign_clconv_dgrad_h3(const float* dyp, const void* wt_h2_dgrad, const float* y_in, const float* a_in, const float* b_in,
                        const float* mean_in, const float* invstd_in, float* g_in, float* stat_part, const float* bound_dy,
                        const float* bound_w, int B, int Tin, int Ci, int Co, int k, void* stream);
int ign_clconv_dgrad_input_h3(const float* dyp, const void* wt_h2_dgrad, float* gx, const float* bound_dy, const float* bound_w,
                              int B, int Tin, int Ci, int Co, int k, void* stream);
int ign_clconv_wgrad_h3(const float* dyp, int dy_pad, const float* x, const float* pro_a, const float* pro_b, float* dw_oik,
                        void* workspace, const float* bound_dy, const float* bound_x, int B, int Tin, int Ci, int Co, int k,
                        void* stream);
int ign_linear_wgrad_h3(const float* dy, const float* x, float* dw, float* db, void* workspace, const float* bound_dy,
                        const float* bound_x, long long M, int Ci, int Co, void* stream);
int ign_bn_bwd_apply_amax(const float* g, const float* y, const float* a, const float* mean, const float* invstd,
                          const float* dbeta, const float* dgamma, float* dyp, float* amax_slot, int B, int T, int C, int pad,
                          int training, void* stream);

/* The three split-bf16 GEMMs with ONE product per step: operands rounded to bf16 (round-to-nearest-even), products and sums in
 * fp32 -- the arithmetic of the reference's default bf16-autocast mode (IGN/exp/experiment_classification.py:319; `--amp`
 * switches it OFF).  Same packed weights (plane 0 is read), same arguments, same workspace as the *_x6 entry points.        */
int ign_clconv_fwd_bf16(const float* x, const void* wt3_fwd, const float* bias, const float* pro_a, const float* pro_b,
                        float* y, float* stat_part, int B, int Tin, int Ci, int Co, int k, void* stream);
int ign_clconv_dgrad_bf16(const float* dyp, const void* wt3_dgrad, const float* y_in, const float* a_in, const float* b_in,
                          const float* mean_in, const float* invstd_in, float* g_in, float* stat_part,
                          int B, int Tin, int Ci, int Co, int k, void* stream);
int ign_clconv_dgrad_input_bf16(const float* dyp, const void* wt3_dgrad, float* gx, int B, int Tin, int Ci, int Co, int k,
                                void* stream);
int ign_clconv_wgrad_bf16(const float* dyp, int dy_pad, const float* x, const float* pro_a, const float* pro_b,
                          float* dw_oik, void* workspace, int B, int Tin, int Ci, int Co, int k, void* stream);
/* A Linear layer's weight AND bias gradient in one pass over dy (M, Co) and x (M, Ci): dW = dy^T x on the split-bf16 k = 1 kernel,
 * db = column sums of dy accumulated by the tiles that stage those values anyway (db may be NULL).  Workspace:
 * ign_clconv_wgrad_x6_workspace_bytes(1, M, Ci, Co, 1).  _bf16: the single-product (autocast) form.  Co % 4 == Ci % 4 == 0. */
int ign_linear_wgrad_x6(const float* dy, const float* x, float* dw, float* db, void* workspace, long long M, int Ci, int Co,
                        void* stream);
int ign_linear_wgrad_bf16(const float* dy, const float* x, float* dw, float* db, void* workspace, long long M, int Ci, int Co,
                          void* stream);
size_t ign_clconv_wgrad_workspace_bytes(int B, int Tin, int Ci, int Co, int k);
int ign_clconv_wgrad(const float* dyp, int dy_pad, const float* x, const float* pro_a, const float* pro_b,
                     float* dw_oik, void* workspace, int B, int Tin, int Ci, int Co, int k, void* stream);

/* BatchNorm1d glue of the same expert (IGN/model/FullyConvNet.py:33,40,47; torch.nn.BatchNorm1d semantics: biased batch
 * variance for normalisation, unbiased for running_var, momentum update).  C % 4 == 0, C <= 1024.
 * finalize_fwd: partial sums (nparts, 2, C) over R rows -> a = gamma*invstd, b = beta - a*mean (so BN(y) = a*y + b),
 *   mean, invstd; updates running_mean / running_var in place when they are not NULL.
 * affine_eval: the same a, b, mean, invstd from the running statistics (module.eval()).
 * relu_pool_fwd: pooled[b,c] = mean_t relu(a_c*y[b,t,c] + b_c)            (BatchNorm + ReLU + AdaptiveAvgPool1d(1)).
 * relu_pool_bwd: g[b,t,c] = gpool[b,c]/T * [a_c*y + b_c > 0] and per-block partials (ign_bn_relu_pool_bwd_parts(B,T), 2, C)
 *   of sum g and sum g*yhat (part NULL: the sums are not written -- an input-only backward with running statistics reads none).
 * finalize_bwd: partials -> dbeta = sum g, dgamma = sum g*yhat.
 * bwd_apply: dy = a*(g - (dbeta + yhat*dgamma)/R) [training] or a*g [eval], written into (B, pad + T + pad, C) with the
 *   pad rows zeroed (the layout ign_clconv_dgrad / ign_clconv_wgrad read).                                          */
int ign_bn_finalize_fwd(const float* part, int nparts, long long R, int C, const float* gamma, const float* beta,
                        float eps, float momentum, float* running_mean, float* running_var,
                        float* a, float* b, float* mean, float* invstd, void* stream);
int ign_bn_affine_eval(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                       float eps, int C, float* a, float* b, float* mean, float* invstd, void* stream);
int ign_bn_relu_pool_fwd(const float* y, const float* a, const float* b, float* pooled, int B, int T, int C, void* stream);
/* The same with the FCN expert's class head in the same launch: logits[b][n] = bias[n] + sum_c pooled[b][c] W[n][c]  (W (N,C),
 * bias nullable; replaces nn.Linear at IGN/model/FullyConvNet.py:50,58 on top of the pooling): a sample's pooled row is complete
 * inside its block.  `pooled` is still written (the head's weight gradient needs it: ign_head_bwd).                          */
int ign_bn_relu_pool_head_fwd(const float* y, const float* a, const float* b, float* pooled, const float* W, const float* bias,
                              float* logits, int B, int T, int C, int N, void* stream);
long long ign_bn_relu_pool_bwd_parts(int B, int T);
int ign_bn_relu_pool_bwd(const float* y, const float* gpool, const float* a, const float* b, const float* mean,
                         const float* invstd, float* g, float* part, int B, int T, int C, void* stream);
int ign_bn_finalize_bwd(const float* part, int nparts, int C, float* dbeta, float* dgamma, void* stream);
int ign_bn_bwd_apply(const float* g, const float* y, const float* a, const float* mean, const float* invstd,
                     const float* dbeta, const float* dgamma, float* dyp, int B, int T, int C, int pad, int training,
                     void* stream);

/* Per-kernel HIP-event timing (measurement only; off by default).  When enabled every kernel launch made by
 * this library is bracketed by hipEventRecord on the caller's stream.  ign_timing_read() waits for the recorded
 * events of `label` ("shp_fwd", "shp_bwd", "reduce_parts", "instnorm", "attn_fwd", "attn_bwd_dkdv", "attn_bwd_dq",
 * "attn_delta", "head_fwd", "head_bwd_x", "head_bwd_w", "adam", "adamw", "ema", "swap_flat", "grad_norm", "scale_flat", "gather_acc",
 * "conv1_sumsq_fwd", "conv1_sumsq_bwd", "dwconv1d", "dwconv1d_bwd_w"), and returns the accumulated
 * device milliseconds and launch count since the last enable.  Not for use under graph capture.             */
int ign_timing_enable(int on);
int ign_timing_read(const char* label, double* total_ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif /* IGN_ABI_H */
