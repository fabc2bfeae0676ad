// The per-step learning-rate schedule and the EMA decay warm-up: ONE rule for the scheduled tick kernel (ign_optim.hip, on the
// device) and for ign_sched_lr (on the host, for logging and tests); restated in numpy float64 in utils/optim_rule.py.
//
//   s = 1, 2, ... the optimizer step; W warm-up steps, M the floor, S the run's total number of optimizer steps
//   s <  W             lr = base * s / W
//   constant, s >= W   lr = base
//   cosine,   s >= W   lr = M + (base - M) * 0.5 * (1 + cos(pi * t / T)),  t = min(s - W, T),  T = max(1, S - W)
//                      (CosineAnnealingLR's closed form: lr(W) = base, lr(S) = M)
//   EMA decay          d = min(D, (1 + s) / (10 + s))
// Everything in double, rounded to float once.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IGN_SCHED_HD __host__ __device__
#else
#define IGN_SCHED_HD
#endif

enum { IGN_SCHED_CONSTANT = 0, IGN_SCHED_COSINE = 1 };

IGN_SCHED_HD inline bool ign_sched_valid(int kind, double base, long long warmup, double min_lr, long long total) {
    return (kind == IGN_SCHED_CONSTANT || kind == IGN_SCHED_COSINE) && base >= 0.0 && warmup >= 0 && total >= 0 && min_lr >= 0.0 &&
           min_lr <= base;                                     // false for a NaN as well
}

IGN_SCHED_HD inline float ign_sched_lr_at(int kind, double base, long long warmup, double min_lr, long long total, long long s) {
    double lr = base;
    if (s < warmup) {
        lr = base * (double)s / (double)warmup;
    } else if (kind == IGN_SCHED_COSINE) {
        const long long T = total - warmup > 1 ? total - warmup : 1;
        const long long t = s - warmup < T ? s - warmup : T;
        lr = min_lr + (base - min_lr) * 0.5 * (1.0 + cos(3.14159265358979323846 * (double)t / (double)T));
    }
    return (float)lr;
}

IGN_SCHED_HD inline float ign_ema_decay_at(double decay, long long s) {
    const double warm = (1.0 + (double)s) / (10.0 + (double)s);
    return (float)(decay < warm ? decay : warm);
}
