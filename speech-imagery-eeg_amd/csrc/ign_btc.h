// What the out-of-place passes over a (B, T, C) training batch share (ign_augment.hip, ign_warp.hip, ign_mix.hip): the checks every
// launcher makes before its own, and the length of a sample as a kernel may use it.
#pragma once
#include "ign_common.h"

// Pointers, dimensions, the 32-bit flat index and the overlap rule; 0, or the error is set under the caller's name.  A block reads
// rows of x that another block writes in out (a shifted row, the two source rows of a warped one, the partner's rows), so ANY
// overlap of the two buffers is a race: refused when |x - out| < B * T * C * 4 bytes.
static inline int ign_btc_check(const char* who, const float* x, const float* out, int B, int T, int C) {
    if (!x || !out || B < 1 || T < 1 || C < 1) {
        ign_set_error("%s: null pointer or non-positive dimension (B=%d T=%d C=%d)", who, B, T, C);
        return IGN_E_ARG;
    }
    const long long TC = (long long)T * C;
    if (TC > 0x7fff0000LL) {
        ign_set_error("%s: T*C=%lld does not fit a 32-bit index", who, TC);
        return IGN_E_TOOBIG;
    }
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out, bytes = (uintptr_t)B * (uintptr_t)TC * sizeof(float);
    if ((xa <= oa ? oa - xa : xa - oa) < bytes) {
        ign_set_error("%s: out of place only (a block reads rows that another block writes): x and out overlap", who);
        return IGN_E_ARG;
    }
    return 0;
}

// B samples of `tiles` blocks each have to fit one grid
static inline int ign_btc_grid_check(const char* who, int B, int T, int C, long long tiles) {
    if ((long long)B * tiles <= 0x7fffffffLL) return 0;
    ign_set_error("%s: B=%d T=%d C=%d needs more blocks than a grid has", who, B, T, C);
    return IGN_E_TOOBIG;
}

static inline bool ign_rate_ok(float r) { return r >= 0.f && r < 1.f; }        // a rate in [0, 1); false for NaN

// The length of sample b in a kernel; device data: clamped, never trusted as an index bound.  A macro, not a __forceinline__
// function: through a function's value parameters the compiler folds the warp kernels' conditions on the length differently
// (two more scalar instructions per block); the expression in place leaves the code of all six kernels as it was.
#define IGN_BTC_LEN(len, b, T) ((len) ? min(max((len)[b], 0), (T)) : (T))
