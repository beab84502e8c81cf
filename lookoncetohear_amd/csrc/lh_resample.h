// Polyphase sinc resampling (include/lookonce_hip.h, ABI 23): the ONE inner product of lh_resample (lh_render.hip) and of the
// session nodes lh_session_resample_in / lh_session_resample_out / lh_session_resample_out_any (lh_stream.hip).
//
// With g = gcd(orig, new), o = orig / g, n = new / g, K = 2 width + o, output block q and phase p:
//     y[q n + p] = sum_{k < K} xpad[q o + k] * bank[p][k]          xpad = width zeros, x, zeros
// (the `sinc_interp_hann` bank of lookoncetohear_amd/resample.py, made in fp64 on the host and cast to fp32).
// One accumulation order everywhere: a single fp32 accumulator that starts at +0, one fmaf per tap, taps in ascending k, no
// tap skipped.  A kernel only chooses WHERE tap k comes from (LDS, a ring, a zero outside the signal), never the arithmetic,
// so a stream resampled in packets of any size carries the bits of the stream resampled in one piece.
#pragma once
#include "lh_common.h"

namespace lh {

constexpr int RS_MAX_RATIO = 4096;             // o and n
constexpr int RS_SPAN = 8192;                  // input samples a workgroup of k_resample stages (32 KiB of LDS)

// the tap sources: `x[k]` for a staged span, `ring[(c + k) & mask]` for a per-slot ring addressed by a sample counter
struct TapSpan {
    const float* x;
    __device__ __forceinline__ float operator()(int k) const { return x[k]; }
};
struct TapRing {
    const float* ring;
    unsigned c, mask;
    __device__ __forceinline__ float operator()(int k) const { return ring[(c + (unsigned)k) & mask]; }
};

template <class Tap>
__device__ __forceinline__ float resample_dot(const Tap tap, const float* __restrict__ row, int K) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(tap(k), row[k], acc);
    return acc;
}

// The same chain twice, for the two channels of one output, against a column of the transposed image bankT[K][n] (`col` =
// bankT + p): tap k of phase p lies at col[k n], so the 64 consecutive phases of a wave read 64 consecutive floats.
template <class Tap>
__device__ __forceinline__ void resample_dot2_t(const Tap tap0, const Tap tap1, const float* __restrict__ col, int n, int K,
                                                float& y0, float& y1) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll 16                              // 16 bank loads in flight per wave: the loop is bound by their latency, not by the fmaf
    for (int k = 0; k < K; ++k) {
        const float b = col[(long)k * n];
        a0 = fmaf(tap0(k), b, a0);
        a1 = fmaf(tap1(k), b, a1);
    }
    y0 = a0;
    y1 = a1;
}

// what every entry point accepts: the tile of k_resample must hold one block's taps
inline bool resample_ratio_ok(int o, int n, int width) {
    return o >= 1 && o <= RS_MAX_RATIO && n >= 1 && n <= RS_MAX_RATIO && width >= 1 && (long)o + 2L * width + 8 <= RS_SPAN;
}

}  // namespace lh
