// Overlap-save FFT convolution of the binaural rendering row (reference
// src/datasets/multi_ch_simulator.py:40-61): split out of lh_render.hip so that it can be compiled WITHOUT the
// vectorisers.  Its complex multiplies become v_pk_mul_f32 / v_pk_fma_f32 with op_sel:[0,1] (src1's halves crossed)
// under SLP — the one packed-fp32 form that returns wrong lanes 48..63 next to matrix-heavy kernels on this chip
// (profiles/r03c_packed_fp32_corruption.txt, lookoncetohear_amd/build.py).
// Below it: the moving-source renderer's kernels — k_fir_moving and k_path_nearest (lh_render_moving, lh_path_nearest), and the
// partitioned overlap-save form for room-length responses, k_bank_spectra and k_moving_fft (lh_bank_spectra, lh_render_moving_fft).
#include "lh_common.h"

namespace lh {

// ------------------------------------------------------------------------------------------------------
// Overlap-save FFT convolution for room-length responses (1024 <= Lh <= 4097): 8192-point complex FFTs in LDS.
//   * both ears in ONE transform pair: x is real, so  ifft( fft(x) . fft(h_L + i h_R) ) = y_L + i y_R ;
//   * the forward transform is decimation-in-frequency (natural in, bit-reversed out), the inverse decimation-in-time
//     (bit-reversed in, natural out) and the spectra are multiplied in bit-reversed order: no reordering pass at all;
//   * a workgroup owns one row (source) and a group of consecutive 4096-sample output blocks: the response's spectrum
//     is computed once, kept in 64 VGPRs per thread (the 32 bins the thread multiplies), and reused for every block;
//   * twiddles exp(-2 pi i k / 8192) are tabulated in LDS once per workgroup (sincospi, ~1 ulp).
// 20 blocks x 2 transforms x 13 x 4096 butterflies per row against 80000 x 4096 x 2 multiply-adds for the direct form
// (~1/16 of the FLOPs); the arithmetic is fp32 with the usual O(eps log F) error, inside the same tolerance.
// ------------------------------------------------------------------------------------------------------
constexpr int FC_LOG = 13, FC_F = 1 << FC_LOG;    // transform size
constexpr int FC_L = FC_F / 2;                    // outputs per block (Lh - 1 <= FC_F - FC_L)
constexpr int FC_PER = FC_F / 256;                // points per thread

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)

// forward, decimation in frequency: natural order in, bit-reversed order out.  Ends with a barrier.
__device__ __forceinline__ void fft_dif(float2* d, const float2* tw, int tid) {
    for (int lg = FC_LOG; lg >= 1; --lg) {
        const int half = 1 << (lg - 1), ts = FC_LOG - lg;        // twiddle index = j << ts
        for (int k = tid; k < FC_F / 2; k += 256) {
            const int j = k & (half - 1), a = ((k >> (lg - 1)) << lg) + j, b = a + half;
            const float2 u = d[a], v = d[b];
            d[a] = make_float2(u.x + v.x, u.y + v.y);
            d[b] = cmul(make_float2(u.x - v.x, u.y - v.y), tw[j << ts]);
        }
        __syncthreads();
    }
}
// inverse (unscaled), decimation in time: bit-reversed order in, natural order out.  Ends with a barrier.
__device__ __forceinline__ void ifft_dit(float2* d, const float2* tw, int tid) {
    for (int lg = 1; lg <= FC_LOG; ++lg) {
        const int half = 1 << (lg - 1), ts = FC_LOG - lg;
        for (int k = tid; k < FC_F / 2; k += 256) {
            const int j = k & (half - 1), a = ((k >> (lg - 1)) << lg) + j, b = a + half;
            const float2 u = d[a], v = cmulc(d[b], tw[j << ts]);
            d[a] = make_float2(u.x + v.x, u.y + v.y);
            d[b] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

// grid (ceil(nblocks / blocks_per_wg), rows); x [rows][N], h [rows][2][Lh], gain [rows], y [rows][2][N]
__global__ void __launch_bounds__(256) k_fft_conv(const float* __restrict__ x, const float* __restrict__ h,
                                                  const float* __restrict__ gain, float* __restrict__ y, int N, int Lh,
                                                  int blocks_per_wg) {
    __shared__ float2 d[FC_F];
    __shared__ float2 tw[FC_F / 2];
    const int tid = threadIdx.x, row = blockIdx.y;
    const int nblocks = (N + FC_L - 1) / FC_L;
    const int q0 = blockIdx.x * blocks_per_wg, q1 = min(q0 + blocks_per_wg, nblocks);
    for (int k = tid; k < FC_F / 2; k += 256) {
        float sn, cs;
        sincospif(-2.0f * (float)k / (float)FC_F, &sn, &cs);
        tw[k] = make_float2(cs, sn);
    }
    const float* hl = h + (long)row * 2 * Lh;
    for (int i = tid; i < FC_F; i += 256) d[i] = i < Lh ? make_float2(hl[i], hl[Lh + i]) : make_float2(0.f, 0.f);
    __syncthreads();
    fft_dif(d, tw, tid);
    float2 W[FC_PER];                                             // spectrum of h_L + i h_R, this thread's bins
#pragma unroll
    for (int j = 0; j < FC_PER; ++j) W[j] = d[tid + 256 * j];
    const float g = gain[row] * (1.0f / FC_F);
    const float* xr = x + (long)row * N;
    float* yl = y + (long)row * 2 * N;
    for (int q = q0; q < q1; ++q) {
        __syncthreads();                                          // previous block's outputs / the W reads are done
        const int lo = q * FC_L - (FC_F - FC_L);                  // segment x[lo .. lo + F)
        for (int i = tid; i < FC_F; i += 256) {
            const int p = lo + i;
            d[i] = make_float2((p >= 0 && p < N) ? xr[p] : 0.f, 0.f);
        }
        __syncthreads();
        fft_dif(d, tw, tid);
#pragma unroll
        for (int j = 0; j < FC_PER; ++j) d[tid + 256 * j] = cmul(d[tid + 256 * j], W[j]);
        __syncthreads();
        ifft_dit(d, tw, tid);
        for (int i = tid; i < FC_L; i += 256) {                   // the last FC_L points of the circular result are linear
            const int n = q * FC_L + i;
            if (n < N) {
                const float2 v = d[FC_F - FC_L + i];
                yl[n] = v.x * g;
                yl[N + n] = v.y * g;
            }
        }
    }
}


int launch_fft_conv(const float* x, const float* h, const float* gain, float* y, int N, int Lh, int rows, hipStream_t st) {
    // 5 output blocks of 4096 samples per workgroup
    const int nblocks = (N + FC_L - 1) / FC_L, bpw = 5;
    hipLaunchKernelGGL(k_fft_conv, dim3((nblocks + bpw - 1) / bpw, rows), dim3(256), 0, st, x, h, gain, y, N, Lh, bpw);
    return check_launch();
}

// ------------------------------------------------------------------------------------------------------
// Moving sources: a time-varying FIR (include/lookonce_hip.h, lh_render_moving).  The arithmetic is the project's OWN
// definition — the reference renders its moving scenes with a native library (`moving_sources.so`, bound by
// src/datasets/motion_simulator.py:30-95) whose source is absent, so nothing here is pinned to it; only the interface
// (one response bank per scene, a path point per frame, add_source / simulate) follows that binding.
//
//   f = n / frame,  w = (float)(n % frame) / (float)frame,  ha = bank[idx[f]][ear],  hb = bank[idx[f + 1]][ear]
//   a = sum_k ha[k] x[n - k],  b = sum_k hb[k] x[n - k]   (each ONE fp32 fmaf chain over k ascending from 0.f: k_fir_causal's)
//   y[n] = fmaf(w, b - a, a) * gain
//
// an output-side cross-fade between the responses of consecutive path points.  It lives in this file, not next to
// k_fir_causal, because this one is compiled without the vectorisers: the library's packed-fp32 budget
// (tests/test_cabi_symbols.py) is spent on the static FIR.
//
// k_fir_moving: one wave = one ear of one segment (at most 512 outputs, 8 per lane) of ONE frame, so both tap sets are
// wave-uniform and load as scalars; frame % 8 == 0 keeps a lane's 8 outputs inside the frame.  A workgroup is four
// waves: two consecutive segments x two ears of one row.  The span of x they need is staged in LDS in stages of MV_KT
// taps (k_fir_causal's padded layout and register sliding window); every staged sample feeds both ears and both chains:
// 8 LDS reads per 128 FMAs.  A frame whose two path points name the same bank entry runs one chain (b - a would be
// exactly 0): a wave-uniform branch, same bits for finite input.  No atomics; every output is written by one lane.
// ------------------------------------------------------------------------------------------------------
constexpr int MV_R = 8;                          // outputs per lane
constexpr int MV_SEG = 64 * MV_R;                // outputs per wave at most: 512
constexpr int MV_OUT = 2 * MV_SEG;               // output extent of a workgroup's two segments: at most 1024
constexpr int MV_KT = 1024;                      // taps per LDS stage (multiple of 2 MV_R)
constexpr int MV_SPAN = MV_OUT + MV_KT + MV_R;   // samples staged per stage

// `TWO`: hb differs from ha.  One stage: taps k0 .. k0 + kend of the chains of this lane's 8 outputs, whose first one sits
// u * 8 samples into the workgroup's extent.
template <bool TWO>
__device__ __forceinline__ void mv_stage(const float* __restrict__ xs, const float* __restrict__ ha, const float* __restrict__ hb,
                                         float (&acc_a)[MV_R], float (&acc_b)[MV_R], int u, int k0, int kend, int Lh) {
    float wa[MV_R], wb[MV_R];
    {
        const float* wp = xs + 9 * (u + MV_KT / 8 + 1);
#pragma unroll
        for (int j = 0; j < MV_R - 1; ++j) wb[j] = wp[j];
        wb[MV_R - 1] = 0.f;
    }
    auto chunk = [&](float (&lo)[MV_R], const float (&hi)[MV_R], int k) {
        const float* wp = xs + 9 * (u + (MV_KT - k) / 8);
#pragma unroll
        for (int j = 0; j < MV_R; ++j) lo[j] = wp[j];
        const int kt0 = k0 + k;
        float ka[MV_R], kb[MV_R];
        if (kt0 + MV_R <= Lh) {                                    // wave-uniform: 32-byte scalar loads
#pragma unroll
            for (int kk = 0; kk < MV_R; ++kk) {
                ka[kk] = ha[kt0 + kk];
                kb[kk] = TWO ? hb[kt0 + kk] : 0.f;
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < MV_R; ++kk) {
                ka[kk] = kt0 + kk < Lh ? ha[kt0 + kk] : 0.f;
                kb[kk] = TWO && kt0 + kk < Lh ? hb[kt0 + kk] : 0.f;
            }
        }
#pragma unroll
        for (int kk = 0; kk < MV_R; ++kk)
#pragma unroll
            for (int r = 0; r < MV_R; ++r) {
                const int i = MV_R - 1 + r - kk;                   // compile-time after unrolling
                const float xv = i >= MV_R ? hi[i - MV_R] : lo[i];
                acc_a[r] = fmaf(ka[kk], xv, acc_a[r]);
                if (TWO) acc_b[r] = fmaf(kb[kk], xv, acc_b[r]);
            }
    };
    for (int k = 0; k < kend; k += 2 * MV_R) {
        chunk(wa, wb, k);
        if (k + MV_R < kend) chunk(wb, wa, k + MV_R);
    }
}

// grid (ceil(segments / 2), B * S1), segments = ceil(N / frame) * spf, spf = ceil(frame / MV_SEG)
// x [B*S1][N], bank [K][P][2][Lh], bank_of [B], idx [B*S1][F], gain [B*S1], y [B*S1][2][N]
__global__ void __launch_bounds__(256) k_fir_moving(const float* __restrict__ x, const float* __restrict__ bank,
                                                    const int* __restrict__ bank_of, const int* __restrict__ idx,
                                                    const float* __restrict__ gain, float* __restrict__ y, int S1, int N, int Lh,
                                                    int P, int K, int F, int frame, int spf) {
    __shared__ float xs[MV_SPAN + MV_SPAN / 8 + 8];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id(tid);
    const int row = blockIdx.y, ear = w & 1;
    // the workgroup's two segments; a segment is part j of frame f: outputs [f frame + j MV_SEG, ... + cnt)
    const int sg0 = blockIdx.x * 2, sg = sg0 + (w >> 1);
    const int n_lo = (sg0 / spf) * frame + (sg0 % spf) * MV_SEG;         // first output of the workgroup (a multiple of 8)
    const int f = sg / spf, j = sg - f * spf;
    const long nw = (long)f * frame + (long)j * MV_SEG;                  // the wave's first output: in [n_lo, n_lo + MV_SEG]
    const int cnt = nw < N ? min(min(MV_SEG, frame - j * MV_SEG), (int)(N - nw)) : 0;      // 0: a wave with nothing to do
    const int u = (cnt ? (int)(nw - n_lo) / MV_R : 0) + lane;            // < 128
    // clamped when read: no argument of the C ABI can make the kernel read outside the bank
    const int bk = min(max(bank_of[row / S1], 0), K - 1);
    const int fa = min(f, F - 2);                                        // (f <= F - 2 for every wave with cnt > 0)
    const int ia = min(max(idx[(long)row * F + fa], 0), P - 1), ib = min(max(idx[(long)row * F + fa + 1], 0), P - 1);
    const float* ha = bank + (((long)bk * P + ia) * 2 + ear) * Lh;
    const float* hb = bank + (((long)bk * P + ib) * 2 + ear) * Lh;
    const bool two = ia != ib;
    const float* xc = x + (long)row * N;
    float acc_a[MV_R], acc_b[MV_R];
#pragma unroll
    for (int r = 0; r < MV_R; ++r) acc_a[r] = acc_b[r] = 0.f;
    // taps beyond the last output only ever meet x[<0] = 0: skip them (per workgroup for the barriers, per wave for the work)
    const int lh_wg = (int)min((long)Lh, (long)n_lo + MV_OUT), lh_w = cnt ? (int)min((long)Lh, nw + cnt) : 0;
    for (int k0 = 0; k0 < lh_wg; k0 += MV_KT) {
        // staged sample i holds x[lo + i], lo = n_lo - k0 - MV_KT - MV_R + 1 (zeros outside [0, N)); this stage's taps reach
        // back to i = MV_KT - (its tap count, rounded up to 8)
        const long lo = (long)n_lo - k0 - MV_KT - MV_R + 1;
        const int i0 = MV_KT - ((min(MV_KT, lh_wg - k0) + MV_R - 1) & ~(MV_R - 1));
        __syncthreads();
        for (int i = i0 + tid; i < MV_SPAN; i += 256) {
            const long p = lo + i;
            xs[i + (i >> 3)] = (p >= 0 && p < N) ? xc[p] : 0.f;
        }
        __syncthreads();
        const int kend = min(MV_KT, lh_w - k0);                          // <= 0: nothing for this wave in this stage
        if (two) mv_stage<true>(xs, ha, hb, acc_a, acc_b, u, k0, kend, Lh);
        else mv_stage<false>(xs, ha, hb, acc_a, acc_b, u, k0, kend, Lh);
    }
    if (lane * MV_R >= cnt) return;
    const float g = gain[row];
    const int m0 = j * MV_SEG + lane * MV_R;                             // position in the frame of the lane's first output
    const float fr = (float)frame;
    float out[MV_R];
#pragma unroll
    for (int r = 0; r < MV_R; ++r) {
        const float a = acc_a[r];
        out[r] = (two ? fmaf((float)(m0 + r) / fr, acc_b[r] - a, a) : a) * g;
    }
    float* yc = y + ((long)row * 2 + ear) * N;
    const long n = nw + lane * MV_R;
    if (n + MV_R <= N && ((N & 3) == 0)) {
        *reinterpret_cast<float4*>(&yc[n]) = make_float4(out[0], out[1], out[2], out[3]);
        *reinterpret_cast<float4*>(&yc[n + 4]) = make_float4(out[4], out[5], out[6], out[7]);
    } else {
#pragma unroll
        for (int r = 0; r < MV_R; ++r)
            if (n + r < N) yc[n + r] = out[r];
    }
}

int launch_fir_moving(const float* x, const float* bank, const int* bank_of, const int* idx, const float* gain, float* y,
                      int rows, int S1, int N, int Lh, int P, int K, int F, int frame, hipStream_t st) {
    const int spf = (frame + MV_SEG - 1) / MV_SEG;
    const long segs = ((long)N + frame - 1) / frame * spf;               // <= N / 8 + spf
    hipLaunchKernelGGL(k_fir_moving, dim3((unsigned)((segs + 1) / 2), rows), dim3(256), 0, st, x, bank, bank_of, idx, gain, y, S1,
                       N, Lh, P, K, F, frame, spf);
    return check_launch();
}

// ------------------------------------------------------------------------------------------------------
// Moving sources at room length (include/lookonce_hip.h, lh_bank_spectra / lh_render_moving_fft): the same definition as
// k_fir_moving, with the two convolutions a and b_ computed by uniformly partitioned overlap-save.  The cross-fade is on the
// OUTPUT side, so for the outputs of frame q the whole response of path point q (and q + 1) applies to all past input:
//     block q = outputs [q frame, (q + 1) frame) = the last `frame` points of  ifft( sum_{j < Q, q - j m >= 0} X[q - j m] . H[e][j] )
//     X[q]    = fft of x[(q + 1) frame - MF_Z, (q + 1) frame)                     (zeros outside [0, N); the row's alone)
//     H[e][j] = fft of (hL + i hR)[j Lp, (j + 1) Lp) / MF_Z, zero-padded           (the bank's alone: lh_bank_spectra)
//     m = max(1, (MF_Z + 1 - frame) / frame),  Lp = m frame  (frame + Lp - 1 <= MF_Z),  Q = ceil(Lh / Lp)
// exact for responses that change from frame to frame: nothing is interpolated in the frequency domain.  As in k_fft_conv both
// ears share one complex transform, the forward transform leaves bit-reversed order, the spectra are multiplied in that order
// and the inverse takes it back; the 1 / MF_Z of the inverse is folded into H (a power of two: exact).
//
// k_moving_fft: a workgroup of 512 threads owns one row and a run of `run` consecutive frames.  It keeps the ring of the last
// ring = (Q - 1) m + 1 block spectra in LDS when ring <= MF_LDS_RING (8 KiB each; 11 at frame 400 / Lh 4096), else in its own
// slice of the caller's `work`, and recomputes the ring - 1 blocks in front of its run first (real input, not zeros).  Per frame:
// all 512 threads transform the new block; then threads 0..255 run chain a and threads 256..511 chain b_ — sum over j ascending
// in ONE fmaf order, each thread 4 bins as two 16-byte loads of X (LDS) and of H (global, re-read by every row: it is served by
// the caches) — and each half inverts its own sum; a frame whose two path points name one entry leaves the second half idle
// (workgroup-uniform; b_ - a would be exactly 0).  Both chains share every X.  No atomics; every output is written by one thread.
// Radix-2 butterflies on float2 in LDS: stages with a span of at least 32 points are conflict-free (a half-wave reads one 256-byte
// row), the five short-span stages are 2-way (two 128-byte runs of a half-wave fall on the same banks).
// ------------------------------------------------------------------------------------------------------
constexpr int MF_LOG = 10, MF_Z = 1 << MF_LOG;   // transform size
constexpr int MF_LDS_RING = 16;                  // block spectra kept in LDS at most: (16 + 2) x 8 KiB + 4 KiB of the CU's 160 KiB
constexpr int MF_RUN = 25;                       // frames per workgroup at least
constexpr int MF_NT = 512;
constexpr int MF_LH_MAX = 16384, MF_FRAME_MAX = 512;

// 1024-point fft_dif / ifft_dit for NT threads (t < NT).  A thread with `on` false only keeps the barriers.
template <int NT>
__device__ __forceinline__ void fft_dif_z(float2* d, const float2* tw, int t, bool on) {
    for (int lg = MF_LOG; lg >= 1; --lg) {
        const int half = 1 << (lg - 1), ts = MF_LOG - lg;
        if (on)
            for (int k = t; k < MF_Z / 2; k += NT) {
                const int j = k & (half - 1), a = ((k >> (lg - 1)) << lg) + j, b = a + half;
                const float2 u = d[a], v = d[b];
                d[a] = make_float2(u.x + v.x, u.y + v.y);
                d[b] = cmul(make_float2(u.x - v.x, u.y - v.y), tw[j << ts]);
            }
        __syncthreads();
    }
}
template <int NT>
__device__ __forceinline__ void ifft_dit_z(float2* d, const float2* tw, int t, bool on) {
    for (int lg = 1; lg <= MF_LOG; ++lg) {
        const int half = 1 << (lg - 1), ts = MF_LOG - lg;
        if (on)
            for (int k = t; k < MF_Z / 2; k += NT) {
                const int j = k & (half - 1), a = ((k >> (lg - 1)) << lg) + j, b = a + half;
                const float2 u = d[a], v = cmulc(d[b], tw[j << ts]);
                d[a] = make_float2(u.x + v.x, u.y + v.y);
                d[b] = make_float2(u.x - v.x, u.y - v.y);
            }
        __syncthreads();
    }
}
__device__ __forceinline__ void mf_twiddles(float2* tw, int tid, int nt) {
    for (int k = tid; k < MF_Z / 2; k += nt) {
        float sn, cs;
        sincospif(-2.0f * (float)k / (float)MF_Z, &sn, &cs);
        tw[k] = make_float2(cs, sn);
    }
}
// acc += x . h on two complex bins; the order of the four fmaf per bin is the definition of the sum's bits
__device__ __forceinline__ void mf_cmac(float4& acc, const float4 x, const float4 h) {
    acc.x = fmaf(x.x, h.x, acc.x);
    acc.x = fmaf(-x.y, h.y, acc.x);
    acc.y = fmaf(x.x, h.y, acc.y);
    acc.y = fmaf(x.y, h.x, acc.y);
    acc.z = fmaf(x.z, h.z, acc.z);
    acc.z = fmaf(-x.w, h.w, acc.z);
    acc.w = fmaf(x.z, h.w, acc.w);
    acc.w = fmaf(x.w, h.z, acc.w);
}

struct MfPlan {
    int m, Lp, Q, ring, run;
};
// the partitioning of include/lookonce_hip.h; frame in [8, MF_FRAME_MAX], Lh in [1, MF_LH_MAX]
inline MfPlan mf_plan(int Lh, int frame) {
    MfPlan p;
    p.m = (MF_Z + 1 - frame) / frame < 1 ? 1 : (MF_Z + 1 - frame) / frame;
    p.Lp = p.m * frame;
    p.Q = (Lh + p.Lp - 1) / p.Lp;
    p.ring = (p.Q - 1) * p.m + 1;                                        // <= 2033
    p.run = 2 * (p.ring - 1) > MF_RUN ? 2 * (p.ring - 1) : MF_RUN;
    return p;
}

// grid (K P Q), block 256: spec[e][j] = fft_dif of (hL + i hR)[j Lp, (j + 1) Lp) / MF_Z of bank entry e = k P + p
__global__ void __launch_bounds__(256) k_bank_spectra(const float* __restrict__ bank, float2* __restrict__ spec, int Lh, int Lp,
                                                      int Q) {
    __shared__ float2 d[MF_Z];
    __shared__ float2 tw[MF_Z / 2];
    const int tid = threadIdx.x;
    const long e = blockIdx.x / Q;
    const int j = blockIdx.x - (int)e * Q;
    mf_twiddles(tw, tid, 256);
    const float* hl = bank + e * 2 * Lh;
    const int k0 = j * Lp, cnt = min(Lp, Lh - k0);
    for (int i = tid; i < MF_Z; i += 256)
        d[i] = i < cnt ? make_float2(hl[k0 + i] * (1.0f / MF_Z), hl[Lh + k0 + i] * (1.0f / MF_Z)) : make_float2(0.f, 0.f);
    __syncthreads();
    fft_dif_z<256>(d, tw, tid, true);
    float2* out = spec + (long)blockIdx.x * MF_Z;
    for (int i = tid; i < MF_Z; i += 256) out[i] = d[i];
}

// grid (ceil(ceil(N / frame) / run), B * S1), block 512, dynamic LDS: tw [512], buf [2][1024], then the ring [ring][1024]
// (LDS_RING) or one staging block [1024].  x [B*S1][N], spec [K][P][Q][1024], idx [B*S1][F], y [B*S1][2][N],
// work [B*S1][gridDim.x][ring][1024] (not LDS_RING)
template <bool LDS_RING>
__global__ void __launch_bounds__(MF_NT) k_moving_fft(const float* __restrict__ x, const float2* __restrict__ spec,
                                                      const int* __restrict__ bank_of, const int* __restrict__ idx,
                                                      const float* __restrict__ gain, float* __restrict__ y, float2* work, int S1,
                                                      int N, int P, int K, int F, int frame, int m, int Q, int ring, int run) {
    HIP_DYNAMIC_SHARED(float4, lds4)
    float2* tw = reinterpret_cast<float2*>(lds4);
    float2* buf = tw + MF_Z / 2;
    float2* st = buf + 2 * MF_Z;
    const int tid = threadIdx.x, row = blockIdx.y, c = tid >> 8, t = tid & 255;
    const int nblk = (N + frame - 1) / frame;
    const int q0 = blockIdx.x * run, q1 = min(q0 + run, nblk);
    float2* rg = LDS_RING ? st : work + ((long)row * gridDim.x + blockIdx.x) * ring * MF_Z;
    mf_twiddles(tw, tid, MF_NT);
    // clamped when read: no argument of the C ABI can make the kernel read outside the image
    const int bk = min(max(bank_of[row / S1], 0), K - 1);
    const float* xr = x + (long)row * N;
    const int* ir = idx + (long)row * F;
    const float g = gain[row], fr = (float)frame;
    float* yl = y + (long)row * 2 * N;
    float2* mine = buf + c * MF_Z;
    for (int q = max(0, q0 - (ring - 1)); q < q1; ++q) {
        float2* slot = rg + (long)(q % ring) * MF_Z;
        float2* d = LDS_RING ? slot : st;
        // (the slot's last readers, block q - 1's sums, and the staging block's copy are behind a barrier)
        const long lo = (long)(q + 1) * frame - MF_Z;
        for (int i = tid; i < MF_Z; i += MF_NT) {
            const long p = lo + i;
            d[i] = make_float2((p >= 0 && p < N) ? xr[p] : 0.f, 0.f);
        }
        __syncthreads();
        fft_dif_z<MF_NT>(d, tw, tid, true);
        if (!LDS_RING) {
            for (int i = tid; i < MF_Z; i += MF_NT) slot[i] = st[i];
            __syncthreads();
        }
        if (q < q0) continue;                                            // a block in front of the run: its spectrum only
        const int fa = min(q, F - 2);                                    // (q <= F - 2: the entry point checks F)
        const int ia = min(max(ir[fa], 0), P - 1), ib = min(max(ir[fa + 1], 0), P - 1);
        const bool two = ia != ib, on = c == 0 || two;
        if (on) {
            const float4* h = reinterpret_cast<const float4*>(spec + (((long)bk * P + (c ? ib : ia)) * Q) * MF_Z);
            float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
            for (int j = 0; j < Q && q - j * m >= 0; ++j) {
                const float4* xs = reinterpret_cast<const float4*>(rg + (long)((q - j * m) % ring) * MF_Z);
                const float4* hj = h + (long)j * (MF_Z / 2);
                mf_cmac(s0, xs[t], hj[t]);
                mf_cmac(s1, xs[t + 256], hj[t + 256]);
            }
            reinterpret_cast<float4*>(mine)[t] = s0;
            reinterpret_cast<float4*>(mine)[t + 256] = s1;
        }
        __syncthreads();
        ifft_dit_z<256>(mine, tw, t, on);
        for (int i = tid; i < frame; i += MF_NT) {
            const long n = (long)q * frame + i;
            if (n < N) {
                const float2 a = buf[MF_Z - frame + i];
                float l = a.x, r = a.y;
                if (two) {
                    const float2 b = buf[2 * MF_Z - frame + i];
                    const float w = (float)i / fr;
                    l = fmaf(w, b.x - a.x, a.x);
                    r = fmaf(w, b.y - a.y, a.y);
                }
                yl[n] = l * g;
                yl[N + n] = r * g;
            }
        }
    }
}

// LH_OK, or LH_ERR_UNSUPPORTED for a frame or a length outside the partitioned path's range
int moving_fft_supported(int Lh, int frame) {
    return (frame % 8 || frame > MF_FRAME_MAX || Lh > MF_LH_MAX) ? LH_ERR_UNSUPPORTED : LH_OK;
}
bool moving_fft_needs_work(int Lh, int frame) { return mf_plan(Lh, frame).ring > MF_LDS_RING; }

int launch_moving_fft(const float* x, const float* spec, const int* bank_of, const int* idx, const float* gain, float* y,
                      float* work, int rows, int S1, int N, int Lh, int P, int K, int F, int frame, hipStream_t st) {
    const MfPlan p = mf_plan(Lh, frame);
    const int nblk = (N + frame - 1) / frame, runs = (nblk + p.run - 1) / p.run;
    const float2* sp = reinterpret_cast<const float2*>(spec);
    if (p.ring <= MF_LDS_RING) {
        const int bytes = (int)sizeof(float2) * (MF_Z / 2 + 2 * MF_Z + p.ring * MF_Z);
        if (bytes > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_moving_fft<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                bytes) != hipSuccess)
            return LH_ERR_LAUNCH;
        hipLaunchKernelGGL(k_moving_fft<true>, dim3(runs, rows), dim3(MF_NT), bytes, st, x, sp, bank_of, idx, gain, y,
                           (float2*)nullptr, S1, N, P, K, F, frame, p.m, p.Q, p.ring, p.run);
    } else {
        const int bytes = (int)sizeof(float2) * (MF_Z / 2 + 2 * MF_Z + MF_Z);
        hipLaunchKernelGGL(k_moving_fft<false>, dim3(runs, rows), dim3(MF_NT), bytes, st, x, sp, bank_of, idx, gain, y,
                           reinterpret_cast<float2*>(work), S1, N, P, K, F, frame, p.m, p.Q, p.ring, p.run);
    }
    return check_launch();
}

// ------------------------------------------------------------------------------------------------------
// k_path_nearest: the bank lookup of the binding's `simulator_add_source(audio, path)` — for every path point v the bank
// position (unit vectors; the scale of v does not matter) with the largest d_j = fmaf(v.z, p.z, fmaf(v.y, p.y, v.x p.x)),
// the LOWEST such j (a strict > while scanning upward).  A zero vector gives 0; a non-finite point some index in [0, P).
// Not hot (about 26 k points x 1250 positions per batch): one thread per point, the positions through LDS in tiles.
// grid (ceil(F / 256), B * S1)
// ------------------------------------------------------------------------------------------------------
constexpr int PN_TILE = 1024;
__global__ void __launch_bounds__(256) k_path_nearest(const float* __restrict__ paths, const float* __restrict__ positions,
                                                      const int* __restrict__ bank_of, int* __restrict__ idx, int S1, int F, int P,
                                                      int K) {
    __shared__ float ps[PN_TILE * 3];
    const int tid = threadIdx.x, row = blockIdx.y, t = blockIdx.x * 256 + tid;
    const int bk = min(max(bank_of[row / S1], 0), K - 1);
    const float* pos = positions + (long)bk * P * 3;
    float vx = 0.f, vy = 0.f, vz = 0.f;
    if (t < F) {
        const float* v = paths + ((long)row * F + t) * 3;
        vx = v[0], vy = v[1], vz = v[2];
    }
    float best = 0.f;
    int arg = 0;
    for (int p0 = 0; p0 < P; p0 += PN_TILE) {
        const int np = min(PN_TILE, P - p0);
        __syncthreads();
        for (int i = tid; i < np * 3; i += 256) ps[i] = pos[(long)p0 * 3 + i];
        __syncthreads();
        for (int q = 0; q < np; ++q) {
            const float d = fmaf(vz, ps[3 * q + 2], fmaf(vy, ps[3 * q + 1], vx * ps[3 * q]));
            if (p0 + q == 0) best = d;
            else if (d > best) best = d, arg = p0 + q;
        }
    }
    if (t < F) idx[(long)row * F + t] = arg;
}

}  // namespace lh

// The bank's partition spectra for lh_render_moving_fft (include/lookonce_hip.h): they depend on bank, Lh and frame only.
extern "C" int lh_bank_spectra(const float* bank, float* spec, int K, int P, int Lh, int frame, lh_stream_t stream) {
    using namespace lh;
    if (!bank || !spec || ((size_t)spec & 15) || K <= 0 || P <= 0 || Lh <= 0 || frame <= 0) return LH_ERR_ARG;
    if (moving_fft_supported(Lh, frame) != LH_OK) return LH_ERR_UNSUPPORTED;
    const MfPlan p = mf_plan(Lh, frame);
    const long blocks = (long)K * P * p.Q;
    if (blocks > 0x7fffffffL) return LH_ERR_ARG;
    hipLaunchKernelGGL(k_bank_spectra, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bank,
                       reinterpret_cast<float2*>(spec), Lh, p.Lp, p.Q);
    return check_launch();
}

// Bank lookup for lh_render_moving (include/lookonce_hip.h).
extern "C" int lh_path_nearest(const float* paths, const float* positions, const int* bank_of, int* idx, int B, int S1, int F,
                               int P, int K, lh_stream_t stream) {
    using namespace lh;
    if (!paths || !positions || !bank_of || !idx || B <= 0 || S1 <= 0 || F <= 0 || P <= 0 || K <= 0 || (long)B * S1 > 65535)
        return LH_ERR_ARG;
    hipLaunchKernelGGL(k_path_nearest, dim3((F + 255) / 256, B * S1), dim3(256), 0, (hipStream_t)stream, paths, positions, bank_of,
                       idx, S1, F, P, K);
    return check_launch();
}
