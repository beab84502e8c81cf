// On-device evaluation metrics of the reference test loop (reference src/ts_hear_test.py:139-146): per utterance
// SI-SNR(output, target) and SI-SNRi = SI-SNR(output, target) - SI-SNR(mixture, target), averaged over the two
// channels, plus the cosine similarity of the enrollment embedding — so a sharded eval moves 32 bytes per rank
// instead of copying [B, 2, 80000] waveforms to the host.
//
// torchmetrics' scale_invariant_signal_noise_ratio = zero-mean SI-SDR:
//     alpha = (<p,t> + eps) / (<t,t> + eps);  10 log10((|alpha t|^2 + eps) / (|alpha t - p|^2 + eps)),  eps = fp32 eps
// on mean-removed p, t.  The moments are accumulated in fp64 (the noise energy is a difference of nearly equal
// sums), streamed once: 3 waveforms in, 8 doubles per (utterance, channel, chunk) out.
#include "lh_common.h"

namespace lh {

constexpr int MT_CHUNKS = 16;     // workgroups per (utterance, channel)
constexpr int MT_NM = 8;          // sum p, t, m, pp, tt, mm, pt, mt

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (MT_CHUNKS, B*2), block 256
__global__ void __launch_bounds__(256) k_metric_moments(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                        const float* __restrict__ mix, double* __restrict__ part, int n) {
    __shared__ double red[4][MT_NM];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid);
    const long base = (long)blockIdx.y * n;
    const int per = ((n + MT_CHUNKS - 1) / MT_CHUNKS + 3) & ~3;
    const int lo = blockIdx.x * per, hi = min(n, lo + per);
    double s[MT_NM];
#pragma unroll
    for (int k = 0; k < MT_NM; ++k) s[k] = 0.0;
    const bool vec = ((base | lo) & 3) == 0;
    for (int i = lo + tid * 4; i < hi; i += 256 * 4) {
        float p[4], t[4], m[4];
        if (vec && i + 3 < hi) {
            const float4 p4 = *reinterpret_cast<const float4*>(&pred[base + i]);
            const float4 t4 = *reinterpret_cast<const float4*>(&tgt[base + i]);
            const float4 m4 = *reinterpret_cast<const float4*>(&mix[base + i]);
            p[0] = p4.x; p[1] = p4.y; p[2] = p4.z; p[3] = p4.w;
            t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
            m[0] = m4.x; m[1] = m4.y; m[2] = m4.z; m[3] = m4.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = i + j < hi;
                p[j] = ok ? pred[base + i + j] : 0.f;
                t[j] = ok ? tgt[base + i + j] : 0.f;
                m[j] = ok ? mix[base + i + j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double pd = p[j], td = t[j], md = m[j];
            s[0] += pd; s[1] += td; s[2] += md;
            s[3] += pd * pd; s[4] += td * td; s[5] += md * md;
            s[6] += pd * td; s[7] += md * td;
        }
    }
#pragma unroll
    for (int k = 0; k < MT_NM; ++k) {
        const double v = wave_sum_f64(s[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < MT_NM)
        part[((long)blockIdx.y * MT_CHUNKS + blockIdx.x) * MT_NM + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

__device__ __forceinline__ double si_snr_from_moments(double sp, double st, double spp, double stt, double spt, double n) {
    const double eps = 1.1920928955078125e-07;                // torch.finfo(float32).eps
    const double mp = sp / n, mt = st / n;
    const double pt = spt - n * mp * mt, tt = stt - n * mt * mt, pp = spp - n * mp * mp;
    const double alpha = (pt + eps) / (tt + eps);
    const double sig = alpha * alpha * tt;
    const double noise = sig - 2.0 * alpha * pt + pp;
    return 10.0 * log10((sig + eps) / (fmax(noise, 0.0) + eps));
}

// per-utterance rows [B][3] = (output_sisnr, si_snr_i, embedding_sim).  One wave per utterance, four utterances per
// workgroup, grid ceil(B / 4): lanes 0..15 add up the 16 chunk partials of their (channel, moment), all 64 lanes share the
// cosine similarity.  (Rounds 1-4 ran ONE workgroup whose four waves walked B / 4 utterances each — four software fp64
// log10 chains per utterance back to back: 57 us per call at B = 32, 0.8 % of the batch-32 step for 96 numbers.)
__global__ void __launch_bounds__(256) k_metric_finish(const double* __restrict__ part, const float* __restrict__ emb,
                                                       const float* __restrict__ emb_gt, float* __restrict__ rows,
                                                       int B, int n, int edim) {
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid);
    double* rows64 = const_cast<double*>(part) + (long)B * 2 * MT_CHUNKS * MT_NM;     // [B][3] tail of the scratch
    const int b = blockIdx.x * 4 + wave;
    if (b >= B) return;
    double m = 0.0;                                           // lane = ch * 8 + k (< 16): moment k of channel ch
    if (lane < 2 * MT_NM) {
        double pc[MT_CHUNKS];
#pragma unroll
        for (int c = 0; c < MT_CHUNKS; ++c) pc[c] = part[(((long)b * 2 + (lane >> 3)) * MT_CHUNKS + c) * MT_NM + (lane & 7)];
#pragma unroll
        for (int c = 0; c < MT_CHUNKS; ++c) m += pc[c];       // chunk order: the sum does not depend on the launch shape
    }
    double out_sisnr = 0.0, snr_i = 0.0;
    for (int ch = 0; ch < 2; ++ch) {
        double mm[MT_NM];
#pragma unroll
        for (int k = 0; k < MT_NM; ++k) mm[k] = __shfl(m, ch * MT_NM + k);
        const double so = si_snr_from_moments(mm[0], mm[1], mm[3], mm[4], mm[6], (double)n);
        const double sm = si_snr_from_moments(mm[2], mm[1], mm[5], mm[4], mm[7], (double)n);
        out_sisnr += 0.5 * so;
        snr_i += 0.5 * (so - sm);
    }
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int i = lane; i < edim; i += 64) {
        const double x = emb[(long)b * edim + i], yv = emb_gt[(long)b * edim + i];
        ab += x * yv; aa += x * x; bb += yv * yv;
    }
    ab = wave_sum_f64(ab); aa = wave_sum_f64(aa); bb = wave_sum_f64(bb);
    const double cosv = ab / (fmax(sqrt(aa), 1e-8) * fmax(sqrt(bb), 1e-8));         // F.cosine_similarity, eps 1e-8
    if (lane == 0) {
        rows[b * 3 + 0] = (float)out_sisnr;
        rows[b * 3 + 1] = (float)snr_i;
        rows[b * 3 + 2] = (float)cosv;
        rows64[b * 3 + 0] = snr_i; rows64[b * 3 + 1] = out_sisnr; rows64[b * 3 + 2] = cosv;
    }
}

// sums[4] (fp64) = [sum si_snr_i, sum output_sisnr, sum embedding_sim, B]: one wave, lane k adds column k of the fp64 rows in
// utterance order (sequential: bit-reproducible, and the same order as the single-thread loop of rounds 1-4)
__global__ void __launch_bounds__(64) k_metric_total(const double* __restrict__ part, double* __restrict__ sums, int B) {
    const double* rows64 = part + (long)B * 2 * MT_CHUNKS * MT_NM;
    const int k = threadIdx.x;
    if (k < 3) {
        double a = 0.0;
        for (int b = 0; b < B; ++b) a += rows64[b * 3 + k];
        sums[k] = a;
    } else if (k == 3) {
        sums[3] = (double)B;
    }
}


// ---- binaural cue errors (reference src/eval/binaural.py: itd_diff, ild_diff, chunk_and_mask) ------------------------------
// Per segment and signal (est, gt): the circular cross-correlation cc[tau] = sum_m L[(m + tau) mod len] R[m] over the lags
// -BC_TMAX..BC_TMAX and the channel energies, as DIRECT fp64 sums (the reference goes through rfft / irfft; a product of two
// fp32 samples is exact in fp64, so every term is exact and only the additions round).  A segment is the whole clip (static
// mode) or a frame of `frame` samples, the last one zero-padded (moving mode).
//   k_bc_tiles     grid (tiles, segments, B): one workgroup per BC_TILE positions of a segment.  Lane l owns the BC_RUN
//                  positions m0 = tile * BC_TILE + l * BC_RUN ..; it reads its BC_RUN right samples once and a window of
//                  BC_RUN + 2 BC_TMAX left samples (the halo read modulo the segment length), then every (sample, lag) pair
//                  is one fp64 FMA on registers.  Partials: [B][C][tiles][est, gt][BC_NV] (lags, sum L^2, sum R^2, 0).
//   k_bc_segments  grid (segments, B): adds the tile partials in tile order; argmax |cc| (first maximum wins, as np.argmax),
//                  ILD, ITD and the gt-RMS mask of the segment -> record [B][C][BC_REC].
//   k_bc_rows      one wave per utterance: the counted segments' aggregate (mean |dITD|, |mean ILD_est - mean ILD_gt|).
//   k_bc_total     the all-reduce payload: sums and counts of the finite rows, in utterance order.
// Fixed reduction orders throughout and no atomics: bit-identical from run to run, and row b depends on utterance b only.
constexpr int BC_TMAX = 16;                       // largest supported round(1e-3 sr): sr <= 16499
constexpr int BC_LAGS = 2 * BC_TMAX + 1;
constexpr int BC_RUN = 16;                        // positions per lane
constexpr int BC_TILE = 256 * BC_RUN;
constexpr int BC_NV = BC_LAGS + 3;                // lags, sum L^2, sum R^2, pad
constexpr int BC_REC = 8;                         // tau_est, tau_gt, ild_est, ild_gt, itd_est, itd_gt, counted, 0

__device__ __forceinline__ int bc_wrap(int p, int len) {
    p %= len;
    return p < 0 ? p + len : p;
}

// grid (tiles, C, B), block 256
__global__ void __launch_bounds__(256) k_bc_tiles(const float* __restrict__ est, const float* __restrict__ gt,
                                                  double* __restrict__ part, int n, int seglen) {
    __shared__ double red[4][2 * BC_NV];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid);
    const int t = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int seg0 = c * seglen;
    const int valid = min(seglen, n - seg0);                  // positions >= valid are the zero padding of the last frame
    const int tend = min(seglen, (t + 1) * BC_TILE);
    const int m0 = t * BC_TILE + tid * BC_RUN;
    for (int sig = 0; sig < 2; ++sig) {
        const float* xl = (sig ? gt : est) + (long)b * 2 * n + seg0;
        const float* xr = xl + n;
        double acc[BC_LAGS + 2];
#pragma unroll
        for (int k = 0; k < BC_LAGS + 2; ++k) acc[k] = 0.0;
        if (m0 < tend) {
            float l[BC_RUN + 2 * BC_TMAX];
            double r[BC_RUN];
            if (m0 >= BC_TMAX && m0 + BC_RUN + BC_TMAX <= valid) {        // interior: no wrap, no padding, whole run
#pragma unroll
                for (int k = 0; k < BC_RUN + 2 * BC_TMAX; ++k) l[k] = xl[m0 - BC_TMAX + k];
#pragma unroll
                for (int j = 0; j < BC_RUN; ++j) r[j] = xr[m0 + j];
            } else {                                                      // circular halo, padding, end of the segment
#pragma unroll
                for (int k = 0; k < BC_RUN + 2 * BC_TMAX; ++k) {
                    const int p = bc_wrap(m0 - BC_TMAX + k, seglen);
                    l[k] = p < valid ? xl[p] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < BC_RUN; ++j) r[j] = (m0 + j < tend && m0 + j < valid) ? xr[m0 + j] : 0.f;
            }
            // left sample q meets right sample j at lag q - j - BC_TMAX: each left value is widened once and used while it is
            // live (acc[k] still takes its terms in increasing j)
#pragma unroll
            for (int q = 0; q < BC_RUN + 2 * BC_TMAX; ++q) {
                const double lq = l[q];
                if (q >= BC_TMAX && q < BC_TMAX + BC_RUN && m0 + q - BC_TMAX < tend) acc[BC_LAGS] = fma(lq, lq, acc[BC_LAGS]);
#pragma unroll
                for (int j = q > 2 * BC_TMAX ? q - 2 * BC_TMAX : 0; j <= (q < BC_RUN - 1 ? q : BC_RUN - 1); ++j)
                    acc[q - j] = fma(lq, r[j], acc[q - j]);
            }
#pragma unroll
            for (int j = 0; j < BC_RUN; ++j) acc[BC_LAGS + 1] = fma(r[j], r[j], acc[BC_LAGS + 1]);
        }
#pragma unroll
        for (int k = 0; k < BC_LAGS + 2; ++k) {
            const double v = wave_sum_f64(acc[k]);
            if (lane == 0) red[wave][sig * BC_NV + k] = v;
        }
    }
    __syncthreads();
    if (tid < 2 * BC_NV) {
        const int k = tid % BC_NV;
        const double v = k < BC_LAGS + 2 ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.0;
        part[(((long)b * gridDim.y + c) * gridDim.x + t) * 2 * BC_NV + tid] = v;
    }
}

// grid (C, B), block 128
__global__ void __launch_bounds__(128) k_bc_segments(const double* __restrict__ part, double* __restrict__ rec, int tiles,
                                                     int tmax, int sr, int frame, double rms_threshold) {
    __shared__ double sv[2 * BC_NV];
    const int tid = threadIdx.x, c = blockIdx.x, b = blockIdx.y, C = gridDim.x;
    const double* p = part + ((long)b * C + c) * tiles * 2 * BC_NV;
    if (tid < 2 * BC_NV) {
        double v = 0.0;
        for (int t = 0; t < tiles; ++t) v += p[(long)t * 2 * BC_NV + tid];          // tile order
        sv[tid] = v;
    }
    __syncthreads();
    double* r = rec + ((long)b * C + c) * BC_REC;
    if (tid < 2) {
        const double* s = sv + tid * BC_NV;
        int arg = BC_TMAX - tmax;                                 // tau = -tmax .. tmax in that order, first maximum wins
        double best = fabs(s[arg]);
        for (int k = arg + 1; k <= BC_TMAX + tmax; ++k) {
            const double a = fabs(s[k]);
            if (best == best && (a != a || a > best)) { best = a; arg = k; }    // np.argmax: the first NaN is the maximum
        }
        const double tau = (double)(arg - BC_TMAX);
        r[tid] = tau;
        r[2 + tid] = 10.0 * log10(s[BC_LAGS] / s[BC_LAGS + 1]);
        r[4 + tid] = tau / (double)sr * 1e6;
    } else if (tid == 2) {
        double counted = 1.0;                                     // static mode: every clip counts
        if (frame > 0) {                                          // max over channels of the gt RMS (NaN propagates, as np.max)
            const double a = sqrt(sv[BC_NV + BC_LAGS] / (double)frame), g = sqrt(sv[BC_NV + BC_LAGS + 1] / (double)frame);
            const double m = (a != a || a >= g) ? a : g;
            counted = m >= rms_threshold ? 1.0 : 0.0;
        }
        r[6] = counted;
        r[7] = 0.0;
    }
}

// rows [B][2] = (delta_itd_us, delta_ild_db).  One wave per utterance, four per workgroup, grid ceil(B / 4)
__global__ void __launch_bounds__(256) k_bc_rows(const double* __restrict__ rec, double* __restrict__ rows, int B, int C) {
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x * 4 + wave_id(tid);
    if (b >= B) return;
    double ditd = 0.0, cnt = 0.0, ild_e = 0.0, ild_g = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double* r = rec + ((long)b * C + c) * BC_REC;
        if (r[6] != 0.0) {
            ditd += fabs(r[4] - r[5]);
            cnt += 1.0;
            ild_e += r[2];
            ild_g += r[3];
        }
    }
    ditd = wave_sum_f64(ditd); cnt = wave_sum_f64(cnt); ild_e = wave_sum_f64(ild_e); ild_g = wave_sum_f64(ild_g);
    if (lane == 0) {
        const double nan = __builtin_nan("");                     // np.mean of no counted segment
        rows[b * 2 + 0] = cnt > 0.0 ? ditd / cnt : nan;
        rows[b * 2 + 1] = cnt > 0.0 ? fabs(ild_e / cnt - ild_g / cnt) : nan;
    }
}

// sums [4] = (sum delta_itd over finite rows, count, sum delta_ild over finite rows, count); lane k walks column k in order
__global__ void __launch_bounds__(64) k_bc_total(const double* __restrict__ rows, double* __restrict__ sums, int B) {
    const int k = threadIdx.x;
    if (k < 2) {
        double s = 0.0, cnt = 0.0;
        for (int b = 0; b < B; ++b) {
            const double v = rows[b * 2 + k];
            if (v - v == 0.0) { s += v; cnt += 1.0; }              // finite: inf - inf and NaN - NaN are NaN
        }
        sums[2 * k] = s;
        sums[2 * k + 1] = cnt;
    }
}

}  // namespace lh

extern "C" int lh_metric_sums(const float* outputs, const float* target, const float* mixture, const float* emb,
                              const float* emb_gt, double* scratch, float* rows, double* sums, int B, int n_samples,
                              int emb_dim, lh_stream_t stream) {
    using namespace lh;
    if (!outputs || !target || !mixture || !emb || !emb_gt || !scratch || !rows || !sums || B <= 0 || n_samples <= 0 ||
        emb_dim <= 0)
        return LH_ERR_ARG;
    hipLaunchKernelGGL(k_metric_moments, dim3(MT_CHUNKS, B * 2), dim3(256), 0, (hipStream_t)stream, outputs, target,
                       mixture, scratch, n_samples);
    hipLaunchKernelGGL(k_metric_finish, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, scratch, emb, emb_gt, rows, B,
                       n_samples, emb_dim);
    hipLaunchKernelGGL(k_metric_total, dim3(1), dim3(64), 0, (hipStream_t)stream, scratch, sums, B);
    return check_launch();
}

extern "C" int lh_binaural_cues(const float* est, const float* gt, double* scratch, double* rows, double* sums, int B,
                                int n_samples, int sr, int frame, double rms_threshold, lh_stream_t stream) {
    using namespace lh;
    if (!est || !gt || !scratch || !rows || !sums || B <= 0 || n_samples <= 0 || sr <= 0 || frame < 0) return LH_ERR_ARG;
    const int tmax = (int)rint(1e-3 * sr);                       // Python round(): ties to even
    if (tmax < 1 || tmax > BC_TMAX || (frame == 0 && (n_samples & 1)) || (frame & 1)) return LH_ERR_UNSUPPORTED;
    const int seglen = frame > 0 ? frame : n_samples;
    const int C = frame > 0 ? (n_samples + frame - 1) / frame : 1;
    const int tiles = (seglen + BC_TILE - 1) / BC_TILE;
    const int te = min(tmax, seglen / 2);                         // compute_itd: t_max is capped at len // 2
    double* part = scratch;
    double* rec = scratch + (long)B * C * tiles * 2 * BC_NV;
    hipLaunchKernelGGL(k_bc_tiles, dim3(tiles, C, B), dim3(256), 0, (hipStream_t)stream, est, gt, part, n_samples, seglen);
    hipLaunchKernelGGL(k_bc_segments, dim3(C, B), dim3(128), 0, (hipStream_t)stream, part, rec, tiles, te, sr, frame,
                       rms_threshold);
    hipLaunchKernelGGL(k_bc_rows, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, rec, rows, B, C);
    hipLaunchKernelGGL(k_bc_total, dim3(1), dim3(64), 0, (hipStream_t)stream, rows, sums, B);
    return check_launch();
}
