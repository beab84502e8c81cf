// Pointwise (per time-frequency unit) channel contractions with fused epilogues:
//   k_linear_res   out = res + W h + b                            (intra_linear / inter_linear + residual)
//   k_qkv_proj_ln  Q/K/V = LN_(f,e)(PReLU(W y + b)) per head       (attn_conv_Q/K/V)
//   k_proj_ln_res  out = (y2 + LN_(f,c)(PReLU(W m + b))) * gain    (attn_concat_proj + residual + speaker gain)
//                  TAPS (last block): P = out . Wd, the 36 deconv tap products per (frame, bin), instead of `out`
//
// These are HBM-streaming stages: every activation byte should cross HBM once per stage, so
//   * workgroups are persistent (grid-stride over row tiles / frames) and keep their weights in VGPRs;
//   * global loads of a tile are all issued before the first dependent LDS write (register staging; hipcc does
//     not unroll a load->ds_write loop by itself and otherwise serialises one HBM round trip per float4), and the
//     next frame is prefetched into registers while the current one is processed;
//   * the contraction runs on split-precision fp16 MFMA ("f16x3": v = hi + lo, products hi*hi + hi*lo + lo*hi on
//     v_mfma_f32_16x16x32_f16 into one accumulator, ~22 mantissa bits, lh_split.h) so the matrix pipe costs
//     ~1/5 of fp32 MFMA;
//   * each WAVE owns output-column tiles (not row tiles): its weight fragments are 16-32 registers instead of
//     112-128, which keeps 2-3 workgroups resident per CU for latency hiding;
//   * LayerNorm / PReLU / residual epilogues run out of LDS with compile-time index algebra.
#include "lh_split.h"
#include <type_traits>

namespace lh {

// ------------------------------------------------------------------------------------------------------
// out[r][0:64] = res[r][0:64] + bias + sum_k h[r][k] * W[o][k]       K in {64, 128}; 64-row tiles
// ------------------------------------------------------------------------------------------------------
template <int K>
__global__ void __launch_bounds__(256) k_linear_res(const float* __restrict__ h, const _Float16* __restrict__ w_pk,
                                                    const float* __restrict__ bias, const float* __restrict__ res,
                                                    float* __restrict__ out, int rows, int seg, long segstride) {
    // rows come in segments of `seg` consecutive rows, segment g starting at row g * segstride (time windows, lh_linear_res_win:
    // seg = Tc * 97 rows of one utterance, segstride = T * 97); the plain call is ONE segment (seg = rows)
    auto grow = [&](long r) -> long { return (r / seg) * segstride + r % seg; };
    constexpr int KS = K / 32, RP = 64, CP = C + 4;
    __shared__ __attribute__((aligned(16))) _Float16 ahi[KS * 4 * RP * 8];
    __shared__ __attribute__((aligned(16))) _Float16 alo[KS * 4 * RP * 8];
    __shared__ __attribute__((aligned(16))) float cs[RP * CP];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid), g4 = lane >> 4, l15 = lane & 15;

    f16x8 wh[KS], wl[KS];
    load_w<KS>(w_pk, wave, lane, wh, wl);              // wave w owns output columns 16w .. 16w+15
    const float bz = bias[wave * 16 + l15];

    const int ntiles = (rows + RP - 1) / RP;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long r0 = (long)tile * RP;
        constexpr int NLD = RP * (K / 4) / 256;
        float4 stg[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) {                // all global loads of the tile in flight
            const int e = tid + 256 * i;
            const long r = grow(min(r0 + e / (K / 4), (long)rows - 1));
            stg[i] = *reinterpret_cast<const float4*>(&h[r * K + (e % (K / 4)) * 4]);
        }
        // residual rows: issue the loads now, they land while the MFMAs run
        float4 rv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const long r = grow(min(r0 + (e >> 4), (long)rows - 1));
            rv[i] = *reinterpret_cast<const float4*>(&res[r * C + (e & 15) * 4]);
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 256 * i;
            store_split4<RP>(ahi, alo, e / (K / 4), (e % (K / 4)) * 4, stg[i]);
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < RP / 16; ++m) {
            const f32x4 acc = mma_tile<RP, KS>(ahi, alo, m, g4, l15, wh, wl, bz);
#pragma unroll
            for (int r = 0; r < 4; ++r) cs[(m * 16 + g4 * 4 + r) * CP + wave * 16 + l15] = acc[r];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, rr = e >> 4, qq = e & 15;
            const long r = r0 + rr;
            if (r < rows) {
                const float4 cv = *reinterpret_cast<const float4*>(&cs[rr * CP + qq * 4]);
                *reinterpret_cast<float4*>(&out[grow(r) * C + qq * 4]) =
                    make_float4(cv.x + rv[i].x, cv.y + rv[i].y, cv.z + rv[i].z, cv.w + rv[i].w);
            }
        }
        // the next tile's staging barrier orders these cs reads before cs is rewritten
    }
}

// Per-head LayerNorm + split-precision store, one wave per head (N values held flat, index i = f*D + e = the
// reference's reshape order, in LDS at ysrc[0 .. 4*NQ); entries >= N are zero; gw / gb are zero-padded to 4*NQ so
// pad outputs are exactly 0).  Round 5: a lane owns QUADS lane + 64 k (rounds 1-4: octets — 76 and 194 octets on 64
// lanes left 34 % of the slots dead, and this phase is 60 % of the VALU-bound kernel's vector instructions; 152 and 388
// quads leave 18 %); out-of-range slots are clamped to the last quad (the code stays branch-free so the affine loads of
// later slots are issued under the arithmetic of earlier ones) and only their statistics contributions and stores are
// masked.  Output formats (lh_common.h):
//   VLAYOUT = 0 (Q / K rows):  quad qd of octet o = qd >> 1 -> hi 4 at [16 o + 4 (qd & 1)], lo 4 eight halves behind
//   VLAYOUT = 1 (V rows):      quad qd -> [hi 4 | lo 4] at [8 qd]
template <int N, int NQ>
struct HeadLN {
    static constexpr int NS = (NQ + 63) / 64;
    float x[NS][4];
    float4 w[NS], b[NS];

    __device__ __forceinline__ static int quad(int lane, int k) { return min(lane + 64 * k, NQ - 1); }
    __device__ __forceinline__ static bool live(int lane, int k) { return 64 * k + 63 < NQ || lane + 64 * k < NQ; }
    // slot k holds only values of the row (no pad, no dead lane): its statistics need no mask
    static constexpr bool inside(int k) { return 4 * (64 * k + 63) + 3 < N; }

    // LDS -> registers; returns the lane's partial sum.  `zero4` = 4 floats of zeros in LDS (16-byte aligned): slots past
    // the row read those instead, so nothing has to be masked out of the sum.
    __device__ __forceinline__ float read(const float* ysrc, const float* zero4, int lane) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const float* src = live(lane, k) ? ysrc + 4 * (lane + 64 * k) : zero4;
            const float4 a = *reinterpret_cast<const float4*>(src);
            x[k][0] = a.x; x[k][1] = a.y; x[k][2] = a.z; x[k][3] = a.w;
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NS; ++k) s += (x[k][0] + x[k][1]) + (x[k][2] + x[k][3]);
        return s;
    }
    __device__ __forceinline__ void load_affine(const float* __restrict__ gw, const float* __restrict__ gb, int lane) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int o = quad(lane, k);
            w[k] = *reinterpret_cast<const float4*>(&gw[4 * o]);
            b[k] = *reinterpret_cast<const float4*>(&gb[4 * o]);
        }
    }
    __device__ __forceinline__ void set_affine(const HeadLN& o) {               // affine held by the caller across frames
#pragma unroll
        for (int k = 0; k < NS; ++k) { w[k] = o.w[k]; b[k] = o.b[k]; }
    }
    __device__ __forceinline__ float center(float mean, int lane) {             // x -= mean; lane's partial sum of squares
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < NS; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = x[k][e] - mean;
                x[k][e] = d;
                if (inside(k)) v = fmaf(d, d, v);
                else v += (4 * (lane + 64 * k) + e < N) ? d * d : 0.f;
            }
        return v;
    }
    // normalise + affine + split -> the row in global memory
    template <int VLAYOUT, int POL = 0>
    __device__ __forceinline__ void store(float rstd, _Float16* dst, int lane) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const float wv[4] = {w[k].x, w[k].y, w[k].z, w[k].w};
            const float bv[4] = {b[k].x, b[k].y, b[k].z, b[k].w};
            f16x2_t h01, l01, h23, l23;
            split_pair(x[k][0] * rstd * wv[0] + bv[0], x[k][1] * rstd * wv[1] + bv[1], h01, l01);
            split_pair(x[k][2] * rstd * wv[2] + bv[2], x[k][3] * rstd * wv[3] + bv[3], h23, l23);
            if (live(lane, k)) {
                const int qd = lane + 64 * k;
                if (VLAYOUT) {
                    cp::st_h8<POL, cp::QKV_ST>(&dst[8 * qd], f16x8{h01[0], h01[1], h23[0], h23[1], l01[0], l01[1], l23[0], l23[1]});
                } else {
                    _Float16* d = dst + 8 * qd - 4 * (qd & 1);
                    cp::st_h4<POL, cp::QKV_ST>(d, f16x4{h01[0], h01[1], h23[0], h23[1]});
                    cp::st_h4<POL, cp::QKV_ST>(d + 8, f16x4{l01[0], l01[1], l23[0], l23[1]});
                }
            }
        }
    }
};
// LDS image of the frame's projection outputs, already in each head's flat LayerNorm order:
//   Q head h at [h * YQS + f*6 + e], K heads behind them, V head h at [Y_V0 + h * 1552 + f*16 + v]
constexpr int YQS = DQKP + 8;              // head stride of the Q / K part (8 extra floats spread the heads over banks)
constexpr int Y_K0 = NH * YQS;
constexpr int Y_V0 = 2 * NH * YQS;
constexpr int Y_N = Y_V0 + NH * DV;        // 11136 floats

#if defined(LH_PROBE_TRACE)               // timing probe build only (scripts/probe_trace.py): workgroup 5, its 4th frame
__device__ unsigned long long lh_qkv_trace_buf[16];
#define QKV_STAMP(k) do { if (blockIdx.x == 5 && tid == 0 && fr == 5 + 3 * (int)gridDim.x) lh_qkv_trace_buf[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define QKV_STAMP(k) do { } while (0)
#endif

// The product phase of k_qkv_proj_ln for one wave: its one (wave 3: V columns 48..63) or two (waves 0..2: Q | K columns
// 16w.. and V columns 64+16w..) column tiles against the 7 row tiles of the frame.  Until this form the seven tiles ran
// one after the other from a rolled loop — LDS reads, wait, one chain of 6 dependent MFMAs, wait, epilogue, then the same
// for the second column tile — so a wave exposed the LDS latency, two accumulator read-outs and the chain length seven
// times per frame with nothing of its own to issue meanwhile.  Now stage m of 8 issues the LDS reads of row tile m + 1 and
// the inverse row scales of tile m, then zips (lh_recur.hip: one MFMA step, a slice of vector work, a scheduling fence) the
// two chains of tile m — independent, so one fills the other's dependency gap — with the epilogue of tile m - 1.
// Each chain keeps its order (lo.hi, hi.lo, hi.hi per k-step, k-steps ascending: mma_tile1) and each output element its
// arithmetic, so the results are bit-identical.  The stages are unrolled with the fences in place (the plain unroll of
// the old loop let the scheduler hoist all 28 reads and spilled): every LDS address is lane base + immediate.
// TWO is wave-uniform (waves 0..2) and also fixes the row stride of the first tile in `yf`: E for Q / K, VD for V.
// Row tile 6 holds one valid row (96: g4 == 0, r == 0); its other 15 rows get neither arithmetic nor a store.
template <bool TWO, bool FAST>
__device__ __forceinline__ void qkv_products(const _Float16* ahi, const _Float16* alo, const float* rinv, float* yf, int g4, int l15,
                                             const f16x8 (&wh0)[2], const f16x8 (&wl0)[2], const f16x8 (&wh1)[2],
                                             const f16x8 (&wl1)[2], float bz0, float bz1, float a0, float sv, int base0, int base1) {
    constexpr int NT = FR_RP / 16, STR0 = TWO ? E : VD;
    static_assert(2 * NH * E == 3 * 16 && NQKV / 16 == 7, "waves 0..2: a Q | K tile and a V tile; wave 3: one V tile");
    ATile a[2];
    float4 iv[2];
    f32x4 r0[2], r1[2];
    float* y0 = yf + base0 + g4 * 4 * STR0;
    float* y1 = yf + base1 + g4 * 4 * VD;
    a_tile_read<FR_RP>(a[0], ahi, alo, 0, g4, l15);
    xp_for<NT + 1>([&](auto m_) {
        constexpr int m = decltype(m_)::value, cur = m & 1, prv = cur ^ 1;
        if (m + 1 < NT) a_tile_read<FR_RP>(a[prv], ahi, alo, m + 1, g4, l15);
        if (m < NT) iv[cur] = *reinterpret_cast<const float4*>(&rinv[m * 16 + g4 * 4]);      // 1 / scale of this lane's 4 rows
        __builtin_amdgcn_sched_barrier(0);
        // epilogue of row r of tile m - 1: bias + PReLU -> yf, already in each head's LayerNorm order
        auto epilogue = [&](auto r_) {
            constexpr int r = decltype(r_)::value, row = (m - 1) * 16 + r;      // + 4 g4: in y0 / y1
            const float ivr = r == 0 ? iv[prv].x : r == 1 ? iv[prv].y : r == 2 ? iv[prv].z : iv[prv].w;
            const float z0 = fmaf(r0[prv][r], ivr, bz0);
            y0[row * STR0] = FAST ? prelu_mm<true>(z0, a0) : prelu_f(z0, a0);
            if (TWO) {
                const float z1 = fmaf(r1[prv][r], ivr, bz1);
                y1[row * VD] = FAST ? prelu_mm<true>(z1, sv) : prelu_f(z1, sv);
            }
        };
        if (m < NT) {
            xp_for<6>([&](auto s_) {
                constexpr int s = decltype(s_)::value, ks = s / 3, j = s % 3;
                const f16x8 av = j == 0 ? a[cur].l[ks] : a[cur].h[ks];
                const f32x4 c0 = s == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : r0[cur];
                r0[cur] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, j == 1 ? wl0[ks] : wh0[ks], c0, 0, 0, 0);
                if (TWO) {
                    const f32x4 c1 = s == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : r1[cur];
                    r1[cur] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, j == 1 ? wl1[ks] : wh1[ks], c1, 0, 0, 0);
                }
                if (m > 0 && s >= 1 && s <= 4) epilogue(std::integral_constant<int, s - 1>{});
                __builtin_amdgcn_sched_barrier(0);
            });
        } else if (g4 == 0) {
            epilogue(std::integral_constant<int, 0>{});
        }
    });
}

// ROWS (ABI 19: the one-frame chunks of a paced session host, lh_qkv_proj_ln_rows) is a template flag, not a run-time branch
// in the persistent loop: the lock-step instantiation sits at 249 of 256 VGPRs and stays, instruction for instruction, the
// code it was.  With ROWS (T = Tc = 1, tw0 = 0) `ring_pos` is write_pos[B]: frame b writes its K / V rows into ring slot
// write_pos[b], a negative entry writes neither (a held or idle row: its Q row is still written, from the zero-gated input).
// POL (lh_cachepol.h): 0 = plain accesses, 1 = the frame load and the Q / K / V stores as the stream table says
// RINGM (ABI 32: a streaming chunk of 2 <= T <= 16 frames on a persistent ring of R = HIST + T rows, whole clip) is a flag
// in the same manner: frame t of the chunk writes its K / V rows into slot (*ring_pos + t) mod R.  The modulo is taken once
// in front of the frame loop; per frame the slot is one scalar add, compare and select (t is wave-uniform).
template <bool ROWS, bool RINGM = false, int POL = 0>
__global__ void __launch_bounds__(256, 2) k_qkv_proj_ln(const float* __restrict__ y, const _Float16* __restrict__ w_pk,
                                                     const float* __restrict__ bias, const float* __restrict__ slopes,
                                                     const float* __restrict__ lnq_w, const float* __restrict__ lnq_b,
                                                     const float* __restrict__ lnk_w, const float* __restrict__ lnk_b,
                                                     const float* __restrict__ lnv_w, const float* __restrict__ lnv_b,
                                                     _Float16* __restrict__ q, _Float16* __restrict__ kx,
                                                     _Float16* __restrict__ vx, int T, int nframes,
                                                     const int* __restrict__ ring_pos, int Tc, int tw0) {
    // time window (lh_qkv_proj_ln_win): frame index fr of the launch = (b, j), j < Tc, is frame t = tw0 + j of utterance b in
    // buffers of T frames; the whole-clip launch is Tc = T, tw0 = 0
    auto gidx = [&](int fr) -> long { return (long)(fr / Tc) * T + tw0 + fr % Tc; };
    __shared__ __attribute__((aligned(16))) _Float16 ahi[FR_A];
    __shared__ __attribute__((aligned(16))) _Float16 alo[FR_A];
    __shared__ __attribute__((aligned(16))) float yf[Y_N];
    // the input is the un-normalised residual stream: every row is scaled by its own power of two before the split and
    // the accumulator rows by the inverse (frame_store_scaled, lh_split.h) — Linear is linear, the bias joins afterwards
    __shared__ __attribute__((aligned(16))) float rinv[FR_RP];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid), g4 = lane >> 4, l15 = lane & 15;

    // wave w owns output-column tiles w and w+4 (of 7): Q|K|V columns 16w.. and 64+16w..
    f16x8 wh0[2], wl0[2], wh1[2], wl1[2];
    load_w<2>(w_pk, wave, lane, wh0, wl0);
    const bool two = wave + 4 < NQKV / 16;
    load_w<2>(w_pk, two ? wave + 4 : wave, lane, wh1, wl1);
    const int c0 = wave * 16 + l15, c1 = c0 + 64;
    const float bz0 = bias[c0], bz1 = bias[two ? c1 : c0];
    const float sq = slopes[0], sk = slopes[1], sv = slopes[2];
    const float a0 = c0 < NH * E ? sq : (c0 < 2 * NH * E ? sk : sv);      // PReLU slope of column c0; c1 is always V
    const bool le1 = sq <= 1.0f && sk <= 1.0f && sv <= 1.0f;            // kernel-uniform: PReLU = max(x, a x)
    // LayerNorm eps of Q, K, V behind the 112 biases: the packer stores 2^k W, 2^k b per LayerNorm group and eps 4^k here
    // (weights.py ln_group; 1e-5 for k = 0) — LN_{eps 4^k}(2^k z) = LN_eps(z), at no instruction in the frame loop
    const float eq = bias[NQKV], ek = bias[NQKV + 1], ev = bias[NQKV + 2];
    // where this lane's columns land in yf: element (f, c) -> base + f * stride
    // (row stride E for Q / K = waves 0..2, VD for V = wave 3: a template argument of qkv_products)
    int base0;
    if (c0 < NH * E) base0 = (c0 / E) * YQS + c0 % E;
    else if (c0 < 2 * NH * E) base0 = Y_K0 + ((c0 - NH * E) / E) * YQS + (c0 - NH * E) % E;
    else base0 = Y_V0 + ((c0 - 2 * NH * E) / VD) * DV + (c0 - 2 * NH * E) % VD;
    const int cv = (two ? c1 : c0) - 2 * NH * E;                  // second tile: always V columns (unused when !two)
    const int base1 = Y_V0 + (cv / VD) * DV + cv % VD;

    frame_zero_pad(ahi, alo, tid);
    if (tid < FR_RP - NF) rinv[NF + tid] = 0.f;                // pad rows: finite
    for (int i = tid; i < 2 * NH * (YQS - DQK); i += 256)      // pad entries 582.. of the Q / K heads stay zero
        yf[(i / (YQS - DQK)) * YQS + DQK + i % (YQS - DQK)] = 0.f;
    // The Q and K LayerNorm affine of this lane's quads stays in registers for the whole persistent loop (48 VGPRs: the
    // rows are shared by all heads and a lane's quads never change).  V's 56 do not fit next to them (249 of 256 VGPRs
    // now) and are still fetched per frame, under the Q / K arithmetic.
    HeadLN<DQK, 2 * QKB> aq, ak;
    aq.load_affine(lnq_w, lnq_b, lane);
    ak.load_affine(lnk_w, lnk_b, lane);
    float4 stg[FR_NLD];
    if ((int)blockIdx.x < nframes) frame_load<POL, cp::QKV_X_LD>(y + gidx(blockIdx.x) * NF * C, tid, stg);
    const long tkp = T + HIST + KV_PAD;
    // K / V row of frame t: HIST + t behind the history rows — or, for a one-frame chunk on a persistent ring
    // (ring_pos != NULL, T = 1), slot (*ring_pos mod 50): the 50 rows are then exactly the attention window, in
    // rotated order, which softmax and P.V do not care about
    static_assert(!(ROWS && RINGM), "per-row positions are one-frame chunks");
    const int krow0 = ROWS ? 0 : RINGM ? (int)((unsigned)*ring_pos % (unsigned)(HIST + T))
                           : ring_pos ? (int)((unsigned)*ring_pos % (unsigned)WIN) : HIST;   // unsigned: never before the ring
    for (int fr = blockIdx.x; fr < nframes; fr += gridDim.x) {      // grid-stride over frames (b*T + t)
        const int b = fr / Tc, t = tw0 + fr % Tc;
        QKV_STAMP(0);
        frame_store_scaled(ahi, alo, rinv, tid, stg);
        __syncthreads();                      // image complete; also orders the previous frame's reads of `yf`
        QKV_STAMP(1);
        if (fr + (int)gridDim.x < nframes) frame_load<POL, cp::QKV_X_LD>(y + gidx(fr + gridDim.x) * NF * C, tid, stg);   // prefetch

        // The 7 row tiles as a software pipeline (stage m: LDS reads of tile m + 1 | MFMAs of tile m | epilogue of tile m - 1),
        // unrolled so that every LDS address is an immediate: qkv_products above.  PReLU as max / min when all three slopes
        // are <= 1 (`le1`, the usual case), else the compare + select form.
        if (two) {
            if (le1) qkv_products<true, true>(ahi, alo, rinv, yf, g4, l15, wh0, wl0, wh1, wl1, bz0, bz1, a0, sv, base0, base1);
            else qkv_products<true, false>(ahi, alo, rinv, yf, g4, l15, wh0, wl0, wh1, wl1, bz0, bz1, a0, sv, base0, base1);
        } else {
            if (le1) qkv_products<false, true>(ahi, alo, rinv, yf, g4, l15, wh0, wl0, wh1, wl1, bz0, bz1, a0, sv, base0, base1);
            else qkv_products<false, false>(ahi, alo, rinv, yf, g4, l15, wh0, wl0, wh1, wl1, bz0, bz1, a0, sv, base0, base1);
        }
        QKV_STAMP(2);
        __syncthreads();
        QKV_STAMP(3);

        // per-head LayerNorm: wave w normalises head w of Q, K and V and writes the split-precision rows
        const int hd = wave;
        const long bh = (long)b * NH + hd;
        float* yq = yf + hd * YQS;
        float* yk = yf + Y_K0 + hd * YQS;
        float* yv = yf + Y_V0 + hd * DV;
        const float* zero8 = yf + DQKP - 8;          // features 600..607 of Q head 0: always zero (16-byte aligned)
        // ROWS: T = 1, fr = b; the row's own slot, wave-uniform
        const int wp = ROWS ? ring_pos[fr] : 0;
        const int krow = ROWS ? (int)((unsigned)wp % (unsigned)WIN) : krow0;
        // RINGM: slot (pos + t) mod R = krow + tk, scalar
        const int tk = RINGM ? (krow + t >= HIST + T ? t - (HIST + T) : t) : t;
        _Float16* qrow = q + (bh * T + t) * LDQKH;
        _Float16* krow_p = kx + (bh * tkp + krow + tk) * LDQKH;
        _Float16* vrow = vx + (bh * tkp + krow + tk) * LDVH;
        // `fr >> 30` is always 0 but ties the lane index to the loop variable: without it LICM hoists every slot address
        // of the three rows (and V's affine) out of the persistent frame loop and the kernel spills
        const int ln = lane + (fr >> 30);
        {   // Q and K together: two independent statistics chains
            HeadLN<DQK, 2 * QKB> lq, lk;
            lq.set_affine(aq);
            lk.set_affine(ak);
            const float sq1 = lq.read(yq, zero8, ln), sk1 = lk.read(yk, zero8, ln);
            const float mq = wave_sum(sq1) * (1.0f / DQK), mk = wave_sum(sk1) * (1.0f / DQK);
            const float vq = lq.center(mq, ln), vk = lk.center(mk, ln);
            const float rq = rsqrtf(wave_sum(vq) * (1.0f / DQK) + eq), rk = rsqrtf(wave_sum(vk) * (1.0f / DQK) + ek);
            lq.template store<0, POL>(rq, qrow, ln);
            if (!ROWS || wp >= 0) lk.template store<0, POL>(rk, krow_p, ln);
        }
        QKV_STAMP(4);
        if (!ROWS || wp >= 0) {
            HeadLN<DV, DV / 4> lv;
            lv.load_affine(lnv_w, lnv_b, ln);
            const float sv1 = lv.read(yv, zero8, ln);
            const float mv = wave_sum(sv1) * (1.0f / DV);
            const float vv = lv.center(mv, ln);
            const float rv = rsqrtf(wave_sum(vv) * (1.0f / DV) + ev);
            lv.template store<1, POL>(rv, vrow, ln);
        }
        QKV_STAMP(5);
    }
}
#if defined(LH_PROBE_TRACE)
}  // namespace lh
extern "C" int lh_probe_qkv_trace_read(unsigned long long* host_dst) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(lh::lh_qkv_trace_buf), sizeof(lh::lh_qkv_trace_buf)) == hipSuccess ? 0 : 1;
}
namespace lh {
#endif

#if defined(LH_DBG_K6)
__device__ unsigned lh_dbg_k6[4];
__device__ float lh_dbg_part[8 * 24 * 256 * 4];
#endif
// ------------------------------------------------------------------------------------------------------
// attn_concat_proj + LN over (f,c) + residual (+ speaker gain); persistent, grid-stride over frames
// FAN (lh_proj_ln_res_fan, ABI 25): `nfan` speaker gains per utterance — gain [B * nfan][97][64], out [B * nfan][T][97][64]; the
// un-gained frame is computed once and stored nfan times, row b * nfan + j under gain[b * nfan + j]
// TAPS (lh_proj_ln_res_taps, ABI 26): the last block's frame only feeds the transposed conv of the back end, whose channel
// contraction P[f][(kt,kf,o)] = sum_c Y[f][c] Wd[c][o][kt][kf] is linear and per (frame, bin).  It runs here, on the finished
// values in `v`, with the arithmetic of k_deconv_istft (lh_backend.hip) bit for bit: the same eight row groups share a
// power of two, the same hi / lo split, the same two accumulator chains.  The frame is not stored: `out` receives
// P [frames][97][36] (0.5625 of the frame's bytes) and `fmax` the frame maximum max |Y| that bounds the spectra there.
// ------------------------------------------------------------------------------------------------------
constexpr int TAP_NP = 36;                  // tap columns (kt, kf, o); the B image pads them to 48
constexpr int TAP_W = 3 * 2 * 64 * 16;      // halves of the packed taps: 3 column tiles x 2 k-steps x 64 lanes x [hi 8 | lo 8]
template <bool FAN, bool TAPS = false, int POL = 0>      // POL: cache policy of merged, the residual and the output (lh_cachepol.h)
__global__ void __launch_bounds__(256, 2) k_proj_ln_res(const float* __restrict__ merged, const _Float16* __restrict__ w_pk,
                                                     const float* __restrict__ bias, const float* __restrict__ slope,
                                                     const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                     const float* __restrict__ y2, const float* __restrict__ gain,
                                                     float* __restrict__ out, int T, int nframes, int Tc, int tw0, int nfan,
                                                     const _Float16* __restrict__ wd_pk, float* __restrict__ fmax) {
    static_assert(!(FAN && TAPS), "the tap products are the last block's output: no gain, no fan-out");
    constexpr int YP = C + 4;
    auto gidx = [&](int fr) -> long { return (long)(fr / Tc) * T + tw0 + fr % Tc; };      // time window, see k_qkv_proj_ln
    __shared__ __attribute__((aligned(16))) _Float16 ahi[FR_A];
    __shared__ __attribute__((aligned(16))) _Float16 alo[FR_A];
    __shared__ __attribute__((aligned(16))) float ys[NF * YP];
    __shared__ float red[4];
    // TAPS: the packed taps as B fragments, 1 / scale of every row of the split frame, the waves' frame maxima
    __shared__ __attribute__((aligned(16))) _Float16 wds[TAPS ? TAP_W : 8];
    __shared__ __attribute__((aligned(16))) float rinv[TAPS ? FR_RP : 4];
    __shared__ float wm[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid), g4 = lane >> 4, l15 = lane & 15;
    if (TAPS) {
        for (int i = tid; i < TAP_W / 8; i += 256)
            *reinterpret_cast<f16x8*>(&wds[i * 8]) = *reinterpret_cast<const f16x8*>(&wd_pk[i * 8]);
        if (tid < FR_RP - NF) rinv[NF + tid] = 0.f;            // pad rows: finite
    }                                       // (the first frame's staging barrier orders these before their readers)

    f16x8 wh[2], wl[2];
    load_w<2>(w_pk, wave, lane, wh, wl);   // wave w owns output channels 16w .. 16w+15
    const float bz = bias[wave * 16 + l15];
    const float a = slope[0];
    const float eps = bias[C];              // eps 4^k of the packed 2^k W, 2^k b (weights.py ln_group), see k_qkv_proj_ln
    // LayerNorm affine of this thread's fixed float4 slots, resident for all frames of the persistent loop
    constexpr int N = NF * C, N4 = N / 4;
    constexpr int NSLOT = (N4 + 255) / 256;      // 7
    float4 pw[NSLOT], pb[NSLOT];
#pragma unroll
    for (int k = 0; k < NSLOT; ++k) {
        const int i = min(tid + 256 * k, N4 - 1);
        pw[k] = *reinterpret_cast<const float4*>(&lnw[i * 4]);
        pb[k] = *reinterpret_cast<const float4*>(&lnb[i * 4]);
    }

    frame_zero_pad(ahi, alo, tid);
    float4 stg[FR_NLD];
    if ((int)blockIdx.x < nframes) frame_load_heads<POL, cp::PROJ_MERGED_LD>(merged + gidx(blockIdx.x) * N, tid, stg);
    for (int fidx = blockIdx.x; fidx < nframes; fidx += gridDim.x) {     // grid-stride over frames (b*T + t)
        const int b = fidx / Tc;
        const long fr = gidx(fidx) * N;
        frame_store(ahi, alo, tid, stg);
        __syncthreads();                      // image complete; also orders the previous frame's reads of `ys`
        if (fidx + (int)gridDim.x < nframes) frame_load_heads<POL, cp::PROJ_MERGED_LD>(merged + gidx(fidx + gridDim.x) * N, tid, stg);

        // residual rows of this frame: loads in flight during the MFMA + statistics phases
        float4 rv[NSLOT];
#pragma unroll
        for (int k = 0; k < NSLOT; ++k)
            rv[k] = cp::ld_f4<POL, cp::PROJ_RES_LD>(&y2[fr + (long)min(tid + 256 * k, N4 - 1) * 4]);

        // row tiles 0..5 hold rows 0..95 (all valid); only tile 6 (rows 96..111, one valid) needs the bounds check
        // (round 5: one accumulator chain, PReLU as max / min when the slope allows it — see k_qkv_proj_ln)
        auto row_tile = [&](int m, auto checked, auto fast) {
            const f32x4 acc = mma_tile1<FR_RP, 2>(ahi, alo, m, g4, l15, wh, wl, bz);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m * 16 + g4 * 4 + r;
                if (!checked.value || row < NF)
                    ys[row * YP + wave * 16 + l15] = fast.value ? prelu_mm<true>(acc[r], a) : prelu_f(acc[r], a);
            }
        };
        if (a <= 1.0f) {
#pragma unroll 1
            for (int m = 0; m < NF / 16; ++m) row_tile(m, std::false_type{}, std::true_type{});
            row_tile(NF / 16, std::true_type{}, std::true_type{});
        } else {
#pragma unroll 1
            for (int m = 0; m < NF / 16; ++m) row_tile(m, std::false_type{}, std::false_type{});
            row_tile(NF / 16, std::true_type{}, std::false_type{});
        }
        __syncthreads();

        // joint LayerNorm over all 97*64 values of the frame (flat index f*64 + c), float4 granules
        float4 v[NSLOT];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NSLOT; ++k) {
            const int i = min(tid + 256 * k, N4 - 1);
            v[k] = *reinterpret_cast<const float4*>(&ys[(i >> 4) * YP + (i & 15) * 4]);
        }
#pragma unroll
        for (int k = 0; k < NSLOT; ++k)
            if (tid + 256 * k < N4) s += v[k].x + v[k].y + v[k].z + v[k].w;
        const float mean = block_sum_256(s, red) * (1.0f / N);
        float vs = 0.f;
#pragma unroll
        for (int k = 0; k < NSLOT; ++k) {
            const float dx = v[k].x - mean, dy = v[k].y - mean, dz = v[k].z - mean, dw = v[k].w - mean;
#if defined(LH_DBG_K6)            // anatomy probe of profiles/r03c_packed_fp32_corruption.txt (scripts/race_probe.py)
            if (tid + 256 * k < N4) {
                vs += dx * dx + dy * dy + dz * dz + dw * dw;
                if (k == 6) atomicAdd(&lh_dbg_k6[1], 1u);
            }
            if (k == 6 && tid == 0) atomicAdd(&lh_dbg_k6[0], 1u);
            if (k == 6 && tid == 255) atomicAdd(&lh_dbg_k6[2], 1u);
#else
            if (tid + 256 * k < N4) vs += dx * dx + dy * dy + dz * dz + dw * dw;
#endif
        }
#if defined(LH_DBG_K6)
        if (blockIdx.x < 8 && fidx / (int)gridDim.x < 24) {
            float* d = lh_dbg_part + ((blockIdx.x * 24 + fidx / (int)gridDim.x) * 256 + tid) * 4;
            d[0] = vs; d[1] = mean; d[2] = v[6].x; d[3] = s;
        }
#endif
        const float rstd = rsqrtf(block_sum_256(vs, red) * (1.0f / N) + eps);
        // residual + normalised value per slot, then (block 0 only) ALL speaker-gain loads of the frame, then the stores:
        // vmcnt counts loads and stores in one order, so a gain load issued behind the previous slot's store is usable only
        // once that store has been acknowledged — interleaved, every slot paid a store round trip
#pragma unroll
        for (int k = 0; k < NSLOT; ++k) {
            v[k].x = rv[k].x + (v[k].x - mean) * rstd * pw[k].x + pb[k].x;
            v[k].y = rv[k].y + (v[k].y - mean) * rstd * pw[k].y + pb[k].y;
            v[k].z = rv[k].z + (v[k].z - mean) * rstd * pw[k].z + pb[k].z;
            v[k].w = rv[k].w + (v[k].w - mean) * rstd * pw[k].w + pb[k].w;
        }
        if (FAN) {
            // one target after the other, each in the order above (its gain loads, then its stores); `rv` (the residual, used
            // up by now) takes the gains and then the products: `v` stays the un-gained frame and no third array is live
            const float* gj = gain + (long)b * nfan * N;
            long fo = fr + (long)b * (nfan - 1) * T * N;        // frame (b, t) of out row b * nfan
#pragma unroll 1
            for (int j = 0; j < nfan; ++j, gj += N, fo += (long)T * N) {
#pragma unroll
                for (int k = 0; k < NSLOT; ++k)
                    rv[k] = *reinterpret_cast<const float4*>(&gj[(long)min(tid + 256 * k, N4 - 1) * 4]);
#pragma unroll
                for (int k = 0; k < NSLOT; ++k) pin_here(rv[k]);        // (or a slot's load sinks into its store's branch, behind stores)
#pragma unroll
                for (int k = 0; k < NSLOT; ++k) {
                    rv[k].x = v[k].x * rv[k].x; rv[k].y = v[k].y * rv[k].y; rv[k].z = v[k].z * rv[k].z; rv[k].w = v[k].w * rv[k].w;
                }
#pragma unroll
                for (int k = 0; k < NSLOT; ++k) {
                    const int i = tid + 256 * k;
                    if (i < N4) cp::st_f4<POL, cp::PROJ_ST>(&out[fo + i * 4], rv[k]);
                }
            }
            continue;
        }
        if (TAPS) {
            // The frame -> the (free) A images, split like k_deconv_istft::stage_frame: rows r with (r & 31) >> 2 == g share one
            // power of two.  Slot k holds row (tid >> 4) + 16 k, so group `wave` is this wave's even slots and group
            // `wave + 4` its odd ones.  The back end staged 4 float4 per thread on 512 threads with the element index
            // clamped to the frame, so every group but 0 also saw the frame's LAST float4 (row 96, channels 60..63) — here
            // slot 6 of every thread but the first 16, clamped the same way: it joins both maxima.
            const int tx = tid + (fidx >> 30);      // always tid: keeps this phase's per-thread addresses out of the frame loop's registers
            float me = 0.f, mo = 0.f;
#pragma unroll
            for (int k = 0; k < NSLOT; k += 2) me = fmaxf(me, absmax4(v[k]));
#pragma unroll
            for (int k = 1; k < NSLOT; k += 2) mo = fmaxf(mo, absmax4(v[k]));
            static_assert(NSLOT == 7 && N4 - 1 - 256 * (NSLOT - 1) == 15, "slot 6: row 96 in threads 0..15, the clamped last float4 elsewhere");
            if (tid >= 16) mo = fmaxf(mo, absmax4(v[NSLOT - 1]));
            const float ge = wave_max_uniform(me), go = wave_max_uniform(mo);
            float sce, ive, sco, ivo;
            pow2_scale<FR_TE>(ge, sce, ive);
            pow2_scale<FR_TE>(go, sco, ivo);
#pragma unroll
            for (int k = 0; k < NSLOT; ++k) {
                const int i = tx + 256 * k;
                const float sc = (k & 1) ? sco : sce;
                if (i < N4) {
                    store_split4<FR_RP>(ahi, alo, i >> 4, (i & 15) * 4, make_float4(v[k].x * sc, v[k].y * sc, v[k].z * sc, v[k].w * sc));
                    if ((i & 15) == 0) rinv[i >> 4] = (k & 1) ? ivo : ive;
                }
            }
            if (lane == 0) wm[wave] = fmaxf(ge, go);
            __syncthreads();                  // image, rinv and wm complete (the statistics' barriers are behind every read of ys)
            // P = Y (97 x 64) . Wd (64 x 48): wave w owns row tiles w and w + 4, three column tiles each; per tile the chains of
            // the back end — am: hi.hi, ac: hi.lo then lo.hi, k-steps ascending — and (am + ac) * rinv[row]
#pragma unroll 1
            for (int mt = wave; mt < FR_RP / 16; mt += 4) {
                const int ln = lane + (mt >> 30);     // always lane: keeps the tap fragments' reads inside the loop (48 registers)
                f16x8 ah[2], al[2];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int idx = a_slot<FR_RP>(ks * 4 + g4, mt * 16 + l15);
                    ah[ks] = *reinterpret_cast<const f16x8*>(&ahi[idx]);
                    al[ks] = *reinterpret_cast<const f16x8*>(&alo[idx]);
                }
                const float4 iv4 = *reinterpret_cast<const float4*>(&rinv[mt * 16 + g4 * 4]);
                const float iv[4] = {iv4.x, iv4.y, iv4.z, iv4.w};
#pragma unroll
                for (int nt = 0; nt < 3; ++nt) {
                    f32x4 am = f32x4{0.f, 0.f, 0.f, 0.f}, ac = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const f16x8 th = *reinterpret_cast<const f16x8*>(&wds[((nt * 2 + ks) * 64 + ln) * 16]);
                        const f16x8 tl = *reinterpret_cast<const f16x8*>(&wds[((nt * 2 + ks) * 64 + ln) * 16 + 8]);
                        am = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ks], th, am, 0, 0, 0);
                        ac = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[ks], tl, ac, 0, 0, 0);
                        ac = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[ks], th, ac, 0, 0, 0);
                    }
                    const int col = nt * 16 + l15;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = mt * 16 + g4 * 4 + r;
                        if (f < NF && col < TAP_NP) ys[f * TAP_NP + col] = (am[r] + ac[r]) * iv[r];
                    }
                }
            }
            __syncthreads();                  // P complete in ys; the A reads are behind the next frame's frame_store
            const long gf = gidx(fidx);
            float* pd = out + gf * (NF * TAP_NP);
            constexpr int PQ = NF * TAP_NP / 4;       // 873 float4, rows of 36 floats back to back
#pragma unroll
            for (int k = 0; k < (PQ + 255) / 256; ++k) {
                const int i = tx + 256 * k;
                if (i < PQ) cp::st_f4<POL, cp::PROJ_ST>(&pd[i * 4], *reinterpret_cast<const float4*>(&ys[i * 4]));
            }
            if (tid == 0) fmax[gf] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
            continue;                         // (the next frame's staging barrier orders these ys reads before ys is rewritten)
        }
        if (gain) {
#pragma unroll
            for (int k = 0; k < NSLOT; ++k)
                rv[k] = *reinterpret_cast<const float4*>(&gain[(long)b * N + (long)min(tid + 256 * k, N4 - 1) * 4]);
#pragma unroll
            for (int k = 0; k < NSLOT; ++k) {
                v[k].x *= rv[k].x; v[k].y *= rv[k].y; v[k].z *= rv[k].z; v[k].w *= rv[k].w;
            }
        }
#pragma unroll
        for (int k = 0; k < NSLOT; ++k) {
            const int i = tid + 256 * k;
            if (i < N4) cp::st_f4<POL, cp::PROJ_ST>(&out[fr + i * 4], v[k]);
        }
    }
}

}  // namespace lh

static int launch_linear_res(const float* h, const void* w_pk, const float* bias, const float* res, float* out, int rows, int K,
                             int seg, long segstride, hipStream_t st) {
    using namespace lh;
    const int ntiles = (rows + 63) / 64;
    const int grid = ntiles < 768 ? ntiles : 768;
    if (K == 128)
        hipLaunchKernelGGL((k_linear_res<128>), dim3(grid), dim3(256), 0, st, h, (const _Float16*)w_pk, bias, res, out, rows, seg,
                           segstride);
    else if (K == 64)
        hipLaunchKernelGGL((k_linear_res<64>), dim3(grid), dim3(256), 0, st, h, (const _Float16*)w_pk, bias, res, out, rows, seg,
                           segstride);
    else
        return LH_ERR_UNSUPPORTED;
    return check_launch();
}

extern "C" int lh_linear_res(const float* h, const void* w_pk, const float* bias, const float* res, float* out,
                             int rows, int K, lh_stream_t stream) {
    if (!h || !w_pk || !bias || !res || !out || rows <= 0) return LH_ERR_ARG;
    return launch_linear_res(h, w_pk, bias, res, out, rows, K, rows, 0L, (hipStream_t)stream);
}

// time window: rows (b, t0 + j, f) of [B][T][97][..] buffers — h [B*T*97][K], res / out [B*T*97][64]
extern "C" int lh_linear_res_win(const float* h, const void* w_pk, const float* bias, const float* res, float* out, int B, int T,
                                 int t0, int Tc, int K, lh_stream_t stream) {
    using namespace lh;
    if (!h || !w_pk || !bias || !res || !out || B <= 0 || T <= 0 || t0 < 0 || Tc <= 0 || t0 + Tc > T) return LH_ERR_ARG;
    const long off = (long)t0 * NF;
    return launch_linear_res(h + off * K, w_pk, bias, res + off * C, out + off * C, B * Tc * NF, K, Tc * NF, (long)T * NF,
                             (hipStream_t)stream);
}

extern "C" int lh_qkv_proj_ln_win(const float* y, const void* w_pk, const float* bias, const float* slopes,
                                  const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                                  const float* lnv_w, const float* lnv_b, void* q, void* kx, void* vx, const int* ring_pos,
                                  int B, int T, int t0, int Tc, lh_stream_t stream) {
    using namespace lh;
    if (!y || !w_pk || !bias || !slopes || !lnq_w || !lnq_b || !lnk_w || !lnk_b || !lnv_w || !lnv_b || !q || !kx ||
        !vx || B <= 0 || T <= 0 || (ring_pos && (T > 16 || t0 != 0 || Tc != T)) || t0 < 0 || Tc <= 0 || t0 + Tc > T)
        return LH_ERR_ARG;
    const int nframes = B * Tc;
    // a streaming chunk of several frames on its ring (ABI 32): a launch of its own, plain accesses like the one-frame chunk
    if (ring_pos && T > 1)
        hipLaunchKernelGGL((k_qkv_proj_ln<false, true, 0>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream,
                           y, (const _Float16*)w_pk, bias, slopes, lnq_w, lnq_b, lnk_w, lnk_b, lnv_w, lnv_b, (_Float16*)q,
                           (_Float16*)kx, (_Float16*)vx, T, nframes, ring_pos, Tc, t0);
    // cache policy by the footprint of the launch's largest stream (the frames of x; V is as large): lh_cachepol.h
    else if (cp::nt_on((long)nframes * NF * C * 4))
        hipLaunchKernelGGL((k_qkv_proj_ln<false, false, 1>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream, y,
                           (const _Float16*)w_pk, bias, slopes, lnq_w, lnq_b, lnk_w, lnk_b, lnv_w, lnv_b, (_Float16*)q,
                           (_Float16*)kx, (_Float16*)vx, T, nframes, ring_pos, Tc, t0);
    else
        hipLaunchKernelGGL((k_qkv_proj_ln<false, false, 0>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream, y,
                           (const _Float16*)w_pk, bias, slopes, lnq_w, lnq_b, lnk_w, lnk_b, lnv_w, lnv_b, (_Float16*)q,
                           (_Float16*)kx, (_Float16*)vx, T, nframes, ring_pos, Tc, t0);
    return check_launch();
}

extern "C" int lh_qkv_proj_ln(const float* y, const void* w_pk, const float* bias, const float* slopes,
                              const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                              const float* lnv_w, const float* lnv_b, void* q, void* kx, void* vx, const int* ring_pos,
                              int B, int T, lh_stream_t stream) {
    return lh_qkv_proj_ln_win(y, w_pk, bias, slopes, lnq_w, lnq_b, lnk_w, lnk_b, lnv_w, lnv_b, q, kx, vx, ring_pos, B, T, 0, T,
                              stream);
}

extern "C" int lh_qkv_proj_ln_rows(const float* y, const void* w_pk, const float* bias, const float* slopes,
                                   const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                                   const float* lnv_w, const float* lnv_b, void* q, void* kx, void* vx, const int* write_pos,
                                   int B, lh_stream_t stream) {
    using namespace lh;
    if (!y || !w_pk || !bias || !slopes || !lnq_w || !lnq_b || !lnk_w || !lnk_b || !lnv_w || !lnv_b || !q || !kx || !vx ||
        !write_pos || B <= 0)
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_qkv_proj_ln<true, false, 0>), dim3(B < 512 ? B : 512), dim3(256), 0, (hipStream_t)stream, y,
                       (const _Float16*)w_pk, bias, slopes, lnq_w, lnq_b, lnk_w, lnk_b, lnv_w, lnv_b, (_Float16*)q,
                       (_Float16*)kx, (_Float16*)vx, 1, B, write_pos, 1, 0);
    return check_launch();
}

extern "C" int lh_proj_ln_res_win(const float* merged, const void* w_pk, const float* bias, const float* slope,
                                  const float* ln_w, const float* ln_b, const float* y2, const float* gain, float* out,
                                  int B, int T, int t0, int Tc, lh_stream_t stream) {
    using namespace lh;
    if (!merged || !w_pk || !bias || !slope || !ln_w || !ln_b || !y2 || !out || B <= 0 || T <= 0 || t0 < 0 || Tc <= 0 ||
        t0 + Tc > T)
        return LH_ERR_ARG;
    const int nframes = B * Tc;
    if (cp::nt_on((long)nframes * NF * C * 4))
        hipLaunchKernelGGL((k_proj_ln_res<false, false, 1>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream,
                           merged, (const _Float16*)w_pk, bias, slope, ln_w, ln_b, y2, gain, out, T, nframes, Tc, t0, 1,
                           (const _Float16*)nullptr, (float*)nullptr);
    else
        hipLaunchKernelGGL((k_proj_ln_res<false, false, 0>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream,
                           merged, (const _Float16*)w_pk, bias, slope, ln_w, ln_b, y2, gain, out, T, nframes, Tc, t0, 1,
                           (const _Float16*)nullptr, (float*)nullptr);
    return check_launch();
}

extern "C" int lh_proj_ln_res(const float* merged, const void* w_pk, const float* bias, const float* slope,
                              const float* ln_w, const float* ln_b, const float* y2, const float* gain, float* out,
                              int B, int T, lh_stream_t stream) {
    return lh_proj_ln_res_win(merged, w_pk, bias, slope, ln_w, ln_b, y2, gain, out, B, T, 0, T, stream);
}

// tap products (ABI 26): the last block's stage in front of lh_taps_istft — p_out [B][T][97][36], fmax [B][T]
extern "C" int lh_proj_ln_res_taps_win(const float* merged, const void* w_pk, const float* bias, const float* slope,
                                       const float* ln_w, const float* ln_b, const float* y2, const void* wdec_pk, float* p_out,
                                       float* fmax, int B, int T, int t0, int Tc, lh_stream_t stream) {
    using namespace lh;
    if (!merged || !w_pk || !bias || !slope || !ln_w || !ln_b || !y2 || !wdec_pk || !p_out || !fmax || B <= 0 || T <= 0 ||
        t0 < 0 || Tc <= 0 || t0 + Tc > T)
        return LH_ERR_ARG;
    const int nframes = B * Tc;
    if (cp::nt_on((long)nframes * NF * C * 4))
        hipLaunchKernelGGL((k_proj_ln_res<false, true, 1>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream,
                           merged, (const _Float16*)w_pk, bias, slope, ln_w, ln_b, y2, (const float*)nullptr, p_out, T, nframes, Tc,
                           t0, 1, (const _Float16*)wdec_pk, fmax);
    else
        hipLaunchKernelGGL((k_proj_ln_res<false, true, 0>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream,
                           merged, (const _Float16*)w_pk, bias, slope, ln_w, ln_b, y2, (const float*)nullptr, p_out, T, nframes, Tc,
                           t0, 1, (const _Float16*)wdec_pk, fmax);
    return check_launch();
}

extern "C" int lh_proj_ln_res_taps(const float* merged, const void* w_pk, const float* bias, const float* slope,
                                   const float* ln_w, const float* ln_b, const float* y2, const void* wdec_pk, float* p_out,
                                   float* fmax, int B, int T, lh_stream_t stream) {
    return lh_proj_ln_res_taps_win(merged, w_pk, bias, slope, ln_w, ln_b, y2, wdec_pk, p_out, fmax, B, T, 0, T, stream);
}

// fan-out (ABI 25): K gains per utterance, out row b * K + j = the frame of utterance b under gain[b * K + j]
extern "C" int lh_proj_ln_res_fan_win(const float* merged, const void* w_pk, const float* bias, const float* slope,
                                      const float* ln_w, const float* ln_b, const float* y2, const float* gain, float* out,
                                      int B, int T, int t0, int Tc, int K, lh_stream_t stream) {
    using namespace lh;
    if (!gain || K < 1) return LH_ERR_ARG;
    if (K == 1) return lh_proj_ln_res_win(merged, w_pk, bias, slope, ln_w, ln_b, y2, gain, out, B, T, t0, Tc, stream);
    if (!merged || !w_pk || !bias || !slope || !ln_w || !ln_b || !y2 || !out || B <= 0 || T <= 0 || t0 < 0 || Tc <= 0 ||
        t0 + Tc > T)
        return LH_ERR_ARG;
    const int nframes = B * Tc;
    if (cp::nt_on((long)nframes * NF * C * 4))
        hipLaunchKernelGGL((k_proj_ln_res<true, false, 1>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream,
                           merged, (const _Float16*)w_pk, bias, slope, ln_w, ln_b, y2, gain, out, T, nframes, Tc, t0, K,
                           (const _Float16*)nullptr, (float*)nullptr);
    else
        hipLaunchKernelGGL((k_proj_ln_res<true, false, 0>), dim3(nframes < 512 ? nframes : 512), dim3(256), 0, (hipStream_t)stream,
                           merged, (const _Float16*)w_pk, bias, slope, ln_w, ln_b, y2, gain, out, T, nframes, Tc, t0, K,
                           (const _Float16*)nullptr, (float*)nullptr);
    return check_launch();
}

extern "C" int lh_proj_ln_res_fan(const float* merged, const void* w_pk, const float* bias, const float* slope,
                                  const float* ln_w, const float* ln_b, const float* y2, const float* gain, float* out,
                                  int B, int T, int K, lh_stream_t stream) {
    return lh_proj_ln_res_fan_win(merged, w_pk, bias, slope, ln_w, ln_b, y2, gain, out, B, T, 0, T, K, stream);
}

#if defined(LH_DBG_K6)
extern "C" int lh_dbg_part_read(float* host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(lh::lh_dbg_part), sizeof(lh::lh_dbg_part)) == hipSuccess ? 0 : 1;
}
extern "C" int lh_dbg_k6_read(unsigned* host4, int reset) {
    if (hipMemcpyFromSymbol(host4, HIP_SYMBOL(lh::lh_dbg_k6), 16) != hipSuccess) return 1;
    if (reset) { unsigned z[4] = {0, 0, 0, 0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(lh::lh_dbg_k6), z, 16); }
    return 0;
}
#endif
