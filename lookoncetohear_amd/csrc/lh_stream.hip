// Low-latency intra-frame BiLSTM for the streaming / small-batch case (BASELINE configs[1]: batch-1, 8 ms chunks).
//
// With one frame per utterance in flight there is ONE real sequence per (utterance, direction): the tiled MFMA
// recurrence (lh_lstm.hip) then runs a 16-row tile with 15 dead rows and pays ~1.1 us per step for 54 matrix
// instructions and a workgroup barrier — 97 steps x 3 blocks = 0.32 of the 0.60 ms chunk.  Here a workgroup owns one
// (frame, direction) and treats the step as what it is, a 256 x 64 mat-vec:
//   1. the input half of all 97 steps is hoisted out of the recurrence: G_x = LN(x) W_ih'^T + b as ONE
//      [97 x 64] x [64 x 256] split-precision MFMA GEMM into LDS (LayerNorm affine folded into W_ih', b);
//   2. the step is latency, not throughput: ONE wave per SIMD (256 threads) and four lanes per hidden unit.  Lane
//      (unit u, slice s) keeps the 16-wide k slice s of the unit's four gate rows of W_hh (64 fp32 registers), reads its
//      16 values of h_{t-1} from LDS (4 broadcast reads instead of the 8 of a half row) and does the 64 FMAs as 32 packed
//      ones (v_pk_fma_f32 on whole register pairs: the safe form, build.py).  The four partial sums per gate are then
//      REDUCE-SCATTERED over the quad with DPP quad permutes (the gate slots of a lane are XOR-rotated by its slice
//      index, so lane s ends up with the full sum of gate s after three DPP adds, against 12 adds for an all-reduce),
//      so every lane evaluates ONE gate non-linearity (2 transcendentals per lane and step instead of 8 on one lane in
//      eight), and two more quad permutes bring i*g and o to the lane that holds the cell state.  4 transcendental + ~70 other instructions per step on an otherwise empty SIMD, one barrier:
//      0.49 -> 0.36-0.38 us per step (profiles/r03k_*).
// Reference: tfgridnet_causal.py:505-512 (intra_norm + intra_rnn); output in the unfused layout [rows][128] consumed
// by lh_linear_res.
#include "lh_quad.h"
#include "lh_resample.h"

namespace lh {

constexpr int IS_NLD = (NF * 16 + IS_NT - 1) / IS_NT;

// grid = n_frames * 2 (direction = blockIdx & 1), block 512
__global__ void __launch_bounds__(IS_NT) k_intra_stream(const float* __restrict__ x, const _Float16* __restrict__ wih_pk,
                                                        const float* __restrict__ b_sum, const float* __restrict__ whh,
                                                        float* __restrict__ h_out, int n_frames) {
    __shared__ __attribute__((aligned(16))) _Float16 ahi[FR_A];          // LN(x) of the frame, A image [97 -> 112 x 64]
    __shared__ __attribute__((aligned(16))) _Float16 alo[FR_A];
    __shared__ __attribute__((aligned(16))) float gxs[NF * IS_GP];       // input half of the gates, [step][column]
    __shared__ __attribute__((aligned(16))) float hs[2][H];              // h_{t-1} / h_t
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid), g4 = lane >> 4, l15 = lane & 15;
    const int frame = blockIdx.x >> 1, dir = blockIdx.x & 1;
    const float* xf = x + (long)frame * NF * C;

    // Thread tid = 4 u + s < 256: hidden unit u, k slice s (quad_step)
    const int unit = (tid & (IS_NR - 1)) >> 2, qs = tid & 3;
    f32x2 wr[4][8];
    quad_load_w(whh + (long)dir * IS_GP * H, unit, qs, wr);

    // ---- LayerNorm over the 64 channels of every (frame, f) row (affine folded into the weights), split to fp16 hi/lo
    static_assert(FR_A % 8 == 0, "16-byte zero fill");
    for (int i = tid; i < FR_A / 8; i += IS_NT) {
        *reinterpret_cast<f16x8*>(&ahi[i * 8]) = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        *reinterpret_cast<f16x8*>(&alo[i * 8]) = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IS_NLD; ++i) {
        const int e = tid + IS_NT * i, ec = min(e, NF * 16 - 1);       // 16 threads per row; clamped copies are not stored
        float4 v = *reinterpret_cast<const float4*>(&xf[(ec >> 4) * C + (ec & 15) * 4]);
        const float mean = group16_sum(v.x + v.y + v.z + v.w) * (1.0f / C);
        v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
        const float var = group16_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w) * (1.0f / C);
        const float rstd = rsqrtf(var + LN_EPS);
        if (e < NF * 16)
            store_split4<FR_RP>(ahi, alo, e >> 4, (e & 15) * 4, make_float4(v.x * rstd, v.y * rstd, v.z * rstd, v.w * rstd));
    }
    if (tid < H) hs[0][tid] = 0.f;
    __syncthreads();

    // ---- G_x[p][n] = b[n] + LN(x)[p] . W_ih'[n]: wave w owns column tiles 2w, 2w+1
#pragma unroll 1
    for (int i = 0; i < 16 / IS_NW; ++i) {
        const int nt = (16 / IS_NW) * wave + i;
        f16x8 wh[2], wl[2];
        load_w<2>(wih_pk + (long)dir * 16 * 2 * 64 * 16, nt, lane, wh, wl);
        const float bz = b_sum[dir * IS_GP + nt * 16 + l15];
#pragma unroll 1
        for (int m = 0; m < FR_RP / 16; ++m) {
            const f32x4 acc = mma_tile<FR_RP, 2>(ahi, alo, m, g4, l15, wh, wl, bz);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = m * 16 + g4 * 4 + r;
                if (p < NF) gxs[p * IS_GP + nt * 16 + l15] = acc[r];
            }
        }
    }
    __syncthreads();

    // ---- recurrence: zero initial state (the intra LSTM carries nothing between frames)
    if (tid >= IS_NR) {
        for (int it = 0; it < NF; ++it) QS_SYNC();
        return;
    }
    float c = 0.f;                                      // (scaled by QS_K2; zero either way)
    const float gscale = quad_gate_scale(qs);
    float* hrow = h_out + ((long)frame * NF) * 2 * H + dir * H + unit;
    for (int it = 0; it < NF; ++it) {
        const int p = dir ? NF - 1 - it : it;
        const float gx = gscale * gxs[p * IS_GP + tid];
        const float hv = quad_step(wr, hs[it & 1] + 16 * qs, gx, c, qs);
        if (qs == 1) {
            hs[(it + 1) & 1][unit] = hv;
            hrow[(long)p * 2 * H] = hv;
        }
        QS_SYNC();
    }
}

// ------------------------------------------------------------------------------------------------------
// Inter-frame LSTM for few sequences (batch 1-2 offline since round 6; the kernel serves any number): LayerNorm -> causal LSTM over time with carried (h, c) ->
// Linear(64->64) -> + residual  (tfgridnet_causal.py:521-538), one workgroup per sequence (b, f).
// The tiled kernel (k_ln_lstm_lin) needs 16 sequences per workgroup: at batch 1 that is 7 workgroups walking 625
// steps at ~1.1 us each (0.7 ms per block, 2.1 of the 3.0 ms forward).  Here every sequence gets its own CU and the
// step is the same quad-lane 256 x 64 mat-vec as in k_intra_stream (quad_step); the time axis is cut into chunks of 64 steps whose input
// half (LN(x) W_ih'^T + b) and output projection (h W_lin^T + b + residual) run as split-precision MFMA GEMMs before
// and after the chunk's recurrence.
// ------------------------------------------------------------------------------------------------------
constexpr int IM_TC = 64;                  // steps per chunk
constexpr int IM_A = 2 * 4 * IM_TC * 8;    // halves per [64 x 64] A image
constexpr int IM_XP = C + 4;               // raw-x staging row

__global__ void __launch_bounds__(IS_NT) k_inter_matvec(const float* __restrict__ x, const _Float16* __restrict__ wih_pk,
                                                        const float* __restrict__ b_sum, const float* __restrict__ whh,
                                                        const _Float16* __restrict__ wlin_pk, const float* __restrict__ blin,
                                                        const float* __restrict__ h0, const float* __restrict__ c0,
                                                        float* __restrict__ hN, float* __restrict__ cN,
                                                        float* __restrict__ out, int T, int Tfull, int tw0, int cflags) {
    // time window (lh_inter_matvec_win): steps 0 .. T-1 of the launch are frames tw0 .. tw0+T-1 of buffers laid out for Tfull
    // frames; cflags bit 0 = c0 holds the kernel's scaled cell state (QS_K2 c, written by the previous window with bit 1),
    // bit 1 = cN is written that way (like k_inter_xp: the windows then reproduce the whole-clip launch bit for bit when
    // they start on multiples of the 64-step chunk)
    __shared__ __attribute__((aligned(16))) _Float16 xhi[IM_A];          // LN(x) of the chunk's steps
    __shared__ __attribute__((aligned(16))) _Float16 xlo[IM_A];
    __shared__ __attribute__((aligned(16))) _Float16 hhi[IM_A];          // h_t of the chunk's steps
    __shared__ __attribute__((aligned(16))) _Float16 hlo[IM_A];
    __shared__ __attribute__((aligned(16))) float xraw[IM_TC * IM_XP];   // un-normalised rows (residual)
    __shared__ __attribute__((aligned(16))) float gxs[IM_TC * IS_GP];    // input half of the gates, [step][column]
    __shared__ __attribute__((aligned(16))) float hs[2][H];              // h_{t-1} / h_t
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid), g4 = lane >> 4, l15 = lane & 15;
    const int seq = blockIdx.x, b = seq / NF, f = seq % NF;              // state row b*97 + f
    const float* xs = x + (((long)b * Tfull + tw0) * NF + f) * C;        // step t -> + t * 97 * 64
    float* os = out + (((long)b * Tfull + tw0) * NF + f) * C;
    const long tstride = (long)NF * C;

    const int unit = (tid & (IS_NR - 1)) >> 2, qs = tid & 3;            // hidden unit, k slice (quad_step): threads < 256
    f32x2 wr[4][8];
    quad_load_w(whh, unit, qs, wr);
    const bool cell_lane = qs == 1 && tid < IS_NR;
    float c = cell_lane ? ((cflags & 1) ? 1.0f : QS_K2) * c0[(long)seq * H + unit] : 0.f;       // carried times QS_K2
    const float gscale = quad_gate_scale(qs);
    if (tid < H) hs[0][tid] = h0[(long)seq * H + tid];
    int hb = 0;                                                          // hs buffer holding h_{t-1}

    for (int t0 = 0; t0 < T; t0 += IM_TC) {
        const int nst = min(IM_TC, T - t0);
        // ---- stage the chunk: raw rows (residual) and LayerNorm'ed rows as the x A image; 16 threads per row
#pragma unroll
        for (int i = 0; i < IM_TC * 16 / IS_NT; ++i) {
            const int e = tid + IS_NT * i, r = e >> 4, q4 = (e & 15) * 4;
            float4 v = *reinterpret_cast<const float4*>(&xs[(long)min(t0 + r, T - 1) * tstride + q4]);
            *reinterpret_cast<float4*>(&xraw[r * IM_XP + q4]) = v;
            const float mean = group16_sum(v.x + v.y + v.z + v.w) * (1.0f / C);
            v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
            const float var = group16_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w) * (1.0f / C);
            const float rstd = rsqrtf(var + LN_EPS);
            store_split4<IM_TC>(xhi, xlo, r, q4, make_float4(v.x * rstd, v.y * rstd, v.z * rstd, v.w * rstd));
        }
        __syncthreads();
        // ---- G_x[step][n] = b[n] + LN(x)[step] . W_ih'[n]: wave w owns column tiles 2w, 2w+1
#pragma unroll 1
        for (int i = 0; i < 16 / IS_NW; ++i) {
            const int nt = (16 / IS_NW) * wave + i;
            f16x8 wh[2], wl[2];
            load_w<2>(wih_pk, nt, lane, wh, wl);
            const float bz = b_sum[nt * 16 + l15];
#pragma unroll 1
            for (int m = 0; m < IM_TC / 16; ++m) {
                const f32x4 acc = mma_tile<IM_TC, 2>(xhi, xlo, m, g4, l15, wh, wl, bz);
#pragma unroll
                for (int r = 0; r < 4; ++r) gxs[(m * 16 + g4 * 4 + r) * IS_GP + nt * 16 + l15] = acc[r];
            }
        }
        __syncthreads();
        // ---- recurrence over the chunk's steps (see k_intra_stream); h_t also goes into the projection's A image
        if (tid >= IS_NR) {
            for (int it = 0; it < nst; ++it) QS_SYNC();
            hb ^= nst & 1;
        } else {
            for (int it = 0; it < nst; ++it) {
                const float gx = gscale * gxs[it * IS_GP + tid];
                const float hv = quad_step(wr, hs[hb] + 16 * qs, gx, c, qs);
                if (cell_lane) {
                    hs[hb ^ 1][unit] = hv;
                    _Float16 hh, hl_;
                    split_hl(hv, hh, hl_);
                    const int idx = a_index<IM_TC>(it, unit);
                    hhi[idx] = hh;
                    hlo[idx] = hl_;
                }
                hb ^= 1;
                QS_SYNC();
            }
        }
        // ---- projection + residual: out[step][o] = x[step][o] + b[o] + sum_u h[step][u] W_lin[o][u]; 16 (row tile,
        //      column tile) products over the waves
#pragma unroll 1
        for (int p = wave; p < (IM_TC / 16) * 4; p += IS_NW) {
            const int mt = p >> 2, nt = p & 3;
            f16x8 wh[2], wl[2];
            load_w<2>(wlin_pk, nt, lane, wh, wl);
            const f32x4 acc = mma_tile<IM_TC, 2>(hhi, hlo, mt, g4, l15, wh, wl, blin[nt * 16 + l15]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int st = mt * 16 + g4 * 4 + r;
                if (st < nst) os[(long)(t0 + st) * tstride + nt * 16 + l15] = acc[r] + xraw[st * IM_XP + nt * 16 + l15];
            }
        }
        __syncthreads();
    }
    if (tid < H) hN[(long)seq * H + tid] = hs[hb][tid];
    if (cell_lane) cN[(long)seq * H + unit] = c * ((cflags & 2) ? 1.0f : 1.0f / QS_K2);
}

// ------------------------------------------------------------------------------------------------------
// Streaming sessions (include/lookonce_hip.h, ABI 16): the first and the last node of a batched streamer's per-chunk graph.
// Slots (batch rows) open, close and fail one at a time while the chunk loop goes on in lock-step.  Plain streaming
// kernels: a few word loads and the slot's 1.5 KB input row per wave to decide, 16-byte stores to zero a slot's state.
// One kernel per role — k_session_begin, k_session_end, k_session_move, k_session_capture — and two compile-time flags for
// the forms a host can take; what a form does not have is not in its instantiation (if constexpr), not tested at run time:
//   ROWS  (ABI 18) a compacting host: the words, the gated chunk and the state belong to ROW r, the input row, the output row,
//         the hold word and the fault word to the listener's SLOT slot_of[r].  Without it row r is slot r.
//   PACED (ABI 19) a listener whose chunk is late is HELD for the step instead of stalling the others.  hold[S] is one more
//         input word per slot, posted by the host like the commands; pos[S] is the row's own K / V ring position and
//         write_pos[S] what the chunk's kernels get of it.
// Who writes what, in every form: every decision is a function of unmodified inputs (cmd, active, the input row; PACED:
// hold).  k_session_begin writes the gated input, the state it zeroes and (PACED) write_pos, never a word, so every workgroup
// of a row reaches the same decision; k_session_end (one workgroup per row, after every other kernel of the chunk) repeats
// that decision and is the only writer of cmd / active / fault.  A compacting host has one more writer, BEFORE both:
// k_session_move copies a moved row's `active`, device command word and (PACED) pos with the row, and the two kernels then
// decide from the moved words.  lh_ring_advance_rows is the only other writer of pos.
// ------------------------------------------------------------------------------------------------------
struct SessSpans { lh_span_t s[LH_SESSION_MAX_SPANS]; int n; };     // travels in the kernel arguments
constexpr int SS_NT = 256;
constexpr int SS_IN4 = NMIC * NFFT / 4;        // 96 float4 per input row
constexpr int SS_OUT4 = NSRC * HOP / 4;        // 64 float4 per output row
static_assert(SS_IN4 == 64 + 32 && SS_OUT4 == 64, "one wave reads an input row in two loads; index masks below");

__device__ __forceinline__ bool nonfinite4(const float4& v) {
    const unsigned m = 0x7f800000u;                // exponent all ones: inf / NaN
    return (__float_as_uint(v.x) & m) == m || (__float_as_uint(v.y) & m) == m || (__float_as_uint(v.z) & m) == m ||
           (__float_as_uint(v.w) & m) == m;
}
__device__ __forceinline__ bool wave_any(bool p) {           // every lane of the wave calls it
    int v = p ? 1 : 0;
    v |= __shfl_xor(v, 32); v |= __shfl_xor(v, 16); v |= __shfl_xor(v, 8);
    v |= __shfl_xor(v, 4);  v |= __shfl_xor(v, 2);  v |= __shfl_xor(v, 1);
    return v != 0;
}

struct SessDecision { unsigned cmd, gen; bool bad_in, live; };      // gen: the opening's generation, 0 = idle
struct SessLoads { unsigned host, dev, act; float4 x0, x1; };
// Both kernels are latency: a handful of dependent memory round trips at ~1-2 us each is all they cost when nothing happens.
// So everything a decision needs is REQUESTED AT ONCE and unconditionally — the three words and the wave's two float4 of the
// slot's input row — and only then looked at.
// `s` indexes the words, `in_row` the input rows: the same number in the lock-step kernels, row and slot in the row forms.
__device__ __forceinline__ SessLoads sess_load(const float* __restrict__ chunk_in, const unsigned* cmd, const unsigned* active,
                                               int S, int s, int in_row, int lane) {
    SessLoads l;
    const float4* in4 = reinterpret_cast<const float4*>(chunk_in + (long)in_row * NMIC * NFFT);
    l.host = cmd[s];
    l.dev = cmd[S + s];
    l.act = active[s];
    l.x0 = in4[lane];
    l.x1 = in4[64 + (lane & (SS_IN4 - 64 - 1))];   // 32 more float4: the upper half-wave reads them again
    return l;
}
// Wave-uniform, and the same in every wave of every workgroup of the chunk's two session kernels; every lane calls it.
// A held row (PACED) is open and not consuming: live to the words, zeros to the separator, and never judged.
__device__ __forceinline__ SessDecision sess_decide(const SessLoads& l, bool held) {
    SessDecision d;
    d.cmd = l.host | l.dev;
    d.gen = l.act;
    if (d.cmd & LH_SESSION_OPEN) {
        d.gen = (l.host >> LH_SESSION_GEN_SHIFT) & 0x7fffffu;
        if (d.gen == 0) d.gen = 1;
    } else if (d.cmd & LH_SESSION_CLOSE) {
        d.gen = 0;
    }
    d.bad_in = wave_any(nonfinite4(l.x0) || nonfinite4(l.x1)) && d.gen != 0;      // an idle slot's input row is ignored
    d.live = d.gen != 0 && !d.bad_in;
    if (held) d.bad_in = false, d.live = d.gen != 0;
    return d;
}
// ROWS: one more dependent load.  A row without a slot (< 0, or not a slot) decides as if the host had posted CLOSE: it is
// idle whatever its words say, and a RESET the device posted on it is still served.
struct SessRow { int slot; bool owned; };
template <bool ROWS>
__device__ __forceinline__ SessRow sess_row(const int* __restrict__ slot_of, int r, int S) {
    if constexpr (ROWS) {
        const int slot = slot_of[r];
        const bool owned = slot >= 0 && slot < S;
        return SessRow{owned ? slot : 0, owned};
    } else {
        return SessRow{r, true};
    }
}

// grid (tiles, rows launched), block 256; the words keep their stride S.  PACED: tile 0 writes write_pos[row]: -1 for a held
// or non-live row (lh_qkv_proj_ln_rows then writes no K / V row), 0 for a row that serves a RESET, pos[row] otherwise.  A held
// row's commands are served: a RESET zeroes its state here, and the chunk's kernels still run, on the zero-gated input.
template <bool ROWS, bool PACED>
__global__ void __launch_bounds__(SS_NT) k_session_begin(SessSpans sp, const float* __restrict__ chunk_in,
                                                         float* __restrict__ chunk, const unsigned* __restrict__ cmd,
                                                         const unsigned* __restrict__ active, const int* __restrict__ slot_of,
                                                         const unsigned* __restrict__ hold, const int* __restrict__ pos,
                                                         int* __restrict__ write_pos, int S) {
    const int tid = threadIdx.x, r = blockIdx.y, tile = blockIdx.x, ntile = gridDim.x;
    const SessRow w = sess_row<ROWS>(slot_of, r, S);
    SessLoads l = sess_load(chunk_in, cmd, active, S, r, w.slot, tid & 63);
    unsigned h = 0u;
    int p = 0;
    if constexpr (PACED) h = hold[w.slot], p = pos[r];
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 mine = reinterpret_cast<const float4*>(chunk_in)[(long)w.slot * SS_IN4 + min(tid, SS_IN4 - 1)];
    if (!w.owned) l.host = LH_SESSION_CLOSE;
    const bool held = PACED && w.owned && h != 0u;
    const SessDecision d = sess_decide(l, held);
    const bool takes = d.live && !held;            // the row consumes this chunk
    if (tile == 0) {
        if (tid < SS_IN4)                          // gather and gate: only a live listener's samples reach the separator
            reinterpret_cast<float4*>(chunk)[(long)r * SS_IN4 + tid] = takes ? mine : z;
        if constexpr (PACED)
            if (tid == 0) write_pos[r] = !takes ? -1 : (d.cmd & LH_SESSION_RESET) ? 0 : p;
    }
    if (!(d.cmd & LH_SESSION_RESET) && !d.bad_in) return;
    for (int i = 0; i < sp.n; ++i) {               // this tile's share of the row's slice of every state tensor
        const long n16 = (long)(sp.s[i].bytes >> 4);
        float4* q = reinterpret_cast<float4*>(static_cast<char*>(sp.s[i].base) + (unsigned long long)r * sp.s[i].bytes);
        const long hi = n16 * (tile + 1) / ntile;
        for (long j = n16 * tile / ntile + tid; j < hi; j += SS_NT) q[j] = z;
    }
}

// grid rows launched (+ 1 with ROWS), block 1024.  One workgroup per row scans the row's output and fresh (h, c), sp: 150 KB.
// Every thread requests its share of up to SE_SP spans in one go (SE_U float4 per span: 2048 cover a 97 x 64 state row) before
// it looks at any of them — a loop that waited for each load took 26 us per chunk (profiles/r08a_sessions_cost.txt).
// ROWS: the workgroup scatters the row's output, or zeros, to out[slot_of[r]], reports under the SLOT's number and takes the
// row's entry out of the move table; the workgroup after the last row silences every slot that has no row among those
// launched, so every row of `out` is written in every chunk.  Without ROWS there is one output buffer, `out`.
// PACED: a held row is never judged, neither its input row nor what the kernels made of the zeros.  Their output is thrown
// away, and the row's slice of every tensor of the ping-pong set the chunk READ is copied over the set it WROTE (cp.s[2 i] the
// tensor read, cp.s[2 i + 1] the one written in its place; bytes; the rings and pos were never touched), so after the step
// the row is, bit for bit, what it was before.  CLOSE is served as ever; a RESET that begin served (the carried state is then
// the zeros) is posted again for as long as the row is held, so that the chunk that takes the listener's first samples still
// finds it and starts the ring at 0.
constexpr int SE_NT = 1024, SE_SP = LH_SESSION_MAX_END_SPANS, SE_U = 2, SM_U = 4;
template <bool ROWS, bool PACED>
__global__ void __launch_bounds__(SE_NT) k_session_end(SessSpans sp, SessSpans cp, const float* __restrict__ chunk_in,
                                                       const float* __restrict__ out_rows, float* __restrict__ out,
                                                       unsigned* cmd, unsigned* active, unsigned* fault,
                                                       const unsigned* __restrict__ hold,
                                                       const int* __restrict__ slot_of, const int* __restrict__ row_of,
                                                       int* from, int n_rows, int S) {
    __shared__ int wbad[SE_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, r = blockIdx.x;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (ROWS) {
        if (r >= n_rows) {                         // the whole workgroup: 16 slots of 64 float4 per pass
            for (int q = tid >> 6; q < S; q += SE_NT / 64) {
                const int qr = row_of[q];
                if (qr < 0 || qr >= n_rows) reinterpret_cast<float4*>(out)[(long)q * SS_OUT4 + lane] = z;
            }
            return;
        }
    }
    const SessRow w = sess_row<ROWS>(slot_of, r, S);
    SessLoads l = sess_load(chunk_in, cmd, active, S, r, w.slot, lane);
    unsigned h = 0u;
    if constexpr (PACED) h = hold[w.slot];
    // without ROWS there is one output buffer, scanned in place: out_rows is `out` or nothing, and never dereferenced
    const float4 ov = reinterpret_cast<const float4*>(ROWS ? out_rows : out)[(long)r * SS_OUT4 + (tid & (SS_OUT4 - 1))];
    // branch-free: a span the table does not have is span 0 again, an index past the end is the last one (re-reading is free)
    float4 v[SE_SP][SE_U];
#pragma unroll
    for (int i = 0; i < SE_SP; ++i) {
        const lh_span_t sq = sp.s[i < sp.n ? i : 0];
        const int last = (int)min((long)(sq.bytes >> 4), (long)SE_U * SE_NT) - 1;
        const float4* q = reinterpret_cast<const float4*>(static_cast<const char*>(sq.base) + (unsigned long long)r * sq.bytes);
#pragma unroll
        for (int u = 0; u < SE_U; ++u) v[i][u] = q[min(tid + u * SE_NT, last)];
    }
    bool bad = nonfinite4(ov);
#pragma unroll
    for (int i = 0; i < SE_SP; ++i)
#pragma unroll
        for (int u = 0; u < SE_U; ++u) bad |= nonfinite4(v[i][u]);
    // longer spans than the streamer's: the rest, the slow way.  No streamer reaches this loop; the direct calls of
    // tests/session_kernel_cases.py do, on the emulator and on the device, with probes at float4 2048, 2049 and n16 - 1
    for (int i = 0; i < sp.n; ++i) {
        const long n16 = (long)(sp.s[i].bytes >> 4);
        const float4* q = reinterpret_cast<const float4*>(static_cast<const char*>(sp.s[i].base) +
                                                          (unsigned long long)r * sp.s[i].bytes);
        for (long j = tid + (long)SE_U * SE_NT; j < n16; j += SE_NT) bad |= nonfinite4(q[j]);
    }
    if (!w.owned) l.host = LH_SESSION_CLOSE;
    const bool held = PACED && w.owned && h != 0u;           // uniform over the workgroup
    if constexpr (PACED) {
        if (held) {
            // carry: what the chunk's kernels wrote from the zeros is overwritten with what the row had.  A thread's SM_U loads
            // are requested together; thread t only ever touches elements t + k SE_NT, the ones it scanned above
            for (int i = 0; i + 1 < cp.n; i += 2) {
                const long n16 = (long)(cp.s[i].bytes >> 4);
                const unsigned long long off = (unsigned long long)r * cp.s[i].bytes;
                const float4* ps = reinterpret_cast<const float4*>(static_cast<const char*>(cp.s[i].base) + off);
                float4* pd = reinterpret_cast<float4*>(static_cast<char*>(cp.s[i + 1].base) + off);
                for (long j = tid; j < n16; j += (long)SM_U * SE_NT) {
                    float4 c[SM_U];
#pragma unroll
                    for (int u = 0; u < SM_U; ++u) c[u] = ps[min(j + (long)u * SE_NT, n16 - 1)];
#pragma unroll
                    for (int u = 0; u < SM_U; ++u)
                        if (j + (long)u * SE_NT < n16) pd[j + (long)u * SE_NT] = c[u];
                }
            }
        }
    }
    const SessDecision d = sess_decide(l, held);
    bad = wave_any(bad);
    if (lane == 0) wbad[tid >> 6] = bad ? 1 : 0;
    __syncthreads();                               // also: every wave has read the words thread 0 is about to write
    int any = 0;
#pragma unroll
    for (int q = 0; q < SE_NT / 64; ++q) any |= wbad[q];
    // a true fp32 overflow from finite input: non-finite output or fresh (h, c) of a live row.  A held row's scan has no verdict
    const bool overflow = d.live && !held && any != 0;
    const bool on = d.live && !overflow;
    const bool sounds = on && !held;
    // Every form keeps the store to `out` it had.  A row that does not sound is silenced in all of them.  The row form also
    // scatters a sounding row to its slot, in every chunk; the paced forms, which a slot host gives out_rows == out, do so
    // unless that would copy the row onto itself; the lock-step form never has to
    const bool scatter = PACED ? out_rows != out : ROWS;
    if (w.owned && tid < SS_OUT4 && (!sounds || scatter))
        reinterpret_cast<float4*>(out)[(long)w.slot * SS_OUT4 + tid] = sounds ? ov : z;
    if (tid == 0) {
        active[r] = on ? d.gen : 0u;
        // pinned host memory the host reads in place: plain stores at system scope, like the range flag (lh_backend.hip).
        // An unowned row is idle: nothing to report
        if (w.owned) {
            if (d.bad_in || overflow) __hip_atomic_store(&fault[w.slot], d.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else if (d.cmd & LH_SESSION_OPEN) __hip_atomic_store(&fault[w.slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        cmd[r] = 0u;
        // held through its RESET: the row's first consumed chunk must still see it (ring position 0)
        cmd[S + r] = (overflow || (held && on && (d.cmd & LH_SESSION_RESET))) ? (unsigned)LH_SESSION_RESET : 0u;
        if constexpr (ROWS || PACED)
            if (from) from[r] = 0;
    }
}


// Row moves (ABI 18): the first node of a compacting host's chunk.  from[d] = r + 1 copies row r over row d — the row's slice
// of every span (the state of lh_session_begin's table and the speaker gain), its `active` word and the command word the
// device posted on it: everything a row owns but the host's command word, which the host addresses to the row's new place
// itself.  Bytes, not numbers: 16-byte loads and stores, a thread's SM_U loads requested together before it stores any.  The
// host hands out disjoint pairs (every source lies above, every destination below the new row count), so the workgroups of
// one launch share nothing; a row without an entry costs its workgroups one word load.  lh_session_end_rows zeroes the
// entries afterwards: the table is read-only here, and a replay without a new table moves nothing.
// PACED: the row's ring position goes with it.
template <bool PACED>
__global__ void __launch_bounds__(SS_NT) k_session_move(SessSpans sp, const int* __restrict__ from, unsigned* cmd,
                                                        unsigned* active, int* pos, int S) {
    const int tid = threadIdx.x, dst = blockIdx.y, tile = blockIdx.x, ntile = gridDim.x;
    const int src = from[dst] - 1;
    if (src < 0 || src >= S || src == dst) return;
    if (tile == 0 && tid == 0) {
        const unsigned a = active[src], c = cmd[S + src];
        int p = 0;
        if constexpr (PACED) p = pos[src];
        active[dst] = a;
        cmd[S + dst] = c;
        if constexpr (PACED) pos[dst] = p;
    }
    for (int i = 0; i < sp.n; ++i) {
        const long n16 = (long)(sp.s[i].bytes >> 4);
        const float4* ps = reinterpret_cast<const float4*>(static_cast<const char*>(sp.s[i].base) +
                                                           (unsigned long long)src * sp.s[i].bytes);
        float4* pd = reinterpret_cast<float4*>(static_cast<char*>(sp.s[i].base) + (unsigned long long)dst * sp.s[i].bytes);
        const long hi = n16 * (tile + 1) / ntile;
        for (long j = n16 * tile / ntile + tid; j < hi; j += (long)SM_U * SS_NT) {
            float4 v[SM_U];
#pragma unroll
            for (int u = 0; u < SM_U; ++u) v[u] = ps[min(j + (long)u * SS_NT, hi - 1)];
#pragma unroll
            for (int u = 0; u < SM_U; ++u)
                if (j + (long)u * SS_NT < hi) pd[j + (long)u * SS_NT] = v[u];
        }
    }
}

// Enrollment capture (ABI 17): one more node of the per-chunk graph, right after k_session_begin, in a streamer built for
// enrollment.  An armed slot records the 128 NEW samples of both channels of its input row at the device-side chunk count —
// the 64 look-ahead samples are the head of the next chunk's row and are recorded (and judged) then.  One wave per slot: 64
// lanes x one float4 are the 256 samples, and that wave is the only writer of the slot's words and of its clip.  Pure latency
// like the two kernels above, so the three words and the lane's float4 are requested together before any is looked at.
// The clip is read by stream-ordered work only (the host enqueues the embedder behind an event it records after it has seen
// the done word), so the done word needs no release: it tells the host WHICH chunk finished the clip, not that the bytes
// are visible to the host.
// PACED: a held slot's commands are served, its row is neither recorded nor judged.
constexpr int SC_NT = 64;
static_assert(NMIC * HOP / 4 == SC_NT && HOP / 4 == 32, "one float4 per lane: lane = 32 channel + float4 of the channel");
template <bool PACED>
__global__ void __launch_bounds__(SC_NT) k_session_capture(const float* __restrict__ chunk_in, float* __restrict__ enroll,
                                                           unsigned* ecmd, unsigned* estate, unsigned* edone,
                                                           const unsigned* __restrict__ hold, int n_chunks, int S) {
    const int s = blockIdx.x, lane = threadIdx.x, ch = lane >> 5, q = lane & 31;
    const unsigned cmd = ecmd[s];
    unsigned held = 0u;
    if constexpr (PACED) held = hold[s];
    unsigned gen = estate[s], k = estate[S + s];
    const float4 v = reinterpret_cast<const float4*>(chunk_in + ((long)s * NMIC + ch) * NFFT)[q];
    if (cmd & LH_ENROLL_CANCEL) gen = 0u;
    if (cmd & LH_ENROLL_ARM) {                     // also mid-capture: starts again under the new generation
        gen = (cmd >> LH_ENROLL_GEN_SHIFT) & 0x7fffffu;
        if (gen == 0u) gen = 1u;
        k = 0u;
    }
    // wave-uniform: an idle (or held) slot with nothing posted costs the loads above
    if (cmd == 0u && (gen == 0u || held != 0u)) return;
    unsigned done = 0u;
    if (gen != 0u && held == 0u) {
        if (wave_any(nonfinite4(v))) {
            done = gen | LH_ENROLL_FAULT;
        } else {
            k = min(k, (unsigned)n_chunks - 1u);   // the count is device-owned and < n_chunks; never index past the clip
            reinterpret_cast<float4*>(enroll + ((long)s * NMIC + ch) * HOP * n_chunks + (long)HOP * k)[q] = v;
            if (++k == (unsigned)n_chunks) done = gen;
        }
    }
    if (done != 0u || gen == 0u) gen = 0u, k = 0u;
    if (lane == 0) {
        if (cmd != 0u) ecmd[s] = 0u;
        estate[s] = gen;
        estate[S + s] = k;
        // pinned host memory the host reads in place, like fault[S]
        if (done != 0u) __hip_atomic_store(&edone[s], done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Monitor mix (ABI 30): one more node of the per-chunk graph, after k_session_end and ahead of the resample / 16-bit node, in a
// streamer built with a monitor.  Output row j of a slot covers samples [128 j, 128 j + 128) of the slot's stream, and those are
// the first 128 samples of input row j: the dry path needs no delay line, out = wet y + dry x on the rows as they lie.  Two
// gains per slot ramp linearly towards the targets the host posts, `step` per sample; the gain of sample n is a function of the
// gain at the chunk's start, never of sample n - 1, so the lanes share nothing and the ramp lands on its target exactly.
// k_session_capture's shape: one wave per slot, by SLOT in every form, lane = 32 channel + float4 of the channel, and that wave
// is the only writer of the slot's gains and (after k_session_end) of its row.  Pure latency again: the four words and the
// lane's two float4 are requested together before any is looked at; the gains come through lane 0, so every lane holds them
// before lane 0, the writer below, goes on.
// PACED: a held slot's row is the zeros k_session_end wrote and its gains wait for the listener.
static_assert(NSRC * HOP / 4 == SC_NT, "one float4 of the output row per lane, as of the input row");
__device__ __forceinline__ float mix_gain(float g0, float t, float step, int n) {
    const float d = t - g0, lim = (float)(n + 1) * step;
    return fabsf(d) <= lim ? t : g0 + copysignf(lim, d);
}
template <bool PACED>
__global__ void __launch_bounds__(SC_NT) k_session_mix(const float* __restrict__ chunk_in, float* out,
                                                       const float* __restrict__ target, float* gain,
                                                       const unsigned* __restrict__ hold, float step, int S) {
    const int s = blockIdx.x, lane = threadIdx.x, ch = lane >> 5, q = lane & 31;
    float4* row = reinterpret_cast<float4*>(out + ((long)s * NSRC + ch) * HOP) + q;
    const float wt = target[s], dt = target[S + s];
    const float w0 = __shfl(gain[s], 0), d0 = __shfl(gain[S + s], 0);
    unsigned held = 0u;
    if constexpr (PACED) held = hold[s];
    const float4 x = reinterpret_cast<const float4*>(chunk_in + ((long)s * NMIC + ch) * NFFT)[q];
    const float4 y = *row;
    if (held != 0u) return;                        // wave-uniform, like everything up to the stores
    const bool dry_off = d0 == 0.f && dt == 0.f;
    if (dry_off && w0 == 1.f && wt == 1.f) return;       // settled at the defaults: the row keeps its bits, signed zeros included
    const int n = 4 * q;
    float4 r;
    if (dry_off) {                                 // x is not part of the result: 0 * NaN cannot leak
        r.x = mix_gain(w0, wt, step, n) * y.x;
        r.y = mix_gain(w0, wt, step, n + 1) * y.y;
        r.z = mix_gain(w0, wt, step, n + 2) * y.z;
        r.w = mix_gain(w0, wt, step, n + 3) * y.w;
    } else if (wave_any(nonfinite4(x))) {          // no fault: an idle slot has none, k_session_end has judged an open one
        r = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        r.x = fmaf(mix_gain(w0, wt, step, n), y.x, mix_gain(d0, dt, step, n) * x.x);
        r.y = fmaf(mix_gain(w0, wt, step, n + 1), y.y, mix_gain(d0, dt, step, n + 1) * x.y);
        r.z = fmaf(mix_gain(w0, wt, step, n + 2), y.z, mix_gain(d0, dt, step, n + 2) * x.z);
        r.w = fmaf(mix_gain(w0, wt, step, n + 3), y.w, mix_gain(d0, dt, step, n + 3) * x.w);
    }
    *row = r;
    if (lane == 0) {
        gain[s] = mix_gain(w0, wt, step, HOP - 1);
        gain[S + s] = mix_gain(d0, dt, step, HOP - 1);
    }
}

// ------------------------------------------------------------------------------------------------------
// Suspend / resume (ABI 20): one listener's state out of the buffers as a snapshot, and back into any row of any host of the
// same model (layout: include/lookonce_hip.h).  Not nodes of the per-chunk graph: the host enqueues them between two chunks,
// and only in a step that suspends or resumes.  Copies like k_session_move — bytes, 16-byte loads and stores, a thread's SM_U
// loads requested together before it stores any — over a grid of (tile, section): one section per flat span, one per ring,
// and a last one (its tile 0 only) for the header, the words and the embedding.  A ring section is the `window` leading rows
// of each of the row's heads: the snapshot holds them densely, [head][window row][row bytes], the ring has `rows` per head.
// Who writes what: save writes the snapshot only.  Restore writes row `row`'s sections, cmd[1][row], the embedding, and in a
// paced host the row's position word, which no other workgroup of the launch reads (there delta is 0 without looking); in a
// lock-step host the shared counter is read by every workgroup and written by none.  The row is idle while restore runs.
// ------------------------------------------------------------------------------------------------------
struct SnapLayout { SessSpans flat, rings; int heads, rows, window; unsigned embed_bytes; };
constexpr int SNAP_NT = SS_NT, SNAP_TILES = 32;
constexpr unsigned SNAP_WORDS = LH_SNAPSHOT_HEADER_BYTES, SNAP_EMBED = SNAP_WORDS + 16;

__host__ __device__ inline unsigned long long snap_ring_bytes(const SnapLayout& L, int i) {
    return (unsigned long long)L.heads * L.window * L.rings.s[i].bytes;
}
// byte offset of section q: flat spans first, then the rings; q = n_flat + n_rings is the total
__host__ __device__ inline unsigned long long snap_offset(const SnapLayout& L, int q) {
    unsigned long long o = SNAP_EMBED + L.embed_bytes;
    for (int i = 0; i < L.flat.n && i < q; ++i) o += L.flat.s[i].bytes;
    for (int i = 0; i < L.rings.n && L.flat.n + i < q; ++i) o += snap_ring_bytes(L, i);
    return o;
}
__device__ __forceinline__ unsigned snap_header_word(const SnapLayout& L, int i) {
    const int nf = L.flat.n, nr = L.rings.n;
    switch (i) {
        case 0: return (unsigned)LH_SNAPSHOT_MAGIC;
        case 1: return (unsigned)LH_SNAPSHOT_VERSION;
        case 2: return (unsigned)snap_offset(L, nf + nr);
        case 3: return (unsigned)nf;
        case 4: return (unsigned)nr;
        case 5: return (unsigned)L.heads;
        case 6: return (unsigned)L.window;
        case 7: return L.embed_bytes;
        default: break;
    }
    if (i < 8 + nf) return (unsigned)L.flat.s[i - 8].bytes;
    if (i < 8 + nf + nr) return (unsigned)L.rings.s[i - 8 - nf].bytes;
    return 0u;
}
// this tile's share of n16 float4: dst[di(j)] = src[si(j)], j in [n16 tile / ntile, n16 (tile + 1) / ntile)
template <class SI, class DI>
__device__ __forceinline__ void snap_copy(const float4* __restrict__ src, float4* __restrict__ dst, long n16, int tile, int ntile,
                                          int tid, SI si, DI di) {
    const long hi = n16 * (tile + 1) / ntile;
    for (long j = n16 * tile / ntile + tid; j < hi; j += (long)SM_U * SNAP_NT) {
        float4 v[SM_U];
#pragma unroll
        for (int u = 0; u < SM_U; ++u) v[u] = src[si(min(j + (long)u * SNAP_NT, hi - 1))];
#pragma unroll
        for (int u = 0; u < SM_U; ++u)
            if (j + (long)u * SNAP_NT < hi) dst[di(j + (long)u * SNAP_NT)] = v[u];
    }
}
struct SnapDense { __device__ long operator()(long j) const { return j; } };
// dense index j = (head, window row, float4 of the row) -> float4 index from the base of the row's ring rows; the window row is
// rotated by `delta` in [0, window)
struct SnapRing {
    unsigned rb16, per_head, window, delta;
    long head_stride;                              // float4 between two heads of the ring: rows * rb16
    __device__ long operator()(long j) const {
        const unsigned head = (unsigned)j / per_head, rem = (unsigned)j - head * per_head;
        unsigned row = rem / rb16;
        const unsigned col = rem - row * rb16;
        row += delta;
        if (row >= window) row -= window;
        return (long)head * head_stride + (long)row * rb16 + col;
    }
};
__device__ __forceinline__ SnapRing snap_ring(const SnapLayout& L, int i, unsigned delta) {
    const unsigned rb16 = (unsigned)(L.rings.s[i].bytes >> 4);
    return SnapRing{rb16, (unsigned)L.window * rb16, (unsigned)L.window, delta, (long)L.rows * rb16};
}
__device__ __forceinline__ int snap_wrap(int p, int window) {      // any word -> [0, window): a position never indexes past a ring
    p %= window;
    return p < 0 ? p + window : p;
}

// One listener's sections over blockIdx (tile, section): row `row` of the buffers -> `snap`.  `embed` is the listener's own
// embedding, `pos` the word that holds the row's position.
__device__ __forceinline__ void snap_save(const SnapLayout& L, int row, const float4* __restrict__ embed, char* __restrict__ snap,
                                          const unsigned* __restrict__ cmd, const unsigned* __restrict__ active,
                                          const int* __restrict__ pos, int S) {
    const int tid = threadIdx.x, q = blockIdx.y, tile = blockIdx.x, ntile = gridDim.x;
    const int nf = L.flat.n, nr = L.rings.n;
    if (q < nf) {
        const lh_span_t sq = L.flat.s[q];
        snap_copy(reinterpret_cast<const float4*>(static_cast<const char*>(sq.base) + (unsigned long long)row * sq.bytes),
                  reinterpret_cast<float4*>(snap + snap_offset(L, q)), (long)(sq.bytes >> 4), tile, ntile, tid, SnapDense{},
                  SnapDense{});
    } else if (q < nf + nr) {
        const int i = q - nf;
        const SnapRing ring = snap_ring(L, i, 0u);
        const float4* src = reinterpret_cast<const float4*>(L.rings.s[i].base) + (long)row * L.heads * ring.head_stride;
        snap_copy(src, reinterpret_cast<float4*>(snap + snap_offset(L, q)), (long)L.heads * ring.per_head, tile, ntile, tid, ring,
                  SnapDense{});
    } else if (tile == 0) {
        const unsigned a = active[row], c = cmd[S + row];
        const int p = pos[0];
        const int e16 = (int)(L.embed_bytes >> 4);
        float4* pe = reinterpret_cast<float4*>(snap + SNAP_EMBED);
        for (int j = tid; j < e16; j += SNAP_NT) pe[j] = embed[j];
        if (tid == 0) {                            // 68 words by one lane, behind the other sections' 5 MB
            unsigned* hw = reinterpret_cast<unsigned*>(snap);
            for (int w = 0; w < LH_SNAPSHOT_HEADER_BYTES / 4; ++w) hw[w] = snap_header_word(L, w);
            hw += SNAP_WORDS / 4;
            hw[0] = a, hw[1] = c, hw[2] = (unsigned)snap_wrap(p, L.window), hw[3] = 0u;
        }
    }
}
// The way back: `snap` -> row `row`, the listener's embedding, cmd[1][row] and, in a paced host, the row's position word
// `pos_row` (else NULL: the rings are rotated to the shared counter).  `fault` is the slot's own word.
__device__ __forceinline__ void snap_restore(const SnapLayout& L, int row, float4* __restrict__ embed, const char* __restrict__ snap,
                                             unsigned* cmd, int* pos_row, const int* __restrict__ pos_shared, unsigned* fault,
                                             unsigned gen, int S) {
    const int tid = threadIdx.x, q = blockIdx.y, tile = blockIdx.x, ntile = gridDim.x;
    const int nf = L.flat.n, nr = L.rings.n;
    const unsigned* words = reinterpret_cast<const unsigned*>(snap + SNAP_WORDS);
    const unsigned was_active = words[0], was_cmd = words[1];
    const int saved = snap_wrap((int)words[2], L.window);
    if (q < nf) {
        const lh_span_t sq = L.flat.s[q];
        snap_copy(reinterpret_cast<const float4*>(snap + snap_offset(L, q)),
                  reinterpret_cast<float4*>(static_cast<char*>(sq.base) + (unsigned long long)row * sq.bytes),
                  (long)(sq.bytes >> 4), tile, ntile, tid, SnapDense{}, SnapDense{});
    } else if (q < nf + nr) {
        const int i = q - nf;
        // a lock-step target: the listener's oldest row (at `saved`) becomes the row the shared counter overwrites next
        const int delta = pos_shared ? snap_wrap(snap_wrap(pos_shared[0], L.window) - saved, L.window) : 0;
        const SnapRing ring = snap_ring(L, i, (unsigned)delta);
        float4* dst = reinterpret_cast<float4*>(L.rings.s[i].base) + (long)row * L.heads * ring.head_stride;
        snap_copy(reinterpret_cast<const float4*>(snap + snap_offset(L, q)), dst, (long)L.heads * ring.per_head, tile, ntile, tid,
                  SnapDense{}, ring);
    } else if (tile == 0) {
        const int e16 = (int)(L.embed_bytes >> 4);
        const float4* pe = reinterpret_cast<const float4*>(snap + SNAP_EMBED);
        for (int j = tid; j < e16; j += SNAP_NT) embed[j] = pe[j];
        if (tid == 0) {
            cmd[S + row] = was_cmd;
            if (pos_row) pos_row[0] = saved;
            if (was_active == 0u) {                   // a dead snapshot stays dead: the host's OPEN is taken back, the fault reported
                cmd[row] = (unsigned)(LH_SESSION_CLOSE | LH_SESSION_RESET);
                __hip_atomic_store(fault, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// grid (SNAP_TILES, n_flat + n_rings + 1), block 256
__global__ void __launch_bounds__(SNAP_NT) k_session_save(SnapLayout L, const float4* __restrict__ embed, char* __restrict__ snap,
                                                          const unsigned* __restrict__ cmd, const unsigned* __restrict__ active,
                                                          const int* __restrict__ pos, int row, int S) {
    snap_save(L, row, embed, snap, cmd, active, pos, S);
}
// grid (SNAP_TILES, n_flat + n_rings + 1), block 256.  Exactly one of pos_row / pos_shared.
__global__ void __launch_bounds__(SNAP_NT) k_session_restore(SnapLayout L, float4* __restrict__ embed, const char* __restrict__ snap,
                                                             unsigned* cmd, int* pos_row, const int* __restrict__ pos_shared,
                                                             unsigned* fault, unsigned gen, int row, int S) {
    snap_restore(L, row, embed, snap, cmd, pos_row, pos_shared, fault, gen, S);
}

// Suspend / resume of many listeners (ABI 21): the two kernels above with the listener as a third grid dimension and a table in
// device memory that says, per item, which row, whose slot, which snapshot of a [.][stride] buffer.  The same sections, the same
// copy (snap_copy, the layout helpers), the same words; embed, fault and the position words are BASES here, indexed by slot,
// slot and row.  An item whose row or slot is outside [0, S) or whose index is negative is skipped by all of its workgroups
// before any address is formed.  The host hands out distinct rows, slots and (for save) indexes: the workgroups of two items
// share nothing but the read-only shared counter.
struct SnapItem { int row, slot, index; unsigned gen; bool ok; };
__device__ __forceinline__ SnapItem snap_item(const lh_snap_item_t* __restrict__ items, int i, int S) {
    const lh_snap_item_t it = items[i];
    return SnapItem{it.row, it.slot, it.index, it.gen,
                    (unsigned)it.row < (unsigned)S && (unsigned)it.slot < (unsigned)S && it.index >= 0};
}

// grid (tiles, n_flat + n_rings + 1, n_items), block 256.  Exactly one of pos_rows / pos_shared.
__global__ void __launch_bounds__(SNAP_NT) k_session_save_rows(SnapLayout L, const char* __restrict__ embed, char* __restrict__ snaps,
                                                               unsigned long long stride, const unsigned* __restrict__ cmd,
                                                               const unsigned* __restrict__ active,
                                                               const int* __restrict__ pos_rows, const int* __restrict__ pos_shared,
                                                               const lh_snap_item_t* __restrict__ items, int S) {
    const SnapItem it = snap_item(items, blockIdx.z, S);
    if (!it.ok) return;
    snap_save(L, it.row, reinterpret_cast<const float4*>(embed + (unsigned long long)it.slot * L.embed_bytes),
              snaps + (unsigned long long)it.index * stride, cmd, active, pos_rows ? pos_rows + it.row : pos_shared, S);
}
// grid (tiles, n_flat + n_rings + 1, n_items), block 256.  Exactly one of pos_rows / pos_shared; every item is rotated by its
// own delta, from its own saved position.
__global__ void __launch_bounds__(SNAP_NT) k_session_restore_rows(SnapLayout L, char* __restrict__ embed,
                                                                  const char* __restrict__ snaps, unsigned long long stride,
                                                                  unsigned* cmd, int* pos_rows, const int* __restrict__ pos_shared,
                                                                  unsigned* fault, const lh_snap_item_t* __restrict__ items, int S) {
    const SnapItem it = snap_item(items, blockIdx.z, S);
    if (!it.ok) return;
    snap_restore(L, it.row, reinterpret_cast<float4*>(embed + (unsigned long long)it.slot * L.embed_bytes),
                 snaps + (unsigned long long)it.index * stride, cmd, pos_rows ? pos_rows + it.row : nullptr, pos_shared,
                 fault + it.slot, it.gen, S);
}

// ------------------------------------------------------------------------------------------------------
// Packets (ABI 22): the clients' PCM goes in as it arrives and the device cuts its own windows.  Per slot and channel a ring
// fifo[S][2][R] of fp32 samples, R a power of two, and two 32-bit sample counters that wrap modulo 2^32: wr[s] samples written,
// rd[s] samples consumed.  R divides 2^32, so the ring index is `counter & (R - 1)` and the fill is the unsigned difference
// wr - rd, both across the wrap.  Who writes what:
//   k_session_feed   (eager, between two chunks) writes the samples of its items and wr[slot] = at + n, where `at` is the HOST's
//                    mirror of the counter: no thread reads wr, so the workgroups of an item have nothing to race on.  An item
//                    with FLUSH also writes rd[slot] = 0 (and takes `at` as 0): the slot's buffered input is dropped.
//   k_session_frame  (first node of the chunk's graph, one wave per slot) is the only other writer of rd[s] and the only writer
//                    of hold[s]; it reads both counters before it writes either word.
// The two never run at once (one stream), and the host mirrors both counters with the same arithmetic: it knows what every
// launch will find, so the device follows and nothing is ever read back.
// rd only moves by 128 from 0: a window starts on a multiple of 128 samples, R is a multiple of 256, so every float4 of a
// window lies inside the ring and the frame kernel moves 16 bytes at a time — bytes, not numbers.
// ------------------------------------------------------------------------------------------------------
constexpr int SF_NT = 256, SF_MAX_TILES = 16;
struct FeedItem { int slot, n; long off; unsigned at, flags; bool ok; };
// An item is served or skipped WHOLE, and every workgroup of it decides alike from the same five words, before an address
// is formed: slot in [0, S), 0 <= n <= R, and both channels [off, off + 2 n) inside the staging buffer of `elems` elements.
__device__ __forceinline__ FeedItem feed_item(const lh_feed_item_t* __restrict__ items, int i, int S, int R,
                                              unsigned long long elems) {
    const lh_feed_item_t it = items[i];
    FeedItem f{it.slot, it.n, (long)it.offset, it.at, it.flags, false};
    f.ok = (unsigned)it.slot < (unsigned)S && it.n >= 0 && it.n <= R && it.offset >= 0 &&
           (unsigned long long)it.offset + 2ull * (unsigned long long)it.n <= elems;
    if (f.flags & LH_FEED_FLUSH) f.at = 0u;
    return f;
}

// grid (tiles, n_items), block 256.  T = unsigned (fp32 samples, copied as bit patterns) or short (s16, scaled by 2^-15: exact)
template <class T>
__global__ void __launch_bounds__(SF_NT) k_session_feed(const T* __restrict__ staging, unsigned long long elems,
                                                        const lh_feed_item_t* __restrict__ items, unsigned* __restrict__ fifo,
                                                        unsigned* wr, unsigned* rd, int R, int S) {
    const int tid = threadIdx.x, tile = blockIdx.x, ntile = gridDim.x;
    const FeedItem f = feed_item(items, blockIdx.y, S, R, elems);
    if (!f.ok) return;
    const unsigned mask = (unsigned)R - 1u;
    const T* src = staging + f.off;                            // planar: channel 0 [0, n), channel 1 [n, 2 n)
    unsigned* ring = fifo + (long)f.slot * NMIC * R;
    for (int e = tile * SF_NT + tid; e < NMIC * f.n; e += ntile * SF_NT) {
        const int ch = e >= f.n ? 1 : 0, i = e - ch * f.n;
        unsigned bits;
        if constexpr (sizeof(T) == 2) bits = __float_as_uint((float)src[e] * (1.0f / 32768.0f));
        else bits = src[e];
        ring[(long)ch * R + ((f.at + (unsigned)i) & mask)] = bits;
    }
    if (tile == 0 && tid == 0) {
        wr[f.slot] = f.at + (unsigned)f.n;
        if (f.flags & LH_FEED_FLUSH) rd[f.slot] = 0u;
    }
}

// grid S, block 64: one wave per slot.  Pure latency like k_session_capture: the two counters and the lane's float4s of the
// window are requested together (the masked ring index is inside the ring whatever the counters hold) and only then looked at.
constexpr int PK_WIN4 = NFFT / 4;              // 48 float4 per channel of a window
static_assert(NMIC * PK_WIN4 == SS_IN4 && HOP % 4 == 0, "the window is the input row of the session kernels");
__global__ void __launch_bounds__(SC_NT) k_session_frame(const float* __restrict__ fifo, const unsigned* __restrict__ wr,
                                                         unsigned* rd, float* __restrict__ chunk_in, unsigned* hold, int R, int S) {
    const int s = blockIdx.x, lane = threadIdx.x;
    // every lane has loaded both counters before any lane goes on: lane 0, the writer below, cannot overtake a reader
    const unsigned w = __shfl(wr[s], 0), r = __shfl(rd[s], 0), mask = (unsigned)R - 1u;
    const int j0 = lane, j1 = 64 + (lane & (SS_IN4 - 64 - 1));          // float4 of the [2][192] row; lanes >= 32 repeat j1
    const float4* ring = reinterpret_cast<const float4*>(fifo + (long)s * NMIC * R);
    const int R4 = R >> 2;
    const float4 v0 = ring[(j0 / PK_WIN4) * R4 + (int)(((r + 4u * (unsigned)(j0 % PK_WIN4)) & mask) >> 2)];
    const float4 v1 = ring[(j1 / PK_WIN4) * R4 + (int)(((r + 4u * (unsigned)(j1 % PK_WIN4)) & mask) >> 2)];
    const bool takes = w - r >= (unsigned)NFFT;                         // wave-uniform
    if (takes) {
        float4* row = reinterpret_cast<float4*>(chunk_in + (long)s * NMIC * NFFT);
        row[j0] = v0;
        if (lane < SS_IN4 - 64) row[j1] = v1;
    }
    if (lane == 0) {
        if (takes) rd[s] = r + (unsigned)HOP;
        hold[s] = takes ? 0u : 1u;
    }
}

// grid over 8 samples per thread, block 256: out [S][2][128] fp32 -> out16 [S][2][128] int16, one 16-byte store per thread
__device__ __forceinline__ unsigned emit_s16(float x) {
    float y = rintf(x * 32768.0f);                             // round half even; the scaling by 2^15 is exact
    y = x != x ? 0.f : fminf(fmaxf(y, -32768.0f), 32767.0f);   // NaN -> 0, +-inf saturate
    return (unsigned)(int)y & 0xffffu;
}
__global__ void __launch_bounds__(SS_NT) k_session_emit_s16(const float4* __restrict__ out, int4* __restrict__ out16, int n8) {
    const int i = blockIdx.x * SS_NT + threadIdx.x;
    if (i >= n8) return;
    const float4 a = out[2 * i], b = out[2 * i + 1];
    int4 p;
    p.x = (int)(emit_s16(a.x) | (emit_s16(a.y) << 16));
    p.y = (int)(emit_s16(a.z) | (emit_s16(a.w) << 16));
    p.z = (int)(emit_s16(b.x) | (emit_s16(b.y) << 16));
    p.w = (int)(emit_s16(b.z) | (emit_s16(b.w) << 16));
    out16[i] = p;
}

// ------------------------------------------------------------------------------------------------------
// Client rate (ABI 23): the packet host at the client's own sample rate.  The packets land, through k_session_feed unchanged, in a
// second ring raw[S][2][R_in] at the client rate (with two counters of its own); k_session_resample_in turns whole blocks of it
// into 16 kHz samples of the FIFO above, and k_session_resample_out turns every chunk's 16 kHz row into a row at the client
// rate.  Both call resample_dot of lh_resample.h, so what they make equals lh_resample of the whole stream, bit for bit.
//   k_session_resample_in   (eager, behind the feed of the same push; grid tile x item)  An item is (slot, the 16 kHz write
//                    counter before it, whole output blocks, the raw counter of the first block's first tap) — all the HOST's
//                    mirrors, modulo 2^32: the kernel reads no counter, so the workgroups of an item have nothing to race on.
//                    Output j of the item is block j / n, phase j % n; its taps are raw samples [tap + (j / n) o, ... + K).  The
//                    stream's left pad of `width` zeros is the zeroed ring below counter 0.  One thread stores wr[slot].
//   k_session_resample_out  (a graph node after the end kernel, one workgroup per slot)  [tail | row] of a slot and channel is
//                    staged in LDS, T = width + D o carried samples and the chunk's 128; output j of the step reads taps
//                    [(j / n) o, (j / n) o + K) of it; the last T samples become the tail.  A held slot: a zero row, the tail
//                    stays.  The zeroed tail at start is the left pad and the fixed delay of D blocks in one.
// ------------------------------------------------------------------------------------------------------
constexpr int RI_NT = 256, RI_MAX_TILES = 16;
__global__ void __launch_bounds__(RI_NT) k_session_resample_in(const float* __restrict__ raw, int R_in,
                                                               const lh_resample_item_t* __restrict__ items,
                                                               float* __restrict__ fifo, unsigned* wr, int R, int S,
                                                               const float* __restrict__ bank, int o, int n, int width) {
    const int tid = threadIdx.x, tile = blockIdx.x, ntile = gridDim.x, K = 2 * width + o;
    const lh_resample_item_t it = items[blockIdx.y];
    // served or skipped whole, by every workgroup alike and before an address is formed
    if ((unsigned)it.slot >= (unsigned)S || it.blocks < 0 || (long)it.blocks * n > R ||
        (it.blocks > 0 && (long)(it.blocks - 1) * o + K > R_in))
        return;
    const int per = it.blocks * n;                             // new 16 kHz samples per channel
    const unsigned mask = (unsigned)R - 1u, mask_in = (unsigned)R_in - 1u;
    const float* ring_in = raw + (long)it.slot * NMIC * R_in;
    float* ring = fifo + (long)it.slot * NMIC * R;
    for (int e = tile * RI_NT + tid; e < NMIC * per; e += ntile * RI_NT) {
        const int ch = e >= per ? 1 : 0, j = e - ch * per, q = j / n, p = j - q * n;
        const TapRing tap{ring_in + (long)ch * R_in, it.tap + (unsigned)q * (unsigned)o, mask_in};
        ring[(long)ch * R + ((it.wr + (unsigned)j) & mask)] = resample_dot(tap, bank + p * K, K);
    }
    if (tile == 0 && tid == 0) wr[it.slot] = it.wr + (unsigned)per;
}

constexpr int RO_NT = 256, RO_XS = 1024;       // staged samples per channel: tail + chunk
template <bool S16>
__global__ void __launch_bounds__(RO_NT) k_session_resample_out(const float* __restrict__ out, float* __restrict__ tail,
                                                                const unsigned* __restrict__ hold, void* __restrict__ out_client,
                                                                const float* __restrict__ bank, int o, int n, int width, int T) {
    __shared__ float xs[NSRC][RO_XS];
    const int s = blockIdx.x, tid = threadIdx.x, K = 2 * width + o, hop_c = HOP / o * n, len = T + HOP;
    float* row32 = reinterpret_cast<float*>(out_client) + (long)s * NSRC * hop_c;
    short* row16 = reinterpret_cast<short*>(out_client) + (long)s * NSRC * hop_c;
    if (hold[s] != 0u) {                                       // block-uniform
        for (int e = tid; e < NSRC * hop_c; e += RO_NT) {
            if constexpr (S16) row16[e] = 0;
            else row32[e] = 0.f;
        }
        return;
    }
    float* tl = tail + (long)s * NSRC * T;
    const float* row = out + (long)s * NSRC * HOP;
    for (int i = tid; i < NSRC * len; i += RO_NT) {
        const int ch = i / len, j = i - ch * len;
        xs[ch][j] = j < T ? tl[ch * T + j] : row[ch * HOP + j - T];
    }
    __syncthreads();                                           // the old tail has been read by everyone
    for (int e = tid; e < NSRC * hop_c; e += RO_NT) {
        const int ch = e / hop_c, j = e - ch * hop_c, q = j / n, p = j - q * n;
        const float v = resample_dot(TapSpan{xs[ch] + q * o}, bank + p * K, K);
        if constexpr (S16) row16[e] = (short)emit_s16(v);
        else row32[e] = v;
    }
    for (int i = tid; i < NSRC * T; i += RO_NT) {
        const int ch = i / T, j = i - ch * T;
        tl[i] = xs[ch][HOP + j];
    }
}

// Any rate (ABI 31): the out node where o does not divide 128 (44.1 kHz: o = 160, n = 441) — a FRACTIONAL hop.  A period of
// P = o / gcd(128, o) live steps consumes 128 P samples, a whole number of blocks, and makes 128 P n / o outputs; the step at
// phase r of its slot emits outputs [c(r), c(r + 1)) of the period, c(r) = floor(128 r n / o): floor or ceil of 128 n / o of
// them, counted here and mirrored by the host in the same integers.  Output m = q n + p reads the K taps that start at 16 kHz
// sample q o - width - d of the period, d = width + o - 1 the fixed delay: in [tail | row], T = K + o + ceil(o / n) - 1 carried
// samples and the 128 new ones (the row starts at sample 128 r of the period), that is index q o - 128 r + T - width - d.  For
// r < P and m in [c(r), c(r + 1)):  128 r - (o - 1) <= q o <= 128 r + 127, so the K taps lie in [T - K - o + 2, T + 128).
// One workgroup per slot; a thread makes BOTH channels of its outputs from one read of the bank, which is the transposed
// image [K][n]: the 64 outputs of a wave have consecutive phases p (wrapping at n once at most), so a tap is 64 consecutive
// floats, and the outputs of one block q share their LDS address (a broadcast).  The slot's phase word, count word and tail
// have this workgroup as their one writer.
// 512 threads: the 353 outputs of a 44.1 kHz step are one round, and a thread's chain of K dependent fmaf is the kernel's length
constexpr int RA_NT = 512, RA_XS = 1427;       // staged samples per channel: what 11 025 Hz needs, T = 1299 and the chunk
template <bool S16>
__global__ void __launch_bounds__(RA_NT) k_session_resample_out_any(const float* __restrict__ out, float* __restrict__ tail,
                                                                    unsigned* __restrict__ phase, const unsigned* __restrict__ hold,
                                                                    void* __restrict__ out_client, int* __restrict__ count,
                                                                    const float* __restrict__ bank_t, int o, int n, int width,
                                                                    int T, int P, int Q, int hop_max) {
    static_assert(NSRC == 2, "resample_dot2_t makes the two channels of an output");
    __shared__ float xs[NSRC][RA_XS];
    const int s = blockIdx.x, tid = threadIdx.x, K = 2 * width + o, len = T + HOP;
    float* row32 = reinterpret_cast<float*>(out_client) + (long)s * NSRC * hop_max;
    short* row16 = reinterpret_cast<short*>(out_client) + (long)s * NSRC * hop_max;
    if (hold[s] != 0u) {                                       // block-uniform: a zero row, count 0, tail and phase stay
        for (int e = tid; e < NSRC * hop_max; e += RA_NT) {
            if constexpr (S16) row16[e] = 0;
            else row32[e] = 0.f;
        }
        if (tid == 0) count[s] = 0;
        return;
    }
    const int r = (int)(phase[s] % (unsigned)P);               // whatever the word holds: r < P before any index is formed
    // c(r) = 128 r n / o = Q r n / P with Q = 128 / gcd(128, o): Q (r + 1) n <= 128 * 4096 * 4096 = 2^31, unsigned 32-bit
    const unsigned Qn = (unsigned)Q * (unsigned)n;
    const int c0 = (int)(Qn * (unsigned)r / (unsigned)P), cnt = (int)(Qn * (unsigned)(r + 1) / (unsigned)P) - c0;
    float* tl = tail + (long)s * NSRC * T;
    const float* row = out + (long)s * NSRC * HOP;
    for (int i = tid; i < NSRC * len; i += RA_NT) {
        const int ch = i / len, j = i - ch * len;
        xs[ch][j] = j < T ? tl[ch * T + j] : row[ch * HOP + j - T];
    }
    __syncthreads();                                           // the old tail and the phase word have been read by everyone
    const int base0 = T - 2 * width - o + 1 - HOP * r;
    for (int j = tid; j < hop_max; j += RA_NT) {
        float v0 = 0.f, v1 = 0.f;                              // at and beyond the count: zeros
        if (j < cnt) {
            const int m = c0 + j, q = m / n, p = m - q * n, base = base0 + q * o;
            resample_dot2_t(TapSpan{xs[0] + base}, TapSpan{xs[1] + base}, bank_t + p, n, K, v0, v1);
        }
        if constexpr (S16) {
            row16[j] = (short)emit_s16(v0);
            row16[hop_max + j] = (short)emit_s16(v1);
        } else {
            row32[j] = v0;
            row32[hop_max + j] = v1;
        }
    }
    for (int i = tid; i < NSRC * T; i += RA_NT) {
        const int ch = i / T, j = i - ch * T;
        tl[i] = xs[ch][HOP + j];
    }
    if (tid == 0) {
        phase[s] = r + 1 == P ? 0u : (unsigned)(r + 1);
        count[s] = cnt;
    }
}

}  // namespace lh

extern "C" int lh_intra_stream(const float* x, const void* wih_pk, const float* b_sum, const float* whh, float* h_out,
                               int n_frames, lh_stream_t stream) {
    using namespace lh;
    if (!x || !wih_pk || !b_sum || !whh || !h_out || n_frames <= 0) return LH_ERR_ARG;
    hipLaunchKernelGGL(k_intra_stream, dim3(2 * n_frames), dim3(IS_NT), 0, (hipStream_t)stream, x, (const _Float16*)wih_pk,
                       b_sum, whh, h_out, n_frames);
    return check_launch();
}

extern "C" int lh_inter_matvec_win(const float* x, const void* wih_pk, const float* b_sum, const float* whh, const void* wlin_pk,
                                   const float* blin, const float* h0, const float* c0, float* hN, float* cN, float* out,
                                   int B, int T, int t0, int Tc, int carry, lh_stream_t stream) {
    using namespace lh;
    if (!x || !wih_pk || !b_sum || !whh || !wlin_pk || !blin || !h0 || !c0 || !hN || !cN || !out || B <= 0 || T <= 0)
        return LH_ERR_ARG;
    if (h0 == hN || c0 == cN || x == out || t0 < 0 || Tc <= 0 || t0 + Tc > T || (carry & ~3)) return LH_ERR_ARG;
    hipLaunchKernelGGL(k_inter_matvec, dim3(B * NF), dim3(IS_NT), 0, (hipStream_t)stream, x, (const _Float16*)wih_pk, b_sum,
                       whh, (const _Float16*)wlin_pk, blin, h0, c0, hN, cN, out, Tc, T, t0, carry);
    return check_launch();
}

extern "C" int lh_inter_matvec(const float* x, const void* wih_pk, const float* b_sum, const float* whh, const void* wlin_pk,
                               const float* blin, const float* h0, const float* c0, float* hN, float* cN, float* out,
                               int B, int T, lh_stream_t stream) {
    return lh_inter_matvec_win(x, wih_pk, b_sum, whh, wlin_pk, blin, h0, c0, hN, cN, out, B, T, 0, T, 0, stream);
}

namespace lh {
static bool sess_spans(const lh_span_t* spans, int n_spans, SessSpans& sp) {
    if (!spans || n_spans < 1 || n_spans > LH_SESSION_MAX_SPANS) return false;
    sp = SessSpans{};
    for (int i = 0; i < n_spans; ++i) {
        if (!spans[i].base || ((unsigned long long)(size_t)spans[i].base & 15) || !spans[i].bytes || (spans[i].bytes & 15))
            return false;
        sp.s[i] = spans[i];
    }
    sp.n = n_spans;
    return true;
}
// Tiles of the begin and move kernels per row launched.  ~10 MB of state per slot, mostly rings: enough tiles that one RESET is
// microseconds (64 workgroups zero a slot in ~13 us), few enough that the idle launch of a large batch stays a handful of
// early-out workgroups per CU
static int sess_tiles(int n) { return n <= 16 ? 64 : (n >= 64 ? 16 : 1024 / n); }
}  // namespace lh

extern "C" int lh_session_begin(const lh_span_t* spans, int n_spans, const float* chunk_in, float* chunk, const unsigned* cmd,
                                const unsigned* active, int S, lh_stream_t stream) {
    using namespace lh;
    SessSpans sp;
    if (!chunk_in || !chunk || chunk_in == chunk || !cmd || !active || S <= 0 || !sess_spans(spans, n_spans, sp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_begin<false, false>), dim3(sess_tiles(S), S), dim3(SS_NT), 0, (hipStream_t)stream, sp,
                       chunk_in, chunk, cmd, active, (const int*)nullptr, (const unsigned*)nullptr, (const int*)nullptr,
                       (int*)nullptr, S);
    return check_launch();
}

extern "C" int lh_session_end(const lh_span_t* spans, int n_spans, const float* chunk_in, float* out, unsigned* cmd,
                              unsigned* active, unsigned* fault, int S, lh_stream_t stream) {
    using namespace lh;
    SessSpans sp;
    if (!chunk_in || !out || !cmd || !active || !fault || S <= 0 || n_spans > SE_SP || !sess_spans(spans, n_spans, sp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_end<false, false>), dim3(S), dim3(SE_NT), 0, (hipStream_t)stream, sp, SessSpans{}, chunk_in,
                       (const float*)out, out, cmd, active, fault, (const unsigned*)nullptr, (const int*)nullptr,
                       (const int*)nullptr, (int*)nullptr, S, S);
    return check_launch();
}

extern "C" int lh_session_move(const lh_span_t* spans, int n_spans, const int* from, unsigned* cmd, unsigned* active, int n_rows,
                               int S, lh_stream_t stream) {
    using namespace lh;
    SessSpans sp;
    if (!from || !cmd || !active || S <= 0 || n_rows < 1 || n_rows > S || !sess_spans(spans, n_spans, sp)) return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_move<false>), dim3(sess_tiles(n_rows), n_rows), dim3(SS_NT), 0, (hipStream_t)stream, sp, from,
                       cmd, active, (int*)nullptr, S);
    return check_launch();
}

extern "C" int lh_session_begin_rows(const lh_span_t* spans, int n_spans, const float* chunk_in, float* chunk,
                                     const unsigned* cmd, const unsigned* active, const int* slot_of, int n_rows, int S,
                                     lh_stream_t stream) {
    using namespace lh;
    SessSpans sp;
    if (!chunk_in || !chunk || chunk_in == chunk || !cmd || !active || !slot_of || S <= 0 || n_rows < 1 || n_rows > S ||
        !sess_spans(spans, n_spans, sp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_begin<true, false>), dim3(sess_tiles(n_rows), n_rows), dim3(SS_NT), 0, (hipStream_t)stream, sp,
                       chunk_in, chunk, cmd, active, slot_of, (const unsigned*)nullptr, (const int*)nullptr, (int*)nullptr, S);
    return check_launch();
}

extern "C" int lh_session_end_rows(const lh_span_t* spans, int n_spans, const float* chunk_in, const float* out_rows, float* out,
                                   unsigned* cmd, unsigned* active, unsigned* fault, const int* slot_of, const int* row_of,
                                   int* from, int n_rows, int S, lh_stream_t stream) {
    using namespace lh;
    SessSpans sp;
    if (!chunk_in || !out_rows || !out || out_rows == out || !cmd || !active || !fault || !slot_of || !row_of || S <= 0 ||
        n_rows < 1 || n_rows > S || n_spans > SE_SP || !sess_spans(spans, n_spans, sp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_end<true, false>), dim3(n_rows + 1), dim3(SE_NT), 0, (hipStream_t)stream, sp, SessSpans{},
                       chunk_in, out_rows, out, cmd, active, fault, (const unsigned*)nullptr, slot_of, row_of, from, n_rows, S);
    return check_launch();
}

extern "C" int lh_session_capture(const float* chunk_in, float* enroll, unsigned* ecmd, unsigned* estate, unsigned* edone,
                                  int n_chunks, int S, lh_stream_t stream) {
    using namespace lh;
    if (!chunk_in || !enroll || !ecmd || !estate || !edone || S <= 0 || n_chunks < 1) return LH_ERR_ARG;
    if (((unsigned long long)(size_t)enroll & 15) || ((unsigned long long)(size_t)chunk_in & 15)) return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_capture<false>), dim3(S), dim3(SC_NT), 0, (hipStream_t)stream, chunk_in, enroll, ecmd, estate,
                       edone, (const unsigned*)nullptr, n_chunks, S);
    return check_launch();
}

// ---- paced sessions (ABI 19) ------------------------------------------------------------------------------------------------
namespace lh {
// the carry table of lh_session_end_paced: n_pairs x (read, written), equal sizes
static bool sess_pairs(const lh_span_t* carry, int n_pairs, SessSpans& cp) {
    if (n_pairs < 1 || 2 * n_pairs > LH_SESSION_MAX_SPANS || !sess_spans(carry, 2 * n_pairs, cp)) return false;
    for (int i = 0; i < n_pairs; ++i)
        if (carry[2 * i].bytes != carry[2 * i + 1].bytes || carry[2 * i].base == carry[2 * i + 1].base) return false;
    return true;
}
}  // namespace lh

extern "C" int lh_session_begin_paced(const lh_span_t* spans, int n_spans, const float* chunk_in, float* chunk,
                                      const unsigned* cmd, const unsigned* active, const unsigned* hold, const int* pos,
                                      int* write_pos, int S, lh_stream_t stream) {
    using namespace lh;
    SessSpans sp;
    if (!chunk_in || !chunk || chunk_in == chunk || !cmd || !active || !hold || !pos || !write_pos || pos == write_pos ||
        S <= 0 || !sess_spans(spans, n_spans, sp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_begin<false, true>), dim3(sess_tiles(S), S), dim3(SS_NT), 0, (hipStream_t)stream, sp, chunk_in,
                       chunk, cmd, active, (const int*)nullptr, hold, pos, write_pos, S);
    return check_launch();
}

extern "C" int lh_session_begin_rows_paced(const lh_span_t* spans, int n_spans, const float* chunk_in, float* chunk,
                                           const unsigned* cmd, const unsigned* active, const int* slot_of,
                                           const unsigned* hold, const int* pos, int* write_pos, int n_rows, int S,
                                           lh_stream_t stream) {
    using namespace lh;
    SessSpans sp;
    if (!chunk_in || !chunk || chunk_in == chunk || !cmd || !active || !slot_of || !hold || !pos || !write_pos ||
        pos == write_pos || S <= 0 || n_rows < 1 || n_rows > S || !sess_spans(spans, n_spans, sp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_begin<true, true>), dim3(sess_tiles(n_rows), n_rows), dim3(SS_NT), 0, (hipStream_t)stream, sp,
                       chunk_in, chunk, cmd, active, slot_of, hold, pos, write_pos, S);
    return check_launch();
}

extern "C" int lh_session_end_paced(const lh_span_t* spans, int n_spans, const lh_span_t* carry, int n_pairs,
                                    const float* chunk_in, float* out, unsigned* cmd, unsigned* active, unsigned* fault,
                                    const unsigned* hold, int S, lh_stream_t stream) {
    using namespace lh;
    SessSpans sp, cp;
    if (!chunk_in || !out || !cmd || !active || !fault || !hold || S <= 0 || n_spans > SE_SP || !sess_spans(spans, n_spans, sp) ||
        !sess_pairs(carry, n_pairs, cp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_end<false, true>), dim3(S), dim3(SE_NT), 0, (hipStream_t)stream, sp, cp, chunk_in,
                       (const float*)out, out, cmd, active, fault, hold, (const int*)nullptr, (const int*)nullptr, (int*)nullptr, S, S);
    return check_launch();
}

extern "C" int lh_session_end_rows_paced(const lh_span_t* spans, int n_spans, const lh_span_t* carry, int n_pairs,
                                         const float* chunk_in, const float* out_rows, float* out, unsigned* cmd,
                                         unsigned* active, unsigned* fault, const unsigned* hold, const int* slot_of,
                                         const int* row_of, int* from, int n_rows, int S, lh_stream_t stream) {
    using namespace lh;
    SessSpans sp, cp;
    if (!chunk_in || !out_rows || !out || out_rows == out || !cmd || !active || !fault || !hold || !slot_of || !row_of ||
        S <= 0 || n_rows < 1 || n_rows > S || n_spans > SE_SP || !sess_spans(spans, n_spans, sp) ||
        !sess_pairs(carry, n_pairs, cp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_end<true, true>), dim3(n_rows + 1), dim3(SE_NT), 0, (hipStream_t)stream, sp, cp, chunk_in,
                       out_rows, out, cmd, active, fault, hold, slot_of, row_of, from, n_rows, S);
    return check_launch();
}

extern "C" int lh_session_move_paced(const lh_span_t* spans, int n_spans, const int* from, unsigned* cmd, unsigned* active,
                                     int* pos, int n_rows, int S, lh_stream_t stream) {
    using namespace lh;
    SessSpans sp;
    if (!from || !cmd || !active || !pos || S <= 0 || n_rows < 1 || n_rows > S || !sess_spans(spans, n_spans, sp))
        return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_move<true>), dim3(sess_tiles(n_rows), n_rows), dim3(SS_NT), 0, (hipStream_t)stream, sp, from,
                       cmd, active, pos, S);
    return check_launch();
}

extern "C" int lh_session_capture_paced(const float* chunk_in, float* enroll, unsigned* ecmd, unsigned* estate, unsigned* edone,
                                        const unsigned* hold, int n_chunks, int S, lh_stream_t stream) {
    using namespace lh;
    if (!chunk_in || !enroll || !ecmd || !estate || !edone || !hold || S <= 0 || n_chunks < 1) return LH_ERR_ARG;
    if (((unsigned long long)(size_t)enroll & 15) || ((unsigned long long)(size_t)chunk_in & 15)) return LH_ERR_ARG;
    hipLaunchKernelGGL((k_session_capture<true>), dim3(S), dim3(SC_NT), 0, (hipStream_t)stream, chunk_in, enroll, ecmd, estate,
                       edone, hold, n_chunks, S);
    return check_launch();
}

// ---- suspend / resume (ABI 20) ----------------------------------------------------------------------------------------------
namespace lh {
static bool aligned16(const void* p) { return p && !((unsigned long long)(size_t)p & 15); }
// the two tables, the ring geometry and the snapshot buffer of lh_session_save / lh_session_restore
static bool snap_layout(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads, int ring_rows,
                        int window, const void* embed, int embed_bytes, const void* snap, unsigned long long snap_bytes,
                        int row, int S, SnapLayout& L) {
    L = SnapLayout{};
    if (!sess_spans(flat, n_flat, L.flat) || n_rings > LH_SNAPSHOT_MAX_RINGS || !sess_spans(rings, n_rings, L.rings)) return false;
    if (8 + n_flat + n_rings > LH_SNAPSHOT_HEADER_BYTES / 4) return false;
    if (heads < 1 || window < 1 || ring_rows < window || embed_bytes < 16 || (embed_bytes & 15)) return false;
    if (!aligned16(embed) || !aligned16(snap) || S <= 0 || row < 0 || row >= S) return false;
    L.heads = heads, L.rows = ring_rows, L.window = window, L.embed_bytes = (unsigned)embed_bytes;
    unsigned long long total = SNAP_EMBED + L.embed_bytes;
    for (int i = 0; i < n_flat; ++i) {
        if (flat[i].bytes >> 31) return false;
        total += flat[i].bytes;
    }
    for (int i = 0; i < n_rings; ++i) {
        if (rings[i].bytes >> 31 || snap_ring_bytes(L, i) >> 31) return false;
        total += snap_ring_bytes(L, i);
    }
    return total == snap_offset(L, n_flat + n_rings) && !(total >> 31) && snap_bytes >= total;
}
}  // namespace lh

extern "C" int lh_session_save(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads, int ring_rows,
                               int window, const void* embed, int embed_bytes, void* snap, unsigned long long snap_bytes,
                               const unsigned* cmd, const unsigned* active, const int* pos, int row, int S, lh_stream_t stream) {
    using namespace lh;
    SnapLayout L;
    if (!cmd || !active || !pos ||
        !snap_layout(flat, n_flat, rings, n_rings, heads, ring_rows, window, embed, embed_bytes, snap, snap_bytes, row, S, L))
        return LH_ERR_ARG;
    hipLaunchKernelGGL(k_session_save, dim3(SNAP_TILES, n_flat + n_rings + 1), dim3(SNAP_NT), 0, (hipStream_t)stream, L,
                       (const float4*)embed, (char*)snap, cmd, active, pos, row, S);
    return check_launch();
}

extern "C" int lh_session_restore(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads,
                                  int ring_rows, int window, void* embed, int embed_bytes, const void* snap,
                                  unsigned long long snap_bytes, unsigned* cmd, int* pos_row, const int* pos_shared,
                                  unsigned* fault, int gen, int row, int S, lh_stream_t stream) {
    using namespace lh;
    SnapLayout L;
    if (!cmd || !fault || !pos_row == !pos_shared || gen < 1 || gen > 0x7fffff ||
        !snap_layout(flat, n_flat, rings, n_rings, heads, ring_rows, window, embed, embed_bytes, snap, snap_bytes, row, S, L))
        return LH_ERR_ARG;
    hipLaunchKernelGGL(k_session_restore, dim3(SNAP_TILES, n_flat + n_rings + 1), dim3(SNAP_NT), 0, (hipStream_t)stream, L,
                       (float4*)embed, (const char*)snap, cmd, pos_row, pos_shared, fault, (unsigned)gen, row, S);
    return check_launch();
}

// ---- suspend / resume of many listeners (ABI 21) ----------------------------------------------------------------------------
namespace lh {
// Tiles per (item, section): SNAP_TILES, what the single kernels use, whatever the number of items.  With 64 items in flight
// that is some 50 000 workgroups, most of them with less than one 16 KB pass to copy, and it is still the count to keep:
// measured at S = 64, k = 64 (profiles/suspend_many_cost.txt), 4 to 64 tiles cost the same within the run's scatter — park
// +619 to +666 us, return +484 to +497 us — and 2 tiles cost 110 to 150 us more.  lh_set_tuning(18, n) sets another count for such
// A/B runs; 0 = SNAP_TILES.
static int g_snap_tiles = 0;
int snap_set_tiles(int v) {
    if (v < 0 || v > 1024) return LH_ERR_ARG;
    g_snap_tiles = v;
    return LH_OK;
}
static int snap_tiles() { return g_snap_tiles ? g_snap_tiles : SNAP_TILES; }
static bool snap_rows_args(unsigned long long snap_stride, const void* pos_rows, const void* pos_shared, const void* items,
                           int n_items, int S) {
    return !(snap_stride & 15) && !pos_rows != !pos_shared && items && !((unsigned long long)(size_t)items & 3) && n_items >= 1 &&
           n_items <= S;
}
}  // namespace lh

extern "C" int lh_session_save_rows(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads,
                                    int ring_rows, int window, const void* embed, int embed_bytes, void* snaps,
                                    unsigned long long snap_stride, const unsigned* cmd, const unsigned* active,
                                    const int* pos_rows, const int* pos_shared, const lh_snap_item_t* items, int n_items, int S,
                                    lh_stream_t stream) {
    using namespace lh;
    SnapLayout L;
    if (!cmd || !active ||
        !snap_layout(flat, n_flat, rings, n_rings, heads, ring_rows, window, embed, embed_bytes, snaps, snap_stride, 0, S, L) ||
        !snap_rows_args(snap_stride, pos_rows, pos_shared, items, n_items, S))
        return LH_ERR_ARG;
    hipLaunchKernelGGL(k_session_save_rows, dim3(snap_tiles(), n_flat + n_rings + 1, n_items), dim3(SNAP_NT), 0,
                       (hipStream_t)stream, L, (const char*)embed, (char*)snaps, snap_stride, cmd, active, pos_rows, pos_shared,
                       items, S);
    return check_launch();
}

extern "C" int lh_session_restore_rows(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads,
                                       int ring_rows, int window, void* embed, int embed_bytes, const void* snaps,
                                       unsigned long long snap_stride, unsigned* cmd, int* pos_rows, const int* pos_shared,
                                       unsigned* fault, const lh_snap_item_t* items, int n_items, int S, lh_stream_t stream) {
    using namespace lh;
    SnapLayout L;
    if (!cmd || !fault ||
        !snap_layout(flat, n_flat, rings, n_rings, heads, ring_rows, window, embed, embed_bytes, snaps, snap_stride, 0, S, L) ||
        !snap_rows_args(snap_stride, pos_rows, pos_shared, items, n_items, S))
        return LH_ERR_ARG;
    hipLaunchKernelGGL(k_session_restore_rows, dim3(snap_tiles(), n_flat + n_rings + 1, n_items), dim3(SNAP_NT), 0,
                       (hipStream_t)stream, L, (char*)embed, (const char*)snaps, snap_stride, cmd, pos_rows, pos_shared, fault,
                       items, S);
    return check_launch();
}

// ---- packets (ABI 22) ---------------------------------------------------------------------------------------------------------
namespace lh {
static bool aligned_to(const void* p, unsigned a) { return p && !((unsigned long long)(size_t)p & (a - 1u)); }
static bool fifo_args(const void* fifo, const void* wr, const void* rd, int R, int S) {
    return aligned16(fifo) && aligned_to(wr, 4) && aligned_to(rd, 4) && wr != rd && S > 0 && R >= 256 && R <= (1 << 24) &&
           !(R & (R - 1));
}
}  // namespace lh

extern "C" int lh_session_feed(const void* staging, unsigned long long staging_bytes, int format, const lh_feed_item_t* items,
                               int n_items, float* fifo, unsigned* wr, unsigned* rd, int R, int S, lh_stream_t stream) {
    using namespace lh;
    if ((format != LH_FEED_F32 && format != LH_FEED_S16) || !aligned_to(staging, 4) || !aligned_to(items, 4) || n_items < 1 ||
        n_items > 65535 || !fifo_args(fifo, wr, rd, R, S))
        return LH_ERR_ARG;
    // a packet is a few hundred samples: tiles enough for an item that fills the ring, a handful of early-out workgroups else
    const int want = NMIC * R / (4 * SF_NT), tiles = want < 1 ? 1 : (want > SF_MAX_TILES ? SF_MAX_TILES : want);
    if (format == LH_FEED_S16)
        hipLaunchKernelGGL(k_session_feed<short>, dim3(tiles, n_items), dim3(SF_NT), 0, (hipStream_t)stream,
                           (const short*)staging, staging_bytes / 2, items, (unsigned*)fifo, wr, rd, R, S);
    else
        hipLaunchKernelGGL(k_session_feed<unsigned>, dim3(tiles, n_items), dim3(SF_NT), 0, (hipStream_t)stream,
                           (const unsigned*)staging, staging_bytes / 4, items, (unsigned*)fifo, wr, rd, R, S);
    return check_launch();
}

extern "C" int lh_session_frame(const float* fifo, const unsigned* wr, unsigned* rd, float* chunk_in, unsigned* hold, int R, int S,
                                lh_stream_t stream) {
    using namespace lh;
    if (!aligned16(chunk_in) || !aligned_to(hold, 4) || !fifo_args(fifo, wr, rd, R, S)) return LH_ERR_ARG;
    hipLaunchKernelGGL(k_session_frame, dim3(S), dim3(SC_NT), 0, (hipStream_t)stream, fifo, wr, rd, chunk_in, hold, R, S);
    return check_launch();
}

extern "C" int lh_session_emit_s16(const float* out, short* out16, int S, lh_stream_t stream) {
    using namespace lh;
    if (!aligned16(out) || !aligned16(out16) || (const void*)out == (const void*)out16 || S <= 0) return LH_ERR_ARG;
    const int n8 = S * NSRC * HOP / 8;
    hipLaunchKernelGGL(k_session_emit_s16, dim3((n8 + SS_NT - 1) / SS_NT), dim3(SS_NT), 0, (hipStream_t)stream,
                       (const float4*)out, (int4*)out16, n8);
    return check_launch();
}

// ---- client rate (ABI 23) -----------------------------------------------------------------------------------------------------
namespace lh {
// carried 16 kHz samples of the out node: the taps below a step's first block, T = width + D o with D = ceil((width + o) / o)
static int resample_out_tail(int o, int width) { return width + (width + 2 * o - 1) / o * o; }
}  // namespace lh

extern "C" int lh_session_resample_in(const float* raw, int R_in, const lh_resample_item_t* items, int n_items, float* fifo,
                                      unsigned* wr, int R, int S, const float* bank, int o, int n, int width, lh_stream_t stream) {
    using namespace lh;
    const auto ring_ok = [](int r) { return r >= 256 && r <= (1 << 24) && !(r & (r - 1)); };
    if (!aligned16(raw) || !aligned16(fifo) || (const void*)raw == (const void*)fifo || !aligned_to(items, 4) || !aligned_to(wr, 4) ||
        !aligned_to(bank, 4) || n_items < 1 || n_items > 65535 || S <= 0 || !ring_ok(R) || !ring_ok(R_in) ||
        !resample_ratio_ok(o, n, width) || 2 * width + o > R_in)
        return LH_ERR_ARG;
    const int want = NMIC * R / (4 * RI_NT), tiles = want < 1 ? 1 : (want > RI_MAX_TILES ? RI_MAX_TILES : want);
    hipLaunchKernelGGL(k_session_resample_in, dim3(tiles, n_items), dim3(RI_NT), 0, (hipStream_t)stream, raw, R_in, items, fifo, wr,
                       R, S, bank, o, n, width);
    return check_launch();
}

extern "C" int lh_session_resample_out(const float* out, float* tail, const unsigned* hold, void* out_client, int format, int S,
                                       const float* bank, int o, int n, int width, lh_stream_t stream) {
    using namespace lh;
    if ((format != LH_FEED_F32 && format != LH_FEED_S16) || !aligned16(out) || !aligned_to(tail, 4) || !aligned_to(hold, 4) ||
        !aligned16(out_client) || (const void*)out == (const void*)out_client || (const void*)tail == (const void*)out ||
        !aligned_to(bank, 4) || S <= 0 || !resample_ratio_ok(o, n, width) || HOP % o || resample_out_tail(o, width) + HOP > RO_XS)
        return LH_ERR_ARG;
    const int T = resample_out_tail(o, width);
    if (format == LH_FEED_S16)
        hipLaunchKernelGGL(k_session_resample_out<true>, dim3(S), dim3(RO_NT), 0, (hipStream_t)stream, out, tail, hold, out_client,
                           bank, o, n, width, T);
    else
        hipLaunchKernelGGL(k_session_resample_out<false>, dim3(S), dim3(RO_NT), 0, (hipStream_t)stream, out, tail, hold, out_client,
                           bank, o, n, width, T);
    return check_launch();
}

// ---- any rate (ABI 31) --------------------------------------------------------------------------------------------------------
extern "C" int lh_session_resample_out_any(const float* out, float* tail, unsigned* phase, const unsigned* hold, void* out_client,
                                           int* count, int format, int S, const float* bank_t, int o, int n, int width,
                                           lh_stream_t stream) {
    using namespace lh;
    const void* const bufs[] = {out, tail, phase, hold, out_client, count, bank_t};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (bufs[i] == bufs[j]) return LH_ERR_ARG;         // two nulls among them
    if ((format != LH_FEED_F32 && format != LH_FEED_S16) || !aligned16(out) || !aligned16(tail) || !aligned16(out_client) ||
        !aligned_to(phase, 4) || !aligned_to(hold, 4) || !aligned_to(count, 4) || !aligned_to(bank_t, 4) || S <= 0 ||
        !resample_ratio_ok(o, n, width))
        return LH_ERR_ARG;
    int g = HOP, b = o;
    while (b) { const int t = g % b; g = b; b = t; }           // gcd(128, o)
    const int K = 2 * width + o, T = K + o + (o + n - 1) / n - 1, P = o / g, Q = HOP / g;
    const int hop_max = (int)(((long)HOP * n + o - 1) / o);
    if (T + HOP > RA_XS) return LH_ERR_ARG;
    if (format == LH_FEED_S16)
        hipLaunchKernelGGL(k_session_resample_out_any<true>, dim3(S), dim3(RA_NT), 0, (hipStream_t)stream, out, tail, phase, hold,
                           out_client, count, bank_t, o, n, width, T, P, Q, hop_max);
    else
        hipLaunchKernelGGL(k_session_resample_out_any<false>, dim3(S), dim3(RA_NT), 0, (hipStream_t)stream, out, tail, phase, hold,
                           out_client, count, bank_t, o, n, width, T, P, Q, hop_max);
    return check_launch();
}

// ---- monitor mix (ABI 30) -----------------------------------------------------------------------------------------------------
extern "C" int lh_session_mix(const float* chunk_in, float* out, const float* target, float* gain, const unsigned* hold,
                              float step, int S, lh_stream_t stream) {
    using namespace lh;
    if (!aligned16(chunk_in) || !aligned16(out) || (const void*)chunk_in == (const void*)out || !aligned_to(target, 4) ||
        !aligned_to(gain, 4) || (const void*)target == (const void*)gain || (hold && !aligned_to(hold, 4)) || S <= 0 ||
        !(step > 0.f && step <= 1.f))
        return LH_ERR_ARG;
    if (hold)
        hipLaunchKernelGGL((k_session_mix<true>), dim3(S), dim3(SC_NT), 0, (hipStream_t)stream, chunk_in, out, target, gain, hold,
                           step, S);
    else
        hipLaunchKernelGGL((k_session_mix<false>), dim3(S), dim3(SC_NT), 0, (hipStream_t)stream, chunk_in, out, target, gain,
                           (const unsigned*)nullptr, step, S);
    return check_launch();
}
