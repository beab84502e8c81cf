/* lookonce_hip.h — C ABI of the MI355X-native LookOnceToHear separator forward path.
 *
 * Drop-in boundary: the reference selects its model by a dotted string
 * (`utils.import_attr(model)(**model_params)`, reference src/ts_hear_embed_pl_module.py:25 with the string
 * from configs/tsh.json:4).  `lookoncetohear_amd.net.Net` is that class; it owns parameters and streaming
 * state as torch tensors and calls the stateless entry points below with raw device pointers on the current
 * HIP stream.  Conventions (same as the only C-ABI precedent in the reference,
 * src/datasets/motion_simulator.py:41-46): every function returns int, 0 = OK, and the caller asserts.
 *   - all pointers are DEVICE pointers to fp32 unless stated; nothing is allocated or freed here;
 *   - activations are channel-last  X[b][t][f][c]  (B,T,F=97,C=64);
 *   - `*_in` / `*_out` state pairs must not alias (several workgroups read the old state while one writes
 *     the new one);
 *   - shape constants are those of configs/tsh.json (nfft 192, hop 128, F 97, C 64, H 64, heads 4, E 6,
 *     Vd 16, window 50, 2 mics, 2 sources); `lh_check_config` returns LH_ERR_UNSUPPORTED for anything else.
 *
 * Each entry point cites the reference lines it replaces.
 */
#ifndef LOOKONCE_HIP_H
#define LOOKONCE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* lh_stream_t; /* hipStream_t */

enum {
    LH_OK = 0,
    LH_ERR_ARG = 1,         /* null pointer / non-positive size */
    LH_ERR_UNSUPPORTED = 2, /* shape constants differ from the compiled configuration */
    LH_ERR_LAUNCH = 3,      /* hipGetLastError() != hipSuccess after the launch */
    LH_ERR_RANGE = 4        /* lh_range_status only: a non-finite output sample was produced since the caller's last check */
};

/* Range contract of the split-precision ("f16x3") arithmetic.  Operands are carried as fp16 hi + fp16 lo, so every value
 * a kernel SPLITS must satisfy |v| < 65504 AFTER the kernel's own scaling.  LayerNorm outputs, hidden states, attention
 * rows and weights always do.  The kernels that read un-normalised data (the waveform in lh_stft_conv_in, the residual
 * stream in lh_qkv_proj_ln and lh_deconv_istft) multiply each row / tile by an exact power of two chosen from its own
 * maximum before the split and undo it after the fp32 accumulation (since ABI 12), so any finite fp32 input whose exact
 * result is finite in fp32 is computed to the same ~22 bits relative to the row maximum — the reference's behaviour
 * (plain fp32, tfgridnet_causal.py:188-283).  What remains is a GUARD for non-finite data: lh_deconv_istft raises a
 * CALLER-OWNED flag for a non-finite output sample and stores it as the caller asks (`keep_nonfinite`, ABI 13: as it is —
 * the reference's behaviour, the default of the offline host — or as 0 for a listener):
 *   range_flag       two 32-bit words of DEVICE-ACCESSIBLE memory (device memory, or pinned host memory the caller reads
 *                    directly — the streaming host does that and needs no polling launch at all), zero-initialised by the
 *                    caller: [0] = sticky word lh_deconv_istft sets to 1 with a system-scope store (NULL = no reporting),
 *                    [1] = the value the last fetch took out of [0].  Each Net / Streamer / host thread owns its own, so
 *                    concurrent forwards on one device cannot consume or clear one another's flag (ABI <= 11 kept one
 *                    word per device).
 *   lh_range_status: [1] = atomicExch([0], 0) on `stream`, copies [1] to the host, WAITS for the stream; LH_OK, or
 *                    LH_ERR_RANGE when it was set.  The one entry point that synchronises: call it once per forward.
 *   lh_range_flag_copy: the same exchange followed by an asynchronous copy of [1] to `host_pinned` (4 bytes of pinned host
 *                    memory) on `stream`, no wait (the streaming host looks at the word when later chunks arrive).
 *   lh_range_flag_clear: asynchronous clear of both words on `stream`.
 *   lh_selftest_fp16_subnormal: runs one v_mfma_f32_16x16x32_f16 on fp16-subnormal operands (the un-rescaled lo halves
 *                    rely on the matrix core taking them at full value); LH_OK, or LH_ERR_UNSUPPORTED when they are
 *                    flushed.  Synchronises. */
int lh_range_status(unsigned* range_flag, lh_stream_t stream);
int lh_range_flag_copy(unsigned* range_flag, void* host_pinned, lh_stream_t stream);
int lh_range_flag_clear(unsigned* range_flag, lh_stream_t stream);
int lh_selftest_fp16_subnormal(lh_stream_t stream);

/* Contraction arithmetic of the recurrent kernels (argument `mode`):
 *   LH_GEMM_F32   exact fp32 MFMA (v_mfma_f32_16x16x4_f32); w_pk = fp32 image  [dirs][4][4][32][64]
 *   LH_GEMM_F16X3 split precision: each fp32 operand = fp16 hi + fp16 lo, three fp16 MFMAs
 *                 (hi*hi, hi*lo, lo*hi) accumulated in fp32 (~22 mantissa bits).  Every split-precision image and
 *                 row of every entry point stores lo = fp16(v - hi), NOT rescaled (fp16 subnormals go through the
 *                 matrix core at full value, lh_selftest_fp16_subnormal checks it): the recurrent kernels since ABI 6,
 *                 the other separator kernels since ABI 9, the embedder entry points (lh_emb_*) since ABI 10;
 *                 w_pk = fp16 image [dirs][4 waves][4 gates][4 ksteps][64 lanes][hi 8 | lo 8] (lo unscaled) of
 *                 [W_ih * ln_w | W_hh] and b_sum = b_ih + b_hh + W_ih ln_b, rows of both scaled by the exponent factor of their gate (-log2 e for i, f, o;
 *                 -2 log2 e for g: weights.py gate_prescale). The LayerNorm affine is folded into
 *                 the image (weights.py pack_block), the kernel only standardises x; ln_w/ln_b are ignored  */
enum { LH_GEMM_F32 = 0, LH_GEMM_F16X3 = 1 };

/* ABI version of this header (32); bumped on any signature or buffer-contract change (29: the LayerNorm eps behind the bias
 * of lh_qkv_proj_ln*, lh_proj_ln_res*, lh_emb_attn_block and lh_emb_head, below; 32: streaming chunks of several frames —
 * ring_pos of lh_qkv_proj_ln* for T <= 16, lh_local_attn_ring, lh_ring_advance_by). */
int lh_abi_version(void);

/* Launch-shape tuning knobs (benchmark A/B only; 0 = automatic): key 0 = sequences-per-workgroup/16 of the
 * intra LSTM, key 1 = same for the inter LSTM, key 2 = fused intra kernel (0 = k_intra_xp, the hand-ordered
 * software-pipelined step; 2 = the previous k_ln_lstm_lin), key 3 = 0 switches off the issue-priority de-phasing of
 * the two workgroups that share a CU in k_ln_lstm_lin (default on), key 4 = query frames per attention workgroup
 * (1 / 2 = tiles of 16, 3 = 40 frames in three tiles, 5 = 79 frames in five; 0 = automatic; 4 is refused), key 5 = fused inter kernel (0 = k_inter_xp,
 * the hand-ordered step with per-phase issue priority; 2 = the previous k_lstm_lin8p), key 6 = runs of consecutive tiles per utterance in
 * lh_deconv_istft (0 = automatic: 256 / B), key 7 = bytes of dynamic LDS added to k_intra_xp launches (timing probe:
 * one workgroup per CU), key 8 = issue priority in k_intra_xp (0 = none, 1 = static priority for the odd wave slot of a SIMD: default, 2 / 3 =
 * every wave raised during the on-chain / off-chain phase of the step), key 9 = issue priority in k_inter_xp (0 = none,
 * 1 / 2 = the LayerNorm / projection waves, 3 = every wave during the on-chain phase: default, 4 = off-chain phase; + 16 = the
 * two roles on the other four waves: A/B only, 6-8 % slower),
 * key 16 = issue priority for the on-chain MFMAs of the embedder's recurrent kernel k_emb_rec (0 = off: default, 1 = on),
 * key 19 = cache policy of the frame kernels' once-touched streams (csrc/lh_cachepol.h): 0 = plain accesses always, 1 = non-temporal
 * when the launch's frame stream is at least 256 MiB (default), 2 = at any size — in the launches that have a policy at all:
 * lh_qkv_proj_ln_rows and the one-tile attention shape (clips of at most 16 frames, or key 4 = 1) are streaming paths and run
 * plain accesses under every value; outputs do not depend on the key; other values: LH_ERR_ARG. */
int lh_set_tuning(int key, int value);

/* Query frames per attention workgroup (16, 32, 40 or 79) that lh_local_attn / lh_local_attn_win use for a whole clip of
 * T frames at batch B under the current key 4: *frames (a host word).  A time window whose t0 is a multiple of it is cut
 * into the tiles of the whole-clip launch, and its outputs are then the whole-clip launch's bit for bit. */
int lh_attn_tile_frames(int B, int T, int* frames);

/* Validates model_params (reference net.py:21-49 / configs/tsh.json:5-19) against the compiled constants. */
int lh_check_config(int nfft, int hop, int n_mics, int emb_dim, int n_blocks_unused, int lstm_hidden,
                    int n_heads, int attn_window, int n_srcs, int spk_emb_dim);

/* A.1  STFT analysis + re/im channel split + causal 3x3 Conv2d(4->64).
 * Replaces tfgridnet_causal.py:229-242 (asteroid Encoder conv1d, cat/transpose, conv_buf halo, self.conv).
 *   x            [B][2][n_samples]                 n_samples = 128*T + 64
 *   conv_buf_in  [B][4][2][97]   conv_buf_out same shape (last two frames of the halo-extended spectrum)
 *   wfb_pk       split-precision B image [13 tiles][6 ksteps][64 lanes][hi 8 | lo 8] of enc.filterbank._filters
 *                [194 rows -> 208][192 samples]
 *   wconv_pk     split-precision B image [4 tiles][2 ksteps][64 lanes][hi 8 | lo 8] of conv.0.weight as [64 channels]
 *                x [K = 64]:  k = 16 kf + 4 kt + ch  (kf, kt < 3, ch < 4), zero elsewhere  (weights.py pack_all);
 *                bconv [64]
 *   z            [B][T][97][64]  out
 */
int lh_stft_conv_in(const float* x, const float* conv_buf_in, float* conv_buf_out, const void* wfb_pk,
                    const void* wconv_pk, const float* bconv, float* z, int B, int T, int n_samples,
                    lh_stream_t stream);

/* A.2  speaker gain  g = LayerNorm_6208(W e + b)  stored f-major:  gain[b][f][c] = g[b][c*97+f].
 * Replaces tfgridnet_causal.py:247-248 (embed_to_feats_proj + reshape).
 *   emb [B][256]; w [6208][256]; bias, ln_w, ln_b [6208]; scratch [B][6208] (raw projection, workspace);
 *   gain [B][97][64] out
 */
int lh_embed_proj_ln(const float* emb, const float* w, const float* bias, const float* ln_w, const float* ln_b,
                     float* scratch, float* gain, int B, lh_stream_t stream);

/* A.3.1  intra-frame path: LayerNorm(C) -> BiLSTM over frequency (zero initial state) ; hidden states only.
 * Replaces tfgridnet_causal.py:505-512 (intra_norm, intra_rnn).
 *   x      [B*T][97][64]
 *   ln_w/b [64]
 *   w_pk   [2 dirs][4 waves][4 gates][32 ksteps][64 lanes]  MFMA B-operand image of [W_ih | W_hh]^T (see
 *          lookoncetohear_amd/weights.py: pack_lstm);  b_sum [2][256] = bias_ih + bias_hh
 *   h_out  [B*T*97][128]   (forward hidden in cols 0..63, reverse in 64..127)
 */
int lh_ln_lstm_intra(const float* x, const float* ln_w, const float* ln_b, const void* w_pk, const float* b_sum,
                     float* h_out, int n_frames /* B*T */, int mode, lh_stream_t stream);

/* A.3.2  inter-frame path: LayerNorm(C) -> causal LSTM over time with carried state ; hidden states only.
 * Replaces tfgridnet_causal.py:521-532 (inter_norm, transpose/reshape to [B*F,T,C], inter_rnn, h0/c0 in/out).
 *   x [B][T][97][64]; h0,c0,hN,cN [B*97][64] (sequence index b*97+f); w_pk [1][4][4][32][64]; b_sum [256]
 *   h_out [B*T*97][64] in the same (b,t,f) row order as x
 */
int lh_ln_lstm_inter(const float* x, const float* ln_w, const float* ln_b, const void* w_pk, const float* b_sum,
                     const float* h0, const float* c0, float* hN, float* cN, float* h_out, int B, int T, int mode,
                     lh_stream_t stream);

/* A.3.1 for very few frames (streaming, batch-1): same result as lh_ln_lstm_intra, one workgroup per (frame, direction):
 * the input half of all 97 steps as one MFMA GEMM, the recurrent half as a 256 x 64 fp32 mat-vec per step.
 *   x [n_frames][97][64]; h_out [n_frames*97][128]
 *   wih_pk fp16 hi/lo B image [2 dirs][16 ntiles][2 ksteps][64 lanes][16] of W_ih * ln_w with the gate columns in the
 *   kernel's order (column n = PyTorch row (n&3)*64 + (n>>5)*8 + ((n>>3)&3)*2 + ((n>>2)&1));  b_sum [2][256] in the
 *   same order;  whh [2][512][32] fp32 = the same rows of W_hh cut into their two k halves (weights.py pack_block:
 *   intra_s_*)
 */
int lh_intra_stream(const float* x, const void* wih_pk, const float* b_sum, const float* whh, float* h_out,
                    int n_frames, lh_stream_t stream);

/* A.3.2 + Linear fused for few sequences (the host uses it while they fit one round of CUs: batch <= 2): same result as lh_inter_block, one workgroup per sequence
 * (b, f), 64-step chunks: input half and output projection as MFMA GEMMs around a mat-vec recurrence.
 *   x, out [B][T][97][64] (must not alias); h0, c0, hN, cN [B*97][64]
 *   wih_pk [16 ntiles][2 ksteps][64 lanes][16], b_sum [256], whh [512][32]: the lh_intra_stream layouts for the inter
 *   LSTM (weights.py pack_block: inter_s_*);  wlin_pk [4][2][64][16], blin [64] as lh_inter_block
 */
int lh_inter_matvec(const float* x, const void* wih_pk, const float* b_sum, const float* whh, const void* wlin_pk,
                    const float* blin, const float* h0, const float* c0, float* hN, float* cN, float* out, int B, int T,
                    lh_stream_t stream);

/* A.3.1 + Linear fused (split-precision mode): LayerNorm -> BiLSTM over frequency -> Linear(128->64) -> + residual in
 * ONE kernel; replaces tfgridnet_causal.py:505-516.  A workgroup runs the forward then the reverse direction over its
 * sequences and accumulates both halves of the projection into the same output rows (no hidden-state round trip).
 *   x, out [B*T][97][64] (must not alias); w_pk / b_sum as lh_ln_lstm_intra in LH_GEMM_F16X3 mode;
 *   wlin_pk [2 passes][4 ntiles][2 ksteps][64 lanes][hi 8 | lo 8] = intra_linear.weight[:, 0:64] and [:, 64:128]
 *   (weights.py pack_linear_f16x3(unscaled=True): lo = fp16(w - hi)); blin [64]
 */
int lh_intra_block(const float* x, const void* w_pk, const float* b_sum, const void* wlin_pk, const float* blin,
                   float* out, int n_frames, lh_stream_t stream);

/* A.3.2 + Linear fused: LayerNorm -> causal LSTM over time (state in/out) -> Linear(64->64) -> + residual;
 * replaces tfgridnet_causal.py:521-538.   x, out [B][T][97][64]; wlin_pk [4][2][64][16] fp16 hi/lo (lo unscaled,
 * weights.py `inter_lin_wu`); blin [64]
 *   w_pk   [8 waves][2 tiles][4 ksteps][64 lanes][hi 8 | lo 8] fp16 (weights.py pack_lstm_f16x3_w8, `inter_w8`): the
 *          eight-wave kernel multiplies transposed (weights = MFMA A operand); lane l of (wave v, tile m, kstep ks)
 *          holds row gate*64 + unit of [W_ih * ln_w | W_hh], gate = (l & 15) & 3, unit = 8v + 2 ((l & 15) >> 2) + m,
 *          at k = 32 ks + 8 (l >> 4) + j; lo unscaled, rows scaled by the gate's exponent factor;
 *   b_sum  [256] in PyTorch gate order (i, f, g, o) x 64, same scaling (weights.py `inter_b16`)
 */
int lh_inter_block(const float* x, const void* w_pk, const float* b_sum, const void* wlin_pk, const float* blin,
                   const float* h0, const float* c0, float* hN, float* cN, float* out, int B, int T,
                   lh_stream_t stream);

/* Row-wise Linear(K->64) + bias + residual:  out[r][:] = res[r][:] + W h[r][:] + b.
 * Replaces intra_linear + residual (tfgridnet_causal.py:513-516, K=128) and inter_linear + view/transpose +
 * residual (:534-538, K=64).   h [rows][K]; bias [64]; res,out [rows][64];
 *   w_pk  split-precision fp16 image [4 ntiles][K/32 ksteps][64 lanes][hi 8 | lo 8] (weights.py pack_linear_f16x3)
 */
int lh_linear_res(const float* h, const void* w_pk, const float* bias, const float* res, float* out, int rows,
                  int K, lh_stream_t stream);

/* Split-precision activation rows shared by lh_qkv_proj_ln / lh_local_attn / lh_ring_pack / lh_ring_unpack.
 * Every value v is stored as two fp16 numbers  hi = fp16(v), lo = fp16(v - hi)  (4 bytes per element,
 * like fp32; v ~ hi + lo keeps ~22 mantissa bits for |v| >= 2^-3 and an absolute 2^-25 below) in the order the
 * attention MFMA operands consume:
 *   q   [B*4][T][1216 halves]          per row 76 blocks of 8 features (f*6+e), each [hi 8 | lo 8]; features
 *                                      582..607 are zero
 *   kx  [B*4][T+49+PAD][1216 halves]   same row format; rows 0..48 = history (K_buf), row 49+t = K[t]
 *   vx  [B*4][T+49+PAD][3104 halves]   per row 388 quads of 4 columns (f*16+v), each [hi 4 | lo 4]
 * PAD = LH_KV_PAD_ROWS rows behind row T+48 that the CALLER zero-fills once and the library never writes: attention
 * tiles read (without needing them) up to 47 rows past their last key. */
#define LH_KV_PAD_ROWS 48

/* A.3.3  Q/K/V: pointwise Linear + PReLU, head split, joint LayerNorm over (f,e) per head.
 * Replaces attn_conv_Q/K/V (tfgridnet_causal.py:354-387, used :547-551) and the K/V history concat (:553-562):
 * K and V rows are written at row (49 + t) of the history-extended buffers.
 *   y      [B][T][97][64]
 *   w_pk   fp16 hi/lo image [7 ntiles][2 ksteps][64 lanes][16] of the stacked weight, rows 0..23 Q(h*6+e),
 *          24..47 K, 48..111 V(h*16+v); bias [112 + 3]
 *          Q, K and V are three LayerNorm groups.  A group whose largest |w| is below 2^-4 is stored as 2^k W, 2^k b (k the
 *          smallest that brings it to 2^-4 or above; weights.py ln_group), because the un-rescaled lo half of a weight has an
 *          absolute floor of 2^-25; bias[112..114] = eps 4^k of Q, K, V (1e-5 for k = 0), which the kernel adds to the
 *          variance: PReLU is positively homogeneous and a power of two exact, so LN_{eps 4^k}(2^k z) = LN_eps(z).
 *   slopes [3] PReLU slopes (Q,K,V);  lnq_w/b, lnk_w/b [608] = the 582 affine values zero-padded;  lnv_w/b [1552]
 *   q, kx, vx  split-precision rows (above)
 *   ring_pos   NULL, or (T = 1) a device counter: the K / V row goes to slot (*ring_pos mod 50) of a persistent
 *              50-row ring instead of row 49 — rows 0..49 are then exactly the window of the one query frame, in
 *              rotated order (softmax and P.V are order-free), and no history row ever has to be moved;
 *              or (ABI 32, 2 <= T <= 16, the whole clip only) the position word of a ring of 49 + T rows, "frames per
 *              chunk" below.  T > 16 with ring_pos: LH_ERR_ARG.
 *
 * Frames per chunk (ABI 32).  A streamer that serves m frames per chunk (1 <= m <= 16) keeps, per block and (batch, head), a
 * ring of R = 49 + m rows: the FIRST R rows of kx / vx buffers of m + 49 + LH_KV_PAD_ROWS rows — the shape lh_local_attn
 * expects for T = m.  The 48 rows behind the ring are zeroed once by the caller and never written.  `pos`, a device word in
 * [0, R), names the slot that frame 0 of the next chunk goes to:
 *   write   frame j of the chunk (j < m) goes to slot ((unsigned)pos + j) mod R          (lh_qkv_proj_ln, ring_pos = &pos)
 *   read    logical history-extended row n (n = 0..48: history, oldest first; n = 49 + j: the chunk's frame j) is physical
 *           row ((unsigned)pos + m + n) mod R for n < R.  Rows n >= R, which the tile over-reads without needing them, are
 *           physical row n: the zero pad rows, and R >= 50 keeps every such read inside the buffer (lh_local_attn_ring)
 *   after   pos = (pos + m) mod R                                                         (lh_ring_advance_by)
 * With m = 1 this is the 50-row ring above: R = 50, write at pos mod 50; every row is then in the one frame's window and
 * lh_local_attn itself serves the read.
 */
int lh_qkv_proj_ln(const float* y, const void* w_pk, const float* bias, const float* slopes, const float* lnq_w,
                   const float* lnq_b, const float* lnk_w, const float* lnk_b, const float* lnv_w,
                   const float* lnv_b, void* q, void* kx, void* vx, const int* ring_pos, int B, int T,
                   lh_stream_t stream);

/* lh_qkv_proj_ln for one-frame chunks (T = 1) whose rows each own a ring position (ABI 19, paced sessions below):
 *   write_pos  [B] device words: row b writes its K and V rows into ring slot write_pos[b] (mod 50) of its persistent
 *              rings; a NEGATIVE entry writes no K / V row (a held or idle row of a paced host).  The Q row is written
 *              either way.  The zero pad rows behind the 50 ring rows are written by neither form.
 * Row b's Q / K / V bits are those of lh_qkv_proj_ln with *ring_pos = write_pos[b]: a separate instantiation of the same
 * kernel body. */
int lh_qkv_proj_ln_rows(const float* y, const void* w_pk, const float* bias, const float* slopes, const float* lnq_w,
                        const float* lnq_b, const float* lnk_w, const float* lnk_b, const float* lnv_w,
                        const float* lnv_b, void* q, void* kx, void* vx, const int* write_pos, int B,
                        lh_stream_t stream);

/* A.3.5  local windowed attention over exactly 50 slots (frames t-49..t incl. history rows, no mask) with
 * the head merge fused into the store.  Replaces tfgridnet_causal.py:564-581 without materialising the
 * 50x unfolded K/V (`_causal_unfold_chunk`, :429-454).
 *   q, kx, vx  split-precision rows (above)
 *   merged [B][T][4][97][16]   merged[b][t][h][f][v] = O[b*4+h][t][f*16+v]   (head-major frame slabs)
 */
int lh_local_attn(const void* q, const void* kx, const void* vx, float* merged, int B, int T, lh_stream_t stream);
/* lh_local_attn on a ring (ABI 32, "frames per chunk" above): 1 <= T <= 16 query frames whose history-extended rows are read
 * through the read rule; *ring_pos is the value the lh_qkv_proj_ln launch of the same chunk saw.  The row map goes into the
 * row addresses only: the output is bit for bit that of lh_local_attn on the same rows laid out contiguously.  Launch
 * geometry of lh_local_attn for T <= 16.  LH_ERR_ARG: a null pointer, T < 1 or T > 16. */
int lh_local_attn_ring(const void* q, const void* kx, const void* vx, float* merged, const int* ring_pos, int B, int T,
                       lh_stream_t stream);

/* A.3.4  streaming state <-> history rows (tfgridnet_causal.py:553-562).  The reference carries the last 49 K / V
 * rows as fp32 state:  lh_ring_pack writes k_buf [B*4][49][582] / v_buf [B*4][49][1552] into rows 0..48 of kx / vx
 * before lh_qkv_proj_ln;  lh_ring_unpack reads rows T..T+48 (the new history) back into fp32 state tensors
 * (hi + lo, i.e. exactly the values the attention kernel used). */
int lh_ring_pack(const float* k_buf, const float* v_buf, void* kx, void* vx, int B, int T, lh_stream_t stream);
int lh_ring_unpack(const void* kx, const void* vx, float* k_buf, float* v_buf, int B, int T, lh_stream_t stream);
/* Streaming ring slot counter (lh_qkv_proj_ln's ring_pos): *ring_pos = (*ring_pos + 1) mod modulo, on the device and in
 * stream order — one node of the captured per-chunk graph (the reference has no counterpart: it shifts K_buf / V_buf by
 * one row per chunk, tfgridnet_causal.py:553-562).  modulo in [1, 2^30]. */
int lh_ring_advance(int* ring_pos, int modulo, lh_stream_t stream);
/* ... by `step` slots (ABI 32: a chunk of `step` frames on a ring of `modulo` rows): *ring_pos = (*ring_pos + step) mod modulo,
 * 1 <= step <= modulo <= 2^30. */
int lh_ring_advance_by(int* ring_pos, int step, int modulo, lh_stream_t stream);
/* Per-row form (ABI 19): pos[r] = (write_pos[r] + 1) mod modulo where write_pos[r] >= 0, untouched otherwise, r < n_rows.
 * The only writer of a paced host's ring positions apart from a row move.  LH_ERR_ARG: null, pos == write_pos, n_rows < 1. */
int lh_ring_advance_rows(int* pos, const int* write_pos, int modulo, int n_rows, lh_stream_t stream);

/* A.3.6  attn_concat_proj: Linear(64->64)+PReLU, joint LayerNorm over (f,c), residual; optional speaker gain.
 * Replaces tfgridnet_causal.py:583-588 and, when gain != NULL, the `batch = batch * embed` applied to the
 * input of block 1 (:250-251):  out = (y2 + LN(PReLU(W m + b))) * gain[b][f][c].
 *   merged [B][T][4][97][16] (lh_local_attn's output order); y2, out [B][T][97][64]; w_pk fp16 hi/lo image [4][2][64][16]; bias [64 + 1]: b, then eps 4^k of the 2^k W, 2^k b stored (as lh_qkv_proj_ln; all forms of this stage); slope [1]; ln_w/b [6208]; gain [B][97][64]|NULL
 */
int lh_proj_ln_res(const float* merged, const void* w_pk, const float* bias, const float* slope,
                   const float* ln_w, const float* ln_b, const float* y2, const float* gain, float* out, int B,
                   int T, lh_stream_t stream);
/* Fan-out form (ABI 25): K enrolled speakers per mixture.  The embedding enters the network only here, in front of block 1
 * (tfgridnet_causal.py:247-251), so the front end and block 0 of a mixture are the same for every one of its targets: the
 * un-gained frame y2 + LN(PReLU(W m + b)) is computed once and stored K times,
 *   out[b * K + j] = (y2[b] + LN(PReLU(W m[b] + b))) * gain[b * K + j],   0 <= j < K,
 * each product the single fp32 multiply of lh_proj_ln_res: row b * K + j has the bits of lh_proj_ln_res with gain[b * K + j].
 *   merged [B][T][4][97][16], y2 [B][T][97][64] and the weights as above; gain [B*K][97][64]; out [B*K][T][97][64]
 * lh_proj_ln_res_fan_win: frames [t0, t0 + Tc) of every row, like lh_proj_ln_res_win (time windows, below).
 * LH_ERR_ARG: a null pointer (gain included), K < 1, a window outside [0, T).  (Net.forward_many, lookoncetohear_amd/net.py) */
int lh_proj_ln_res_fan(const float* merged, const void* w_pk, const float* bias, const float* slope, const float* ln_w,
                       const float* ln_b, const float* y2, const float* gain, float* out, int B, int T, int K,
                       lh_stream_t stream);
int lh_proj_ln_res_fan_win(const float* merged, const void* w_pk, const float* bias, const float* slope, const float* ln_w,
                           const float* ln_b, const float* y2, const float* gain, float* out, int B, int T, int t0, int Tc,
                           int K, lh_stream_t stream);

/* A.4  causal ConvTranspose2d(64->4,3x3) + spectrum re-pack + iSTFT synthesis/overlap-add.
 * Replaces tfgridnet_causal.py:256-273 and the look-ahead trim of net.py:61.
 *   y [B][T][97][64]; deconv_buf_in/out [B][64][2][97]; istft_buf_in/out [B][2][194][1]
 *   wdec_pk fp16 hi/lo B image [3 ntiles][2 ksteps][64 lanes][16] of deconv.weight as [(kt,kf,o) 36 -> 48] x [64 c];
 *   bdec [4]; wfb_dec fp16 hi/lo B image [12 ntiles][7 ksteps][64 lanes][16] of dec.filterbank._filters^T
 *   [192 samples] x [194 -> 224 rows]   (weights.py pack_linear_f16x3)
 *   wave_out [B][2][128*T];  range_flag: the caller's two-word flag (range contract above) or NULL;
 *   keep_nonfinite (ABI 13): what a non-finite output sample is stored as — 1: as it is (inf / NaN reach the caller exactly
 *   as from the reference's plain-fp32 forward, nothing is hidden; the offline host `Net` passes 1), 0: as 0 (silence, not
 *   NaN, reaches a listener; the streaming host passes 0).  The flag is raised either way.
 */
int lh_deconv_istft(const float* y, const float* deconv_buf_in, float* deconv_buf_out, const float* istft_buf_in,
                    float* istft_buf_out, const void* wdec_pk, const float* bdec, const void* wfb_dec,
                    float* wave_out, unsigned* range_flag, int keep_nonfinite, int B, int T, lh_stream_t stream);

/* Tap products (ABI 26): the last block's A.3.6 and A.4 as one pair, from the ZERO state and with no state out (an offline
 * forward).  The transposed conv's channel contraction P[t][f][(kt,kf,o)] = sum_c Y[t][f][c] Wd[c][o][kt][kf] is linear and per
 * (frame, bin), so the stage that makes Y does it while Y is in registers:
 *   lh_proj_ln_res_taps   lh_proj_ln_res without gain that stores, instead of the frame, its 36 tap products
 *                         p_out [B][T][97][36] (0.5625 of the frame's bytes) and the frame maximum fmax [B][T] = max |Y[b][t]|
 *                         (bounds the spectra in lh_taps_istft).  wdec_pk = lh_deconv_istft's tap image, the rest as above;
 *                         `_win`: frames [t0, t0 + Tc) like lh_proj_ln_res_win.
 *   lh_taps_istft         lh_deconv_istft from there: 9-term gather, spectrum re-pack, synthesis, overlap-add.  The carried
 *                         conv halo and spectrum are zero.  wdec_pk is only read for the bound W1.  wave_out, range_flag and
 *                         keep_nonfinite as in lh_deconv_istft; lh_set_tuning key 6 applies.
 * Same groups of rows under one power of two, same accumulator chains, same sum order: wave_out has the BITS of
 * lh_proj_ln_res(gain = NULL) -> lh_deconv_istft on zero deconv_buf_in / istft_buf_in.
 * LH_ERR_ARG: a null pointer (range_flag may be NULL), B <= 0, T <= 0, a window outside [0, T). */
int lh_proj_ln_res_taps(const float* merged, const void* w_pk, const float* bias, const float* slope, const float* ln_w,
                        const float* ln_b, const float* y2, const void* wdec_pk, float* p_out, float* fmax, int B, int T,
                        lh_stream_t stream);
int lh_proj_ln_res_taps_win(const float* merged, const void* w_pk, const float* bias, const float* slope, const float* ln_w,
                            const float* ln_b, const float* y2, const void* wdec_pk, float* p_out, float* fmax, int B, int T,
                            int t0, int Tc, lh_stream_t stream);
int lh_taps_istft(const float* p, const float* fmax, const void* wdec_pk, const float* bdec, const void* wfb_dec,
                  float* wave_out, unsigned* range_flag, int keep_nonfinite, int B, int T, lh_stream_t stream);

/* ---- time windows (ABI 14) ------------------------------------------------------------------------------------------------
 * Every stage of a GridNetBlock is causal in time (tfgridnet_causal.py:489-590): the intra pass is per frame, the inter LSTM
 * carries (h, c) (:521-532), the attention sees the 49 previous K / V rows (:553-562) and the frame stages are per frame.  The
 * `_win` entry points run the SAME kernels on frames [t0, t0 + Tc) of every utterance of buffers laid out for T frames
 * ([B][T][97][64] activations, q [4B][T][..], kx / vx [4B][T + 49 + PAD][..]); `lh_X(..., B, T, s)` is `lh_X_win(..., B, T, 0,
 * T, s)`.  A host can then cut the time axis and run block i on window k + 1 beside block i + 1 on window k on separate
 * streams (lookoncetohear_amd/net.py, `Net.time_chunks`): the inter LSTM's 625-step dependent chain, which fills only 194 of
 * the 256 CUs, overlaps with the other stages.  State hand-over between windows of one block, all on the device:
 *   lh_inter_block_win   (hN, cN) of window k are (h0, c0) of window k + 1 (distinct buffers per window).  `carry`: bit 0 =
 *                        c0 holds the kernel's internal cell state (-2 log2(e) c, written by the previous window with bit 1),
 *                        bit 1 = cN is written in that form; 0 = both are the reference's c (tfgridnet_causal.py:526-532).  With
 *                        the inner boundaries carried in the internal form the windows reproduce the whole-clip launch bit
 *                        for bit (c / k followed by k * c is two roundings);
 *   lh_qkv_proj_ln_win   writes rows 49 + t of kx / vx, lh_local_attn_win of window k + 1 reads rows t0 .. of the same
 *                        buffers: the history IS the previous window's rows, nothing is packed or unpacked.  (Attention tiles
 *                        read — never need — up to 47 rows past the window: they must hold finite values, e.g. the zeros of the
 *                        allocation or an earlier forward's rows.)
 * Tc >= 2 for lh_inter_block_win; t0 + Tc <= T. */
int lh_intra_block_win(const float* x, const void* w_pk, const float* b_sum, const void* wlin_pk, const float* blin,
                       float* out, int B, int T, int t0, int Tc, lh_stream_t stream);
int lh_inter_block_win(const float* x, const void* w_pk, const float* b_sum, const void* wlin_pk, const float* blin,
                       const float* h0, const float* c0, float* hN, float* cN, float* out, int B, int T, int t0, int Tc,
                       int carry, lh_stream_t stream);
/* the unfused intra pair of small batches on a window (split-precision mode): lh_ln_lstm_intra + lh_linear_res on frames (b, t0 + j);
 * h_out / h [B*T*97][128] in the (b, t, f) row order of x */
int lh_ln_lstm_intra_win(const float* x, const float* ln_w, const float* ln_b, const void* w_pk, const float* b_sum, float* h_out,
                         int B, int T, int t0, int Tc, lh_stream_t stream);
int lh_linear_res_win(const float* h, const void* w_pk, const float* bias, const float* res, float* out, int B, int T, int t0,
                      int Tc, int K, lh_stream_t stream);
/* the few-sequences form of the inter stage (lh_inter_matvec) on a window; `carry` as above.  Windows that start on multiples of
 * its 64-step chunk reproduce the whole-clip launch bit for bit. */
int lh_inter_matvec_win(const float* x, const void* wih_pk, const float* b_sum, const float* whh, const void* wlin_pk,
                        const float* blin, const float* h0, const float* c0, float* hN, float* cN, float* out, int B, int T,
                        int t0, int Tc, int carry, lh_stream_t stream);
int lh_qkv_proj_ln_win(const float* y, const void* w_pk, const float* bias, const float* slopes, const float* lnq_w,
                       const float* lnq_b, const float* lnk_w, const float* lnk_b, const float* lnv_w,
                       const float* lnv_b, void* q, void* kx, void* vx, const int* ring_pos, int B, int T, int t0, int Tc,
                       lh_stream_t stream);
int lh_local_attn_win(const void* q, const void* kx, const void* vx, float* merged, int B, int T, int t0, int Tc,
                      lh_stream_t stream);
int lh_proj_ln_res_win(const float* merged, const void* w_pk, const float* bias, const float* slope, const float* ln_w,
                       const float* ln_b, const float* y2, const float* gain, float* out, int B, int T, int t0, int Tc,
                       lh_stream_t stream);

/* ---- plain-fp32 reference kernels of the frame stages (gemm_mode "f32all"; lh_ref32.hip) ----------------------------------
 * NON-PRODUCT: test / diagnosis kernels that ship in the library so that a host can bisect a disagreement with a real
 * checkpoint without a second build.  Never benchmark them, never route a product path through them.
 * The product frame kernels above are split-precision (fp16 hi + lo, ~22 bits) in EVERY arithmetic mode; with these and the
 * exact fp32-MFMA recurrences (lh_ln_lstm_intra / _inter in LH_GEMM_F32) a forward exists whose every contraction is an
 * fp32 fmaf chain like the reference's (tfgridnet_causal.py:188-283): the A/B that separates split-precision error from a
 * kernel bug on a real checkpoint.  Written for obviousness (one thread per output, natural summation order), ~50x slower
 * than the product path, test / diagnosis only.  Weights are the PyTorch tensors of the state dict as they are (no packed
 * images); activations channel-last [B][T][97][64] like everywhere else; Q / K / V plain fp32:
 *   q [4B][T][582], kx [4B][T+49][582], vx [4B][T+49][1552] (rows 0..48 = K_buf / V_buf, copied by the caller).
 * lh_ref32_stft_conv_in   :229-242   filters = enc.filterbank._filters [194][1][192]; conv_w [64][4][3][3]; spec_scratch
 *                                    [B][4][T+2][97]
 * lh_ref32_linear         out[r][n] = (res[r][n] +) act(bias[n] + sum_k in[r][k] w[n][k]); slope = PReLU weight or NULL
 * lh_ref32_head_ln        :360-376   head split + LayerNorm over (f, d) of columns col0 + h*D + d of `pre` [B][T][97][ncol]
 *                                    into dst[(b*4+h)][row0 + t][f*D + d]; D = 6 (Q, K) or 16 (V)
 * lh_ref32_local_attn     :564-581   50 slots, no mask; merged [B][T][4][97][16]
 * lh_ref32_proj_ln_res    :583-588, 250-251   w [64][64]; rows_scratch, pre_scratch [B*T*97][64]
 * lh_ref32_deconv_istft   :256-273, net.py:61   deconv_w [64][4][3][3]; filters = dec.filterbank._filters; sx_scratch
 *                                    [B][2][T+1][194]; non-finite samples are stored as they are (no flag)
 */
int lh_ref32_stft_conv_in(const float* x, const float* conv_buf_in, float* conv_buf_out, const float* filters,
                          const float* conv_w, const float* conv_b, float* spec_scratch, float* out, int B, int T,
                          int n_samples, lh_stream_t stream);
int lh_ref32_linear(const float* in, const float* w, const float* bias, const float* slope, const float* res, float* out,
                    int rows, int K, int N, lh_stream_t stream);
int lh_ref32_head_ln(const float* pre, int ncol, int col0, int D, const float* ln_w, const float* ln_b, float* dst,
                     int row0, int rows_per_bh, int B, int T, lh_stream_t stream);
int lh_ref32_local_attn(const float* q, const float* kx, const float* vx, float* merged, int B, int T, lh_stream_t stream);
int lh_ref32_proj_ln_res(const float* merged, const float* w, const float* bias, const float* slope, const float* ln_w,
                         const float* ln_b, const float* y2, const float* gain, float* rows_scratch, float* pre_scratch,
                         float* out, int B, int T, lh_stream_t stream);
int lh_ref32_deconv_istft(const float* y, const float* deconv_buf_in, float* deconv_buf_out, const float* istft_buf_in,
                          float* istft_buf_out, const float* deconv_w, const float* deconv_b, const float* filters,
                          float* sx_scratch, float* wave_out, int B, int T, lh_stream_t stream);

/* ---- enrollment embedder (reference src/models/tfgridnet_orig/tfgridnet.py:88-127 + espnet2 TF-GridNet trunk) ----
 * Front end, tfgridnet.py:109-117: x / std(x) (unbiased, over samples and mics), STFT(n_fft 128, hop 64, hann, centred
 * with reflect padding), re/im channel stacking, Conv2d(4->64, 3x3, padding 1), GroupNorm(1, 64).
 *   x [B][2][n_samples]; inv_std [B] (out); wfb_pk fp32 MFMA image [9][32][64] of the windowed DFT rows [128 x 130];
 *   wconv_pk [4][9][64] of conv.0.weight as [36 taps] x [64]; bconv, gn_w, gn_b [64];
 *   gn_part fp64 scratch [B * ceil(T/14)][2]; z [B][T][65][64] out, T = n_samples/64 + 1
 *   xsplit_next  NULL, or 2*B*T*65*64 fp16: z channel-normalised and split, for lh_emb_axis_fused(have_xsplit = 1)
 */
int lh_emb_frontend(const float* x, float* inv_std, const float* wfb_pk, const float* wconv_pk, const float* bconv,
                    const float* gn_w, const float* gn_b, double* gn_part, float* z, void* xsplit_next, int B, int T,
                    int n_samples, lh_stream_t stream);

#ifdef LH_LEGACY  /* A/B lab builds only (-DLH_LEGACY): not exported by the product library */
/* One axis path of an espnet2 GridNetBlock of the embedder (intra: inter = 0, sequences = frames, scan over the 65
 * bins; inter = 1: sequences = bins, scan over time): LayerNorm(C) -> unfold(4) -> BiLSTM(256 -> 64) ->
 * ConvTranspose1d(128 -> 64, 4) -> + residual, as three launches (input GEMM over all windows, recurrence, gather-GEMM).
 *   x, out [B][T][65][64] (no alias); wih_pk fp16 hi/lo image [32][8][64][16] (both directions, LN affine folded,
 *   features window-major, columns (dir, unit, gate)); bih [512]; whh_pk [2][4][4][2][64][16]; wct_pk [4][16][64][16]
 *   of the taps as [64] x [4*128]; bct [64]; xsplit scratch 2*B*T*65*64 fp16 (hi | lo images of the channel-
 *   normalised input); gx scratch [nseq*P][512]; hbuf scratch [nseq*P][128] (P = L - 3)
 */
int lh_emb_axis(const float* x, const void* wih_pk, const float* bih, const void* whh_pk, const void* wct_pk,
                const float* bct, void* xsplit, float* gx, float* hbuf, float* out, int B, int T, int inter,
                lh_stream_t stream);
#endif /* LH_LEGACY */

/* The same axis path without the gate pre-activation round trip (round 4): LayerNorm + split -> ONE recurrent kernel that
 * computes the 256-wide input half one step ahead of the dependent chain (weights resident in registers, one workgroup of
 * 16 sequences x one direction per CU) and writes the hidden states as fp16 hi | lo images -> transposed-conv GEMM + residual.
 *   wrec_pk  fp16 [2 dirs][8 waves][40 fragments][64 lanes][8]: MFMA A fragments of [W_ih (4 window slots) | W_hh], rows
 *            ordered (unit, gate), LayerNorm gamma and the gates' exponent factors folded in (embed_net.py pack_rec)
 *   brec     [2][256] in (unit, gate) order, same folding;  wct_pk, bct as lh_emb_axis
 *   xsplit   scratch 2*B*T*65*64 fp16;  hsplit scratch 2*nseq*P*128 fp16 (hi | lo images of the hidden states)
 *   have_xsplit  non-zero: xsplit already holds the channel-normalised, split x (left there by the previous axis call's
 *            emit_split or by lh_emb_attn_block's xsplit_next) and the normalisation launch is skipped
 *   emit_split   non-zero: xsplit is overwritten with the normalised, split OUT rows once the recurrence has consumed it */
int lh_emb_axis_fused(const float* x, const void* wrec_pk, const float* brec, const void* wct_pk, const float* bct,
                      void* xsplit, void* hsplit, float* out, int B, int T, int inter, int have_xsplit, int emit_split,
                      lh_stream_t stream);

/* The inter axis for SMALL batches (ABI 14): as lh_emb_axis_fused(inter = 1) with the recurrence on one workgroup per (sequence,
 * direction) — the quad-lane mat-vec step of the separator's batch-1 kernels, 0.39 us per step against 1.4 us for a 16-sequence
 * tile that a single enrollment fills with 9 workgroups.  Same result to fp32 rounding.
 *   wih_pk  fp16 hi/lo B image [2 dirs x 16 ntiles][8 ksteps][64 lanes][16] of W_ih' [256 x 256] (LayerNorm gamma folded, K = window
 *           slot*64 + channel in natural tap order, columns (direction, unit, gate));  bih [2][256] same column order
 *           (b_ih + b_hh + W_ih beta);  whh fp32 [2][256][64], row 4 unit + gate;  the rest as lh_emb_axis_fused */
int lh_emb_axis_mv(const float* x, const void* wih_pk, const float* bih, const float* whh, const void* wct_pk,
                   const float* bct, void* xsplit, void* hsplit, float* out, int B, int T, int have_xsplit, int emit_split,
                   lh_stream_t stream);

/* Enrollment embedder, attention branch of one GridNetBlock (espnet2 GridNetBlock.forward attention part, restated in
 * oracle/embedder_oracle.py:149-168): per-head Q/K/V 1x1 conv + PReLU + LayerNorm over (channel, bin), full T x T
 * softmax attention per (head, utterance), head merge, attn_concat_proj (1x1 conv + PReLU + LayerNorm) + residual.
 * Tp = T rounded up to a multiple of 64.
 *   y2, out  [B][T][65][64];  merged scratch [B][T][65][64]
 *   q, k     scratch fp16 [2][4B][T][544] (hi | lo images);  v scratch fp32 [4B][T][1040]
 *   vt       scratch fp16 [2][4B][1040][Tp];  sc scratch fp32 [4B][T][Tp];  p scratch fp16 [2][4B][T][Tp]
 *   wqkv_pk  fp16 hi/lo image [8][2][64][16] of the stacked conv weights [128 x 64] (Q h*8+e | K | V h*16+v)
 *   slopes [128] (PReLU slope of each output column's head conv);  bqkv [128 + 12]: the biases, then eps 4^k of the twelve
 *            LayerNorm groups (Q heads 0..3, K heads 0..3, V heads 0..3), each head conv stored as 2^k W, 2^k b (lh_qkv_proj_ln)
 *   lnq_*, lnk_* [4][520], lnv_* [4][1040]: LayerNorm affine re-ordered to (bin*d + channel)
 *   wproj_pk [4][2][64][16]; bproj [64 + 1] (b, eps 4^k); slope_p [1]; lnp_* [4160] re-ordered to (bin*64 + channel)
 *   xsplit_next  NULL, or 2*B*T*65*64 fp16: the channel-normalised, split `out` rows for the next block's intra axis call
 *            (lh_emb_axis_fused have_xsplit)
 */
int lh_emb_attn_block(const float* y2, const void* wqkv_pk, const float* bqkv, const float* slopes,
                      const float* lnq_w, const float* lnq_b, const float* lnk_w, const float* lnk_b,
                      const float* lnv_w, const float* lnv_b, const void* wproj_pk, const float* bproj,
                      const float* slope_p, const float* lnp_w, const float* lnp_b, void* q, void* k, float* v,
                      void* vt, float* sc, void* p, float* merged, float* out, void* xsplit_next, int B, int T,
                      lh_stream_t stream);

/* Enrollment embedder head (reference src/models/tfgridnet_orig/tfgridnet.py:120-127): Linear(65*64 -> 256) per
 * frame, LayerNorm(256), mean over frames.
 *   z [B][T][65][64];  w_pk fp16 hi/lo image [16][130][64][16] of the weight with inputs re-ordered to (bin*64 + c)
 *   ln_w, ln_b [256];  bias [256 + 1] (b, then eps 4^k of the 2^k W, 2^k b stored: lh_qkv_proj_ln);  part scratch [B][ceil(T/64)][256];  emb [B][256]
 */
int lh_emb_head(const float* z, const void* w_pk, const float* bias, const float* ln_w, const float* ln_b,
                float* part, float* emb, int B, int T, lh_stream_t stream);

/* Binaural rendering, the data-pipeline step before the separator (reference src/datasets/multi_ch_simulator.py:40-61
 * `_convolve` = `scipy.signal.convolve(src, rir[ear])[:len(src)]` per source and ear;
 * src/datasets/MixLibriSpeechNoisyEnrollNorm.py:176-202 noise scale, peak normalisation, mixture, target).
 *   src      [B][S1][N]       mono rows: the sources first, the noise bed LAST
 *   rir      [B][S1][2][Lh]   impulse response per row and ear (shorter ones zero-padded to Lh)
 *   gain     [B][S1]          applied after the convolution: 1 for sources, `noise_scale` for the noise row
 *   tgt_idx  [B] int32        row returned as `target`
 *   events   [B][S1][2][N]    out: rendered rows before peak normalisation
 *   peak     [B] uint32       out: bit pattern of the fp32 peak of |mixture| (the reference's `norm_factor`)
 *   mixture, target [B][2][N] out: divided by the peak when it exceeds 1 (IEEE division, reference order of sums)
 */
int lh_render_binaural(const float* src, const float* rir, const float* gain, const int* tgt_idx, float* events,
                       unsigned* peak, float* mixture, float* target, int B, int S1, int N, int Lh, lh_stream_t stream);

/* Moving sources (ABI 24): lh_render_binaural with impulse responses that change along a path, one point per `frame`
 * samples.  The INTERFACE follows the reference's binding of its native simulator (src/datasets/motion_simulator.py:30-95:
 * simulator_set_hrtf -> `bank`, simulator_add_source(audio, path) -> lh_path_nearest, simulator_simulate ->
 * lh_render_moving); the ARITHMETIC is this project's own definition, stated here — the native library and its source are
 * absent, so nothing below is a restatement pinned to the reference.
 * Per utterance b, row s (sources first, the noise bed LAST), ear e, sample n < N:
 *     f  = n / frame (integer),  w = (float)(n % frame) / (float)frame      (fp32 IEEE division)
 *     ha = bank[bank_of[b]][idx[b][s][f]][e],  hb = bank[bank_of[b]][idx[b][s][f + 1]][e]
 *     a  = sum_{k < Lh} ha[k] x[n - k],  b_ = sum_{k < Lh} hb[k] x[n - k]   (x[< 0] = 0; each one fp32 fmaf chain over k
 *                                                                            ascending from 0.f)
 *     events[b][s][e][n] = fmaf(w, b_ - a, a) * gain[b][s]
 * an output-side linear cross-fade between the responses of consecutive path points: the filter belongs to the output
 * sample.  Where idx[f] == idx[f + 1] the row has the bits of lh_render_binaural's direct form (Lh < 1024 or Lh > 4097) with
 * that response.  Direct form at every Lh.
 *   bank     [K][P][2][Lh]    K response banks of P entries (one bank per utterance: the reference picks one SOFA file per scene)
 *   bank_of  [B] int32        in [0, K)
 *   idx      [B][S1][F] int32 bank entry per path point, F >= ceil(N / frame) + 1 (extra points are ignored); bank_of and
 *                             idx are clamped into range where they are read
 *   everything else as lh_render_binaural; peak, mixture and target keep its exact semantics.
 * LH_ERR_ARG: null pointer, a dimension <= 0, B * S1 > 65535, F < ceil(N / frame) + 1.  LH_ERR_UNSUPPORTED: frame % 8 != 0.
 * A refused call writes nothing.  No atomics in the FIR: bit-identical from call to call, and row b does not depend on the
 * other utterances.
 *
 * lh_path_nearest: idx[b][s][t] = the LOWEST j with the largest d_j = fmaf(v.z, p_j.z, fmaf(v.y, p_j.y, v.x * p_j.x)) in
 * fp32, v = paths[b][s][t], p_j = positions[bank_of[b]][j] (unit vectors: the caller converts SOFA coordinates; the scale
 * of v does not matter).  A zero vector gives 0; a non-finite point gives SOME index in [0, P).
 *   paths [B][S1][F][3], positions [K][P][3], bank_of [B] in [0, K), idx [B][S1][F] out
 * LH_ERR_ARG: null pointer, a dimension <= 0, B * S1 > 65535. */
int lh_path_nearest(const float* paths, const float* positions, const int* bank_of, int* idx, int B, int S1, int F, int P, int K,
                    lh_stream_t stream);
int lh_render_moving(const float* src, const float* bank, const int* bank_of, const int* idx, const float* gain,
                     const int* tgt_idx, float* events, unsigned* peak, float* mixture, float* target, int B, int S1, int N,
                     int Lh, int P, int K, int F, int frame, lh_stream_t stream);

/* Moving sources at room length (ABI 27): lh_render_moving's definition — the same f, w, blend, gain, peak, mixture, target,
 * clamping and refusals — with a and b_ computed by fp32 uniformly partitioned overlap-save instead of one fmaf chain each.
 * The cross-fade is on the output side, so the whole response of path point f (and f + 1) applies to all past input of the
 * outputs of frame f: nothing is approximated because the responses change.  The partitioning, integer arithmetic:
 *     FZ = 1024 (transform size),  m = max(1, (FZ + 1 - frame) / frame),  Lp = m * frame  (frame + Lp - 1 <= FZ),
 *     Q = ceil(Lh / Lp) partitions,  RING = (Q - 1) * m + 1 block spectra a frame looks back over,
 *     RUN = max(25, 2 * (RING - 1)) frames per workgroup
 *     block q = outputs [q frame, (q + 1) frame) = the last `frame` points of the inverse transform of
 *               sum_{j < Q, q - j m >= 0} X[q - j m] . H[j],  j ascending, one fp32 fmaf order
 *     X[q]    = transform of x[(q + 1) frame - FZ, (q + 1) frame), zeros outside [0, N)
 *     H[p][j] = transform of (hL + i hR)[j Lp, (j + 1) Lp) of entry p, zero-padded, scaled by 1 / FZ (both ears in one transform)
 * lh_bank_spectra writes the H of a whole bank; they depend on bank, Lh and frame only, so a caller with a fixed bank
 * computes them once.
 *   bank     [K][P][2][Lh]
 *   spec     [K][P][Q][FZ] complex fp32 (K * P * Q * 8 KiB), 16-byte aligned: an opaque image (the bins are in the
 *            transform's bit-reversed order) for lh_render_moving_fft with the same Lh and frame
 *   work     scratch of lh_render_moving_fft, 16-byte aligned: unused (may be NULL) when RING <= 16; else
 *            B * S1 * ceil(ceil(N / frame) / RUN) * RING * FZ complex fp32 (8 bytes each): the workgroups' block spectra
 *   everything else as lh_render_moving.
 * LH_ERR_ARG: as lh_render_moving, and a NULL or misaligned spec, or work where it is needed.  LH_ERR_UNSUPPORTED:
 * frame % 8 != 0, frame > 512 (2 frame - 1 must fit the transform), Lh > 16384.  A refused call writes nothing.  No atomics in
 * the convolution: bit-identical from call to call, row b does not depend on the other utterances, and a frame whose two path
 * points name one entry has the bits of that entry alone.  Every events row is within (4e-6 max(1, sqrt(Lh / 256)) + 2^-21) of
 * the float64 definition, relative to the row's largest |a|, |b_| times its gain (lh_render_moving's bound). */
int lh_bank_spectra(const float* bank, float* spec, int K, int P, int Lh, int frame, lh_stream_t stream);
int lh_render_moving_fft(const float* src, const float* spec, const int* bank_of, const int* idx, const float* gain,
                         const int* tgt_idx, float* events, unsigned* peak, float* mixture, float* target, float* work, int B,
                         int S1, int N, int Lh, int P, int K, int F, int frame, lh_stream_t stream);

/* Eval metrics on the device (reference src/ts_hear_test.py:139-146, torchmetrics SI-SNR restated): per utterance
 * output_sisnr, si_snr_i (both averaged over the 2 channels) and cosine(embedding, embedding_gt); fp64 moments.
 *   outputs, target, mixture [B][2][n_samples]; emb, emb_gt [B][emb_dim]
 *   scratch  fp64 workspace, B*2*16*8 + B*3 doubles
 *   rows     [B][3] fp32 = (output_sisnr, si_snr_i, embedding_sim)   (the CSV columns of ts_hear_test.py:149-151)
 *   sums     [4] fp64 = (sum si_snr_i, sum output_sisnr, sum embedding_sim, B): the all-reduce payload
 */
int lh_metric_sums(const float* outputs, const float* target, const float* mixture, const float* emb,
                   const float* emb_gt, double* scratch, float* rows, double* sums, int B, int n_samples,
                   int emb_dim, lh_stream_t stream);

/* Binaural cue errors on the device (ABI 15; reference src/eval/binaural.py: itd_diff, ild_diff, chunk_and_mask): per utterance
 * the change of the interaural time and level differences between the estimate and the target, from direct fp64 sums.
 *   est, gt   [B][2][n_samples] (channel 0 = left, 1 = right); sr = sample rate
 *   frame     0: static mode, one segment = the whole clip; > 0: moving mode, segments of `frame` samples (the reference's
 *             round(0.25 sr)), the last one zero-padded, counted when max over channels of sqrt(mean(gt^2)) over the frame
 *             is >= rms_threshold (ignored in static mode)
 *   per segment: ILD = 10 log10(sum L^2 / sum R^2); tau = argmax |cc[tau]| over tau = -t .. t (first maximum wins) of the
 *             circular cross-correlation cc[tau] = sum_n L[(n + tau) mod len] R[n], t = min(round(1e-3 sr), len / 2);
 *             ITD = tau / sr * 1e6 us
 *   scratch   fp64 workspace, B*C*(T*72 + 8) doubles, with len = (frame ? frame : n_samples), C = (frame ? ceil(n_samples /
 *             frame) : 1) segments and T = ceil(len / 4096) tiles per segment; its tail [B][C][8] holds the segment records
 *             (tau_est, tau_gt, ild_est, ild_gt, itd_est, itd_gt, counted, 0)
 *   rows      [B][2] fp64 = (delta_itd_us, delta_ild_db): static |ITD_est - ITD_gt|, |ILD_est - ILD_gt|; moving: the mean over
 *             counted segments of |ITD_est - ITD_gt|, and |mean ILD_est - mean ILD_gt|; NaN when no segment counts
 *   sums      [4] fp64 = (sum delta_itd over finite rows, count, sum delta_ild over finite rows, count)
 * LH_ERR_UNSUPPORTED unless 1 <= round(1e-3 sr) <= 16 (ties to even: sr 500 .. 16500), for an odd n_samples in static mode
 * and for an odd frame.  No atomics:
 * bit-identical from run to run, and row b does not depend on the other utterances of the batch.
 */
int lh_binaural_cues(const float* est, const float* gt, double* scratch, double* rows, double* sums, int B, int n_samples,
                     int sr, int frame, double rms_threshold, lh_stream_t stream);

/* ---- streaming sessions (ABI 16 - 20) ----------------------------------------------------------------------------------------
 * A batched streaming host serves S listener SLOTS in lock-step (one 8 ms chunk of every slot per step; slot = batch row of
 * every streaming entry point above).  These two launches bracket the chunk's launch sequence — first and last node of a
 * captured per-chunk graph — and let slots open, close and fail one at a time, on the device and without a host wait (the
 * reference has no counterpart: its streaming loop, `Net.predict(chunk, embed, state, pad=False)`, serves one listener).
 *   lh_span_t  one tensor of per-slot streaming state: slot s owns bytes [s * bytes, (s + 1) * bytes) from `base`; `base`
 *              and `bytes` are multiples of 16 (the store width).  lh_session_begin takes EVERY state tensor of the chunk
 *              loop (both ping-pong sets of conv / deconv / iSTFT tails and inter-LSTM h, c; every K / V ring: 4 ring rows
 *              per slot), lh_session_end the (h, c) tensors the chunk has just WRITTEN.  The table is a HOST array of
 *              n_spans <= LH_SESSION_MAX_SPANS entries: it is validated here and travels in the launch's own arguments (a
 *              captured graph keeps it), so no entry point reads device memory or waits.
 *   chunk_in   [S][2][192] the step's input as the clients sent it (never written);  chunk [S][2][192] what the separator
 *              reads: the row of a live slot, zeros for every other slot
 *   cmd        [2][S] words of LH_SESSION_* bits: row 0 posted by the host (one asynchronous copy ahead of the step), row 1
 *              posted by lh_session_end for the next chunk — separate words, so the host's copy cannot erase a RESET the
 *              device posted meanwhile.  lh_session_begin acts on row 0 | row 1; lh_session_end consumes both.
 *              Bits 8..30 of a host word with LH_SESSION_OPEN: the opening's generation (non-zero; a field of 0 becomes 1)
 *   active     [S] 0 = idle, else the generation of the slot's current opening
 *   fault      [S] DEVICE-ACCESSIBLE words the host reads in place (pinned host memory, written with system-scope vector
 *              stores like the range flag above): set to the generation of the opening the device closed
 *   out        [S][2][128] the chunk's output (lh_deconv_istft with keep_nonfinite = 1 and no range flag: nothing is hidden
 *              from lh_session_end)
 * Per slot, with c = cmd[0][s] | cmd[1][s]:  open = c has OPEN ? 1 : c has CLOSE ? 0 : active[s] != 0;  bad_in = open and one
 * of the 384 samples of chunk_in[s] is inf / NaN;  live = open and not bad_in.
 *   lh_session_begin  (grid over slot x tile) writes chunk[s] and, when c has RESET or bad_in, zeroes the slot's slice of
 *              every span with 16-byte stores: non-finite data never enters the separator kernels and a re-used slot keeps
 *              nothing of its previous listener.  It writes no word, so the workgroups of a slot all decide alike; a slot
 *              with nothing pending and finite input costs a few loads per wave.
 *   lh_session_end    (one workgroup per slot, the only writer of the words) overflow = live and a non-finite value in out[s]
 *              or in the slot's slice of a span (a true fp32 overflow from finite input);  active[s] = generation if live and
 *              not overflow, else 0;  fault[s] = 0 when c has OPEN, then the generation when bad_in or overflow;
 *              cmd[0][s] = 0, cmd[1][s] = overflow ? RESET : 0;  out[s] = 0 unless the slot is active now.
 * LH_ERR_ARG: null pointer, S <= 0, n_spans outside [1, LH_SESSION_MAX_SPANS] (lh_session_end: LH_SESSION_MAX_END_SPANS, the
 * (h, c) pairs of four blocks), a span with a null or unaligned base or a size that is 0 or not a multiple of 16.  Neither entry point allocates or synchronises. */
typedef struct { void* base; unsigned long long bytes; } lh_span_t;
enum { LH_SESSION_RESET = 1, LH_SESSION_OPEN = 2, LH_SESSION_CLOSE = 4, LH_SESSION_GEN_SHIFT = 8, LH_SESSION_MAX_SPANS = 32,
       LH_SESSION_MAX_END_SPANS = 8 };
int lh_session_begin(const lh_span_t* spans, int n_spans, const float* chunk_in, float* chunk, const unsigned* cmd,
                     const unsigned* active, int S, lh_stream_t stream);
int lh_session_end(const lh_span_t* spans, int n_spans, const float* chunk_in, float* out, unsigned* cmd, unsigned* active,
                   unsigned* fault, int S, lh_stream_t stream);

/* Row compaction (ABI 18): a host that is rarely full keeps its open listeners in the leading ROWS of the same buffers and
 * launches every kernel of the chunk for n_rows <= S of them.  SLOT stays the listener's number towards the clients (chunk_in,
 * out, fault, the enrollment words); ROW is the batch row of every streaming entry point, of the spans, of chunk and of the
 * words cmd [2][S] / active [S], whose stride stays S.  Call order of one chunk, all with the same n_rows:
 *   lh_session_move -> lh_session_begin_rows -> (lh_session_capture, by slot, S) -> the chunk's launches with B = n_rows ->
 *   lh_ring_advance -> lh_session_end_rows.
 *   from       [S] device words, the move table: from[d] = r + 1 copies row r over row d; 0, d + 1 and every value outside
 *              [1, S] = nothing.  Posted by the host with
 *              the other tables (one asynchronous copy ahead of the step), read by lh_session_move for d < n_rows, zeroed by
 *              lh_session_end_rows — a replay without a new table moves nothing.  The pairs of one launch must be disjoint:
 *              every source above, every destination below the host's new row count.
 *   slot_of    [S] row -> slot, negative or not below S = the row has no listener: it is idle whatever its words say (the
 *              host's word counts as CLOSE and nothing else; a RESET the device posted on it is still served), reads no
 *              input and reports nothing; its `active` and command words are still written
 *   row_of     [S] slot -> row, negative = none
 *   lh_session_move       (grid over row x tile; spans = lh_session_begin's table plus the speaker gain) copies the row's slice
 *              of every span with 16-byte loads and stores, active[r] -> active[d] and cmd[1][r] -> cmd[1][d].  Bytes, not
 *              numbers: a moved listener keeps its bits.  The source row is not cleared: the host takes its slot away
 *              (slot_of) or opens it for the next listener (OPEN comes with RESET).
 *   lh_session_begin_rows lh_session_begin for row r: decides from cmd[.][r], active[r] and chunk_in[slot_of[r]], writes
 *              chunk[r] and zeroes row r's slice of every span
 *   lh_session_end_rows   lh_session_end for row r (spans: the (h, c) just written): reads out_rows[r], writes it, or zeros, to
 *              out[slot_of[r]], fault[slot_of[r]], the words of row r, from[r] = 0 (from may be null); one more workgroup
 *              zeroes out[s] of every slot whose row_of[s] is not in [0, n_rows).  out_rows [S][2][128] is what
 *              lh_deconv_istft wrote, out [S][2][128] what the clients get.
 * A fault the host has not seen yet may travel with a move: the moved `active` word is then 0 and a pending RESET moves along,
 * so the row is idle and clean in its new place and the fault stays reported under the slot with its generation.
 * LH_ERR_ARG: as above, and n_rows outside [1, S], out_rows == out.  None of the three allocates or synchronises. */
int lh_session_move(const lh_span_t* spans, int n_spans, const int* from, unsigned* cmd, unsigned* active, int n_rows, int S,
                    lh_stream_t stream);
int lh_session_begin_rows(const lh_span_t* spans, int n_spans, const float* chunk_in, float* chunk, const unsigned* cmd,
                          const unsigned* active, const int* slot_of, int n_rows, int S, lh_stream_t stream);
int lh_session_end_rows(const lh_span_t* spans, int n_spans, const float* chunk_in, const float* out_rows, float* out,
                        unsigned* cmd, unsigned* active, unsigned* fault, const int* slot_of, const int* row_of, int* from,
                        int n_rows, int S, lh_stream_t stream);

/* Enrollment capture (ABI 17): "look once" from the listener's own stream.  One more node of the per-chunk graph, right after
 * lh_session_begin, in a host built for enrollment: an ARMED slot's next n_chunks input rows are recorded on the device, and a
 * word in pinned host memory tells the host when the clip is complete — the host then runs the enrollment embedder
 * (lh_emb_*) on it beside the chunk loop and opens the slot (LH_SESSION_OPEN) with the result, never waiting for the device.
 *   chunk_in   [S][2][192] as above (never written)
 *   enroll     [S][2][128 * n_chunks] fp32, 16-byte aligned: slot s, channel ch, chunk k of the capture -> samples
 *              [128 k, 128 k + 128) = samples [0, 128) of chunk_in[s][ch].  The 64 look-ahead samples of a row are the first
 *              64 new samples of the next row and are not recorded twice: a complete clip is the 128 * n_chunks contiguous
 *              stream samples from the arming chunk on.
 *   ecmd       [S] posted by the host like cmd (one asynchronous copy ahead of the step, only when something is pending):
 *              LH_ENROLL_ARM | generation << LH_ENROLL_GEN_SHIFT (generation in 1 .. 2^23 - 1), or LH_ENROLL_CANCEL.
 *              Consumed here: a posted word is written back as 0.
 *   estate     [2][S] device-owned, zero at start: row 0 the generation being captured (0 = none), row 1 the chunks recorded
 *   edone      [S] DEVICE-ACCESSIBLE words the host reads in place (pinned host memory, system-scope vector stores, like
 *              fault): `generation` once the n_chunks-th chunk is recorded, `generation | LH_ENROLL_FAULT` when the capture
 *              was aborted.  The clip itself is for stream-ordered readers: enqueue them after having seen the word.
 * Per slot and chunk (one wave per slot, the only writer of the slot's words and clip): CANCEL clears the state and writes
 * nothing to edone; ARM sets the generation and the count to 0 — also in mid-capture, which starts again; an armed slot
 * whose 256 samples to record hold an inf / NaN is disarmed with the FAULT word (a non-finite look-ahead sample alone is
 * judged when it becomes a recorded sample, in the next chunk); otherwise the samples are stored at the count, the count
 * advances and at n_chunks the slot is disarmed with the done word.  A disarmed slot's clip is not written until the next ARM.
 * The count lives on the device: the two alternating graphs have fixed arguments and a capture crosses both.
 * LH_ERR_ARG: null pointer, S <= 0, n_chunks < 1, chunk_in or enroll not 16-byte aligned.  Neither allocates nor synchronises. */
enum { LH_ENROLL_ARM = 1, LH_ENROLL_CANCEL = 2, LH_ENROLL_GEN_SHIFT = 8, LH_ENROLL_FAULT = 0x80000000u };
int lh_session_capture(const float* chunk_in, float* enroll, unsigned* ecmd, unsigned* estate, unsigned* edone, int n_chunks,
                       int S, lh_stream_t stream);

/* Monitor mix (ABI 30): what the listener hears is wet * separated + dry * room.  One more node of the per-chunk graph, after
 * lh_session_end[_rows][_paced] and ahead of lh_session_resample_out / lh_session_emit_s16, in a host built with a monitor.
 * It addresses everything by SLOT, in every flavour.  Output row j of a slot covers samples [128 j, 128 j + 128) of the slot's
 * stream, and those are samples [0, 128) of input row j: the dry path is the input row itself, with no delay line, and the
 * two paths are aligned to the sample behind whatever framing and resampling the host does around the 16 kHz rows.
 *   chunk_in   [S][2][192] as above (never written), 16-byte aligned
 *   out        [S][2][128] the rows lh_session_end* left, 16-byte aligned: a row that does not sound is exact zeros.  Mixed in
 *              place
 *   target     [2][S] fp32: the wet targets, then the dry targets, in [0, 1].  Posted by the host like hold (one asynchronous
 *              copy ahead of the step, only when one changed); read only
 *   gain       [2][S] fp32: the current wet and dry gains, device-owned; the host sets them to wet 1, dry 0 at start
 *   hold       [S] the hold words of a paced host, NULL in a lock-step host
 *   step       1.0f / (float)ramp_samples: a full 0 -> 1 swing takes ramp_samples samples at 16 kHz
 * Per slot and chunk (one wave per slot, the only writer of the slot's gains and row), for each of the two gains, with g0 its
 * value at the chunk's start and t its target:
 *     d = t - g0;   lim = (float)(n + 1) * step  (one fp32 multiply);   g(n) = |d| <= lim ? t : g0 + copysign(lim, d),  n = 0 .. 127
 * and afterwards gain = g(127): linear, monotone, exactly t at the end, and t may change in mid-ramp.  Then, in this order:
 *   1. hold[s] != 0: nothing is written — the row is the zeros the end entry point wrote — and both gains stay: the ramp
 *      resumes with the listener;
 *   2. wet g0 == t == 1 and dry g0 == t == 0 (the defaults, settled): the row is not touched and keeps the bits, signed zeros
 *      included, of a host without the node;
 *   3. dry g0 == t == 0: out = wet(n) * y.  The input row does not enter the result: a NaN there cannot leak through 0 * NaN;
 *   4. one of the 256 samples chunk_in[s][c][0 .. 127] is inf / NaN: the row is exact zeros, and the gains advance.  No fault
 *      is reported: an idle slot has none, an open slot's input was judged by lh_session_end.  The look-ahead samples
 *      128 .. 191 are not part of the row and are not looked at;
 *   5. otherwise out[s][c][n] = fmaf(wet(n), y, dry(n) * x[s][c][n]), y the row as found.
 * No atomics, nothing is read back, bit-identical from run to run.
 * LH_ERR_ARG: a null pointer (hold excepted), chunk_in or out not 16-byte aligned, target / gain / hold not 4-byte aligned,
 * target == gain, S <= 0, step not in (0, 1] (NaN included).  Neither allocates nor synchronises. */
int lh_session_mix(const float* chunk_in, float* out, const float* target, float* gain, const unsigned* hold, float step, int S,
                   lh_stream_t stream);

/* Paced sessions (ABI 19): a listener whose chunk is late is HELD for the step — the other slots are not stalled and the
 * held one is, after the step, bit for bit what it was before.  Every row owns its K / V ring position, so a listener's
 * samples depend on their own chunks only: not on when the slot was opened, not on who else was held.  The entry points
 * above with three more device arrays; their lock-step forms are untouched and a host uses one family or the other.
 *   hold       [S] words by SLOT (the row forms look them up through slot_of), non-zero = held in this step.  Posted by the
 *              host like cmd, only when the mask changes.
 *   pos        [S] the ROW's ring position in [0, 50), zero at start.  Written by lh_ring_advance_rows, copied by
 *              lh_session_move_paced with the row, by nothing else.
 *   write_pos  [S] per row, written by the begin entry points for lh_qkv_proj_ln_rows and lh_ring_advance_rows: -1 for a row
 *              that is held or not live, 0 for a row serving a RESET (OPEN comes with RESET), pos[r] otherwise.
 *   carry      2 n_pairs spans (host array, validated and passed like `spans`): carry[2 i] a state tensor the chunk READ,
 *              carry[2 i + 1] the tensor of the other ping-pong set it WROTE in its place — the conv, deconv and iSTFT tails
 *              and (h, c) of every block.  2 n_pairs <= LH_SESSION_MAX_SPANS, equal sizes, distinct bases.
 * Call order of one chunk:  (lh_session_move_paced ->) lh_session_begin[_rows]_paced -> (lh_session_capture_paced) ->
 * the chunk's launches with lh_qkv_proj_ln_rows(write_pos) in place of lh_qkv_proj_ln -> lh_ring_advance_rows ->
 * lh_session_end[_rows]_paced.
 * A held row:  its input row is not looked at (it may be NaN) and zeros go to the separator;  write_pos = -1, so no K / V row
 * is written and pos stays;  the end entry point passes no verdict on what the kernels made of the zeros, writes zeros to the
 * row's output and copies the row's slice of every carry[2 i] over carry[2 i + 1] with 16-byte loads and stores — bytes, not
 * numbers.  A held row costs what a live row costs: pacing buys correctness under jitter, not time.
 * Commands are served whether or not the row is held.  CLOSE: as above.  RESET (with OPEN): begin zeroes the state, so the
 * zeros are carried; the row is active; and end posts RESET again in cmd[1][r] for as long as the row is held, so the chunk
 * that takes the listener's first samples zeroes once more and starts the ring at slot 0.
 * A capturing slot that is held serves ARM / CANCEL, records nothing and is not judged: the clip is the samples of the
 * chunks the slot was present for.
 * LH_ERR_ARG: as for the lock-step forms, and a null hold / pos / write_pos, pos == write_pos, n_pairs < 1 or too many, a pair
 * of unequal sizes or one tensor twice.  None of them allocates or synchronises. */
int lh_session_begin_paced(const lh_span_t* spans, int n_spans, const float* chunk_in, float* chunk, const unsigned* cmd,
                           const unsigned* active, const unsigned* hold, const int* pos, int* write_pos, int S,
                           lh_stream_t stream);
int lh_session_end_paced(const lh_span_t* spans, int n_spans, const lh_span_t* carry, int n_pairs, const float* chunk_in,
                         float* out, unsigned* cmd, unsigned* active, unsigned* fault, const unsigned* hold, int S,
                         lh_stream_t stream);
int lh_session_move_paced(const lh_span_t* spans, int n_spans, const int* from, unsigned* cmd, unsigned* active, int* pos,
                          int n_rows, int S, lh_stream_t stream);
int lh_session_begin_rows_paced(const lh_span_t* spans, int n_spans, const float* chunk_in, float* chunk, const unsigned* cmd,
                                const unsigned* active, const int* slot_of, const unsigned* hold, const int* pos,
                                int* write_pos, int n_rows, int S, lh_stream_t stream);
int lh_session_end_rows_paced(const lh_span_t* spans, int n_spans, const lh_span_t* carry, int n_pairs, const float* chunk_in,
                              const float* out_rows, float* out, unsigned* cmd, unsigned* active, unsigned* fault,
                              const unsigned* hold, const int* slot_of, const int* row_of, int* from, int n_rows, int S,
                              lh_stream_t stream);
int lh_session_capture_paced(const float* chunk_in, float* enroll, unsigned* ecmd, unsigned* estate, unsigned* edone,
                             const unsigned* hold, int n_chunks, int S, lh_stream_t stream);

/* Suspend / resume (ABI 20): one listener's state leaves the buffers of a session host as bytes — a SNAPSHOT — and enters any
 * row of any host of the same model: to park a listener who is away, to move one to another host or GPU, to keep a session
 * across a restart.  Two launches that the host enqueues between two chunks (not nodes of a captured graph, and only in a step
 * that suspends or resumes): both copy bytes, not numbers, with 16-byte loads and stores over a grid of (tile, section).
 * Snapshot layout, every section at a multiple of 16 bytes, little endian, `snap` 16-byte aligned:
 *   0     header, LH_SNAPSHOT_HEADER_BYTES = 64 words:  [0] LH_SNAPSHOT_MAGIC  [1] LH_SNAPSHOT_VERSION  [2] total bytes
 *         [3] n_flat  [4] n_rings  [5] heads  [6] window  [7] embed_bytes  [8 ..) bytes of each flat span, then the row bytes
 *         of each ring; the rest 0.  Written by lh_session_save from its own arguments.
 *   256   words:  [0] active[row]  [1] cmd[1][row]  [2] ring position in [0, window)  [3] 0
 *   272   the speaker embedding, embed_bytes
 *   ...   the row's slice of flat span 0, 1, ..: the tails and (h, c) of the LIVE ping-pong set (the one the next chunk reads)
 *   ...   ring 0, 1, ..: [heads][window][row bytes] — the window rows only, in ring order; the LH_KV_PAD_ROWS zero rows and the
 *         dead ping-pong set are not part of a listener
 * About 5.4 MB for the 3-block model against ~10 MB that a row occupies.
 *   flat       host table like lh_session_begin's (validated here, travels in the launch arguments): n_flat in
 *              [1, LH_SESSION_MAX_SPANS] tensors of which row r owns bytes [r * bytes, (r + 1) * bytes)
 *   rings      host table of n_rings in [1, LH_SNAPSHOT_MAX_RINGS] K / V rings; `bytes` is the size of ONE ring row (a multiple
 *              of 16).  Row r owns heads * ring_rows ring rows from row r * heads * ring_rows on, of which the first `window`
 *              of every head are copied;  1 <= window <= ring_rows
 *   embed      the listener's speaker embedding [embed_bytes], 16-byte aligned, embed_bytes a positive multiple of 16
 *   cmd, active  the words of the bracket kernels, stride S;  row in [0, S)
 * lh_session_save     reads row `row` and the device word `pos` — the row's own position of a paced host, the shared counter of
 *              a lock-step one — and writes every byte of the layout.  The host's buffers are not written.
 * lh_session_restore  writes the same sections into row `row` (the flat spans are those of the TARGET's live set), cmd[1][row]
 *              from the snapshot, and the embedding; pad rows, the other rows and the dead set are untouched.  Exactly one of
 *              pos_row / pos_shared is given.  pos_row (a paced target: the row's own position word): ring rows go back where
 *              they were and *pos_row = the saved position — the raw order is what makes the continuation bit-identical.
 *              pos_shared (a lock-step target: the shared counter, read only): ring row j goes to (j + delta) mod window with
 *              delta = (*pos_shared - saved position) mod window, so the listener's oldest row is again the next one the
 *              counter overwrites.  The host then opens the row with LH_SESSION_OPEN | generation and NO RESET: restore has
 *              written every byte a RESET would zero that the chunk does not rewrite itself.
 *              A DEAD snapshot — words[0] == 0: the device had closed the listener in the chunk before the save — must not come
 *              alive: restore then overwrites the host's command cmd[0][row] with CLOSE | RESET and stores `gen`, the
 *              generation of the opening the host has posted, to *fault (the slot's fault word, written like lh_session_end
 *              does): the row is idle and zeroed, and the host learns of the fault as of any other.  Enqueue restore AFTER
 *              the step's copy of the host's command words for that reason.  A non-zero words[0] with RESET in words[1] is a
 *              paced listener opened and held who has consumed nothing: alive, the RESET travels and is served.
 * State is only meaningful under the weights it was computed with; neither entry point can check that.
 * LH_ERR_ARG: null or unaligned pointer, a table entry as for lh_session_begin, bad counts (n_flat + n_rings > 56, heads < 1,
 * window outside [1, ring_rows]), row outside [0, S), snap_bytes smaller than the layout or the layout 2^31 bytes or more;
 * restore: both or neither of pos_row / pos_shared, gen outside [1, 2^23).  Neither allocates, synchronises or reads device
 * memory on the host. */
enum { LH_SNAPSHOT_MAGIC = 0x5353484c /* "LHSS" */, LH_SNAPSHOT_VERSION = 1, LH_SNAPSHOT_HEADER_BYTES = 256,
       LH_SNAPSHOT_MAX_RINGS = 8 };
int lh_session_save(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads, int ring_rows,
                    int window, const void* embed, int embed_bytes, void* snap, unsigned long long snap_bytes,
                    const unsigned* cmd, const unsigned* active, const int* pos, int row, int S, lh_stream_t stream);
int lh_session_restore(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads, int ring_rows,
                       int window, void* embed, int embed_bytes, const void* snap, unsigned long long snap_bytes,
                       unsigned* cmd, int* pos_row, const int* pos_shared, unsigned* fault, int gen, int row, int S,
                       lh_stream_t stream);

/* Suspend / resume of many listeners (ABI 21): the two launches above for any number of listeners at once — draining a GPU,
 * rebalancing, adopting another host's listeners between two chunks.  ONE launch each, whatever n_items is: the grid is
 * (tile, section, item).  The single forms are what they were.  Arguments as above, except:
 *   items      table of n_items entries in DEVICE memory (4-byte aligned), n_items in [1, S].  Item i acts on row items[i].row,
 *              whose listener is slot items[i].slot; its snapshot lies at snaps + items[i].index * snap_stride; `gen` (restore
 *              only) is the generation of the opening the host has posted for the slot, what the single form takes as `gen`.
 *              The host hands out distinct rows and slots (and, for save, distinct indexes); restore may name any subset of a
 *              buffer's snapshots.  On the device an item whose row or slot is outside [0, S) or whose index is negative is
 *              skipped whole, by every workgroup, before an address is formed; that `index` stays inside the caller's buffer is
 *              the caller's to keep — the entry points do not know its size.
 *   snaps, snap_stride   a [.][snap_stride] buffer, 16-byte aligned, snap_stride a multiple of 16 and at least the layout's
 *              bytes.  Save writes the first `layout` bytes of a snapshot — byte for byte what lh_session_save writes for that
 *              row — and not the padding up to snap_stride.
 *   embed      [S][embed_bytes], by SLOT (the single forms take the listener's own).   fault  [S] by slot.
 *   pos_rows / pos_shared   exactly one.  pos_rows: [S] by row, a paced host's position words — save reads, restore writes
 *              pos_rows[row].  pos_shared: a lock-step host's counter — read by both; restore rotates every item by its own
 *              delta = (*pos_shared - its saved position) mod window.
 * Tiles per (item, section): 32, as in the single forms, for any n_items (measured flat from 4 to 64 tiles with 64 listeners
 * in flight, profiles/suspend_many_cost.txt); lh_set_tuning(18, n) sets another count for A/B runs, 0 = 32.
 * lh_embed_proj_ln_rows: lh_embed_proj_ln for the rows of such a table, in the same two kernels whatever n_items is —
 * gain[items[i].row] from embed[items[i].slot], both [S][.]; scratch [S][6208] by row.  A row's bits are those of
 * lh_embed_proj_ln on that row alone.  Items outside [0, S) are skipped; `index` and `gen` are not looked at.
 * LH_ERR_ARG: what the single forms refuse, n_items outside [1, S], a null or misaligned items, snap_stride smaller than the
 * layout or not a multiple of 16, both or neither of pos_rows / pos_shared.  None allocates, synchronises or reads device
 * memory on the host. */
typedef struct { int row; int slot; unsigned gen; int index; } lh_snap_item_t;   /* 16 bytes */
int lh_session_save_rows(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads, int ring_rows,
                         int window, const void* embed, int embed_bytes, void* snaps, unsigned long long snap_stride,
                         const unsigned* cmd, const unsigned* active, const int* pos_rows, const int* pos_shared,
                         const lh_snap_item_t* items, int n_items, int S, lh_stream_t stream);
int lh_session_restore_rows(const lh_span_t* flat, int n_flat, const lh_span_t* rings, int n_rings, int heads, int ring_rows,
                            int window, void* embed, int embed_bytes, const void* snaps, unsigned long long snap_stride,
                            unsigned* cmd, int* pos_rows, const int* pos_shared, unsigned* fault, const lh_snap_item_t* items,
                            int n_items, int S, lh_stream_t stream);
int lh_embed_proj_ln_rows(const float* embed, const float* w, const float* bias, const float* ln_w, const float* ln_b,
                          float* scratch, float* gain, const lh_snap_item_t* items, int n_items, int S, lh_stream_t stream);

/* Packets (ABI 22): the transport side of a paced host.  Clients send contiguous PCM in packets of any size, fp32 or 16-bit;
 * the device keeps a small input FIFO per slot, cuts its own [2][192] windows (128 new samples + 64 look-ahead) into chunk_in
 * and decides by itself which slots are present — the host copies neither windows nor hold words.  Everything behind chunk_in
 * and hold is the paced family above, unchanged.
 *   fifo       [S][2][R] fp32, 16-byte aligned: a ring per slot and channel.  R a power of two, 256 <= R <= 2^24.
 *   wr, rd     [S] each, 32-bit SAMPLE COUNTERS that wrap modulo 2^32 (at 16 kHz: after 74 hours), zero at start.  R divides
 *              2^32, so sample c lives at ring index c & (R - 1) and the fill is the unsigned difference wr[s] - rd[s], both
 *              across the wrap.  rd only ever moves by 128 from 0: every window starts on a multiple of 128 samples and meets
 *              the ring's end only at a multiple of 64, so windows move 16 bytes at a time.
 *   staging    device buffer with the samples of one tick's packets, 4-byte aligned, staging_bytes long; `format` says what an
 *              element is: LH_FEED_F32 (4 bytes, copied as bit patterns) or LH_FEED_S16 (2 bytes, value * 2^-15: exact).
 *   items      table of n_items >= 1 entries in DEVICE memory (4-byte aligned).  Item i is one packet of items[i].n samples for
 *              slot items[i].slot, planar in staging: channel 0 at elements [offset, offset + n), channel 1 at
 *              [offset + n, offset + 2 n).  `at` is the slot's write counter before the packet — the HOST's mirror of wr[slot].
 *              flags: LH_FEED_FLUSH drops the slot's buffered input first: rd[slot] = 0 and `at` is taken as 0; n = 0 is legal.
 *              The host hands out at most one item per slot per call, and never more than R - (wr - rd) samples: the entry
 *              points cannot know that, a ring that is overrun loses its oldest samples.
 * Who writes which word:
 *   lh_session_feed   (an eager launch between two chunks, like lh_session_restore_rows; grid over tile x item) stores sample i
 *              of an item to fifo[slot][ch][(at + i) & (R - 1)] and, one thread per item, wr[slot] = at + n (FLUSH: and
 *              rd[slot] = 0).  No thread READS wr, so the workgroups of an item have nothing to race on.  Skipped whole, by every
 *              workgroup and before any address is formed: an item whose slot is outside [0, S), whose n is negative or larger
 *              than R, or whose samples would reach outside [0, staging_bytes).
 *   lh_session_frame  (the FIRST node of the chunk's graph; one wave per slot, the only writer of hold[s] and the only other
 *              writer of rd[s]; it reads both counters before it writes either word)  avail = wr[s] - rd[s].  avail >= 192:
 *              samples [rd, rd + 192) of both channels go to chunk_in[s], hold[s] = 0, rd[s] += 128.  Otherwise hold[s] = 1 and
 *              chunk_in[s] is not touched — no paced kernel looks at a held row's input.  It does not ask what the slot is:
 *              open, capturing and idle slots are framed alike, as the lock-step forms gate an idle slot's row.
 *   lh_session_emit_s16  (a node after lh_session_end[_rows]_paced, in a host that answers in 16-bit PCM)  out [S][2][128] fp32 ->
 *              out16 [S][2][128] int16, both 16-byte aligned:  y = clamp(rint(32768 x), -32768, 32767), round half even,
 *              saturating, NaN -> 0 (the end kernel has zeroed every faulted or held row, so none arrives from a session).
 * The feed launch and the chunk's graph are ordered by the stream, and the host mirrors both counters with the same arithmetic:
 * it knows what every launch will find, the device follows, and no word is ever read back.
 * LH_ERR_ARG: null or misaligned pointer, wr == rd, S <= 0, R not a power of two in [256, 2^24], n_items outside [1, 65535],
 * an unknown format, out == out16.  None of the three allocates, synchronises or reads device memory on the host. */
enum { LH_FEED_F32 = 0, LH_FEED_S16 = 1, LH_FEED_FLUSH = 1 };
typedef struct { int slot; int offset; int n; unsigned at; unsigned flags; } lh_feed_item_t;   /* 20 bytes */
int lh_session_feed(const void* staging, unsigned long long staging_bytes, int format, const lh_feed_item_t* items, int n_items,
                    float* fifo, unsigned* wr, unsigned* rd, int R, int S, lh_stream_t stream);
int lh_session_frame(const float* fifo, const unsigned* wr, unsigned* rd, float* chunk_in, unsigned* hold, int R, int S,
                     lh_stream_t stream);
int lh_session_emit_s16(const float* out, short* out16, int S, lh_stream_t stream);

/* Client rate (ABI 23): polyphase sinc resampling, offline for the data pipeline and per slot for a packet host whose clients
 * capture and play at their own rate (48, 32, 24, 8 kHz ...).  The arithmetic is torchaudio's published `sinc_interp_hann`
 * algorithm, restated (csrc/lh_resample.h; lookoncetohear_amd/resample.py makes the bank):
 *     g = gcd(orig, new), o = orig / g, n = new / g, K = 2 width + o
 *     y[q n + p] = sum_{k < K} xpad[q o + k] * bank[p][k]          xpad = width zeros, x, width + o zeros
 *     len(y) = ceil(n len(x) / o)
 *   bank      [n][K] fp32 in device memory, made in fp64 on the host and cast.
 * Every kernel accumulates alike — one fp32 accumulator from +0, one fmaf per tap, ascending k — so a stream that went through
 * the session nodes in packets of any size carries the bits of lh_resample of the whole stream.
 *   lh_resample   x [rows][n_in] (16-byte aligned) -> y [rows][n_out], n_out = ceil(n_in n / o); one launch.
 *   lh_session_resample_in   (an eager launch, behind the lh_session_feed of the same tick)  lh_session_feed, unchanged, lands the
 *              client-rate packets in a second ring raw [S][2][R_in] with two counters of its own; this launch turns whole
 *              blocks of it into 16 kHz samples of the fifo of the packets section and stores wr[slot] — the only other writer of
 *              that word.  items: n_items >= 1 entries in DEVICE memory.  Item i makes items[i].blocks blocks (blocks * n
 *              samples per channel) for items[i].slot: sample j goes to fifo[slot][ch][(wr + j) & (R - 1)], its taps are raw
 *              samples [tap + (j / n) o, tap + (j / n) o + K) at ring index counter & (R_in - 1); then wr[slot] = wr + blocks n.
 *              `wr` is the slot's 16 kHz write counter before the item, `tap` the raw counter of the first block's first tap —
 *              both the HOST's mirrors, modulo 2^32: the kernel reads no counter.  A stream starts at raw counter 0 with
 *              tap = -width: the host zeroes the slot's raw ring when it flushes it, and those zeros are the left pad.  The host
 *              hands out a block only when all K of its samples have been pushed.  Skipped whole: an item whose slot is outside
 *              [0, S), whose blocks are negative, make more than R samples or read more than R_in.
 *   lh_session_resample_out  (a graph node after lh_session_end[_rows]_paced, one workgroup per slot; in a client-rate host it
 *              takes the place of lh_session_emit_s16)  out [S][2][128] at 16 kHz and tail [S][2][T], T = width + D o,
 *              D = ceil((width + o) / o), zero at start -> out_client [S][2][128 n / o]; o must divide 128.  Step t emits
 *              blocks [Q t - D, Q (t + 1) - D), Q = 128 / o, of the resampled stream of rows: lh_resample of D o zeros followed by
 *              the rows, a fixed delay of D o samples at 16 kHz.  Then the tail is the last T samples of (tail, row).
 *              format: LH_FEED_F32 (float rows) or LH_FEED_S16 (int16 rows, the rounding of lh_session_emit_s16).
 *              hold[s] != 0: a zero row, and the slot's tail is not advanced.
 * LH_ERR_ARG: null or misaligned pointer (x, raw, fifo, out, out_client: 16 bytes), aliased buffers, o or n outside [1, 4096],
 * width < 1 or o + 2 width + 8 > 8192, n_out not ceil(n_in n / o), rows outside [1, 65535], R or R_in not a power of two in
 * [256, 2^24], R_in < K (too few samples for one block), n_items outside [1, 65535], S <= 0, an unknown format, o not a divisor
 * of 128 or T > 896 (lh_session_resample_out).  None of the three allocates, synchronises or reads device memory on the host. */
typedef struct { int slot; int blocks; unsigned wr; unsigned tap; } lh_resample_item_t;   /* 16 bytes */
int lh_resample(const float* x, float* y, const float* bank, int rows, int n_in, int n_out, int o, int n, int width,
                lh_stream_t stream);
int lh_session_resample_in(const float* raw, int R_in, const lh_resample_item_t* items, int n_items, float* fifo, unsigned* wr,
                           int R, int S, const float* bank, int o, int n, int width, lh_stream_t stream);
int lh_session_resample_out(const float* out, float* tail, const unsigned* hold, void* out_client, int format, int S,
                            const float* bank, int o, int n, int width, lh_stream_t stream);

/* Any rate (ABI 31): the out node for client rates that are no multiple of 125 Hz — 44 100 Hz (o = 160, n = 441), 22 050, 11 025,
 * 88 200 — where a 128-sample chunk is not a whole number of client samples (352.8 at 44.1 kHz).  The hop is FRACTIONAL: a live
 * step of a slot yields floor(128 n / o) or ceil(128 n / o) samples, counted on the device and mirrored by the host in the same
 * integers, so nothing is read back.  With (width, o, n) of the 16 kHz -> client bank and K = 2 width + o:
 *     d = width + o - 1          the delay at 16 kHz: the least at which every tap of a step's outputs lies in rows already made
 *     P = o / gcd(128, o)        live steps per period (5 for 44.1 / 22.05 / 11.025 kHz, 1 where o divides 128)
 *     r in [0, P)                the slot's phase: live steps taken, mod P;   c(r) = floor(128 r n / o)
 *     T = K + o + ceil(o / n) - 1        carried samples (334 toward 44.1 kHz, 1299 toward 11.025 kHz)
 * A live step at phase r emits samples m in [c(r), c(r + 1)) of the current period; with m = q n + p and xs = the slot's tail
 * followed by the chunk's 128-sample row,
 *     sample m = sum_{k < K} xs[q o - width - d - 128 r + T + k] * bank[p][k]
 * in the arithmetic above (one fp32 accumulator from +0, one fmaf per tap, ascending k, no tap skipped).  Then the tail is the
 * last T samples of xs and the phase (r + 1) mod P.  The zeroed tail at start is the left pad and the delay in one: the
 * concatenation of a slot's live steps equals lh_resample of d zeros followed by its live rows, bit for bit.  Toward 44.1 kHz the
 * counts of a period are 352, 353, 353, 353, 353.
 *   out        [S][2][128]  the 16 kHz rows                      tail   [S][2][T], zero at start
 *   phase      [S] unsigned, zero at start: the kernel is its only writer besides the host's zeroing (flush, reset).  A word
 *              outside [0, P) is reduced mod P before any index is formed: no value of it moves an address out of the staged span
 *   hold       [S]; hold[s] != 0: a zero row, count 0, tail and phase untouched
 *   out_client [S][2][hop_max], hop_max = ceil(128 n / o), float (LH_FEED_F32) or int16 (LH_FEED_S16, the rounding of
 *              lh_session_emit_s16); samples at and beyond the slot's count are zeros.  Rows of 353 samples cannot be aligned:
 *              only the base pointers of out, tail and out_client need 16 bytes
 *   count      [S] int: the valid samples of each slot's row in this step
 *   bank_t     [K][n] fp32: the TRANSPOSED image of the bank (the same values), so that the 64 consecutive phases of a wave read
 *              64 consecutive floats per tap
 * One workgroup per slot, [tail | row] staged in LDS: 1427 floats per channel, what 11 025 Hz needs.
 * LH_ERR_ARG: a null or misaligned pointer, two arguments naming one buffer, o or n outside [1, 4096], width < 1, T + 128 > 1427,
 * an unknown format, S <= 0.  Does not allocate, synchronise or read device memory on the host. */
int lh_session_resample_out_any(const float* out, float* tail, unsigned* phase, const unsigned* hold, void* out_client, int* count,
                                int format, int S, const float* bank_t, int o, int n, int width, lh_stream_t stream);

/* The path's ONE exchange step, for hosts that drive this ABI without Python: all-reduce (sum) of the
 * fp64 metric sums written by lh_metric_sums over one process per GPU — RCCL over xGMI, 32 bytes, latency-bound.
 * Replaces the reference's Lightning `sync_dist` all-reduce (src/ts_hear_embed_pl_module.py:82-107).  RCCL is bound
 * with dlopen at the first call (LOOKONCE_RCCL_LIB overrides the name; an RCCL already mapped into the process is
 * reused): LH_ERR_UNSUPPORTED when no RCCL can be found.  The Python host uses torch.distributed instead.
 *   lh_comm_unique_id  rank 0: 128 opaque bytes to hand to every rank through the host's own channel (ncclGetUniqueId)
 *   lh_comm_init       collective over all ranks, on each rank's current device (ncclCommInitRank)
 *   lh_allreduce_f64   in place, on `stream` (ncclAllReduce, ncclFloat64, ncclSum)
 */
int lh_comm_unique_id(void* id128);
int lh_comm_init(const void* id128, int n_ranks, int rank, void** comm);
int lh_allreduce_f64(void* comm, double* buf, int count, lh_stream_t stream);
int lh_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* LOOKONCE_HIP_H */
