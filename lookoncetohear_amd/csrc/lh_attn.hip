// Local (50-slot) causal attention with fused head merge, SURVEY.md §8a rows a15-a18.
//
// The reference materialises a 50x sliding-window copy of K and V (`_causal_unfold_chunk`,
// tfgridnet_causal.py:429-454: 67 % of its CPU time).  Here a workgroup owns TQ = 16*MQ consecutive query frames of
// one (batch, head): the TQ+49 history-extended K/V rows they can see are read ONCE from the ring-extended buffers.
//
// Q, K and V arrive as split-precision fp16 pairs (v = hi + lo, lo un-rescaled; written by k_qkv_proj_ln in exactly the
// order the v_mfma_f32_16x16x32_f16 operands want, lh_common.h), so both contractions run as three fp16 MFMAs per tile
// (hi*hi + hi*lo + lo*hi into one accumulator, ~22 mantissa bits) with no conversion work in this kernel:
//   * scores  S = Q K^T: banded tile products (query tile mq x key tiles mq..mq+4), the 19 feature k-steps split
//     over the 4 waves, partial sums reduced through LDS (79-frame tiles: whole products per wave, no partial sums);
//     A and B fragments are 32-byte row segments straight from global memory (two-deep register ring);
//   * softmax over exactly the 50 in-window slots (zero history rows take part, no mask — reference behaviour),
//     P written to LDS as fp16 hi/lo rows;
//   * O = P V: per 32-key step a lane loads the [hi 4 | lo 4] quads of 8 key rows for its 4 columns (256-byte row
//     segments per 16 lanes) and regroups them lane-locally into the four column tiles' B operands; the three key
//     steps form a register ring that is refilled for the wave's next column group right after use.
// The output keeps the head-major order [B][T][head][97][16] (full-line stores) — the projection kernel reads it in
// that order.  Workgroups of one (batch, head) are placed on one XCD (blockIdx % 8) so neighbouring tiles re-read
// the shared 49 rows from that XCD's L2 instead of HBM.  kx / vx carry KV_PAD zero rows behind row T+48: tiles
// read (never need) up to 47 rows past their last key and 0 * finite = 0.
#include "lh_common.h"
#include "lh_cachepol.h"

namespace lh {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
struct Frag { f16x8 h, l; };               // 8 k-values of one operand row: hi and lo halves
struct VQuad { f16x4 h, l; };              // one key row, 4 columns

constexpr int AT_KSTEPS = (DQKP + 31) / 32;   // 19 feature k-steps of 32
constexpr int AT_CG = (DV + 63) / 64;         // 25 column groups of 64 V columns

#if defined(LH_PROBE_TRACE)               // timing probe build only (scripts/probe_trace.py): workgroup 803, wave 0
__device__ unsigned long long lh_attn_trace_buf[16];
#define AT_STAMP(k) do { if (blockIdx.x == 803 && blockIdx.y == 0 && tid == 0) lh_attn_trace_buf[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define AT_STAMP(k) do { } while (0)
#endif
// RMAP (ABI 32, lh_local_attn_ring: a streaming chunk of T <= 16 frames, one tile, t0 = 0) is a template flag: the first
// R = HIST + T rows of kx / vx are a persistent ring and logical history-extended row n lives in physical row
// (*ring_pos + T + n) mod R for n < R; rows n >= R (read, never needed) are the zero pad rows, physical row n (R >= 50 keeps
// them inside the buffer).  The map goes into the K row offsets and the V row bases, computed once per lane; the loops, the
// MFMA order and so the bits are those of the contiguous kernel.  The last argument is the ring position word — an empty
// struct in every other instantiation, which stay the code they were.
struct NoRing {};
template <bool RMAP> struct RingWord { typedef NoRing type; };
template <> struct RingWord<true> { typedef const int* type; };
template <int MQ, int RING, int TQ = 16 * MQ, bool RMAP = false, int POL = 0>      // POL: cache policy of Q, K, V and merged (lh_cachepol.h)
__global__ void __launch_bounds__(256, 2) k_local_attn(const _Float16* __restrict__ q, const _Float16* __restrict__ kx,
                                                       const _Float16* __restrict__ vx, float* __restrict__ merged,
                                                       int BH, int T, int ntt, int tw0, int tend,
                                                       typename RingWord<RMAP>::type ring_pos) {
    // TQ query frames per workgroup in MQ MFMA row tiles (TQ = 16 MQ, or 40 in 3 tiles: 625 frames are then 16 tiles
    // per (batch, head), 2048 workgroups at batch 32 = exactly four rounds of the 512 resident workgroups; or 79 in 5
    // tiles: 8 tiles per (batch, head), two rounds — attn_form below)
    constexpr int NKEYS = TQ + HIST;           // key rows they can see (65 / 81 / 89 / 128)
    constexpr int NKT = (NKEYS + 15) / 16;     // key tiles in the score phase (5 / 6 / 8)
    constexpr int NK = NKT * 16;
    constexpr int ND = 5;                      // key tiles per query tile: nt = mq .. mq+4 (as far as they exist)
    constexpr int NB = ND * 16;                // band width stored per query row
    constexpr int PKS = (NKEYS + 31) / 32;     // 32-key steps in P.V (3; 79-frame tiles: 128 keys = exactly 4)
    constexpr int PP = PKS * 32 + 8;           // P row stride in halves (208 / 272 bytes: conflict-free ds_read_b128)
    // OWN (79-frame tiles, MQ = 5): a wave owns whole tile products over all 19 k-steps — the five of query tile `wave` and
    // product (4, 4 + wave) of the band's 24 — instead of every product over a quarter of the k-steps.  No partial sums:
    // `sp` is one copy (25 KB; four copies of an 80 x 80 band would be 102 KB), and 69 KB of LDS keep two workgroups per CU.
    constexpr bool OWN = MQ > 4;
    // OWN reads 128 key rows, 30 more than the pad rows cover behind a tile that starts at the clip's last frame.  A tile whose
    // rows 96..127 would lie behind the buffer (t0 > T - 31) has fewer than 31 frames, and keys 96..127 belong to queries 47..78
    // only: it reads rows 64..95 a second time in their place (KBACK) — scores nobody uses, and P is exactly 0 there.
    constexpr int KBACK = OWN ? 32 : 0;
    static_assert(TQ <= 16 * MQ && TQ > 16 * (MQ - 1) && NK - 1 - KBACK <= HIST + KV_PAD, "tile geometry");
    static_assert(!OWN || (MQ == 5 && NKT == 8 && NKEYS == PKS * 32), "wave-owned products: 4 x 5 + 4 of the band");
    // frames of a pulled-back tile < NK - HIST - KV_PAD <= NK - KBACK - HIST = the first query that sees key NK - KBACK
    static_assert(KBACK <= KV_PAD && KBACK % 32 == 0, "a pulled-back tile has no query that sees the rows it replaces");
    static_assert(!RMAP || (MQ == 1 && TQ == 16), "the ring map serves the one-tile form");
    __shared__ __attribute__((aligned(16))) float sp[OWN ? 1 : 4][TQ][NB];  // (per-wave partial) scores, band-relative columns (d, l15)
    __shared__ __attribute__((aligned(16))) _Float16 ph[16 * MQ][PP];
    __shared__ __attribute__((aligned(16))) _Float16 pl[16 * MQ][PP];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(tid), g4 = lane >> 4, l15 = lane & 15;
    // XCD-aware placement: the tiles of (batch, head) bh all run on XCD bh % 8
    const int xcd = blockIdx.x & 7, kk = blockIdx.x >> 3;
    const int bh = (kk / ntt) * 8 + xcd;
    const int t0 = tw0 + (kk % ntt) * TQ;        // time window [tw0, tend) of the T frames (lh_local_attn_win; whole clip: 0, T)
    if (bh >= BH) return;
    const long TKP = T + HIST + KV_PAD;
    const _Float16* qb = q + (long)bh * T * LDQKH;
    const _Float16* kb = kx + ((long)bh * TKP + t0) * LDQKH;
    const _Float16* vb = vx + ((long)bh * TKP + t0) * LDVH;
    const int kback = t0 + NK - 1 > T + HIST + KV_PAD - 1 ? KBACK : 0;      // scalar: rows the last 32 key rows are pulled back by
    // RMAP: physical row of logical row n (t0 = 0).  rbase = (*ring_pos + T) mod R is scalar; unsigned: never before the ring
    int rrows = 0, rbase = 0;
    if constexpr (RMAP) {
        rrows = HIST + T;
        rbase = (int)(((unsigned)*ring_pos + (unsigned)T) % (unsigned)rrows);
    }
    auto xrow = [&](int n) -> int {
        if constexpr (RMAP) {
            const int p = rbase + n;
            return n >= rrows ? n : p >= rrows ? p - rrows : p;
        } else {
            return n;
        }
    };

    AT_STAMP(0);
    // ---- scores: S[i][n] = <Q[t0+i], Kx[t0+n]>
    if constexpr (OWN) {
        // Every product sums k-steps ascending, hi*hi, hi*lo, lo*hi.  A wave's six products take Q tile `wave` (its own: straight
        // from global memory) and Q tile 4 and K tiles wave .. wave+4 (key tile 4 + wave is the last of them), which its
        // neighbours take too: fetched per wave, 28 fragments a k-step for 13 different ones, the phase ran at the rate of the
        // bytes it ASKED for (the two workgroups of a CU have four times L1's 32 KB in flight, a line is gone before the next wave
        // asks: 170e3 cycles of a workgroup's 282e3, profiles/attn_wide_tile_ab.txt).  So the workgroup loads the 8 K tiles and Q
        // tile 4 of a k-step once, 4.5 16-byte chunks per thread, and shares them through LDS: two staging buffers of 144 rows x
        // 144 bytes (row stride 36 words: conflict-free ds_read_b128) in the space of `ph` and `sp`, which the phase does not need
        // before its end; one barrier per k-step, and the global loads run SD steps ahead in registers (7 per step).
        constexpr int SD = 4, SROW = 72;       // steps in flight; staging row stride in halves
        static_assert(144 * SROW * 2 <= (int)sizeof(ph) && 144 * SROW * 2 <= (int)sizeof(sp), "staging buffers");
        _Float16* const stg[2] = {&ph[0][0], reinterpret_cast<_Float16*>(&sp[0][0][0])};
        f32x4 am[ND + 1];
#pragma unroll
        for (int d = 0; d <= ND; ++d) am[d] = f32x4{0.f, 0.f, 0.f, 0.f};
        // chunk c = tid + 256 i of a k-step: row c / 8 (0..127: key rows, 128..143: Q tile 4), 16-byte column c % 8
        const int crow = tid >> 3, ccol = (tid & 7) * 8;
        const _Float16* const kc = kb + crow * LDQKH + ccol;                                  // + 32 i rows
        const _Float16* const qc = qb + min(t0 + 64 + (crow & 15), tend - 1) * LDQKH + ccol;  // i = 4: threads 0..127
        const _Float16* const qw = qb + min(t0 + wave * 16 + l15, tend - 1) * LDQKH + g4 * 16;
        f16x8 gk[SD][5];
        Frag gq[SD];
        auto gload = [&](int s, f16x8 (&dk)[5], Frag& dq) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dk[i] = cp::ld_h8<POL, cp::ATT_K_LD>(kc + (i * 32 - (i == 3 ? kback : 0)) * LDQKH + s * 64);
            if (wave < 2) dk[4] = cp::ld_h8<POL, cp::ATT_Q_LD>(qc + s * 64);      // wave-uniform
            dq.h = cp::ld_h8<POL, cp::ATT_Q_LD>(qw + s * 64);
            dq.l = cp::ld_h8<POL, cp::ATT_Q_LD>(qw + s * 64 + 8);
        };
        auto lstore = [&](_Float16* dst, const f16x8 (&sk)[5]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<f16x8*>(dst + (crow + 32 * i) * SROW + ccol) = sk[i];
            if (wave < 2) *reinterpret_cast<f16x8*>(dst + (crow + 128) * SROW + ccol) = sk[4];
        };
        auto frag = [&](const _Float16* src, int tile) {
            const _Float16* p = src + (tile * 16 + l15) * SROW + g4 * 16;
            return Frag{*reinterpret_cast<const f16x8*>(p), *reinterpret_cast<const f16x8*>(p + 8)};
        };
        auto mma3 = [&](f32x4& acc, const Frag& a, const Frag& b) {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h, b.h, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h, b.l, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.l, b.h, acc, 0, 0, 0);
        };
#pragma unroll
        for (int s = 0; s < SD; ++s) gload(s, gk[s], gq[s]);
        lstore(stg[0], gk[0]);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < AT_KSTEPS; ++s) {
            // step s + 1 into the buffer that step s - 1 was read from (the barrier that closed step s - 1 is behind us)
            if (s + 1 < AT_KSTEPS) lstore(stg[(s + 1) & 1], gk[(s + 1) % SD]);
            const _Float16* src = stg[s & 1];
            const Frag q4 = frag(src, 8);
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const Frag kf = frag(src, wave + d);
                mma3(am[d], gq[s % SD], kf);
                if (d == ND - 1) mma3(am[ND], q4, kf);
            }
            if (s + SD < AT_KSTEPS) gload(s + SD, gk[s % SD], gq[s % SD]);
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int d = 0; d < ND; ++d) sp[0][wave * 16 + g4 * 4 + r][d * 16 + l15] = am[d][r];
            if (64 + g4 * 4 + r < TQ) sp[0][64 + g4 * 4 + r][wave * 16 + l15] = am[ND][r];
        }
    } else {      // feature k-steps s = wave, wave+4, ... of 19: every wave carries every product, partial sums through `sp`
        f32x4 am[MQ][ND];
#pragma unroll
        for (int mq = 0; mq < MQ; ++mq)
#pragma unroll
            for (int d = 0; d < ND; ++d) am[mq][d] = f32x4{0.f, 0.f, 0.f, 0.f};
        int qoff[MQ], koff[NKT];
#pragma unroll
        for (int mq = 0; mq < MQ; ++mq) qoff[mq] = min(t0 + mq * 16 + l15, tend - 1) * LDQKH + g4 * 16;
#pragma unroll
        for (int nt = 0; nt < NKT; ++nt) koff[nt] = xrow(nt * 16 + l15) * LDQKH + g4 * 16;
        constexpr int NIT = (AT_KSTEPS + 3) / 4;       // 5 (wave 3 runs 4)
        Frag fq[2][MQ], fk[2][NKT];
        auto fetch = [&](int it, Frag (&dq)[MQ], Frag (&dk)[NKT]) {
            const int s = min(wave + 4 * it, AT_KSTEPS - 1);
#pragma unroll
            for (int mq = 0; mq < MQ; ++mq) {
                const _Float16* p = qb + qoff[mq] + s * 64;
                dq[mq].h = cp::ld_h8<POL, cp::ATT_Q_LD>(p);
                dq[mq].l = cp::ld_h8<POL, cp::ATT_Q_LD>(p + 8);
            }
#pragma unroll
            for (int nt = 0; nt < NKT; ++nt) {
                const _Float16* p = kb + koff[nt] + s * 64;
                dk[nt].h = cp::ld_h8<POL, cp::ATT_K_LD>(p);
                dk[nt].l = cp::ld_h8<POL, cp::ATT_K_LD>(p + 8);
            }
        };
        auto mma = [&](const Frag (&sq)[MQ], const Frag (&sk)[NKT]) {
#pragma unroll
            for (int mq = 0; mq < MQ; ++mq)
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    if (mq + d >= NKT) continue;       // compile-time: the last tile of a 40-frame workgroup sees 4 key tiles
                    const Frag& kf = sk[mq + d];
                    am[mq][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sq[mq].h, kf.h, am[mq][d], 0, 0, 0);
                    am[mq][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sq[mq].h, kf.l, am[mq][d], 0, 0, 0);
                    am[mq][d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sq[mq].l, kf.h, am[mq][d], 0, 0, 0);
                }
        };
        fetch(0, fq[0], fk[0]);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (it + 1 < NIT) fetch(it + 1, fq[(it + 1) & 1], fk[(it + 1) & 1]);
            if (wave + 4 * it < AT_KSTEPS) mma(fq[it & 1], fk[it & 1]);       // wave-uniform
        }
#pragma unroll
        for (int mq = 0; mq < MQ; ++mq)
#pragma unroll
            for (int d = 0; d < ND; ++d)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = mq * 16 + g4 * 4 + r;
                    if (TQ == 16 * MQ || row < TQ) sp[wave][row][d * 16 + l15] = am[mq][d][r];
                }
    }
    AT_STAMP(1);
    __syncthreads();
    AT_STAMP(2);

    // ---- softmax over the 50 slots n = i .. i+49 of query i; 16 threads per query, P as fp16 hi/lo rows
    {
        const float scale = 1.0f / sqrtf((float)DQK);
        constexpr int NU = PKS * 2;               // 6 / 8 column slots of 16 per thread (96 / 128 key columns)
#pragma unroll
        for (int pass = 0; pass < MQ; ++pass) {
            const int ir = pass * 16 + (tid >> 4), sub = tid & 15;
            const int i = min(ir, TQ - 1);         // rows past TQ (40-frame tiles) recompute row TQ-1 and store nothing
            float sv[NU];
            float mx = -3.0e38f;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int n = sub + 16 * u, j = n - i;
                const int c = n - pass * 16;           // band-relative column; in [0, 65) whenever j is in the window
                float s = -3.0e38f;
                if (j >= 0 && j < WIN) {
                    if constexpr (OWN) s = sp[0][i][c] * scale;
                    else s = (sp[0][i][c] + sp[1][i][c] + sp[2][i][c] + sp[3][i][c]) * scale;
                }
                sv[u] = s;
                mx = fmaxf(mx, s);
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            float sum = 0.f;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int j = sub + 16 * u - i;
                sv[u] = (j >= 0 && j < WIN) ? __expf(sv[u] - mx) : 0.f;
                sum += sv[u];
            }
            sum = group16_sum(sum);
            const float inv = 1.0f / sum;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const float p = sv[u] * inv;           // exactly 0 outside the band
                _Float16 h, l;
                split_hl(p, h, l);
                if (TQ == 16 * MQ || ir < TQ) {
                    ph[ir][sub + 16 * u] = h;
                    pl[ir][sub + 16 * u] = l;
                }
            }
        }
    }
    AT_STAMP(3);
    __syncthreads();
    AT_STAMP(4);

    // ---- O = P . Vx ; each wave takes column groups of 64 (4 MFMA column tiles interleaved so a lane loads one
    //      [hi 4 | lo 4] quad of a V row per key); the head merge is fused into the store
    {
        const int b = bh / NH, hd = bh % NH;
        // gridDim.y workgroups share one (batch, head, tile): each recomputes the (cheap) scores and takes every
        // gridDim.y-th round of column groups — a chunk of ONE frame would otherwise keep 4 of the 256 CUs busy
        const int part = blockIdx.y, nsplit = gridDim.y;
        // key row of (step ks, slot j) for this lane: 32 ks + 8 g4 + j; rows >= NKEYS are never needed (P = 0 there)
        auto qcol = [&](int cg) { return min(min(cg, AT_CG - 1) * 16 + l15, DV / 4 - 1) * 8; };   // quad offset in halves
        // Register ring over the flattened (column group, key step) sequence of this wave: step s uses slot s % RING
        // and, before its MFMAs, refills the slot of step s-1 with the rows of step s+RING-1.
        VQuad ring[RING][8];
        // Every load is UNCONDITIONAL (round 5): a lane whose row is >= NKEYS (last key step only: P is exactly 0 there, and
        // 0 * finite = 0) reads the row the lanes one quarter below load in the SAME instruction (same cache lines, no extra
        // traffic) instead of skipping the load.  Behind the per-lane `row < NKEYS` branches of rounds 1-4 hipcc lost count
        // of the loads in flight and drained them all (s_waitcnt vmcnt(0) right behind the refill, once per column group:
        // the whole L2 latency exposed); in straight-line code the waits are exact and the refill stays in flight.
        auto fill = [&](int slot, int ks, int qc) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int r = 32 * ks + 8 * g4 + j;
                if (32 * ks + 31 >= NKEYS) {                   // (compile-time per unrolled step: the last key step only)
                    r = r >= NKEYS ? r - 8 : r;
                    r = r >= NKEYS ? NKEYS - 1 : r;
                }
                // OWN: the row is a scalar base and the lane's part one 32-bit offset per column group (as 64-bit lane addresses
                // the 32 rows of a column group were hoisted out of the loop: 64 registers, and the kernel spilled)
                const _Float16* p = OWN ? (vb + (32 * ks + j - (ks == 3 ? kback : 0)) * LDVH) + (unsigned)(8 * g4 * LDVH + qc) : vb + xrow(r) * LDVH + qc;
                VQuad v;
                if constexpr (cp::nt(POL, cp::ATT_V_LD)) {        // one 16-byte access, as the plain pair of 8-byte ones is merged into
                    const f16x8 hl = cp::ld_h8<POL, cp::ATT_V_LD>(p);
                    v.h = f16x4{hl[0], hl[1], hl[2], hl[3]};
                    v.l = f16x4{hl[4], hl[5], hl[6], hl[7]};
                } else {
                    v.h = *reinterpret_cast<const f16x4*>(p);
                    v.l = *reinterpret_cast<const f16x4*>(p + 4);
                }
                ring[slot][j] = v;
            }
        };
#pragma unroll
        for (int s = 0; s < RING - 1; ++s) fill(s % RING, s % PKS, qcol(wave + 4 * (part + nsplit * (s / PKS))));
        f32x4 am[MQ][4];
        // fully unrolled (7 column groups for wave 0, 6 for the others): exact vmcnt waits instead of a drain of the
        // ring at every loop back-edge
        constexpr int NSTEP = ((AT_CG + 3) / 4) * PKS;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            const int ks = s % PKS, cg = wave + 4 * (part + nsplit * (s / PKS));
            if (cg >= AT_CG) break;                    // wave-uniform
            if (ks == 0) {
#pragma unroll
                for (int mq = 0; mq < MQ; ++mq)
#pragma unroll
                    for (int c = 0; c < 4; ++c) am[mq][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            {
                const int sn = s + RING - 1, cgn = wave + 4 * (part + nsplit * (sn / PKS));
                fill(sn % RING, sn % PKS, qcol(cgn));      // (no `cgn < AT_CG` branch: qcol clamps, the wave's last refill is a re-read)
                // the refill goes out HERE: without the fence hipcc sinks the loads below this step's MFMAs, next to their
                // first use (it saves the ring's registers that way) and every step waits out a full V-row load
                __builtin_amdgcn_sched_barrier(0);
            }
            // regroup: column tile c takes element c of the 8 key rows -> one f16x8 B operand (hi and lo)
            f16x8 bh8[4], bl8[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    bh8[c][j] = ring[s % RING][j].h[c];
                    bl8[c][j] = ring[s % RING][j].l[c];
                }
#pragma unroll
            for (int mq = 0; mq < MQ; ++mq) {
                const f16x8 pa = *reinterpret_cast<const f16x8*>(&ph[mq * 16 + l15][ks * 32 + g4 * 8]);
                const f16x8 pb = *reinterpret_cast<const f16x8*>(&pl[mq * 16 + l15][ks * 32 + g4 * 8]);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    am[mq][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, bh8[c], am[mq][c], 0, 0, 0);
                    am[mq][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, bl8[c], am[mq][c], 0, 0, 0);
                    am[mq][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pb, bh8[c], am[mq][c], 0, 0, 0);
                }
            }
            const int col = cg * 64 + l15 * 4;
            if (ks == PKS - 1 && col < DV) {
#pragma unroll
                for (int mq = 0; mq < MQ; ++mq)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int t = t0 + mq * 16 + g4 * 4 + r;
                        float* dst;
                        // (OWN, 20 rows per lane: the row of (mq, r) and the column group are a scalar base, the lane's part one
                        // 32-bit offset for the whole kernel)
                        if constexpr (OWN) dst = (merged + (((long)b * T + t0 + mq * 16 + r) * NH + hd) * DV + cg * 64) + (unsigned)(g4 * 4 * (NH * DV) + l15 * 4);
                        else dst = &merged[(((long)b * T + t) * NH + hd) * DV + col];
                        if (t < tend && (TQ == 16 * MQ || mq * 16 + g4 * 4 + r < TQ))      // head-major slab [b][t][hd][f][v]: one head's frame is 6208 contiguous bytes
                            cp::st_f4<POL, cp::ATT_MERGED_ST>(dst, make_float4(am[mq][0][r], am[mq][1][r], am[mq][2][r], am[mq][3][r]));
                    }
            }
        }
    }
    AT_STAMP(5);
}

// ------------------------------------------------------------------------------------------------------
// Streaming state <-> ring rows: the reference carries K_buf [4B][49][582] / V_buf [4B][49][1552] as fp32
// (tfgridnet_causal.py:553-562); the history rows of kx / vx hold the same numbers as split fp16 pairs.
//   pack:   rows 0..48 of kx / vx   <- K_buf / V_buf
//   unpack: K_buf / V_buf           <- rows T..T+48 of kx / vx  (hi + lo: the value the attention kernel used)
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ring_pack(const float* __restrict__ kbuf, const float* __restrict__ vbuf,
                                                   _Float16* __restrict__ kx, _Float16* __restrict__ vx, long tkp, int BH) {
    const long nk = (long)BH * HIST * QKB, nv = (long)BH * HIST * (DV / 4);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nk + nv; i += (long)gridDim.x * 256) {
        if (i < nk) {                                   // one 8-feature block of a K row
            const long row = i / QKB;
            const int blk = (int)(i % QKB);
            const long bh = row / HIST, r = row % HIST;
            f16x8 h8, l8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int f = blk * 8 + e;
                const float v = f < DQK ? kbuf[row * DQK + f] : 0.f;
                _Float16 h, l;
                split_hl(v, h, l);
                h8[e] = h;
                l8[e] = l;
            }
            _Float16* d = kx + (bh * tkp + r) * LDQKH + blk * 16;
            *reinterpret_cast<f16x8*>(d) = h8;
            *reinterpret_cast<f16x8*>(d + 8) = l8;
        } else {                                        // one 4-column quad of a V row
            const long k = i - nk;
            const long row = k / (DV / 4);
            const int qd = (int)(k % (DV / 4));
            const long bh = row / HIST, r = row % HIST;
            const float4 v4 = *reinterpret_cast<const float4*>(&vbuf[row * DV + qd * 4]);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                _Float16 h, l;
                split_hl(v[e], h, l);
                o[e] = h;
                o[4 + e] = l;
            }
            *reinterpret_cast<f16x8*>(vx + (bh * tkp + r) * LDVH + qd * 8) = o;
        }
    }
}

__global__ void __launch_bounds__(256) k_ring_unpack(const _Float16* __restrict__ kx, const _Float16* __restrict__ vx,
                                                     float* __restrict__ kbuf, float* __restrict__ vbuf, long tkp, int T,
                                                     int BH) {
    const long nk = (long)BH * HIST * QKB, nv = (long)BH * HIST * (DV / 4);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nk + nv; i += (long)gridDim.x * 256) {
        if (i < nk) {
            const long row = i / QKB;
            const int blk = (int)(i % QKB);
            const long bh = row / HIST, r = row % HIST;
            const _Float16* s = kx + (bh * tkp + T + r) * LDQKH + blk * 16;
            const f16x8 h8 = *reinterpret_cast<const f16x8*>(s), l8 = *reinterpret_cast<const f16x8*>(s + 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int f = blk * 8 + e;
                if (f < DQK) kbuf[row * DQK + f] = (float)h8[e] + (float)l8[e];
            }
        } else {
            const long k = i - nk;
            const long row = k / (DV / 4);
            const int qd = (int)(k % (DV / 4));
            const long bh = row / HIST, r = row % HIST;
            const f16x8 o = *reinterpret_cast<const f16x8*>(vx + (bh * tkp + T + r) * LDVH + qd * 8);
            *reinterpret_cast<float4*>(&vbuf[row * DV + qd * 4]) =
                make_float4((float)o[0] + (float)o[4], (float)o[1] + (float)o[5], (float)o[2] + (float)o[6],
                            (float)o[3] + (float)o[7]);
        }
    }
}

}  // namespace lh
#if defined(LH_PROBE_TRACE)
extern "C" int lh_probe_attn_trace_read(unsigned long long* host_dst) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(lh::lh_attn_trace_buf), sizeof(lh::lh_attn_trace_buf)) == hipSuccess ? 0 : 1;
}
#endif
namespace lh {
static int g_attn_mq = 0;              // lh_set_tuning key 4: 0 = automatic, 1 / 2 = query tiles of 16 frames per workgroup,
                                       // 3 = 40 frames in three tiles, 5 = 79 frames in five (the value is the number of MFMA row
                                       // tiles but for 3's short third tile; four tiles have no kernel and 4 stays refused)
int attn_set_mq(int v) {
    if (v < 0 || v > 5 || v == 4) return LH_ERR_ARG;
    g_attn_mq = v;
    return LH_OK;
}

// Tile form of a launch, from the WHOLE clip's shape: one 16-frame tile when the clip is that short (streaming: T = 1); two
// tiles share every K / V row they load (25 instead of 44 KB of L2 traffic per query; 0.36 against 0.43 ms at B = 32); 40
// frames in three tiles once the launch has more workgroups than the 512 resident ones (12 % fewer K / V rows per query,
// and at B = 32, T = 625 exactly four rounds of workgroups instead of five: 0.343 against 0.356 ms) — below that a launch
// is latency-bound and the shorter workgroup wins; 79 frames in five tiles (128 key rows = four whole P.V steps, 1.62 K / V
// rows per query against 2.23) once even those fill the 512 resident slots twice.
static int attn_form(int B, int Tshape) {
    const int bh8 = (B * NH + 7) / 8 * 8;
    int mq = g_attn_mq;
    if (Tshape <= 16) mq = 1;
    else if (mq == 0) mq = (long)bh8 * ((Tshape + 78) / 79) >= 1024 ? 5 : (long)bh8 * ((Tshape + 31) / 32) > 512 ? 3 : 2;
    return mq;
}
static int attn_tq(int mq) { return mq == 5 ? 79 : mq == 3 ? 40 : 16 * mq; }

}  // namespace lh

extern "C" int lh_attn_tile_frames(int B, int T, int* frames) {
    if (!frames || B <= 0 || T <= 0) return LH_ERR_ARG;
    *frames = lh::attn_tq(lh::attn_form(B, T));
    return LH_OK;
}

extern "C" int lh_local_attn_win(const void* q, const void* kx, const void* vx, float* merged, int B, int T, int t0, int Tc,
                                 lh_stream_t stream) {
    using namespace lh;
    if (!q || !kx || !vx || !merged || B <= 0 || T <= 0 || t0 < 0 || Tc <= 0 || t0 + Tc > T) return LH_ERR_ARG;
    const int Tfull = T;
    // tile shape from the WHOLE clip (a window then cuts the time axis into the same tiles as the whole-clip launch when t0
    // is a multiple of the tile length: bit-identical outputs); tile count and bounds from the window
    const int Tshape = T;
    T = Tc;
    const int BH = B * NH;
    const int bh8 = (BH + 7) / 8 * 8;
    // Query frames per workgroup: attn_form.  The V ring is two-deep: a three-deep one (228 registers since the
    // single-accumulator split) measured 3 % slower.
    const int mq = attn_form(B, Tshape);
    const int tq = attn_tq(mq);
    const int ntt = (T + tq - 1) / tq;
    // latency-bound launches (a handful of workgroups): split the V columns of a tile over 7 workgroups
    const dim3 grid(bh8 * ntt, bh8 * ntt <= 64 ? 7 : 1);
    const _Float16 *qh = (const _Float16*)q, *kh = (const _Float16*)kx, *vh = (const _Float16*)vx;
    // cache policy by the footprint of the launch's largest stream (merged; V is as large): lh_cachepol.h.  The one-tile
    // shape is the streaming chunk's and stays plain.
    const bool pol = cp::nt_on((long)B * Tc * NF * C * 4);
    if (mq == 1)
        hipLaunchKernelGGL((k_local_attn<1, 3, 16, false, 0>), grid, dim3(256), 0, (hipStream_t)stream, qh, kh, vh, merged, BH, Tfull, ntt, t0, t0 + Tc, NoRing{});
    else if (mq == 5 && pol)
        hipLaunchKernelGGL((k_local_attn<5, 2, 79, false, 1>), grid, dim3(256), 0, (hipStream_t)stream, qh, kh, vh, merged, BH, Tfull, ntt, t0, t0 + Tc, NoRing{});
    else if (mq == 5)
        hipLaunchKernelGGL((k_local_attn<5, 2, 79, false, 0>), grid, dim3(256), 0, (hipStream_t)stream, qh, kh, vh, merged, BH, Tfull, ntt, t0, t0 + Tc, NoRing{});
    else if (mq == 3 && pol)
        hipLaunchKernelGGL((k_local_attn<3, 2, 40, false, 1>), grid, dim3(256), 0, (hipStream_t)stream, qh, kh, vh, merged, BH, Tfull, ntt, t0, t0 + Tc, NoRing{});
    else if (mq == 3)
        hipLaunchKernelGGL((k_local_attn<3, 2, 40, false, 0>), grid, dim3(256), 0, (hipStream_t)stream, qh, kh, vh, merged, BH, Tfull, ntt, t0, t0 + Tc, NoRing{});
    else if (pol)
        hipLaunchKernelGGL((k_local_attn<2, 2, 32, false, 1>), grid, dim3(256), 0, (hipStream_t)stream, qh, kh, vh, merged, BH, Tfull, ntt, t0, t0 + Tc, NoRing{});
    else
        hipLaunchKernelGGL((k_local_attn<2, 2, 32, false, 0>), grid, dim3(256), 0, (hipStream_t)stream, qh, kh, vh, merged, BH, Tfull, ntt, t0, t0 + Tc, NoRing{});
    return check_launch();
}

extern "C" int lh_local_attn(const void* q, const void* kx, const void* vx, float* merged, int B, int T,
                             lh_stream_t stream) {
    return lh_local_attn_win(q, kx, vx, merged, B, T, 0, T, stream);
}

// lh_local_attn for a streaming chunk of T <= 16 frames on the persistent ring (include/lookonce_hip.h, "frames per chunk"):
// the launch geometry of the one-tile form above, the ring map instantiation
extern "C" int lh_local_attn_ring(const void* q, const void* kx, const void* vx, float* merged, const int* ring_pos, int B, int T,
                                  lh_stream_t stream) {
    using namespace lh;
    if (!q || !kx || !vx || !merged || !ring_pos || B <= 0 || T < 1 || T > 16) return LH_ERR_ARG;
    const int BH = B * NH;
    const int bh8 = (BH + 7) / 8 * 8;
    const dim3 grid(bh8, bh8 <= 64 ? 7 : 1);      // ntt = 1
    hipLaunchKernelGGL((k_local_attn<1, 3, 16, true, 0>), grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)q,
                       (const _Float16*)kx, (const _Float16*)vx, merged, BH, T, 1, 0, T, ring_pos);
    return check_launch();
}

extern "C" int lh_ring_pack(const float* k_buf, const float* v_buf, void* kx, void* vx, int B, int T,
                            lh_stream_t stream) {
    using namespace lh;
    if (!k_buf || !v_buf || !kx || !vx || B <= 0 || T <= 0) return LH_ERR_ARG;
    const int BH = B * NH;
    const long n = (long)BH * HIST * (QKB + DV / 4);
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_ring_pack, dim3(grid), dim3(256), 0, (hipStream_t)stream, k_buf, v_buf, (_Float16*)kx,
                       (_Float16*)vx, (long)T + HIST + KV_PAD, BH);
    return check_launch();
}

namespace lh {
__global__ void k_ring_advance(int* pos, int modulo) {
    const int p = *pos + 1;
    *pos = p >= modulo ? p - modulo : p;
}
}  // namespace lh

extern "C" int lh_ring_advance(int* ring_pos, int modulo, lh_stream_t stream) {
    if (!ring_pos || modulo < 1 || modulo > (1 << 30)) return LH_ERR_ARG;
    hipLaunchKernelGGL(lh::k_ring_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, ring_pos, modulo);
    return lh::check_launch();
}

namespace lh {
__global__ void k_ring_advance_by(int* pos, int step, int modulo) {
    *pos = (int)(((unsigned)*pos + (unsigned)step) % (unsigned)modulo);
}
}  // namespace lh

extern "C" int lh_ring_advance_by(int* ring_pos, int step, int modulo, lh_stream_t stream) {
    if (!ring_pos || step < 1 || step > modulo || modulo > (1 << 30)) return LH_ERR_ARG;
    hipLaunchKernelGGL(lh::k_ring_advance_by, dim3(1), dim3(1), 0, (hipStream_t)stream, ring_pos, step, modulo);
    return lh::check_launch();
}

namespace lh {
// one thread per row: the only writer of a paced session host's per-row ring positions (lh_stream.hip, "paced sessions")
__global__ void k_ring_advance_rows(int* pos, const int* __restrict__ write_pos, int modulo, int n_rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int w = write_pos[r];
    if (w < 0) return;                             // the row consumed no chunk
    const int p = (int)((unsigned)w % (unsigned)modulo) + 1;
    pos[r] = p >= modulo ? 0 : p;
}
}  // namespace lh

extern "C" int lh_ring_advance_rows(int* pos, const int* write_pos, int modulo, int n_rows, lh_stream_t stream) {
    if (!pos || !write_pos || pos == write_pos || modulo < 1 || modulo > (1 << 30) || n_rows < 1) return LH_ERR_ARG;
    hipLaunchKernelGGL(lh::k_ring_advance_rows, dim3((n_rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, pos, write_pos,
                       modulo, n_rows);
    return lh::check_launch();
}

extern "C" int lh_ring_unpack(const void* kx, const void* vx, float* k_buf, float* v_buf, int B, int T,
                              lh_stream_t stream) {
    using namespace lh;
    if (!k_buf || !v_buf || !kx || !vx || B <= 0 || T <= 0) return LH_ERR_ARG;
    const int BH = B * NH;
    const long n = (long)BH * HIST * (QKB + DV / 4);
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_ring_unpack, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const _Float16*)kx,
                       (const _Float16*)vx, k_buf, v_buf, (long)T + HIST + KV_PAD, T, BH);
    return check_launch();
}
