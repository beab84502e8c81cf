// Cache policy per activation stream (DESIGN.md §11 "cache policy", profiles/cache_policy_ab.txt).
// At large batches every stream between two kernels of a block (x, Q / K / V, merged: 186..497 MB at B = 32) is far larger
// than L2 (4 MiB per XCD) and the Infinity Cache (256 MiB): a line is written once, read once or twice a launch later, and
// under the default policy still takes cache ways on the way through.  The helpers below are the 16-byte (and the two
// 8-byte) accesses the kernels already make, with the non-temporal replacement hint (`nt` on global_load / global_store:
// a hint about REPLACEMENT only, never scope or coherence) switched per stream at compile time:
//   POL = 0  the plain access, today's code exactly;
//   POL > 0  non-temporal when the stream's bit is set in NT_MASK.
// Instruction count and order do not change and hipcc counts `nt` loads in vmcnt like plain ones, so the hand-ordered
// kernels keep their waits.  The host picks POL per launch from the launch's footprint (nt_on below): small batches and
// streaming chunks fit in cache, the next kernel's hit is the point there, and they run POL 0.
#pragma once
#include "lh_common.h"

namespace lh {
namespace cp {

enum Stream : unsigned {
    QKV_X_LD = 0,        // k_qkv_proj_ln: the frame of x
    QKV_ST = 1,          //                Q, K and V rows
    ATT_Q_LD = 2,        // k_local_attn:  Q fragments (read by one workgroup only)
    ATT_K_LD = 3,        //                K fragments (49 of a tile's rows are re-read by its neighbour)
    ATT_V_LD = 4,        //                V quads (the same)
    ATT_MERGED_ST = 5,   //                merged
    PROJ_MERGED_LD = 6,  // k_proj_ln_res: merged
    PROJ_RES_LD = 7,     //                the residual x
    PROJ_ST = 8,         //                x (plain, FAN) or the tap products (TAPS)
    N_STREAMS = 9
};

// The committed table (profiles/cache_policy_ab.txt, B = 32, each stage timed behind its predecessor in a forward's order):
//   kept   QKV_X_LD + QKV_ST           the attention launch behind them -15 .. -17 us of 325 (the pair costs k_qkv_proj_ln itself
//                                      nothing; the stores alone cost it +37 us, the load alone costs attention +13)
//          ATT_MERGED_ST + PROJ_MERGED_LD   k_proj_ln_res behind them -37 us of 281 (each alone -15 .. -18), attention +2 .. +4
//   lost   ATT_Q_LD +12 .. +16 us, ATT_K_LD +45, ATT_V_LD +92 (re-read by the neighbouring tile: as expected)
//          PROJ_ST takes back 15 us of the projection's gain; PROJ_RES_LD: -6 us there, within the scatter of the chain
// The rows of the two recurrences, the front end's store and the back end's load were tried the same way (a lab patch with
// the same helpers): every one within the run's scatter, so those kernels stay untouched.
// Lab builds override the table: python -m lookoncetohear_amd.build --variant NAME -DLH_NT_MASK=0x...
#ifndef LH_NT_MASK
#define LH_NT_MASK 0x63u
#endif
constexpr unsigned NT_MASK = LH_NT_MASK;
static_assert(NT_MASK < (1u << N_STREAMS), "LH_NT_MASK names a stream that does not exist");

constexpr bool nt(int pol, unsigned s) { return pol != 0 && ((NT_MASK >> s) & 1u) != 0; }

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

template <int POL, unsigned S>
__device__ __forceinline__ float4 ld_f4(const void* p) {
    if constexpr (nt(POL, S)) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
        return make_float4(v[0], v[1], v[2], v[3]);
    } else {
        return *reinterpret_cast<const float4*>(p);
    }
}
template <int POL, unsigned S>
__device__ __forceinline__ void st_f4(void* p, const float4& v) {
    if constexpr (nt(POL, S)) {
        const f32x4 q = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(q, reinterpret_cast<f32x4*>(p));
    } else {
        *reinterpret_cast<float4*>(p) = v;
    }
}
template <int POL, unsigned S>
__device__ __forceinline__ h8 ld_h8(const _Float16* p) {
    if constexpr (nt(POL, S)) return __builtin_nontemporal_load(reinterpret_cast<const h8*>(p));
    else return *reinterpret_cast<const h8*>(p);
}
template <int POL, unsigned S>
__device__ __forceinline__ void st_h8(_Float16* p, const h8& v) {
    if constexpr (nt(POL, S)) __builtin_nontemporal_store(v, reinterpret_cast<h8*>(p));
    else *reinterpret_cast<h8*>(p) = v;
}
template <int POL, unsigned S>
__device__ __forceinline__ void st_h4(_Float16* p, const h4& v) {
    if constexpr (nt(POL, S)) __builtin_nontemporal_store(v, reinterpret_cast<h4*>(p));
    else *reinterpret_cast<h4*>(p) = v;
}

// lh_set_tuning(19, v): 0 = never, 1 = by footprint (default), 2 = always.  One switch for the whole library (lh_lstm.hip).
int nt_mode();
// Footprint from which a launch runs its POL > 0 instantiation.  NOT a measured optimum: in the sweep of
// profiles/cache_policy_ab.txt (B = 4 .. 32, policy forced off / on) forced-on is never slower, but only B = 32 (474 MiB per
// launch) gains more than the run's scatter and the next size below, B = 24 in two windows, is 178 MiB per launch — the
// threshold is only bracketed, (178, 474] MiB.  256 MiB is the point inside the bracket with a reason of its own: the
// Infinity Cache's size, from which no line of the stream survives to the next launch.  One-window launches between 256 and
// 474 MiB (batches 18 .. 31) select POL 1 on that reasoning, not on a measurement.
constexpr long NT_MIN_BYTES = 256L << 20;
static inline bool nt_on(long stream_bytes) {      // static: NT_MASK may differ between the sources of a lab build
    const int m = nt_mode();
    return NT_MASK != 0 && (m == 2 || (m == 1 && stream_bytes >= NT_MIN_BYTES));
}

}  // namespace cp
}  // namespace lh
