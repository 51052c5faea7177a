// decode_dev.hpp -- what the decoder's units (decoder.hip, decode_repack.hip, decode_small.hip,
// decode_few.hip, decode_layered.hip, decode_api.hip) share on the device side: the check modes, the debug sites, the
// accessors of the frame-innermost arrays, the RangeSel fields, the packed / templated degree
// bounds with their host-side dispatch.  Included by .hip files only.
#pragma once
#include "glibc_math.hpp"
#include "qamr_internal.hpp"
#include "strict_pack.hpp"

namespace qr {

enum CheckMode { kFirst = 0, kNormal = 1, kParityOnly = 2 };

// check sites (qr_debug_asserts reports the first failure's site)
enum DebugSite {
    kDbgLaneFrame = 1,     // lane_frame: a listed column outside the sweep's range
    kDbgNarrowFrame = 2,   // narrow sweeps: lane frame outside the repacked range's first 64 columns
    kDbgNarrowNode = 3,    // narrow sweeps: check id / CSR offset out of range
    kDbgRepackList = 4,    // k_repack_rows: list entry not ascending or outside [f0, f0 + w)
    kDbgRepackSlot = 5,    // gather_rows: a slot's byte offset outside its row group
    kDbgRepackFid = 6,     // hand-out / commit / k_repack_output: frame id outside [0, ld)
    kDbgCompact = 7,       // k_compact: list index outside the range
    kDbgResPost = 8,       // k_resident: posterior index outside [0, V)
    kDbgResMsg = 9,        // k_resident: LDS message index outside [0, C D)
    // 10, 11: the interpolation grid's (grid_interp.hpp GridDebugSite); 12..16: mi.hip (MiDebugSite)
    kDbgFewCheck = 17,     // few-frame check sweep: lane -> (class, check): check id or its degree
    kDbgFewPost = 18,      // few-frame check sweep: gathered posterior index outside [0, V)
    kDbgFewSlot = 19,      // few-frame sweeps: message slot outside [0, E)
    // 20..24: npstream.hip (NpDebugSite); 25, 26: lappr_info.hip (InfoDebugSite)
    kDbgLayCheck = 27,     // layered check sweep: check id outside [0, C) or not of the launch's degree
    kDbgLayVar = 28,       // layered check sweep: variable outside [0, V)
    kDbgLayEdge = 29,      // layered check sweep: edge (message row) outside [0, E)
    kDbgLayFrame = 30,     // layered check sweep: frame column outside [0, ld)
};

// Check-node arithmetic: the reference's box-plus bit for bit -- glibc exp/log restated
// (glibc_math.hpp, the box-plus part of its tables, 8 KiB, staged in LDS per workgroup; a few
// constants pinned in VGPRs, GlibcK) -- so every message, posterior and output LAPPR is
// identical to the reference's.  (Rounds 1-4 also carried two approximate arithmetics; they
// missed north_star's 1e-6 LAPPR bar at configs[3] and were removed.)

// Edge-message access: NT = non-temporal (streamed once per sweep; keeps the
// re-read posteriors resident in L2/MALL instead of the message stream).
template <bool NT>
__device__ __forceinline__ double ld_msg(const double *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT>
__device__ __forceinline__ void st_msg(double *p, double v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// Read-only graph data (CSR) at a wave-uniform index through the constant address space:
// the load becomes a scalar s_load instead of a vector load + v_readfirstlane (the
// compiler cannot prove the generic pointer is not written by the kernel's own stores).
template <typename T>
__device__ __forceinline__ T sld(const T *p) {
    return *(const __attribute__((address_space(4))) T *)p;
}

// Message / posterior access of the check sweep through a raw buffer resource built from
// the (wave-uniform) row pointer in scalar registers: the lane's byte offset goes in the
// instruction's VGPR offset, so an access costs no VALU (a flat/global access needs a
// 64-bit v_lshl_add per access here, the compiler hoists base + lane offset and adds the
// scalar row offset per access).
typedef unsigned int qr_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const double *rowp, int ld) {
    // word 3 = 0x00020000: DATA_FORMAT 32 (raw dword access), no swizzle; num_records = row bytes
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(rowp), (short)0, ld * 8, 0x00020000);
}

// Row `row` (wave-uniform) of a frame-innermost array: the row offset is computed in
// scalar registers; lanes add their byte offset f * sizeof(T).
template <typename T>
__device__ __forceinline__ T *row_ptr(T *base, int row, int ld) {
    return base + (size_t)(uint32_t)__builtin_amdgcn_readfirstlane(row) * (size_t)ld;
}
// Element at byte offset `boff` (32-bit, = f * sizeof(T)) of a wave-uniform row.
template <typename T>
__device__ __forceinline__ T *at_byte(T *rowp, uint32_t boff) {
    return (T *)((char *)rowp + boff);
}
// Load / store of the lane's double in a wave-uniform row (row pointer rowp, ld doubles).
template <bool NT>
__device__ __forceinline__ double ld_row(const double *rowp, uint32_t b8, int ld) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(row_rsrc(rowp, ld), b8, 0, NT ? 2 : 0));
}
template <bool NT>
__device__ __forceinline__ void st_row(double *rowp, uint32_t b8, int ld, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(qr_u32x2, v), row_rsrc(rowp, ld), b8, 0, NT ? 2 : 0);
}

// Block geometry shared by the check and variable sweeps: 256 threads = `ft`
// consecutive frames (ft = 64 << k, a multiple of the wavefront) x (256/ft)
// node lanes; every wave therefore covers 64 frames of ONE node, which makes
// the node index wave-uniform (readfirstlane -> scalar loads of the CSR).
struct Geom {
    int lft;  // log2(ft)
    int per;  // nodes per thread
};

// The state of one frame range of the two-stream schedule, in device memory (the workspace's
// count block), read by every launch of that range and written only by a repack's commit (k_repack_rows): whether
// the range has moved to the repack work set, its width there (its running frames occupy the
// first columns), how many repacks it went through, and which of the work set's two column sets
// (messages, LAPPRs, syndrome bits) holds it: a repack gathers the running columns of one set
// into the other, so no column is overwritten while another thread may still read it.
// kSelTransit: the range was repacked at its last decision point and the sweeps that follow it
// (its variable sweep, then its check sweeps) have not all run yet: their messages still live in
// the old column set, at the frames' old columns (the active-frame list, which the commit leaves
// as it is until the next status launch rebuilds it).
enum RangeSelField { kSelOn = 0, kSelW = 1, kSelRepacks = 2, kSelArrive = 3, kSelBuf = 4, kSelTransit = 5, kSelInts = 6 };

// The frame id of column f: f itself, or fid_w[f] once the range (RangeSel sel, or null) lives
// in the repack work set.
__device__ __forceinline__ const int32_t *range_fid(const int32_t *sel, const int32_t *fid_w) {
    return (sel && sld(sel + kSelOn)) ? fid_w : nullptr;
}

// The syndrome sign of a check's outputs (decoder.pyx:360-369: s * message, s = -1 when the
// syndrome bit is set): s * x with s = +-1 only flips x's sign bit (for NaN too, as the compiled
// multiply by the selected constant did), so it is one XOR of the high word with a per-check mask
// instead of the compiler's XOR + select per output.
__device__ __forceinline__ uint32_t sign_mask(uint8_t sb) { return sb ? 0x80000000u : 0u; }
__device__ __forceinline__ double apply_sign(double x, uint32_t smask) { return g_make(g_hi(x) ^ smask, g_lo(x)); }

// Degrees whose round loop the compiler still unrolls fully (above, the packed update's
// register arrays would be indexed dynamically, i.e. live in scratch): the unpacked strict
// update runs there.
constexpr int kPackMaxDeg = 10;
// The strict arithmetic's finite flag: when every input LAPPR of the batch's frames is below
// a bound 2^e (a device flag computed by the decode's first variable sweep), no inf or NaN can
// arise in any sweep: |c2v| <= max |v2c| (a box-plus never exceeds its smaller operand, to
// rounding) and |v2c| <= |L| + (dv - 1) max |c2v|, so X_t = max |post| + max |c2v| after
// sweep t obeys X_{t+1} <= |L| + (dv + 1) X_t and every value (box-plus arguments, twice
// that) stays below 2^e (dv + 1)^(max_it + 2), which e = 1000 - (max_it + 2) log2(dv_max + 1)
// keeps finite.  The check sweeps then run the packed update with the one-instruction clamp
// (strict_pack.hpp kClampFinite) instead of the NaN-preserving two-instruction one.
// LDS of the packed strict update: one buffer per wavefront of a block.
constexpr int kPackLdsDoubles = 4 * kPackWaveDoubles;
template <int D>
constexpr bool kPacked = D <= kPackMaxDeg;

// The templated check degrees are 2..kMaxTemplDeg; a class above takes the runtime-degree kernel
// (k_check_generic, decoder.hip).
constexpr int kMaxTemplDeg = 16;

// deg in LO..HI -> f(std::integral_constant<int, deg>{}), the degree as a compile-time constant;
// false (and no call) outside the range.  Host code: the launch sites of the kernels templated
// on the check degree (2..kMaxTemplDeg, or 2..kPackMaxDeg for those that run only the packed update).
template <int LO, int HI, class F>
inline bool dispatch_degree(int deg, F f) {
    return dispatch_int_seq<LO>(deg, f, std::make_integer_sequence<int, HI - LO + 1>{});
}

}  // namespace qr
