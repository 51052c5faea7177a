// decoder.hip -- batched flooding sum-product LDPC syndrome decoder for gfx950.
//
// Reference: qamreconciliation/decoder.pyx (Decoder, _decode :391-436).
//
// Layout (HBM, frame-innermost): every per-edge / per-node quantity of frame f
// lives at row[node] * ld + f.  A wavefront = 64 consecutive frames of ONE
// check (or variable), so every message access is a contiguous 512-B run no
// matter how irregular the Tanner graph is; the graph itself (CSR) is
// wave-uniform and travels through the scalar cache.
//
// Only c2v[E][ld] and post[V][ld] are stored: the reference's v2c is
// post - c2v (decoder.pyx:295-297) and is recomputed in the check kernel,
// bit-identically.  All per-node arithmetic stays sequential in one lane in
// the reference's order (the F/B box-plus recursion is not associative).
//
// Schedule per iteration t (decoder.pyx:424-433):
//   k_check<t==1 ? First : Normal>   c2v(t) from post(t-1); also the parity of
//                                    post(t-1) (the check at the end of
//                                    iteration t-1, fused: it reads post anyway)
//   k_status(t-1)                    frames whose post(t-1) satisfies the
//                                    syndrome stop with (1, t-1)
//   k_var                            post(t) = lappr + sum c2v (ascending edge)
// plus an initial parity check of the input (decoder.pyx:400-405) and a final
// parity check after the last sweep.  Schedules (decode_batch_device): the two
// frame halves pipelined on two streams (run_split2, the DVB-S2 default; the
// running frames of a converging half are listed (k_compact) and, once they are
// few, moved to contiguous columns (column repack)); all frames in lock-step
// (run_flat); small codes with one launch per iteration (run_iter) or one launch
// per decode with a workgroup per frame and its messages in LDS (k_resident), both in
// decode_small.hip.  The column repack's kernels: decode_repack.hip.  A few frames on frame-major
// arrays (decode_frames_device, qr_decode_host): decode_few.hip.  The layered (serial-check)
// schedule, which reuses this unit's parity-only and init sweeps: decode_layered.hip.  The C entry points: decode_api.hip.
// This unit: the frame-parallel check and variable sweeps, the status and compaction kernels,
// the workspace layout and the launch layer of run_flat and run_split2.
#include "debug_check.hpp"
#include "decode_dev.hpp"
#include "decode_host.hpp"

namespace qr {

// One check sweep over the frame columns [f_off, f_off + ny*ft) of one degree class.
struct CheckArgs {
    const int32_t *checks;  // the class's check ids
    int64_t n_checks;
    const int32_t *chk_ptr, *chk_edge, *chk_var;
    const double *post;
    double *c2v;
    const uint8_t *synd;
    const uint8_t *active;
    uint8_t *unsat;
    int ld, f_off;
    Geom g;
    unsigned nbx;  // blocks along the check axis
    const GlibcTables *gglibc;
    double *fb;          // runtime-degree kernel: F scratch of the class (row fb_base)
    int64_t fb_base;
    const int32_t *alist;   // active-frame list (frame ids at alist[f_off + p]) or null
    const int32_t *acount;  // its length
    const int32_t *finite;  // strict arithmetic: 1 iff the batch's input LAPPRs are all finite (or null)
    // Short-tail grid (knob check_tail; k_check only): a 1-D grid whose first nmain blocks sweep
    // frame tiles 1.. with g.per checks per thread (block b: tile 1 + b / nbx, check block
    // b % nbx) and whose last blocks sweep frame tile 0 with per_t checks per thread -- the
    // workgroups dispatched last are the short ones, so the launch drains in ~a quarter of a
    // workgroup's time.  nmain = 0: the plain 2-D grid (nbx x frame tiles).
    unsigned nmain;
    int per_t;
    // Column repack (run_split2): sel -> the range's RangeSel, or null.  Once the device has
    // repacked the range (sel[kSelOn]) its posteriors live in the work set (post_w) and its
    // messages and syndrome bits in the work set's column set sel[kSelBuf] (c2v / c2v_alt,
    // synd_w[0] / synd_w[1]).
    const int32_t *sel;
    const double *post_w;
    const uint8_t *synd_w[2];
    double *c2v_alt;
    // set by select_range: 1 for the first sweep after a repack (its messages are read from the
    // old column set at the frames' old columns, c2v_rd / the list; everything else is read and
    // written in the new columns, see k_repack_rows)
    int transit;
    const double *c2v_rd;
};

// One variable sweep over the frame columns [f_off, f_off + ny*ft).
struct VarArgs {
    int64_t V;
    const int32_t *var_ptr, *var_edge;
    const double *lappr, *c2v;
    double *post;
    const uint8_t *active;
    int ld, f_off;
    Geom g;
    unsigned nbx;
    const int32_t *alist, *acount;  // as CheckArgs
    unsigned nby;  // frame tiles (grid-stride launches)
    int gs;        // 1: a capped 1-D grid walks the nbx x nby tiles (the paced sweeps of run_split2, knob var_pace)
    int boost;     // gs grid = boost x the paced width; as the live frame tiles drop to nby / k, min(k, boost) widths sweep
    // INIT sweep only: the strict arithmetic's finite flag (see kPackMaxDeg) is cleared when an
    // input LAPPR of a frame < fin_B is not below fin_bound in magnitude (null: not computed)
    int32_t *finite;
    double fin_bound;
    int fin_B;
    const int32_t *sel;  // as CheckArgs: the range's RangeSel or null; work-set LAPPRs / posteriors / messages
    const double *lappr_w[2];
    double *post_w;
    const double *c2v_alt;
    int transit;  // as CheckArgs (set by select_range); in transit c2v is the old column set
};

// Kernel-uniform: the arrays a range's launch reads once the device has repacked the range.
__device__ __forceinline__ void select_range(CheckArgs &a) {
    if (a.sel && sld(a.sel + kSelOn)) {
        const int b = sld(a.sel + kSelBuf);
        a.post = a.post_w;
        a.synd = b ? a.synd_w[1] : a.synd_w[0];  // (selects: a dynamic index would put a in scratch)
        double *const c0 = a.c2v, *const c1 = a.c2v_alt;
        a.c2v = b ? c1 : c0;
        a.transit = sld(a.sel + kSelTransit);
        a.c2v_rd = a.transit ? (b ? c0 : c1) : a.c2v;
    }
}
__device__ __forceinline__ void select_range(VarArgs &a) {
    if (a.sel && sld(a.sel + kSelOn)) {
        const int b = sld(a.sel + kSelBuf);
        a.lappr = b ? a.lappr_w[1] : a.lappr_w[0];
        a.post = a.post_w;
        a.transit = sld(a.sel + kSelTransit);
        if (a.transit ? !b : b) a.c2v = a.c2v_alt;  // transit: the old set
    }
}

// Active-frame compaction (converging operating points, decoder.pyx:431-433: frames stop
// at their own iteration).  Without a list a sweep's lane p of the frame range is frame
// f_off + p and stopped frames in a partly stopped wavefront run along; with one (built
// by k_compact after every status update) lane p is the p-th still-running frame, the
// range's tail blocks exit at once, and lanes past the count (live = false) repeat the
// last frame's reads but store nothing (a store would race with that frame's own lane,
// which may still read the old message).
__device__ __forceinline__ bool frames_block_live(const int32_t *acount, unsigned by, int lft) {
    return !acount || (int)(by << lft) < *acount;
}
__device__ __forceinline__ int lane_frame(const int32_t *alist, const int32_t *acount, int f_off, int p, bool &live) {
    live = true;
    if (!alist) return f_off + p;
    const int cnt = *acount;
    live = p < cnt;
    const int f = alist[f_off + (live ? p : cnt - 1)];
    QR_DCHECK(f >= f_off + (live ? p : cnt - 1), kDbgLaneFrame, f, f_off + p);  // ascending, in the range
    return f;
}


// The inputs of one check update: gathered posteriors, own c2v messages, syndrome bit.
// The gathered posteriors of check j+1 are issued before the arithmetic of check j on the
// unpacked paths (the packed strict update needs those registers: with the prefetch it runs
// at 3 waves/SIMD, 142 VGPRs); the own (streamed, row-contiguous) messages are loaded on use.
template <int D, int MODE, bool NT, bool TRANSIT = false>
struct CheckIn {
    double p[D], c[D];
    int base;
    uint8_t sb;
    __device__ __forceinline__ void load(const CheckArgs &a, int64_t ci, int f) {
        const int ld = a.ld;
        const uint32_t b8 = (uint32_t)f * 8u;
        const int cc = sld(a.checks + ci);
        base = sld(a.chk_ptr + cc);
        sb = *at_byte(row_ptr(a.synd, cc, ld), (uint32_t)f);
#pragma unroll
        for (int i = 0; i < D; ++i) p[i] = ld_row<false>(row_ptr(a.post, sld(a.chk_var + base + i), ld), b8, ld);
    }
    // fc: the frame's column of its messages (in transit its old column, c2v_rd the old set)
    __device__ __forceinline__ void load_c(const CheckArgs &a, int fc) {
        if (MODE != kNormal) return;
        const uint32_t b8 = (uint32_t)fc * 8u;
        const double *c2v = TRANSIT ? a.c2v_rd : a.c2v;
#pragma unroll
        for (int i = 0; i < D; ++i) c[i] = ld_row<NT>(row_ptr(c2v, sld(a.chk_edge + base + i), a.ld), b8, a.ld);
    }
};

// decoder.pyx:322-369 for one check (strict box-plus).
// Packed strict update (D <= kPackMaxDeg): strict_pack.hpp.  Otherwise
// F[i] = bp(F[i-1], m[i]); the backward values B[i] = bp(B[i+1], m[i]) are consumed as
// they are produced (out_i = bp(F[i-1], B[i+1])): the same operands as
// decoder.pyx:341-367, one live B instead of D.  Lane byte offset b8 = f * 8.
template <int D, bool NT, bool FIN = false>
__device__ __forceinline__ void check_exact(const CheckArgs &a, const double (&m)[D], int base, uint8_t sb, uint32_t b8,
                                            const GlibcTablesBP &tab, const GlibcK &K, double *hb = nullptr,
                                            bool live = true) {
    const int ld = a.ld;
    const double s = sb ? -1.0 : 1.0;
    if constexpr (kPacked<D>) {
        double out[D];
        double *wb = hb + (threadIdx.x >> 6) * kPackWaveDoubles;
        check_strict_packed<D, FIN ? kClampFinite : kClampFull>(m, out, wb, tab, K);
        const uint32_t smask = sign_mask(sb);
#pragma unroll
        for (int i = 0; i < D; ++i)
            if (live) st_row<NT>(row_ptr(a.c2v, sld(a.chk_edge + base + i), ld), b8, ld, apply_sign(out[i], smask));
        return;
    }
    double F[D - 1];
    F[0] = m[0];
#pragma unroll
    for (int i = 1; i < D - 1; ++i) F[i] = box_plus_strict(F[i - 1], m[i], tab, K);
    if (live) st_row<NT>(row_ptr(a.c2v, sld(a.chk_edge + base + D - 1), ld), b8, ld, s * F[D - 2]);
    double Bn = m[D - 1];
#pragma unroll
    for (int i = D - 2; i > 0; --i) {
        const double o = s * box_plus_strict(F[i - 1], Bn, tab, K);
        if (live) st_row<NT>(row_ptr(a.c2v, sld(a.chk_edge + base + i), ld), b8, ld, o);
        Bn = box_plus_strict(Bn, m[i], tab, K);
    }
    if (live) st_row<NT>(row_ptr(a.c2v, sld(a.chk_edge + base), ld), b8, ld, s * Bn);
}

// One lane = one (check, frame); each thread walks `per` checks of one degree class.
// decoder.pyx:322-369 (F/B recursion) with the parity test of decoder.pyx:235-257
// fused on the posteriors it gathers anyway.  Unpacked paths are software-pipelined: the
// posterior gathers of check j+1 are issued before the box-plus arithmetic of check j.
template <int D, int MODE, bool NT, bool FIN = false, bool TRANSIT = false>
__device__ __forceinline__ void check_block(const CheckArgs &a, unsigned bx, unsigned by, int per,
                                            const GlibcTablesBP &tab, double *hb) {
    const int ft = 1 << a.g.lft;
    const int nsub = 256 >> a.g.lft;
    bool live;
    const int lp = (int)(by << a.g.lft) + (threadIdx.x & (ft - 1));
    const int fl = lane_frame(a.alist, a.acount, a.f_off, lp, live);
    // TRANSIT (the first check sweep after a repack): the lane's frame sits in column f_off + lp of
    // the new set; only its old messages are still at its listed (old) column fl
    const int f = TRANSIT ? a.f_off + lp : fl;
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> a.g.lft);
    // Waves whose 64 frames all stopped leave; in a partly stopped wave the stopped
    // lanes run along (no divergent exit, so the loop state stays scalar): their
    // messages are never read again and their posteriors (the output) are not touched.
    // Lanes past the compacted count (repeating the last listed frame) count as stopped:
    // once fewer than a tile's frames remain, the tile's empty waves leave at once.
    const bool act = live && a.active[f] != 0;
    if (!wave_any(act)) return;
    int64_t ci = (int64_t)bx * per * nsub + sub;
    if (ci >= a.n_checks) return;
    uint32_t bad = 0;
    const auto K = GlibcK::pinned();
    constexpr bool kPrefetch = !kPacked<D>;
    CheckIn<D, MODE, NT, TRANSIT> nx;
    nx.load(a, ci, f);
    for (int j = 0; j < per; ++j) {
        // consume check j's inputs (m, parity) before its registers take check j+1's
        nx.load_c(a, TRANSIT ? fl : f);
        uint32_t par = nx.sb;
        double m[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double p = nx.p[i];
            if (MODE != kFirst) par ^= (p < 0.0) ? 1u : 0u;   // decoder.pyx:243-246
            if (MODE == kNormal) m[i] = p - nx.c[i];           // :296-297
            else m[i] = p;  // first sweep: c2v == 0 and p - 0.0 == p
        }
        struct { int base; uint8_t sb; } cur = {nx.base, nx.sb};
        const int64_t cn = ci + nsub;
        const bool more = (j + 1 < per) && cn < a.n_checks;   // wave-uniform
        if (kPrefetch && more) nx.load(a, cn, f);
        if (MODE != kFirst) bad |= (par == 1u) ? 1u : 0u;  // satisfied iff (parity ^ 1) != 0
        if (MODE != kParityOnly) {
            const uint32_t b8 = (uint32_t)f * 8u;
            check_exact<D, NT, FIN>(a, m, cur.base, cur.sb, b8, tab, K, hb, live);
        }
        if (!more) break;
        if (!kPrefetch) nx.load(a, cn, f);
        ci = cn;
    }
    if (MODE != kFirst && bad && act && live) a.unsat[f] = 1;  // benign race: every writer stores 1
}

// decoder.pyx:285-298: post[v] = lappr[v] + c2v[e_0] + c2v[e_1] + ... (ascending e).
// INIT: the first sweep with c2v == 0 (decoder.pyx:408,420-421): lappr + 0.0 for
// frames still decoding; frames already successful at iteration 0 get a plain
// copy of their input (decoder.pyx:404).  It sweeps all ld columns but writes only frames
// < fin_B: no sweep touches the output's padding columns [B, ld).
// TRANSIT (the first variable sweep after a repack): the frame's LAPPRs and posterior are in
// column f_off + lp of the new set, its messages still at its listed (old) column of the old set.
template <bool INIT, bool NT, bool TRANSIT = false>
__device__ __forceinline__ void var_block(const VarArgs &a, unsigned bx, unsigned by) {
    const int ft = 1 << a.g.lft;
    const int nsub = 256 >> a.g.lft;
    const int ld = a.ld;
    bool live;
    const int lp = (int)(by << a.g.lft) + (threadIdx.x & (ft - 1));
    const int fl = lane_frame(a.alist, a.acount, a.f_off, lp, live);
    const int f = TRANSIT ? a.f_off + lp : fl;
    const int fc = TRANSIT ? fl : f;
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> a.g.lft);
    const bool act = a.active[f] != 0;
    if (!live || (!INIT && !act)) return;
    if (INIT && f >= a.fin_B) return;  // padding columns [B, ld): the output keeps the caller's values
    const int64_t v0 = (int64_t)bx * a.g.per * nsub + sub;
    bool big = false;
    for (int j = 0; j < a.g.per; ++j) {
        const int64_t v = v0 + (int64_t)j * nsub;
        if (v >= a.V) break;
        const int b = sld(a.var_ptr + v), e = sld(a.var_ptr + v + 1);
        double p = ld_msg<NT>(&a.lappr[(size_t)v * ld + f]);
        if (INIT) {
            big |= !(__builtin_fabs(p) < a.fin_bound);
            if (act && e > b) p = p + 0.0;
        } else {
            for (int k = b; k < e; ++k) p += ld_msg<NT>(&a.c2v[(size_t)sld(a.var_edge + k) * ld + fc]);
        }
        a.post[(size_t)v * ld + f] = p;
    }
    if (INIT && a.finite && big && f < a.fin_B) *a.finite = 0;  // every writer stores 0
}

// ---------------------------------------------------------------------------------------
// Narrow sweeps: a repacked range of at most kNarrowW columns (the last running frames of a
// converging half).  The frame-parallel layout gives every check a 64-lane wave of frames, so
// a handful of running frames still pay a whole wave per check, per checks in sequence.  Such
// a range (known only on the device: its RangeSel) switches the SAME launch, kernel-uniformly,
// to lanes = (node, frame): a workgroup task is kNarrowNodes nodes x kNarrowFrames consecutive
// columns (one 128-byte line per row access), one node per lane, tasks walked grid-stride, the
// CSR read per lane.  Every message is the same operation on the same operands as in
// check_block / var_block, so the bits do not depend on the layout.
constexpr int kNarrowFrames = 16;
constexpr int kNarrowNodes = 256 / kNarrowFrames;
constexpr int kNarrowW = 64;

__device__ __forceinline__ bool range_narrow(const int32_t *sel, const int32_t *acount) {
    return sel && acount && sld(sel + kSelOn) && sld(sel + kSelW) <= kNarrowW && !sld(sel + kSelTransit);
}
// Tasks of a narrow sweep over n nodes: (node block, frame group) pairs, frame group fastest, the
// group count (<= 4) rounded up to 2^lg so that a task splits with a shift and a mask (32-bit task
// arithmetic: the variable sweep keeps its register budget)
__device__ __forceinline__ uint32_t narrow_tasks(int64_t n, const int32_t *acount, int &lg) {
    const int ngrp = (sld(acount) + kNarrowFrames - 1) / kNarrowFrames;
    lg = ngrp > 2 ? 2 : ngrp > 1 ? 1 : 0;
    return ngrp > 0 ? (uint32_t)((n + kNarrowNodes - 1) / kNarrowNodes) << lg : 0u;
}

// The NaN-preserving clamp always (the finite flag's one-instruction clamp gives the same bits
// on finite inputs; the narrow body is not worth a second copy).
template <int D>
__device__ __forceinline__ void check_narrow(const CheckArgs &a, uint32_t task, int lg, const GlibcTablesBP &tab,
                                             double *hb, const GlibcK &K) {
    bool live;
    const int grp = (int)(task & ((1u << lg) - 1u));
    const int f = lane_frame(a.alist, a.acount, a.f_off, grp * kNarrowFrames + (int)(threadIdx.x % kNarrowFrames), live);
    const bool act = live && a.active[f] != 0;
    if (!wave_any(act)) return;  // wave-uniform: the packed update exchanges within the wave
    const int64_t ci = (int64_t)(task >> lg) * kNarrowNodes + threadIdx.x / kNarrowFrames;
    const bool valid = ci < a.n_checks;
    const int cc = a.checks[valid ? ci : a.n_checks - 1];
    int base = a.chk_ptr[cc];
    QR_DCHECK(f >= a.f_off && f < a.f_off + kNarrowW, kDbgNarrowFrame, f, a.f_off);
    QR_DCHECK(cc >= 0 && base >= 0 && a.chk_ptr[cc + 1] - base == D, kDbgNarrowNode, cc, base);
    const size_t ld = a.ld;
    const uint8_t sb = a.synd[(size_t)cc * ld + f];
    uint32_t par = sb;
    double m[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const double p = a.post[(size_t)a.chk_var[base + i] * ld + f];
        par ^= (p < 0.0) ? 1u : 0u;                                // decoder.pyx:243-246
        m[i] = p - a.c2v[(size_t)a.chk_edge[base + i] * ld + f];  // :296-297
    }
    double out[D];
    check_strict_packed<D, kClampFull>(m, out, hb + (threadIdx.x >> 6) * kPackWaveDoubles, tab, K);
    // the stores re-read the edge ids: D message addresses held across the update would raise
    // the kernel's register budget (its frame-parallel body runs at 4 waves/SIMD)
    __asm__ volatile("" : "+v"(base));
    const double s = sb ? -1.0 : 1.0;
    if (valid && act) {
#pragma unroll
        for (int i = 0; i < D; ++i) a.c2v[(size_t)a.chk_edge[base + i] * ld + f] = s * out[i];
        if (par == 1u) a.unsat[f] = 1;  // benign race: every writer stores 1
    }
}

template <int D>
__device__ __forceinline__ void check_narrow_sweep(const CheckArgs &a, GlibcTablesBP &tab, double *hb) {
    int lg;
    const uint32_t ntask = narrow_tasks(a.n_checks, a.acount, lg);
    const uint32_t nb = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;
    if (b >= ntask) return;  // block-uniform
    stage_glibc_tables(&tab, a.gglibc);
    const auto K = GlibcK::pinned();
    for (uint32_t t = b; t < ntask; t += nb) check_narrow<D>(a, t, lg, tab, hb, K);
}

__device__ __forceinline__ void var_narrow_sweep(const VarArgs &a) {
    int lg;
    const uint32_t ntask = narrow_tasks(a.V, a.acount, lg);
    const uint32_t nb = gridDim.x * gridDim.y;
    const size_t ld = a.ld;
    for (uint32_t t = blockIdx.y * gridDim.x + blockIdx.x; t < ntask; t += nb) {
        bool live;
        const int grp = (int)(t & ((1u << lg) - 1u));
        const int f = lane_frame(a.alist, a.acount, a.f_off, grp * kNarrowFrames + (int)(threadIdx.x % kNarrowFrames), live);
        const int64_t v = (int64_t)(t >> lg) * kNarrowNodes + threadIdx.x / kNarrowFrames;
        if (!live || v >= a.V || !a.active[f]) continue;
        QR_DCHECK(f >= a.f_off && f < a.f_off + kNarrowW, kDbgNarrowFrame, f, a.f_off);
        double p = a.lappr[(size_t)v * ld + f];
        const int b = a.var_ptr[v], e = a.var_ptr[v + 1];
        for (int k = b; k < e; ++k) p += a.c2v[(size_t)a.var_edge[k] * ld + f];  // decoder.pyx:292-293
        a.post[(size_t)v * ld + f] = p;
    }
}

// QR_EXPERIMENT_CLOCK (diagnostic builds only, scripts/diag/clock_check.py): every workgroup of
// the degree-7 main-loop check sweep stamps the shader clock (ClkScope, qamr_internal.hpp) around
// its work and adds its spans to g_clk (the frame-resident decode: g_clk_res, decode_small.hip); the
// effective clock of the unprofiled launch is sum(cycles) / sum(ticks) x 100 MHz
// (MI355X_MICROARCH.md 'DVFS give-back' item 6).  qr_debug_clock reads and clears both sums.
#if QR_EXPERIMENT_CLOCK
__device__ unsigned long long g_clk[3];
// realtime start / end of every workgroup of the last such launch (up to kWgTimes workgroups):
// the launch's occupancy over time, i.e. how much of it is the drain at its end
__device__ unsigned long long g_wgt[2 * kWgTimes];
#endif
template <int D, int MODE, bool NT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 8))) k_check(CheckArgs a) {
    __shared__ GlibcTablesBP tab;
    __shared__ double hb[kPackLdsDoubles];
    select_range(a);
    if constexpr (MODE == kNormal && kPacked<D>) {
        if (range_narrow(a.sel, a.acount)) {  // kernel-uniform
            check_narrow_sweep<D>(a, tab, hb);
            return;
        }
    }
    unsigned bx = blockIdx.x, by = blockIdx.y;
    int per = a.g.per;
    if (a.nmain) {  // short-tail 1-D grid (block-uniform)
        if (bx < a.nmain) {
            by = 1 + bx / a.nbx;
            bx -= (by - 1) * a.nbx;
        } else {
            bx -= a.nmain;
            by = 0;
            per = a.per_t;
        }
    }
    if (!frames_block_live(a.acount, by, a.g.lft)) return;  // block-uniform
#if QR_EXPERIMENT_CLOCK
    ClkScope clk(D == 7 && MODE == kNormal, g_clk, g_wgt);
#endif
    if (MODE != kParityOnly) stage_glibc_tables(&tab, a.gglibc);
    // Every templated degree, packed or not: select_range has switched the launch to the new
    // column set whatever D is, so a class that kept the listed (old) columns here would read the
    // posteriors and flags of other frames (run_split2 takes every code of max degree <= 16).
    if constexpr (MODE == kNormal) {
        if (a.transit) {  // kernel-uniform: the first sweep after a repack (NaN-preserving clamp)
            check_block<D, MODE, NT, false, true>(a, bx, by, per, tab, hb);
            return;
        }
    }
    if constexpr (MODE != kParityOnly && kPacked<D>) {
        if (a.finite && sld(a.finite)) {  // kernel-uniform: one of the two bodies runs
            check_block<D, MODE, NT, true>(a, bx, by, per, tab, hb);
            return;
        }
    }
    check_block<D, MODE, NT, false>(a, bx, by, per, tab, hb);
}

template <bool INIT, bool NT, bool TRANSIT>
__device__ __forceinline__ void var_sweep_body(const VarArgs &a);

template <bool INIT, bool NT>
__global__ void __launch_bounds__(256) k_var(VarArgs a) {
    select_range(a);
    if (!INIT && range_narrow(a.sel, a.acount)) {  // kernel-uniform
        var_narrow_sweep(a);
        return;
    }
    if (!INIT && a.transit) var_sweep_body<INIT, NT, true>(a);  // kernel-uniform
    else var_sweep_body<INIT, NT, false>(a);
}

template <bool INIT, bool NT, bool TRANSIT>
__device__ __forceinline__ void var_sweep_body(const VarArgs &a) {
    if (a.gs) {  // capped grid: tile t = (bx fastest, by), the grid's blocks sweep a moving window
        unsigned ny = a.nby, stride = gridDim.x;
        if (a.boost > 1) {
            // The pacing spreads a full sweep over the concurrent check launch; once most frames
            // have stopped, both launches shrink and a paced sweep of the few live tiles would be
            // latency-bound (a few workgroups per CU walking many blocks each): widen it.
            const unsigned w = gridDim.x / (unsigned)a.boost;
            unsigned live = a.nby;
            if (a.acount) live = min(a.nby, (unsigned)((*a.acount + (1 << a.g.lft) - 1) >> a.g.lft));
            const unsigned m = live ? min((unsigned)a.boost, max(1u, a.nby / live)) : 1u;
            stride = w * m;
            ny = live;
            if (blockIdx.x >= stride) return;
        }
        const unsigned n = a.nbx * ny;
        for (unsigned t = blockIdx.x; t < n; t += stride) {
            const unsigned by = t / a.nbx, bx = t - by * a.nbx;
            if (frames_block_live(a.acount, by, a.g.lft)) var_block<INIT, NT, TRANSIT>(a, bx, by);
        }
        return;
    }
    if (!frames_block_live(a.acount, blockIdx.y, a.g.lft)) return;
    var_block<INIT, NT, TRANSIT>(a, blockIdx.x, blockIdx.y);
}


// Check degrees above the templated range (2..kMaxTemplDeg) take a runtime-degree kernel
// with no per-lane arrays, so any degree works (the reference sizes its F/B buffer per
// check, decoder.pyx:131-141): the forward values F_0..F_{d-3} of the reference's
// recursion are parked in an HBM scratch laid out like c2v (one row of ld doubles per
// (check, i), frame-innermost, coalesced), and the backward pass re-reads each v2c =
// post - c2v(old) before it overwrites that edge's message:
//   forward  F_0 = m_0, F_i = bp(F_{i-1}, m_i)              (rows i-1 <- F_{i-1})
//   backward c2v[e_{d-1}] = s F_{d-2}; B = m_{d-1};
//            for i = d-2..1: c2v[e_i] = s bp(F_{i-1}, B); B = bp(B, m_i)
//            c2v[e_0] = s B
// (decoder.pyx:322-369: the same box-plus operands in the same order per output.)
template <int MODE>
__global__ void __launch_bounds__(256) k_check_generic(CheckArgs a) {
    __shared__ GlibcTablesBP tab;
    select_range(a);
    if (MODE != kParityOnly) stage_glibc_tables(&tab, a.gglibc);
    const int ft = 1 << a.g.lft;
    const int nsub = 256 >> a.g.lft;
    const int ld = a.ld;
    if (!frames_block_live(a.acount, blockIdx.y, a.g.lft)) return;
    bool live;
    const int f = lane_frame(a.alist, a.acount, a.f_off, (int)(blockIdx.y << a.g.lft) + (threadIdx.x & (ft - 1)), live);
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> a.g.lft);
    if (!live || !a.active[f]) return;
    const auto K = GlibcK::pinned();
    const int64_t c0 = (int64_t)blockIdx.x * a.g.per * nsub + sub;
    const uint32_t b8 = (uint32_t)f * 8u;
    uint32_t bad = 0;
    for (int j = 0; j < a.g.per; ++j) {
        const int64_t ci = c0 + (int64_t)j * nsub;
        if (ci >= a.n_checks) break;
        const int c = sld(a.checks + ci);
        const int base = sld(a.chk_ptr + c);
        const int d = sld(a.chk_ptr + c + 1) - base;
        const uint8_t sb = *at_byte(row_ptr(a.synd, c, ld), (uint32_t)f);
        const double s = sb ? -1.0 : 1.0;
        uint32_t par = sb;
        // v2c of edge i (decoder.pyx:296-297; first sweep: c2v == 0), parity of post
        auto msg = [&](int i, bool count) {
            const double p = *at_byte(row_ptr(a.post, sld(a.chk_var + base + i), ld), b8);
            if (count && MODE != kFirst) par ^= (p < 0.0) ? 1u : 0u;
            return (MODE == kNormal) ? p - *at_byte(row_ptr(a.c2v, sld(a.chk_edge + base + i), ld), b8) : p;
        };
        if (MODE == kParityOnly) {
            for (int i = 0; i < d; ++i) (void)msg(i, true);
            bad |= (par == 1u) ? 1u : 0u;
            continue;
        }
        double *fb = a.fb + (size_t)(a.fb_base + ci * (int64_t)(d - 2)) * ld;
        double F = msg(0, true);
        for (int i = 1; i <= d - 2; ++i) {
            *at_byte(fb + (size_t)(i - 1) * ld, b8) = F;  // F_{i-1}
            F = box_plus_strict(F, msg(i, true), tab, K);
        }
        double Bn = msg(d - 1, true);
        if (MODE != kFirst) bad |= (par == 1u) ? 1u : 0u;
        *at_byte(row_ptr(a.c2v, sld(a.chk_edge + base + d - 1), ld), b8) = s * F;  // s F_{d-2}
        for (int i = d - 2; i >= 1; --i) {
            const double m = msg(i, false);  // before its edge's message is replaced
            const double Fi = *at_byte(fb + (size_t)(i - 1) * ld, b8);
            *at_byte(row_ptr(a.c2v, sld(a.chk_edge + base + i), ld), b8) = s * box_plus_strict(Fi, Bn, tab, K);
            Bn = box_plus_strict(Bn, m, tab, K);
        }
        *at_byte(row_ptr(a.c2v, sld(a.chk_edge + base), ld), b8) = s * Bn;
    }
    if (MODE != kFirst && bad) a.unsat[f] = 1;
}

// rsel: the two ranges' RangeSel (widths w0, w1), initialised here for every schedule.
__global__ void k_init_status(int B, int ld, uint8_t *active, uint8_t *success, int32_t *iters, int32_t *finite,
                              int32_t *rsel, int w0, int w1) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f == 0) *finite = 1;
    if (f < 2 * kSelInts) rsel[f] = (f % kSelInts == kSelW) ? (f < kSelInts ? w0 : w1) : 0;
    if (f >= ld) return;
    active[f] = (f < B) ? 1 : 0;
    if (f < B) {
        success[f] = 0;
        iters[f] = 0;
    }
}

// Frames in [f0, f1) whose posterior after sweep t satisfies the syndrome stop with
// (success=1, iterations=t) (decoder.pyx:431-433, :402-405 for t = 0).  On the
// final call every still-active frame stops with (0, max_iterations) (:435-436).
// sel / fid_w: see range_fid.
__global__ void k_status(int f0, int f1, int t, int final_call, int32_t final_iters,
                         const uint8_t *__restrict__ unsat_t, uint8_t *active, uint8_t *success, int32_t *iters,
                         const int32_t *sel, const int32_t *__restrict__ fid_w) {
    const int f = f0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= f1 || !active[f]) return;
    const int32_t *fid = range_fid(sel, fid_w);
    const int id = fid ? fid[f] : f;
    if (!unsat_t[f]) {
        success[id] = 1;
        iters[id] = t;
        active[f] = 0;
    } else if (final_call) {
        success[id] = 0;
        iters[id] = final_iters;
        active[f] = 0;
    }
}

// The still-running frames of [f0, f1) in ascending order -> list[f0 + 0 .. count).
// One workgroup of 1024 threads: per 1024-frame chunk a wave ballot, the waves' counts
// through LDS, one store per running frame.  STATUS: the status update of sweep t
// (k_status, never the final call) is applied first, frame by frame, by the same thread:
// one launch instead of two between the check sweeps of the two-stream schedule.
// sel / fid_w as k_status (a repacked range holds frames only in its first sel[kSelW] columns).
template <bool STATUS>
__global__ void __launch_bounds__(1024) k_compact(int f0, int f1, uint8_t *__restrict__ active,
                                                  int32_t *__restrict__ list, int32_t *__restrict__ count, int t,
                                                  const uint8_t *__restrict__ unsat_t, uint8_t *__restrict__ success,
                                                  int32_t *__restrict__ iters, const int32_t *sel,
                                                  const int32_t *__restrict__ fid_w) {
    __shared__ int wsum[16];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t *fid = range_fid(sel, fid_w);
    if (fid) f1 = min(f1, f0 + sld(sel + kSelW));
    int base = 0;  // running count (every thread keeps the same value)
    for (int c0 = f0; c0 < f1; c0 += 1024) {
        const int f = c0 + (int)threadIdx.x;
        bool a = f < f1 && active[f];
        if (STATUS && a && !unsat_t[f]) {  // k_status: satisfied -> (1, t), stops
            const int id = fid ? fid[f] : f;
            success[id] = 1;
            iters[id] = t;
            active[f] = 0;
            a = false;
        }
        const uint64_t m = __ballot(a);
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        int off = base, tot = 0;
        for (int i = 0; i < 16; ++i) {
            off += i < w ? wsum[i] : 0;
            tot += wsum[i];
        }
        QR_DCHECK(!a || off + __popcll(m & ((1ull << lane) - 1ull)) <= f - f0, kDbgCompact, off, f - f0);
        if (a) list[f0 + off + __popcll(m & ((1ull << lane) - 1ull))] = f;
        base += tot;
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
        *count = base;
        // the status launch after a range's check sweep: the sweeps of a repack's transition have
        // all run (variable sweep, side and main check sweeps), the list is in the new columns
        if (STATUS && sel) const_cast<int32_t *>(sel)[kSelTransit] = 0;
    }
}

// ------------------------------------------------------------------ launch
struct DecodeWs {
    double *c2v;
    double *c2v2;    // the second message buffer of the fused small-code schedule (run_iter), or null
    uint8_t *active;
    uint8_t *unsat;  // (max_it + 2) rows of ld flags
    double *fb;      // F scratch of the runtime-degree classes (fb_rows rows of ld), or null
    int32_t *alist;  // active-frame lists of the frame ranges (ld entries)
    int32_t *acount; // their lengths: [0] range starting at frame 0, [1] the second half;
                     // [2] the finite flag of the input LAPPRs (first variable sweep);
                     // [4, 16) the two ranges' RangeSel (rsel)
    int32_t *rsel;
    // the work set of the column repack (k_repack_rows, run_split2): posteriors and the frame id
    // of each column of the repacked ranges, and two column sets of LAPPRs and syndrome bits (and
    // of messages: set 0 is c2v above, set 1 c2v_alt) that consecutive repacks gather into in
    // turn; present when the caller's workspace has room for it (ws_bytes counts it when knob
    // repack is on)
    struct WorkSet {
        double *post;
        double *lappr[2];
        uint8_t *synd[2];
        double *c2v_alt;
        int32_t *fid;
    } rs;
    bool repack;
    size_t base_bytes, set_bytes;  // of the base part; of the work set when the workspace carries it, else 0
};

// The decode workspace, laid out here and nowhere else: the base part every schedule needs, then
// the repack work set.  With a null base the walk only measures (base_bytes, set_bytes; every
// pointer null); with the caller's buffer of ws_size bytes it yields the pointers.
// knob repack (default 1): the workspace carries the work set of the repacked ranges when the
// two-stream schedule can run (ld % 512 == 0) and the set takes at most 1/8 of the device's
// memory (N=64800, ld=4096: 4.4 GB of 288 GB); a decode uses it when ws_size has room for it.
static DecodeWs ws_layout(const qr_code *code, int ld, int max_it, void *base = nullptr, size_t ws_size = 0) {
    DecodeWs w;
    Cursor c{(uintptr_t)base};
    const size_t msgs = (size_t)code->E * ld, posts = (size_t)code->V * ld;
    w.c2v = c.take<double>(msgs);
    w.c2v2 = iter_code(code, ld) ? c.take<double>(msgs) : nullptr;
    w.active = c.take<uint8_t>((size_t)ld);
    w.unsat = c.take<uint8_t>((size_t)unsat_rows(max_it) * ld);
    w.fb = code->fb_rows ? c.take<double>((size_t)code->fb_rows * ld) : nullptr;
    w.alist = c.take<int32_t>((size_t)ld);
    w.acount = c.take<int32_t>(64);  // the 256-byte count block
    w.rsel = w.acount + 4;
    w.base_bytes = c.off;
    w.rs.post = c.take<double>(posts);
    for (int k = 0; k < 2; ++k) {
        w.rs.lappr[k] = c.take<double>(posts);
        w.rs.synd[k] = c.take<uint8_t>((size_t)code->C * ld);
    }
    w.rs.c2v_alt = c.take<double>(msgs);
    w.rs.fid = c.take<int32_t>((size_t)ld);
    const size_t set = c.off - w.base_bytes;
    w.set_bytes = g_tune.repack.load() && ld % 512 == 0 && set <= code->mem_bytes / 8 ? set : 0;
    w.repack = w.set_bytes > 0 && ws_size >= w.base_bytes + w.set_bytes;
    if (!w.repack) w.rs = DecodeWs::WorkSet{};
    return w;
}
size_t ws_bytes(const qr_code *code, int ld, int max_it) {
    const DecodeWs w = ws_layout(code, ld, max_it);
    return w.base_bytes + w.set_bytes;
}

// Frame tile ft (a divisor of ncols, <= ft_req) and nodes per thread.  Small problems (few
// nodes x few frame tiles, e.g. the reg-(3,6) N=1008 code of configs[1]) get fewer nodes per
// thread, down to 1, so that a launch still has ~min_blocks workgroups to spread over the
// 256 CUs (knob min_blocks, 0 = off); the DVB-S2 launches keep their per.
Geom make_geom(int ncols, int ft_req, int per, int64_t nodes) {
    int ft = 256;
    while (ft > 64 && (ft > ft_req || ncols % ft)) ft >>= 1;
    int lft = 6;
    while ((1 << lft) < ft) ++lft;
    per = per < 1 ? 1 : per;
    const int64_t target = g_tune.min_blocks.load();
    if (nodes > 0 && target > 0) {
        const int64_t tiles = ncols >> lft, nsub = 256 >> lft;
        const int64_t fit = nodes * tiles / (target * nsub);   // per that gives ~target blocks
        if (fit < per) per = (int)(fit < 1 ? 1 : fit);
    }
    return Geom{lft, per};
}

// Everything one decode call needs to issue its launches.
struct Plan {
    const qr_code *code;
    int B, ld;
    const double *lappr;
    const uint8_t *synd;
    double *post;
    uint8_t *success;
    int32_t *iters;
    DecodeWs w;
    bool nt;
    hipStream_t s;
    int lds_pad = 0;  // dynamic LDS reserved by each check workgroup (caps their CU residency)
    bool compact = false;  // sweeps of the main loop read the active-frame lists
    int var_pace = 0;      // variable sweeps: workgroups per 128 frames (0 = one per tile)
    // run_split2 with the device-steered column repack: every launch of a range carries the
    // range's RangeSel (steer); parity-only sweeps read the active-frame lists too (list_parity:
    // the final sweep)
    bool steer = false;
    bool list_parity = false;

    const int32_t *count_of(int f0) const { return w.acount + (f0 == 0 ? 0 : 1); }
    const int32_t *sel_of(int f0) const { return steer ? w.rsel + (f0 == 0 ? 0 : kSelInts) : nullptr; }

    CheckArgs check_args(const DegreeClass &cls, const double *post_in, uint8_t *unsat, int f0, int f1) const {
        CheckArgs a;
        a.checks = cls.d_checks;
        a.n_checks = cls.n;
        a.chk_ptr = code->d_chk_ptr;
        a.chk_edge = code->d_chk_edge;
        a.chk_var = code->d_chk_var;
        a.post = post_in;
        a.c2v = w.c2v;
        a.synd = synd;
        a.active = w.active;
        a.unsat = unsat;
        a.ld = ld;
        a.f_off = f0;
        a.g = make_geom(f1 - f0, g_tune.check_ft.load(), g_tune.check_per.load(), cls.n);
        const int64_t per_block = (int64_t)a.g.per * (256 >> a.g.lft);
        a.nbx = (unsigned)((cls.n + per_block - 1) / per_block);
        a.gglibc = code->d_gtab;
        a.fb = w.fb;
        a.fb_base = cls.fb_base;
        a.alist = a.acount = nullptr;
        a.finite = w.acount + 2;
        a.nmain = 0;
        a.per_t = a.g.per;
        a.sel = sel_of(f0);
        a.post_w = w.rs.post;
        a.synd_w[0] = w.rs.synd[0];
        a.synd_w[1] = w.rs.synd[1];
        a.c2v_alt = w.rs.c2v_alt;
        a.transit = 0;
        a.c2v_rd = a.c2v;
        return a;
    }
    VarArgs var_args(int f0, int f1) const {
        VarArgs a;
        a.V = code->V;
        a.var_ptr = code->d_var_ptr;
        a.var_edge = code->d_var_edge;
        a.lappr = lappr;
        a.c2v = w.c2v;
        a.post = post;
        a.active = w.active;
        a.ld = ld;
        a.f_off = f0;
        a.g = make_geom(f1 - f0, g_tune.var_ft.load(), g_tune.var_per.load(), code->V);
        const int64_t per_block = (int64_t)a.g.per * (256 >> a.g.lft);
        a.nbx = (unsigned)((code->V + per_block - 1) / per_block);
        a.alist = a.acount = nullptr;
        a.nby = (unsigned)((f1 - f0) >> a.g.lft);
        a.gs = 0;
        a.boost = 1;
        a.finite = nullptr;
        a.fin_bound = 0.0;
        a.fin_B = 0;
        a.sel = sel_of(f0);
        a.lappr_w[0] = w.rs.lappr[0];
        a.lappr_w[1] = w.rs.lappr[1];
        a.post_w = w.rs.post;
        a.c2v_alt = w.rs.c2v_alt;
        a.transit = 0;
        return a;
    }
};

template <int MODE, bool NT>
static int launch_check_class(const Plan &P, const DegreeClass &cls, const double *post_in, uint8_t *unsat, int f0,
                              int f1) {
    CheckArgs a = P.check_args(cls, post_in, unsat, f0, f1);
    if (P.compact && (MODE != kParityOnly || P.list_parity)) {
        a.alist = P.w.alist;
        a.acount = P.count_of(f0);
    }
    const dim3 grid2(a.nbx, (unsigned)((f1 - f0) >> a.g.lft));   // the plain 2-D grid
    dim3 grid = grid2;
    // knob check_tail (default 4; 0 = off; MI355X: +1 %): frame tile 0 is swept last with per / check_tail
    // checks per thread (the templated degrees only; the runtime-degree kernel keeps the 2-D grid)
    const int tail = g_tune.check_tail.load();
    const bool templ = cls.degree >= 2 && cls.degree <= kMaxTemplDeg;
    if (tail > 1 && grid.y >= 2 && templ && a.g.per >= tail) {
        const int64_t per_block_t = (int64_t)(a.g.per / tail) * (256 >> a.g.lft);
        const int64_t nbx_t = (cls.n + per_block_t - 1) / per_block_t;
        a.nmain = a.nbx * (grid.y - 1);
        a.per_t = a.g.per / tail;
        grid = dim3((unsigned)(a.nmain + nbx_t), 1);
    }
    ProfScope ps(profiling_on() ? std::string(MODE == kParityOnly ? "parity_d" : MODE == kFirst ? "check1_d" : "check_d") +
                                      std::to_string(cls.degree)
                                : std::string(),
                 P.s);
    const bool handled = dispatch_degree<2, kMaxTemplDeg>(
        cls.degree, [&](auto d) { k_check<d.value, MODE, NT><<<grid, 256, P.lds_pad, P.s>>>(a); });
    if (!handled) {  // the runtime-degree kernel decodes its frame tile from blockIdx.y: 2-D grid only
        a.nmain = 0;
        a.per_t = a.g.per;
        k_check_generic<MODE><<<grid2, 256, 0, P.s>>>(a);
    }
    QR_LAUNCH_CHECK();
    return QR_OK;
}

// Check sweep of frames [f0, f1) over every degree class except `skip` (index or -1).
template <int MODE>
static int launch_checks(const Plan &P, const double *post_in, uint8_t *unsat, int f0, int f1, int skip = -1) {
    for (int k = 0; k < (int)P.code->classes.size(); ++k) {
        if (k == skip) continue;
        const DegreeClass &cls = P.code->classes[k];
        int rc = P.nt ? launch_check_class<MODE, true>(P, cls, post_in, unsat, f0, f1)
                      : launch_check_class<MODE, false>(P, cls, post_in, unsat, f0, f1);
        if (rc) return rc;
    }
    return QR_OK;
}

template <bool INIT>
static int launch_var(const Plan &P, int f0, int f1, int32_t *finite = nullptr, double fin_bound = 0.0) {
    ProfScope ps(INIT ? "var_init" : "var", P.s);
    VarArgs a = P.var_args(f0, f1);
    a.finite = finite;
    a.fin_bound = fin_bound;
    a.fin_B = P.B;
    if (P.compact && !INIT) {
        a.alist = P.w.alist;
        a.acount = P.count_of(f0);
    }
    dim3 grid(a.nbx, a.nby);
    // Paced sweep (the two-stream schedule's variable sweeps, Plan::var_pace): at most var_pace
    // workgroups per 128 frames of the sweep, each walking its tiles grid-stride, so that the sweep streams its
    // bytes over about the length of the concurrent check sweep instead of saturating HBM for
    // the first ~40 % of it.
    const int64_t cap = (int64_t)P.var_pace * (((int64_t)a.nby << a.g.lft) / 128);  // per 128 frames
    if (cap > 0 && (int64_t)a.nbx * a.nby > cap) {
        a.gs = 1;
        // knob var_boost (default 4, 1 = off): the sweep widens as the live tiles drop
        a.boost = std::max(1, std::min(g_tune.var_boost.load(), 16));
        grid = dim3((unsigned)(cap * a.boost), 1);
    }
    if (P.nt) k_var<INIT, true><<<grid, 256, 0, P.s>>>(a);
    else k_var<INIT, false><<<grid, 256, 0, P.s>>>(a);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int launch_init_status(int B, int ld, uint8_t *active, uint8_t *success, int32_t *iters, int32_t *finite, int32_t *rsel,
                       int w0, int w1, hipStream_t s) {
    k_init_status<<<(ld + 255) / 256, 256, 0, s>>>(B, ld, active, success, iters, finite, rsel, w0, w1);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

// k_status over the columns [f0, f1) (nothing to launch when the range is empty)
int launch_status(int f0, int f1, int t, int final_call, int32_t final_iters, const uint8_t *unsat_t, uint8_t *active,
                  uint8_t *success, int32_t *iters, const int32_t *sel, const int32_t *fid, hipStream_t s) {
    ProfScope ps("status", s);
    if (f1 <= f0) return QR_OK;
    k_status<<<(f1 - f0 + 255) / 256, 256, 0, s>>>(f0, f1, t, final_call, final_iters, unsat_t, active, success, iters, sel,
                                                   fid);
    QR_LAUNCH_CHECK();
    return QR_OK;
}
static int launch_status(const Plan &P, int f0, int f1, int t, int final_call, int32_t final_iters,
                         const uint8_t *unsat_t) {
    return launch_status(f0, std::min(f1, P.B), t, final_call, final_iters, unsat_t, P.w.active, P.success, P.iters,
                         P.sel_of(f0), P.w.rs.fid, P.s);
}

// Rebuild the active-frame list of [f0, f1) after a status update (no-op without compaction).
static int launch_compact(const Plan &P, int f0, int f1) {
    if (!P.compact) return QR_OK;
    k_compact<false><<<1, 1024, 0, P.s>>>(f0, f1, P.w.active, P.w.alist, const_cast<int32_t *>(P.count_of(f0)), 0,
                                          nullptr, nullptr, nullptr, P.sel_of(f0), P.w.rs.fid);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

// Status update of sweep t (not the final call) + list rebuild of [f0, f1): one launch with
// compaction, k_status alone without.
static int launch_status_compact(const Plan &P, int f0, int f1, int t, const uint8_t *unsat_t) {
    if (!P.compact) return launch_status(P, f0, f1, t, 0, 0, unsat_t);
    ProfScope ps("status", P.s);
    k_compact<true><<<1, 1024, 0, P.s>>>(f0, f1, P.w.active, P.w.alist, const_cast<int32_t *>(P.count_of(f0)), t,
                                         unsat_t, P.success, P.iters, P.sel_of(f0), P.w.rs.fid);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

// Flooding schedule, all frames in lock-step (decoder.pyx:424-433).
static int run_flat(const Plan &P, int max_it) {
    const int ld = P.ld;
    int rc;
    for (int t = 1; t <= max_it; ++t) {
        uint8_t *unsat_prev = P.w.unsat + (size_t)(t - 1) * ld;
        if (t == 1) {
            if ((rc = launch_checks<kFirst>(P, P.post, unsat_prev, 0, ld))) return rc;
        } else {
            if ((rc = launch_checks<kNormal>(P, P.post, unsat_prev, 0, ld))) return rc;
            if ((rc = launch_status_compact(P, 0, ld, t - 1, unsat_prev))) return rc;
        }
        if ((rc = launch_var<false>(P, 0, ld))) return rc;
    }
    return QR_OK;
}

// The two-stream schedule (split = 3): the batch is cut in two frame halves A | B whose sweeps
// run half an iteration apart, as separate kernels on two streams.  C = check sweep (+ parity
// of the previous posteriors), S = status update, V = variable sweep; per frame the order
// C(t) -> S(t-1) -> V(t) -> C(t+1) is exactly that of run_flat.  The caller's stream s runs
// the check sweeps and status updates, s2 the variable sweeps, events order them:
//   s : C_A(1) | [wait vB] C_B(t) S_B(t-1) | [wait vA] C_A(t+1) S_A(t) | ...
//   s2:        | [wait cA] V_A(t)          | [wait cB] V_B(t)           | ...
// The variable sweep's 12-VGPR waves fill whatever the 128-VGPR check waves leave of
// each SIMD and stream their messages under the check sweep's fp64 arithmetic (rounds 1-2
// ran both sweeps as the workgroups of one launch, where the variable workgroups took whole
// check-sized slots: 5.35 ms per half-iteration against 5.15 here, strict arithmetic,
// MI355X, B=4096).  The variable sweeps are paced
// (knob var_pace, workgroups per 128 frames, default 28): unpaced, the sweep saturates HBM for
// the first ~1.7 ms of the 4.3 ms check launch beside it and the check sweep's gathers stall
// (VALU issue 0.72 of the launch); paced to stream over the whole check launch, 4.15 ms and
// 0.85 (MI355X, B=4096: 8.96 k -> 9.70 k frames/s on one box).  Knob lds_pad_kb reserves
// LDS per check workgroup to cap their residency (40/48 KB -> 3 per CU: 5.22-5.26 ms;
// 64 KB -> 2: 5.65 ms; 0 = default).
// The second stream of the two-stream schedules and its events, created on first use (all or
// nothing; the caller holds code->mu).
int side_stream(const qr_code *code, hipStream_t *out) {
    if (!code->s2) {
        hipStream_t s2 = nullptr;
        hipEvent_t ev[5] = {};
        hipError_t e = hipStreamCreateWithFlags(&s2, hipStreamNonBlocking);
        for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        if (e != hipSuccess) {
            for (auto x : ev)
                if (x) (void)hipEventDestroy(x);
            if (s2) (void)hipStreamDestroy(s2);
            return set_error(QR_EDEVICE, "decode: second stream: %s", hipGetErrorString(e));
        }
        for (int i = 0; i < 5; ++i) code->ev[i] = ev[i];
        code->s2 = s2;
    }
    *out = code->s2;
    return QR_OK;
}

// A repack decision point of the range starting at column f0, on P.s (the variable stream): one
// launch, k_repack_rows, decides and, when it repacks, moves the columns and (its last
// workgroup) updates the range's state.
static int launch_repack(const Plan &P, int f0) {
    RepackArgs r;
    r.f0 = f0;
    r.ld = P.ld;
    r.pct = std::clamp(g_tune.repack_pct.load(), 1, 90);
    r.V = P.code->V;
    r.C = P.code->C;
    r.count = P.count_of(f0);
    r.sel = P.w.rsel + (f0 == 0 ? 0 : kSelInts);
    r.list = P.w.alist;
    r.active = P.w.active;
    r.out_post = P.post;
    r.lappr_in = P.lappr;
    r.synd_in = P.synd;
    r.post_w = P.w.rs.post;
    for (int k = 0; k < 2; ++k) {
        r.lappr_w[k] = P.w.rs.lappr[k];
        r.synd_w[k] = P.w.rs.synd[k];
    }
    r.fid_w = P.w.rs.fid;
    ProfScope ps("repack", P.s);
    // repack_grid workgroups walk the row groups; when the device decides not to repack they all
    // leave at once (a few microseconds on the variable stream)
    return launch_repack_rows(r, (unsigned)std::clamp(g_tune.repack_grid.load(), 1, 4096), P.s);
}

// *finalized: the final parity check, status and output were issued here (device-steered repack).
static int run_split2(const Plan &P, int max_it, bool *finalized) {
    const qr_code *code = P.code;
    // held while this decode ENQUEUES on the code's second stream and events; nothing here waits
    // for the GPU
    std::lock_guard<std::mutex> lk(code->mu);
    *finalized = false;
    hipStream_t s2 = nullptr;
    if (int rc0 = side_stream(code, &s2)) return rc0;
    hipEvent_t fork = code->ev[0], cA = code->ev[1], cB = code->ev[2], vA = code->ev[3], vB = code->ev[4];
    const int ld = P.ld, h = ld / 2;  // ld % 512 == 0: both ranges are h columns wide
    // Column repack (knob repack, default 1; needs the workspace's work set), decided on the device
    // at every decision point (k_repack_rows before each variable sweep of a
    // range): the host enqueues the same launches whatever the data, never reads anything back
    // and never waits, so the decode is asynchronous and capturable (the host runs far ahead of
    // the GPU anyway: counts it could read without waiting would be an iteration-old at best).
    const bool rp = P.compact && P.w.repack && g_tune.repack.load();
    Plan base = P;
    base.steer = rp;
    Plan Pb = base;  // status launches (P.s)
    Plan V = base;
    V.s = s2;
    V.var_pace = g_tune.var_pace.load();
    Plan C = base;
    C.lds_pad = std::max(0, g_tune.lds_pad_kb.load()) * 1024;
    auto row = [&](int t) { return P.w.unsat + (size_t)t * ld; };
    // Knob side (default 1): the check sweeps of the small degree classes (DVB-S2: the one
    // degree-6 check) run on the variable stream right after the variable sweep they follow,
    // under the other half's big check launch, instead of as a ~30 us launch of their own on
    // the critical check stream.  Per frame the order is unchanged: var(t) -> side checks
    // (t+1) -> [event] big checks(t+1) -> status(t) -> compaction -> [event] var(t+1).
    int big = 0;
    int64_t side_edges = 0;
    for (int k = 1; k < (int)code->classes.size(); ++k)
        if (code->classes[k].n > code->classes[big].n) big = k;
    for (int k = 0; k < (int)code->classes.size(); ++k)
        if (k != big) side_edges += code->classes[k].n * code->classes[k].degree;
    const bool side = g_tune.side.load() && code->classes.size() > 1 && side_edges * 8 <= code->E;
    auto checks_main = [&](int t, int k) {  // check sweep t >= 2 of range k on the check stream
        const int f0 = k * h, f1 = f0 + h;
        if (!side) return launch_checks<kNormal>(C, P.post, row(t - 1), f0, f1);
        const DegreeClass &cls = code->classes[big];
        return P.nt ? launch_check_class<kNormal, true>(C, cls, P.post, row(t - 1), f0, f1)
                    : launch_check_class<kNormal, false>(C, cls, P.post, row(t - 1), f0, f1);
    };
    auto checks_side = [&](int t, int k) {  // the other classes of check sweep t, on V.s
        if (!side) return (int)QR_OK;
        return launch_checks<kNormal>(V, P.post, row(t - 1), k * h, (k + 1) * h, big);
    };
    // range k's variable sweep t, preceded by its repack decision point (the status launch it
    // waits for wrote the count the device decides on); the copies run under the other range's
    // check launch.  No decision before the last variable sweep: a repack's transition ends with
    // the check sweep that follows it (the final parity sweep reads the columns of the list).
    auto var_sweep = [&](int k, int t) {
        const int f0 = k * h;
        if (rp && t < max_it) {
            if (int rc0 = launch_repack(V, f0)) return rc0;
        }
        return launch_var<false>(V, f0, f0 + h);
    };
    auto status = [&](int k, int ts) -> int {
        return launch_status_compact(Pb, k * h, (k + 1) * h, ts, row(ts));
    };
    int rc;
    QR_HIP(hipEventRecord(fork, P.s));
    QR_HIP(hipStreamWaitEvent(V.s, fork, 0));
    if ((rc = launch_checks<kFirst>(C, P.post, row(0), 0, h))) return rc;
    QR_HIP(hipEventRecord(cA, P.s));
    for (int t = 1; t <= max_it; ++t) {
        QR_HIP(hipStreamWaitEvent(V.s, cA, 0));
        if ((rc = var_sweep(0, t))) return rc;
        if (t < max_it && (rc = checks_side(t + 1, 0))) return rc;
        QR_HIP(hipEventRecord(vA, V.s));
        if (t == 1) {
            if ((rc = launch_checks<kFirst>(C, P.post, row(0), h, ld))) return rc;
        } else {
            QR_HIP(hipStreamWaitEvent(P.s, vB, 0));
            if ((rc = checks_main(t, 1))) return rc;
            if ((rc = status(1, t - 1))) return rc;
        }
        QR_HIP(hipEventRecord(cB, P.s));
        if (t < max_it) {
            QR_HIP(hipStreamWaitEvent(P.s, vA, 0));
            if ((rc = checks_main(t + 1, 0))) return rc;
            if ((rc = status(0, t))) return rc;
            QR_HIP(hipEventRecord(cA, P.s));
        }
        QR_HIP(hipStreamWaitEvent(V.s, cB, 0));
        if ((rc = var_sweep(1, t))) return rc;
        if (t < max_it && (rc = checks_side(t + 1, 1))) return rc;
        QR_HIP(hipEventRecord(vB, V.s));
    }
    // join: everything after (final parity check, status) follows both sweeps (vB follows cB)
    QR_HIP(hipStreamWaitEvent(P.s, vA, 0));
    QR_HIP(hipStreamWaitEvent(P.s, vB, 0));
    if (!rp) return QR_OK;
    // decoder.pyx:424-436 per range, wherever its frames live: the parity of the last posteriors
    // of its running frames (the lists), the final status, then every frame of a repacked range
    // hands its posteriors to the output
    uint8_t *unsat_last = row(max_it);
    Plan F = base;
    F.list_parity = true;
    for (int k = 0; k < 2; ++k) {
        const int f0 = k * h;
        if ((rc = launch_checks<kParityOnly>(F, P.post, unsat_last, f0, f0 + h))) return rc;
        if ((rc = launch_status(F, f0, f0 + h, max_it, 1, max_it, unsat_last))) return rc;
        ProfScope ps("repack_out", P.s);
        rc = launch_repack_output(code->V, f0, ld, F.sel_of(f0), P.w.rs.fid, P.w.rs.post, P.post, 4096, P.s);
        if (rc) return rc;
    }
    *finalized = true;
    return QR_OK;
}

int decode_batch_device(const qr_code *code, int B, int ld, const double *lappr, const uint8_t *synd, int max_it,
                        double *final_post, uint8_t *success, int32_t *iters, void *ws_ptr, size_t ws_size,
                        hipStream_t s) {
    if (B <= 0 || ld < B || ld % kWave)
        return set_error(QR_EVALUE, "decode: need 0 < B <= ld and ld %% 64 == 0 (B=%d, ld=%d)", B, ld);
    if (!lappr || !synd || !final_post || !success || !iters || !ws_ptr)
        return set_error(QR_EVALUE, "decode: null pointer argument");
    if (!ws_aligned(ws_ptr)) return set_error(QR_EVALUE, "decode: workspace must be 256-byte aligned");
    const DecodeWs w = ws_layout(code, ld, max_it, ws_ptr, ws_size);
    if (ws_size < w.base_bytes)
        return set_error(QR_EVALUE, "decode: workspace too small (%zu < %zu)", ws_size, w.base_bytes);
    DeviceGuard dg(code->device);
    if (takes_resident(code, max_it))
        return run_resident(code, B, ld, lappr, synd, max_it, final_post, success, iters, w.rsel, s);
    Plan P{code, B, ld, lappr, synd, final_post, success, iters, w, g_tune.nt.load() != 0, s};
    int rc;
    QR_HIP(hipMemsetAsync(P.w.unsat, 0, (size_t)unsat_rows(max_it) * ld, s));
    if ((rc = launch_init_status(B, ld, P.w.active, success, iters, P.w.acount + 2, P.w.rsel, ld / 2, ld - ld / 2, s)))
        return rc;
    // the strict arithmetic's finite flag: no bound, never set; otherwise the first variable sweep
    // computes it, which reads every LAPPR anyway
    const double fin_bound = finite_bound(max_it, code->max_dv);
    if (fin_bound == 0.0) QR_HIP(hipMemsetAsync(P.w.acount + 2, 0, sizeof(int32_t), s));
    int32_t *fin_flag = fin_bound > 0.0 ? P.w.acount + 2 : nullptr;
    // decoder.pyx:400-405: the input itself may already satisfy the syndrome.
    if ((rc = launch_checks<kParityOnly>(P, lappr, P.w.unsat, 0, ld))) return rc;
    if ((rc = launch_status(P, 0, ld, 0, 0, 0, P.w.unsat))) return rc;
    // decoder.pyx:408-421: c2v = 0, first variable sweep.
    if ((rc = launch_var<true>(P, 0, ld, fin_flag, fin_bound))) return rc;
    int max_deg = 0;
    int64_t max_n = 0;
    for (const auto &c : code->classes) max_deg = std::max(max_deg, c.degree), max_n = std::max(max_n, c.n);
    // Knob split: 0 or 1 = lock-step always, 3 (default) = the two-stream schedule where it pays.
    // It overlaps one half's check sweep with the other half's variable sweep;
    // that pays only when a half's check launch fills the chip on its own (DVB-S2 N=64800:
    // 1013 check blocks x 16 frame tiles at B = 4096).  A small code (configs[1]: reg-(3,6)
    // N=1008, B = 1024: 64 blocks) runs all frames in lock-step instead -- 4.9x the frames/s
    // of the split schedule on MI355X.  Knob split_min_blocks (0 = always split).
    const Geom gh = make_geom(ld / 2, g_tune.check_ft.load(), g_tune.check_per.load());
    const int64_t half_blocks = (max_n + (int64_t)gh.per * (256 >> gh.lft) - 1) / ((int64_t)gh.per * (256 >> gh.lft)) *
                                ((ld / 2) >> gh.lft);
    const bool split = g_tune.split.load() == 3 && ld % 512 == 0 && max_deg <= 16 && half_blocks >= g_tune.split_min_blocks.load();
    const bool iter = !split && max_it > 0 && g_tune.fused_iter.load() && P.w.c2v2;
    if (iter) {
        const IterRun R{code,  B,      ld,      lappr,    synd,     final_post, success,
                        iters, w.c2v,  w.c2v2,  w.unsat,  w.active, w.acount,   s};
        if ((rc = run_iter(R, max_it))) return rc;
        // P(max_it + 1) was the parity sweep of the last posteriors; every frame still running stops
        return launch_status(P, 0, ld, max_it, 1, max_it, P.w.unsat + (size_t)max_it * ld);
    }
    // active-frame lists of the ranges the schedule sweeps (after the iteration-0 status)
    P.compact = g_tune.compact.load() != 0;
    if (split) {
        if ((rc = launch_compact(P, 0, ld / 2)) || (rc = launch_compact(P, ld / 2, ld))) return rc;
    } else if ((rc = launch_compact(P, 0, ld))) {
        return rc;
    }
    bool finalized = false;
    if ((rc = split ? run_split2(P, max_it, &finalized) : run_flat(P, max_it))) return rc;
    if (finalized) return QR_OK;
    // Check after the last sweep; then every frame still running stops with (0, max).
    const int tf = max_it > 0 ? max_it : 0;
    uint8_t *unsat_last = P.w.unsat + (size_t)tf * ld;
    if (max_it > 0) {
        if ((rc = launch_checks<kParityOnly>(P, final_post, unsat_last, 0, ld))) return rc;
    } else {
        // decoder.pyx:424 with max_iterations <= 0: no sweep, no check -> (0, max_iterations)
        QR_HIP(hipMemsetAsync(unsat_last, 1, (size_t)ld, s));
    }
    if ((rc = launch_status(P, 0, ld, tf, 1, max_it, unsat_last))) return rc;
    return QR_OK;
}

// A plan over the caller's arrays alone (no message buffer, lists or work set): what the two
// sweeps below read.  counts: a count block (its finite flag's address travels in the arguments;
// neither sweep reads it).
static Plan bare_plan(const qr_code *code, int B, int ld, const double *lappr, const uint8_t *synd, double *post,
                      const uint8_t *active, int32_t *counts, hipStream_t s) {
    DecodeWs w{};
    w.active = const_cast<uint8_t *>(active);
    w.acount = counts;
    w.rsel = counts + 4;
    return Plan{code, B, ld, lappr, synd, post, nullptr, nullptr, w, g_tune.nt.load() != 0, s};
}

int launch_parity_sweep(const qr_code *code, int B, int ld, const double *post, const uint8_t *synd,
                        const uint8_t *active, uint8_t *unsat, int32_t *counts, hipStream_t s) {
    const Plan P = bare_plan(code, B, ld, nullptr, synd, nullptr, active, counts, s);
    return launch_checks<kParityOnly>(P, post, unsat, 0, ld);
}

int launch_var_init(const qr_code *code, int B, int ld, const double *lappr, double *post, const uint8_t *active,
                    int32_t *counts, hipStream_t s) {
    const Plan P = bare_plan(code, B, ld, lappr, nullptr, post, active, counts, s);
    return launch_var<true>(P, 0, ld);
}

#if QR_DEBUG_ASSERT
// the list every unit compiled with checks registers its counter's reader in (debug_check.hpp)
DebugReaders &debug_readers() {
    static DebugReaders readers;
    return readers;
}
#endif

}  // namespace qr

using namespace qr;

extern "C" {

#if QR_DEBUG_ASSERT
// Debug build only (libqamr_debug.so; not in include/qamr.h): out = {failed device checks of every
// unit, first failing site, its two values} -- the first unit with a failure in the order the
// units registered (debug_check.hpp); reads and clears every unit's counter.
QR_API int qr_debug_asserts(int64_t *out) {
    if (hipDeviceSynchronize() != hipSuccess) return QR_EDEVICE;
    for (int i = 0; i < 4; ++i) out[i] = 0;
    const qr::DebugReaders &units = qr::debug_readers();
    if (units.n > qr::DebugReaders::kMax) return QR_EVALUE;  // a unit's reader was dropped
    for (int k = 0; k < units.n; ++k) {
        unsigned long long u[4] = {};
        if (!units.fn[k](u)) return QR_EDEVICE;
        if (u[0] && !out[0])
            for (int i = 1; i < 4; ++i) out[i] = (int64_t)u[i];
        out[0] += (int64_t)u[0];
    }
    return QR_OK;
}
#endif

#if QR_EXPERIMENT_CLOCK
// Diagnostic builds only (not in include/qamr.h): out = {sum cycles, sum ticks, workgroups} of the
// stamped check sweep and of k_resident together; reads and clears both.
QR_API int qr_debug_clock(int64_t *out) {
    unsigned long long h[3] = {0, 0, 0}, r[3] = {0, 0, 0};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(qr::g_clk), sizeof(h)) != hipSuccess) return QR_EDEVICE;
    const unsigned long long z[3] = {0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(qr::g_clk), z, sizeof(z)) != hipSuccess) return QR_EDEVICE;
    if (!qr::resident_clock_read_clear(r)) return QR_EDEVICE;  // k_resident's (decode_small.hip)
    for (int i = 0; i < 3; ++i) out[i] = (int64_t)(h[i] + r[i]);
    return QR_OK;
}
// out[2 n]: realtime {start, end} of workgroups 0..n-1 of the last stamped launch
QR_API int qr_debug_wg_times(int64_t *out, int32_t n) {
    if (n < 0 || n > qr::kWgTimes) return QR_EVALUE;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(qr::g_wgt), (size_t)n * 16) != hipSuccess) return QR_EDEVICE;
    return QR_OK;
}
#endif

int qr_decode_repack_stats(const qr_code *code, int32_t ld, int32_t max_it, const void *ws, size_t ws_size,
                           int32_t *out) {
    if (!code || !ws || !out) return set_error(QR_EVALUE, "null argument");
    if (ld <= 0 || ld % kWave) return set_error(QR_EVALUE, "ld must be a positive multiple of 64");
    const DecodeWs w = ws_layout(code, ld, max_it, const_cast<void *>(ws), ws_size);
    if (ws_size < w.base_bytes) return set_error(QR_EVALUE, "workspace too small");
    int32_t sel[2 * kSelInts];
    DeviceGuard dg(code->device);
    QR_HIP(hipMemcpy(sel, w.rsel, sizeof(sel), hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; ++k) {
        out[k] = sel[k * kSelInts + kSelRepacks];
        out[2 + k] = sel[k * kSelInts + kSelW];
    }
    return QR_OK;
}

}  // extern "C"
