// decode_repack.hip -- the column repack of the two-stream decode schedule (decoder.hip
// run_split2): k_repack_rows, k_repack_output and their launchers.
#include "debug_check.hpp"
#include "decode_dev.hpp"
#include "decode_host.hpp"

namespace qr {

// Column repack of a converging frame range (run_split2, knob repack).  With the active-frame
// lists a sweep's lanes map to the still-running frames, but those frames' columns lie
// scattered over the range: once most frames have stopped, every 8-byte message access of a
// lane is a cache line of its own, and a launch over a few hundred frames costs as much as one
// over the whole range (MI355X, 4-PAM 4.0 dB: 3.7 ms for 418 running frames of 2048, 1.6 ms
// for 76).  The repack moves the running frames' columns to the front of the range, so the
// lanes read contiguous columns again.  Each column copy moves the same bits: the decode's
// arithmetic is untouched.
//
// Everything is decided on the device, so the decode stays asynchronous and capturable: at
// each decision point (before a range's variable sweep, on the variable stream) k_repack_rows
// reads the range's running-frame count (written by its last status launch) and its RangeSel;
// when the running frames fill at most pct % of the range's width w, the range moves to
// w' = max(64, count rounded up to 64):
//   * messages, LAPPRs, syndrome bits: gathered from the range's current column set into the
//     other one of the work set's two (set 0: the workspace's c2v rows + lappr_w[0] / synd_w[0],
//     set 1: c2v_alt + lappr_w[1] / synd_w[1]; the first repack reads the caller's LAPPRs and
//     syndrome bits and the workspace's messages, and writes set 1).  Source and destination
//     never alias, so the moves need no ordering between threads: no barrier, any grid, every
//     load of a thread in flight at once -- the row moves run at copy bandwidth (round 5
//     compacted in place, one barrier per row chunk: 2-3 ms per repack, latency-bound);
//   * posteriors are not moved (the variable sweep right after writes every running frame's
//     posterior in its new column, in the work set's post rows); frames stopped since the last
//     repack first hand theirs to the caller's output through fid (again barrier-free:
//     work set -> output);
//   * fid[column] = the frame the column holds (-1: none), the list becomes the identity, the
//     active flags follow the frames.
// The decision points run on the variable stream beside the other range's check launch, whose
// waves hold 4 x 120 of the 512 VGPRs of a SIMD: the repack waves must fit in the 32 left, or
// their workgroups are dispatched only as check workgroups retire (a first 48-VGPR version waited
// ~0.26 ms per decision point at 4-PAM 4.0 dB).  So each thread's slots (source and destination
// element offsets of a group of rows) are computed once and held in registers for all the row
// groups it moves, and loads and stores are raw buffer accesses off a scalar base.
// Register note (MI355X, measured, mechanism not established): the kernels launched beside the
// check waves (120 VGPRs allocated, 4 per SIMD) must allocate 16 or 32 VGPRs, not 24.  With this
// kernel at 24 (22 used) every dense iteration ran slower, although at a dense iteration it only
// reads two words and exits: headline 9 547 vs 9 790 frames/s (same box, alternating runs), 9 798
// with the round's earlier 28-VGPR version; a variable sweep at 24 (18 used) cost the same
// (9 552 vs 9 776).  So k_repack_rows allocates 32 (an empty asm clobbering v31) and k_var stays
// at 16 (32-bit task arithmetic in its narrow sweep); tests/test_vgpr_budget.py checks both in the
// built code object.
constexpr int kRepackThreads = 256;
constexpr int kRepackPer = 4;  // slots per thread per chunk
constexpr int kRepackChunk = kRepackThreads * kRepackPer;
// workgroups of k_repack_rows: knob repack_grid (default 128: the fewer, the less the moves
// disturb the other range's check launch beside them -- 4.0 dB +0.6 % over 512, 32 too few)

// The decision, taken identically by every workgroup of k_repack_rows.
__device__ __forceinline__ bool repack_go(const RepackArgs &r, int &cnt, int &w, int &w_new) {
    cnt = sld(r.count);
    w = sld(r.sel + kSelW);
    if (w <= 64 || cnt <= 0 || (int64_t)cnt * 100 > (int64_t)w * r.pct) return false;
    w_new = max(64, (cnt + 63) / 64 * 64);
    return w_new < w;
}

// make every load of this thread complete, then the workgroup barrier: the loaded values are
// in registers before any thread of the workgroup overwrites what they were loaded from
__device__ __forceinline__ void loads_done_barrier() {
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
}

// Raw buffer access to a run of rows of a frame-innermost array (base in scalar registers, the
// lane's byte offset in a VGPR): an offset past the run reads 0 and drops the store, so empty slots
// need no branch.
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const T *p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(p), (short)0, bytes, 0x00020000);
}
__device__ __forceinline__ double rb_load(__amdgpu_buffer_rsrc_t r, uint32_t off, double) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
__device__ __forceinline__ uint8_t rb_load(__amdgpu_buffer_rsrc_t r, uint32_t off, uint8_t) {
    return __builtin_amdgcn_raw_buffer_load_b8(r, off, 0, 0);
}
__device__ __forceinline__ void rb_store(__amdgpu_buffer_rsrc_t r, uint32_t off, double v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(qr_u32x2, v), r, off, 0, 0);
}
__device__ __forceinline__ void rb_store(__amdgpu_buffer_rsrc_t r, uint32_t off, uint8_t v) {
    __builtin_amdgcn_raw_buffer_store_b8(v, r, off, 0, 0);
}

// Gather the columns of this thread's slots from rows [0, n) of src into dst, row groups of rg
// rows walked grid-stride by the workgroups: slot u of a group = (row j < rg of the group, one
// column); src_el / dst_el: its byte offsets inside a group of double rows (8 (j ld + column)),
// kRepackNone for an empty slot (a byte row group shifts them right by 3; an empty slot's offset
// stays past the group either way).  src and dst never alias (two column sets, or work set ->
// output), so there is no ordering to keep.
constexpr uint32_t kRepackNone = 0xFFFFFFF0u;  // past any group: loads 0, stores nothing
template <typename TS, typename TD>
__device__ __forceinline__ void gather_rows(const TS *src, TD *dst, int64_t n, int ld, int dst_ld, int rg,
                                            const uint32_t (&src_el)[kRepackPer],
                                            const uint32_t (&dst_el)[kRepackPer]) {
    constexpr int sh = sizeof(TS) == 8 ? 0 : 3;
    // two row groups per step: the loads of both are in flight together (the moves are bound by
    // the memory round trip of each step, not by bandwidth)
    const int64_t stride = (int64_t)gridDim.x * rg;
    for (int64_t g0 = (int64_t)blockIdx.x * rg; g0 < n; g0 += 2 * stride) {
        const int64_t g1 = g0 + stride;
        const int n0 = (int)min<int64_t>(rg, n - g0);                       // block-uniform
        const int n1 = g1 < n ? (int)min<int64_t>(rg, n - g1) : 0;          // (0: no second group)
        const auto s0 = make_rsrc(src + (size_t)g0 * ld, n0 * ld * (int)sizeof(TS));
        const auto d0 = make_rsrc(dst + (size_t)g0 * dst_ld, n0 * dst_ld * (int)sizeof(TD));
        const auto s1 = make_rsrc(src + (size_t)(n1 ? g1 : g0) * ld, n1 * ld * (int)sizeof(TS));
        const auto d1 = make_rsrc(dst + (size_t)(n1 ? g1 : g0) * dst_ld, n1 * dst_ld * (int)sizeof(TD));
        TS v0[kRepackPer], v1[kRepackPer];
#if QR_DEBUG_ASSERT
        // a slot lies inside a full group of rg rows (slots of rows j >= n0 in the last, short group
        // fall past the buffer's range by design: their loads read 0, their stores are dropped)
        for (int u = 0; u < kRepackPer; ++u) {
            QR_DCHECK(src_el[u] == kRepackNone || (src_el[u] >> sh) < (uint32_t)(rg * ld * (int)sizeof(TS)), kDbgRepackSlot,
                      src_el[u], n0);
            QR_DCHECK(dst_el[u] == kRepackNone || (dst_el[u] >> sh) < (uint32_t)(rg * dst_ld * (int)sizeof(TD)),
                      kDbgRepackSlot, dst_el[u], n0);
        }
#endif
#pragma unroll
        for (int u = 0; u < kRepackPer; ++u) v0[u] = rb_load(s0, src_el[u] >> sh, TS(0));
#pragma unroll
        for (int u = 0; u < kRepackPer; ++u) v1[u] = rb_load(s1, src_el[u] >> sh, TS(0));
#pragma unroll
        for (int u = 0; u < kRepackPer; ++u) rb_store(d0, dst_el[u] >> sh, v0[u]);
#pragma unroll
        for (int u = 0; u < kRepackPer; ++u) rb_store(d1, dst_el[u] >> sh, v1[u]);
    }
}

// The commit of a repack (by the workgroup of k_repack_rows that finishes last): frame ids, active
// flags and the RangeSel (now in column set nb, in transit).  The list keeps the frames' old
// columns: the transition sweeps read the messages there; the next status launch rebuilds it.
__device__ __forceinline__ void repack_commit(const RepackArgs &r, int cnt, int w, int w_new, bool on, int nb) {
    const int f0 = r.f0;
    for (int p0 = 0; p0 < cnt; p0 += kRepackThreads) {
        const int p = p0 + (int)threadIdx.x;
        int id = 0;
        if (p < cnt) {
            const int sc = r.list[f0 + p];
            id = on ? r.fid_w[sc] : sc;  // column = frame in the caller's arrays
            QR_DCHECK(sc >= f0 + p && sc < f0 + w && id >= 0 && id < r.ld, kDbgRepackFid, sc, id);
        }
        loads_done_barrier();  // fid_w is compacted in place: every read of this chunk first
        if (p < cnt) {
            r.fid_w[f0 + p] = id;
            r.active[f0 + p] = 1;
        }
    }
    for (int p = cnt + (int)threadIdx.x; p < w; p += kRepackThreads) {
        r.fid_w[f0 + p] = -1;
        r.active[f0 + p] = 0;
    }
    if (threadIdx.x == 0) {
        r.sel[kSelOn] = 1;
        r.sel[kSelW] = w_new;
        r.sel[kSelRepacks] += 1;
        r.sel[kSelArrive] = 0;
        r.sel[kSelBuf] = nb;
        r.sel[kSelTransit] = 1;
    }
}

// The row moves of a repack.  Posteriors are not moved: the range's variable sweep right after
// rewrites every running frame's posterior in its new column; only the frames stopped since the
// last repack hand theirs (in the work set) to the output first.
__global__ void __launch_bounds__(kRepackThreads) k_repack_rows(RepackArgs r) {
    int cnt, w, w_new;
    // allocate 32 VGPRs (the code needs fewer): see the register note above
    __asm__ volatile("" ::: "v31");
    if (!repack_go(r, cnt, w, w_new)) return;  // kernel-uniform
    const bool on = sld(r.sel + kSelOn) != 0;
    const int b = on ? sld(r.sel + kSelBuf) : 0, nb = on ? 1 - b : 1;  // source / destination column set
    const int ld = r.ld, f0 = r.f0;
    if (on) {
        // frames stopped since the last repack (a column < w with a frame id, no longer active)
        // hand their posteriors to the output: slots (row j of rg, column q < w)
        const int rg = w <= kRepackChunk / 2 ? min(16, kRepackChunk / w) : 1;
        for (int q0 = 0; q0 < w; q0 += kRepackChunk) {
            const int qc = min(w - q0, kRepackChunk);
            uint32_t src_el[kRepackPer], dst_el[kRepackPer];
#pragma unroll
            for (int u = 0; u < kRepackPer; ++u) {
                const int sl = u * kRepackThreads + (int)threadIdx.x;
                const int j = sl / qc, q = q0 + sl - j * qc;
                const int id = j < rg ? r.fid_w[f0 + q] : -1;
                const bool go = id >= 0 && !r.active[f0 + q];
                QR_DCHECK(id < ld, kDbgRepackFid, id, q);
                src_el[u] = go ? (uint32_t)(j * ld + f0 + q) * 8u : kRepackNone;
                dst_el[u] = go ? (uint32_t)(j * ld + id) * 8u : kRepackNone;
            }
            gather_rows<double, double>(r.post_w, r.out_post, r.V, ld, ld, rg, src_el, dst_el);
        }
    }
    // a small count moves several rows per group: rg rows x cnt columns fill the slots
    const int rg = cnt <= kRepackChunk / 2 ? min(16, kRepackChunk / cnt) : 1;
    for (int p0 = 0; p0 < cnt; p0 += kRepackChunk) {
        const int pc = min(cnt - p0, kRepackChunk);  // columns of this chunk (rg = 1 unless one chunk)
        uint32_t src_el[kRepackPer], dst_el[kRepackPer];
#pragma unroll
        for (int u = 0; u < kRepackPer; ++u) {
            const int sl = u * kRepackThreads + (int)threadIdx.x;
            const int j = sl / pc, q = sl - j * pc;
            const bool ok = j < rg;
            QR_DCHECK(!ok || (r.list[f0 + p0 + q] >= f0 + p0 + q && r.list[f0 + p0 + q] < f0 + w), kDbgRepackList,
                      r.list[f0 + p0 + q], f0 + p0 + q);
            src_el[u] = ok ? (uint32_t)(j * ld + r.list[f0 + p0 + q]) * 8u : kRepackNone;
            dst_el[u] = ok ? (uint32_t)(j * ld + f0 + p0 + q) * 8u : kRepackNone;
        }
        // source set b, destination set nb (selects, not dynamic indices into the kernel arguments);
        // the messages are not moved here: the transition sweeps read them at the old columns
        gather_rows<double, double>(!on ? r.lappr_in : b ? r.lappr_w[1] : r.lappr_w[0], nb ? r.lappr_w[1] : r.lappr_w[0],
                                    r.V, ld, ld, rg, src_el, dst_el);
        gather_rows<uint8_t, uint8_t>(!on ? r.synd_in : b ? r.synd_w[1] : r.synd_w[0], nb ? r.synd_w[1] : r.synd_w[0],
                                      r.C, ld, ld, rg, src_el, dst_el);
    }
    // the workgroup that arrives last commits: every other one has read the list, frame ids and
    // active flags it needed (its loads completed before its arrival), so the commit's rewrites of
    // them race with nothing; the next launches see everything (kernel boundary)
    __shared__ int last;
    loads_done_barrier();
    if (threadIdx.x == 0) last = atomicAdd(r.sel + kSelArrive, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (last) repack_commit(r, cnt, w, w_new, on, nb);
}


// The range's final width is known only here, so the work is (row, 64-column chunk) units, one
// per wave, walked grid-stride by every wave of the grid: a narrow range (the usual end of a
// converging one) still gets the whole grid (one unit per wave, rows in parallel).
__global__ void __launch_bounds__(256) k_repack_output(int64_t rows, int f0, int ld, const int32_t *sel,
                                                       const int32_t *__restrict__ fid_w,
                                                       const double *__restrict__ post_w, double *__restrict__ out_post) {
    if (!sld(sel + kSelOn)) return;  // kernel-uniform: never repacked (the output is the posteriors)
    const int w = sld(sel + kSelW);
    const int nq = (w + 63) >> 6;
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6), units = rows * nq;
    for (int64_t u = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); u < units; u += nwaves) {
        const int64_t v = u / nq;
        const int q = (int)(u - v * nq) * 64 + lane;
        const int id = q < w ? fid_w[f0 + q] : -1;
        if (id < 0) continue;
        QR_DCHECK(id < ld, kDbgRepackFid, id, q);
        out_post[(size_t)v * ld + id] = post_w[(size_t)v * ld + f0 + q];
    }
}

int launch_repack_rows(const RepackArgs &r, unsigned grid, hipStream_t s) {
    k_repack_rows<<<grid, kRepackThreads, 0, s>>>(r);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int launch_repack_output(int64_t rows, int f0, int ld, const int32_t *sel, const int32_t *fid_w, const double *post_w,
                         double *out_post, unsigned grid, hipStream_t s) {
    k_repack_output<<<grid, 256, 0, s>>>(rows, f0, ld, sel, fid_w, post_w, out_post);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

}  // namespace qr
