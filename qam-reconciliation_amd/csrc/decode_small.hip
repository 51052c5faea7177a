// decode_small.hip -- the two decode schedules of small codes (decode_batch_device, decoder.hip,
// routes to them): one launch per iteration (k_iter, run_iter) and one launch per decode with a
// workgroup per frame and its messages in LDS (k_resident, run_resident).
#include "debug_check.hpp"
#include "decode_dev.hpp"
#include "decode_host.hpp"

namespace qr {

// Small codes (configs[1], reg-(3,6) N=1008): ONE launch per iteration.  A sweep of such a
// code is a few microseconds of chip work, so the three launches of the flat schedule
// (check, status, variable) are dominated by dispatch and drain.  Here the check sweep
// computes the posteriors it needs itself, from the previous iteration's messages:
//   post(t-1)[v] = lappr[v] + c2v(t-1)[e_0] + c2v(t-1)[e_1] + ...   (ascending edge id,
//                  decoder.pyx:292-293 -- the same additions, so the same bits)
// and the check whose edge is v's first edge stores it (the decoder's output), so no
// variable sweep is needed.  The messages are double-buffered by iteration parity (a check
// of iteration t reads c2v(t-1) of edges other checks are rewriting).  Launch P(t):
//   * status of iteration t-2 (t >= 3): frames whose post(t-2) satisfied the syndrome stop
//     with (1, t-2); the check of index 0 of each frame writes it, every lane derives the
//     same running flag act = active && unsat(t-2) (so the write races benignly);
//   * post(t-1) on the fly, its parity (unsat(t-1), t >= 2), c2v(t) (t <= max_it).
// Per frame the order is the reference's: check(t) -> status(t-1) -> var(t) -> check(t+1);
// P(max_it + 1) is the final parity sweep.  Used for single-degree-class codes with D <= 10
// when the two-stream schedule does not pay (knob fused_iter).
struct IterArgs {
    const int32_t *checks;
    int64_t n_checks;
    const int32_t *chk_ptr, *chk_edge, *chk_var, *var_ptr, *var_edge;
    const double *lappr;
    double *post;
    const double *c2v_in;  // c2v(t-1), or null at t = 1 (all messages 0)
    double *c2v_out;       // c2v(t), or null in the final parity sweep
    const uint8_t *synd;
    uint8_t *active, *success;
    int32_t *iters;
    const uint8_t *unsat_s;  // row t-2 (status to apply), or null
    uint8_t *unsat_p;        // row t-1 (parity of post(t-1)), or null at t = 1
    int32_t status_iter;     // t - 2
    int ld, f_off;           // the launch sweeps frames [f_off, f_off + gridDim.y * ft)
    Geom g;
    unsigned nbx;
    const GlibcTables *gglibc;
    const int32_t *finite;
};

// Every access is cached (no non-temporal hint): a small code's messages, posteriors and LAPPRs
// are re-read every iteration from L2 / MALL.
template <int D, bool FIN>
__device__ __forceinline__ void iter_block(const IterArgs &a, unsigned bx, unsigned by, const GlibcTablesBP &tab,
                                           double *hb) {
    const int ft = 1 << a.g.lft;
    const int nsub = 256 >> a.g.lft;
    const int ld = a.ld;
    const int f = a.f_off + (int)(by << a.g.lft) + (threadIdx.x & (ft - 1));
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> a.g.lft);
    const bool was = a.active[f] != 0;
    const bool act = was && (!a.unsat_s || a.unsat_s[f] != 0);
    int64_t ci = (int64_t)bx * a.g.per * nsub + sub;
    if (ci == 0 && was && !act) {  // decoder.pyx:431-433 for iteration t-2
        a.success[f] = 1;
        a.iters[f] = a.status_iter;
        a.active[f] = 0;
    }
    if (!wave_any(act)) return;
    const auto K = GlibcK::pinned();
    const uint32_t b8 = (uint32_t)f * 8u;
    uint32_t bad = 0;
    for (int j = 0; j < a.g.per; ++j, ci += nsub) {
        if (ci >= a.n_checks) break;
        const int cc = sld(a.checks + ci);
        const int base = sld(a.chk_ptr + cc);
        uint32_t par = *at_byte(row_ptr(a.synd, cc, ld), (uint32_t)f);
        double m[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int v = sld(a.chk_var + base + i), e = sld(a.chk_edge + base + i);
            const int vb = sld(a.var_ptr + v), ve = sld(a.var_ptr + v + 1);
            double p = ld_row<false>(row_ptr(a.lappr, v, ld), b8, ld);
            double own = 0.0;
            for (int k = vb; k < ve; ++k) {  // decoder.pyx:292-293, ascending edge id
                const int ek = sld(a.var_edge + k);
                const double c = a.c2v_in ? ld_row<false>(row_ptr(a.c2v_in, ek, ld), b8, ld) : 0.0;
                p += c;
                own = (ek == e) ? c : own;
            }
            if (act && sld(a.var_edge + vb) == e) st_row<false>(row_ptr(a.post, v, ld), b8, ld, p);
            par ^= (p < 0.0) ? 1u : 0u;  // decoder.pyx:243-246
            m[i] = p - own;              // :296-297
        }
        bad |= (par == 1u) ? 1u : 0u;
        if (a.c2v_out) {
            const double s = *at_byte(row_ptr(a.synd, cc, ld), (uint32_t)f) ? -1.0 : 1.0;
            double out[D];
            double *wb = hb + (threadIdx.x >> 6) * kPackWaveDoubles;
            check_strict_packed<D, FIN ? kClampFinite : kClampFull>(m, out, wb, tab, K);
#pragma unroll
            for (int i = 0; i < D; ++i)
                if (act) st_row<false>(row_ptr(a.c2v_out, sld(a.chk_edge + base + i), ld), b8, ld, s * out[i]);
        }
    }
    if (a.unsat_p && bad && act) a.unsat_p[f] = 1;  // benign race: every writer stores 1
}

template <int D>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 8))) k_iter(IterArgs a) {
    __shared__ GlibcTablesBP tab;
    __shared__ double hb[4 * kPackWaveDoubles];
    if (a.c2v_out) stage_glibc_tables(&tab, a.gglibc);
    if (a.finite && sld(a.finite)) iter_block<D, true>(a, blockIdx.x, blockIdx.y, tab, hb);
    else iter_block<D, false>(a, blockIdx.x, blockIdx.y, tab, hb);
}

// ---------------------------------------------------------------------------------------
// Small codes, frame-resident (knob resident, default 1): ONE launch per decode, one
// workgroup per frame for all its iterations, the frame's messages and posteriors in LDS
// (configs[1], reg-(3,6) N=1008: 24 KiB of c2v + 8 KiB of posteriors).  Lane = check in the
// check phase (check c's messages at slots D c .. D c + D - 1: single-degree codes only) and
// lane = variable in the variable phase; each message and posterior is the same operation on
// the same operands as in the frame-parallel kernels (only which lane evaluates it changes),
// so the bits are the reference's.  Per frame the order is decoder.pyx:400-436's:
//   post(0) = lappr (+ 0.0 on connected variables), parity -> stop with (1, 0) and the input;
//   t = 1..max_it: check phase c2v(t) from post(t-1) (+ parity of post(t-1) for t >= 2 ->
//   stop with (1, t-1) and post(t-1)); variable phase post(t) = lappr + sum c2v(t) in
//   ascending edge order;  then parity of post(max_it) -> (1 or 0, max_it).
// A frame stops on its own iteration (no lock-step), no per-iteration launch, no HBM
// traffic for the messages.  In LDS message (c, i) lives at i C + c, so the lanes of a check
// phase (consecutive checks) touch consecutive doubles.  Workgroup b takes frame (b % 8) ceil(B / 8) + b / 8, so the frames
// of one XCD are contiguous columns and their LAPPR sectors stay in that XCD's L2.
constexpr int kResThreads = 512;
constexpr int kResMaxIter = 10000;  // one launch runs every iteration: bound its length
constexpr int kResStaticLds = (int)sizeof(GlibcTablesBP) + (kResThreads / 64) * kPackWaveDoubles * 8;

struct ResArgs {
    int C, V, B, ld, max_it;
    const int32_t *chk_var;              // check CSR: check c's variables at D c .. D c + D - 1
    const int32_t *var_ptr, *var_msg;    // per variable, its edges (ascending) as LDS message indices
    const double *lappr;
    const uint8_t *synd;
    double *post;
    uint8_t *success;
    int32_t *iters;
    const GlibcTables *gglibc;
    double fin_bound;  // |lappr| below it for every variable -> the finite clamp (0: never)
    int dv;            // every variable of degree dv <= 3 and E < 2^16 (0: otherwise)
    int32_t *rsel;     // the workspace's RangeSel block: reset to "never repacked" (repack stats)
    int w0, w1;        // its initial widths
};

// parity of the posteriors in LDS (decoder.pyx:235-257): 1 iff some check of this thread fails
template <int D>
__device__ __forceinline__ uint32_t res_parity(const ResArgs &a, int f, const double *post) {
    uint32_t bad = 0;
    for (int c = threadIdx.x; c < a.C; c += kResThreads) {
        uint32_t par = a.synd[(size_t)c * a.ld + f];
#pragma unroll
        for (int i = 0; i < D; ++i) par ^= (post[a.chk_var[c * D + i]] < 0.0) ? 1u : 0u;
        bad |= (par == 1u) ? 1u : 0u;
    }
    return bad;
}

__device__ __forceinline__ void res_finish(const ResArgs &a, int f, const double *post, int ok, int32_t it) {
    for (int v = threadIdx.x; v < a.V; v += kResThreads) a.post[(size_t)v * a.ld + f] = post[v];
    if (threadIdx.x == 0) {
        a.success[f] = (uint8_t)ok;
        a.iters[f] = it;
    }
}

template <int D, bool FIN>
__device__ __forceinline__ void resident_loop(const ResArgs &a, int f, double *msg, double *post,
                                              const GlibcTablesBP &tab, double *wb) {
    const int tid = threadIdx.x;
    const size_t ld = a.ld;
    const auto K = GlibcK::pinned();
    // the first check of this thread (all of them when C <= kResThreads): its syndrome bit stays
    // in a register across the iterations (its variable indices are re-read from L1: pinning
    // them too spilled with the variable phase's registers below, 907 k vs 911 k frames/s)
    const int c_first = min(tid, a.C - 1);
    const uint8_t sb_first = a.synd[(size_t)c_first * ld + f];
    // the LAPPRs of this lane's (at most two) variables stay in registers when V <= 2 x 512
    // (configs[1]: 1 008), instead of an L2 read per variable per iteration
    const bool lreg = a.V <= 2 * kResThreads;  // block-uniform
    const double l0 = lreg && tid < a.V ? a.lappr[(size_t)tid * ld + f] : 0.0;
    const double l1 = lreg && tid + kResThreads < a.V ? a.lappr[(size_t)(tid + kResThreads) * ld + f] : 0.0;
    // regular variable degree dv <= 3 (configs[1]: 3): the LDS message indices of those two
    // variables' edges too, two 16-bit indices per register, instead of index loads per iteration
    const int dv = lreg ? a.dv : 0;  // block-uniform
    uint32_t vm[3] = {0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (q < dv) {
            const uint32_t i0 = tid < a.V ? (uint32_t)a.var_msg[tid * dv + q] : 0u;
            const uint32_t i1 = tid + kResThreads < a.V ? (uint32_t)a.var_msg[(tid + kResThreads) * dv + q] : 0u;
            vm[q] = i0 | i1 << 16;
        }
    }
    for (int t = 1; t <= a.max_it; ++t) {
        uint32_t bad = 0;
        for (int c0 = 0; c0 < a.C; c0 += kResThreads) {
            if (c0 + (tid & ~63) >= a.C) break;  // wave-uniform: no check left for this wave
            const int c = c0 + tid;
            const bool live = c < a.C;
            const int cc = live ? c : a.C - 1;  // surplus lanes repeat the last check, store nothing
            const uint8_t sb = c0 == 0 ? sb_first : a.synd[(size_t)cc * ld + f];
            uint32_t par = sb;
            double m[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                QR_DCHECK(a.chk_var[cc * D + i] >= 0 && a.chk_var[cc * D + i] < a.V, kDbgResPost, cc, a.chk_var[cc * D + i]);
                QR_DCHECK(i * a.C + cc < a.C * D, kDbgResMsg, cc, i);
                const double p = post[a.chk_var[cc * D + i]];
                par ^= (p < 0.0) ? 1u : 0u;     // decoder.pyx:243-246
                m[i] = p - msg[i * a.C + cc];    // :296-297
            }
            if (live) bad |= (par == 1u) ? 1u : 0u;
            double out[D];
            check_strict_packed<D, FIN ? kClampFinite : kClampFull>(m, out, wb, tab, K);
            const uint32_t smask = sign_mask(sb);
            if (live) {
#pragma unroll
                for (int i = 0; i < D; ++i) msg[i * a.C + cc] = apply_sign(out[i], smask);  // only this lane reads them back
            }
        }
        // the parity of post(t-1) (t = 1: post(0), whose parity is the input's, already tested)
        const int any_bad = __syncthreads_or((int)bad);
        if (t >= 2 && !any_bad) {  // decoder.pyx:431-433 at iteration t-1
            res_finish(a, f, post, 1, t - 1);
            return;
        }
        // decoder.pyx:285-298, two variables per lane at a time: their (latency-bound, L1/L2)
        // LAPPR and index loads are issued together; each sum keeps its ascending edge order
        if (dv) {  // block-uniform: LAPPRs and message indices in registers
            double p0 = l0, p1 = l1;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (q < dv) {
                    QR_DCHECK((vm[q] & 0xFFFFu) < (uint32_t)(a.C * D) && (vm[q] >> 16) < (uint32_t)(a.C * D), kDbgResMsg,
                              vm[q] & 0xFFFFu, vm[q] >> 16);
                    const double m0 = msg[vm[q] & 0xFFFFu], m1 = msg[vm[q] >> 16];
                    p0 += m0;
                    p1 += m1;
                }
            }
            if (tid < a.V) post[tid] = p0;
            if (tid + kResThreads < a.V) post[tid + kResThreads] = p1;
        }
        for (int v0 = dv ? a.V : tid; v0 < a.V; v0 += 2 * kResThreads) {
            const int v1 = v0 + kResThreads;
            const bool two = v1 < a.V;
            const int w1 = two ? v1 : v0;
            double p0 = lreg ? l0 : a.lappr[(size_t)v0 * ld + f];
            double p1 = lreg ? l1 : a.lappr[(size_t)w1 * ld + f];
            const int b0 = a.var_ptr[v0], e0 = a.var_ptr[v0 + 1];
            const int b1 = a.var_ptr[w1], e1 = a.var_ptr[w1 + 1];
            const int n = max(e0 - b0, e1 - b1);
            for (int q = 0; q < n; ++q) {
                const bool h0 = b0 + q < e0, h1 = b1 + q < e1;
                QR_DCHECK(a.var_msg[h0 ? b0 + q : 0] < a.C * D && a.var_msg[h1 ? b1 + q : 0] < a.C * D, kDbgResMsg,
                          a.var_msg[h0 ? b0 + q : 0], a.var_msg[h1 ? b1 + q : 0]);
                const double m0 = msg[a.var_msg[h0 ? b0 + q : 0]];  // (edge 0: an in-bounds dummy)
                const double m1 = msg[a.var_msg[h1 ? b1 + q : 0]];
                if (h0) p0 += m0;
                if (h1) p1 += m1;
            }
            post[v0] = p0;
            if (two) post[v1] = p1;
        }
        __syncthreads();
    }
    const int any_bad = __syncthreads_or((int)res_parity<D>(a, f, post));
    res_finish(a, f, post, any_bad ? 0 : 1, a.max_it);  // decoder.pyx:435-436
}

// QR_EXPERIMENT_CLOCK (diagnostic builds only, see g_clk in decoder.hip): every workgroup of the
// frame-resident decode adds its shader-clock and realtime spans to g_clk_res; qr_debug_clock
// (decoder.hip) reads and clears it with the check sweep's sums.
#if QR_EXPERIMENT_CLOCK
__device__ unsigned long long g_clk_res[3];
bool resident_clock_read_clear(unsigned long long h[3]) {
    const unsigned long long z[3] = {0, 0, 0};
    return hipMemcpyFromSymbol(h, HIP_SYMBOL(g_clk_res), sizeof(z)) == hipSuccess &&
           hipMemcpyToSymbol(HIP_SYMBOL(g_clk_res), z, sizeof(z)) == hipSuccess;
}
#endif
template <int D>
__global__ void __launch_bounds__(kResThreads) __attribute__((amdgpu_waves_per_eu(4, 8))) k_resident(ResArgs a) {
    extern __shared__ double res_dyn[];
    __shared__ GlibcTablesBP tab;
    __shared__ double hb[(kResThreads / 64) * kPackWaveDoubles];
#if QR_EXPERIMENT_CLOCK
    ClkScope clk(true, g_clk_res, nullptr);  // every exit below is block-uniform
#endif
    const int q = (a.B + 7) / 8;
    const int f = (int)(blockIdx.x & 7u) * q + (int)(blockIdx.x >> 3);
    // qr_decode_repack_stats after a frame-resident decode: 0 repacks, widths ld/2 (no extra launch)
    if (blockIdx.x == 0 && threadIdx.x < 2 * kSelInts)
        a.rsel[threadIdx.x] = (threadIdx.x % kSelInts == kSelW) ? (threadIdx.x < kSelInts ? a.w0 : a.w1) : 0;
    if (f >= a.B) return;  // block-uniform
    stage_glibc_tables(&tab, a.gglibc);
    const int tid = threadIdx.x;
    const size_t ld = a.ld;
    double *msg = res_dyn, *post = res_dyn + (size_t)a.C * D;
    for (int s = tid; s < a.C * D; s += kResThreads) msg[s] = 0.0;
    bool small = true;
    for (int v = tid; v < a.V; v += kResThreads) {  // decoder.pyx:408,420-421
        const double x = a.lappr[(size_t)v * ld + f];
        small &= __builtin_fabs(x) < a.fin_bound;
        post[v] = (a.var_ptr[v + 1] > a.var_ptr[v]) ? x + 0.0 : x;
    }
    const int fin = __syncthreads_and((int)small);
    // decoder.pyx:400-405: post(0) has the input's signs (only -0.0 -> +0.0 differs)
    if (!__syncthreads_or((int)res_parity<D>(a, f, post))) {
        for (int v = tid; v < a.V; v += kResThreads) a.post[(size_t)v * ld + f] = a.lappr[(size_t)v * ld + f];
        if (tid == 0) {
            a.success[f] = 1;
            a.iters[f] = 0;
        }
        return;
    }
    double *wb = hb + (tid >> 6) * kPackWaveDoubles;
    if (fin) resident_loop<D, true>(a, f, msg, post, tab, wb);
    else resident_loop<D, false>(a, f, msg, post, tab, wb);
}

// Codes the one-launch-per-iteration schedule (k_iter) can run: one check-degree class of a
// packed degree, bounded variable degrees, and messages small enough to double-buffer.
bool iter_code(const qr_code *code, int ld) {
    return code->classes.size() == 1 && code->classes[0].degree >= 2 && code->classes[0].degree <= kPackMaxDeg &&
           code->max_dv <= 64 && (size_t)code->E * ld * sizeof(double) <= ((size_t)1 << 30);
}

// The one-launch-per-iteration schedule of small codes (k_iter): P(1) .. P(max_it + 1), the last
// one the final parity sweep.  Knob iter_streams (default 2): the frames are cut into that many
// ranges, each an independent chain of launches on its own stream (frames never depend on other
// frames), so one range's gathers overlap another range's arithmetic instead of every launch
// running a load phase then a compute phase.
int run_iter(const IterRun &P, int max_it) {
    const DegreeClass &cls = P.code->classes[0];
    const int ld = P.ld;
    IterArgs a;
    a.checks = cls.d_checks;
    a.n_checks = cls.n;
    a.chk_ptr = P.code->d_chk_ptr;
    a.chk_edge = P.code->d_chk_edge;
    a.chk_var = P.code->d_chk_var;
    a.var_ptr = P.code->d_var_ptr;
    a.var_edge = P.code->d_var_edge;
    a.lappr = P.lappr;
    a.post = P.post;
    a.synd = P.synd;
    a.active = P.active;
    a.success = P.success;
    a.iters = P.iters;
    a.ld = ld;
    // 64-frame tiles (MI355X, configs[1]: 42.3 vs 43.3 us per iteration at 128)
    a.g = make_geom(ld, std::min(64, g_tune.check_ft.load()), g_tune.check_per.load(), cls.n);
    const int64_t per_block = (int64_t)a.g.per * (256 >> a.g.lft);
    a.nbx = (unsigned)((cls.n + per_block - 1) / per_block);
    a.gglibc = P.code->d_gtab;
    a.finite = P.acount + 2;
    double *buf[2] = {P.c2v, P.c2v2};
    const int tiles = ld >> a.g.lft;
    const int nst = std::max(1, std::min({g_tune.iter_streams.load(), 2, tiles}));
    const qr_code *code = P.code;
    std::unique_lock<std::mutex> lk(code->mu, std::defer_lock);
    hipStream_t st[2] = {P.s, P.s};
    if (nst == 2) {
        lk.lock();
        if (int rc0 = side_stream(code, &st[1])) return rc0;
        QR_HIP(hipEventRecord(code->ev[0], P.s));
        QR_HIP(hipStreamWaitEvent(st[1], code->ev[0], 0));
    }
    // enqueue order interleaves the ranges; each stream runs its own chain
    for (int t = 1; t <= max_it + 1; ++t) {
        a.c2v_in = t == 1 ? nullptr : buf[(t - 1) & 1];
        a.c2v_out = t <= max_it ? buf[t & 1] : nullptr;
        a.unsat_s = t >= 3 ? P.unsat + (size_t)(t - 2) * ld : nullptr;
        a.unsat_p = t >= 2 ? P.unsat + (size_t)(t - 1) * ld : nullptr;
        a.status_iter = t - 2;
        for (int r = 0; r < nst; ++r) {
            const int t0 = tiles * r / nst, t1 = tiles * (r + 1) / nst;
            a.f_off = t0 << a.g.lft;
            const dim3 grid(a.nbx, (unsigned)(t1 - t0));
            ProfScope ps(profiling_on() ? "iter_d" + std::to_string(cls.degree) : std::string(), st[r]);
            const bool handled = dispatch_degree<2, kPackMaxDeg>(
                cls.degree, [&](auto d) { k_iter<d.value><<<grid, 256, 0, st[r]>>>(a); });
            if (!handled) return set_error(QR_EVALUE, "decode: no fused-iteration kernel for degree %d", cls.degree);
            QR_LAUNCH_CHECK();
        }
    }
    if (nst == 2) {  // join: the final status follows both chains
        QR_HIP(hipEventRecord(code->ev[4], st[1]));
        QR_HIP(hipStreamWaitEvent(P.s, code->ev[4], 0));
    }
    return QR_OK;
}

// The frame-resident decode (k_resident) runs a code whose messages and posteriors fit two
// workgroups' LDS per CU (so 16 waves of <= 128 VGPRs per CU) under the strict arithmetic.
static size_t resident_lds(const qr_code *code) { return (size_t)(code->E + code->V) * sizeof(double); }
static bool resident_code(const qr_code *code) {
    // 80 KiB keeps two workgroups per gfx950 CU (160 KiB); never more than the device lets a
    // workgroup take (otherwise the fused-iteration or flat schedule runs the code)
    const size_t lds_cap = std::min<size_t>(80 * 1024, code->lds_per_block);
    return g_tune.resident.load() && code->classes.size() == 1 &&
           code->classes[0].degree >= 2 && code->classes[0].degree <= kPackMaxDeg &&
           code->classes[0].n == code->C && code->C <= INT32_MAX / kPackMaxDeg && code->V < INT32_MAX &&
           resident_lds(code) + kResStaticLds <= lds_cap;
}

int run_resident(const qr_code *code, int B, int ld, const double *lappr, const uint8_t *synd, int max_it,
                 double *final_post, uint8_t *success, int32_t *iters, int32_t *rsel, hipStream_t s) {
    ResArgs a;
    a.rsel = rsel;
    a.w0 = ld / 2;
    a.w1 = ld - ld / 2;
    a.C = (int)code->C;
    a.V = (int)code->V;
    a.B = B;
    a.ld = ld;
    a.max_it = max_it;
    a.chk_var = code->d_chk_var;
    a.var_ptr = code->d_var_ptr;
    a.var_msg = code->d_var_msg;
    a.lappr = lappr;
    a.synd = synd;
    a.post = final_post;
    a.success = success;
    a.iters = iters;
    a.gglibc = code->d_gtab;
    a.fin_bound = finite_bound(max_it, code->max_dv);
    a.dv = code->reg_dv >= 1 && code->reg_dv <= 3 && code->E < 65536 ? code->reg_dv : 0;
    const unsigned grid = (unsigned)(8 * ((B + 7) / 8));
    const size_t lds = resident_lds(code);
    ProfScope ps(profiling_on() ? "resident_d" + std::to_string(code->classes[0].degree) : std::string(), s);
    const bool handled = dispatch_degree<2, kPackMaxDeg>(
        code->classes[0].degree, [&](auto d) { k_resident<d.value><<<grid, kResThreads, lds, s>>>(a); });
    if (!handled) return set_error(QR_EVALUE, "decode: no frame-resident kernel for degree %d", code->classes[0].degree);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

// decode_batch_device runs this decode frame-resident (k_resident)
bool takes_resident(const qr_code *code, int max_it) {
    return max_it > 0 && max_it <= kResMaxIter && resident_code(code);
}

}  // namespace qr
