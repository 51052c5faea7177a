// decode_layered.hip -- the layered (serial-check) sum-product schedule for gfx950.
//
// The flooding decode (decoder.hip; decoder.pyx:391-436) updates every posterior after a whole
// check sweep.  Here the posteriors are updated after every check, so the later checks of an
// iteration already see the earlier checks' messages: the same box-plus and the same F/B
// recursion (decoder.pyx:322-369, :41-45), about half the iterations.  The reference has no such
// schedule; this library defines it (include/qamr.h qr_decode_layered_device) and the results are
// bit-exact against that definition.  All arithmetic is IEEE fp64, unfused, glibc exp/log.
// Per frame:
//
//   if check_lappr(lappr, synd): return (1, 0, copy of lappr)               decoder.pyx:400-405
//   post[v] = lappr[v] + 0.0 for every v with an edge, lappr[v] otherwise   the flooding init sweep
//   c2v[e] = 0.0
//   for it in 0 .. max_iterations-1:
//       for c in schedule order:
//           edges e_0..e_{d-1} of c in ascending edge id, variables v_i
//           old_i = c2v[e_i];  m_i = post[v_i] - old_i                      all i, before any write
//           new_0..new_{d-1} = the reference's check rule on m with the syndrome sign
//           for i ascending:  post[v_i] = (post[v_i] - old_i) + new_i;  c2v[e_i] = new_i
//       if check_lappr(post, synd): return (1, it+1, post)                  decoder.pyx:431-433
//   return (0, max_iterations, post)
//
// post[v_i] in the update line is read again: where v_i occurs once in the check it equals m_i
// bit for bit and the kernel reuses m_i; where a check holds a variable twice (parallel edges:
// qr_code::d_chk_repeat, wave-uniform) the second edge reads what the first left.
//
// Schedule order: (layer_of[c], c), the layers first-fit in ascending check id (host_build.hpp
// build_layers).  The checks of one layer share no variable, so they run in any order with the
// same bits: one launch per non-empty (layer, check degree), enqueued in schedule order on the
// caller's stream; the kernel boundary is the only synchronisation between layers.  A lane is one
// (check, frame) in the frame-innermost layout [n][ld] as in k_check (decoder.hip): a wave is one
// check x 64 frames.  Waves whose 64 frames have all stopped leave; stopped lanes of a live wave
// run along and store no posterior (and, past the first iteration, no message).  The posteriors live in the caller's output, updated in place; the
// messages in c2v [E][ld] of the workspace.  The first iteration reads no message (old_i = 0.0:
// x - 0.0 == x for every x), so c2v needs no clearing and a frame's messages are all written by
// its first iteration before its second reads them.  After the last layer of an iteration a
// parity-only sweep over the posteriors (the flooding decode's, kParityOnly) and the status
// launch (k_status) stop the frames whose posteriors satisfy the syndrome.
//
// What bounds it: an iteration is one launch per (layer, degree) instead of one per degree, each
// over 1 / layers of the checks, so small codes and small batches are launch-bound; the box-plus
// arithmetic per check is the flooding sweep's.
#include "debug_check.hpp"
#include "decode_dev.hpp"
#include "decode_host.hpp"

namespace qr {

struct LayerArgs {
    const int32_t *checks;  // the (layer, degree) segment's check ids, ascending
    int64_t n_checks;
    const int32_t *chk_ptr, *chk_edge, *chk_var;
    const uint8_t *repeat;  // per check: 1 iff it holds a variable more than once
    double *post;
    double *c2v;
    const uint8_t *synd;
    const uint8_t *active;
    int ld;
    Geom g;
    const GlibcTables *gglibc;
    int64_t V, E, C;  // the debug build's bounds
};

// new_0..new_{D-1} before the syndrome sign.  D <= kPackMaxDeg: the packed strict update with the
// clamp valid for any input; above, F[i] = bp(F[i-1], m[i]) and the backward values consumed as
// they are produced, the operands of decoder.pyx:341-367 in their order (check_exact, decoder.hip).
template <int D>
__device__ __forceinline__ void layer_rule(const double (&m)[D], double (&out)[D], double *hb,
                                           const GlibcTablesBP &tab, const GlibcK &K) {
    if constexpr (kPacked<D>) {
        check_strict_packed<D, kClampFull>(m, out, hb + (threadIdx.x >> 6) * kPackWaveDoubles, tab, K);
    } else {
        double F[D - 1];
        F[0] = m[0];
#pragma unroll
        for (int i = 1; i < D - 1; ++i) F[i] = box_plus_strict(F[i - 1], m[i], tab, K);
        out[D - 1] = F[D - 2];
        double Bn = m[D - 1];
#pragma unroll
        for (int i = D - 2; i > 0; --i) {
            out[i] = box_plus_strict(F[i - 1], Bn, tab, K);
            Bn = box_plus_strict(Bn, m[i], tab, K);
        }
        out[0] = Bn;
    }
}

// One lane = one (check, frame); each thread walks `per` checks of the segment.  FIRST: the first
// iteration (every message is 0.0 and is not read).
template <int D, bool FIRST>
__global__ void __launch_bounds__(256) k_layer_check(LayerArgs a) {
    __shared__ GlibcTablesBP tab;
    __shared__ double hb[kPacked<D> ? kPackLdsDoubles : 1];
    stage_glibc_tables(&tab, a.gglibc);
    const int ft = 1 << a.g.lft;
    const int nsub = 256 >> a.g.lft;
    const int ld = a.ld;
    const int f = (int)(blockIdx.y << a.g.lft) + (int)(threadIdx.x & (ft - 1));
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> a.g.lft);
    QR_DCHECK(f >= 0 && f < ld, kDbgLayFrame, f, ld);
    const bool act = a.active[f] != 0;
    if (!wave_any(act)) return;  // no barrier follows: the packed update exchanges within the wave
    const auto K = GlibcK::pinned();
    const uint32_t b8 = (uint32_t)f * 8u;
    int64_t ci = (int64_t)blockIdx.x * a.g.per * nsub + sub;
    for (int j = 0; j < a.g.per && ci < a.n_checks; ++j, ci += nsub) {  // wave-uniform
        const int cc = sld(a.checks + ci);
        const int base = sld(a.chk_ptr + cc);
        QR_DCHECK(cc >= 0 && cc < a.C && sld(a.chk_ptr + cc + 1) - base == D, kDbgLayCheck, cc, base);
        QR_DCHECK(base >= 0 && base + D <= a.E, kDbgLayEdge, base, a.E);
        const uint8_t sb = *at_byte(row_ptr(a.synd, cc, ld), (uint32_t)f);
        double m[D], out[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int v = sld(a.chk_var + base + i), e = sld(a.chk_edge + base + i);
            QR_DCHECK(v >= 0 && v < a.V, kDbgLayVar, v, a.V);
            QR_DCHECK(e >= 0 && e < a.E, kDbgLayEdge, e, a.E);
            const double p = ld_row<false>(row_ptr(a.post, v, ld), b8, ld);
            if constexpr (FIRST) m[i] = p;  // p - 0.0 == p
            else m[i] = p - ld_row<false>(row_ptr(a.c2v, e, ld), b8, ld);
        }
        layer_rule<D>(m, out, hb, tab, K);
        const uint32_t smask = sign_mask(sb);
        // A stopped lane of a live wave stores no posterior.  In the first iteration it does store
        // its messages (into the workspace only): the later iterations' loads of that lane then read
        // what this call wrote, whatever the workspace held on entry.
        const bool wr_msg = FIRST || act;
        if (!sld(a.repeat + cc)) {  // wave-uniform; every v_i once: post[v_i] still holds p_i, p_i - old_i == m_i
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double o = apply_sign(out[i], smask);
                if (act) st_row<false>(row_ptr(a.post, sld(a.chk_var + base + i), ld), b8, ld, m[i] + o);
                if (wr_msg) st_row<false>(row_ptr(a.c2v, sld(a.chk_edge + base + i), ld), b8, ld, o);
            }
        } else {
            // a variable twice: in ascending edge order, the posterior read again (plain accesses:
            // each load follows the lane's own store to the same address in program order)
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double o = apply_sign(out[i], smask);
                double *const pp = a.post + (size_t)sld(a.chk_var + base + i) * (size_t)ld + f;
                double *const cp = a.c2v + (size_t)sld(a.chk_edge + base + i) * (size_t)ld + f;
                if (act) {
                    const double old = FIRST ? 0.0 : *cp;
                    *pp = (*pp - old) + o;
                }
                if (wr_msg) *cp = o;
            }
        }
    }
}

// ------------------------------------------------------------------ workspace and launch
struct LayeredWs {
    double *c2v;
    uint8_t *active;
    uint8_t *unsat;   // one row of ld flags per syndrome test: iterations 0..max_it, plus one
    int32_t *counts;  // the 256-byte count block of k_init_status
    size_t bytes;
};
static LayeredWs layered_layout(const qr_code *code, int ld, int max_it, void *base = nullptr) {
    LayeredWs w;
    Cursor c{(uintptr_t)base};
    w.c2v = c.take<double>((size_t)code->E * ld);
    w.active = c.take<uint8_t>((size_t)ld);
    w.unsat = c.take<uint8_t>((size_t)unsat_rows(max_it) * ld);
    w.counts = c.take<int32_t>(64);
    w.bytes = c.off;
    return w;
}
size_t layered_ws_bytes(const qr_code *code, int ld, int max_it) { return layered_layout(code, ld, max_it).bytes; }

template <bool FIRST>
static int launch_layer(const qr_code *code, const LayerSegDev &g, const LayeredWs &w, int ld, const uint8_t *synd,
                        double *post, hipStream_t s) {
    LayerArgs a;
    a.checks = code->d_layer_checks + g.off;
    a.n_checks = g.n;
    a.chk_ptr = code->d_chk_ptr;
    a.chk_edge = code->d_chk_edge;
    a.chk_var = code->d_chk_var;
    a.repeat = code->d_chk_repeat;
    a.post = post;
    a.c2v = w.c2v;
    a.synd = synd;
    a.active = w.active;
    a.ld = ld;
    a.g = make_geom(ld, g_tune.check_ft.load(), g_tune.check_per.load(), g.n);
    a.gglibc = code->d_gtab;
    a.V = code->V;
    a.E = code->E;
    a.C = code->C;
    const int64_t per_block = (int64_t)a.g.per * (256 >> a.g.lft);
    const dim3 grid((unsigned)((g.n + per_block - 1) / per_block), (unsigned)(ld >> a.g.lft));
    ProfScope pa("layer_check", s);
    ProfScope pd(profiling_on() ? "layer_check_d" + std::to_string(g.degree) : std::string(), s);
    const bool handled = dispatch_degree<2, kMaxTemplDeg>(
        g.degree, [&](auto d) { k_layer_check<d.value, FIRST><<<grid, 256, 0, s>>>(a); });
    if (!handled) return set_error(QR_EINTERNAL, "layered decode: no kernel for check degree %d", g.degree);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

int decode_layered_device(const qr_code *code, int B, int ld, const double *lappr, const uint8_t *synd, int max_it,
                          double *final_post, uint8_t *success, int32_t *iters, void *ws_ptr, size_t ws_size,
                          hipStream_t s) {
    if (B <= 0 || ld < B || ld % kWave)
        return set_error(QR_EVALUE, "layered decode: need 0 < B <= ld and ld %% 64 == 0 (B=%d, ld=%d)", B, ld);
    if (max_it < 0) return set_error(QR_EVALUE, "layered decode: max_iterations must not be negative (%d)", max_it);
    if (!lappr || !synd || !final_post || !success || !iters || !ws_ptr)
        return set_error(QR_EVALUE, "layered decode: null pointer argument");
    if (!ws_aligned(ws_ptr)) return set_error(QR_EVALUE, "layered decode: workspace must be 256-byte aligned");
    if (code->max_dc > kMaxTemplDeg)
        return set_error(QR_EUNSUPPORTED, "layered decode: check degree %d above %d", code->max_dc, kMaxTemplDeg);
    const LayeredWs w = layered_layout(code, ld, max_it, ws_ptr);
    if (ws_size < w.bytes)
        return set_error(QR_EVALUE, "layered decode: workspace too small (%zu < %zu)", ws_size, w.bytes);
    DeviceGuard dg(code->device);
    int rc;
    auto row = [&](int t) { return w.unsat + (size_t)t * ld; };
    auto status = [&](int t, int final_call) {
        return launch_status(0, B, t, final_call, max_it, row(t), w.active, success, iters, nullptr, nullptr, s);
    };
    QR_HIP(hipMemsetAsync(w.unsat, 0, (size_t)unsat_rows(max_it) * ld, s));
    if ((rc = launch_init_status(B, ld, w.active, success, iters, w.counts + 2, w.counts + 4, ld / 2, ld - ld / 2, s)))
        return rc;
    // decoder.pyx:400-405: the input itself may already satisfy the syndrome; then the init sweep
    if ((rc = launch_parity_sweep(code, B, ld, lappr, synd, w.active, row(0), w.counts, s))) return rc;
    if ((rc = status(0, 0))) return rc;
    if ((rc = launch_var_init(code, B, ld, lappr, final_post, w.active, w.counts, s))) return rc;
    if (max_it == 0) {  // no iteration, no test: every frame still running ends with (0, 0)
        QR_HIP(hipMemsetAsync(row(0), 1, (size_t)ld, s));
        return status(0, 1);
    }
    for (int t = 1; t <= max_it; ++t) {
        for (const LayerSegDev &g : code->layer_segs) {
            rc = t == 1 ? launch_layer<true>(code, g, w, ld, synd, final_post, s)
                        : launch_layer<false>(code, g, w, ld, synd, final_post, s);
            if (rc) return rc;
        }
        {
            ProfScope ps("layer_parity", s);
            if ((rc = launch_parity_sweep(code, B, ld, final_post, synd, w.active, row(t), w.counts, s))) return rc;
        }
        // satisfied -> (1, t); after the last iteration every frame still running -> (0, max_it)
        if ((rc = status(t, t == max_it))) return rc;
    }
    return QR_OK;
}

}  // namespace qr
