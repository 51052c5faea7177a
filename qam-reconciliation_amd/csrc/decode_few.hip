// decode_few.hip -- the few-frame decode schedule (k_few_check, k_few_var, run_few: a lane per
// check / variable of one frame) and the frame-major decode that routes to it or, through a
// transpose, to decode_batch_device (decoder.hip).
#include "debug_check.hpp"
#include "decode_dev.hpp"
#include "decode_host.hpp"

namespace qr {

// Few frames (qr_decode_frames_device with B <= knob few_max; Decoder.decode's one frame): the
// frame-parallel sweeps give every check a wave of 64 frames, so a single frame keeps 1 lane of
// 64 busy, and k_resident takes only single-class codes whose messages fit LDS.  Here the
// arithmetic of k_resident's loop body is cut at its barriers into launches: a lane is one check
// (k_few_check) or one variable (k_few_var) of the frame blockIdx.y, messages and posteriors
// live in HBM, frame-major -- posteriors post[f][v] (the caller's output array), messages
// msg[f][slot] with the slots of host_build.hpp build_few_layout (class k: base_k + i n_k + j,
// so a wave's lanes read consecutive doubles for each edge position i) -- and a code may have
// several degree classes, one check launch per class (the degree is then uniform per launch,
// as the packed update needs it per wave).  Each message and posterior is the same operation on
// the same operands as in the frame-parallel kernels, so the bits are the reference's.  The
// launch boundary is the only synchronisation: no workgroup waits for another.
constexpr int kFewThreads = 256;

struct FewCheckArgs {
    const int32_t *checks;  // the class's check ids, ascending
    int n;                  // its checks
    int64_t base;           // its first message slot
    int64_t E, V, C;
    const int32_t *chk_ptr, *chk_var;
    const double *post;  // [B][V]
    double *msg;         // [B][E]
    const uint8_t *synd;  // [B][C]
    const uint8_t *active;
    uint8_t *unsat;
    const int32_t *finite;  // as CheckArgs
    const GlibcTables *gglibc;
};

// decoder.pyx:322-369 for the lane's check, the D messages handed to store(i, c2v_i) with the
// syndrome sign applied: the packed update for D <= kPackMaxDeg, otherwise the F/B recursion as in
// check_exact (decoder.hip).
template <int D, bool FIN, class ST>
__device__ __forceinline__ void few_update(const double (&m)[D], uint32_t smask, double *wb, const GlibcTablesBP &tab,
                                           const GlibcK &K, ST store) {
    if constexpr (kPacked<D>) {
        double out[D];
        check_strict_packed<D, FIN ? kClampFinite : kClampFull>(m, out, wb, tab, K);
#pragma unroll
        for (int i = 0; i < D; ++i) store(i, apply_sign(out[i], smask));
    } else {
        double F[D - 1];
        F[0] = m[0];
#pragma unroll
        for (int i = 1; i < D - 1; ++i) F[i] = box_plus_strict(F[i - 1], m[i], tab, K);
        store(D - 1, apply_sign(F[D - 2], smask));
        double Bn = m[D - 1];
#pragma unroll
        for (int i = D - 2; i > 0; --i) {
            store(i, apply_sign(box_plus_strict(F[i - 1], Bn, tab, K), smask));
            Bn = box_plus_strict(Bn, m[i], tab, K);
        }
        store(0, apply_sign(Bn, smask));
    }
}

template <int D, int MODE, bool FIN>
__device__ __forceinline__ void few_check_body(const FewCheckArgs &a, int f, const GlibcTablesBP &tab, double *hb) {
    const int j0 = (int)(blockIdx.x * kFewThreads + threadIdx.x);
    if ((j0 & ~63) >= a.n) return;  // wave-uniform: no check left for this wave
    // surplus lanes of the class's last wave repeat its last check and store nothing
    const bool live = j0 < a.n;
    const int j = live ? j0 : a.n - 1;
    const int cc = a.checks[j];
    QR_DCHECK(cc >= 0 && cc < a.C && a.chk_ptr[cc + 1] - a.chk_ptr[cc] == D, kDbgFewCheck, cc, j);
    const int cb = a.chk_ptr[cc];
    const double *post = a.post + (size_t)f * a.V;
    double *msg = a.msg + (size_t)f * a.E + a.base + j;  // edge position i at msg[i n]
    const uint8_t sb = a.synd[(size_t)f * a.C + cc];
    uint32_t par = sb;
    double m[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const int v = a.chk_var[cb + i];
        QR_DCHECK(v >= 0 && v < a.V, kDbgFewPost, cc, v);
        QR_DCHECK(a.base + (int64_t)i * a.n + j >= 0 && a.base + (int64_t)i * a.n + j < a.E, kDbgFewSlot, cc, i);
        const double p = post[v];
        if (MODE != kFirst) par ^= (p < 0.0) ? 1u : 0u;           // decoder.pyx:243-246
        if (MODE == kNormal) m[i] = p - msg[(size_t)i * a.n];      // :296-297
        else m[i] = p;  // first sweep: c2v == 0 and p - 0.0 == p
    }
    if (MODE != kFirst && live && par == 1u) a.unsat[f] = 1;  // benign race: every writer stores 1
    if constexpr (MODE != kParityOnly) {
        const auto K = GlibcK::pinned();
        few_update<D, FIN>(m, sign_mask(sb), hb + (threadIdx.x >> 6) * kPackWaveDoubles, tab, K, [&](int i, double x) {
            if (live) msg[(size_t)i * a.n] = x;  // only this lane reads it back
        });
    }
}

template <int D, int MODE>
__global__ void __launch_bounds__(kFewThreads) k_few_check(FewCheckArgs a) {
    __shared__ GlibcTablesBP tab;
    __shared__ double hb[(kFewThreads / 64) * kPackWaveDoubles];
    const int f = (int)blockIdx.y;
    if (!a.active[f]) return;  // block-uniform: the frame has stopped
    if (MODE != kParityOnly) stage_glibc_tables(&tab, a.gglibc);
    if constexpr (MODE != kParityOnly && kPacked<D>) {
        if (sld(a.finite)) {  // kernel-uniform: one of the two bodies runs
            few_check_body<D, MODE, true>(a, f, tab, hb);
            return;
        }
    }
    few_check_body<D, MODE, false>(a, f, tab, hb);
}

struct FewVarArgs {
    int64_t V, E;
    const int32_t *var_ptr, *var_slot;
    const double *lappr;  // [B][V]
    const double *msg;    // [B][E]
    double *post;         // [B][V]
    const uint8_t *active;
    int32_t *finite;      // INIT: cleared when an input LAPPR is not below fin_bound (null: not computed)
    double fin_bound;
};

// decoder.pyx:285-298 for the lane's variable, the sum in ascending edge id.  INIT: as var_block's
// (lappr + 0.0 on connected variables of frames still decoding, a plain copy for frames that
// stopped at iteration 0, the batch's finite flag).
template <bool INIT>
__global__ void __launch_bounds__(kFewThreads) k_few_var(FewVarArgs a) {
    const int f = (int)blockIdx.y;
    const bool act = a.active[f] != 0;
    if (!INIT && !act) return;  // block-uniform
    const int64_t v = (int64_t)blockIdx.x * kFewThreads + threadIdx.x;
    if (v >= a.V) return;
    const int b = a.var_ptr[v], e = a.var_ptr[v + 1];
    double p = a.lappr[(size_t)f * a.V + v];
    if (INIT) {
        if (a.finite && !(__builtin_fabs(p) < a.fin_bound)) *a.finite = 0;  // every writer stores 0
        if (act && e > b) p = p + 0.0;
    } else {
        const double *msg = a.msg + (size_t)f * a.E;
        for (int k = b; k < e; ++k) {
            QR_DCHECK(a.var_slot[k] >= 0 && a.var_slot[k] < a.E, kDbgFewSlot, v, a.var_slot[k]);
            p += msg[a.var_slot[k]];  // decoder.pyx:292-293
        }
    }
    a.post[(size_t)f * a.V + v] = p;
}

// ------------------------------------------------------------------ the few-frame schedule
// Codes the few-frame sweeps can run: every check degree templated (2..kMaxTemplDeg).
static bool few_code(const qr_code *code) {
    for (const auto &c : code->classes)
        if (c.degree < 2 || c.degree > kMaxTemplDeg) return false;
    return !code->classes.empty();
}
// qr_decode_frames_device decodes these B frames with run_few
static bool few_route(const qr_code *code, int B, int max_it) {
    return B <= std::min(g_tune.few_max.load(), kFewMaxLimit) && max_it >= 0 && few_code(code) &&
           !takes_resident(code, max_it);
}

// The few-frame workspace: messages msg[B][E], then the flags of the frame-parallel schedules at
// leading dimension ldf = B rounded up to the wavefront (k_init_status / k_status are reused).
struct FewWs {
    double *msg;
    uint8_t *active, *unsat;
    int32_t *acount;  // [2] the finite flag, [4, 16) the RangeSel block k_init_status resets
    size_t bytes;
};
static FewWs few_layout(const qr_code *code, int B, int max_it, void *base = nullptr) {
    FewWs w;
    Cursor c{(uintptr_t)base};
    const size_t ldf = align_up((size_t)B, kWave);
    w.msg = c.take<double>((size_t)code->E * B);
    w.active = c.take<uint8_t>(ldf);
    w.unsat = c.take<uint8_t>((size_t)unsat_rows(max_it) * ldf);
    w.acount = c.take<int32_t>(64);
    w.bytes = c.off;
    return w;
}

struct FewPlan {
    const qr_code *code;
    int B, ldf;
    const double *lappr;
    const uint8_t *synd;
    double *post;
    FewWs w;
    hipStream_t s;
};

// One check sweep: a launch per degree class, all named few_check.
template <int MODE>
static int launch_few_checks(const FewPlan &P, const double *post_in, uint8_t *unsat) {
    const qr_code *code = P.code;
    for (const DegreeClass &cls : code->classes) {
        FewCheckArgs a;
        a.checks = cls.d_checks;
        a.n = (int)cls.n;
        a.base = cls.few_base;
        a.E = code->E;
        a.V = code->V;
        a.C = code->C;
        a.chk_ptr = code->d_chk_ptr;
        a.chk_var = code->d_chk_var;
        a.post = post_in;
        a.msg = P.w.msg;
        a.synd = P.synd;
        a.active = P.w.active;
        a.unsat = unsat;
        a.finite = P.w.acount + 2;
        a.gglibc = code->d_gtab;
        const dim3 grid((unsigned)((cls.n + kFewThreads - 1) / kFewThreads), (unsigned)P.B);
        ProfScope ps("few_check", P.s);
        const bool handled = dispatch_degree<2, kMaxTemplDeg>(
            cls.degree, [&](auto d) { k_few_check<d.value, MODE><<<grid, kFewThreads, 0, P.s>>>(a); });
        if (!handled) return set_error(QR_EVALUE, "decode: no few-frame kernel for degree %d", cls.degree);
        QR_LAUNCH_CHECK();
    }
    return QR_OK;
}

template <bool INIT>
static int launch_few_var(const FewPlan &P, int32_t *finite = nullptr, double fin_bound = 0.0) {
    ProfScope ps(INIT ? "few_var_init" : "few_var", P.s);
    FewVarArgs a;
    a.V = P.code->V;
    a.E = P.code->E;
    a.var_ptr = P.code->d_var_ptr;
    a.var_slot = P.code->d_var_msg;
    a.lappr = P.lappr;
    a.msg = P.w.msg;
    a.post = P.post;
    a.active = P.w.active;
    a.finite = finite;
    a.fin_bound = fin_bound;
    const dim3 grid((unsigned)((P.code->V + kFewThreads - 1) / kFewThreads), (unsigned)P.B);
    k_few_var<INIT><<<grid, kFewThreads, 0, P.s>>>(a);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

// decoder.pyx:391-436 on frame-major arrays, in run_flat's order: parity of the input ->
// status(0) -> first variable sweep -> for t = 1..max_it: C(t), S(t-1), V(t) -> parity of the
// last posteriors -> final status.  Every data-dependent decision is taken on the device (the
// sweeps of a stopped frame leave at once), nothing is allocated and nothing waits: one stream,
// capturable.  The posteriors live in the caller's output array.
static int run_few(const qr_code *code, int B, const double *lappr, const uint8_t *synd, int max_it, double *final_post,
                   uint8_t *success, int32_t *iters, void *ws_ptr, hipStream_t s) {
    FewPlan P{code, B, (int)align_up((size_t)B, kWave), lappr, synd, final_post, few_layout(code, B, max_it, ws_ptr), s};
    const int ldf = P.ldf;
    int rc;
    auto row = [&](int t) { return P.w.unsat + (size_t)t * ldf; };
    auto status = [&](int t, int final_call) {  // k_status over the B frames (no repacked range)
        return launch_status(0, B, t, final_call, final_call ? max_it : 0, row(t), P.w.active, success, iters, nullptr,
                             nullptr, s);
    };
    QR_HIP(hipMemsetAsync(P.w.unsat, 0, (size_t)unsat_rows(max_it) * ldf, s));
    if ((rc = launch_init_status(B, ldf, P.w.active, success, iters, P.w.acount + 2, P.w.acount + 4, ldf / 2,
                                 ldf - ldf / 2, s)))
        return rc;
    const double fin_bound = finite_bound(max_it, code->max_dv);
    if (fin_bound == 0.0) QR_HIP(hipMemsetAsync(P.w.acount + 2, 0, sizeof(int32_t), s));
    if ((rc = launch_few_checks<kParityOnly>(P, lappr, row(0)))) return rc;  // decoder.pyx:400-405
    if ((rc = status(0, 0))) return rc;
    if ((rc = launch_few_var<true>(P, fin_bound > 0.0 ? P.w.acount + 2 : nullptr, fin_bound))) return rc;
    for (int t = 1; t <= max_it; ++t) {  // decoder.pyx:424-433
        if (t == 1) {
            if ((rc = launch_few_checks<kFirst>(P, P.post, row(0)))) return rc;
        } else {
            if ((rc = launch_few_checks<kNormal>(P, P.post, row(t - 1)))) return rc;
            if ((rc = status(t - 1, 0))) return rc;
        }
        if ((rc = launch_few_var<false>(P))) return rc;
    }
    if (max_it > 0) {
        if ((rc = launch_few_checks<kParityOnly>(P, P.post, row(max_it)))) return rc;
    } else {
        // decoder.pyx:424 with max_iterations = 0: no sweep, no check -> (0, 0)
        QR_HIP(hipMemsetAsync(row(0), 1, (size_t)ldf, s));
    }
    return status(max_it, 1);
}

// ------------------------------------------------------------------ frame-major decode
// The frame-parallel route of decode_frames_device stages the transposed input and output at the
// head of the workspace, at ld = B rounded up to the wavefront; decode_batch_device's own
// workspace follows.
struct FramesStage {
    double *lappr_fi, *final_fi;
    uint8_t *synd_fi;
    size_t bytes;
};
static FramesStage frames_stage(const qr_code *code, int ld, void *base = nullptr) {
    FramesStage w;
    Cursor c{(uintptr_t)base};
    w.lappr_fi = c.take<double>((size_t)code->V * ld);
    w.final_fi = c.take<double>((size_t)code->V * ld);
    w.synd_fi = c.take<uint8_t>((size_t)code->C * ld);
    w.bytes = c.off;
    return w;
}

// Room for either route, whatever knob few_max says when the decode is issued.
size_t frames_ws_bytes(const qr_code *code, int B, int max_it) {
    const int ld = (int)align_up((size_t)B, kWave);
    size_t n = frames_stage(code, ld).bytes + ws_bytes(code, ld, max_it);
    if (B <= kFewMaxLimit && max_it >= 0 && few_code(code)) n = std::max(n, few_layout(code, B, max_it).bytes);
    return n;
}

int decode_frames_device(const qr_code *code, int B, const double *lappr, const uint8_t *synd, int max_it,
                         double *final_post, uint8_t *success, int32_t *iters, void *ws_ptr, size_t ws_size,
                         hipStream_t s) {
    if (B <= 0 || B > INT32_MAX - kWave) return set_error(QR_EVALUE, "decode: B must be positive (B=%d)", B);
    if (!lappr || !synd || !final_post || !success || !iters || !ws_ptr)
        return set_error(QR_EVALUE, "decode: null pointer argument");
    if (!ws_aligned(ws_ptr)) return set_error(QR_EVALUE, "decode: workspace must be 256-byte aligned");
    DeviceGuard dg(code->device);
    if (few_route(code, B, max_it)) {
        const size_t need = few_layout(code, B, max_it).bytes;
        if (ws_size < need) return set_error(QR_EVALUE, "decode: workspace too small (%zu < %zu)", ws_size, need);
        return run_few(code, B, lappr, synd, max_it, final_post, success, iters, ws_ptr, s);
    }
    const int ld = (int)align_up((size_t)B, kWave);
    const FramesStage st = frames_stage(code, ld, ws_ptr);
    if (ws_size < st.bytes) return set_error(QR_EVALUE, "decode: workspace too small (%zu < %zu)", ws_size, st.bytes);
    int rc;
    if ((rc = launch_transpose_to_fi_f64(B, ld, code->V, lappr, st.lappr_fi, s))) return rc;
    if ((rc = launch_transpose_to_fi_u8(B, ld, code->C, synd, st.synd_fi, s))) return rc;
    if ((rc = decode_batch_device(code, B, ld, st.lappr_fi, st.synd_fi, max_it, st.final_fi, success, iters,
                                  (char *)ws_ptr + st.bytes, ws_size - st.bytes, s)))
        return rc;
    return launch_transpose_to_fm_f64(B, ld, code->V, st.final_fi, final_post, s);
}

}  // namespace qr
