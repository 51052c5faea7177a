// decode_api.hip -- the decoder's C entry points (include/qamr.h): the code handle, the tuning
// knobs, the decode calls (their schedules live in decoder.hip, decode_small.hip and
// decode_few.hip) and the node-level unit-test surface with its kernels.
#include "decode_dev.hpp"
#include "decode_host.hpp"
#include "host_build.hpp"

namespace qr {

Tuning g_tune;

// ------------------------------------------------- unit-test surface kernels
// One frame, frame-major arrays (ld == 1 layout), lane = node.
__global__ void k_check_lappr_nodes(int64_t C, const int32_t *chk_ptr, const int32_t *chk_var, const double *lappr,
                                    const uint8_t *synd, uint8_t *out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    uint8_t parity = synd[c];
    for (int k = chk_ptr[c]; k < chk_ptr[c + 1]; ++k)
        if (lappr[chk_var[k]] < 0) parity ^= 1;  // decoder.pyx:241-248
    out[c] = parity ^ 1;
}

__global__ void k_check_word_nodes(int64_t C, const int32_t *chk_ptr, const int32_t *chk_var, const uint8_t *word,
                                   const uint8_t *synd, uint8_t *out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    uint8_t parity = synd[c];
    for (int k = chk_ptr[c]; k < chk_ptr[c + 1]; ++k) parity ^= word[chk_var[k]];  // decoder.pyx:182-187
    out[c] = parity ^ 1;
}

__global__ void k_var_nodes(const int64_t *nodes, int64_t n, const int32_t *var_ptr, const int32_t *var_edge,
                            const double *lappr, const double *c2v, double *v2c, double *updated) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t v = nodes[i];
    double p = lappr[v];
    for (int k = var_ptr[v]; k < var_ptr[v + 1]; ++k) p += c2v[var_edge[k]];
    updated[v] = p;
    for (int k = var_ptr[v]; k < var_ptr[v + 1]; ++k) v2c[var_edge[k]] = p - c2v[var_edge[k]];
}

// The node-level surface (process_check_node, decoder.pyx:322-369) for any degree: v2c is
// a separate input here, so the forward values can be parked in the output slots
// c2v[e_i] <- F_{i-1} and replaced in the backward pass.
__global__ void k_check_nodes(const int64_t *nodes, int64_t n, const int32_t *chk_ptr, const int32_t *chk_edge,
                              const uint8_t *synd, double *c2v, const double *v2c, const GlibcTables *gtab) {
    __shared__ GlibcTables tab;
    stage_glibc_tables(&tab, gtab);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t c = nodes[i];
    const int base = chk_ptr[c], d = chk_ptr[c + 1] - base;
    const double s = synd[c] ? -1.0 : 1.0;
    const int32_t *e = chk_edge + base;
    double F = v2c[e[0]];
    for (int k = 1; k <= d - 2; ++k) {
        c2v[e[k]] = F;  // F_{k-1}
        F = box_plus_strict(F, v2c[e[k]], tab);
    }
    double Bn = v2c[e[d - 1]];
    c2v[e[d - 1]] = s * F;
    for (int k = d - 2; k >= 1; --k) {
        const double Fk = c2v[e[k]];
        c2v[e[k]] = s * box_plus_strict(Fk, Bn, tab);
        Bn = box_plus_strict(Bn, v2c[e[k]], tab);
    }
    c2v[e[0]] = s * Bn;
}

}  // namespace qr

// ===================================================================== C-ABI
using namespace qr;

static int free_code(qr_code *c) {
    if (!c) return QR_OK;
    DeviceGuard g(c->device);
    for (auto &cls : c->classes) (void)hipFree(cls.d_checks);
    (void)hipFree(c->d_chk_ptr);
    (void)hipFree(c->d_chk_edge);
    (void)hipFree(c->d_chk_var);
    (void)hipFree(c->d_var_ptr);
    (void)hipFree(c->d_var_edge);
    (void)hipFree(c->d_var_msg);
    (void)hipFree(c->d_gtab);
    (void)hipFree(c->d_layer_checks);
    (void)hipFree(c->d_chk_repeat);
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->s2) (void)hipStreamDestroy(c->s2);
    delete c;
    return QR_OK;
}

template <typename T>
static int upload(T **dst, const std::vector<T> &src) {
    QR_HIP(hipMalloc((void **)dst, std::max<size_t>(1, src.size()) * sizeof(T)));
    if (!src.empty()) QR_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return QR_OK;
}

extern "C" {

int qr_code_create(const int64_t *e_to_v, const int64_t *e_to_c, int64_t nv, int64_t nc, int32_t device,
                   qr_code **out) {
    if (!out) return set_error(QR_EVALUE, "null output handle");
    *out = nullptr;
    TannerCsr T;  // host_build.hpp (decoder.pyx:60-146)
    std::string err;
    if (int rc = build_tanner_csr(e_to_v, e_to_c, nv, nc, T, err)) return set_error(rc, "%s", err.c_str());
    const int64_t E = T.E, V = T.V, C = T.C;
    const int32_t max_dc = T.max_dc, max_dv = T.max_dv;
    std::vector<int32_t> &chk_ptr = T.chk_ptr, &chk_edge = T.chk_edge, &chk_var = T.chk_var, &var_ptr = T.var_ptr,
                         &var_edge = T.var_edge;
    std::vector<std::vector<int32_t>> &by_deg = T.by_deg;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(QR_EDEVICE, "no HIP device available (libqamr has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(QR_EVALUE, "device %d out of range (%d devices)", device, ndev);
    DeviceGuard g(device);
    qr_code *code = new qr_code();
    code->E = E;
    code->V = V;
    code->C = C;
    code->max_dc = max_dc;
    code->max_dv = max_dv;
    code->reg_dv = max_dv;  // the common variable degree, or 0
    for (int64_t v = 0; v < V; ++v)
        if (var_ptr[(size_t)v + 1] - var_ptr[(size_t)v] != max_dv) code->reg_dv = 0;
    code->device = device;
    code->scratch.device = device;
    {
        size_t mem = 0;
        int lds = 0;
        if (hipDeviceTotalMem(&mem, device) != hipSuccess) mem = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) lds = 0;
        code->mem_bytes = mem;
        code->lds_per_block = (size_t)(lds > 0 ? lds : 0);
    }
    int rc = QR_OK;
    if ((rc = upload(&code->d_chk_ptr, chk_ptr)) || (rc = upload(&code->d_chk_edge, chk_edge)) ||
        (rc = upload(&code->d_chk_var, chk_var)) || (rc = upload(&code->d_var_ptr, var_ptr)) ||
        (rc = upload(&code->d_var_edge, var_edge))) {
        free_code(code);
        return rc;
    }
    // the message slot of every edge in the node-parallel layout, in the variable CSR's order (the
    // few-frame schedule; a single-class code: i * C + c, the frame-resident decode's LDS index)
    FewLayout few;
    build_few_layout(T, few);
    if ((rc = upload(&code->d_var_msg, few.var_slot))) {
        free_code(code);
        return rc;
    }
    {
        std::vector<GlibcTables> gt(1);
        build_glibc_tables(&gt[0]);
        if ((rc = upload(&code->d_gtab, gt))) {
            free_code(code);
            return rc;
        }
    }
    {
        // the layered schedule's layers and check lists (decode_layered.hip), uploaded once
        Layers lay;
        build_layers(T, lay);
        code->n_layers = lay.n_layers;
        code->layer_of = lay.layer_of;
        for (const LayerSeg &g : lay.segs) code->layer_segs.push_back(LayerSegDev{g.layer, g.degree, g.off, g.n});
        if ((rc = upload(&code->d_layer_checks, lay.checks)) || (rc = upload(&code->d_chk_repeat, lay.repeat))) {
            free_code(code);
            return rc;
        }
    }
    for (int d = 0; d < (int)by_deg.size(); ++d) {
        if (by_deg[d].empty()) continue;
        DegreeClass cls{d, (int64_t)by_deg[d].size(), nullptr};
        cls.few_base = few.classes[code->classes.size()].base;  // the same order: ascending degree
        if (d > kMaxTemplDeg) {
            cls.fb_base = code->fb_rows;
            code->fb_rows += cls.n * (d - 2);
        }
        if ((rc = upload(&cls.d_checks, by_deg[d]))) {
            free_code(code);
            return rc;
        }
        code->classes.push_back(cls);
    }
    *out = code;
    return QR_OK;
}

int qr_code_destroy(qr_code *code) { return free_code(code); }

// name -> knob (nullptr if unknown)
static std::atomic<int> *tune_knob(const char *name) {
    static const std::pair<const char *, std::atomic<int> *> knobs[] = {
        {"check_ft", &g_tune.check_ft},     {"check_per", &g_tune.check_per},
        {"var_ft", &g_tune.var_ft},         {"var_per", &g_tune.var_per},
        {"nt", &g_tune.nt},                 {"split", &g_tune.split},
        {"lds_pad_kb", &g_tune.lds_pad_kb}, {"compact", &g_tune.compact},
        {"side", &g_tune.side},             {"demap_fast", &g_demap_fast},
        {"demap_hyp", &g_demap_hyp},        {"min_blocks", &g_tune.min_blocks},
        {"interp_fast", &g_interp_fast},    {"interp_seg", &g_interp_seg},
        {"split_min_blocks", &g_tune.split_min_blocks},
        {"var_pace", &g_tune.var_pace},     {"check_tail", &g_tune.check_tail}, {"var_boost", &g_tune.var_boost},
        {"fused_iter", &g_tune.fused_iter}, {"iter_streams", &g_tune.iter_streams},
        {"resident", &g_tune.resident},   {"repack", &g_tune.repack},
        {"repack_pct", &g_tune.repack_pct}, {"repack_grid", &g_tune.repack_grid},
        {"few_max", &g_tune.few_max},     {"np_slack_pct", &g_np_slack_pct},
    };
    const std::string n = name ? name : "";
    for (const auto &k : knobs)
        if (n == k.first) return k.second;
    return nullptr;
}

int qr_tune_set(const char *name, int64_t value) {
    std::atomic<int> *k = tune_knob(name);
    if (!k) return set_error(QR_EVALUE, "unknown tuning knob '%s'", name ? name : "");
    if (value < 0 || value > 4096 || (k == &g_tune.split && value != 0 && value != 1 && value != 3) ||
        (k == &g_tune.few_max && value > kFewMaxLimit))
        return set_error(QR_EVALUE, "tuning value out of range");
    k->store((int)value);
    return QR_OK;
}

int qr_tune_get(const char *name, int64_t *value) {
    const std::atomic<int> *k = tune_knob(name);
    if (!k || !value) return set_error(QR_EVALUE, "unknown tuning knob '%s'", name ? name : "");
    *value = k->load();
    return QR_OK;
}

int qr_code_info(const qr_code *code, int64_t *vnum, int64_t *cnum, int64_t *ednum, int32_t *max_dc,
                 int32_t *max_dv) {
    if (!code) return set_error(QR_EVALUE, "null code");
    if (vnum) *vnum = code->V;
    if (cnum) *cnum = code->C;
    if (ednum) *ednum = code->E;
    if (max_dc) *max_dc = code->max_dc;
    if (max_dv) *max_dv = code->max_dv;
    return QR_OK;
}

int qr_decode_workspace_size(const qr_code *code, int32_t ld, int32_t max_it, size_t *bytes) {
    if (!code || !bytes) return set_error(QR_EVALUE, "null argument");
    if (ld <= 0 || ld % kWave) return set_error(QR_EVALUE, "ld must be a positive multiple of 64");
    *bytes = ws_bytes(code, ld, max_it);
    return QR_OK;
}

int qr_decode_batch_device(const qr_code *code, int32_t B, int32_t ld, const double *d_lappr, const uint8_t *d_synd,
                           int32_t max_it, double *d_final, uint8_t *d_success, int32_t *d_iters, void *ws,
                           size_t ws_size, void *stream) {
    if (!code) return set_error(QR_EVALUE, "null code");
    return decode_batch_device(code, B, ld, d_lappr, d_synd, max_it, d_final, d_success, d_iters, ws, ws_size,
                               (hipStream_t)stream);
}

int qr_decode_frames_workspace_size(const qr_code *code, int32_t B, int32_t max_it, size_t *bytes) {
    if (!code || !bytes) return set_error(QR_EVALUE, "null argument");
    if (B <= 0 || B > INT32_MAX - kWave) return set_error(QR_EVALUE, "B must be positive");
    *bytes = frames_ws_bytes(code, B, max_it);
    return QR_OK;
}

int qr_decode_frames_device(const qr_code *code, int32_t B, const double *d_lappr, const uint8_t *d_synd, int32_t max_it,
                            double *d_final, uint8_t *d_success, int32_t *d_iters, void *ws, size_t ws_size,
                            void *stream) {
    if (!code) return set_error(QR_EVALUE, "null code");
    return decode_frames_device(code, B, d_lappr, d_synd, max_it, d_final, d_success, d_iters, ws, ws_size,
                                (hipStream_t)stream);
}

int qr_code_layers(const qr_code *code, int32_t *n_layers, int32_t *layer_of) {
    if (!code) return set_error(QR_EVALUE, "null code");
    if (n_layers) *n_layers = code->n_layers;
    if (layer_of) std::copy(code->layer_of.begin(), code->layer_of.end(), layer_of);
    return QR_OK;
}

int qr_decode_layered_workspace_size(const qr_code *code, int32_t ld, int32_t max_it, size_t *bytes) {
    if (!code || !bytes) return set_error(QR_EVALUE, "null argument");
    if (ld <= 0 || ld % kWave) return set_error(QR_EVALUE, "ld must be a positive multiple of 64");
    if (max_it < 0) return set_error(QR_EVALUE, "max_iterations must not be negative");
    *bytes = layered_ws_bytes(code, ld, max_it);
    return QR_OK;
}

int qr_decode_layered_device(const qr_code *code, int32_t B, int32_t ld, const double *d_lappr, const uint8_t *d_synd,
                             int32_t max_it, double *d_final, uint8_t *d_success, int32_t *d_iters, void *ws,
                             size_t ws_size, void *stream) {
    if (!code) return set_error(QR_EVALUE, "null code");
    return decode_layered_device(code, B, ld, d_lappr, d_synd, max_it, d_final, d_success, d_iters, ws, ws_size,
                                 (hipStream_t)stream);
}

// Frame-major host arrays: transposed on the device into ld = B rounded up to the wavefront,
// decoded there, transposed back (the handle's scratch holds the staging and the workspace).
int qr_decode_layered_host(const qr_code *code, int32_t B, const double *lappr, const uint8_t *synd, int32_t max_it,
                           double *final_lappr, uint8_t *success, int32_t *iterations) {
    if (!code) return set_error(QR_EVALUE, "null code");
    if (B <= 0 || B > INT32_MAX - kWave) return set_error(QR_EVALUE, "B must be positive");
    if (max_it < 0) return set_error(QR_EVALUE, "max_iterations must not be negative");
    if (int rc = check_host_arrays(B, lappr, synd, final_lappr, success, iterations)) return rc;
    if (code->max_dc > kMaxTemplDeg)
        return set_error(QR_EUNSUPPORTED, "layered decode: check degree %d above %d", code->max_dc, kMaxTemplDeg);
    const size_t V = code->V, C = code->C, nB = (size_t)B;
    const int ld = (int)align_up(nB, kWave);
    const size_t wsb = layered_ws_bytes(code, ld, max_it);
    HostTrip t(code->scratch, code->device);
    double *d_fm, *d_lfi, *d_ffi;  // d_fm: the frame-major LAPPRs in, then the frame-major result out
    uint8_t *d_sfm, *d_sfi, *d_succ;
    int32_t *d_it;
    char *d_ws;
    if (!t.take(&d_fm, V * nB, &d_lfi, V * ld, &d_ffi, V * ld, &d_sfm, C * nB, &d_sfi, C * ld, &d_succ, nB, &d_it, nB,
                &d_ws, wsb))
        return t.rc;
    t.up(d_fm, lappr, V * nB);
    t.up(d_sfm, synd, C * nB);
    hipStream_t s = nullptr;
    if (t.ok()) t.rc = launch_transpose_to_fi_f64(B, ld, (int64_t)V, d_fm, d_lfi, s);
    if (t.ok()) t.rc = launch_transpose_to_fi_u8(B, ld, (int64_t)C, d_sfm, d_sfi, s);
    if (t.ok()) t.rc = decode_layered_device(code, B, ld, d_lfi, d_sfi, max_it, d_ffi, d_succ, d_it, d_ws, wsb, s);
    if (t.ok()) t.rc = launch_transpose_to_fm_f64(B, ld, (int64_t)V, d_ffi, d_fm, s);
    t.down(final_lappr, d_fm, V * nB);
    t.down(success, d_succ, nB);
    t.down(iterations, d_it, nB);
    return t.rc;
}

int qr_decode_host(const qr_code *code, int32_t B, const double *lappr, const uint8_t *synd, int32_t max_it,
                   double *final_lappr, uint8_t *success, int32_t *iterations) {
    if (!code) return set_error(QR_EVALUE, "null code");
    if (B <= 0) return set_error(QR_EVALUE, "B must be positive");
    if (B > INT32_MAX - kWave) return set_error(QR_EVALUE, "B too large");
    const size_t V = code->V, C = code->C;
    const size_t wsb = frames_ws_bytes(code, B, max_it);
    DeviceGuard g(code->device);
    std::lock_guard<std::mutex> lk(code->scratch.mu);
    double *d_lappr, *d_final;  // frame-major, as the caller's
    uint8_t *d_synd, *d_succ;
    int32_t *d_it;
    char *d_ws;
    int rc = code->scratch.take(&d_lappr, V * B, &d_final, V * B, &d_synd, C * B, &d_succ, (size_t)B, &d_it, (size_t)B,
                                &d_ws, wsb);
    if (rc) return rc;
    hipStream_t s = nullptr;
    QR_HIP(hipMemcpyAsync(d_lappr, lappr, V * B * 8, hipMemcpyHostToDevice, s));
    QR_HIP(hipMemcpyAsync(d_synd, synd, C * B, hipMemcpyHostToDevice, s));
    if ((rc = decode_frames_device(code, B, d_lappr, d_synd, max_it, d_final, d_succ, d_it, d_ws, wsb, s))) return rc;
    QR_HIP(hipMemcpyAsync(final_lappr, d_final, V * B * 8, hipMemcpyDeviceToHost, s));
    QR_HIP(hipMemcpyAsync(success, d_succ, B, hipMemcpyDeviceToHost, s));
    QR_HIP(hipMemcpyAsync(iterations, d_it, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    QR_HIP(hipStreamSynchronize(s));
    return QR_OK;
}

// ------------------------------------------------------ unit-test surface
static int check_nodes_common(const qr_code *code, const void *vals, size_t val_bytes, const uint8_t *synd,
                              uint8_t *check_ok, uint8_t *all_ok, bool is_word) {
    if (!code) return set_error(QR_EVALUE, "null code");
    const size_t C = code->C;
    if (int rc = check_host_arrays((int64_t)C, vals, synd)) return rc;
    HostTrip t(code->scratch, code->device);
    uint8_t *d_vals, *d_synd, *d_ok;
    if (!t.take(&d_vals, val_bytes, &d_synd, C, &d_ok, C)) return t.rc;
    t.up(d_vals, (const uint8_t *)vals, val_bytes);
    t.up(d_synd, synd, C);
    if (t.ok()) {
        if (is_word)
            k_check_word_nodes<<<(unsigned)((C + 255) / 256), 256>>>(C, code->d_chk_ptr, code->d_chk_var, d_vals, d_synd,
                                                                      d_ok);
        else
            k_check_lappr_nodes<<<(unsigned)((C + 255) / 256), 256>>>(C, code->d_chk_ptr, code->d_chk_var,
                                                                       (const double *)d_vals, d_synd, d_ok);
        t.launched();
    }
    std::vector<uint8_t> ok(C);
    t.down(ok.data(), d_ok, C);
    if (!t.ok()) return t.rc;
    uint8_t all = 1;
    for (size_t c = 0; c < C; ++c) {
        if (check_ok) check_ok[c] = ok[c];
        if (!ok[c]) all = 0;  // decoder.pyx:214-217, :254-257
    }
    if (all_ok) *all_ok = all;
    return QR_OK;
}

int qr_check_lappr_host(const qr_code *code, const double *lappr, const uint8_t *synd, uint8_t *check_ok,
                        uint8_t *all_ok) {
    if (!code) return set_error(QR_EVALUE, "null code");
    return check_nodes_common(code, lappr, (size_t)code->V * 8, synd, check_ok, all_ok, false);
}

int qr_check_word_host(const qr_code *code, const uint8_t *word, const uint8_t *synd, uint8_t *check_ok,
                       uint8_t *all_ok) {
    if (!code) return set_error(QR_EVALUE, "null code");
    return check_nodes_common(code, word, (size_t)code->V, synd, check_ok, all_ok, true);
}

int qr_process_var_nodes_host(const qr_code *code, const int64_t *nodes, int64_t n, const double *lappr,
                              const double *c2v, double *v2c, double *updated) {
    if (!code) return set_error(QR_EVALUE, "null code");
    if (int rc = check_host_arrays(n, nodes, lappr, c2v, v2c, updated)) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (nodes[i] < 0 || nodes[i] >= code->V) return set_error(QR_EVALUE, "variable node index out of range");
    if (n == 0) return QR_OK;
    HostTrip t(code->scratch, code->device);
    const size_t V = code->V, E = code->E;
    int64_t *d_nodes;
    double *d_lappr, *d_upd, *d_c2v, *d_v2c;
    if (!t.take(&d_nodes, (size_t)n, &d_lappr, V, &d_upd, V, &d_c2v, E, &d_v2c, E)) return t.rc;
    t.up(d_nodes, nodes, n);
    t.up(d_lappr, lappr, V);
    t.up(d_upd, updated, V);
    t.up(d_c2v, c2v, E);
    t.up(d_v2c, v2c, E);
    if (t.ok()) {
        k_var_nodes<<<(unsigned)((n + 255) / 256), 256>>>(d_nodes, n, code->d_var_ptr, code->d_var_edge, d_lappr, d_c2v,
                                                          d_v2c, d_upd);
        t.launched();
    }
    t.down(v2c, d_v2c, E);
    t.down(updated, d_upd, V);
    return t.rc;
}

int qr_process_check_nodes_host(const qr_code *code, const int64_t *nodes, int64_t n, const uint8_t *synd,
                                double *c2v, const double *v2c) {
    if (!code) return set_error(QR_EVALUE, "null code");
    if (int rc = check_host_arrays(n, nodes, synd, c2v, v2c)) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (nodes[i] < 0 || nodes[i] >= code->C) return set_error(QR_EVALUE, "check node index out of range");
    if (n == 0) return QR_OK;
    HostTrip t(code->scratch, code->device);
    const size_t C = code->C, E = code->E;
    int64_t *d_nodes;
    uint8_t *d_synd;
    double *d_c2v, *d_v2c;
    if (!t.take(&d_nodes, (size_t)n, &d_synd, C, &d_c2v, E, &d_v2c, E)) return t.rc;
    t.up(d_nodes, nodes, n);
    t.up(d_synd, synd, C);
    t.up(d_c2v, c2v, E);
    t.up(d_v2c, v2c, E);
    if (t.ok()) {
        k_check_nodes<<<(unsigned)((n + 255) / 256), 256>>>(d_nodes, n, code->d_chk_ptr, code->d_chk_edge, d_synd, d_c2v,
                                                            d_v2c, code->d_gtab);
        t.launched();
    }
    t.down(c2v, d_c2v, E);
    return t.rc;
}

}  // extern "C"
