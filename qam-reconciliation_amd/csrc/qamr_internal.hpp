// qamr_internal.hpp -- shared host-side definitions of libqamr.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "qamr.h"
#include "qamr_math.hpp"
#include "exp_table.hpp"
#include "glibc_math.hpp"

namespace qr {

// ------------------------------------------------------------------ errors
int set_error(int code, const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define QR_HIP(call)                                                            \
    do {                                                                        \
        hipError_t _qr_e = (call);                                              \
        if (_qr_e != hipSuccess) return ::qr::hip_fail(_qr_e, #call, __FILE__, __LINE__); \
    } while (0)

#define QR_LAUNCH_CHECK() QR_HIP(hipGetLastError())

// --------------------------------------------------------------- profiling
// hipEvent pair recorded on the launch stream around one kernel launch.
struct ProfScope {
    ProfScope(std::string name, hipStream_t s);
    ~ProfScope();
    std::string name_;
    hipStream_t s_;
    hipEvent_t a_ = nullptr, b_ = nullptr;
    bool capture_ = false;  // recorded into a graph being captured (external event-record nodes)
    void record(hipEvent_t e);
};
bool profiling_on();

// ------------------------------------------------------------------ layout
constexpr int kWave = 64;
inline int frame_tile(int ld) { return (ld % 256 == 0) ? 256 : (ld % 128 == 0) ? 128 : 64; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// v in LO..LO+N-1 -> f(std::integral_constant<int, v>{}), the value as a compile-time constant;
// false (and no call) outside the range.  Under dispatch_bps (demap_wave.hpp) and dispatch_degree
// (decode_dev.hpp).
template <int LO, class F, int... I>
inline bool dispatch_int_seq(int v, F &f, std::integer_sequence<int, I...>) {
    return ((v == LO + I && (f(std::integral_constant<int, LO + I>{}), true)) || ...);
}

// Bump cursor over a device buffer: take<T>(n) is the next n elements of T, 256-byte aligned
// from a 256-byte aligned base (ws_aligned: what every entry requires of a caller's workspace;
// hipMalloc's blocks, and so Scratch's, are).
// With a null base it only measures: every take is null and off counts the bytes walked.
inline bool ws_aligned(const void *p) { return ((uintptr_t)p & 255) == 0; }

struct Cursor {
    uintptr_t base;
    size_t off = 0;
    template <typename T>
    T *take(size_t n) {
        T *p = base ? (T *)(base + off) : nullptr;
        off += align_up(n * sizeof(T), 256);
        return p;
    }
};

// Device scratch owned by a handle, grown on demand (host-API calls only).
struct Scratch {
    std::mutex mu;
    void *ptr = nullptr;
    size_t bytes = 0;
    int device = 0;
    int reserve(size_t want);  // caller holds mu
    // take(&p0, n0, &p1, n1, ...): reserve room for n0 elements of *p0's type, n1 of *p1's, ...
    // (a Cursor walk) and point p0, p1, ... at them (caller holds mu).
    template <typename... A>
    int take(A... regions) {
        Cursor m{0};
        walk(m, regions...);
        if (int rc = reserve(m.off)) return rc;
        Cursor c{(uintptr_t)ptr};
        walk(c, regions...);
        return 0;
    }
    template <typename T, typename... A>
    static void walk(Cursor &c, T **p, size_t n, A... rest) {
        *p = c.take<T>(n);
        if constexpr (sizeof...(rest) > 0) walk(c, rest...);
    }
    ~Scratch();
};

// Kernel launchers shared between translation units.
int launch_transpose_to_fi_f64(int B, int ld, int64_t n, const double *src, double *dst, hipStream_t s);
int launch_transpose_to_fm_f64(int B, int ld, int64_t n, const double *src, double *dst, hipStream_t s);
int launch_transpose_to_fi_u8(int B, int ld, int64_t n, const uint8_t *src, uint8_t *dst, hipStream_t s);
int launch_transpose_to_fi_i64(int B, int ld, int64_t n, const int64_t *src, int64_t *dst, hipStream_t s);

extern std::atomic<int> g_demap_fast;  // demap.hip (tuning knob "demap_fast")
extern std::atomic<int> g_demap_hyp;   // demap.hip (tuning knob "demap_hyp")
extern std::atomic<int> g_interp_fast; // demap_interp.hip (tuning knob "interp_fast")
extern std::atomic<int> g_interp_seg;  // demap_interp.hip (tuning knob "interp_seg")
extern std::atomic<int> g_np_slack_pct; // npstream.hip (tuning knob "np_slack_pct")

// Host helpers shared by demap.hip, demap_interp.hip, mi.hip and binary_channel.hip.
int check_shape(int B, int ld, int64_t S);                // demap.hip: 0 < B <= ld, ld % 64 == 0, S > 0
unsigned demap_wave_grid(int device, int64_t items);      // demap.hip: workgroups of a grid-stride launch
// demap.hip: the two launches of qr_count_errors_device; neg = the `final < 0` rule of binary_channel.hip
int launch_count_errors(bool neg, int B, int ld, int64_t K, const double *d_final, const uint8_t *d_word,
                        const uint8_t *d_success, const int32_t *d_iters, int32_t *ferr, int64_t *d_counters,
                        hipStream_t s);
// demap.hip: its second launch alone (ferr[B] -> the five counters), for rate_adapt.hip's row-listed count
int launch_count_finish(int B, const int32_t *ferr, const uint8_t *d_success, const int32_t *d_iters, int64_t *d_counters,
                        hipStream_t s);
struct GridView;                                          // grid_interp.hpp
GridView grid_view(const qr_demap *dm);                   // demap_interp.hip: the handle's grid, as the kernels take it
bool grid_fast(const qr_demap *dm);                       // demap_interp.hip: body (b) of the grid's index search
int need_grid(const qr_demap *dm);                        // demap_interp.hip: an error unless the grid was created

// Debug build (libqamr_debug.so, QR_DEBUG_ASSERT=1): device-side index checks (debug_check.hpp).
// Every unit that carries checks counts its own failures and registers its reader there;
// qr_debug_asserts (decoder.hip) reports their sum and the first failing unit's site.
#ifndef QR_DEBUG_ASSERT
#define QR_DEBUG_ASSERT 0
#endif

struct DeviceGuard {
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev_);
        if (prev_ != dev) (void)hipSetDevice(dev);
        dev_ = dev;
    }
    ~DeviceGuard() {
        if (prev_ != dev_) (void)hipSetDevice(prev_);
    }
    int prev_ = 0, dev_ = 0;
};

// The argument rule of every *_host entry that takes n elements from host arrays: a negative n and,
// with n > 0, a null array are QR_EVALUE (n == 0 is the caller's early QR_OK, before any device call).
template <typename... P>
inline int check_host_arrays(int64_t n, const P *...arrays) {
    if (n < 0) return set_error(QR_EVALUE, "negative size");
    if (n > 0 && (... || !arrays)) return set_error(QR_EVALUE, "null pointer argument");
    return QR_OK;
}

// One round trip of host arrays through a handle's scratch.  It holds the device and the scratch's
// lock for its lifetime; an entry reads: validate, take, up, launch, down, return rc.  The first
// failure stays in rc and turns the later copies into no-ops; byte counts are formed here, in size_t.
struct HostTrip {
    HostTrip(Scratch &s, int device) : g_(device), lk_(s.mu), scratch_(s) {}
    template <typename... A>
    bool take(A... regions) {  // Scratch::take; false (and rc) when the scratch cannot grow
        rc = scratch_.take(regions...);
        return rc == QR_OK;
    }
    template <typename T>
    void up(T *dev, const T *host, size_t n) { copy(dev, host, n * sizeof(T), hipMemcpyHostToDevice); }
    template <typename T>
    void down(T *host, const T *dev, size_t n) { copy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost); }
    bool ok() const { return rc == QR_OK; }  // launch only then: a failed upload left the inputs unset
    void launched() { fail(hipGetLastError(), "launch"); }
    int rc = QR_OK;

  private:
    void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        if (rc == QR_OK) fail(hipMemcpy(dst, src, bytes, kind), "hipMemcpy");
    }
    void fail(hipError_t e, const char *what) {
        if (e != hipSuccess) rc = hip_fail(e, what, __FILE__, __LINE__);
    }
    DeviceGuard g_;
    std::lock_guard<std::mutex> lk_;
    Scratch &scratch_;
};

// Diagnostic twin only (libqamr_clock.so, QR_EXPERIMENT_CLOCK=1; the product library carries no
// stamp): a workgroup's shader-clock (s_memtime) and 100 MHz realtime (s_memrealtime) spans added
// to acc[0..2] = {cycles, ticks, workgroups} by thread 0 (vector atomics) when the scope ends, and
// its realtime start / end stored in wgt (first kWgTimes workgroups) if given.  Every thread of
// the workgroup must reach the end of the scope (it ends with a barrier).
#ifndef QR_EXPERIMENT_CLOCK
#define QR_EXPERIMENT_CLOCK 0
#endif
constexpr int kWgTimes = 1 << 16;
#if QR_EXPERIMENT_CLOCK
struct ClkScope {
    bool on;
    unsigned long long *acc, *wgt;
    uint64_t c0, r0;
    __device__ ClkScope(bool on_, unsigned long long *acc_, unsigned long long *wgt_) : on(on_), acc(acc_), wgt(wgt_) {
        c0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
    }
    __device__ ~ClkScope() {
        __syncthreads();
        if (on && threadIdx.x == 0) {
            const uint64_t c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
            atomicAdd(&acc[0], (unsigned long long)(c1 - c0));
            atomicAdd(&acc[1], (unsigned long long)(r1 - r0));
            atomicAdd(&acc[2], 1ull);
            const unsigned b = blockIdx.y * gridDim.x + blockIdx.x;
            if (wgt && b < (unsigned)kWgTimes) {
                wgt[2 * b] = r0;
                wgt[2 * b + 1] = r1;
            }
        }
    }
};
#endif

}  // namespace qr

// --------------------------------------------------------------- handles
struct DegreeClass {
    int32_t degree;
    int64_t n;
    int32_t *d_checks;  // check ids of this degree, ascending
    // degree > kMaxTemplDeg (runtime-degree kernel): first row of this class's forward
    // values in the decode workspace's F scratch (n * (degree - 2) rows of ld doubles)
    int64_t fb_base = 0;
    // first message slot of the class in the node-parallel layout (host_build.hpp build_few_layout)
    int64_t few_base = 0;
};

// One launch of the layered schedule: the checks of one degree in one layer.
struct LayerSegDev {
    int32_t layer, degree;
    int64_t off, n;
};

struct qr_code {
    int64_t E = 0, V = 0, C = 0;
    int32_t max_dc = 0, max_dv = 0;
    int32_t reg_dv = 0;  // every variable node's degree when they are all equal, else 0
    int device = 0;
    size_t mem_bytes = 0;       // the device's memory (bounds the optional repack work set)
    size_t lds_per_block = 0;   // LDS a workgroup may take (the frame-resident decode needs it)
    // CSR, int32 (E < 2^31): per check, edge ids ascending and their variables;
    // per variable, edge ids ascending.
    int32_t *d_chk_ptr = nullptr, *d_chk_edge = nullptr, *d_chk_var = nullptr;
    int32_t *d_var_ptr = nullptr, *d_var_edge = nullptr;
    // per variable, edges ascending as above, each given by its message slot in the node-parallel
    // layout (host_build.hpp build_few_layout: the few-frame schedule's msg[f][slot]; for a
    // single-class code i * C + c, edge i of check c, the frame-resident decode's LDS index)
    int32_t *d_var_msg = nullptr;
    std::vector<DegreeClass> classes;
    int64_t fb_rows = 0;  // rows of the F scratch (sum over runtime-degree classes)
    qr::GlibcTables *d_gtab = nullptr; // strict box-plus: glibc exp/log data (glibc_math.hpp)
    // layered schedule (host_build.hpp build_layers, decode_layered.hip): every check's layer, the
    // non-empty (layer, degree) segments in schedule order with their ascending check ids
    // (d_layer_checks[off, off + n)), and per check whether it repeats a variable
    int32_t n_layers = 0;
    std::vector<int32_t> layer_of;
    std::vector<LayerSegDev> layer_segs;
    int32_t *d_layer_checks = nullptr;
    uint8_t *d_chk_repeat = nullptr;
    mutable qr::Scratch scratch;
    // two-stream schedule (decoder.hip run_split2; run_iter, decode_small.hip): a second stream for the variable
    // sweeps and the events that order the two; created on first use, guarded by mu
    // while a decode enqueues (concurrent decodes on one code enqueue one at a time).
    mutable std::mutex mu;
    mutable hipStream_t s2 = nullptr;
    mutable hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

// Interpolation grid of NoiseMapper.g_inv (noisemapper.pyx:135-144), built on demand by
// qr_demap_grid_create: the tabulated uniform-mixture CDF and its abscissae, interleaved.
struct DemapGrid {
    int32_t n = 0;                 // n_points (0 = not created)
    int32_t nc = 0;                // entries of the coarse table, ceil(n / 2^seg_shift)
    int32_t seg_shift = 0;         // log2 of the entries per coarse-table segment
    int32_t seg_req = 0;           // the knob value it was built under
    int nondecreasing = 0;         // F[r + 1] >= F[r] for every r (one pass at creation)
    double trunc = 0, step = 0;    // the parameters it was built from
    int64_t nips = 0;
    double2 *d_pairs = nullptr;    // [n] {F[r], y[r]}
    double *d_coarse = nullptr;    // [nc] F[c << seg_shift]
    std::vector<double2> h_pairs;  // host copy (qr_demap_grid_host)
};

struct qr_demap {
    int device = 0;
    DemapGrid grid;                         // guarded by scratch.mu while it is (re)built
    qr::DemapTables h;                      // host copy
    qr::DemapTables *d_tables = nullptr;    // device copy
    qr::MathTables *d_mtab = nullptr;       // exp table for the Newton root search
    double2 *d_quant = nullptr;             // F_Y^-1 Hermite nodes (Newton start), may be null
    double *d_ftab = nullptr;               // Taylor table of F_Y (Newton), may be null
    double *d_mi = nullptr;                 // p_Xhat[M] then fwrd_transition_probability[M][M] (qr_demap_mi_tables)
    mutable qr::Scratch scratch;
};
