// decode_host.hpp -- what the decoder's units share on the host side: the tuning knobs, the
// workspace helpers, and the declarations of what one unit calls in another (decoder.hip: the
// frame-parallel schedules and the status kernels; decode_repack.hip: the column repack;
// decode_small.hip: k_iter and k_resident; decode_few.hip: the few-frame schedule and the
// frame-major route; decode_layered.hip: the layered schedule; decode_api.hip: the C entry points).
#pragma once
#include <algorithm>
#include <cmath>

#include "qamr_internal.hpp"

namespace qr {

// Knob few_max: qr_decode_frames_device (and with it qr_decode_host) decodes B <= few_max frames
// of an eligible code with the few-frame schedule (run_few); 0 = off, at most kFewMaxLimit.  The
// default is the largest batch at which the schedule beat the frame-parallel path of the commit
// before it on MI355X (scripts/few_frame_rate.py, profiles/few/README.md).
constexpr int kFewMaxLimit = 64;
constexpr int kFewMaxDefault = 16;

// Runtime tuning knobs (qr_tune_set); defaults picked by scripts/tune.py on MI355X.
struct Tuning {
    std::atomic<int> check_ft{128}, check_per{16}, var_ft{128}, var_per{8}, nt{1}, split{3},
        lds_pad_kb{0}, compact{1}, side{1}, min_blocks{2048}, split_min_blocks{1024}, var_pace{28},
        check_tail{4}, fused_iter{1}, iter_streams{2}, var_boost{4}, resident{1}, repack{1},
        repack_pct{80}, repack_grid{128}, few_max{kFewMaxDefault};
};
extern Tuning g_tune;  // decode_api.hip, beside the knob table

// rows of the unsat flags: one per sweep 0..max_it, plus one (no int overflow at INT_MAX)
inline int64_t unsat_rows(int max_it) { return (int64_t)(max_it > 0 ? max_it : 0) + 2; }

// The finite clamp's bound (see kPackMaxDeg): 2^e with e = 1000 - (max_it + 2) log2(max_dv + 1),
// or 0 when e < 1 (no bound: the flag stays clear).  In double, compared before the cast: max_it
// may be as large as INT_MAX.
inline double finite_bound(int max_it, int max_dv) {
    const double x = ((double)std::max(max_it, 0) + 2.0) * std::log2((double)max_dv + 1.0);
    return x > 999.0 ? 0.0 : std::ldexp(1.0, 1000 - (int)std::ceil(x));
}

// ---- decoder.hip
struct Geom;  // decode_dev.hpp
Geom make_geom(int ncols, int ft_req, int per, int64_t nodes = 0);
int side_stream(const qr_code *code, hipStream_t *out);  // the caller holds code->mu
size_t ws_bytes(const qr_code *code, int ld, int max_it);
int decode_batch_device(const qr_code *code, int B, int ld, const double *lappr, const uint8_t *synd, int max_it,
                        double *final_post, uint8_t *success, int32_t *iters, void *ws_ptr, size_t ws_size,
                        hipStream_t s);
// k_init_status and k_status (the few-frame schedule reuses them; null sel / fid: no repacked range)
int launch_init_status(int B, int ld, uint8_t *active, uint8_t *success, int32_t *iters, int32_t *finite, int32_t *rsel,
                       int w0, int w1, hipStream_t s);
int launch_status(int f0, int f1, int t, int final_call, int32_t final_iters, const uint8_t *unsat_t, uint8_t *active,
                  uint8_t *success, int32_t *iters, const int32_t *sel, const int32_t *fid, hipStream_t s);

// The two sweeps of the flooding decode that the layered schedule (decode_layered.hip) reuses, over
// all ld columns with no active-frame list: the parity-only check sweep of `post` (k_check
// <kParityOnly>: unsat[f] = 1 for every running frame with an unsatisfied check; unsat zeroed by
// the caller) and the init variable sweep (k_var<true>: post = lappr + 0.0, a plain copy for
// frames that stopped at iteration 0; columns [B, ld) not written).  counts: the caller's
// 256-byte count block (k_init_status has set it).
int launch_parity_sweep(const qr_code *code, int B, int ld, const double *post, const uint8_t *synd,
                        const uint8_t *active, uint8_t *unsat, int32_t *counts, hipStream_t s);
int launch_var_init(const qr_code *code, int B, int ld, const double *lappr, double *post, const uint8_t *active,
                    int32_t *counts, hipStream_t s);

// ---- decode_layered.hip: the layered (serial-check) schedule
size_t layered_ws_bytes(const qr_code *code, int ld, int max_it);
int decode_layered_device(const qr_code *code, int B, int ld, const double *lappr, const uint8_t *synd, int max_it,
                          double *final_post, uint8_t *success, int32_t *iters, void *ws_ptr, size_t ws_size,
                          hipStream_t s);

// ---- decode_repack.hip: the two launches of the column repack (run_split2 fills the arguments)
struct RepackArgs {
    int f0, ld, pct;  // the range's first column; repack threshold (percent)
    int64_t V, C;
    const int32_t *count;  // the range's running-frame count
    int32_t *sel;          // its RangeSel
    int32_t *list;         // active-frame list (absolute columns, list[f0 + p])
    uint8_t *active;
    double *out_post;            // the caller's posterior output (frame f at column f)
    const double *lappr_in;      // the caller's LAPPRs
    const uint8_t *synd_in;      // the caller's syndrome bits
    double *post_w;              // the work set's posteriors
    double *lappr_w[2];          // its LAPPRs and syndrome bits, column sets 0 and 1
    uint8_t *synd_w[2];
    int32_t *fid_w;
};
int launch_repack_rows(const RepackArgs &r, unsigned grid, hipStream_t s);
int launch_repack_output(int64_t rows, int f0, int ld, const int32_t *sel, const int32_t *fid_w, const double *post_w,
                         double *out_post, unsigned grid, hipStream_t s);

// ---- decode_small.hip
// What run_iter reads of a decode: the caller's arrays and the workspace's message buffers and flags.
struct IterRun {
    const qr_code *code;
    int B, ld;
    const double *lappr;
    const uint8_t *synd;
    double *post;
    uint8_t *success;
    int32_t *iters;
    double *c2v, *c2v2;
    uint8_t *unsat, *active;
    int32_t *acount;
    hipStream_t s;
};
bool iter_code(const qr_code *code, int ld);
int run_iter(const IterRun &P, int max_it);
bool takes_resident(const qr_code *code, int max_it);
int run_resident(const qr_code *code, int B, int ld, const double *lappr, const uint8_t *synd, int max_it,
                 double *final_post, uint8_t *success, int32_t *iters, int32_t *rsel, hipStream_t s);
#if QR_EXPERIMENT_CLOCK
bool resident_clock_read_clear(unsigned long long h[3]);  // k_resident's {cycles, ticks, workgroups}
#endif

// ---- decode_few.hip
size_t frames_ws_bytes(const qr_code *code, int B, int max_it);
int decode_frames_device(const qr_code *code, int B, const double *lappr, const uint8_t *synd, int max_it,
                         double *final_post, uint8_t *success, int32_t *iters, void *ws_ptr, size_t ws_size,
                         hipStream_t s);

}  // namespace qr
