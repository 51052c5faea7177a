/*
 * qamr.h -- C-ABI of libqamr.so, the MI355X (gfx950) LDPC syndrome decoder and
 * PAM/BICM soft demapper that replaces the hot path of
 * moriglia/qam-reconciliation.
 *
 * The reference exposes this path only as Cython extension types (no C-ABI):
 *   qamreconciliation.Decoder(e_to_v, e_to_c)            decoder.pyx:92-146
 *   Decoder.decode(lappr, synd, max_iterations)           decoder.pyx:441-455
 *   Decoder._decode(...)  (cdef, called by the sims)      decoder.pyx:391-436
 *   NoiseMapper(pa, noise_var, sign_config)               noisemapper.pyx:103-236
 *   NoiseMapper.demap_lappr_array(n, j)                   noisemapper.pyx:544-559
 * Every entry point below names the reference interface it replaces.  The
 * Python facade (qam-reconciliation_amd/qamr) binds these with ctypes; see
 * INTEGRATION.md for the binding a maintainer would add on the reference side.
 *
 * Conventions
 *  - Every function returns an int status (QR_OK = 0).  On error
 *    qr_last_error() returns a thread-local message.  Status -> Python:
 *    QR_EVALUE -> ValueError, QR_EMEMORY -> MemoryError, others -> RuntimeError.
 *  - "_host" functions take host (CPU) buffers, frame-major ([B][V] etc.), and
 *    run synchronously on the device the handle was created on.
 *  - "_device" functions take device (HBM) pointers in the FRAME-INNERMOST
 *    layout: element (node n, frame f) lives at ptr[n * ld + f], with
 *    B <= ld and ld a multiple of 64 (one wavefront = 64 frames).  They are
 *    asynchronous on `stream` (a hipStream_t; NULL = the null stream), make no
 *    allocation and no host synchronisation (graph-capturable).
 *  - A caller's device workspace (d_workspace of qr_decode_batch_device, qr_decode_frames_device,
 *    qr_decode_layered_device, qr_mi_montecarlo_device, qr_lappr_info_device, qr_npstream_frames_device) must be 256-byte
 *    aligned: the arrays inside it are placed at 256-byte steps from its base.  A misaligned base
 *    is QR_EVALUE before any launch.  The library writes nothing outside
 *    [d_workspace, d_workspace + the size its *_workspace_size returned), and reads nothing inside
 *    it that the same call has not written: what the workspace holds on entry never matters.
 *  - All arithmetic is IEEE fp64, unfused, in the reference's operation order.
 */
#ifndef QAMR_H
#define QAMR_H
#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define QR_API __attribute__((visibility("default")))
#else
#define QR_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define QR_OK 0
#define QR_EVALUE 1      /* -> ValueError  */
#define QR_EMEMORY 2     /* -> MemoryError */
#define QR_EDEVICE 3     /* HIP runtime error -> RuntimeError */
#define QR_EUNSUPPORTED 4
#define QR_EINTERNAL 5   /* a bounded retry ran out (qr_npstream_frames_device) -> RuntimeError */

typedef struct qr_code qr_code;   /* Tanner graph resident in HBM   */
typedef struct qr_demap qr_demap; /* NoiseMapper tables in HBM      */
typedef struct qr_npstream qr_npstream; /* numpy's legacy global stream (MT19937 state + cached normal) */

/* ------------------------------------------------------------------ misc */
QR_API const char *qr_last_error(void);
QR_API int qr_version(int32_t *major, int32_t *minor);
QR_API int qr_device_count(int32_t *count);

/* Per-kernel timing with hipEvents on the launch stream (bench.py uses it to
 * price the dominant kernel).  Off by default; zero cost when off. */
QR_API int qr_profile_enable(int32_t on);
QR_API int qr_profile_reset(void);
/* Restrict the timing to the launches whose profile name is in the comma-separated list
 * `names` (NULL or "" = every launch): the events of the other launches are not recorded
 * at all, so timing only the kernel being priced perturbs the stream less. */
QR_API int qr_profile_select(const char *names);
/* name: "check" (one check sweep, all degree classes), "check_d<D>" (the launch
 * for check degree D), "check1" (first sweep), "var", "var_init", "status",
 * "parity", "demap", "demap_interp", "bob", "syndrome", "count"; the few-frame schedule:
 * "few_check" (every check-sweep launch), "few_var", "few_var_init"; the layered schedule:
 * "layer_check" (every layer launch), "layer_check_d<D>", "layer_parity"; numpy's stream: "np_words",
 * "np_scan", "np_chain", "np_fill".  Synchronises pending events. */
QR_API int qr_profile_query(const char *name, double *total_ms, int64_t *launches);

/* Kernel-geometry knobs (process-wide; performance only, results unchanged):
 * "check_ft"/"var_ft" frames per workgroup (64/128/256), "check_per"/"var_per"
 * nodes per thread, "nt" non-temporal edge-message stream (0/1), "split"
 * (0 or 1 = all frames in lock-step, 3 = the default: two frame halves half an
 * iteration apart on two streams, so one half's check sweep overlaps the other
 * half's variable sweep, where a half batch fills the chip; any other value is
 * QR_EVALUE), "demap_fast" (1 = Newton-located root +
 * replayed bisection, bit-identical to 0 = the reference's brute-force search),
 * "interp_fast" (index search of the interpolated g_inv: 1 = coarse table + segment bisection
 * where the grid is nondecreasing, 0 = the reference's __binsearch probe for probe),
 * "interp_seg" (log2 of the grid entries per coarse-table segment, default 4, used from 1 to 20
 * and raised until the coarse table has at most 4096 entries; read by qr_demap_grid_create, which
 * rebuilds a grid made under another value), "resident" (1 = small single-degree codes decode
 * frame-resident in LDS, one launch per decode), "few_max" (qr_decode_frames_device and
 * qr_decode_host decode up to this many frames with the few-frame schedule; 0..64, 0 = off, any
 * other value is QR_EVALUE and changes nothing), "np_slack_pct" (qr_npstream_*: percent of the
 * slack that the first generated range of a call gets past its mean, default 100; 0 = the mean
 * alone, so about every other call tops up). */
QR_API int qr_tune_set(const char *name, int64_t value);
QR_API int qr_tune_get(const char *name, int64_t *value);

/* ------------------------------------------------------------ Tanner graph */
/* Replaces Decoder.__cinit__ (decoder.pyx:93-146).  e_to_v / e_to_c: host int64
 * edge lists (edge e joins variable e_to_v[e] and check e_to_c[e]).  V = max+1,
 * C = max+1 (decoder.pyx:101-103).  Per-check and per-variable edge lists keep
 * ascending edge id (decoder.pyx:73-75).  QR_EVALUE on size mismatch
 * (decoder.pyx:96-97), negative ids, or a check of degree < 2 (undefined
 * behaviour in the reference, decoder.pyx:135-141; rejected here). */
QR_API int qr_code_create(const int64_t *e_to_v, const int64_t *e_to_c, int64_t n_edges_v, int64_t n_edges_c,
                   int32_t device, qr_code **out);
QR_API int qr_code_destroy(qr_code *code);
/* Decoder.vnum / cnum / ednum properties (decoder.pyx:157-172). */
QR_API int qr_code_info(const qr_code *code, int64_t *vnum, int64_t *cnum, int64_t *ednum, int32_t *max_check_degree,
                 int32_t *max_var_degree);

/* ------------------------------------------------------------------ decode */
/* Device workspace (bytes) for qr_decode_batch_device at leading dim ld and
 * max_iterations (edge messages E*ld fp64 + per-frame flags; with tuning knob "repack" on
 * (default) and ld % 512 == 0, plus the column-repack work set: posteriors, frame ids and two
 * column sets of messages, LAPPRs and syndrome bits used in turn by consecutive repacks (the
 * repack gathers LAPPRs and syndrome bits, the check sweep after it writes the messages),
 * (8E + 24V + 2C + 4)*ld bytes -- a workspace without it runs the same decode without the
 * repack). */
QR_API int qr_decode_workspace_size(const qr_code *code, int32_t ld, int32_t max_iterations, size_t *bytes);

/* Batched Decoder._decode (decoder.pyx:391-436) of B independent frames.
 *   d_lappr [V][ld] fp64   input LAPPRs          (not modified)
 *   d_synd  [C][ld] uint8  target syndromes      (0/1)
 *   d_final [V][ld] fp64   final LAPPRs = posterior after the last variable sweep,
 *                          or a copy of d_lappr when the input already satisfies
 *                          the syndrome (decoder.pyx:400-405); the padding columns
 *                          [B, ld) are not written
 *   d_success[B] uint8, d_iters[B] int32: the (success, iterations) pair of
 *                          _decode for every frame (decoder.pyx:433,436).
 * Per-frame early termination; results per frame are identical to decoding
 * that frame alone.
 * Asynchronous: every launch is enqueued on `stream` (the two-stream schedule also on a
 * library-owned second stream, forked from and joined back into `stream` by events) and the
 * call returns without waiting for the GPU; every schedule decision that depends on the data
 * (early termination, active-frame lists, column repack) is taken on the device, so the call
 * is capturable into a HIP graph and the replay computes the same results. */
QR_API int qr_decode_batch_device(const qr_code *code, int32_t B, int32_t ld, const double *d_lappr, const uint8_t *d_synd,
                           int32_t max_iterations, double *d_final, uint8_t *d_success, int32_t *d_iters,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/* Diagnostics of the column repack of the last qr_decode_batch_device that used this workspace
 * (the same code, ld, max_iterations and workspace): out[0], out[1] = how many times the device
 * repacked frame range 0 / 1 of the two-stream schedule, out[2], out[3] = the width each range
 * ended at (0 repacks and width ld / 2 for a range never repacked, and for every decode that did
 * not take the two-stream schedule).
 * Synchronous device-to-host copy: call after the decode has completed. */
QR_API int qr_decode_repack_stats(const qr_code *code, int32_t ld, int32_t max_iterations, const void *d_workspace,
                                  size_t workspace_bytes, int32_t *out);

/* Batched Decoder._decode on FRAME-MAJOR device arrays: d_lappr [B][V], d_synd [B][C] -> d_final [B][V],
 * d_success [B], d_iters [B].  Any B >= 1.
 * B <= tuning knob "few_max" frames of a code whose check degrees all lie in 2..16 (and that the
 * frame-resident decode does not take: see knob "resident") run the few-frame schedule straight on
 * the caller's arrays: a lane is one check (or one variable) of one frame, one launch per sweep and
 * degree class, messages frame-major in the workspace.  Anything else is transposed into the
 * workspace, decoded by qr_decode_batch_device at ld = B rounded up to 64, and transposed back.
 * Either way the results are those of qr_decode_batch_device, bit for bit.
 * qr_decode_frames_workspace_size covers both routes, so a knob changed between sizing and decoding
 * cannot make the workspace short.  Asynchronous on `stream`, no allocation, capturable into a HIP
 * graph; errors as qr_decode_batch_device. */
QR_API int qr_decode_frames_workspace_size(const qr_code *code, int32_t B, int32_t max_iterations, size_t *bytes);
QR_API int qr_decode_frames_device(const qr_code *code, int32_t B, const double *d_lappr, const uint8_t *d_synd,
                            int32_t max_iterations, double *d_final, uint8_t *d_success, int32_t *d_iters,
                            void *d_workspace, size_t workspace_bytes, void *stream);

/* Decoder.decode (decoder.pyx:441-455) for B frames from host memory,
 * frame-major: lappr[B][V], synd[B][C], final[B][V]: host-to-device copies, qr_decode_frames_device
 * on the handle's scratch, device-to-host copies. */
QR_API int qr_decode_host(const qr_code *code, int32_t B, const double *lappr, const uint8_t *synd, int32_t max_iterations,
                   double *final_lappr, uint8_t *success, int32_t *iterations);

/* ------------------------------------------------- layered decode schedule */
/* A layered (serial-check) sum-product schedule.  The reference has none: this library defines
 * it, and the entries below are bit-exact against the definition.  The posteriors are updated
 * after every check instead of after a whole sweep, so the later checks of an iteration see the
 * earlier checks' messages; the box-plus and the F/B recursion are the flooding decoder's
 * (decoder.pyx:322-369, :41-45), IEEE fp64, unfused, glibc exp/log.  Per frame:
 *
 *   if check_lappr(lappr, synd): return (1, 0, copy of lappr)              (decoder.pyx:400-405)
 *   post[v] = lappr[v] + 0.0 for every v with an edge, lappr[v] otherwise
 *   c2v[e]  = 0.0
 *   for it in 0 .. max_iterations-1:
 *       for c in schedule order:
 *           edges e_0..e_{d-1} of c in ascending edge id, variables v_i
 *           old_i = c2v[e_i];  m_i = post[v_i] - old_i                     (all i, before any write)
 *           new_0..new_{d-1} = the reference's check rule on m with the syndrome sign
 *           for i ascending:  post[v_i] = (post[v_i] - old_i) + new_i;  c2v[e_i] = new_i
 *       if check_lappr(post, synd): return (1, it+1, post)                 (decoder.pyx:431-433)
 *   return (0, max_iterations, post)
 *
 * post[v_i] in the update line is read again: a check that holds a variable twice (parallel
 * edges) updates it twice, the second edge from what the first left.  A frame that has stopped is
 * not touched again; max_iterations = 0 gives (0, 0, post) after the init line.
 * Schedule order: by (layer_of[c], c), where layer_of[c] is the smallest l >= 0 such that no check
 * c' < c with layer_of[c'] = l shares a variable with c (first-fit in ascending check id).  The
 * checks of one layer share no variable, so the order within a layer does not change a bit. */

/* The layers of a code: *n_layers, and layer_of[C] (or NULL). */
QR_API int qr_code_layers(const qr_code *code, int32_t *n_layers, int32_t *layer_of);

/* Device workspace (bytes) of qr_decode_layered_device at leading dim ld and max_iterations (edge
 * messages E*ld fp64 + per-frame flags).  A negative max_iterations is QR_EVALUE. */
QR_API int qr_decode_layered_workspace_size(const qr_code *code, int32_t ld, int32_t max_iterations, size_t *bytes);

/* The layered decode of B independent frames; layouts and error rules as qr_decode_batch_device
 * (0 < B <= ld, ld % 64 == 0, a 256-byte aligned workspace of at least the size above, no null
 * pointer; else QR_EVALUE before any launch), and a negative max_iterations is QR_EVALUE too.  A
 * code with a check degree above 16 is QR_EUNSUPPORTED before any launch.
 *   d_final [V][ld] fp64   the posteriors, updated in place while the decode runs; at the end the
 *                          final LAPPRs of the definition; the padding columns [B, ld) are not written
 *   d_success[B], d_iters[B]: the (success, iterations) pair of every frame.
 * One launch per non-empty (layer, check degree) in schedule order, then per iteration a syndrome
 * test of the posteriors and the status update, all on `stream`: the kernel boundary is the only
 * synchronisation between layers.  Asynchronous, no allocation, every data-dependent decision on
 * the device: capturable into a HIP graph (a linear one; no second stream). */
QR_API int qr_decode_layered_device(const qr_code *code, int32_t B, int32_t ld, const double *d_lappr,
                                    const uint8_t *d_synd, int32_t max_iterations, double *d_final, uint8_t *d_success,
                                    int32_t *d_iters, void *d_workspace, size_t workspace_bytes, void *stream);

/* The layered decode of B frames from host memory, frame-major: lappr[B][V], synd[B][C],
 * final[B][V]: copies to the handle's scratch, transposed there into ld = B rounded up to 64,
 * qr_decode_layered_device, transposed and copied back. */
QR_API int qr_decode_layered_host(const qr_code *code, int32_t B, const double *lappr, const uint8_t *synd,
                                  int32_t max_iterations, double *final_lappr, uint8_t *success, int32_t *iterations);

/* --------------------------------------------- Decoder unit-test surface */
/* Every *_host entry that takes n elements from host arrays follows one rule: a null handle is
 * QR_EVALUE; n < 0 is QR_EVALUE ("negative size"); n == 0 is QR_OK with no device call; a null
 * array with n > 0 is QR_EVALUE ("null pointer argument"). */
/* Decoder.check_lappr (decoder.pyx:235-281): per-check satisfied flags
 * (check_ok[C]) and the whole-word flag, for one frame, computed on the GPU.  A null lappr or
 * synd is QR_EVALUE (it used to be read); check_ok and all_ok may be null. */
QR_API int qr_check_lappr_host(const qr_code *code, const double *lappr, const uint8_t *synd, uint8_t *check_ok,
                        uint8_t *all_ok);
/* Decoder.check_synd_node / check_word (decoder.pyx:177-232) on a hard word.  A null word or
 * synd is QR_EVALUE (it used to be read). */
QR_API int qr_check_word_host(const qr_code *code, const uint8_t *word, const uint8_t *synd, uint8_t *check_ok,
                       uint8_t *all_ok);
/* Decoder.process_var_node (decoder.pyx:285-319) for a list of variable nodes:
 * updated[v] = lappr[v] + sum c2v[e]; v2c[e] = updated[v] - c2v[e].  n_nodes < 0 is QR_EVALUE
 * (it used to be QR_OK), and so is a null array with n_nodes > 0 (it used to be read). */
QR_API int qr_process_var_nodes_host(const qr_code *code, const int64_t *nodes, int64_t n_nodes, const double *lappr,
                              const double *c2v, double *v2c, double *updated);
/* Decoder.process_check_node (decoder.pyx:322-388) for a list of check nodes.  n_nodes < 0 is
 * QR_EVALUE (it used to be QR_OK), and so is a null array with n_nodes > 0 (it used to be read). */
QR_API int qr_process_check_nodes_host(const qr_code *code, const int64_t *nodes, int64_t n_nodes, const uint8_t *synd,
                                double *c2v, const double *v2c);

/* ------------------------------------------------------------ soft demap */
/* Replaces the hot-path part of NoiseMapper.__cinit__ (noisemapper.pyx:103-162)
 * for a PAMAlphabet (alphabet.pyx:35-76): constellation[M], probabilities[M]
 * (NULL = uniform), thresholds[M+1], noise_var > 0, sign_config[M] (NULL = zeros).
 * Computes F_Y_thresholds / delta_F_Y with the scipy-exact erf and uploads the
 * tables to `device`. */
QR_API int qr_demap_create(int32_t bit_per_symbol, const double *constellation, const double *probabilities,
                    const double *thresholds, double noise_var, const uint8_t *sign_config, int32_t device,
                    qr_demap **out);
QR_API int qr_demap_destroy(qr_demap *dm);
/* F_Y_thresholds[M+1], delta_F_Y[M] as the reference exposes them (noisemapper.pxd). */
QR_API int qr_demap_tables(const qr_demap *dm, double *F_Y_thresholds, double *delta_F_Y);

/* Batched NoiseMapper.demap_lappr_array (noisemapper.pyx:544-559) fused with the
 * LLR scaling of the softening pipeline (reconciliation.pyx:143-145):
 *   d_n [S][ld] fp64, d_j [S][ld] int64 (transmitted symbol index 0..M-1)
 *   d_lappr [S*bps][ld] fp64: d_lappr[(s*bps + k)*ld + f] = alpha * LAPPR of Gray bit k
 * i.e. directly the decoder's input layout (variable node v = s*bps + k).
 * Out-of-range symbol indices yield NaN LAPPRs. */
QR_API int qr_demap_batch_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *d_n,
                          const int64_t *d_j, double alpha, double *d_lappr, void *stream);
/* NoiseMapper.demap_lappr_array for one array from host memory: lappr[S*bps].  S < 0 is QR_EVALUE
 * (it used to be QR_OK), and so is a null array with S > 0 (it used to be read). */
QR_API int qr_demap_host(const qr_demap *dm, int64_t S, const double *n, const int64_t *j, double *lappr);

/* NoiseMapper.g_inv_search (noisemapper.pyx:310-345) over arrays, i.e.
 * NoiseMapper.demap_noise_search (noisemapper.pyx:407-419): y_hat[k] = the root of
 * F_Y(y) = target(n_hat[k], i[k]) by the reference's doubling bracket + bisection to
 * hi - lo <= y_accuracy (default 1e-9 in the reference).  Bit-identical to the
 * reference.  i[k] outside [0, M) gives NaN (out-of-bounds reads in the reference);
 * the bracket + bisection loops are capped at 2200 steps (NaN), where the reference
 * loops forever (targets outside [0, 1], y_accuracy below the spacing of the doubles
 * near the root).  Host arrays of n elements; synchronous. */
QR_API int qr_g_inv_search_host(const qr_demap *dm, int64_t n, const double *n_hat, const int64_t *i,
                                double y_accuracy, double *y_hat);
/* NoiseMapper.F_Y (noisemapper.pyx:264-275): F[k] = (sum_m F_Z(y[k], a_m, sigma)) / M, the
 * uniformly weighted mixture CDF (the cpdef ignores the alphabet's probabilities).  Host
 * arrays of n elements; synchronous. */
QR_API int qr_F_Y_host(const qr_demap *dm, int64_t n, const double *y, double *F);

/* -------------------------------- table-interpolated g_inv, formulation 1 */
/* The interpolation grid of NoiseMapper.__cinit__ (noisemapper.pyx:135-144), built on demand
 * in HBM: y_range = numpy.linspace(y_low, y_high, n_points) with the truncation rule of
 * :135-141 and n_points of :142 (`step` is the alphabet's, pa.step), F_Y_values = F_Y(y_range)
 * (:264-275, the function qr_F_Y_host computes).  Calling it again with the same three
 * parameters does nothing; other parameters rebuild the tables (synchronously: no launch that
 * reads them may be pending or captured).  QR_EVALUE unless trunkation_threshold > 0,
 * n_intervals_per_step > 0, step > 0 and 2 <= n_points <= 2^26.  Synchronous. */
QR_API int qr_demap_grid_create(qr_demap *dm, double trunkation_threshold, int64_t n_intervals_per_step, double step);
/* n_points (noisemapper.pyx:142) and whether F_Y_values is nondecreasing (checked in one pass
 * when the grid is built; the shortcut index search is used only then).  QR_EVALUE before
 * qr_demap_grid_create. */
QR_API int qr_demap_grid_info(const qr_demap *dm, int32_t *n_points, int32_t *nondecreasing);
/* NoiseMapper.y_range / F_Y_values (noisemapper.pyx:255-261): host arrays of n_points doubles
 * (either may be NULL). */
QR_API int qr_demap_grid_host(const qr_demap *dm, double *y_range, double *F_Y_values);
/* NoiseMapper.g_inv (noisemapper.pyx:295-307) over arrays, i.e. NoiseMapper.demap_noise
 * (:391-403): y_hat[k] = __interp(F_Y_values, y_range, target(n_hat[k], i[k])) with
 * __binsearch / __interp of :27-63.  Bit-identical to the reference; i[k] outside [0, M) gives
 * NaN (out-of-bounds reads in the reference).  Host arrays of n elements; synchronous. */
QR_API int qr_g_inv_host(const qr_demap *dm, int64_t n, const double *n_hat, const int64_t *i, double *y_hat);
/* NoiseMapper.demap_lappr_simplified_array ("Formulation 1", noisemapper.pyx:563-620) for one
 * array from host memory: lappr[S*bps], any bit_per_symbol.  Out-of-range symbol indices
 * yield NaN LAPPRs. */
QR_API int qr_demap_simplified_host(const qr_demap *dm, int64_t S, const double *n, const int64_t *j, double *lappr);
/* Batched NoiseMapper.demap_lappr_simplified_array (noisemapper.pyx:563-620) fused with the LLR
 * scaling (reconciliation.pyx:143-145); arguments, layouts and the NaN convention of
 * qr_demap_batch_device.  QR_EVALUE if the grid has not been created, QR_EUNSUPPORTED for
 * bit_per_symbol > 6.  The padding columns [B, ld) are not written. */
QR_API int qr_demap_simplified_batch_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *d_n,
                                            const int64_t *d_j, double alpha, double *d_lappr, void *stream);

/* ------------------------------ Monte-Carlo mutual information (estimator) */
/* The tables montecarlo_information reads beside the NoiseMapper's own
 * (mutual_information.pyx:218-224): p_xhat[M] = P_xhat(nm) (:29-39) and fwrd[M*M] =
 * nm.fwrd_transition_probability, row-major [x][x_hat] (noisemapper.pyx:166-182).  A synchronous
 * upload, like qr_demap_grid_create; calling it again replaces the values. */
QR_API int qr_demap_mi_tables(qr_demap *dm, const double *p_xhat, const double *fwrd);
/* Bytes of the per-sample term planes [3][S][ld] that qr_mi_montecarlo_device needs as workspace
 * when the caller does not ask for the terms.  QR_EVALUE unless ld % 64 == 0, ld > 0, S >= 1. */
QR_API int qr_mi_workspace_size(int32_t ld, int64_t S, size_t *bytes);
/* Batched montecarlo_information (mutual_information.pyx:245-297: the loop over the N samples and
 * the three divisions by N) on samples already drawn (:239-243 are the caller's), frame-innermost
 * with one "frame" per call of the reference, i.e. per block of S samples:
 *   d_x [S][ld] int64 (x_ind), d_y [S][ld] fp64 (y), B blocks in columns [0, B);
 *   Bob's x_hat = hard_decide_index(y) and n = map_noise(y, x_hat) (:242-243) are computed inside;
 *   d_info [3][ld] fp64: I(X;Xhat), I(X;Y), I(X,N;Xhat) of block f at d_info[q*ld + f];
 *   d_terms [3][S][ld] fp64 or NULL: the per-sample terms log2(...) of :259, :269, :295, summed in
 *     sample order into d_info; with NULL they live in d_workspace (qr_mi_workspace_size bytes).
 * which_mask bit q = which[q] of the reference: a quantity whose bit is clear is not computed, its
 * d_info is 0.0 / S and its term plane is not written.  Bit-identical to the reference for identical
 * inputs (glibc exp / log2, the interpolated g_inv and the searched g_inv_search at 1e-9).  An x
 * outside [0, M) gives NaN terms for that sample.  The padding columns [B, ld) are not written.
 * QR_EVALUE: S < 1 (the reference divides by zero), B < 1, B > ld, ld % 64 != 0, a null handle, the
 * grid (qr_demap_grid_create) or the tables (qr_demap_mi_tables) missing, a short workspace.
 * QR_EUNSUPPORTED for bit_per_symbol > 6.  Two launches on `stream`, asynchronous, no allocation,
 * capturable into a graph. */
QR_API int qr_mi_montecarlo_device(const qr_demap *dm, uint32_t which_mask, int32_t B, int32_t ld, int64_t S,
                                   const int64_t *d_x, const double *d_y, double *d_info, double *d_terms,
                                   void *d_workspace, size_t workspace_bytes, void *stream);
/* montecarlo_information (mutual_information.pyx:245-297) for one block of N samples from host
 * memory: x[N], y[N], which[3] (NULL = all three), out[3], terms [3][N] or NULL.  Synchronous. */
QR_API int qr_mi_montecarlo_host(const qr_demap *dm, int64_t N, const int64_t *x, const double *y,
                                 const uint8_t *which, double *out, double *terms);
/* out[k] = log2(x[k]) by the device's restatement of glibc's log2 (mutual_information.pyx:19), host
 * arrays of n elements, synchronous.  For tests.  Not a reference interface. */
QR_API int qr_log2_host(int64_t n, const double *x, double *out);

/* ------------------------------ LAPPR information rate (BICM generalised mutual information) */
/* What the LAPPRs carry to the bit-wise decoder, at A scales alpha of the LAPPRs at once.  Not a
 * reference interface; the definition is this library's and the results are bit-exact against it.
 * Per element v = s * bit_per_symbol + k (symbol s, level k), word bit w in {0, 1} and scale alpha:
 *   x = alpha * L, negated when w == 0;  m = x > 0 ? x : 0.0;
 *   t = m * 1.4426950408889634 + log2(1.0 + exp(-|x|)),
 * every operation rounded separately (no FMA), exp and log2 glibc's.  NaN gives NaN, x = +inf gives
 * +inf, x = -inf gives 0.0.  The sums: a chunk is QR_LAPPR_INFO_CHUNK consecutive symbols of one frame
 * and level, added from 0.0 in ascending s; loss[a][k][f] adds the frame's chunks from 0.0 in
 * ascending order; total[a][k] adds loss[a][k][f] from 0.0 over f = 0 .. B-1.  errors[k][f] counts the
 * elements whose decided bit (0 iff L >= 0, so NaN decides 1: utils.pyx:35-38, on the unscaled L)
 * differs from w; total_errors[k] is their sum over the frames.  The rate of level k at scale a is
 * 1 - total[a][k] / (B S) bits, the caller's division. */
#define QR_LAPPR_INFO_CHUNK 256
/* Bytes of the chunk sums qr_lappr_info_device needs as workspace.  QR_EVALUE unless bit_per_symbol
 * in 1..8, ld > 0, ld % 64 == 0, S >= 1, A in 1..16. */
QR_API int qr_lappr_info_workspace_size(int32_t bit_per_symbol, int32_t ld, int64_t S, int32_t A, size_t *bytes);
/* The batch, frame-innermost as the decoder takes it: d_lappr [S*bps][ld] fp64, d_word [S*bps][ld]
 * uint8, B frames in columns [0, B); alphas[A] in HOST memory (they travel as kernel arguments);
 * d_loss [A][bps][ld] fp64, d_errors [bps][ld] int32, d_total [A][bps] fp64, d_total_errors [bps]
 * int64.  The padding columns [B, ld) are neither read into any output nor written.
 * QR_EVALUE: bit_per_symbol outside 1..8, A outside 1..16, a scale that is not finite, S < 1, B < 1,
 * B > ld, ld % 64 != 0, a null pointer, a short workspace.  Two launches on `stream` of the current
 * device, asynchronous, no allocation, capturable into a graph. */
QR_API int qr_lappr_info_device(int32_t bit_per_symbol, int32_t B, int32_t ld, int64_t S, const double *d_lappr,
                                const uint8_t *d_word, int32_t A, const double *alphas, double *d_loss,
                                int32_t *d_errors, double *d_total, int64_t *d_total_errors, void *d_workspace,
                                size_t workspace_bytes, void *stream);
/* One frame from host memory in the reference's interleaved layout (lappr[S*bps], word[S*bps], element
 * s * bps + k), through the same kernels on GPU `device`: loss[A][bps] fp64, errors[bps] int64.
 * Synchronous. */
QR_API int qr_lappr_info_host(int32_t device, int32_t bit_per_symbol, int64_t S, const double *lappr,
                              const uint8_t *word, int32_t A, const double *alphas, double *loss, int64_t *errors);

/* ------------------------------ sampled density evolution of a code ensemble */
/* Whether a degree distribution decodes an empirical LLR density (the softened LAPPRs at a scale
 * alpha, say) within T iterations: the decoder's arithmetic applied to random draws from populations of
 * M messages instead of to a graph.  Not a reference interface; the definition is this library's and the
 * results are bit-exact against it.  All arithmetic is IEEE fp64, every operation rounded separately (no
 * FMA), exp and log glibc's as in the decoder.
 *
 * Random indices, counter-based (uint64, wrapping):
 *   mix(x):  x = (x ^ x>>30) * 0xBF58476D1CE4E5B9;  x = (x ^ x>>27) * 0x94D049BB133111EB;  return x ^ x>>31
 *   ctr(t, phase, j, k) = ((t*4 + phase) * 2^32 + j) * 512 + k
 *   z = mix(seed + 0x9E3779B97F4A7C15 * (ctr + 1))
 *   rnd(t, phase, j, k, n) = ((z >> 32) * n) >> 32            for 1 <= n < 2^31
 * (with seed 0, ctr = 0, 1, 2 give SplitMix64's first outputs 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4,
 * 0x06C45D188009454F).
 *
 * Inputs: a channel population u[Mu] of signed LAPPRs (u > 0: correct); the ensemble's degree tables
 * edge_vdeg[Ne], edge_cdeg[Ne] (per edge of a multiset of edges, the degree of its variable and of its
 * check: the edge perspective) and node_vdeg[Nv] (per variable: the node perspective; 0 is an isolated
 * variable); the population size M, the iterations T, a 64-bit seed.  Variable degrees 1..255 (node_vdeg
 * 0..255), check degrees 2..255; Mu, Ne, Nv in [1, 2^31), M in [1, 2^30], T in [0, 10000].
 *
 * c2v(0)[j] = +0.0 for every j.  For t = 1..T and every j in [0, M):
 *   phase 0 (variable):  d = edge_vdeg[rnd(t,0,j,0,Ne)];   s = u[rnd(t,0,j,1,Mu)]
 *                        for k = 0 .. d-2 ascending:  s = s + c2v(t-1)[rnd(t,0,j,2+k,M)]
 *                        v2c(t)[j] = s
 *   phase 1 (check):     d = edge_cdeg[rnd(t,1,j,0,Ne)];   F = v2c(t)[rnd(t,1,j,2,M)]
 *                        for k = 1 .. d-2 ascending:  F = box_plus(F, v2c(t)[rnd(t,1,j,2+k,M)])
 *                        c2v(t)[j] = F
 * box_plus is the reference's (decoder.pyx:41-45) in its operand order, F the first operand; no syndrome
 * sign (the population is already signed).  For t = 0..T, phase 2 is the decision of
 * count_errors_from_lappr (lappr >= 0 is correct; NaN counts as an error):
 *   d = node_vdeg[rnd(t,2,j,0,Nv)];   p = u[rnd(t,2,j,1,Mu)]
 *   for k = 0 .. d-1 ascending:  p = p + c2v(t)[rnd(t,2,j,2+k,M)]
 *   errors[t] = #{ j : !(p >= 0) }
 * Outputs: errors[T+1] int64 and the populations v2c(T)[M], c2v(T)[M]; for T = 0 v2c is not written and
 * c2v is all +0.0.
 *
 * Limitation: the bit levels are mixed i.i.d. over the variables (the usual BICM approximation); which
 * level sits on which variable of an irregular code is not modelled. */
typedef struct qr_de_tables qr_de_tables; /* an ensemble's three degree tables in HBM */
/* The tables from host arrays: every degree validated on the host (QR_EVALUE: Ne or Nv outside [1, 2^31),
 * a variable degree outside 1..255, a node degree outside 0..255, a check degree outside 2..255, a null
 * pointer; all before any device call), uploaded once to GPU `device`. */
QR_API int qr_de_tables_create(int32_t device, int64_t Ne, const int32_t *edge_vdeg, const int32_t *edge_cdeg,
                               int64_t Nv, const int32_t *node_vdeg, qr_de_tables **out);
QR_API int qr_de_tables_destroy(qr_de_tables *tables);
/* Signed population from a batch: for row r and frame f < B of the decoder's frame-innermost [rows][ld]
 * arrays, x = alpha * d_lappr[r][f] (one rounding) and d_u[r * B + f] = x where d_word[r][f] == 0, x with
 * its sign bit flipped otherwise (NaN keeps its payload).  The padding columns [B, ld) are not read.
 * QR_EVALUE: B < 1, B > ld, ld % 64 != 0, rows < 1, rows * B >= 2^31, an alpha that is not finite, a null
 * pointer.  One launch on `stream` of the current device, asynchronous. */
QR_API int qr_de_population_device(int32_t B, int32_t ld, int64_t rows, const double *d_lappr, const uint8_t *d_word,
                                   double alpha, double *d_u, void *stream);
/* The evolution above on the tables' device: d_u [Mu], d_v2c [M], d_c2v [M] fp64, d_errors [T+1] int64.
 * It clears d_c2v and d_errors (hipMemsetAsync), then 1 + 3T launches on `stream`; asynchronous, no
 * allocation, no workspace, capturable into a graph.  QR_EVALUE, before any launch and with no output
 * written: Mu outside [1, 2^31), M outside [1, 2^30], T outside [0, 10000], a null pointer. */
QR_API int qr_de_evolve_device(const qr_de_tables *tables, int64_t Mu, const double *d_u, int64_t M, int32_t T,
                               uint64_t seed, double *d_v2c, double *d_c2v, int64_t *d_errors, void *stream);
/* The same from host arrays on GPU `device` (the tables as qr_de_tables_create takes them): synchronous
 * copies around qr_de_evolve_device, for one-off use and tests.  v2c is left alone when T == 0. */
QR_API int qr_de_evolve_host(int32_t device, int64_t Ne, const int32_t *edge_vdeg, const int32_t *edge_cdeg, int64_t Nv,
                             const int32_t *node_vdeg, int64_t Mu, const double *u, int64_t M, int32_t T, uint64_t seed,
                             double *v2c, double *c2v, int64_t *errors);

/* The arithmetic primitives of the bit-exact paths (glibc exp / log, the box-plus built from them,
 * cephes erf, the demapper's division by 2 sigma^2), evaluated on the device element by element:
 * out[k] = fn(a[k]) or fn(a[k], b[k]), host arrays of n elements, synchronous, on the caller's current
 * device.  For tests (tests/test_gpu_device_math.py).  Not a reference interface.
 *
 * Each fn is one kernel that calls the device function as the product kernels call it; `variant` names
 * the table home (and GlibcK form) of a product call site:
 *   QR_MATH_HOME_SWEEP   GlibcTablesBP in LDS, staged from a code handle's table (built on the host by
 *                        build_glibc_tables), GlibcK::pinned(): the check sweeps (decoder.hip
 *                        check_block / check_exact, the runtime-degree sweep), the frame-resident decode
 *                        (decode_small.hip) and the few-frame decode (decode_few.hip)
 *   QR_MATH_HOME_NODE    GlibcTables in LDS from the same table, default GlibcK: k_check_nodes
 *                        (decode_api.hip, qr_process_check_nodes_host)
 *   QR_MATH_HOME_CONST   the __constant__ kGlibcConst read in place: k_direct_lappr (demap.hip), erfc_ge1
 *                        (qamr_math.hpp), the per-symbol formulation-1 demapper (demap_interp.hip), the
 *                        polar Box-Muller of npstream.hip
 *   QR_MATH_HOME_EXPLOG  GlibcExpLog in LDS, staged from kGlibcConst: k_demap_wave (demap.hip) and the
 *                        wave formulation-1 demapper (demap_interp.hip)
 *   QR_MATH_HOME_DEMAP   GlibcTables in LDS, staged from kGlibcConst: k_demap / demap_symbol
 *   QR_MATH_HOME_MI      {exp table, log2 table} in LDS, copied from kGlibcConst: k_mi_terms, k_mi_quad
 * and the homes each fn accepts (any other is QR_EVALUE):
 *   EXP (g_exp, |a| < 512 or NaN; no product call site of its own)        NODE, CONST
 *   EXP_NEG (g_exp_neg, a in [-37.51, 0] or NaN), LOG_U, LOG_U_SEL (a in [1, 2] or NaN),
 *   H_STRICT, H_STRICT_SEL (h_strict<false / true>, any a),
 *   BOX_PLUS, BOX_PLUS_SEL (box_plus_strict_t<false / true>(a, b))       SWEEP, NODE
 *   EXP_FULL, LOG_FULL (any a), LOG (g_log, a positive normal; reached through g_log_full)
 *                                                                         CONST, EXPLOG, DEMAP
 *   EXP_WAVE (g_exp_wave, any a; wavefront w holds elements [64 w, 64 w + 64))   EXPLOG, MI
 *   ERF (cephes_erf, any a; its erfc branch reads kGlibcConst)            CONST
 *   DIV_TWO_S2 (a / b by div_two_s2 with two_s2 = b[k], inv_two_s2 = RN(1 / b[k]) formed on the host as
 *     the demapper's tables form it)                                      CONST
 *   H_PACKED (strict_pack.hpp h_packed<clamp>, nj arguments per lane, home SWEEP -- its only call sites):
 *     variant = clamp * 8 + (nj - 1), clamp 0 = kClampNone, 1 = kClampFull, 2 = kClampFinite, nj 1..8;
 *     wavefront w holds elements [64 nj w, 64 nj (w + 1)), argument j of lane l at 64 nj w + 64 j + l;
 *     out[k] = h(|a[k]|) = log(1.0 + exp(-|a[k]|)).
 * Lanes past n run along on the argument 1.0 and store nothing.  b is read by BOX_PLUS, BOX_PLUS_SEL
 * and DIV_TWO_S2 only (NULL otherwise).  QR_EVALUE: an unknown fn or variant, n < 0, a null array with
 * n > 0; n == 0 is QR_OK before any device call. */
enum {
    QR_MATH_EXP = 0, QR_MATH_EXP_NEG, QR_MATH_EXP_FULL, QR_MATH_EXP_WAVE, QR_MATH_LOG, QR_MATH_LOG_U, QR_MATH_LOG_U_SEL,
    QR_MATH_LOG_FULL, QR_MATH_H_STRICT, QR_MATH_H_STRICT_SEL, QR_MATH_BOX_PLUS, QR_MATH_BOX_PLUS_SEL, QR_MATH_ERF,
    QR_MATH_DIV_TWO_S2, QR_MATH_H_PACKED
};
enum {
    QR_MATH_HOME_SWEEP = 0, QR_MATH_HOME_NODE, QR_MATH_HOME_CONST, QR_MATH_HOME_EXPLOG, QR_MATH_HOME_DEMAP,
    QR_MATH_HOME_MI
};
QR_API int qr_math_eval_host(int32_t fn, int32_t variant, int64_t n, const double *a, const double *b, double *out);

/* ------------------------------ quad-integrated mutual information */
/* mutual_information_base_scheme (mutual_information.pyx:123-148, kind 0: the integral of
 * mutual_information_base_scheme_arg, :43-119, over [0, 1]) and mutual_information_X_Y (:202-208, kind 1:
 * the integral of mutual_information_X_Y_int_arg, :175-199, over (-inf, inf)) as scipy.integrate.quad
 * computes them: QUADPACK's QAGS / QAGI restated operation by operation, the integrands evaluated on
 * the GPU with glibc's exp / log2 and the interpolated g_inv.  P integrals ("problems") in one call:
 *   dms [P]: the problem's demapper (all of one bit_per_symbol <= 6 and one device, each with its grid,
 *     qr_demap_grid_create; the same handle may appear many times);
 *   p_xhat [P][M] (host; kind 0 only, NULL otherwise): P_xhat of each problem (:29-39);
 *   sign_cfg [P][M] (host) or NULL: each problem's sign configuration instead of its handle's (it enters
 *     only g_inv's target, noisemapper.pyx:297-307, so one handle per noise variance serves every
 *     configuration);
 *   epsabs, epsrel, limit: quad's arguments (its defaults: 1.49e-8, 1.49e-8, 50);
 *   result, abserr, neval, ier [P] (host): quad's I, its error estimate, infodict["neval"], and QUADPACK's
 *     ier; any non-zero ier is one of the cases in which scipy warns (6 also for QUADPACK's own refusal
 *     of epsabs <= 0 with epsrel < max(50 eps, 0.5e-28)).
 * Bit-identical to the reference for identical inputs, the integrals it returns as -inf included; a
 * problem's results do not depend on what else is in the batch.  Round r evaluates the pending rule(s)
 * of every unfinished problem in one launch on `stream` and copies 8 doubles per problem back; the
 * integrator's decisions are taken on the calling thread in between, so the call is synchronous, ends
 * after at most `limit` rounds, allocates its device buffers itself and cannot be captured into a graph.
 * QR_EVALUE: P < 0, limit < 1, a kind other than 0 / 1, a null handle or output, handles of different
 * bit_per_symbol or device, a missing grid, kind 0 without p_xhat.  QR_EUNSUPPORTED for
 * bit_per_symbol > 6. */
QR_API int qr_mi_quad_batch(const qr_demap *const *dms, const double *p_xhat, const uint8_t *sign_cfg, int32_t P,
                            int32_t kind, double epsabs, double epsrel, int32_t limit, double *result, double *abserr,
                            int32_t *neval, int32_t *ier, void *stream);
/* out[5] = {rounds, launches, work items, ns of host bookkeeping, ns in all} of the calling thread's last
 * qr_mi_quad_batch.  For measurement.  Not a reference interface. */
QR_API int qr_mi_quad_stats(int64_t *out);
/* The integrands themselves over arrays: f[k] = mutual_information_base_scheme_arg(x[k], nm, p_Xhat)
 * (kind 0; p_Xhat as given to qr_demap_mi_tables) or mutual_information_X_Y_int_arg(x[k], nm) (kind 1),
 * with the handle's own sign configuration.  Device arrays, one launch on `stream`, asynchronous,
 * capturable; the host version copies in, launches once and copies out.  The grid must exist. */
QR_API int qr_mi_integrand_device(const qr_demap *dm, int32_t kind, int64_t n, const double *d_x, double *d_f,
                                  void *stream);
QR_API int qr_mi_integrand_host(const qr_demap *dm, int32_t kind, int64_t n, const double *x, double *f);
/* One work item of the batch's kernel with its debug pointer, for tests: the rule(s) of `nh` (1 or 2)
 * intervals [a[h], b[h]] of one problem (kind 0: the 21-point rule on the interval; kind 1: the
 * transformed 15-point rule, the interval within (0, 1]); p_xhat [M] (host, kind 0), sign_cfg [M] or NULL.
 * sums [nh][4] = {result, |(resk - resg) hlgth|, resabs, resasc} as the kernel leaves them (the pow step of
 * the error estimate is the host's); nodes [nh][21][2] (kind 0) or [nh][30][2] (kind 1), or NULL: each lane's
 * {abscissa, integrand value}, kind 0 in node order (the centre, the 10 nodes below it outermost first, the
 * 10 above it), kind 1 as pairs (+T, -T) per node.  Synchronous.  Not a reference interface. */
QR_API int qr_mi_quad_rule_host(const qr_demap *dm, const double *p_xhat, const uint8_t *sign_cfg, int32_t kind,
                                int32_t nh, const double *a, const double *b, double *sums, double *nodes);
/* The integrator alone over a C callback, on the host (no device call), for tests: kind 0 is
 * quad(f, a, b), kind 1 quad(f, -inf, inf) (a, b ignored); `last` is infodict["last"].  Outputs may be
 * NULL.  QR_EVALUE for a null f, limit < 1 or another kind.  Not a reference interface. */
typedef double (*qr_quad_fn)(double x, void *user);
QR_API int qr_quad_host(qr_quad_fn f, void *user, int32_t kind, double a, double b, double epsabs, double epsrel,
                        int32_t limit, double *result, double *abserr, int32_t *neval, int32_t *ier, int32_t *last);

/* ---------------------------------------------- softening pipeline (Bob) */
/* NoiseMapper.hard_decide_index + map_noise (noisemapper.pyx:349-388) and
 * PAMAlphabet.demap_symbols_to_bits (alphabet.pyx:98-107), fused, frame-innermost:
 *   d_y[S][ld] -> d_xhat[S][ld] int64, d_nhat[S][ld] fp64, d_word[S*bps][ld] uint8 */
QR_API int qr_bob_map_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *d_y, int64_t *d_xhat,
                      double *d_nhat, uint8_t *d_word, void *stream);
/* NoiseMapper.map_noise (noisemapper.pyx:373-388) with caller-given indices:
 * d_nhat[s][f] = g(d_y[s][f], d_index[s][f]) (noisemapper.pyx:289-292). */
QR_API int qr_map_noise_device(const qr_demap *dm, int32_t B, int32_t ld, int64_t S, const double *d_y,
                               const int64_t *d_index, double *d_nhat, void *stream);
/* PAMAlphabet.demap_symbols_to_bits (alphabet.pyx:98-107): d_x[S][ld] -> d_word[S*bps][ld]
 * (padding frames f in [B, ld) get the bits of symbol 0). */
QR_API int qr_symbols_to_bits_device(int32_t bit_per_symbol, int32_t B, int32_t ld, int64_t S, const int64_t *d_x,
                                     uint8_t *d_word, void *stream);
/* Direct reconciliation LAPPRs (sims/reconciliation.pyx:25-51, _y_to_lappr_grey):
 * d_y[S][ld] -> d_lappr[S*bps][ld], two_variance = 2 * noise variance. */
QR_API int qr_direct_lappr_device(const qr_demap *dm, double two_variance, int32_t B, int32_t ld, int64_t S,
                                  const double *d_y, double *d_lappr, void *stream);
/* Hard reverse reconciliation LAPPRs (noisemapper.pyx:423-432, bare_llr):
 * d_lappr[(s*bps+k)][f] = d_table[x * bps + k] with the device table[M][bps]. */
QR_API int qr_bare_llr_device(int32_t bit_per_symbol, const double *d_table, int32_t B, int32_t ld, int64_t S,
                              const int64_t *d_x, double *d_lappr, void *stream);
/* Matrix.eval_syndrome (matrix.pyx:55-60): d_word[V][ld] -> d_synd[C][ld]. */
QR_API int qr_syndrome_device(const qr_code *code, int32_t B, int32_t ld, const uint8_t *d_word, uint8_t *d_synd,
                       void *stream);
/* count_errors_from_lappr (utils.pyx:27-40) over the first K variable nodes of
 * every frame plus the frame bookkeeping of simulate_softening_snr_dB
 * (reconciliation.pyx:149-157), accumulated into d_counters (int64[5], not
 * cleared): {bit_errors, frame_errors, successes, iteration_sum_of_successes, frames}.
 * d_frame_errors[B] (int32) receives the per-frame bit-error counts. */
QR_API int qr_count_errors_device(int32_t B, int32_t ld, int64_t K, const double *d_final, const uint8_t *d_word,
                           const uint8_t *d_success, const int32_t *d_iters, int32_t *d_frame_errors,
                           int64_t *d_counters, void *stream);

/* ------------------------------------------------------- rate adaptation */
/* Rate adaptation of one mother code (puncturing, shortening, blind rounds).  Not a reference
 * interface: the definition is this library's (qamr/rate_adapt.py expand_host states it on the host).
 * Of the V variables, n carry the payload, s are shortened and p are punctured; d_slot int32[V] says
 * which: d_slot[v] = k >= 0 makes v payload row k (0 <= k < n), d_slot[v] = -1 - j makes it filler j
 * (j < s shortened, s <= j < s + p punctured).  With the frame-innermost d_lappr_pay [n][ld],
 * d_word_pay [n][ld], d_fill [p + s][ld] (bits, any non-zero byte is 1) and d_revealed_or_null
 * int32[ld] (absent: 0 for every frame), for every frame f < B:
 *   payload row k : d_lappr[v][f] = d_lappr_pay[k][f] and d_word[v][f] = d_word_pay[k][f], bit for
 *                   bit (NaN payloads, +-inf and -0.0 are kept);
 *   filler j      : d_word[v][f] = d_fill[j][f] != 0; the filler is known iff
 *                   j < s + max(d_revealed[f], 0) (any count >= p discloses everything); a known filler
 *                   takes +L for bit 0 and -L for bit 1, an unknown one +0.0.
 * L is the LAPPR of a disclosed bit and must be finite: box_plus(inf, inf) is NaN in the reference's
 * arithmetic (|a - b| is NaN), and a decode with +-inf at the shortened positions returns NaN for
 * every LAPPR of every frame.  QR_SHORTENED_LAPPR = 1e300 is the value the reference itself uses for
 * a certain bit (noisemapper.pyx:218), and box_plus(1e300, 1e300) is 1e300.
 * One launch on `stream`, asynchronous, allocates nothing, capturable; only columns [0, B) of
 * d_lappr [V][ld] and d_word [V][ld] are written.  The LAPPR arrays must be 16-byte aligned, the bit
 * arrays 8-byte aligned.  QR_EVALUE before the device is touched: a null pointer (other than
 * d_revealed_or_null), a misaligned array, B < 1, B > ld, ld % 64 != 0, n + p + s != V, n < 1, p < 0,
 * s < 0, L not finite or <= 0. */
#define QR_SHORTENED_LAPPR 1e300
QR_API int qr_rate_adapt_expand_device(int64_t V, int64_t n, int64_t p, int64_t s, const int32_t *d_slot, int32_t B,
                                       int32_t ld, const double *d_lappr_pay, const uint8_t *d_word_pay,
                                       const uint8_t *d_fill, const int32_t *d_revealed_or_null, double L,
                                       double *d_lappr, uint8_t *d_word, void *stream);
/* qr_count_errors_device over the rows d_rows int32[n_rows] of the [V][ld] arrays in place of the
 * first K (a rate-adapted frame's payload rows): the same decision rule (utils.pyx:27-40: a NaN
 * decides 1), per-frame counts and five counters, accumulated the same way; with d_rows = 0..K-1 its
 * outputs are qr_count_errors_device's.  QR_EVALUE for a null pointer, a bad B / ld, n_rows < 0. */
QR_API int qr_count_errors_rows_device(int32_t B, int32_t ld, int64_t n_rows, const int32_t *d_rows,
                                       const double *d_final, const uint8_t *d_word, const uint8_t *d_success,
                                       const int32_t *d_iters, int32_t *d_frame_errors, int64_t *d_counters,
                                       void *stream);

/* ------------------------------------ code evaluation on a binary channel */
/* The decoder's input of sims/sim_decode.py and sims/sim_direct.py, frame-innermost:
 * d_word[V][ld] (bits), d_z[V][ld] (standard normal draws) -> d_llr[V][ld], columns [0, B) only.
 *   hard == 0 (sim_decode.py:98-100): coef * ((1 - 2 w) + vsqrt * z), coef = 2 alpha / v;
 *   hard != 0 (:69-71): coef * sign((1 - 2 w) + vsqrt * z), coef = LLR0, sign as numpy.sign
 *     (-1, 0, +1, NaN for NaN, +0.0 for -0.0).
 * Every operation is rounded on its own and the last one is a multiply, so coef = inf against a
 * zero gives NaN as in the reference.  One launch on `stream`, asynchronous, allocates nothing,
 * capturable.  QR_EVALUE: a null pointer, B < 1, B > ld, ld % 64 != 0, V < 1. */
QR_API int qr_biawgn_llr_device(int32_t hard, double coef, double vsqrt, int32_t B, int32_t ld, int64_t V,
                                const uint8_t *d_word, const double *d_z, double *d_llr, void *stream);
/* The decoder's input of sims/sim_bsc.py:58-61: d_llr = coef * (1 - 2 (w ^ (u < rber))) with
 * d_u[V][ld] uniform draws in [0, 1) and coef = log2(1 - rber) - log2(rber); d_rx_or_null[V][ld],
 * when given, receives the channel's output bits w ^ (u < rber).  Same layout, checks and launch
 * properties as qr_biawgn_llr_device. */
QR_API int qr_bsc_llr_device(double coef, double rber, int32_t B, int32_t ld, int64_t V, const uint8_t *d_word,
                             const double *d_u, double *d_llr, uint8_t *d_rx_or_null, void *stream);
/* qr_count_errors_device with the decision rule of sim_decode.py:80 and sim_bsc.py:66: a bit is 1
 * iff its final LAPPR is < 0, so a NaN decides 0 (count_errors_from_lappr decides 1 for it).  Same
 * arguments, outputs and counters; K = V counts every bit (the BSC script).  QR_EVALUE for a null
 * pointer as well. */
QR_API int qr_count_errors_neg_device(int32_t B, int32_t ld, int64_t K, const double *d_final, const uint8_t *d_word,
                                      const uint8_t *d_success, const int32_t *d_iters, int32_t *d_frame_errors,
                                      int64_t *d_counters, void *stream);

/* ---------------------------------------------------------- numpy's stream */
/* numpy's legacy global stream (np.random.seed / get_state: MT19937, random_sample, choice with p,
 * the polar legacy_gauss) continued on the GPU, bit for bit and in numpy's consumption order.  The
 * state is np.random.get_state()'s: key[624] (the untempered current block), pos (0..624; 624 =
 * regenerate before the next word), has_gauss and the cached normal.  Every call below draws from
 * the handle's state and moves it; each one SYNCHRONISES the host with `stream` (the state after a
 * call is read back from the device) and therefore cannot be captured into a graph.  Calls on one
 * handle are serialised.  QR_EVALUE for null pointers and negative counts; a count of 0 is QR_OK
 * and draws nothing. */
QR_API int qr_npstream_create(const uint32_t *key, int32_t pos, int32_t has_gauss, double gauss, int32_t device,
                              qr_npstream **out);
QR_API int qr_npstream_destroy(qr_npstream *st);
/* The current state; any output pointer may be null.  gauss is 0.0 when has_gauss is 0. */
QR_API int qr_npstream_state(const qr_npstream *st, uint32_t *key, int32_t *pos, int32_t *has_gauss, double *gauss);
/* d_out[n]: the next n words (np.random.bytes(4n) as '<u4'), the next n doubles
 * (np.random.random_sample(n), two words each), the next n normals (np.random.randn(n): the cached
 * value first when has_gauss; an odd count leaves one cached), the next n symbols
 * (np.random.choice(M, size=n, p=p) with d_cdf[M] = p.cumsum() / p.cumsum()[-1] formed by the
 * caller in numpy: the count of d_cdf[k] <= u; the cache is not touched; 2 <= M <= 256). */
QR_API int qr_npstream_words_device(qr_npstream *st, int64_t n, uint32_t *d_out, void *stream);
QR_API int qr_npstream_random_sample_device(qr_npstream *st, int64_t n, double *d_out, void *stream);
QR_API int qr_npstream_standard_normal_device(qr_npstream *st, int64_t n, double *d_out, void *stream);
QR_API int qr_npstream_choice_device(qr_npstream *st, int64_t n, int32_t M, const double *d_cdf, int64_t *d_out,
                                     void *stream);
/* B frames of sims/reconciliation.pyx:129-132 in sequence, frame f in column f: per frame
 * x = np.random.choice(M, size=S, p=p), then y = a[x] + sigma * np.random.randn(S) (the product
 * first, then the sum).  d_x int64 [S][ld], d_y float64 [S][ld], columns B..ld-1 written as zeros;
 * d_frame_words int64 [B]: the words consumed through frame f, cumulative.  The workspace (256-byte
 * aligned, qr_npstream_frames_workspace_size bytes, linear in B * S: about 28 bytes per symbol)
 * holds the generated words, and qr_npstream_seek_frame reads it: keep it unchanged until the seek.
 * The first generated range is the mean consumption plus a slack ("np_slack_pct"); when the frames
 * need more, the range is extended and the frames are located again, at most 8 times, then
 * QR_EINTERNAL.  QR_EVALUE before any launch for a null pointer, B <= 0, ld % 64 != 0, ld < B,
 * S <= 0, M outside 2..256, a short or misaligned workspace, or B * S past 2^31 candidate pairs
 * (split the batch). */
QR_API int qr_npstream_frames_workspace_size(int64_t S, int32_t B, size_t *bytes);
QR_API int qr_npstream_frames_device(qr_npstream *st, int32_t B, int32_t ld, int64_t S, int32_t M, const double *d_cdf,
                                     const double *d_constellation, double sigma, int64_t *d_x, double *d_y,
                                     int64_t *d_frame_words, void *d_workspace, size_t workspace_bytes, void *stream);
/* The state becomes the one after frame w (0-based) of the last qr_npstream_frames_device call on
 * this handle: where a sequential loop that stopped after that frame leaves numpy.  QR_EVALUE when
 * w is no frame of it or another draw was made since. */
QR_API int qr_npstream_seek_frame(qr_npstream *st, int32_t w);

/* --------------------------------------------------------- layout helpers */
/* Frame-major [B][n] <-> frame-innermost [n][ld] transposes on the device. */
QR_API int qr_to_frame_innermost_f64(int32_t B, int32_t ld, int64_t n, const double *d_src, double *d_dst, void *stream);
QR_API int qr_to_frame_major_f64(int32_t B, int32_t ld, int64_t n, const double *d_src, double *d_dst, void *stream);
QR_API int qr_to_frame_innermost_u8(int32_t B, int32_t ld, int64_t n, const uint8_t *d_src, uint8_t *d_dst, void *stream);
QR_API int qr_to_frame_innermost_i64(int32_t B, int32_t ld, int64_t n, const int64_t *d_src, int64_t *d_dst, void *stream);

/* ------------------------------------------------------------ measurement */
/* Streaming device copy (4 x 16 B per lane in flight, grid-stride): the practical HBM ceiling
 * the decoder's roofline is related to in bench.py. bytes % 16 == 0,
 * 16-B aligned pointers.  Not a reference interface. */
QR_API int qr_stream_copy(const void *d_src, void *d_dst, int64_t bytes, void *stream);

/* Shader-clock probe: n one-wave workgroups, each spinning (scalar only, s_sleep) for
 * `realtime_ticks` of the 100 MHz constant clock and writing {shader cycles, realtime
 * ticks} to d_out[2i], d_out[2i+1].  Launched on a side stream while the decode runs, it
 * reads the clock the chip holds under that load without a profiler attached
 * (MI355X_MICROARCH.md "DVFS give-back" item 6).  Not a reference interface. */
QR_API int qr_clock_probe(int64_t *d_out, int32_t n, int64_t realtime_ticks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QAMR_H */
