// npstream.hip -- numpy's legacy global stream on the GPU: MT19937 words, random_sample, choice with
// p and the polar legacy_gauss, consumed in numpy's order across a batch of frames
// (sims/reconciliation.pyx:129-132: per frame np.random.choice(M, size=S, p=p), then
// np.random.randn(S)); DESIGN.md "numpy's stream on the GPU".
//
// Everything is consumed in doubles (two words each): a frame takes S doubles for its symbols, then
// two per candidate pair of the polar method until it has its normals, so a frame's first double
// depends on how many candidates every earlier frame rejected.  Four steps, the launch boundary
// the only synchronisation between workgroups, every loop bounded by a count known at launch:
//   np_words  state -> whole blocks of tempered words in HBM (one workgroup: the recurrence)
//   np_scan   the accept flag of the candidate (k, k + 1) at every double position k, and the
//             exclusive prefix counts of the flags per parity class of k (sums, scan of sums, add)
//   np_chain  one wave, frames in order: where each frame starts and whether it enters with a
//             cached normal; the last accept of a frame is a select on the prefix counts
//   np_fill   symbols and normals of every (frame, position) in parallel, frame-innermost
#include <algorithm>

#include "qamr_internal.hpp"
#include "debug_check.hpp"
#include "npstream_host.hpp"

namespace qr {

std::atomic<int> g_np_slack_pct{100};  // tuning knob "np_slack_pct" (decode_api.hip)

// debug_check.hpp: the site numbers are one list across the units
enum NpDebugSite {
    kNpSiteWord = 20,    // a word index outside the generated blocks
    kNpSitePrefix = 21,  // a prefix-count or block-sum index outside its array
    kNpSiteChain = 22,   // the chain's select left its bracket or the range
    kNpSiteOut = 23,     // an output index outside [rows, ld)
    kNpSiteRank = 24,    // an accepted candidate's rank outside its frame's pairs
};

constexpr int kNpThreads = 256;
constexpr int kNpPer = 4;                         // class entries per thread of a scan workgroup
constexpr int kNpTile = kNpThreads * kNpPer;      // class entries per scan workgroup
constexpr int64_t kNpWindow = 2048;               // half width of the chain's first bracket

// The generated range as the kernels see it: words[0, nwords) are whole blocks, block 0 the one
// the stream stood in; double k is made of words w0 + 2k and w0 + 2k + 1, k < nd; the candidate of
// class q (the parity of k) and class index i is k = 2i + q, i < nc (so that k + 1 < nd).
struct NpRange {
    const uint32_t *words;
    int64_t nwords;
    int64_t w0, nd, nc;
    uint32_t *pref[2];  // [nc + 1] each: accepts among class entries [0, i); [nc] = all of them
    uint32_t *bsum;     // [2][nb] tile sums, then tile offsets
    int64_t nb;
};

__host__ __device__ __forceinline__ int64_t np_min(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int64_t np_max(int64_t a, int64_t b) { return a > b ? a : b; }

__device__ __forceinline__ double np_double(const NpRange &r, int64_t k) {
    const int64_t w = r.w0 + 2 * k;
    QR_DCHECK(k >= 0 && w + 1 < r.nwords, kNpSiteWord, w, r.nwords);
    const uint32_t a = r.words[w], b = r.words[w + 1];
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

// legacy_gauss's candidate from doubles k and k + 1
struct NpPair {
    double x1, x2, r2;
    __device__ __forceinline__ bool accept() const { return !(r2 >= 1.0 || r2 == 0.0); }
};
__device__ __forceinline__ NpPair np_pair(const NpRange &r, int64_t k) {
#pragma clang fp contract(off)
    NpPair p;
    p.x1 = 2.0 * np_double(r, k) - 1.0;
    p.x2 = 2.0 * np_double(r, k + 1) - 1.0;
    p.r2 = p.x1 * p.x1 + p.x2 * p.x2;
    return p;
}

// ------------------------------------------------------------------ np_words
// key: the untempered block the stream stands in (in), the last block generated (out).  Block b of
// `out` is the tempered key itself when first_is_key and b == 0, else the next block of the
// recurrence new[i] = x[i + 397 mod 624] ^ twist(old[i], x[i + 1]), x the new value where it exists:
// i < 227 reads old values only, 227 <= i < 454 the new [0, 227), 454 <= i < 624 the new [227, 397)
// and, at i = 623, new[0].  Three phases of at most 227 lanes, two LDS copies, a barrier after each.
__global__ void __launch_bounds__(kNpThreads) k_np_words(uint32_t *__restrict__ key, uint32_t *__restrict__ out,
                                                         int64_t nblocks, int first_is_key, int64_t cap_words) {
    __shared__ uint32_t s[2][kMtN];
    const int t = threadIdx.x;
    for (int i = t; i < kMtN; i += kNpThreads) s[0][i] = key[i];
    __syncthreads();
    int cur = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        if (b > 0 || !first_is_key) {
            const uint32_t *o = s[cur];
            uint32_t *n = s[cur ^ 1];
            if (t < kMtN - kMtM) n[t] = o[t + kMtM] ^ mt_twist(o[t], o[t + 1]);
            __syncthreads();
            if (t < kMtN - kMtM) {
                const int i = t + (kMtN - kMtM);
                n[i] = n[t] ^ mt_twist(o[i], o[i + 1]);
            }
            __syncthreads();
            if (t < kMtN - 2 * (kMtN - kMtM)) {
                const int i = t + 2 * (kMtN - kMtM);
                n[i] = n[i - (kMtN - kMtM)] ^ mt_twist(o[i], i == kMtN - 1 ? n[0] : o[i + 1]);
            }
            __syncthreads();
            cur ^= 1;
        }
        for (int i = t; i < kMtN; i += kNpThreads) {
            QR_DCHECK(b * kMtN + i < cap_words, kNpSiteWord, b * kMtN + i, cap_words);
            out[b * kMtN + i] = mt_temper(s[cur][i]);
        }
    }
    for (int i = t; i < kMtN; i += kNpThreads) key[i] = s[cur][i];
}

// out[j] = word w0 + j / double j of the range
__global__ void __launch_bounds__(kNpThreads) k_np_copy_words(NpRange r, int64_t n, uint32_t *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * kNpThreads + threadIdx.x;
    if (j >= n) return;
    QR_DCHECK(r.w0 + j < r.nwords, kNpSiteWord, r.w0 + j, r.nwords);
    out[j] = r.words[r.w0 + j];
}
__global__ void __launch_bounds__(kNpThreads) k_np_doubles(NpRange r, int64_t n, double *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * kNpThreads + threadIdx.x;
    if (j < n) out[j] = np_double(r, j);
}

// ------------------------------------------------------------------- np_scan
// exclusive scan of one value per thread over the workgroup; *total = the workgroup's sum
__device__ __forceinline__ uint32_t np_block_scan(uint32_t v, uint32_t *total) {
    __shared__ uint32_t wsum[kNpThreads / kWave];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t n = __shfl_up(inc, d, kWave);
        if (lane >= d) inc += n;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kNpThreads / kWave; ++i) {
        if (i < w) off += wsum[i];
        tot += wsum[i];
    }
    __syncthreads();
    *total = tot;
    return off + inc - v;
}

// the accept flags of this thread's kNpPer class entries, bit j = entry i0 + j
__device__ __forceinline__ uint32_t np_flags(const NpRange &r, int q, int64_t i0) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < kNpPer; ++j)
        if (i0 + j < r.nc && np_pair(r, 2 * (i0 + j) + q).accept()) m |= 1u << j;
    return m;
}

__global__ void __launch_bounds__(kNpThreads) k_np_scan_sums(NpRange r) {
    const int q = blockIdx.y;
    const int64_t i0 = ((int64_t)blockIdx.x * kNpThreads + threadIdx.x) * kNpPer;
    uint32_t tot;
    (void)np_block_scan(__builtin_popcount(np_flags(r, q, i0)), &tot);
    QR_DCHECK((int64_t)blockIdx.x < r.nb, kNpSitePrefix, blockIdx.x, r.nb);
    if (threadIdx.x == 0) r.bsum[q * r.nb + blockIdx.x] = tot;
}

// tile sums -> tile offsets, one workgroup per class walking its nb sums with a carry
__global__ void __launch_bounds__(kNpThreads) k_np_scan_mid(NpRange r) {
    const int q = blockIdx.x;
    uint32_t carry = 0;
    for (int64_t base = 0; base < r.nb; base += kNpThreads) {
        const int64_t i = base + threadIdx.x;
        uint32_t tot;
        const uint32_t ex = np_block_scan(i < r.nb ? r.bsum[q * r.nb + i] : 0u, &tot);
        if (i < r.nb) r.bsum[q * r.nb + i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) r.pref[q][r.nc] = carry;
}

__global__ void __launch_bounds__(kNpThreads) k_np_scan_add(NpRange r) {
    const int q = blockIdx.y;
    const int64_t i0 = ((int64_t)blockIdx.x * kNpThreads + threadIdx.x) * kNpPer;
    const uint32_t m = np_flags(r, q, i0);
    uint32_t tot;
    uint32_t c = r.bsum[q * r.nb + blockIdx.x] + np_block_scan(__builtin_popcount(m), &tot);
#pragma unroll
    for (int j = 0; j < kNpPer; ++j) {
        if (i0 + j < r.nc) {
            QR_DCHECK(c <= (uint32_t)(i0 + j), kNpSitePrefix, c, i0 + j);
            r.pref[q][i0 + j] = c;
        }
        c += (m >> j) & 1u;
    }
}

// ------------------------------------------------------------------ np_chain
// per frame f: dpos[f] its first double, hg[f] has_gauss on entry; dpos[B], hg[B] the state after
// the batch; frame_words[f] the words consumed through frame f.  flags[0] = 1 and flags[1] = f when
// the range ends inside frame f.
struct NpChainArgs {
    NpRange r;
    int32_t B;
    int64_t nsym, nnorm;
    int32_t hg0;
    int64_t *dpos;
    int32_t *hg;
    int64_t *frame_words;
    int32_t *flags;
};

// smallest i in (lo, hi] with A[i] >= T, given A[lo] < T <= A[hi]: the 64 lanes probe 64 evenly spaced
// entries of (lo, hi] and the ballot keeps one gap; six rounds shrink any range below 2^36 to one entry
__device__ __forceinline__ int64_t np_select(const uint32_t *__restrict__ A, int64_t lo, int64_t hi, uint32_t T,
                                             int64_t n) {
    const int lane = threadIdx.x;
#pragma unroll 1
    for (int round = 0; round < 6; ++round) {
        if (hi - lo <= 1) break;
        const int64_t step = (hi - lo + kWave - 1) / kWave;
        const int64_t p = np_min(lo + (lane + 1) * step, hi);
        QR_DCHECK(p >= 0 && p <= n, kNpSiteChain, p, n);
        const unsigned long long ge = __ballot(A[p] >= T);
        QR_DCHECK(ge != 0ull, kNpSiteChain, lo, hi);
        const int l = ge ? __builtin_ctzll(ge) : kWave - 1;
        const int64_t nlo = l == 0 ? lo : np_min(lo + l * step, hi);
        hi = np_min(lo + (l + 1) * step, hi);
        lo = nlo;
    }
    return hi;
}

__global__ void __launch_bounds__(kWave) k_np_chain(NpChainArgs a) {
    const NpRange &r = a.r;
    int64_t d = 0;
    int32_t hg = a.hg0;
    for (int32_t f = 0; f < a.B; ++f) {
        const int64_t left = a.nnorm - hg;                   // normals the candidates must give
        const int64_t need = left > 0 ? (left + 1) / 2 : 0;  // accepted pairs
        const int64_t c0 = d + a.nsym;                       // first candidate
        int64_t dn = c0;
        bool over = c0 > r.nd;
        if (!over && need > 0) {
            const int q = (int)(c0 & 1);
            const int64_t i0 = c0 >> 1;
            const uint32_t *A = r.pref[q];
            over = i0 >= r.nc;
            if (!over) {
                const uint32_t T = A[i0] + (uint32_t)need;
                over = A[r.nc] < T;
                if (!over) {
                    // the need-th accept at or after i0 is entry i - 1, i the first index with A[i] >= T
                    const int64_t guess = i0 + (int64_t)((double)need / 0.7853981633974483);
                    int64_t lo = np_max(i0, np_min(guess - kNpWindow, r.nc));
                    int64_t hi = np_min(r.nc, np_max(guess + kNpWindow, i0 + 1));
                    if (!(A[lo] < T && T <= A[hi])) {
                        lo = i0;
                        hi = r.nc;
                    }
                    const int64_t i = np_select(A, lo, hi, T, r.nc);
                    QR_DCHECK(i > i0 && i <= r.nc && A[i] == T && A[i - 1] == T - 1, kNpSiteChain, i, T);
                    dn = 2 * (i - 1) + q + 2;
                }
            }
        }
        if (over) {
            if (threadIdx.x == 0) {
                a.flags[0] = 1;
                a.flags[1] = f;
            }
            return;
        }
        if (threadIdx.x == 0) {
            a.dpos[f] = d;
            a.hg[f] = hg;
            a.frame_words[f] = 2 * dn;
        }
        // an odd count leaves the last pair's other value cached; a frame whose only normal was the
        // cached one leaves none; symbols alone (nnorm = 0) do not touch the cache
        if (a.nnorm > 0) hg = left > 0 ? (int32_t)(2 * need - left) : 0;
        d = dn;
    }
    if (threadIdx.x == 0) {
        a.dpos[a.B] = d;
        a.hg[a.B] = hg;
    }
}

// ------------------------------------------------------------------- np_fill
struct NpFillArgs {
    NpRange r;
    int32_t B, ld;
    int64_t nsym, nnorm;
    int32_t M;
    const double *cdf, *a;
    double sigma, gauss0;
    const int64_t *dpos;
    const int32_t *hg;
    int64_t *x;            // [nsym, ld] or null
    double *y;             // [nnorm, ld] or null: the normals, then a[x] + sigma * normal
    double *gauss_after;   // [B]: the normal a frame leaves cached (0.0 when none)
    int64_t cand_blocks;   // workgroups per frame of k_np_fill_normals
};

// one thread per (frame, candidate of the frame's class): an accepted one knows its rank among the
// frame's accepts from the prefix counts and writes f * x2 and f * x1 to its two slots; the last
// one's f * x1, when the frame needs an odd count, is the value cached for the next frame
__global__ void __launch_bounds__(kNpThreads) k_np_fill_normals(NpFillArgs a) {
#pragma clang fp contract(off)
    const NpRange &r = a.r;
    const int32_t f = (int32_t)(blockIdx.x / a.cand_blocks);
    const int64_t j = (int64_t)(blockIdx.x % a.cand_blocks) * kNpThreads + threadIdx.x;
    const int32_t hg = a.hg[f];
    if (j == 0 && f == 0 && hg) a.y[0] = a.gauss0;
    if (j == 0 && !a.hg[f + 1]) a.gauss_after[f] = 0.0;
    const int64_t c0 = a.dpos[f] + a.nsym, end = a.dpos[f + 1];
    const int q = (int)(c0 & 1);
    const int64_t i0 = c0 >> 1, i = i0 + j, k = 2 * i + q;
    if (k + 2 > end) return;  // past the frame's last accepted candidate
    QR_DCHECK(i + 1 <= r.nc, kNpSitePrefix, i, r.nc);
    const uint32_t *A = r.pref[q];
    if (A[i + 1] == A[i]) return;
    const int64_t rank = (int64_t)(A[i] - A[i0]);
    const int64_t slot = hg + 2 * rank;
    QR_DCHECK(slot >= 0 && slot < a.nnorm, kNpSiteRank, slot, a.nnorm);
    const NpPair p = np_pair(r, k);
    const double g = sqrt(-2.0 * g_log_full(p.r2, kGlibcConst) / p.r2);
    a.y[slot * a.ld + f] = g * p.x2;
    if (slot + 1 < a.nnorm) {
        a.y[(slot + 1) * a.ld + f] = g * p.x1;
    } else {
        QR_DCHECK(k + 2 == end && a.hg[f + 1] == 1, kNpSiteRank, k, end);
        a.gauss_after[f] = g * p.x1;
        if (f + 1 < a.B) a.y[f + 1] = g * p.x1;   // slot 0 of the next frame
    }
}

// one thread per (position, column): x = the count of cdf[k] <= u (searchsorted, side='right'),
// y = a[x] + sigma * normal; columns B..ld-1 are zeros
__global__ void __launch_bounds__(kNpThreads) k_np_fill_symbols(NpFillArgs a) {
#pragma clang fp contract(off)
    const int64_t item = (int64_t)blockIdx.x * kNpThreads + threadIdx.x;
    const int64_t s = item / a.ld;
    const int32_t f = (int32_t)(item - s * a.ld);
    if (s >= a.nsym) return;
    QR_DCHECK(item < a.nsym * a.ld, kNpSiteOut, item, a.nsym * a.ld);
    if (f >= a.B) {
        a.x[item] = 0;
        if (a.y) a.y[item] = 0.0;
        return;
    }
    const double u = np_double(a.r, a.dpos[f] + s);
    int32_t x = 0;
    for (int32_t k = 0; k < a.M; ++k) x += a.cdf[k] <= u ? 1 : 0;
    QR_DCHECK(x < a.M, kNpSiteOut, x, a.M);
    a.x[item] = x;
    if (a.y) {
        const double t = a.sigma * a.y[item];
        a.y[item] = a.a[x < a.M ? x : a.M - 1] + t;
    }
}

}  // namespace qr

// ===================================================================== handle
struct qr_npstream {
    int device = 0;
    uint32_t key[qr::kMtN];
    int32_t pos = qr::kMtN, has_gauss = 0;
    double gauss = 0.0;
    // the last frames call (qr_npstream_seek_frame): its words in the caller's workspace, the
    // stream's position in block 0 when it began, and the state after every frame
    const uint32_t *d_words = nullptr;
    int32_t w0 = 0;
    std::vector<int64_t> frame_words;
    std::vector<int32_t> hg;       // [B + 1]
    std::vector<double> gauss_after;
    std::mutex mu;
    qr::Scratch scratch;
};

namespace qr {
namespace {

// the device arrays of one run, carved from a workspace; with a null base only measured
struct NpWs {
    uint32_t *words, *pref[2], *bsum, *key;
    int64_t *dpos, *frame_words;
    int32_t *hg, *flags;
    double *gauss_after;
    int64_t cap_blocks, cap_nc, cap_nb;
};
bool np_carve(Cursor &c, int64_t B, int64_t nsym, int64_t nnorm, NpWs &w) {
    const NpSizing z = np_sizing(B, nsym, nnorm);
    w.cap_blocks = np_blocks(kMtN, z.cap());
    w.cap_nc = w.cap_blocks * kMtN / 4 + 1;
    w.cap_nb = (w.cap_nc + kNpTile - 1) / kNpTile;
    if (w.cap_nc >= (int64_t)1 << 31) return false;
    w.words = c.take<uint32_t>((size_t)w.cap_blocks * kMtN);
    w.pref[0] = c.take<uint32_t>((size_t)w.cap_nc + 1);
    w.pref[1] = c.take<uint32_t>((size_t)w.cap_nc + 1);
    w.bsum = c.take<uint32_t>((size_t)2 * w.cap_nb);
    w.key = c.take<uint32_t>(kMtN);
    w.dpos = c.take<int64_t>((size_t)B + 1);
    w.frame_words = c.take<int64_t>((size_t)B);
    w.hg = c.take<int32_t>((size_t)B + 1);
    w.flags = c.take<int32_t>(4);
    w.gauss_after = c.take<double>((size_t)B);
    return true;
}

unsigned np_grid(int64_t n) { return (unsigned)((n + kNpThreads - 1) / kNpThreads); }

// the handle's state := word offset `off` of the words at d_words (block 0 = the block the call began in)
int np_set_state(qr_npstream *st, const uint32_t *d_words, int64_t off, int32_t hg, double gauss) {
    const NpWhere at = np_locate(off);
    uint32_t blk[kMtN];
    QR_HIP(hipMemcpy(blk, d_words + at.block * kMtN, sizeof blk, hipMemcpyDeviceToHost));
    for (int i = 0; i < kMtN; ++i) st->key[i] = mt_untemper(blk[i]);
    st->pos = at.pos;
    st->has_gauss = hg;
    st->gauss = hg ? gauss : 0.0;
    return QR_OK;
}

// whole blocks [done, blocks) of the range into w.words; the key on the device carries the recurrence
int np_generate(const NpWs &w, int64_t done, int64_t blocks, hipStream_t s) {
    if (blocks <= done) return QR_OK;
    ProfScope ps("np_words", s);
    k_np_words<<<1, kNpThreads, 0, s>>>(w.key, w.words + done * kMtN, blocks - done, done == 0 ? 1 : 0,
                                        (w.cap_blocks - done) * kMtN);
    QR_LAUNCH_CHECK();
    return QR_OK;
}

NpRange np_range(const NpWs &w, int32_t w0, int64_t blocks, int64_t doubles) {
    NpRange r;
    r.words = w.words;
    r.nwords = blocks * kMtN;
    r.w0 = w0;
    r.nd = std::min<int64_t>(doubles, (r.nwords - w0) / 2);
    r.nc = r.nd > 1 ? (r.nd - 1) / 2 : 0;
    r.pref[0] = w.pref[0];
    r.pref[1] = w.pref[1];
    r.bsum = w.bsum;
    r.nb = std::max<int64_t>(1, (r.nc + kNpTile - 1) / kNpTile);
    return r;
}

// B frames of nsym symbol draws (x, with cdf) and nnorm normals (y) from the handle's state; the
// state moves past them.  x / y may be null when nsym / nnorm is 0.  Caller holds st->mu.
int np_run(qr_npstream *st, int32_t B, int32_t ld, int64_t nsym, int64_t nnorm, int32_t M, const double *d_cdf,
           const double *d_a, double sigma, int64_t *d_x, double *d_y, int64_t *d_frame_words, const NpWs &w,
           hipStream_t s) {
    const NpSizing z = np_sizing(B, nsym, nnorm);
    const int32_t w0 = st->pos;
    QR_HIP(hipMemcpyAsync(w.key, st->key, sizeof st->key, hipMemcpyHostToDevice, s));
    int64_t doubles = z.first(g_np_slack_pct.load()), blocks = 0;
    NpChainArgs ca;
    int32_t flags[4] = {0, 0, 0, 0};
    for (int round = 0;; ++round) {
        const int64_t want = std::min(np_blocks(w0, doubles), w.cap_blocks);
        if (int rc = np_generate(w, blocks, want, s)) return rc;
        blocks = want;
        const NpRange r = np_range(w, w0, blocks, doubles);
        {
            ProfScope ps("np_scan", s);
            k_np_scan_sums<<<dim3((unsigned)r.nb, 2), kNpThreads, 0, s>>>(r);
            k_np_scan_mid<<<2, kNpThreads, 0, s>>>(r);
            k_np_scan_add<<<dim3((unsigned)r.nb, 2), kNpThreads, 0, s>>>(r);
            QR_LAUNCH_CHECK();
        }
        QR_HIP(hipMemsetAsync(w.flags, 0, 4 * sizeof(int32_t), s));
        ca = NpChainArgs{r, B, nsym, nnorm, st->has_gauss, w.dpos, w.hg, w.frame_words, w.flags};
        {
            ProfScope ps("np_chain", s);
            k_np_chain<<<1, kWave, 0, s>>>(ca);
            QR_LAUNCH_CHECK();
        }
        QR_HIP(hipMemcpyAsync(flags, w.flags, sizeof flags, hipMemcpyDeviceToHost, s));
        QR_HIP(hipStreamSynchronize(s));
        if (!flags[0]) break;
        if (round == kNpRounds || doubles >= z.cap())
            return set_error(QR_EINTERNAL, "npstream: the generated range ended inside frame %d after %d top-up rounds",
                             flags[1], round);
        doubles = std::min(doubles + z.slack, z.cap());
    }
    std::vector<int64_t> dpos((size_t)B + 1);
    st->hg.resize((size_t)B + 1);
    st->frame_words.resize((size_t)B);
    st->gauss_after.assign((size_t)B, 0.0);
    QR_HIP(hipMemcpyAsync(dpos.data(), w.dpos, dpos.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    QR_HIP(hipMemcpyAsync(st->hg.data(), w.hg, st->hg.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    QR_HIP(hipStreamSynchronize(s));
    int64_t maxcand = 0;
    for (int32_t f = 0; f < B; ++f) {
        st->frame_words[(size_t)f] = 2 * dpos[(size_t)f + 1];
        maxcand = std::max(maxcand, (dpos[(size_t)f + 1] - dpos[(size_t)f] - nsym + 1) / 2);
    }
    NpFillArgs fa{ca.r, B, ld, nsym, nnorm, M, d_cdf, d_a, sigma, st->gauss, w.dpos, w.hg, d_x, d_y, w.gauss_after,
                  std::max<int64_t>(1, (maxcand + kNpThreads - 1) / kNpThreads)};
    if (fa.cand_blocks * B >= (int64_t)1 << 31 || (nsym * ld + kNpThreads - 1) / kNpThreads >= (int64_t)1 << 31)
        return set_error(QR_EVALUE, "npstream: batch too large for one launch");
    {
        ProfScope ps("np_fill", s);
        if (nnorm > 0) k_np_fill_normals<<<(unsigned)(fa.cand_blocks * B), kNpThreads, 0, s>>>(fa);
        if (nsym > 0) k_np_fill_symbols<<<np_grid(nsym * ld), kNpThreads, 0, s>>>(fa);
        QR_LAUNCH_CHECK();
    }
    if (d_frame_words)
        QR_HIP(hipMemcpyAsync(d_frame_words, w.frame_words, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (nnorm > 0)
        QR_HIP(hipMemcpyAsync(st->gauss_after.data(), w.gauss_after, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
    QR_HIP(hipStreamSynchronize(s));
    st->d_words = w.words;
    st->w0 = w0;
    return np_set_state(st, w.words, w0 + st->frame_words[(size_t)B - 1], st->hg[(size_t)B],
                        nnorm > 0 ? st->gauss_after[(size_t)B - 1] : st->gauss);
}

// one "frame" of the handle's own scratch: n words, doubles, symbols or normals to d_out
enum NpKind { kNpWords, kNpDoubles, kNpNormals, kNpChoice };
int np_simple(qr_npstream *st, NpKind kind, int64_t n, int32_t M, const double *d_cdf, void *d_out, hipStream_t s) {
    if (!st || n < 0 || (n > 0 && !d_out)) return set_error(QR_EVALUE, "npstream: null argument or negative count");
    if (n == 0) return QR_OK;
    DeviceGuard g(st->device);
    std::lock_guard<std::mutex> lk(st->mu);
    std::lock_guard<std::mutex> lk2(st->scratch.mu);
    st->d_words = nullptr;  // the scratch may move: no seek into an earlier frames call
    if (kind == kNpNormals || kind == kNpChoice) {
        const int64_t nsym = kind == kNpChoice ? n : 0, nnorm = kind == kNpNormals ? n : 0;
        NpWs w;
        Cursor m{0};
        if (!np_carve(m, 1, nsym, nnorm, w)) return set_error(QR_EVALUE, "npstream: count too large for one call");
        if (int rc = st->scratch.reserve(m.off)) return rc;
        Cursor c{(uintptr_t)st->scratch.ptr};
        np_carve(c, 1, nsym, nnorm, w);
        const int rc = np_run(st, 1, 1, nsym, nnorm, M, d_cdf, nullptr, 0.0, (int64_t *)(nsym ? d_out : nullptr),
                              (double *)(nnorm ? d_out : nullptr), nullptr, w, s);
        st->d_words = nullptr;
        return rc;
    }
    const int64_t words = kind == kNpWords ? n : 2 * n;
    NpWs w{};
    w.cap_blocks = np_blocks(st->pos, (words + 1) / 2);
    Cursor m{0};
    m.take<uint32_t>((size_t)w.cap_blocks * kMtN);
    m.take<uint32_t>(kMtN);
    if (int rc = st->scratch.reserve(m.off)) return rc;
    Cursor c{(uintptr_t)st->scratch.ptr};
    w.words = c.take<uint32_t>((size_t)w.cap_blocks * kMtN);
    w.key = c.take<uint32_t>(kMtN);
    QR_HIP(hipMemcpyAsync(w.key, st->key, sizeof st->key, hipMemcpyHostToDevice, s));
    if (int rc = np_generate(w, 0, w.cap_blocks, s)) return rc;
    NpRange r{};
    r.words = w.words;
    r.nwords = w.cap_blocks * kMtN;
    r.w0 = st->pos;
    r.nd = (r.nwords - r.w0) / 2;
    if (kind == kNpWords) k_np_copy_words<<<np_grid(n), kNpThreads, 0, s>>>(r, n, (uint32_t *)d_out);
    else k_np_doubles<<<np_grid(n), kNpThreads, 0, s>>>(r, n, (double *)d_out);
    QR_LAUNCH_CHECK();
    QR_HIP(hipStreamSynchronize(s));
    return np_set_state(st, w.words, st->pos + words, st->has_gauss, st->gauss);
}

}  // namespace
}  // namespace qr

// ===================================================================== C-ABI
extern "C" {
using namespace qr;

int qr_npstream_create(const uint32_t *key, int32_t pos, int32_t has_gauss, double gauss, int32_t device,
                       qr_npstream **out) {
    if (!key || !out) return set_error(QR_EVALUE, "qr_npstream_create: null argument");
    if (pos < 0 || pos > kMtN || (has_gauss != 0 && has_gauss != 1))
        return set_error(QR_EVALUE, "qr_npstream_create: need 0 <= pos <= 624 and has_gauss 0 or 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(QR_EDEVICE, "no HIP device available (libqamr has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_error(QR_EVALUE, "device %d out of range (%d devices)", device, ndev);
    qr_npstream *st = new qr_npstream();
    st->device = device;
    st->scratch.device = device;
    std::memcpy(st->key, key, sizeof st->key);
    st->pos = pos;
    st->has_gauss = has_gauss;
    st->gauss = has_gauss ? gauss : 0.0;
    *out = st;
    return QR_OK;
}

int qr_npstream_destroy(qr_npstream *st) {
    delete st;
    return QR_OK;
}

int qr_npstream_state(const qr_npstream *st, uint32_t *key, int32_t *pos, int32_t *has_gauss, double *gauss) {
    if (!st) return set_error(QR_EVALUE, "qr_npstream_state: null stream");
    if (key) std::memcpy(key, st->key, sizeof st->key);
    if (pos) *pos = st->pos;
    if (has_gauss) *has_gauss = st->has_gauss;
    if (gauss) *gauss = st->gauss;
    return QR_OK;
}

int qr_npstream_words_device(qr_npstream *st, int64_t n, uint32_t *d_out, void *stream) {
    return np_simple(st, kNpWords, n, 0, nullptr, d_out, (hipStream_t)stream);
}

int qr_npstream_random_sample_device(qr_npstream *st, int64_t n, double *d_out, void *stream) {
    return np_simple(st, kNpDoubles, n, 0, nullptr, d_out, (hipStream_t)stream);
}

int qr_npstream_standard_normal_device(qr_npstream *st, int64_t n, double *d_out, void *stream) {
    return np_simple(st, kNpNormals, n, 0, nullptr, d_out, (hipStream_t)stream);
}

int qr_npstream_choice_device(qr_npstream *st, int64_t n, int32_t M, const double *d_cdf, int64_t *d_out,
                              void *stream) {
    if (M < 2 || M > 256 || !d_cdf) return set_error(QR_EVALUE, "qr_npstream_choice_device: need d_cdf and 2 <= M <= 256");
    return np_simple(st, kNpChoice, n, M, d_cdf, d_out, (hipStream_t)stream);
}

int qr_npstream_frames_workspace_size(int64_t S, int32_t B, size_t *bytes) {
    if (!bytes || S <= 0 || B <= 0) return set_error(QR_EVALUE, "qr_npstream_frames_workspace_size: need S > 0, B > 0");
    NpWs w;
    Cursor m{0};
    if (!np_carve(m, B, S, S, w))
        return set_error(QR_EVALUE, "npstream: B * S too large for one call (2^31 candidates per class)");
    *bytes = m.off;
    return QR_OK;
}

int qr_npstream_frames_device(qr_npstream *st, int32_t B, int32_t ld, int64_t S, int32_t M, const double *d_cdf,
                              const double *d_constellation, double sigma, int64_t *d_x, double *d_y,
                              int64_t *d_frame_words, void *ws, size_t ws_bytes, void *stream) {
    if (!st || !d_cdf || !d_constellation || !d_x || !d_y || !d_frame_words || !ws)
        return set_error(QR_EVALUE, "qr_npstream_frames_device: null argument");
    if (B <= 0 || ld < B || ld % kWave || S <= 0)
        return set_error(QR_EVALUE, "qr_npstream_frames_device: need 0 < B <= ld, ld %% 64 == 0, S > 0 (B=%d ld=%d S=%lld)",
                         B, ld, (long long)S);
    if (M < 2 || M > 256) return set_error(QR_EVALUE, "qr_npstream_frames_device: M = %d outside 2..256", M);
    NpWs w;
    Cursor m{0};
    if (!np_carve(m, B, S, S, w))
        return set_error(QR_EVALUE, "npstream: B * S too large for one call (2^31 candidates per class)");
    if (ws_bytes < m.off || ((uintptr_t)ws & 255))
        return set_error(QR_EVALUE, "qr_npstream_frames_device: workspace of %zu bytes, 256-byte aligned, required (%zu given)",
                         m.off, ws_bytes);
    DeviceGuard g(st->device);
    std::lock_guard<std::mutex> lk(st->mu);
    Cursor c{(uintptr_t)ws};
    np_carve(c, B, S, S, w);
    st->d_words = nullptr;
    return np_run(st, B, ld, S, S, M, d_cdf, d_constellation, sigma, d_x, d_y, d_frame_words, w, (hipStream_t)stream);
}

int qr_npstream_seek_frame(qr_npstream *st, int32_t frame) {
    if (!st) return set_error(QR_EVALUE, "qr_npstream_seek_frame: null stream");
    std::lock_guard<std::mutex> lk(st->mu);
    if (!st->d_words || frame < 0 || (size_t)frame >= st->frame_words.size())
        return set_error(QR_EVALUE, "qr_npstream_seek_frame: frame %d is not a frame of the last frames call", frame);
    DeviceGuard g(st->device);
    return np_set_state(st, st->d_words, st->w0 + st->frame_words[(size_t)frame], st->hg[(size_t)frame + 1],
                        st->gauss_after[(size_t)frame]);
}

}  // extern "C"
