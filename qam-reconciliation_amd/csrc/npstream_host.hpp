// npstream_host.hpp -- the host pieces of numpy's legacy stream (npstream.hip), free of HIP calls:
// MT19937's word functions, the (block, pos) a word offset stands for, and the sizing of the
// generated range.  tests/native/npstream_check.cpp runs them under ASan + UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define QR_NP_HD __host__ __device__ inline
#else
#define QR_NP_HD inline
#endif

namespace qr {

constexpr int kMtN = 624, kMtM = 397;
constexpr uint32_t kMtMatrix = 0x9908b0dfu, kMtUpper = 0x80000000u, kMtLower = 0x7fffffffu;

// new[i] = old-or-new[i + m] ^ mt_twist(old[i], old-or-new[i + 1])
QR_NP_HD uint32_t mt_twist(uint32_t u, uint32_t v) {
    const uint32_t y = (u & kMtUpper) | (v & kMtLower);
    return (y >> 1) ^ ((y & 1u) ? kMtMatrix : 0u);
}

QR_NP_HD uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// the inverse of mt_temper, step by step from the last
inline uint32_t mt_untemper(uint32_t y) {
    y ^= y >> 18;                                   // the high 18 bits were kept: one application undoes it
    uint32_t x = y;                                 // y = x ^ ((x << 15) & mask): 15 bits settle per round
    for (int r = 0; r < 2; ++r) x = y ^ ((x << 15) & 0xefc60000u);
    y = x;                                          // y = x ^ ((x << 7) & mask): 7 bits per round
    for (int r = 0; r < 4; ++r) x = y ^ ((x << 7) & 0x9d2c5680u);
    y = x;                                          // y = x ^ (x >> 11): 11 bits per round
    for (int r = 0; r < 2; ++r) x = y ^ (x >> 11);
    return x;
}

// the block after `key`, in place, in genrand's order (the kernel's three parallel phases compute the same)
inline void mt_next_block(uint32_t key[kMtN]) {
    for (int i = 0; i < kMtN; ++i)
        key[i] = key[(i + kMtM) % kMtN] ^ mt_twist(key[i], key[(i + 1) % kMtN]);
}

// Words are counted from the start of the block the stream stood in when a call began (that block
// is block 0 and is generated whole).  The state at word offset `off` (the next word to hand out):
// the block that holds it and the position inside it; an offset on a block boundary belongs to the
// block before it with pos = 624 (numpy regenerates lazily), offset 0 to block 0 with pos = 0.
struct NpWhere {
    int64_t block;
    int32_t pos;
};
inline NpWhere np_locate(int64_t off) {
    if (off <= 0) return {0, 0};
    const int64_t b = (off - 1) / kMtN;
    return {b, (int32_t)(off - b * kMtN)};
}

// The generated range of a batch, in doubles (two words each), per B frames of nsym symbol draws
// and nnorm normals: the symbols, two doubles per candidate pair at the mean of the negative
// binomial (ceil(nnorm / 2) accepts per frame at p = pi / 4), and a slack of six standard
// deviations of it plus one block and the look-ahead double.  The first range is mean + slack *
// pct / 100; every top-up round adds `slack`; the workspace holds kNpRounds of them past pct = 100.
constexpr int kNpRounds = 8;
struct NpSizing {
    int64_t mean, slack;
    int64_t first(int64_t pct) const {
        const int64_t want = mean + slack * pct / 100, cap_ = cap();
        return want < cap_ ? want : cap_;
    }
    int64_t cap() const { return mean + slack * (kNpRounds + 1); }
};
inline NpSizing np_sizing(int64_t B, int64_t nsym, int64_t nnorm) {
    const double p = 0.7853981633974483;  // pi / 4
    const double pairs = (double)B * (double)((nnorm + 1) / 2);
    const double sd = std::sqrt(pairs * (1.0 - p)) / p;
    NpSizing s;
    s.mean = B * nsym + 2 * (int64_t)std::ceil(pairs / p) + 1;
    s.slack = 2 * (int64_t)std::ceil(6.0 * sd) + kMtN / 2;
    return s;
}
// whole blocks that hold `doubles` doubles from position pos of block 0
inline int64_t np_blocks(int32_t pos, int64_t doubles) {
    const int64_t words = pos + 2 * doubles;
    return words <= kMtN ? 1 : (words + kMtN - 1) / kMtN;
}

}  // namespace qr
