// npstream_check.cpp -- the host pieces of numpy's stream (csrc/npstream_host.hpp) in a stand-alone
// program, built and run under ASan + UBSan by tests/test_npstream_cpu.py.
//
//   npstream_check CASEFILE
//
// CASEFILE (little-endian, written by the test from numpy itself):
//   uint32 key[624], int32 pos            np.random.get_state() at the start
//   int32 n, uint32 words[n]              the next n words (np.random.bytes)
//   int32 m, then m times: int32 consumed, int32 pos, uint32 key[624]
//                                         the state after `consumed` words
// Checks: mt_untemper inverts mt_temper; whole blocks generated with mt_next_block from the key
// and tempered are numpy's words from offset pos on; the state rebuilt from those tempered blocks
// at every recorded offset (np_locate + mt_untemper) is numpy's key and pos; the sizing rule.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "npstream_host.hpp"

using namespace qr;

static int fail(const char *what, long long a, long long b) {
    std::fprintf(stderr, "npstream_check FAILED: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

template <typename T>
static bool rd(std::FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

static int check_sizing() {
    const long long shapes[][3] = {{1, 1, 1}, {5, 1, 1}, {64, 2, 2}, {200, 7, 7}, {130, 504, 504}, {4096, 32400, 32400},
                                   {1, 0, 100003}, {1, 1001, 0}};
    for (const auto &s : shapes) {
        const NpSizing z = np_sizing(s[0], s[1], s[2]);
        const double p = 0.7853981633974483, pairs = (double)s[0] * (double)((s[2] + 1) / 2);
        if (z.mean < s[0] * s[1] + (long long)(2.0 * pairs / p)) return fail("mean below the expectation", z.mean, s[0]);
        if (z.slack < (long long)(2.0 * 6.0 * std::sqrt(pairs * (1 - p)) / p) + kMtN / 2)
            return fail("slack below six standard deviations and a block", z.slack, s[0]);
        if (z.first(0) != z.mean || z.first(100) != z.mean + z.slack) return fail("first range", z.first(0), z.first(100));
        if (z.cap() != z.mean + (kNpRounds + 1) * z.slack || z.first(4096) != z.cap()) return fail("cap", z.cap(), z.first(4096));
        for (int pos : {0, 1, 623, 624}) {
            const long long b = np_blocks(pos, z.mean);
            if (b < 1 || b * kMtN < pos + 2 * z.mean || (b > 1 && (b - 1) * kMtN >= pos + 2 * z.mean))
                return fail("blocks of a range", b, pos);
        }
    }
    if (np_blocks(624, 0) != 1 || np_blocks(0, 312) != 1 || np_blocks(1, 312) != 2) return fail("np_blocks edge", 0, 0);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: npstream_check CASEFILE", argc, 0);
    for (uint32_t x = 0; x < 2000003u; ++x) {
        const uint32_t v = x * 2654435761u + (x >> 3);
        if (mt_untemper(mt_temper(v)) != v) return fail("untemper(temper(v)) != v", v, mt_untemper(mt_temper(v)));
    }
    for (uint32_t v : {0u, 1u, 0x80000000u, 0xffffffffu, 0x9d2c5680u, 0xefc60000u})
        if (mt_untemper(mt_temper(v)) != v) return fail("untemper(temper(v)) != v", v, 0);

    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case file", 0, 0);
    std::vector<uint32_t> key(kMtN);
    int32_t pos = 0, n = 0, m = 0;
    if (!rd(f, key.data(), kMtN) || !rd(f, &pos, 1) || !rd(f, &n, 1) || n < 0) return fail("short case file", 0, 0);
    std::vector<uint32_t> words((size_t)n);
    if (!rd(f, words.data(), (size_t)n) || !rd(f, &m, 1) || m < 0) return fail("short case file", 1, 0);

    // whole blocks from the key, tempered: block 0 is the key itself
    const int64_t blocks = np_blocks(pos, (n + 1) / 2);
    std::vector<uint32_t> w((size_t)blocks * kMtN), k = key;
    for (int64_t b = 0; b < blocks; ++b) {
        if (b) mt_next_block(k.data());
        for (int i = 0; i < kMtN; ++i) w[(size_t)b * kMtN + i] = mt_temper(k[i]);
    }
    for (int32_t j = 0; j < n; ++j)
        if (w[(size_t)pos + j] != words[(size_t)j]) return fail("generated word differs from numpy's", j, w[(size_t)pos + j]);

    for (int32_t c = 0; c < m; ++c) {
        int32_t consumed = 0, pos_ref = 0;
        std::vector<uint32_t> key_ref(kMtN);
        if (!rd(f, &consumed, 1) || !rd(f, &pos_ref, 1) || !rd(f, key_ref.data(), kMtN)) return fail("short case file", 2, c);
        if (consumed < 0 || consumed > n) return fail("recorded offset outside the words", consumed, n);
        const NpWhere at = np_locate((int64_t)pos + consumed);
        if (at.block < 0 || at.block >= blocks) return fail("block outside the generated range", at.block, blocks);
        if (at.pos != pos_ref) return fail("pos", at.pos, pos_ref);
        for (int i = 0; i < kMtN; ++i)
            if (mt_untemper(w[(size_t)at.block * kMtN + i]) != key_ref[i]) return fail("key word", c, i);
    }
    std::fclose(f);
    if (int rc = check_sizing()) return rc;
    std::printf("npstream_check ok: %d words, %d states\n", n, m);
    return 0;
}
