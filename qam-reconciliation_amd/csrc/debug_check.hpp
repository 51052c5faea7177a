// debug_check.hpp -- device-side index checks of the debug build (make -C csrc DEBUG=1 ->
// qamr/libqamr_debug.so, QR_DEBUG_ASSERT=1; SURVEY.md 5 -- the reference turns bounds checks off,
// decoder.pyx:181,240,289,332,399,411): QR_DCHECK(ok, site, a, b) counts every failed check in
// g_dbg and keeps the first failure's site and two values; the first failing lane also prints
// them.  Non-fatal (no trap): the test reads the counts through qr_debug_asserts
// (tests/test_gpu_debug_build.py).  The product library compiles every check away.
//
// No relocatable device code, so every translation unit that includes this header carries its own
// counter; a static object of the unit registers its reader (debug_read_clear) in one list
// (debug_readers, owned by decoder.hip), and qr_debug_asserts (decoder.hip) adds the list up: a
// unit with checks only has to be compiled with QR_DEBUG_ASSERT (the Makefile's DEBUG_SRCS,
// tests/test_host_logic.py).  The site numbers are one list across the units: 1..9 and 17..19 the
// decoder's units (decode_dev.hpp DebugSite), 10..11 grid_interp.hpp (GridDebugSite), 12..16 mi.hip
// (MiDebugSite), 20..24 npstream.hip (NpDebugSite), 25..26 lappr_info.hip (InfoDebugSite), 27..30 decode_layered.hip
// (decode_dev.hpp DebugSite), 31..34 density_evolution.hip (DeDebugSite),
// 35..38 rate_adapt.hip (RaDebugSite).
#pragma once
#include <hip/hip_runtime.h>

#ifndef QR_DEBUG_ASSERT
#define QR_DEBUG_ASSERT 0
#endif

#if QR_DEBUG_ASSERT
namespace qr {
static __device__ unsigned long long g_dbg[4];  // {failed checks, first site, first a, first b}
__device__ __noinline__ void dcheck_fail(int site, long long a, long long b) {
    if (atomicAdd(&g_dbg[0], 1ull) == 0ull) {
        g_dbg[1] = (unsigned long long)site;
        g_dbg[2] = (unsigned long long)a;
        g_dbg[3] = (unsigned long long)b;
        printf("qamr debug check %d failed: a=%lld b=%lld (block %u thread %u)\n", site, a, b, blockIdx.x, threadIdx.x);
    }
}
// h = this unit's {failed checks, first site, first a, first b}; reads and clears them
static bool debug_read_clear(unsigned long long h[4]) {
    const unsigned long long z[4] = {0, 0, 0, 0};
    return hipMemcpyFromSymbol(h, HIP_SYMBOL(g_dbg), sizeof(z)) == hipSuccess &&
           hipMemcpyToSymbol(HIP_SYMBOL(g_dbg), z, sizeof(z)) == hipSuccess;
}
// the readers of every unit of the library that carries checks, in the order the units were linked
using DebugReader = bool (*)(unsigned long long[4]);
struct DebugReaders {
    static constexpr int kMax = 32;  // units; a reader past it is dropped and n still counts it
    DebugReader fn[kMax];
    int n = 0;
    bool add(DebugReader f) {
        if (n < kMax) fn[n] = f;
        return ++n <= kMax;
    }
};
DebugReaders &debug_readers();  // decoder.hip (a function-local static: safe at any initialisation order)
static const bool g_dbg_registered = debug_readers().add(&debug_read_clear);
}  // namespace qr
#endif

// the fail function is device code: a host+device body's checks exist on the device pass only
#if QR_DEBUG_ASSERT && defined(__HIP_DEVICE_COMPILE__)
#define QR_DCHECK(ok, site, a, b)                                             \
    do {                                                                      \
        if (!(ok)) ::qr::dcheck_fail((site), (long long)(a), (long long)(b)); \
    } while (0)
#else
#define QR_DCHECK(ok, site, a, b) ((void)0)
#endif
