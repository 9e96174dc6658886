// ajx_kcommon.h — device helpers shared by the kernel translation units (ajx_kernels.hip,
// ajx_lean.hip): per-device attribute guards, the LDS staging of a ruleset blob, the window
// rings' geometry. (The per-request bodies: ajx_request.h; stage B: ajx_stageb.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "ajx_request.h"

#ifndef AJX_FAST_WAVES
#define AJX_FAST_WAVES 4  // waves per SIMD the single-pass kernels' register budget is set for
#endif

namespace ajx {

// The dynamic-LDS ceiling of a group of kernels is set once per device (the attribute
// belongs to that device's code object); any thread may launch first, so the per-device
// bits are atomic (setting an attribute twice is harmless).
template <class F>
static hipError_t attr_once(std::atomic<uint64_t>& done, F set) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
    if ((e = set()) != hipSuccess) return e;
    done.fetch_or(bit, std::memory_order_acq_rel);
    return hipSuccess;
}

// SHARED kernels: the whole batch uses sets[0], and the ruleset blob (trie, key table,
// patterns, literals, DFA tables, fold code — h->total_bytes, a multiple of 16) is
// copied into dynamic LDS once per workgroup; every thread reaches the barrier. All
// table reads of the scan and the patterns are then ds_reads.
// copies nq 16-byte words, four loads in flight per thread before their stores. The source
// is read as global memory (a blob pointer loaded from the set table is generic: flat
// loads otherwise), every load unconditional (a clamped index past the end), so that
// nothing goes to scratch.
__device__ __forceinline__ void copy_words(uint4* __restrict__ dst, const uint4* __restrict__ src, uint32_t nq,
                                           uint32_t t, uint32_t nt) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(1))) uint4* g = (const __attribute__((address_space(1))) uint4*)src;
#else
    const uint4* g = src;  // (host pass of the kernel source: never run)
#endif
    const uint32_t last = nq - 1u;
    for (uint32_t b = t; b < nq; b += 4u * nt) {
        const uint32_t k1 = b + nt, k2 = b + 2u * nt, k3 = b + 3u * nt;
        const uint4 v0 = g[b];
        const uint4 v1 = g[k1 < nq ? k1 : last];
        const uint4 v2 = g[k2 < nq ? k2 : last];
        const uint4 v3 = g[k3 < nq ? k3 : last];
        dst[b] = v0;
        if (k1 < nq) dst[k1] = v1;
        if (k2 < nq) dst[k2] = v2;
        if (k3 < nq) dst[k3] = v3;
    }
}

template <bool SHARED>
__device__ __forceinline__ const uint8_t* stage_blob(const uint8_t* gblob) {
    if constexpr (SHARED) {
        extern __shared__ uint4 s_blob[];
        const uint32_t nq = reinterpret_cast<const RulesetHdr*>(gblob)->total_bytes / 16;
        copy_words(s_blob, reinterpret_cast<const uint4*>(gblob), nq, threadIdx.x, blockDim.x);
        __syncthreads();
        return reinterpret_cast<const uint8_t*>(s_blob);
    } else {
        return gblob;
    }
}

// the work-item's 128-B window ring in dynamic LDS: [blob copy (SHARED)] [ring: per wave
// 8 chunks x 64 lanes x 16 B]
constexpr uint32_t kWinRingBytesPerWave = 8 * 64 * 16;
// single-pass workgroups of 4, 8 or 16 waves (fast_block): one LDS copy of the ruleset
// blob per workgroup next to its waves' rings, so 16 waves per CU fit the 160 KiB for
// blobs up to ~8 KiB in 4-wave groups, ~16 KiB in 8-wave groups, ~32 KiB in one 16-wave
// group (4 waves/SIMD by registers either way)
constexpr uint32_t kFastBlock = 512;
constexpr uint32_t kFastMaxBlock = 1024;
// dynamic LDS of the single-pass kernels: [blob copy (staged_bytes, 0: none)] [one window
// ring per wave of the workgroup]
struct RingGeom {
    uint32_t ring_off;  // the rings' offset: the blob copy's size, 16-byte aligned
    uint32_t lds;       // dynamic LDS bytes of the workgroup
};
static inline RingGeom ring_geom(uint32_t staged_bytes, uint32_t block, uint32_t ring_bytes = kWinRingBytesPerWave) {
    const uint32_t ring_off = (staged_bytes + 15u) & ~15u;
    return RingGeom{ring_off, ring_off + (block / 64) * ring_bytes};
}
// the workgroup size, 256 .. max_block, that fits the most waves per CU (at most `waves`
// per SIMD, the kernel's register budget) for a staged blob of `blob_bytes` (0: nothing
// staged) next to rings of `ring_bytes` per wave; the smallest such size on a tie: a
// workgroup retires as a unit, so smaller ones leave fewer idle waves behind the longest
// document (measured: c2 4-wave 2.03 ms vs 8-wave 2.11; c3 at 16 waves/CU 2 x 8-wave 3.78
// vs 1 x 16-wave 4.03)
static inline uint32_t staged_block(uint32_t blob_bytes, uint32_t max_block, uint32_t waves, uint32_t ring_bytes) {
    uint32_t best = 0, best_w = 0;
    for (uint32_t b = 256; b <= max_block; b *= 2) {
        const uint32_t lds = ring_geom(blob_bytes, b, ring_bytes).lds;
        uint32_t w = lds <= 160u * 1024u ? (160u * 1024u / lds) * (b / 64) : 0u;
        if (w > 4u * waves) w = 4u * waves;
        if (w > best_w) best = b, best_w = w;
    }
    return best ? best : 256u;
}
// (the token scanner's kernels)
static inline uint32_t fast_block(uint32_t blob_bytes) {
    return staged_block(blob_bytes, kFastMaxBlock, AJX_FAST_WAVES, kWinRingBytesPerWave);
}
__device__ __forceinline__ WinRing lane_ring(uint32_t ring_off) {
    extern __shared__ uint4 s_dyn_ring[];
    WinRing r;
    r.base = reinterpret_cast<uint8_t*>(s_dyn_ring) + ring_off + (threadIdx.x >> 6) * kWinRingBytesPerWave;
    r.lane16 = (threadIdx.x & 63u) * 16u;
    r.cstride = 64u * 16u;
    return r;
}

}  // namespace ajx
