// ajx_lean.hip — the lean single-pass kernel (ajx_lean.h) in its own translation unit, so
// that the walker's code is compiled (and tuned) without the rest of the kernels.
#include <hip/hip_runtime.h>

#include "ajx_kcommon.h"
#include "ajx_kernels.h"
#include "ajx_lean.h"


namespace ajx {

static_assert(64 * kSpanStride <= lean::kRingBytesPerWave, "stage B's span buffers lie in the wave's ring");
constexpr uint32_t kLeanMaxBlock = 1024;
#ifndef AJX_LEAN_MAXBLOCK
#define AJX_LEAN_MAXBLOCK kLeanMaxBlock
#endif

// The lean single-pass kernel (ajx_lean.h): stage A with the lean scan, then stage B in the
// same work-item. Dynamic LDS: [blob copy (SHARED)] [per wave: 64 lanes x 128-B rings,
// chunk-major (lean::kRingStride, kChunkStride)].
#ifndef AJX_LEAN_WAVES
#define AJX_LEAN_WAVES AJX_FAST_WAVES  // waves per SIMD the lean kernel's registers are set for
#endif
// keep_rows bit 1 (bit 0: kKeepRows): the outputs in work-item order (gathered back by
// ajx_unpermute)
constexpr uint32_t kLeanOutByItem = 2u;
// ABL: profiling ablations (kernel modes 15..18, lean::scan_doc): stage A cut short, no stage B.
// ARR: the instance walks arrays on selector paths (lean::Walk). launch_lean picks by the
// ruleset's kLeanArr (RulesetHdr::lean_feat)
template <bool SHARED, int ABL = 0, bool ARR = true>
__global__ __launch_bounds__(AJX_LEAN_MAXBLOCK, AJX_LEAN_WAVES) void ajx_scan_lean(
    const uint8_t* const* __restrict__ sets, const uint32_t* __restrict__ set_of_req,
    const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs, const uint32_t* __restrict__ lens, uint32_t n,
    uint64_t* __restrict__ rows, uint32_t row_stride, uint32_t* __restrict__ slow_count,
    uint32_t* __restrict__ slow_ids, uint8_t* __restrict__ out_tri, int32_t* __restrict__ out_err,
    uint64_t* __restrict__ out_bm, uint32_t stride, uint32_t ring_off, const uint32_t* __restrict__ perm,
    uint32_t keep_rows) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = k < n ? (perm ? perm[k] : k) : 0u;
    const uint32_t o = (keep_rows & kLeanOutByItem) ? k : r;
    keep_rows &= kKeepRows;
    const uint8_t* blob = stage_blob<SHARED>(sets[SHARED || !set_of_req ? 0 : set_of_req[r]]);
    if (k >= n) return;
    extern __shared__ uint4 s_lean_dyn[];
    uint8_t* wring = reinterpret_cast<uint8_t*>(s_lean_dyn) + ring_off + (threadIdx.x >> 6) * lean::kRingBytesPerWave;
    const RowRef row = wave_row(rows, row_stride, k);
    const uint8_t* d = arena + offs[r];
    const uint32_t len = lens[r], lane = threadIdx.x & 63u;
    const uint32_t mis = (uint32_t)((uintptr_t)d & 15u);
    uint64_t dec[2] = {0ull, 0ull};
    lean_request<ABL, ARR>(r, o, blob, d, len, row, wring + lane * 16u, wring + lane * kSpanStride,
                           lean::DmaLoader{reinterpret_cast<const uint4*>(d - mis), (len + mis + 15u) / 16u, wring},
                           keep_rows, slow_count, slow_ids, out_tri, out_err, out_bm, stride, dec);
}

#define AJX_LEAN_K(SH, A, F) reinterpret_cast<const void*>(&ajx_scan_lean<SH, A, F>)
hipError_t launch_lean(const Batch& b, const Results& res, const Work& work, const EvalPlan& plan,
                       const uint32_t* d_perm, hipStream_t stream) {
    if (b.n == 0) return hipSuccess;
    const bool shared = plan.stage_bytes != 0;
    const uint32_t abl = plan.abl;
    static std::atomic<uint64_t> attr_done{0};
    hipError_t e = attr_once(attr_done, [] {
        const void* ks[] = {AJX_LEAN_K(true, 0, false), AJX_LEAN_K(true, 0, true), AJX_LEAN_K(false, 0, true),
#if defined(AJX_LEAN_ABLATIONS)
                            AJX_LEAN_K(true, 1, false), AJX_LEAN_K(true, 2, false), AJX_LEAN_K(true, 3, false),
                            AJX_LEAN_K(true, 4, false), AJX_LEAN_K(true, 1, true), AJX_LEAN_K(true, 2, true),
                            AJX_LEAN_K(true, 3, true), AJX_LEAN_K(true, 4, true)
#endif
        };
        for (const void* k : ks) {
            const hipError_t r = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    });
    if (e != hipSuccess) return e;
    const uint32_t lblock =
        shared ? staged_block(plan.stage_bytes, AJX_LEAN_MAXBLOCK, AJX_LEAN_WAVES, lean::kRingBytesPerWave) : 256u;
    const uint32_t lgrid = (b.n + lblock - 1) / lblock;
    const RingGeom g = ring_geom(plan.stage_bytes, lblock, lean::kRingBytesPerWave);
    const uint32_t keep = (plan.keep_rows ? kKeepRows : 0u) | (plan.out_k && d_perm ? kLeanOutByItem : 0u);
    // (two instances: without and with array walking, by the ruleset's kLeanArr. Its
    // kLeanCaps bit is not looked at: both instances enter captured containers, whether the
    // ruleset needs that or not. Capture-free instances cost the walk loop scratch reloads of
    // spilled scalar registers, which wait behind the ring's loads in flight: measured
    // slower, c2 1.39 against 1.27 ms)
    const bool arr = (plan.lean_feat & kLeanArr) != 0;
    using K = void (*)(const uint8_t* const*, const uint32_t*, const uint8_t*, const uint64_t*, const uint32_t*,
                       uint32_t, uint64_t*, uint32_t, uint32_t*, uint32_t*, uint8_t*, int32_t*, uint64_t*, uint32_t,
                       uint32_t, const uint32_t*, uint32_t);
    K k = nullptr;
    if (abl) {
#if defined(AJX_LEAN_ABLATIONS)
        if (!shared || abl > 4) return hipErrorInvalidValue;
        k = abl == 1 ? (arr ? &ajx_scan_lean<true, 1, true> : &ajx_scan_lean<true, 1, false>)
          : abl == 2 ? (arr ? &ajx_scan_lean<true, 2, true> : &ajx_scan_lean<true, 2, false>)
          : abl == 3 ? (arr ? &ajx_scan_lean<true, 3, true> : &ajx_scan_lean<true, 3, false>)
                     : (arr ? &ajx_scan_lean<true, 4, true> : &ajx_scan_lean<true, 4, false>);
#else
        return hipErrorInvalidValue;  // (a profiling build: scripts/build_variant.sh NAME -DAJX_LEAN_ABLATIONS)
#endif
    } else if (!shared) {
        k = &ajx_scan_lean<false, 0, true>;
    } else {
        k = arr ? &ajx_scan_lean<true, 0, true> : &ajx_scan_lean<true, 0, false>;
    }
    hipLaunchKernelGGL(k, dim3(lgrid), dim3(lblock), g.lds, stream, b.sets, nullptr, b.arena, b.offs, b.lens, b.n,
                       work.rows, work.row_stride, work.slow_count, work.slow_ids, res.tri, res.err, res.bm,
                       res.stride, g.ring_off, d_perm, keep);
    return hipGetLastError();
}
#undef AJX_LEAN_K

// The single-pass kernel for multi-tenant batches (one ruleset per request through
// set_of_req; the caller buckets requests by AuthConfig, so a workgroup's requests form a
// few runs of one ruleset each). The workgroup finds its runs (a run starts where the
// ruleset differs from the previous work-item's) and copies the blobs of its first runs
// into LDS — each blob's hot prefix, [0, hot_bytes), which holds every table this kernel
// reads — as many as fit the staging region; a wave whose requests all fall in staged
// runs reads every table from LDS (each lane from its own run's copy), any other wave
// reads them from global memory. Dynamic LDS: [staging region (ring_off bytes)] [rings].
constexpr uint32_t kTenantRuns = 16;  // runs a workgroup may stage
static_assert(lean::kRingBytesPerWave == kWinRingBytesPerWave, "the tenant kernel's rings serve both scans");
__global__ __launch_bounds__(kFastBlock, AJX_FAST_WAVES) void ajx_scan_fused_tenant(
    const uint8_t* const* __restrict__ sets, const uint32_t* __restrict__ set_of_req,
    const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs, const uint32_t* __restrict__ lens, uint32_t n,
    uint64_t* __restrict__ rows, uint32_t row_stride, uint32_t* __restrict__ slow_count,
    uint32_t* __restrict__ slow_ids, uint8_t* __restrict__ out_tri, int32_t* __restrict__ out_err,
    uint64_t* __restrict__ out_bm, uint32_t stride, uint32_t ring_off, const uint32_t* __restrict__ perm) {
    extern __shared__ uint4 s_stage[];
    __shared__ uint32_t s_wcnt[kFastBlock / 64];
    __shared__ uint32_t s_rsid[kTenantRuns];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, nw = blockDim.x >> 6;
    const uint32_t k = blockIdx.x * blockDim.x + t;  // (the grid covers n: n > 0 here)
    const uint32_t kc = k < n ? k : n - 1u;           // (tail threads: the last request's run)
    const uint32_t r = perm ? perm[kc] : kc;
    const uint32_t sid = set_of_req[r];
    bool start = t == 0;
    if (!start) {
        const uint32_t kp = (k - 1u) < n ? k - 1u : n - 1u;
        start = set_of_req[perm ? perm[kp] : kp] != sid;
    }
    // run index of every work-item: starts before it in the workgroup, minus one
    const uint64_t m = __ballot(start);
    if (lane == 0) s_wcnt[wv] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t base = 0, nrun = 0;
    for (uint32_t i = 0; i < nw; i++) {
        const uint32_t c = s_wcnt[i];
        base += i < wv ? c : 0u;
        nrun += c;
    }
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const uint32_t ridx = base + (uint32_t)__builtin_popcountll(m & upto) - 1u;
    if (start && ridx < kTenantRuns) s_rsid[ridx] = sid;
    __syncthreads();
    // stage the leading runs' blobs while they fit (every thread walks the same list)
    uint32_t nst = 0, off = 0, my_off = 0;
    const uint32_t nr = nrun < kTenantRuns ? nrun : kTenantRuns;
    for (uint32_t j = 0; j < nr; j++) {
        const uint8_t* g = sets[s_rsid[j]];
        const uint32_t bytes = reinterpret_cast<const RulesetHdr*>(g)->hot_bytes;  // (a multiple of 16)
        if (off + bytes > ring_off) break;
        const uint4* src = reinterpret_cast<const uint4*>(g);
        for (uint32_t i = t; i < bytes / 16u; i += blockDim.x) s_stage[off / 16u + i] = src[i];
        if (j == ridx) my_off = off;
        off += bytes;
        nst++;
    }
    __syncthreads();
    const RowRef row = wave_row(rows, row_stride, k);
    const uint8_t* d = arena + offs[r];
    // (wave-uniform: the whole wave takes the LDS tables or the global ones)
    if (__all(ridx < nst)) {
        // a wave whose requests all use one staged ruleset (the caller's bucketing makes most
        // waves so: 84 % of c4's) runs the lean scan on that copy (lean_request,
        // as ajx_scan_lean); a wave of several rulesets, the token scanner with each lane's
        // own copy. (As two kernels, one per kind of wave, each with its own registers: c4
        // 5.57 ms against 4.85 ms for this one.)
        const uint32_t off0 = lean::uni(my_off);
        if (__all(my_off == off0)) {
            const uint8_t* blob = reinterpret_cast<const uint8_t*>(s_stage) + off0;
            if (k >= n) return;
            const uint32_t len = lens[r];
            uint8_t* wring = reinterpret_cast<uint8_t*>(s_stage) + ring_off + wv * lean::kRingBytesPerWave;
            const uint32_t mis = (uint32_t)((uintptr_t)d & 15u);
            uint64_t dec[2] = {0ull, 0ull};
            lean_request<0, true>(r, r, blob, d, len, row, wring + lane * 16u, wring + lane * kSpanStride,
                                  lean::DmaLoader{reinterpret_cast<const uint4*>(d - mis), (len + mis + 15u) / 16u, wring},
                                  0u, slow_count, slow_ids, out_tri, out_err, out_bm, stride, dec);
            return;
        }
    }
    // a wave of several rulesets, or of rulesets not staged: the token scanner, each lane on
    // its own ruleset (its staged copy or the global blob: one generic pointer, one copy of
    // the scanner and of stage B in the kernel, which keeps the lean path's registers)
    const uint8_t* blob = ridx < nst ? reinterpret_cast<const uint8_t*>(s_stage) + my_off : sets[sid];
    if (k >= n) return;
    if (!scan_request(blob, d, lens[r], row, lane_ring(ring_off)) ||
        !finish_request(r, blob, d, row, out_tri, out_err, out_bm, stride)) {
        row[0] = kRowSlow;
        slow_ids[atomicAdd(slow_count, 1u)] = r;
    }
}

hipError_t launch_tenant(const Batch& b, const Results& res, const Work& work, const uint32_t* d_perm,
                         hipStream_t stream) {
    if (b.n == 0) return hipSuccess;
    static std::atomic<uint64_t> attr_done{0};
    hipError_t e = attr_once(attr_done, [] {
        // (the kernel also holds static LDS for its run table: ask only for what its launch
        // uses, the staging region + four window rings)
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&ajx_scan_fused_tenant),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kMaxTenantStageBytes + (kTenantBlock / 64) * kWinRingBytesPerWave);
    });
    if (e != hipSuccess) return e;
    // (staging region: the tenant budget less room for the kernel's static LDS, so two
    // groups still fit a CU)
    const uint32_t tblock = kTenantBlock, tgrid = (b.n + tblock - 1) / tblock;
    const uint32_t toff = kMaxTenantStageBytes - 256u;
    hipLaunchKernelGGL(ajx_scan_fused_tenant, dim3(tgrid), dim3(tblock), toff + (tblock / 64) * kWinRingBytesPerWave,
                       stream, b.sets, b.set_of_req, b.arena, b.offs, b.lens, b.n, work.rows, work.row_stride,
                       work.slow_count, work.slow_ids, res.tri, res.err, res.bm, res.stride, toff, d_perm);
    return hipGetLastError();
}

}  // namespace ajx
