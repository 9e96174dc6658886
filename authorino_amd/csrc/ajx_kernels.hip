// ajx_kernels.hip — the gfx950 kernels of the batched evaluator, except the lean and
// multi-tenant single-pass kernels (ajx_lean.hip), and the launchers of every path.
//
//   ajx_eval_scan<MODS>       the exact scan (ajx_device.h gj_get; exact for arbitrary bytes):
//                             per selector an exact gjson.Get scan, the patterns, the fold
//   ajx_eval_scan_list<MODS>  the same over the slow list a faster kernel left
//   ajx_scan_fast<SHARED>     the token scanner (ajx_fast.h), stage A alone: every selector's
//                             value span into the request's capture row (launch_select)
//   ajx_scan_fused            its stage A then stage B, tables from global memory
//                             (multi-tenant batches without staging)
//   ajx_scan_stream<MODE, MT, LAT, FIN>  the streaming kernel (ajx_stream.h), a span of
//                             requests per wave: the walk, the eager fold; FIN: the stage-B list
//   ajx_stream_finish<MT, EXACT>  its stage B over the stage-B list
//   ajx_len_hist, ajx_len_scan, ajx_len_scatter  large batches' counting sort by length class
//   ajx_unpermute             work-item-ordered outputs back to request order
//   ajx_select_values<TEXT>   gjson.Get per pattern selector, from capture rows or exact
// The per-request and per-span bodies of these kernels are in ajx_request.h and
// ajx_stream_body.h (the host test build runs the same text).
// Launchers: launch_eval_scan, launch_eval_stream, launch_eval_fast (the single-pass paths
// of an EvalPlan, ajx_plan.h), launch_len_order, launch_select, launch_select_rows.
#include <hip/hip_runtime.h>

#include <atomic>

#include "ajx_fast.h"
#include "ajx_modifiers.h"
#include "ajx_stream_body.h"
#include "ajx_kernels.h"
#include "ajx_kcommon.h"

namespace ajx {

template <bool MODS>
__global__ __launch_bounds__(256) void ajx_eval_scan(const uint8_t* const* __restrict__ sets,
                                                     const uint32_t* __restrict__ set_of_req,
                                                     const uint8_t* __restrict__ arena,
                                                     const uint64_t* __restrict__ offs,
                                                     const uint32_t* __restrict__ lens, uint32_t n,
                                                     uint8_t* __restrict__ out_tri, int32_t* __restrict__ out_err,
                                                     uint64_t* __restrict__ out_bm, uint32_t stride) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    if constexpr (MODS) {
        ModBufs mb;
        eval_scan_one<true>(r, sets, set_of_req, arena, offs, lens, out_tri, out_err, out_bm, stride, &mb);
    } else {
        eval_scan_one<false>(r, sets, set_of_req, arena, offs, lens, out_tri, out_err, out_bm, stride, nullptr);
    }
}

// the slow list: grid-stride over the ids the fast kernel appended
template <bool MODS>
__global__ __launch_bounds__(256) void ajx_eval_scan_list(const uint8_t* const* __restrict__ sets,
                                                          const uint32_t* __restrict__ set_of_req,
                                                          const uint8_t* __restrict__ arena,
                                                          const uint64_t* __restrict__ offs,
                                                          const uint32_t* __restrict__ lens,
                                                          const uint32_t* __restrict__ slow_count,
                                                          const uint32_t* __restrict__ slow_ids,
                                                          uint8_t* __restrict__ out_tri, int32_t* __restrict__ out_err,
                                                          uint64_t* __restrict__ out_bm, uint32_t stride) {
    const uint32_t cnt = *slow_count;
    if constexpr (MODS) {
        ModBufs mb;
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x)
            eval_scan_one<true>(slow_ids[i], sets, set_of_req, arena, offs, lens, out_tri, out_err, out_bm, stride,
                                &mb);
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x)
            eval_scan_one<false>(slow_ids[i], sets, set_of_req, arena, offs, lens, out_tri, out_err, out_bm, stride,
                                 nullptr);
    }
}

// the exact scan over the slow list; the instance with modifier buffers when the batch's
// rulesets have modifier chains
static void launch_slow_list(const Batch& b, const Results& res, const Work& work, bool mods, uint32_t sgrid,
                             hipStream_t stream) {
    hipLaunchKernelGGL((mods ? ajx_eval_scan_list<true> : ajx_eval_scan_list<false>), dim3(sgrid), dim3(256), 0, stream,
                       b.sets, b.set_of_req, b.arena, b.offs, b.lens, work.slow_count, work.slow_ids, res.tri, res.err,
                       res.bm, res.stride);
}

// Stage A alone (launch_select): structural scan -> capture rows.
template <bool SHARED>
__global__ __launch_bounds__(kFastMaxBlock, AJX_FAST_WAVES) void ajx_scan_fast(const uint8_t* const* __restrict__ sets,
                                                     const uint32_t* __restrict__ set_of_req,
                                                     const uint8_t* __restrict__ arena,
                                                     const uint64_t* __restrict__ offs,
                                                     const uint32_t* __restrict__ lens, uint32_t n,
                                                     uint64_t* __restrict__ rows, uint32_t row_stride,
                                                     uint32_t* __restrict__ slow_count,
                                                     uint32_t* __restrict__ slow_ids, uint32_t ring_off,
                                                     const uint32_t* __restrict__ perm) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = k < n ? (perm ? perm[k] : k) : 0u;
    const uint8_t* blob = stage_blob<SHARED>(sets[SHARED || !set_of_req ? 0 : set_of_req[r]]);
    if (k >= n) return;
    if (!scan_request(blob, arena + offs[r], lens[r], rows + (size_t)r * row_stride, lane_ring(ring_off)))
        slow_ids[atomicAdd(slow_count, 1u)] = r;
}

// The token-scanner single-pass kernel for multi-tenant batches without staging: stage A
// then stage B in the same work-item, every table read from global memory through the
// request's own ruleset. Requests stage A can not prove gjson-equivalent go to the slow list.
__global__ __launch_bounds__(kFastMaxBlock, AJX_FAST_WAVES) void ajx_scan_fused(const uint8_t* const* __restrict__ sets,
                                                      const uint32_t* __restrict__ set_of_req,
                                                      const uint8_t* __restrict__ arena,
                                                      const uint64_t* __restrict__ offs,
                                                      const uint32_t* __restrict__ lens, uint32_t n,
                                                      uint64_t* __restrict__ rows, uint32_t row_stride,
                                                      uint32_t* __restrict__ slow_count,
                                                      uint32_t* __restrict__ slow_ids, uint8_t* __restrict__ out_tri,
                                                      int32_t* __restrict__ out_err, uint64_t* __restrict__ out_bm,
                                                      uint32_t stride, uint32_t ring_off,
                                                      const uint32_t* __restrict__ perm) {
    // work-item k takes request perm[k] (length-bucketed order, see ajx_len_scatter) or k;
    // its capture row is row k of the wave-interleaved layout (wave_row)
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = k < n ? (perm ? perm[k] : k) : 0u;
    const uint8_t* blob = sets[set_of_req ? set_of_req[r] : 0];
    if (k >= n) return;
    const RowRef row = wave_row(rows, row_stride, k);
    const uint8_t* d = arena + offs[r];
    if (!scan_request(blob, d, lens[r], row, lane_ring(ring_off))) {
        slow_ids[atomicAdd(slow_count, 1u)] = r;
        return;
    }
    if (!finish_request(r, blob, d, row, out_tri, out_err, out_bm, stride)) {
        row[0] = kRowSlow;
        slow_ids[atomicAdd(slow_count, 1u)] = r;
    }
}

// The streaming kernel (ajx_stream_body.h stream_body: the span's walk), then, with FIN (a
// small batch without modifier chains), the stage-B list in the wave that finishes last: the
// requests left to the exact scan and those whose stage B could not run on the LDS copy —
// no second launch.
//
// The list is a call, not inlined, so that the exact scan's registers stay out of the walk's
// own allocation (the inlined list took the kernel to 256 VGPRs, AGPR spills and ~1,400 SGPR
// spills)
template <bool MT>
__device__ __noinline__ void stream_fin_list_call(const uint8_t* const* __restrict__ sets,
                                                  const uint32_t* __restrict__ set_of_req,
                                                  const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                                                  const uint32_t* __restrict__ lens, uint32_t cnt,
                                                  StreamCounters* __restrict__ ctr,
                                                  const uint32_t* __restrict__ stage_ids, uint8_t* __restrict__ out_tri,
                                                  int32_t* __restrict__ out_err, uint64_t* __restrict__ out_bm,
                                                  uint32_t stride, uint64_t* __restrict__ rows_out, uint32_t row_stride,
                                                  uint32_t l) {
    stream_fin_list<MT>(sets, set_of_req, arena, offs, lens, cnt, ctr, stage_ids, out_tri, out_err, out_bm, stride,
                        rows_out, row_stride, l);
}

template <int MODE, bool MT = false, bool LAT = false, bool FIN = false>
__global__ __launch_bounds__(256) void ajx_scan_stream(const uint8_t* const* __restrict__ sets,
                                                       const uint32_t* __restrict__ set_of_req,
                                                       const uint8_t* __restrict__ arena,
                                                       const uint64_t* __restrict__ offs,
                                                       const uint32_t* __restrict__ lens, uint32_t n,
                                                       StreamCounters* __restrict__ ctr,
                                                       uint32_t* __restrict__ slow_ids, uint32_t* __restrict__ stage_ids,
                                                       uint8_t* __restrict__ out_tri, int32_t* __restrict__ out_err,
                                                       uint64_t* __restrict__ out_bm, uint32_t stride, uint32_t wave_off,
                                                       uint32_t wave_bytes, uint64_t* __restrict__ rows_out,
                                                       uint32_t row_stride, uint32_t keep_rows, uint32_t per,
                                                       uint32_t merge_slow) {
    extern __shared__ uint4 s_stream_dyn[];
    const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
    const uint32_t span = blockIdx.x * (blockDim.x >> 6) + w;
    const uint64_t c0 = (keep_rows & kKeepTiming) ? stream::clk_now() : 0ull;  // (profiling)
    const uint8_t* blob0 = MT ? nullptr : stage_blob<true>(sets[0]);
    stream_body<MODE, MT, LAT>(sets, set_of_req, arena, offs, lens, n, ctr, slow_ids, stage_ids, out_tri, out_err,
                               out_bm, stride, wave_off, wave_bytes, rows_out, row_stride, keep_rows, per, merge_slow,
                               reinterpret_cast<uint8_t*>(s_stream_dyn), w, l, span, blob0, c0);
    if constexpr (FIN) {
        __threadfence();  // (this wave's stage-B list entries and rows, before its count)
        uint32_t last = 0;
        if (l == 0) last = atomicAdd(&ctr->waves_done, 1u) + 1u == gridDim.x * (blockDim.x >> 6) ? 1u : 0u;
        if (!wave::readlane(last, 0)) return;
        __threadfence();
        const uint32_t cnt = __hip_atomic_load(&ctr->stage_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cnt)
            stream_fin_list_call<MT>(sets, set_of_req, arena, offs, lens, cnt, ctr, stage_ids, out_tri, out_err, out_bm,
                                     stride, rows_out, row_stride, l);
        // every other wave is done with the counters: back to zero for the next launch on
        // this stream (no fill before it), the slow count published for the host
        __threadfence();
        if (l == 0) {
            ctr->exact_published = __hip_atomic_load(&ctr->slow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ctr->slow = 0;
            ctr->stage_b = 0;
            ctr->waves_done = 0;
        }
    }
}

// Stage B of the streaming kernel: one work-item per request on the stage-B list
// (stream_finish_entry). MT, EXACT: there.
template <bool MT = false, int EXACT = 0>
__global__ __launch_bounds__(256) void ajx_stream_finish(const uint8_t* const* __restrict__ sets,
                                                         const uint32_t* __restrict__ set_of_req,
                                                         const uint8_t* __restrict__ arena,
                                                         const uint64_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ lens,
                                                         const uint32_t* __restrict__ stage_ids,
                                                         uint64_t* __restrict__ rows, uint32_t row_stride,
                                                         StreamCounters* __restrict__ ctr,
                                                         uint32_t* __restrict__ slow_ids, uint8_t* __restrict__ out_tri,
                                                         int32_t* __restrict__ out_err, uint64_t* __restrict__ out_bm,
                                                         uint32_t stride) {
    const uint8_t* blob0 = MT ? nullptr : stage_blob<true>(sets[0]);
    const uint32_t cnt = ctr->stage_b;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        if constexpr (!MT && EXACT == 0) {
            // (this instance keeps the entry in its own words: calling stream_finish_entry<false, 0>,
            // which the host tests run, it named one vector register more)
            const uint32_t e = stage_ids[i];
            const uint32_t r = e & ~kStageExact;
            bool ok = false;
            if (!(e & kStageExact))
                ok = stream::finish_full(r, blob0, arena + offs[r], lens[r], wave_row(rows, row_stride, r), out_tri,
                                         out_err, out_bm, stride);
            if (ok) continue;
            slow_ids[atomicAdd(&ctr->slow, 1u)] = r;
        } else {
            stream_finish_entry<MT, EXACT>(stage_ids[i], blob0, sets, set_of_req, arena, offs, lens, rows, row_stride,
                                           ctr, slow_ids, out_tri, out_err, out_bm, stride);
        }
    }
}

bool stream_eligible(const uint8_t* host_blob, uint32_t blob_bytes) {
    const RulesetHdr* h = reinterpret_cast<const RulesetHdr*>(host_blob);
    return h->off_stream != 0 && blob_bytes <= kMaxSharedBlobBytes && (h->flags & kFlagFastOk) &&
           h->n_selectors <= kFastMaxSelectors;
}

uint32_t stream_records(const uint8_t* host_blob) {
    const RulesetHdr* h = reinterpret_cast<const RulesetHdr*>(host_blob);
    return h->off_stream ? reinterpret_cast<const StreamHdr*>(host_blob + h->off_stream)->n_rec : h->n_selectors;
}

static_assert(kStreamSpan == stream::kSpan, "requests per wave");
static_assert(kStreamStructural == 1 && kStreamNoFold == 2, "the streaming kernel's MODE");

// 4-wave workgroups (the kernel's launch bounds), each with its own blob copy
constexpr uint32_t kStreamBlock = 256;
// the largest batch whose stage-B list the last wave runs itself (FIN): at most 8 list
// entries per lane
constexpr uint32_t kFinMaxN = 512;

hipError_t launch_eval_stream(const Batch& b, const Results& res, const Work& work, const EvalPlan& plan,
                              uint32_t blob_bytes, uint32_t n_rec, uint32_t* d_stage_ids, bool* counters_zero,
                              hipStream_t stream) {
    const bool was_zero = counters_zero && *counters_zero;
    if (counters_zero) *counters_zero = false;
    const uint32_t n = b.n;
    if (n == 0) return hipSuccess;
    if (work.row_stride < 5u + n_rec) return hipErrorInvalidValue;
    const bool mt = b.set_of_req != nullptr;
    const bool timing = plan.stream_mode == kStreamTiming;  // (profiling: the LAT instance's phase clocks)
    const int mode = timing ? 0 : (int)plan.stream_mode;  // (the kernel's MODE: 1 structural pass alone, 2 no fold)
    const bool keep_rows = plan.keep_rows != 0, mods = plan.mods != 0;
    uint32_t per = plan.per;
    if (mt) {
        if (mode != 0) return hipErrorInvalidValue;
        per = 1;
    }
    uint32_t wave_off = (blob_bytes + 15u) & ~15u;
    uint32_t wave_bytes = (stream::lds_bytes(n_rec) + 15u) & ~15u;
    if (mt) {
        // each wave copies its own ruleset's blob next to its LDS when it fits (blob_bytes:
        // the batch's largest), else reads it from global memory: wave_off is that room
        const uint32_t room = 160u * 1024u / (kStreamBlock / 64u);
        uint32_t cap = wave_off;
        if (cap + wave_bytes > room) cap = room > wave_bytes ? (room - wave_bytes) & ~15u : 0u;
        if (cap < 1024u) cap = 0;
        wave_off = cap;
        wave_bytes += cap;
    }
    const uint32_t block = kStreamBlock;
    const uint32_t lds = (mt ? 0u : wave_off) + (block / 64) * wave_bytes;
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    if (per == 0 || per > stream::kSpan) per = stream::kSpan;
    // a small batch (fewer requests per wave, or one per wave under its own ruleset): stage B
    // runs the exact scan too (one launch fewer on the latency path)
    const bool merge = mt || per < stream::kSpan;
    const uint32_t spans = (n + per - 1) / per;
    const uint32_t grid = (spans + block / 64 - 1) / (block / 64);
    // (one fill: the slow count, the stage-B count and the finished-wave count; none after a
    // FIN launch on this stream, whose last wave cleared them)
    StreamCounters* const ctr = stream_counters(work.slow_count);
    hipError_t e = hipSuccess;
    if (!was_zero && (e = hipMemsetAsync(ctr, 0, offsetof(StreamCounters, exact_published), stream)) != hipSuccess)
        return e;
    static std::atomic<uint64_t> attr_done{0};
    e = attr_once(attr_done, [] {
        for (const void* k : {reinterpret_cast<const void*>(&ajx_scan_stream<0>),
                              reinterpret_cast<const void*>(&ajx_scan_stream<1>),
                              reinterpret_cast<const void*>(&ajx_scan_stream<2>),
                              reinterpret_cast<const void*>(&ajx_scan_stream<0, true>),
                              reinterpret_cast<const void*>(&ajx_scan_stream<0, false, true>),
                              reinterpret_cast<const void*>(&ajx_scan_stream<0, true, true>),
                              reinterpret_cast<const void*>(&ajx_scan_stream<0, false, true, true>),
                              reinterpret_cast<const void*>(&ajx_scan_stream<0, true, true, true>),
                              reinterpret_cast<const void*>(&ajx_stream_finish<false>),
                              reinterpret_cast<const void*>(&ajx_stream_finish<false, 1>),
                              reinterpret_cast<const void*>(&ajx_stream_finish<false, 2>),
                              reinterpret_cast<const void*>(&ajx_stream_finish<true, 1>),
                              reinterpret_cast<const void*>(&ajx_stream_finish<true, 2>)}) {
            // (the dynamic ceiling is what the kernel's static LDS leaves of the CU's 160 KiB:
            // stage B's per-thread buffers are static)
            hipFuncAttributes fa;
            hipError_t r = hipFuncGetAttributes(&fa, k);
            if (r != hipSuccess) return r;
            r = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024 - (int)fa.sharedSizeBytes);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    });
    if (e != hipSuccess) return e;
#define AJX_STREAM_LAUNCH(M, T, LT, F)                                                                           \
    hipLaunchKernelGGL((ajx_scan_stream<M, T, LT, F>), dim3(grid), dim3(block), lds, stream, b.sets, b.set_of_req, \
                       b.arena, b.offs, b.lens, n, ctr, work.slow_ids, d_stage_ids, res.tri, res.err, res.bm,      \
                       res.stride, wave_off, wave_bytes, work.rows, work.row_stride,                                \
                       (keep_rows ? kKeepRows : 0u) | (timing ? kKeepTiming : 0u), per, merge ? 1u : 0u)
    const bool lat = merge && !keep_rows;
    // (stage B and the exact scan in the last wave: no second launch). Only for batches of at
    // most kFinMaxN requests: that wave walks the list 64 entries at a time, so a large batch
    // of requests the stream cannot finish (long or deeply nested documents) would put
    // thousands of exact scans behind one wave; larger batches take the grid-stride
    // ajx_stream_finish launch
    const bool fin = lat && !mods && n <= kFinMaxN;
    if (mt && fin)
        AJX_STREAM_LAUNCH(0, true, true, true);
    else if (mt && lat)
        AJX_STREAM_LAUNCH(0, true, true, false);
    else if (mt)
        AJX_STREAM_LAUNCH(0, true, false, false);
    else if (mode == 1)
        AJX_STREAM_LAUNCH(1, false, false, false);
    else if (mode == 2)
        AJX_STREAM_LAUNCH(2, false, false, false);
    else if (fin)
        AJX_STREAM_LAUNCH(0, false, true, true);
    else if (lat)
        AJX_STREAM_LAUNCH(0, false, true, false);
    else
        AJX_STREAM_LAUNCH(0, false, false, false);
#undef AJX_STREAM_LAUNCH
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (counters_zero) *counters_zero = fin && (mt || (mode != 1 && mode != 2));
    if (mode != 0 || fin) return hipSuccess;
    // stage B and the exact scan over their lists (grid-stride: the lists' lengths are on the device)
    const uint32_t fgrid = n < 2048u * 256u ? (n + 255) / 256 : 4096;
#define AJX_FINISH_LAUNCH(T, X, LDS)                                                                            \
    hipLaunchKernelGGL((ajx_stream_finish<T, X>), dim3(fgrid), dim3(256), LDS, stream, b.sets,                     \
                       T ? b.set_of_req : nullptr, b.arena, b.offs, b.lens, d_stage_ids, work.rows,                \
                       work.row_stride, ctr, work.slow_ids, res.tri, res.err, res.bm, res.stride)
    if (mt && mods)
        AJX_FINISH_LAUNCH(true, 2, 0);
    else if (mt)
        AJX_FINISH_LAUNCH(true, 1, 0);
    else if (merge && mods)
        AJX_FINISH_LAUNCH(false, 2, wave_off);
    else if (merge)
        AJX_FINISH_LAUNCH(false, 1, wave_off);
    else
        AJX_FINISH_LAUNCH(false, 0, wave_off);
#undef AJX_FINISH_LAUNCH
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (merge) return hipSuccess;
    const uint32_t sgrid = n < 1024u * 128u ? 2 * ((n + 255) / 256) : 4096;
    launch_slow_list(b, res, work, mods, sgrid, stream);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Length bucketing: a wave of the single-pass kernel runs each window's token loop as
// long as its busiest lane, and the whole document loop as long as its longest
// document, so the 64 requests of a wave should have similar lengths. A counting sort
// by 8-byte length class (longest first; documents over 8 KiB share the last class)
// gives the order work-items take requests in; outputs still go to each request's own
// index. Three small launches over lens[] (4 B
// per request each).
// ---------------------------------------------------------------------------------
constexpr uint32_t kLenBuckets = 1024;

__device__ __forceinline__ uint32_t len_bucket(uint32_t len) {
    const uint32_t b = len >> 3;
    return kLenBuckets - 1u - (b < kLenBuckets ? b : kLenBuckets - 1u);
}

__global__ __launch_bounds__(kLenBuckets) void ajx_len_hist(const uint32_t* __restrict__ lens, uint32_t n,
                                                            uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kLenBuckets];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        atomicAdd(&h[len_bucket(lens[i])], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// exclusive scan of the histogram into per-class cursors (one workgroup).
// cursor[kLenBuckets] = 1 when the lengths span fewer than kLenSpreadMin classes: the
// order would not even out the waves (and scatters the outputs), so the scatter writes
// the identity instead.
constexpr uint32_t kLenSpreadMin = 32;  // 256 bytes
__global__ __launch_bounds__(kLenBuckets) void ajx_len_scan(const uint32_t* __restrict__ hist,
                                                            uint32_t* __restrict__ cursor) {
    __shared__ uint32_t s[kLenBuckets];
    __shared__ uint32_t lo, hi;
    const uint32_t t = threadIdx.x;
    const uint32_t own = hist[t];
    if (t == 0) {
        lo = kLenBuckets;
        hi = 0;
    }
    s[t] = own;
    __syncthreads();
    if (own) {
        atomicMin(&lo, t);
        atomicMax(&hi, t);
    }
    for (uint32_t o = 1; o < kLenBuckets; o <<= 1) {
        const uint32_t v = t >= o ? s[t - o] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    cursor[t] = s[t] - own;
    if (t == 0) cursor[kLenBuckets] = (hi < lo || hi - lo < kLenSpreadMin) ? 1u : 0u;
}

// perm[cursor[class] + rank] = request; one global atomic per (workgroup, class).
// pos_of (optional): pos_of[request] = its work-item, written in request order (coalesced),
// for the gather that puts work-item-ordered outputs back in request order (ajx_unpermute)
__global__ __launch_bounds__(kLenBuckets) void ajx_len_scatter(const uint32_t* __restrict__ lens, uint32_t n,
                                                               uint32_t* __restrict__ cursor,
                                                               uint32_t* __restrict__ perm,
                                                               uint32_t* __restrict__ pos_of) {
    __shared__ uint32_t cnt[kLenBuckets];
    __shared__ uint32_t base[kLenBuckets];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (cursor[kLenBuckets]) {  // narrow length spread: keep the caller's order
        if (i < n) {
            perm[i] = i;
            if (pos_of) pos_of[i] = i;
        }
        return;
    }
    cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t b = 0, rank = 0;
    if (i < n) {
        b = len_bucket(lens[i]);
        rank = atomicAdd(&cnt[b], 1u);
    }
    __syncthreads();
    if (cnt[threadIdx.x]) base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], cnt[threadIdx.x]);
    __syncthreads();
    if (i < n) {
        perm[base[b] + rank] = i;
        if (pos_of) pos_of[i] = base[b] + rank;
    }
}

// outputs written in work-item order (t_*) back to request order: request i's results are
// work-item pos_of[i]'s. One thread per request, so the stores are coalesced; the loads are
// a gather over the work-item-ordered copies (n x (n_out x 5 + stride x 8) bytes, mostly
// still in L2 / MALL behind the kernel that wrote them).
__global__ __launch_bounds__(256) void ajx_unpermute(const uint32_t* __restrict__ pos_of, uint32_t n, uint32_t n_out,
                                                     uint32_t stride, const uint8_t* __restrict__ t_tri,
                                                     const int32_t* __restrict__ t_err,
                                                     const uint64_t* __restrict__ t_bm, uint8_t* __restrict__ tri,
                                                     int32_t* __restrict__ err, uint64_t* __restrict__ bm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t j = pos_of[i];
    for (uint32_t q = 0; q < n_out; q++) {
        tri[(size_t)i * n_out + q] = t_tri[j * n_out + q];
        if (err) err[(size_t)i * n_out + q] = t_err[j * n_out + q];
    }
    if (bm)
        for (uint32_t w = 0; w < stride; w++) bm[(size_t)i * stride + w] = t_bm[j * stride + w];
}

hipError_t launch_len_order(const uint32_t* d_lens, uint32_t n, uint32_t* d_hist, uint32_t* d_perm,
                            uint32_t* d_pos_of, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_hist, 0, (2 * kLenBuckets + 1) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t blocks = (n + kLenBuckets - 1) / kLenBuckets;
    hipLaunchKernelGGL(ajx_len_hist, dim3(blocks < 512 ? blocks : 512), dim3(kLenBuckets), 0, stream, d_lens, n,
                       d_hist);
    hipLaunchKernelGGL(ajx_len_scan, dim3(1), dim3(kLenBuckets), 0, stream, d_hist, d_hist + kLenBuckets);
    hipLaunchKernelGGL(ajx_len_scatter, dim3(blocks), dim3(kLenBuckets), 0, stream, d_lens, n, d_hist + kLenBuckets,
                       d_perm, d_pos_of);
    return hipGetLastError();
}

// gjson.Get per pattern selector (the response / header selectors of SURVEY.md §8 a14):
// one work-item per request (select_request, ajx_request.h).
template <bool TEXT>
__global__ __launch_bounds__(256) void ajx_select_values(const uint8_t* const* __restrict__ sets,
                                                         const uint32_t* __restrict__ set_of_req,
                                                         const uint8_t* __restrict__ arena,
                                                         const uint64_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ lens, uint32_t n,
                                                         uint32_t* __restrict__ out, uint32_t stride,
                                                         const uint64_t* __restrict__ rows, uint32_t row_stride,
                                                         uint32_t p0, const uint32_t* __restrict__ perm,
                                                         uint32_t wave_rows, uint8_t* __restrict__ text,
                                                         uint32_t text_stride) {
    // work-item k: request perm[k] (the order the rows were written in) or k; its row is
    // row k of the wave-interleaved layout (wave_rows: the fused kernels') or row r
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t r = perm ? perm[k] : k;
    select_request<TEXT>(r, k, sets, set_of_req, arena, offs, lens, out, stride, rows, row_stride, p0, wave_rows, text,
                         text_stride);
}

hipError_t launch_select(const Batch& b, uint32_t shared_blob_bytes, const Values& v, const Work& work,
                         const uint32_t* d_perm, hipStream_t stream) {
    const uint32_t n = b.n;
    if (n == 0) return hipSuccess;
    if (work.rows) {  // stage A of the single-pass kernel captures every selector's span
        const bool shared = shared_blob_bytes != 0 && b.set_of_req == nullptr;
        const uint32_t fblock = shared ? fast_block(shared_blob_bytes) : kFastBlock;
        const uint32_t fgrid = (n + fblock - 1) / fblock;
        const RingGeom g = ring_geom(shared ? shared_blob_bytes : 0u, fblock);
        hipError_t e = hipMemsetAsync(work.slow_count, 0, sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        static std::atomic<uint64_t> attr_done{0};
        e = attr_once(attr_done, [] {
            const void* ks[] = {reinterpret_cast<const void*>(&ajx_scan_fast<true>),
                                reinterpret_cast<const void*>(&ajx_scan_fast<false>)};
            for (const void* k : ks) {
                const hipError_t r = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                if (r != hipSuccess) return r;
            }
            return hipSuccess;
        });
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((shared ? ajx_scan_fast<true> : ajx_scan_fast<false>), dim3(fgrid), dim3(fblock), g.lds,
                           stream, b.sets, b.set_of_req, b.arena, b.offs, b.lens, n, work.rows, work.row_stride,
                           work.slow_count, work.slow_ids, g.ring_off, d_perm);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const uint32_t block = 256;
    const uint32_t grid = (n + block - 1) / block;
    hipLaunchKernelGGL((v.text ? ajx_select_values<true> : ajx_select_values<false>), dim3(grid), dim3(block), 0, stream,
                       b.sets, b.set_of_req, b.arena, b.offs, b.lens, n, v.out, v.stride, work.rows, work.row_stride, 0u,
                       nullptr, 0u, v.text, v.text ? v.text_stride : 0u);
    return hipGetLastError();
}

hipError_t launch_select_rows(const Batch& b, const Values& v, const Work& work, uint32_t p0, const uint32_t* d_perm,
                              bool wave_rows, hipStream_t stream) {
    if (b.n == 0) return hipSuccess;
    const uint32_t block = 256;
    const uint32_t grid = (b.n + block - 1) / block;
    hipLaunchKernelGGL(ajx_select_values<false>, dim3(grid), dim3(block), 0, stream, b.sets, nullptr, b.arena, b.offs,
                       b.lens, b.n, v.out, v.stride, work.rows, work.row_stride, p0, d_perm, wave_rows ? 1u : 0u,
                       nullptr, 0u);
    return hipGetLastError();
}

hipError_t launch_eval_scan(const Batch& b, const Results& res, bool mods, hipStream_t stream) {
    if (b.n == 0) return hipSuccess;
    const uint32_t block = 256;
    const uint32_t grid = (b.n + block - 1) / block;
    hipLaunchKernelGGL((mods ? ajx_eval_scan<true> : ajx_eval_scan<false>), dim3(grid), dim3(block), 0, stream, b.sets,
                       b.set_of_req, b.arena, b.offs, b.lens, b.n, res.tri, res.err, res.bm, res.stride);
    return hipGetLastError();
}

hipError_t launch_eval_fast(const Batch& b, const Results& res, const Work& work, const EvalPlan& plan,
                            const uint32_t* d_perm, const uint32_t* d_pos_of, uint8_t* d_tout, hipStream_t stream) {
    const uint32_t n = b.n;
    if (n == 0) return hipSuccess;
    if (plan.path != kPathLean && plan.path != kPathTenant && plan.path != kPathFused) return hipErrorInvalidValue;
    // (the exact scan's grid follows the token scanner's workgroup size for the staged blob)
    const uint32_t block = plan.path == kPathLean && plan.stage_bytes ? fast_block(plan.stage_bytes) : kFastBlock;
    const uint32_t grid = (n + block - 1) / block;
    hipError_t e = hipMemsetAsync(work.slow_count, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (plan.path == kPathLean) {
        // the lean single-pass kernel (one ruleset; ajx_lean.hip), or its profiling ablations
        // (multi-tenant batches: the staged tenant scanner below. Measured on c4, the lean
        // scan with per-lane table parameters took 6.39 ms and one pass per ruleset of a
        // wave 7.3-7.8 ms, against 5.38 ms for the tenant kernel's LDS-staged tables)
        // in length order, the outputs go to d_tout in work-item order and are gathered back
        // (ajx_unpermute) before the exact scan writes its requests' own
        const bool out_k = plan.out_k != 0;  // (with it come d_perm, d_pos_of and d_tout)
        const size_t o_err = ((size_t)n * plan.n_out + 255u) & ~(size_t)255u;
        const size_t o_bm = o_err + (((size_t)n * plan.n_out * 4u + 255u) & ~(size_t)255u);
        const Results k_res =
            out_k ? Results{d_tout, res.err ? reinterpret_cast<int32_t*>(d_tout + o_err) : nullptr,
                            res.bm ? reinterpret_cast<uint64_t*>(d_tout + o_bm) : nullptr, res.stride}
                  : res;
        e = launch_lean(b, k_res, work, plan, d_perm, stream);
        if (e != hipSuccess || plan.abl) return e;
        if (out_k) {
            hipLaunchKernelGGL(ajx_unpermute, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_pos_of, n, plan.n_out,
                               res.stride, k_res.tri, k_res.err, k_res.bm, res.tri, res.err, res.bm);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    } else if (plan.path == kPathTenant) {
        // multi-tenant batch, staging on: each workgroup stages its runs' rulesets, those that
        // fit (ajx_scan_fused_tenant)
        if ((e = launch_tenant(b, res, work, d_perm, stream)) != hipSuccess) return e;
    } else {
        static std::atomic<uint64_t> attr_done{0};
        e = attr_once(attr_done, [] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(&ajx_scan_fused),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        });
        if (e != hipSuccess) return e;
        const RingGeom g = ring_geom(0u, block);
        hipLaunchKernelGGL(ajx_scan_fused, dim3(grid), dim3(block), g.lds, stream, b.sets, b.set_of_req, b.arena,
                           b.offs, b.lens, n, work.rows, work.row_stride, work.slow_count, work.slow_ids, res.tri,
                           res.err, res.bm, res.stride, g.ring_off, d_perm);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t sgrid = grid < 2048 ? 2 * grid : 4096;
    launch_slow_list(b, res, work, plan.mods != 0, sgrid, stream);
    return hipGetLastError();
}

}  // namespace ajx
