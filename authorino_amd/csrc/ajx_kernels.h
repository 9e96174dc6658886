// ajx_kernels.h — host-side launch wrappers for the gfx950 kernels (ajx_kernels.hip,
// ajx_lean.hip). They take the batch, its outputs and the workspace as structs and unpack
// them at the launch: the kernels keep flat __restrict__ parameter lists.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ajx_plan.h"

namespace ajx {

// the requests, on the device: request r is arena[offs[r] .. + lens[r]) under ruleset
// sets[set_of_req[r]] (set_of_req nullptr: every request under sets[0])
struct Batch {
    const uint8_t* const* sets;
    const uint32_t* set_of_req;
    const uint8_t* arena;
    const uint64_t* offs;
    const uint32_t* lens;
    uint32_t n;
};
// the evaluation's outputs: tri-states, error indices and T bitmaps of `stride` u64 words
// per request (err, bm: or nullptr)
struct Results {
    uint8_t* tri;
    int32_t* err;
    uint64_t* bm;
    uint32_t stride;
};
// the stream's workspace: capture rows of row_stride u64 words, and the slow list (the
// requests for the exact scan; slow_ids needs room for n entries)
struct Work {
    uint64_t* rows;
    uint32_t row_stride;
    uint32_t* slow_count;
    uint32_t* slow_ids;
};
// gjson.Get outputs: out = u32[n][stride][3] {start, len, type | esc << 8}; text (optional):
// text_stride bytes per request for built values
struct Values {
    uint32_t* out;
    uint32_t stride;
    uint8_t* text;
    uint32_t text_stride;
};

// The exact scan over every request. mods (here and in EvalPlan): a ruleset of the batch has
// modifier chains (RulesetHdr n_modifiers); the exact scan then runs its instance with
// modifier buffers.
hipError_t launch_eval_scan(const Batch& b, const Results& res, bool mods, hipStream_t stream);

// gjson.Get of every pattern's selector. With work.rows: the single-pass stage A captures all
// spans in one scan per document (rows of 1 + n_selectors u64, requests it can not prove go
// through the exact Get; d_perm: the order work-items take requests in, or nullptr);
// without, the exact Get per selector. shared_blob_bytes: the blob size of sets[0] when
// every request uses it and it fits kMaxSharedBlobBytes, else 0.
hipError_t launch_select(const Batch& b, uint32_t shared_blob_bytes, const Values& v, const Work& work,
                         const uint32_t* d_perm, hipStream_t stream);

// The values of patterns [p0, p0 + stride) of sets[0] from capture rows an earlier
// single-pass evaluation of that ruleset wrote (no document scan; slow rows: exact Get).
// d_perm: that evaluation's work-item order (nullptr: identity); wave_rows: the rows are in
// the fused kernels' wave-interleaved layout (indexed by work-item), else one per request.
hipError_t launch_select_rows(const Batch& b, const Values& v, const Work& work, uint32_t p0, const uint32_t* d_perm,
                              bool wave_rows, hipStream_t stream);

// The single-pass paths of a plan (kPathLean, kPathTenant, kPathFused; kPathInvalid is
// hipErrorInvalidValue): the slow count's fill, the path's kernel, the exact scan of the
// requests it hands over. d_perm: the length order (plan.len_order) or nullptr. With
// plan.out_k the lean kernel writes its outputs to d_tout in work-item order, tri-states |
// error indices | bitmaps at 256-byte aligned offsets (tout_bytes), and ajx_unpermute
// gathers them to request order by d_pos_of (launch_len_order) before the exact scan
// writes its requests' own.
hipError_t launch_eval_fast(const Batch& b, const Results& res, const Work& work, const EvalPlan& plan,
                            const uint32_t* d_perm, const uint32_t* d_pos_of, uint8_t* d_tout, hipStream_t stream);
inline size_t tout_bytes(uint32_t n, uint32_t n_out, uint32_t stride) {
    const size_t a = ((size_t)n * n_out + 255u) & ~(size_t)255u;
    const size_t b = ((size_t)n * n_out * 4u + 255u) & ~(size_t)255u;
    return a + b + (size_t)n * stride * 8u;
}

// The lean single-pass kernel (ajx_lean.hip, one ruleset for the batch): stage A with the
// lean scan and stage B per work-item; requests it can not prove go to work.slow_ids (the
// caller zeroes the count first and runs the exact scan after). Of the plan: stage_bytes
// (the blob of sets[0] staged into LDS; 0: read from global memory), abl (profiling builds
// with AJX_LEAN_ABLATIONS: the stage-A ablations, no stage B), keep_rows, lean_feat
// (RulesetHdr::lean_feat of sets[0]: the walker instance), out_k (res indexed by work-item).
hipError_t launch_lean(const Batch& b, const Results& res, const Work& work, const EvalPlan& plan,
                       const uint32_t* d_perm, hipStream_t stream);

// The multi-tenant single-pass kernel (ajx_lean.hip): each workgroup stages its runs'
// rulesets in LDS; waves of one staged ruleset run the lean scan, others the token scanner.
constexpr uint32_t kTenantBlock = 512;
hipError_t launch_tenant(const Batch& b, const Results& res, const Work& work, const uint32_t* d_perm,
                         hipStream_t stream);

// The streaming kernel (ajx_stream.h), its stage B (ajx_stream_finish) and the exact scan of
// what they hand over: one ruleset for the batch (sets[0], staged in LDS; blob_bytes its
// size, n_rec its stream records), or b.set_of_req (a multi-tenant batch, every ruleset
// stream-eligible): one request per wave under its own ruleset, tables from global memory,
// blob_bytes and n_rec the batch's largest. work.rows: rows of row_stride >= 5 + n_rec words
// for n requests (wave layout, work-item = request): the rows stage B reads, and with
// plan.keep_rows every request's row. d_stage_ids: n u32; work.slow_count: the path's
// StreamCounters (ajx_plan.h), work.slow_ids after them. counters_zero (in): the counters
// are zero already, no fill; (out): this launch leaves them zero (the small-batch instance:
// its last wave clears them, the slow count kept in exact_published). Of the plan: stream_mode, per
// (requests per wave, 1..32: fewer for small batches, so more waves share the walk), mods.
bool stream_eligible(const uint8_t* host_blob, uint32_t blob_bytes);
// capture records of the streaming kernel's rows (n_selectors + exact selectors' prefixes)
uint32_t stream_records(const uint8_t* host_blob);
hipError_t launch_eval_stream(const Batch& b, const Results& res, const Work& work, const EvalPlan& plan,
                              uint32_t blob_bytes, uint32_t n_rec, uint32_t* d_stage_ids, bool* counters_zero,
                              hipStream_t stream);

// Length-bucketed request order for the single-pass kernel: d_perm[n] = request ids,
// longest 8-byte length class first; d_hist needs 2 * 1024 + 1 u32 of scratch.
// d_pos_of (or nullptr): n u32, the inverse (work-item of each request).
hipError_t launch_len_order(const uint32_t* d_lens, uint32_t n, uint32_t* d_hist, uint32_t* d_perm,
                            uint32_t* d_pos_of, hipStream_t stream);

}  // namespace ajx
