// ajx_plan.h — which kernel a batch gets: the kernel modes by name and the launch plan as a
// pure function of the batch's shape and the context's settings. No HIP include:
// authjx_eval_batch_device fills a PlanIn and allocates and launches what plan_eval
// answers; tests/test_plan.py checks the decision table without a GPU.
#pragma once
#include <stdint.h>

namespace ajx {

// Largest ruleset blob the kernels stage into LDS (a batch over one ruleset).
constexpr uint32_t kMaxSharedBlobBytes = 48 * 1024;
// multi-tenant batches: the LDS an 8-wave workgroup stages its runs' blobs in, next to its
// window rings (16 KiB + 8 x 8 KiB rings per group keeps 2 groups = 4 waves/SIMD per CU;
// c4: 83 % of the waves on one staged ruleset, against 80 % for 4-wave groups with 8 KiB)
constexpr uint32_t kMaxTenantStageBytes = 16 * 1024;
constexpr uint32_t kStreamSpan = 32;  // requests per wave at most (stream::kSpan)

// The streaming path's counters, the first words of a workspace's slow buffer; its slow ids
// follow them (stream_slow_ids). One fill zeroes the first three before a launch. (The other
// paths keep one u32 count there and their ids from word 1.)
struct StreamCounters {
    uint32_t slow;        // requests the exact scan decides (the slow list's length)
    uint32_t stage_b;     // entries on the stage-B list
    uint32_t waves_done;  // waves that finished their span (the small-batch instance elects the last)
    uint32_t exact_published;  // the slow count for the host, kept by the wave that zeroed the others
};
constexpr uint32_t kStreamCounterWords = sizeof(StreamCounters) / sizeof(uint32_t);
inline StreamCounters* stream_counters(uint32_t* slow_buf) { return reinterpret_cast<StreamCounters*>(slow_buf); }
inline uint32_t* stream_slow_ids(uint32_t* slow_buf) { return slow_buf + kStreamCounterWords; }

// A workspace's order buffer for n requests: perm[n] | histogram, kPermHistWords | pos_of[n]
// (launch_len_order). The streaming path, which takes no length order, uses the whole
// buffer as its stage-B list (n entries at most).
constexpr uint32_t kPermHistWords = 4096;  // (the sort needs 2 x 1024 + 1)
struct PermBuf {
    uint32_t* p;
    uint32_t n;
    static constexpr uint64_t words(uint32_t n) { return 2ull * n + kPermHistWords; }
    uint32_t* perm() const { return p; }
    uint32_t* hist() const { return p + n; }
    uint32_t* pos_of() const { return p + n + kPermHistWords; }
    uint32_t* stage_list() const { return p; }
};

// Kernel modes (authjx_debug_ablate; bench.py --kernel-mode). 0 is the product; the others
// are for profiling and comparison. The numbers are what the scripts and DESIGN use.
enum KernelMode : int {
    kModeDefault = 0,
    // 15..18, the lean kernel's stage-A ablations, no stage B, the rows hold checksums (builds
    // with AJX_LEAN_ABLATIONS only): loads, + classification, + walk, whole stage A
    kModeLeanLoads = 15, kModeLeanClassify, kModeLeanWalk, kModeLeanStageA,
    // the default kernels off the streaming path, not "full": no length order, no kept rows
    kModeBare = 40,
    kModeLeanForStream = 41,     // the lean kernel where the streaming kernel would run
    kModeStreamStructural = 50,  // the streaming kernel, its structural pass only
    kModeStreamNoFold = 51,      // the streaming kernel without its fold
    kModeStreamAnyN = 52,        // the streaming kernel for a one-ruleset batch of any size
    kModeStreamClocks = 53,      // the streaming kernel's small-batch phase clocks (over the bitmap)
};

inline bool mode_lean_ablation(int m) { return m >= kModeLeanLoads && m <= kModeLeanStageA; }
inline bool mode_known(int m) {
    return m == kModeDefault || mode_lean_ablation(m) || m == kModeBare || m == kModeLeanForStream ||
           (m >= kModeStreamStructural && m <= kModeStreamClocks);
}

// what the decision reads of a batch (its rulesets: sets[0..n_sets)) and of the context
struct PlanIn {
    uint32_t n, n_sets;
    uint32_t all_stream;                // every ruleset is stream-eligible
    uint32_t max_rec, max_sel, max_blob;  // largest stream records, selectors, blob bytes
    uint32_t n_trees, lean_feat;        // of sets[0]: RulesetHdr pad1[0] (0: no forest), lean_feat
    uint32_t mods;                      // a ruleset has modifier chains or text buffers
    uint32_t bitmap;                    // the caller asks for the T bitmap
    int32_t force_scan, mode, len_sort, no_tenant_stage;
    uint32_t stream_max_n;
};

enum Path : uint32_t {
    kPathExact,    // the exact scan over every request
    kPathStream,   // the streaming kernel, its stage B and the exact scan of what they leave
    kPathLean,     // the lean single-pass kernel (one ruleset)
    kPathTenant,   // the multi-tenant kernel, rulesets staged per workgroup
    kPathFused,    // the multi-tenant token scanner, tables from global memory
    kPathInvalid,  // nothing can run this (a lean ablation without a staged blob): a device error
};
enum StreamMode : uint32_t { kStreamFull, kStreamStructural, kStreamNoFold, kStreamTiming };

struct EvalPlan {
    uint32_t path;         // Path
    uint32_t stream_mode;  // StreamMode (kPathStream)
    uint32_t per;          // requests per wave of the streaming kernel
    uint32_t abl;          // 1..4: the lean ablation (modes 15..18), else 0
    uint32_t keep_rows;    // every request's capture row is kept for authjx_select_from_eval_device
    uint32_t rows_stride;  // u64 words per capture row
    uint32_t stage_bytes;  // blob bytes staged in LDS (several rulesets: at most the tenant budget; 0: none)
    uint32_t len_order;    // work-items take requests in length order
    uint32_t want_pos_of;  // the order's inverse is computed too
    uint32_t out_k;        // outputs written in work-item order and gathered back
    uint32_t tout_bm;      // the work-item-ordered copy has a bitmap part
    uint32_t n_out;        // results per request
    uint32_t lean_feat;    // the lean walker instance (3 takes every ruleset)
    uint32_t mods;         // the exact scan's instance with modifier buffers
};

inline EvalPlan plan_eval(const PlanIn& in) {
    EvalPlan p{};
    const int m = in.mode;
    const bool one = in.n_sets == 1;
    const bool ablation = mode_lean_ablation(m);
    const bool dflt = m == kModeDefault || m == kModeStreamClocks;
    // the streaming kernel: small batches (latency; one request per wave for a multi-tenant
    // batch) whose rulesets all have stream tables; any one-ruleset batch under modes 50..52
    const bool any_n = one && m >= kModeStreamStructural && m <= kModeStreamAnyN;
    const bool use_stream = !in.force_scan && in.all_stream && ((dflt && in.n <= in.stream_max_n) || any_n);
    // requests per wave: 32 for throughput, fewer for a small batch (more waves share it)
    const uint32_t q = (in.n + 2047u) / 2048u;
    p.per = !one ? 1u : !dflt || q > kStreamSpan ? kStreamSpan : q < 1u ? 1u : q;
    // (the streaming kernel's rows carry 4 more words: the eager decisions stage B reads)
    const uint32_t sel_stride = 1u + in.max_sel, rec_stride = 1u + in.max_rec;
    p.rows_stride = use_stream ? (sel_stride > rec_stride ? sel_stride : rec_stride) + 4u : sel_stride;
    // a full kernel: its rows and outputs are the product's (15..18: length order kept)
    const bool full = m == kModeDefault || m == kModeLeanForStream || m == kModeStreamAnyN || ablation;
    // rows kept: one forest ruleset (authjx_compile_forest), a full kernel (not the lean
    // ablations: their rows hold checksums). Only the stream and lean kernels honour it,
    // and one ruleset never takes another path
    p.keep_rows = !in.force_scan && one && full && !ablation && in.n_trees != 0;
    p.n_out = one && in.n_trees ? in.n_trees : 1u;
    p.lean_feat = one ? in.lean_feat : 3u;
    p.mods = in.mods != 0;
    if (in.force_scan) {
        p.path = kPathExact;
        return p;
    }
    if (use_stream) {
        p.path = kPathStream;
        p.stream_mode = m == kModeStreamStructural ? kStreamStructural : m == kModeStreamNoFold ? kStreamNoFold
                        : m == kModeStreamClocks ? kStreamTiming : kStreamFull;
        return p;
    }
    // length-bucketed order: one ruleset for the batch (multi-tenant batches keep the
    // caller's bucketing by AuthConfig unless len_sort > 1), a full kernel, batches worth sorting
    p.len_order = in.len_sort && (one || in.len_sort > 1) && full && in.n >= 4096;
    // one result per request: the outputs in work-item order, gathered back by pos_of
    // (forests, several results per request, keep writing at the request: the gather's
    // strided byte copies cost more than the scattered stores, c5 12.0 -> 12.4 ms)
    p.want_pos_of = p.len_order && one && p.n_out == 1;
    p.out_k = p.want_pos_of && !ablation;  // (the ablations compute the inverse and leave it)
    p.tout_bm = p.want_pos_of && in.bitmap;
    // uniform batch: the blob staged once per workgroup; multi-tenant batch: nonzero turns
    // on the per-workgroup staging of its runs' rulesets
    if (one)
        p.stage_bytes = in.max_blob <= kMaxSharedBlobBytes ? in.max_blob : 0u;
    else if (!in.no_tenant_stage)
        p.stage_bytes = in.max_blob < kMaxTenantStageBytes ? in.max_blob : kMaxTenantStageBytes;
    if (ablation) {
        p.abl = (uint32_t)(m - kModeLeanLoads) + 1u;
        p.path = one && p.stage_bytes ? kPathLean : kPathInvalid;
    } else if (one) {
        p.path = kPathLean;
    } else {
        p.path = p.stage_bytes ? kPathTenant : kPathFused;
    }
    return p;
}

}  // namespace ajx
