// ajx_api.cpp — the C-ABI (include/authjx.h): device contexts, reconcile-time compile
// into HBM-resident rulesets, batch evaluation.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "ajx_host.h"
#include "ajx_blob.h"
#include "ajx_kernels.h"

thread_local AjxLastError ajx_last_error;

// The end-of-batch event of a workspace, shared with the registry (authjx_free waits on
// it outside any lock): destroyed when the last holder lets go.
struct EndEvent {
    hipEvent_t ev = nullptr;
    ~EndEvent() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

// Per-stream scratch of a context: every distinct stream a context is called with gets
// its own set table, slow list, capture rows and request order, so batches on two
// streams of one context never share a buffer; calls on one stream take its mutex
// (their kernels are ordered by the stream anyway).
//
// Lifetime: every user (a call through WsLock, the last_* readers) holds a reference,
// taken and dropped under ctx->mu. Releasing the stream (authjx_release_stream, a
// batcher's private streams) retires the workspace: it leaves ctx->ws and ctx->last_ws at
// once, and whoever drops the last reference destroys it.
struct Workspace {
    hipStream_t stream = nullptr;
    uint64_t id = 0;  // registry id (ruleset users)
    uint32_t refs = 0;     // (ctx->mu)
    bool retired = false;  // (ctx->mu)
    std::mutex mu;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // ev1: end of the last batch on this stream
    std::shared_ptr<EndEvent> end;            // owns ev1
    // the ruleset pointer table the kernels index by set_of_req: two slots (device + pinned
    // source each), so a batch over another ruleset list fills the slot the batch before
    // the last one used (its event, not a stream synchronize, guards the reuse)
    const uint8_t** d_sets = nullptr;  // the current slot's device table
    ajx::DeviceBuf sets_dev;
    ajx::PinnedBuf sets_host;
    uint32_t sets_cap = 0;  // entries per slot
    uint32_t sets_slot = 0;
    hipEvent_t sets_ev[2] = {nullptr, nullptr};
    bool sets_ev_rec[2] = {false, false};
    std::vector<const uint8_t*> last_sets;
    ajx::PtrTable progs;  // the render programs of a multi-program batch (with_ptr_table)
    // [0] = count, [1..] = ids: requests for the exact scan (the streaming kernel: its
    // ajx::StreamCounters, the ids after them)
    ajx::DeviceBuf slow;
    // the streaming kernel's small-batch instance (FIN) leaves its counters zero for the next
    // launch on this stream (no fill) and publishes its exact-path count (exact_published)
    bool cnt_zero = false, exact_published = false;
    ajx::DeviceBuf rows;  // stage-A capture rows (u64)
    // length-bucketed request order and the streaming kernel's stage-B list (ajx::PermBuf)
    ajx::DeviceBuf perm;
    ajx::DeviceBuf tout;  // the lean kernel's outputs in work-item order (tout_bytes)
    // the capture rows in `rows`: written by the last single-ruleset, full evaluation of
    // rows_rs over rows_n requests on this stream (nullptr: none usable)
    const authjx_ruleset* rows_rs = nullptr;
    uint32_t rows_n = 0, rows_stride = 0;
    const uint32_t* rows_perm = nullptr;  // that evaluation's work-item order (d_perm or none)
    bool rows_wave = false;               // rows in the fused kernels' wave-interleaved layout
    bool ran = false;  // ev0 / ev1 recorded
};

namespace {
// live workspaces: id -> end-of-last-batch event; authjx_free looks its ruleset's users
// up here (an id that is gone belongs to a workspace already destroyed)
std::mutex g_reg_mu;
std::vector<std::pair<uint64_t, std::shared_ptr<EndEvent>>> g_reg;
uint64_t g_next_ws = 1;

// the workspace of stream s (created on first use); ctx->mu held by the caller
Workspace* workspace_of(authjx_ctx* ctx, hipStream_t s) {
    for (Workspace* w : ctx->ws)
        if (w->stream == s) return w;
    Workspace* w = new Workspace();
    w->stream = s;
    w->end = std::make_shared<EndEvent>();
    if (hipEventCreate(&w->ev0) != hipSuccess || hipEventCreate(&w->end->ev) != hipSuccess) {
        if (w->ev0) (void)hipEventDestroy(w->ev0);
        delete w;
        return nullptr;
    }
    w->ev1 = w->end->ev;
    {
        std::lock_guard<std::mutex> lock(g_reg_mu);
        w->id = g_next_ws++;
        g_reg.push_back({w->id, w->end});
    }
    ctx->ws.push_back(w);
    return w;
}

void destroy_workspace(Workspace* w) {
    if (w->ran) (void)hipEventSynchronize(w->ev1);
    {
        std::lock_guard<std::mutex> lock(g_reg_mu);
        for (size_t i = 0; i < g_reg.size(); i++)
            if (g_reg[i].first == w->id) {
                g_reg.erase(g_reg.begin() + (long)i);
                break;
            }
    }
    for (int k = 0; k < 2; k++) {
        if (w->sets_ev[k]) (void)hipEventDestroy(w->sets_ev[k]);
        if (w->progs.ev[k]) (void)hipEventDestroy(w->progs.ev[k]);
    }
    if (w->ev0) (void)hipEventDestroy(w->ev0);
    delete w;  // (its buffers; ev1 goes with the last holder of w->end)
}

// a reference to w (ctx->mu held by the caller)
Workspace* ws_ref(Workspace* w) {
    if (w) w->refs++;
    return w;
}
// drops a reference; the last one of a retired workspace destroys it
void ws_unref(authjx_ctx* ctx, Workspace* w) {
    bool dead;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        dead = --w->refs == 0 && w->retired;
    }
    if (dead) destroy_workspace(w);  // (waits for the stream's last batch)
}

// d_pre: the caller's device copy of the blob pointers (the micro-batcher's staging buffer,
// one copy with the documents), used as is
int ensure_sets(Workspace* w, int device, const authjx_ruleset* const* sets, uint32_t n_sets,
                const uint8_t* const* d_pre = nullptr) {
    std::vector<const uint8_t*> ptrs(n_sets);
    for (uint32_t i = 0; i < n_sets; i++) {
        if (!sets[i] || sets[i]->device != device) return AUTHJX_EINVAL;
        ptrs[i] = sets[i]->d_blob.data();
    }
    if (d_pre) {
        w->d_sets = const_cast<const uint8_t**>(d_pre);
        w->last_sets.clear();  // (the next call without one copies its table again)
        return AUTHJX_OK;
    }
    if (ptrs == w->last_sets) return AUTHJX_OK;
    if (n_sets > w->sets_cap) {  // (grows: the stream's previous batches may read the old table)
        const uint32_t cap = n_sets < 64 ? 64 : n_sets;
        w->d_sets = nullptr;
        w->sets_cap = 0;
        w->sets_ev_rec[0] = w->sets_ev_rec[1] = false;
        HIP_OK(w->sets_dev.reserve(2 * cap * sizeof(uint8_t*), w->stream));
        HIP_OK(w->sets_host.reserve(2 * cap * sizeof(uint8_t*), w->stream));
        for (int k = 0; k < 2; k++)
            if (!w->sets_ev[k]) HIP_OK(hipEventCreateWithFlags(&w->sets_ev[k], hipEventDisableTiming));
        w->sets_cap = cap;
    }
    // the other slot: free once the last batch that used it has finished
    const uint32_t k = w->d_sets ? 1u - w->sets_slot : 0u;
    if (w->sets_ev_rec[k]) HIP_OK(hipEventSynchronize(w->sets_ev[k]));
    const uint8_t** h = w->sets_host.as<const uint8_t*>() + (size_t)k * w->sets_cap;
    const uint8_t** dv = w->sets_dev.as<const uint8_t*>() + (size_t)k * w->sets_cap;
    std::memcpy(h, ptrs.data(), n_sets * sizeof(uint8_t*));
    HIP_OK(hipMemcpyAsync(dv, h, n_sets * sizeof(uint8_t*), hipMemcpyHostToDevice, w->stream));
    w->sets_slot = k;
    w->d_sets = dv;
    w->last_sets = ptrs;
    return AUTHJX_OK;
}

// capture rows, slow list and request order for a batch of n (grown when needed, after
// this stream's earlier batches are done with the old buffers)
int ensure_work(Workspace* w, uint32_t n, uint32_t row_stride) {
    // (rows for whole waves: the fused kernels' wave-interleaved layout)
    const size_t slow_bytes = ((size_t)n + ajx::kStreamCounterWords) * sizeof(uint32_t);
    const size_t perm_bytes = ajx::PermBuf::words(n) * sizeof(uint32_t);
    const size_t rows_bytes = (size_t)((n + 63u) & ~63u) * row_stride * sizeof(uint64_t);
    if (slow_bytes <= w->slow.capacity() && perm_bytes <= w->perm.capacity() && rows_bytes <= w->rows.capacity())
        return AUTHJX_OK;
    w->rows_rs = nullptr;
    if (slow_bytes > w->slow.capacity()) w->cnt_zero = w->exact_published = false;
    HIP_OK(w->slow.reserve(slow_bytes, w->stream));
    HIP_OK(w->perm.reserve(perm_bytes, w->stream));
    HIP_OK(w->rows.reserve(rows_bytes, w->stream));
    return AUTHJX_OK;
}

// a device call's workspace, locked: ctx->mu only while the workspace is looked up, not
// while waiting for a busy stream's workspace (calls on the context's other streams, the
// batcher's workers among them, go on meanwhile). The reference taken with the lookup keeps
// the workspace alive while this call waits for its mutex, even if its stream is released
// meanwhile. Lock order: w->mu before ctx->mu.
struct WsLock {
    authjx_ctx* ctx;
    Workspace* w = nullptr;
    std::unique_lock<std::mutex> lock;
    WsLock(authjx_ctx* c, void* stream) : ctx(c) {
        {
            std::lock_guard<std::mutex> g(ctx->mu);
            w = ws_ref(workspace_of(ctx, stream ? (hipStream_t)stream : ctx->stream));
        }
        if (w) {
            lock = std::unique_lock<std::mutex>(w->mu);
            std::lock_guard<std::mutex> g(ctx->mu);
            if (!w->retired) ctx->last_ws = w;
        }
    }
    ~WsLock() {
        if (!w) return;
        lock.unlock();
        ws_unref(ctx, w);
    }
    WsLock(const WsLock&) = delete;
    WsLock& operator=(const WsLock&) = delete;
};

// ctx->last_ws with a reference (the last_* readers)
struct LastWs {
    authjx_ctx* ctx;
    Workspace* w = nullptr;
    int force_scan = 0;
    explicit LastWs(authjx_ctx* c) : ctx(c) {
        std::lock_guard<std::mutex> g(ctx->mu);
        w = ws_ref(ctx->last_ws);
        force_scan = ctx->force_scan;
    }
    ~LastWs() {
        if (w) ws_unref(ctx, w);
    }
    LastWs(const LastWs&) = delete;
    LastWs& operator=(const LastWs&) = delete;
};

// after the launches of a batch: ev1 marks its end on the stream; the rulesets record
// this workspace as a user
int batch_done(Workspace* w, const authjx_ruleset* const* sets, uint32_t n_sets) {
    HIP_OK(hipEventRecord(w->ev1, w->stream));
    if (w->sets_ev[w->sets_slot]) {  // (the end of the last batch that read this set-table slot)
        HIP_OK(hipEventRecord(w->sets_ev[w->sets_slot], w->stream));
        w->sets_ev_rec[w->sets_slot] = true;
    }
    w->ran = true;
    for (uint32_t i = 0; i < n_sets; i++) const_cast<authjx_ruleset*>(sets[i])->note_use(w->id);
    return AUTHJX_OK;
}

// what the choice of kernels reads (ajx_plan.h): the batch's shape, its rulesets' facts
// (finish_compile) and the context's settings
ajx::PlanIn plan_in(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets, uint32_t n, bool bitmap) {
    ajx::PlanIn in{};
    in.n = n;
    in.n_sets = n_sets;
    in.all_stream = 1;
    for (uint32_t i = 0; i < n_sets; i++) {
        in.all_stream = in.all_stream && sets[i]->stream_ok;
        in.max_rec = std::max(in.max_rec, sets[i]->stream_rec);
        in.max_sel = std::max(in.max_sel, sets[i]->c.n_selectors);
        in.max_blob = std::max(in.max_blob, sets[i]->blob_bytes);
        in.mods = in.mods || sets[i]->mods;
    }
    in.n_trees = sets[0]->hdr_trees;
    in.lean_feat = sets[0]->lean_feat;
    in.bitmap = bitmap;
    std::lock_guard<std::mutex> g(ctx->mu);
    in.force_scan = ctx->force_scan;
    in.mode = ctx->mode;
    in.len_sort = ctx->len_sort;
    in.no_tenant_stage = ctx->no_tenant_stage;
    in.stream_max_n = ctx->stream_max_n;
    return in;
}

// the kept capture rows of rs hold patterns [first, first + count)'s records: a selector the
// scan decides eagerly has one only when it belongs to a root-less tree of the forest (kEagerKeep)
bool rows_hold_patterns(const authjx_ruleset* rs, uint32_t first, uint32_t count) {
    const uint8_t* blob = rs->c.blob.data();
    const auto* h = reinterpret_cast<const ajx::RulesetHdr*>(blob);
    if (!h->off_eager) return true;
    const auto* pats = reinterpret_cast<const ajx::Pattern*>(blob + h->off_patterns);
    const auto* eg = reinterpret_cast<const ajx::EagerSel*>(blob + h->off_eager);
    for (uint32_t p = first; p < first + count; p++) {
        const uint32_t f = eg[pats[p].selector].pad[0];
        if ((f & ajx::kEagerAll) && !(f & ajx::kEagerKeep)) return false;
    }
    return true;
}

// a host-buffer batch: every span in the arena, every ruleset index below n_sets
bool host_batch_ok(const uint64_t* offs, const uint32_t* lens, const uint32_t* set_of_req, uint32_t n,
                   uint64_t arena_len, uint32_t n_sets) {
    for (uint32_t r = 0; set_of_req && r < n; r++)
        if (set_of_req[r] >= n_sets) return false;
    return ajx::spans_in_arena(offs, lens, n, arena_len);
}

// the inputs of a host-buffer batch in the context's staging buffer (the arena at 0)
struct StagedIn {
    size_t offs, lens, sor;
};
StagedIn lay_inputs(ajx::StageLayout& lay, uint64_t arena_len, uint32_t n, bool with_sor) {
    lay.add(arena_len);
    const size_t offs = lay.add((size_t)n * 8), lens = lay.add((size_t)n * 4);
    return {offs, lens, lay.add(with_sor ? (size_t)n * 4 : 0)};
}

// ctx->batch_mu held: the staging buffer grown to `total` bytes (once ctx->stream is done
// with the old one) and the inputs' uploads queued on ctx->stream
int upload_inputs(authjx_ctx* ctx, size_t total, const StagedIn& o, const uint8_t* arena, uint64_t arena_len,
                  const uint64_t* offs, const uint32_t* lens, const uint32_t* set_of_req, uint32_t n) {
    HIP_OK(hipSetDevice(ctx->device));
    HIP_OK(ctx->stage.reserve(total, ctx->stream));
    uint8_t* b = ctx->stage.data();
    hipStream_t s = ctx->stream;
    HIP_OK(hipMemcpyAsync(b, arena, arena_len, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(b + o.offs, offs, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(b + o.lens, lens, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (set_of_req) HIP_OK(hipMemcpyAsync(b + o.sor, set_of_req, (size_t)n * 4, hipMemcpyHostToDevice, s));
    return AUTHJX_OK;
}

// the compile's second half: the facts plan_in reads, the blob into device memory
int finish_compile(authjx_ctx* ctx, authjx_ruleset* rs, int rc, const std::string& err, authjx_ruleset** out,
                   int32_t* pattern_status, char* errbuf, size_t errcap) {
    if (errbuf && errcap) std::snprintf(errbuf, errcap, "%s", err.c_str());
    if (rc != AUTHJX_OK) {
        delete rs;
        return rc;
    }
    if (pattern_status)
        for (uint32_t i = 0; i < rs->c.n_patterns; i++) pattern_status[i] = rs->c.pattern_status[i];
    const std::vector<uint8_t>& blob = rs->c.blob;
    const auto* h = reinterpret_cast<const ajx::RulesetHdr*>(blob.data());
    rs->device = ctx->device;
    rs->blob_bytes = (uint32_t)blob.size();
    rs->stream_ok = ajx::stream_eligible(blob.data(), rs->blob_bytes);
    rs->stream_rec = ajx::stream_records(blob.data());
    rs->mods = h->n_modifiers != 0 || (h->flags & ajx::kFlagBufs) != 0;
    rs->lean_feat = h->lean_feat;
    rs->hdr_trees = h->pad1[0];
    if (hipSetDevice(ctx->device) != hipSuccess || rs->d_blob.reserve(blob.size()) != hipSuccess ||
        hipMemcpy(rs->d_blob.data(), blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        delete rs;
        return AUTHJX_EDEVICE;
    }
    *out = rs;
    return AUTHJX_OK;
}

}  // namespace

void retire_stream(authjx_ctx* ctx, hipStream_t s) {
    Workspace* w = nullptr;
    bool dead = false;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        for (size_t i = 0; i < ctx->ws.size(); i++)
            if (ctx->ws[i]->stream == s) {
                w = ctx->ws[i];
                ctx->ws.erase(ctx->ws.begin() + (long)i);
                if (ctx->last_ws == w) ctx->last_ws = nullptr;
                w->retired = true;
                dead = w->refs == 0;
                break;
            }
    }
    if (dead) destroy_workspace(w);  // (else the call still on that stream does, when it ends)
}

int with_ptr_table(authjx_ctx* ctx, void* stream, const uint8_t* const* ptrs, uint32_t n,
                   const std::function<hipError_t(const uint8_t* const*, hipStream_t)>& launch) {
    WsLock wl(ctx, stream);
    Workspace* w = wl.w;
    if (!w) return AUTHJX_EDEVICE;
    HIP_OK(hipSetDevice(ctx->device));
    ajx::PtrTable& t = w->progs;
    if (t.last.empty() || !std::equal(t.last.begin(), t.last.end(), ptrs, ptrs + n)) {
        if (n > t.cap) {  // (grows once the stream's earlier batches are done with the old table)
            const uint32_t cap = n < 64 ? 64 : n;
            t.cap = 0;
            t.last.clear();
            t.rec[0] = t.rec[1] = false;
            HIP_OK(t.dev.reserve(2 * (size_t)cap * sizeof(uint8_t*), w->stream));
            HIP_OK(t.host.reserve(2 * (size_t)cap * sizeof(uint8_t*), w->stream));
            for (int k = 0; k < 2; k++)
                if (!t.ev[k]) HIP_OK(hipEventCreateWithFlags(&t.ev[k], hipEventDisableTiming));
            t.cap = cap;
        }
        // the other slot: free once the last batch that read it has finished
        const uint32_t k = t.last.empty() ? 0u : 1u - t.slot;
        if (t.rec[k]) HIP_OK(hipEventSynchronize(t.ev[k]));
        const uint8_t** h = t.host.as<const uint8_t*>() + (size_t)k * t.cap;
        std::memcpy(h, ptrs, n * sizeof(uint8_t*));
        HIP_OK(hipMemcpyAsync(t.dev.as<const uint8_t*>() + (size_t)k * t.cap, h, n * sizeof(uint8_t*),
                              hipMemcpyHostToDevice, w->stream));
        t.slot = k;
        t.last.assign(ptrs, ptrs + n);
    }
    HIP_OK(launch(t.dev.as<const uint8_t*>() + (size_t)t.slot * t.cap, w->stream));
    HIP_OK(hipEventRecord(t.ev[t.slot], w->stream));
    t.rec[t.slot] = true;
    HIP_OK(hipEventRecord(w->ev1, w->stream));  // (retiring the stream waits for this batch)
    w->ran = true;
    return AUTHJX_OK;
}

int eval_device(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets, const uint32_t* d_set_of_req,
                const uint8_t* d_arena, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n,
                uint8_t* d_out_tristate, int32_t* d_out_err_idx, uint64_t* d_out_bitmap, uint32_t bitmap_stride_words,
                void* stream, const uint8_t* const* d_sets_pre) {
    if (!ctx || !sets || n_sets == 0 || (n && (!d_arena || !d_offs || !d_lens || !d_out_tristate)))
        return AUTHJX_EINVAL;
    if (n_sets > 1 && !d_set_of_req) return AUTHJX_EINVAL;
    if (n_sets == 1) d_set_of_req = nullptr;  // every request uses sets[0] (uniform-ruleset kernels)
    uint32_t need_words = 0;
    for (uint32_t i = 0; i < n_sets; i++) {
        if (!sets[i] || sets[i]->c.n_trees != sets[0]->c.n_trees) return AUTHJX_EINVAL;
        need_words = std::max(need_words, (sets[i]->c.n_patterns + 63) / 64);
    }
    if (d_out_bitmap && bitmap_stride_words < need_words) return AUTHJX_EINVAL;
    const ajx::PlanIn in = plan_in(ctx, sets, n_sets, n, d_out_bitmap != nullptr);
    const ajx::EvalPlan plan = ajx::plan_eval(in);
    WsLock wl(ctx, stream);
    Workspace* w = wl.w;
    if (!w) return AUTHJX_EDEVICE;
    hipStream_t s = w->stream;
    HIP_OK(hipSetDevice(ctx->device));
    int rc = ensure_sets(w, ctx->device, sets, n_sets, d_sets_pre);
    if (rc != AUTHJX_OK) return rc;
    if (plan.path != ajx::kPathExact && (rc = ensure_work(w, n, plan.rows_stride)) != AUTHJX_OK) return rc;
    HIP_OK(hipEventRecord(w->ev0, s));
    // capture rows kept for authjx_select_from_eval_device
    w->rows_rs = plan.keep_rows ? sets[0] : nullptr;
    w->rows_n = n;
    w->rows_stride = plan.rows_stride;
    w->rows_perm = nullptr;
    w->rows_wave = true;
    // (the counters are zero only after a FIN launch: every other launch fills them itself)
    bool cnt_zero = w->cnt_zero;
    w->cnt_zero = w->exact_published = false;
    uint32_t* const slow = w->slow.as<uint32_t>();
    const ajx::Batch batch{w->d_sets, d_set_of_req, d_arena, d_offs, d_lens, n};
    const ajx::Results res{d_out_tristate, d_out_err_idx, d_out_bitmap, bitmap_stride_words};
    if (plan.path == ajx::kPathExact) {
        HIP_OK(ajx::launch_eval_scan(batch, res, plan.mods != 0, s));
    } else if (plan.path == ajx::kPathStream) {
        // the streaming kernel (ajx_stream.h), its stage B over the order buffer as the
        // stage-B list; the slow ids after its counters
        const ajx::Work work{w->rows.as<uint64_t>(), plan.rows_stride, slow, ajx::stream_slow_ids(slow)};
        HIP_OK(ajx::launch_eval_stream(batch, res, work, plan, in.max_blob, in.max_rec,
                                       ajx::PermBuf{w->perm.as<uint32_t>(), n}.stage_list(), &cnt_zero, s));
        w->cnt_zero = w->exact_published = cnt_zero;
    } else {
        const uint32_t* perm = nullptr;
        uint32_t* pos_of = nullptr;
        const ajx::PermBuf order{w->perm.as<uint32_t>(), n};
        if (plan.len_order) {
            if (plan.want_pos_of) {
                HIP_OK(w->tout.reserve(ajx::tout_bytes(n, plan.n_out, plan.tout_bm ? bitmap_stride_words : 0u), s));
                pos_of = order.pos_of();
            }
            HIP_OK(ajx::launch_len_order(d_lens, n, order.hist(), order.perm(), pos_of, s));
            perm = order.perm();
        }
        w->rows_perm = perm;
        const ajx::Work work{w->rows.as<uint64_t>(), plan.rows_stride, slow, slow + 1};
        HIP_OK(ajx::launch_eval_fast(batch, res, work, plan, perm, pos_of, pos_of ? w->tout.data() : nullptr, s));
    }
    return batch_done(w, sets, n_sets);
}

extern "C" {

#ifndef AJX_SRC_HASH
#define AJX_SRC_HASH "unknown"
#endif
const char* authjx_build_hash(void) { return AJX_SRC_HASH; }

int authjx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int authjx_init(int device, authjx_ctx** out) {
    if (!out) return AUTHJX_EINVAL;
    *out = nullptr;
    int n = authjx_device_count();
    if (device < 0 || device >= n) return AUTHJX_EDEVICE;
    HIP_OK(hipSetDevice(device));
    authjx_ctx* c = new authjx_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return AUTHJX_EDEVICE;
    }
    *out = c;
    return AUTHJX_OK;
}

void authjx_shutdown(authjx_ctx* ctx) {
    if (!ctx) return;
    // batchers still alive: closed (their queued requests evaluated, workers joined) before
    // the workspaces they use go away
    std::vector<authjx_batcher*> live;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        live = ctx->batchers;
    }
    for (authjx_batcher* b : live) authjx_batcher_destroy(b);
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (Workspace* w : ctx->ws) destroy_workspace(w);  // (no call may run during shutdown)
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int authjx_release_stream(authjx_ctx* ctx, void* stream) {
    if (!ctx || !stream || (hipStream_t)stream == ctx->stream) return AUTHJX_EINVAL;
    (void)hipSetDevice(ctx->device);
    retire_stream(ctx, (hipStream_t)stream);
    return AUTHJX_OK;
}

int authjx_compile(authjx_ctx* ctx, const authjx_tree* tree, authjx_ruleset** out, int32_t* pattern_status,
                   char* errbuf, size_t errcap) {
    if (!ctx || !tree || !out) return AUTHJX_EINVAL;
    *out = nullptr;
    authjx_ruleset* rs = new authjx_ruleset();
    std::string err;
    int rc = ajx::compile_tree(tree, &rs->c, &err);
    return finish_compile(ctx, rs, rc, err, out, pattern_status, errbuf, errcap);
}

int authjx_compile_forest(authjx_ctx* ctx, const authjx_tree* trees, uint32_t n_trees, authjx_ruleset** out,
                          int32_t* pattern_status, char* errbuf, size_t errcap) {
    if (!ctx || !trees || !n_trees || !out) return AUTHJX_EINVAL;
    *out = nullptr;
    authjx_ruleset* rs = new authjx_ruleset();
    std::string err;
    int rc = ajx::compile_forest(trees, n_trees, &rs->c, &err);
    return finish_compile(ctx, rs, rc, err, out, pattern_status, errbuf, errcap);
}

uint32_t authjx_ruleset_trees(const authjx_ruleset* rs) { return rs ? rs->c.n_trees : 0; }

void authjx_free(authjx_ruleset* rs) {
    if (!rs) return;
    if (rs->d_blob.data()) {
        (void)hipSetDevice(rs->device);
        // wait for the last batch of every stream that used this ruleset (not the device:
        // other streams' batches and other work go on); the events are collected under the
        // registry lock and waited on outside it
        std::vector<std::shared_ptr<EndEvent>> evs;
        {
            std::lock_guard<std::mutex> lock(rs->mu);
            std::lock_guard<std::mutex> reg(g_reg_mu);
            for (uint64_t id : rs->users)
                for (const auto& e : g_reg)
                    if (e.first == id) evs.push_back(e.second);
        }
        for (const auto& e : evs) (void)hipEventSynchronize(e->ev);
    }
    delete rs;  // (the blob goes here, after the waits)
}

uint32_t authjx_ruleset_patterns(const authjx_ruleset* rs) { return rs ? rs->c.n_patterns : 0; }
uint32_t authjx_ruleset_selectors(const authjx_ruleset* rs) { return rs ? rs->c.n_selectors : 0; }

size_t authjx_pattern_error(const authjx_ruleset* rs, uint32_t i, char* buf, size_t cap) {
    if (!rs || i >= rs->c.n_patterns) return 0;
    const std::string& e = rs->c.pattern_error[i];
    if (buf && cap) std::snprintf(buf, cap, "%s", e.c_str());
    return e.size();
}

int authjx_eval_batch_device(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                             const uint32_t* d_set_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                             const uint32_t* d_lens, uint32_t n, uint8_t* d_out_tristate, int32_t* d_out_err_idx,
                             uint64_t* d_out_bitmap, uint32_t bitmap_stride_words, void* stream) {
    return eval_device(ctx, sets, n_sets, d_set_of_req, d_arena, d_offs, d_lens, n, d_out_tristate, d_out_err_idx,
                       d_out_bitmap, bitmap_stride_words, stream, nullptr);
}

static_assert(sizeof(authjx_value) == 12, "authjx_value is three u32 words on the device");

int authjx_select_batch_device(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                               const uint32_t* d_set_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                               const uint32_t* d_lens, uint32_t n, authjx_value* d_out_values,
                               uint32_t values_stride, void* stream) {
    return authjx_select_text_batch_device(ctx, sets, n_sets, d_set_of_req, d_arena, d_offs, d_lens, n, d_out_values,
                                           values_stride, nullptr, 0, stream);
}

int authjx_select_text_batch_device(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                                    const uint32_t* d_set_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                                    const uint32_t* d_lens, uint32_t n, authjx_value* d_out_values,
                                    uint32_t values_stride, uint8_t* d_out_text, uint32_t text_stride, void* stream) {
    if (!ctx || !sets || n_sets == 0 || (n && (!d_arena || !d_offs || !d_lens || !d_out_values)))
        return AUTHJX_EINVAL;
    if (d_out_text && text_stride == 0) return AUTHJX_EINVAL;
    if (n_sets > 1 && !d_set_of_req) return AUTHJX_EINVAL;
    if (n_sets == 1) d_set_of_req = nullptr;
    for (uint32_t i = 0; i < n_sets; i++)
        if (!sets[i] || sets[i]->c.n_patterns > values_stride) return AUTHJX_EINVAL;
    const ajx::PlanIn in = plan_in(ctx, sets, n_sets, n, false);  // (the settings, the largest selector count)
    const uint32_t row_stride = 1 + in.max_sel;
    WsLock wl(ctx, stream);
    Workspace* w = wl.w;
    if (!w) return AUTHJX_EDEVICE;
    hipStream_t s = w->stream;
    HIP_OK(hipSetDevice(ctx->device));
    int rc = ensure_sets(w, ctx->device, sets, n_sets);
    if (rc != AUTHJX_OK) return rc;
    const bool exact = in.force_scan != 0;  // the exact Get per selector (cross-check)
    w->rows_rs = nullptr;  // (the rows are rewritten for this ruleset)
    w->cnt_zero = w->exact_published = false;  // (its slow count is filled and left nonzero)
    if (!exact && (rc = ensure_work(w, n, row_stride)) != AUTHJX_OK) return rc;
    const uint32_t* perm = nullptr;
    if (!exact && in.len_sort && n_sets == 1 && n >= 4096) {
        const ajx::PermBuf order{w->perm.as<uint32_t>(), n};
        HIP_OK(ajx::launch_len_order(d_lens, n, order.hist(), order.perm(), nullptr, s));
        perm = order.perm();
    }
    const uint32_t shared_bytes =
        (n_sets == 1 && sets[0]->blob_bytes <= ajx::kMaxSharedBlobBytes) ? sets[0]->blob_bytes : 0u;
    uint32_t* const slow = w->slow.as<uint32_t>();
    const ajx::Batch batch{w->d_sets, d_set_of_req, d_arena, d_offs, d_lens, n};
    const ajx::Values values{reinterpret_cast<uint32_t*>(d_out_values), values_stride, d_out_text, text_stride};
    const ajx::Work work{exact ? nullptr : w->rows.as<uint64_t>(), row_stride, slow, slow + 1};
    HIP_OK(ajx::launch_select(batch, shared_bytes, values, work, perm, s));
    return batch_done(w, sets, n_sets);
}

int authjx_select_from_eval_device(authjx_ctx* ctx, const authjx_ruleset* rs, uint32_t first_pattern,
                                   const uint8_t* d_arena, const uint64_t* d_offs, const uint32_t* d_lens,
                                   uint32_t n, authjx_value* d_out_values, uint32_t values_stride, void* stream) {
    if (!ctx || !rs || values_stride == 0 || (n && (!d_arena || !d_offs || !d_lens || !d_out_values)))
        return AUTHJX_EINVAL;
    if (first_pattern + values_stride > rs->c.n_patterns) return AUTHJX_EINVAL;
    WsLock wl(ctx, stream);
    Workspace* w = wl.w;
    if (!w) return AUTHJX_EDEVICE;
    // the rows must be this stream's last evaluation's, of this ruleset, over this many
    // requests, and hold these patterns' records
    if (w->rows_rs != rs || w->rows_n != n || !rows_hold_patterns(rs, first_pattern, values_stride))
        return AUTHJX_EINVAL;
    hipStream_t s = w->stream;
    HIP_OK(hipSetDevice(ctx->device));
    const authjx_ruleset* one[1] = {rs};
    int rc = ensure_sets(w, ctx->device, one, 1);
    if (rc != AUTHJX_OK) return rc;
    const ajx::Batch batch{w->d_sets, nullptr, d_arena, d_offs, d_lens, n};
    const ajx::Values values{reinterpret_cast<uint32_t*>(d_out_values), values_stride, nullptr, 0};
    const ajx::Work work{w->rows.as<uint64_t>(), w->rows_stride, nullptr, nullptr};
    HIP_OK(ajx::launch_select_rows(batch, values, work, first_pattern, w->rows_perm, w->rows_wave, s));
    return batch_done(w, one, 1);
}

int authjx_select_batch(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                        const uint32_t* set_of_req, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* offs, const uint32_t* lens, uint32_t n, authjx_value* out_values,
                        uint32_t values_stride) {
    return authjx_select_text_batch(ctx, sets, n_sets, set_of_req, arena, arena_len, offs, lens, n, out_values,
                                    values_stride, nullptr, 0);
}

int authjx_select_text_batch(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                             const uint32_t* set_of_req, const uint8_t* arena, uint64_t arena_len,
                             const uint64_t* offs, const uint32_t* lens, uint32_t n, authjx_value* out_values,
                             uint32_t values_stride, uint8_t* out_text, uint32_t text_stride) {
    if (!ctx || (n && (!arena || !offs || !lens || !out_values))) return AUTHJX_EINVAL;
    if (out_text && text_stride == 0) return AUTHJX_EINVAL;
    if (!host_batch_ok(offs, lens, set_of_req, n, arena_len, n_sets)) return AUTHJX_EINVAL;
    const size_t out_bytes = (size_t)n * values_stride * sizeof(authjx_value);
    const size_t text_bytes = out_text ? (size_t)n * text_stride : 0;
    ajx::StageLayout lay;
    const StagedIn in = lay_inputs(lay, arena_len, n, set_of_req != nullptr);
    const size_t o_out = lay.add(out_bytes), o_text = lay.add(text_bytes);
    std::lock_guard<std::mutex> batch_lock(ctx->batch_mu);
    int rc = upload_inputs(ctx, lay.total(), in, arena, arena_len, offs, lens, set_of_req, n);
    if (rc != AUTHJX_OK) return rc;
    uint8_t* b = ctx->stage.data();
    rc = authjx_select_text_batch_device(ctx, sets, n_sets, set_of_req ? (const uint32_t*)(b + in.sor) : nullptr, b,
                                         (const uint64_t*)(b + in.offs), (const uint32_t*)(b + in.lens), n,
                                         (authjx_value*)(b + o_out), values_stride, out_text ? b + o_text : nullptr,
                                         text_stride, nullptr);
    if (rc != AUTHJX_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // (the uploads still read the caller's buffers)
        return rc;
    }
    HIP_OK(hipMemcpyAsync(out_values, b + o_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_text) HIP_OK(hipMemcpyAsync(out_text, b + o_text, text_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    return AUTHJX_OK;
}

// Profiling only (not in authjx.h): the kernel mode (ajx::KernelMode, ajx_plan.h) of the
// context's evaluations; some modes replace stage A by a reduced variant whose outputs are
// meaningless, to price its parts on the hardware. AUTHJX_EINVAL for a number that names
// no mode (the retired 1..3 and 10..12 among them); the mode then stays as it was.
int authjx_debug_ablate(authjx_ctx* ctx, int mode) {
    if (!ctx || !ajx::mode_known(mode)) return AUTHJX_EINVAL;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->mode = mode;
    return AUTHJX_OK;
}


// Profiling only (not in authjx.h): batches of up to n requests take the streaming kernel
// (default 4096; 0: never)
int authjx_debug_stream_max(authjx_ctx* ctx, uint32_t n) {
    if (!ctx) return AUTHJX_EINVAL;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->stream_max_n = n;
    return AUTHJX_OK;
}

// Diagnostics (not in authjx.h): the HIP error behind this thread's last AUTHJX_EDEVICE and
// the source line that saw it ("" when none)
const char* authjx_debug_last_error(void) {
    static thread_local char buf[160];
    const AjxLastError& e = ajx_last_error;
    if (e.err == hipSuccess) return "";
    const char* slash = std::strrchr(e.file, '/');
    std::snprintf(buf, sizeof buf, "%s (%s:%d)", hipGetErrorString(e.err), slash ? slash + 1 : e.file, e.line);
    return buf;
}

// Profiling only (not in authjx.h): the length-bucketed request order off (0), for
// single-ruleset batches (1, default) or for every batch (2).
int authjx_debug_len_sort(authjx_ctx* ctx, int on) {
    if (!ctx) return AUTHJX_EINVAL;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->len_sort = on;  // 0 off, 1 single-ruleset batches, 2 also multi-tenant batches
    return AUTHJX_OK;
}

// Profiling only (not in authjx.h): workgroup-uniform LDS staging of multi-tenant
// rulesets on (1, default) or off (0: every table read from global memory).
int authjx_debug_tenant_stage(authjx_ctx* ctx, int on) {
    if (!ctx) return AUTHJX_EINVAL;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->no_tenant_stage = on ? 0 : 1;
    return AUTHJX_OK;
}

// profiling: a compiled ruleset's device blob size in bytes (what the kernels stage in LDS)
uint32_t authjx_debug_blob_bytes(const authjx_ruleset* rs) { return rs ? (uint32_t)rs->c.blob.size() : 0u; }

int authjx_set_exact_scan(authjx_ctx* ctx, int force) {
    if (!ctx) return AUTHJX_EINVAL;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->force_scan = force ? 1 : 0;
    return AUTHJX_OK;
}

int64_t authjx_last_exact_count(authjx_ctx* ctx) {
    if (!ctx) return AUTHJX_EINVAL;
    LastWs ref(ctx);
    Workspace* w = ref.w;
    if (ref.force_scan || !w) return -1;
    std::lock_guard<std::mutex> lock(w->mu);
    uint32_t* const slow = w->slow.as<uint32_t>();
    if (!slow || !w->ran) return -1;
    uint32_t c = 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipEventSynchronize(w->ev1) != hipSuccess ||
        hipMemcpy(&c, w->exact_published ? &ajx::stream_counters(slow)->exact_published : slow, sizeof c,
                  hipMemcpyDeviceToHost) != hipSuccess)
        return AUTHJX_EDEVICE;
    return (int64_t)c;
}

float authjx_last_kernel_ms(authjx_ctx* ctx) {
    if (!ctx) return 0.f;
    LastWs ref(ctx);
    Workspace* w = ref.w;
    if (!w) return 0.f;
    std::lock_guard<std::mutex> lock(w->mu);
    float ms = 0.f;
    if (!w->ran || hipEventSynchronize(w->ev1) != hipSuccess) return 0.f;
    if (hipEventElapsedTime(&ms, w->ev0, w->ev1) != hipSuccess) return 0.f;
    return ms;
}

int authjx_eval_batch(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets,
                      const uint32_t* set_of_req, const uint8_t* arena, uint64_t arena_len, const uint64_t* offs,
                      const uint32_t* lens, uint32_t n, uint8_t* out_tristate, int32_t* out_err_idx,
                      uint64_t* out_bitmap, uint32_t bitmap_stride_words) {
    if (!ctx || (n && (!arena || !offs || !lens || !out_tristate))) return AUTHJX_EINVAL;
    if (!host_batch_ok(offs, lens, set_of_req, n, arena_len, n_sets)) return AUTHJX_EINVAL;
    if (!sets || n_sets == 0 || !sets[0]) return AUTHJX_EINVAL;
    const size_t nt = sets[0]->c.n_trees;  // results per request
    const size_t bm_bytes = out_bitmap ? (size_t)n * bitmap_stride_words * 8 : 0;
    ajx::StageLayout lay;
    const StagedIn in = lay_inputs(lay, arena_len, n, set_of_req != nullptr);
    const size_t o_tri = lay.add((size_t)n * nt), o_err = lay.add((size_t)n * nt * 4), o_bm = lay.add(bm_bytes);
    std::lock_guard<std::mutex> batch_lock(ctx->batch_mu);
    int rc = upload_inputs(ctx, lay.total(), in, arena, arena_len, offs, lens, set_of_req, n);
    if (rc != AUTHJX_OK) return rc;
    uint8_t* b = ctx->stage.data();
    hipStream_t s = ctx->stream;
    rc = authjx_eval_batch_device(ctx, sets, n_sets, set_of_req ? (const uint32_t*)(b + in.sor) : nullptr, b,
                                  (const uint64_t*)(b + in.offs), (const uint32_t*)(b + in.lens), n, b + o_tri,
                                  out_err_idx ? (int32_t*)(b + o_err) : nullptr,
                                  out_bitmap ? (uint64_t*)(b + o_bm) : nullptr, bitmap_stride_words, nullptr);
    if (rc != AUTHJX_OK) {
        (void)hipStreamSynchronize(s);  // (the uploads still read the caller's buffers)
        return rc;
    }
    HIP_OK(hipMemcpyAsync(out_tristate, b + o_tri, (size_t)n * nt, hipMemcpyDeviceToHost, s));
    if (out_err_idx) HIP_OK(hipMemcpyAsync(out_err_idx, b + o_err, (size_t)n * nt * 4, hipMemcpyDeviceToHost, s));
    if (out_bitmap) HIP_OK(hipMemcpyAsync(out_bitmap, b + o_bm, bm_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return AUTHJX_OK;
}

}  // extern "C"
