// ajx_batcher_api.cpp — the micro-batcher's entry points of the C-ABI (include/authjx.h):
// ajx_batcher.h's queue with the device evaluation (eval_device, ajx_api.cpp) plugged in,
// and behind it, for the batch's phase requests (ajx_phase.h), the select and the render of
// their AuthConfigs' response outputs on the same stream.
#include <atomic>
#include <cstring>
#include <thread>

#include "ajx_host.h"
#include "ajx_batcher.h"
#include "ajx_phase.h"
#include "ajx_phase_api.h"

namespace {

constexpr uint32_t kBatcherMaxWorkers = 8;
// workers per batcher: 2 by default (one packs and launches while the other's batch runs);
// authjx_debug_batcher_workers changes it for batchers created afterwards
std::atomic<uint32_t> g_batcher_workers{2};
// profiling knobs (authjx_debug_batcher_modes), read when a batcher is created: how callers
// are woken (0: one condition variable each, 1: one broadcast per batch, 2: one futex word
// each, 3: as 2, in a binary tree where each woken caller wakes two more), how a worker waits
// for its batch (0: hipStreamSynchronize, 1: polling hipStreamQuery), where the kernel reads
// the batch (0: one copy into device memory, 1: the pinned staging buffer itself)
// (zero-copy is the default: measured p50 3-15 µs lower at 64 producers, the same or more
// decisions/s at 256)
std::atomic<uint32_t> g_batcher_wake{0}, g_batcher_sync{0}, g_batcher_zcopy{1};

}  // namespace

struct authjx_batcher {
    authjx_ctx* ctx = nullptr;
    // per worker: its own stream (its own workspace in ctx) and staging buffers, grown
    // without a synchronize (the worker has waited for its last batch)
    struct Lane {
        hipStream_t stream = nullptr;
        // arena | offs | lens | set_of_req | sets | the phase subset's offs, lens, program
        // indices, program table and per-group ruleset indices | outputs (written by the
        // kernels): tri, err, the phase requests' records and output slots
        ajx::PinnedBuf pinned;
        ajx::DeviceBuf dev;     // the inputs' copy with zero-copy off
        ajx::DeviceBuf mid;     // the phase subset's values and text slots (select -> render)
    } lanes[kBatcherMaxWorkers];
    uint32_t n_lanes = 2;
    uint32_t sync_mode = 0, zcopy = 0;
    ajx::BatchCore* core = nullptr;
    // profiling sums (ns): packing the staging buffer, launch calls, the wait for the device
    std::atomic<uint64_t> pack_ns{0}, launch_ns{0}, sync_ns{0};

    // one batch (ordered by ruleset): pack, one launch (worker `wid` only). The pinned
    // staging buffer carries the documents, offsets, lengths, each request's ruleset index
    // and the rulesets' blob pointers; the kernel reads them from it (mapped host memory;
    // with zero-copy off, one copy into device memory first) and writes the results into
    // it, so a small batch is one kernel (its counters left zero by the last one on this
    // stream) and a synchronize.
    int evaluate(std::vector<ajx::BatchReq*>& reqs, uint32_t wid) {
        Lane& L = lanes[wid];
        const uint32_t n = (uint32_t)reqs.size(), nt = reqs[0]->n_out;
        std::vector<const authjx_ruleset*> sets;
        std::vector<uint32_t> sor(n);
        size_t arena_len = 0;
        for (uint32_t i = 0; i < n; i++) {
            const authjx_ruleset* rs = (const authjx_ruleset*)reqs[i]->rs;
            if (sets.empty() || sets.back() != rs) sets.push_back(rs);
            sor[i] = (uint32_t)sets.size() - 1;
            arena_len += reqs[i]->len;
        }
        ajx::StageLayout lay;
        lay.add(arena_len + 1);  // (the documents, at 0, and a terminating NUL)
        const size_t o_offs = lay.add((size_t)n * 8), o_lens = lay.add((size_t)n * 4);
        const size_t o_sor = lay.add((size_t)n * 4), o_sets = lay.add(sets.size() * sizeof(uint8_t*));
        // the phase requests: further inputs (nothing for a batch without any), outputs,
        // and the values and text slots between the select and the render in device memory
        const ajx::PhasePlan plan = ajx::plan_phases(reqs);
        const uint32_t m = plan.n(), vs = plan.values_stride, rs = plan.records_stride;
        const size_t o_poffs = lay.add((size_t)m * 8), o_plens = lay.add((size_t)m * 4);
        // (a batch with a gated phase request: the gates' blobs behind the programs' in the
        // table, each subset position's tri-state row, and a verdict per position)
        const bool gated = plan.render_gated != nullptr;
        const size_t np = plan.progs.size();
        const size_t o_por = lay.add((size_t)m * 4), o_ptab = lay.add((gated ? 2 : 1) * np * sizeof(uint8_t*));
        const size_t o_psor = lay.add((size_t)m * 4), o_ptor = lay.add(gated ? (size_t)m * 4 : 0);
        const size_t in_bytes = lay.total();  // (the outputs after it: host side only)
        const size_t o_tri = lay.add((size_t)n * nt), o_err = lay.add((size_t)n * nt * 4);
        const size_t o_rec = lay.add((size_t)m * rs * 12), o_ver = lay.add(gated ? (size_t)m * 8 : 0);
        ajx::StageLayout mid;
        const size_t o_val = mid.add((size_t)m * vs * 12);
        std::vector<size_t> o_text(plan.groups.size()), o_out(plan.groups.size());
        for (size_t g = 0; g < plan.groups.size(); g++) {
            o_text[g] = mid.add((size_t)plan.groups[g].count * plan.groups[g].text_stride);
            o_out[g] = lay.add((size_t)plan.groups[g].count * plan.groups[g].out_stride);
        }
        HIP_OK(hipSetDevice(ctx->device));
        HIP_OK(L.pinned.reserve(lay.total()));
        HIP_OK(L.dev.reserve(in_bytes));
        HIP_OK(L.mid.reserve(mid.total()));
        uint8_t* const h = L.pinned.data();
        const uint64_t t0 = ajx::mono_ns();
        uint64_t* offs = (uint64_t*)(h + o_offs);
        uint32_t* lens = (uint32_t*)(h + o_lens);
        size_t at = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (reqs[i]->len) std::memcpy(h + at, reqs[i]->doc, reqs[i]->len);
            offs[i] = at;
            lens[i] = (uint32_t)reqs[i]->len;
            at += reqs[i]->len;
        }
        h[at] = 0;
        std::memcpy(h + o_sor, sor.data(), (size_t)n * 4);
        const uint8_t** hs = (const uint8_t**)(h + o_sets);
        for (size_t k = 0; k < sets.size(); k++) hs[k] = sets[k] ? sets[k]->d_blob.data() : nullptr;
        if (m) {  // (the phase subset reads the same staged documents)
            uint64_t* poffs = (uint64_t*)(h + o_poffs);
            uint32_t* plens = (uint32_t*)(h + o_plens);
            for (uint32_t j = 0; j < m; j++) {
                poffs[j] = offs[plan.req[j]];
                plens[j] = lens[plan.req[j]];
            }
            std::memcpy(h + o_por, plan.prog_of.data(), (size_t)m * 4);
            const uint8_t** pt = (const uint8_t**)(h + o_ptab);
            for (size_t k = 0; k < np; k++) pt[k] = (const uint8_t*)plan.progs[k];
            if (gated) {
                for (size_t k = 0; k < np; k++) pt[np + k] = (const uint8_t*)plan.gates[k];
                std::memcpy(h + o_ptor, plan.tri_row.data(), (size_t)m * 4);
            }
            for (const ajx::PhaseGroup& g : plan.groups)
                std::memcpy(h + o_psor + (size_t)g.first * 4, g.set_of.data(), (size_t)g.count * 4);
        }
        const uint64_t t1 = ajx::mono_ns();
        // (zero-copy: the kernel reads the batch from the mapped staging buffer over PCIe)
        const uint8_t* in = zcopy ? L.pinned.device() : L.dev.data();
        if (!zcopy) HIP_OK(hipMemcpyAsync(L.dev.data(), h, in_bytes, hipMemcpyHostToDevice, L.stream));
        const int rc = eval_device(ctx, sets.data(), (uint32_t)sets.size(), (const uint32_t*)(in + o_sor), in,
                                   (const uint64_t*)(in + o_offs), (const uint32_t*)(in + o_lens), n,
                                   L.pinned.device() + o_tri, (int32_t*)(L.pinned.device() + o_err), nullptr, 0,
                                   L.stream, (const uint8_t* const*)(in + o_sets));
        if (rc != AUTHJX_OK) return rc;
        // the phase requests' values (the multi-set select over their selector rulesets as
        // runs) and outputs (the multi-program render), one pair of launches per group
        uint8_t* const out_dev = L.pinned.device();
        for (size_t gi = 0; gi < plan.groups.size(); gi++) {
            const ajx::PhaseGroup& g = plan.groups[gi];
            const uint64_t* d_offs = (const uint64_t*)(in + o_poffs) + g.first;
            const uint32_t* d_lens = (const uint32_t*)(in + o_plens) + g.first;
            authjx_value* d_val = (authjx_value*)(L.mid.data() + o_val) + (size_t)g.first * vs;
            uint8_t* d_text = g.text_stride ? L.mid.data() + o_text[gi] : nullptr;
            const int rc2 = authjx_select_text_batch_device(
                ctx, (const authjx_ruleset* const*)g.sets.data(), (uint32_t)g.sets.size(),
                (const uint32_t*)(in + o_psor) + g.first, in, d_offs, d_lens, g.count, d_val, vs, d_text,
                g.text_stride, L.stream);
            if (rc2 != AUTHJX_OK) {
                (void)hipStreamSynchronize(L.stream);  // (the evaluation queued above reads the lane's buffers)
                return rc2;
            }
            // the tri-states are read where the evaluation above left them (the lane's mapped
            // output part), before anything is copied back: one gated launch for the group
            if (gated) {
                HIP_OK((hipError_t)plan.render_gated(
                    (const uint8_t* const*)(in + o_ptab), (uint32_t)np, (const uint32_t*)(in + o_por) + g.first, in,
                    d_offs, d_lens, g.count, (const uint32_t*)d_val, vs, d_text, g.text_stride, out_dev + o_out[gi],
                    g.out_stride, (uint32_t*)(out_dev + o_rec) + (size_t)g.first * rs * 3, rs, out_dev + o_tri, nt,
                    (const uint32_t*)(in + o_ptor) + g.first, (uint32_t*)(out_dev + o_ver) + (size_t)g.first * 2,
                    L.stream));
                continue;
            }
            const ajx::PhaseRender render = reqs[plan.req[g.first]]->phase->render;
            HIP_OK((hipError_t)render((const uint8_t* const*)(in + o_ptab), (uint32_t)plan.progs.size(),
                                      (const uint32_t*)(in + o_por) + g.first, in, d_offs, d_lens, g.count,
                                      (const uint32_t*)d_val, vs, d_text, g.text_stride, out_dev + o_out[gi],
                                      g.out_stride, (uint32_t*)(out_dev + o_rec) + (size_t)g.first * rs * 3, rs,
                                      L.stream));
        }
        const uint64_t t2 = ajx::mono_ns();
        if (sync_mode == 1) {
            for (;;) {
                const hipError_t q = hipStreamQuery(L.stream);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) HIP_OK(q);
            }
        } else {
            HIP_OK(hipStreamSynchronize(L.stream));
        }
        const uint64_t t3 = ajx::mono_ns();
        pack_ns.fetch_add(t1 - t0, std::memory_order_relaxed);
        launch_ns.fetch_add(t2 - t1, std::memory_order_relaxed);
        sync_ns.fetch_add(t3 - t2, std::memory_order_relaxed);
        const uint8_t* tri = h + o_tri;
        const int32_t* err = (const int32_t*)(h + o_err);
        for (uint32_t i = 0; i < n; i++) {
            for (uint32_t k = 0; k < nt; k++) {
                reqs[i]->out_tri[k] = tri[(size_t)i * nt + k];
                if (reqs[i]->out_err) reqs[i]->out_err[k] = err[(size_t)i * nt + k];
            }
        }
        for (size_t gi = 0; gi < plan.groups.size(); gi++) {
            const ajx::PhaseGroup& g = plan.groups[gi];
            for (uint32_t j = 0; j < g.count; j++) {
                ajx::deliver_phase(*reqs[plan.req[g.first + j]], h + o_out[gi] + (size_t)j * g.out_stride,
                                   (const uint32_t*)(h + o_rec) + (size_t)(g.first + j) * rs * 3);
                if (gated)
                    ajx::deliver_verdict(*reqs[plan.req[g.first + j]],
                                         (const uint32_t*)(h + o_ver) + (size_t)(g.first + j) * 2);
            }
        }
        return AUTHJX_OK;
    }
};

extern "C" {

int authjx_batcher_create(authjx_ctx* ctx, uint32_t max_batch, uint32_t window_us, uint32_t queue_cap,
                          authjx_batcher** out) {
    if (!ctx || !out || max_batch == 0) return AUTHJX_EINVAL;
    *out = nullptr;
    HIP_OK(hipSetDevice(ctx->device));
    authjx_batcher* b = new authjx_batcher();
    b->ctx = ctx;
    b->n_lanes = std::min<uint32_t>(std::max<uint32_t>(g_batcher_workers.load(), 1u), kBatcherMaxWorkers);
    b->sync_mode = g_batcher_sync.load();
    b->zcopy = g_batcher_zcopy.load();
    for (uint32_t k = 0; k < b->n_lanes; k++)
        if (hipStreamCreateWithFlags(&b->lanes[k].stream, hipStreamNonBlocking) != hipSuccess) {
            for (auto& M : b->lanes)
                if (M.stream) (void)hipStreamDestroy(M.stream);
            delete b;
            return AUTHJX_EDEVICE;
        }
    b->core = new ajx::BatchCore(
        max_batch, (uint64_t)window_us * 1000ull, queue_cap ? queue_cap : 4 * max_batch,
        [b](std::vector<ajx::BatchReq*>& reqs, uint32_t wid) { return b->evaluate(reqs, wid); }, b->n_lanes,
        g_batcher_wake.load());
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        ctx->batchers.push_back(b);
    }
    *out = b;
    return AUTHJX_OK;
}

// Profiling only (not in authjx.h): worker threads (each with its own stream) of the
// batchers created after this call (1..8; default 2). n = 0 returns the current count.
int authjx_debug_batcher_workers(uint32_t n) {
    if (n == 0) return (int)g_batcher_workers.load();
    if (n > kBatcherMaxWorkers) return AUTHJX_EINVAL;
    g_batcher_workers.store(n);
    return AUTHJX_OK;
}

// Profiling only (not in authjx.h): the knobs of g_batcher_wake (0..3) / _sync / _zcopy
// (0 or 1) for the batchers created after this call.
int authjx_debug_batcher_modes(uint32_t wake, uint32_t sync, uint32_t zcopy) {
    if (wake > 3 || sync > 1 || zcopy > 1) return AUTHJX_EINVAL;
    g_batcher_wake.store(wake);
    g_batcher_sync.store(sync);
    g_batcher_zcopy.store(zcopy);
    return AUTHJX_OK;
}

// Profiling only (not in authjx.h): out[0..8] = batches, requests, and the sums in ns of the
// queue wait (per request), evaluation, waking callers, callers' resume (per request),
// packing, launch calls and the device wait (per batch).
int authjx_debug_batcher_profile(authjx_batcher* b, uint64_t* out) {
    if (!b || !out) return AUTHJX_EINVAL;
    const ajx::BatchStats st = b->core->stats();
    const uint64_t v[9] = {st.batches, st.requests, st.wait_ns, st.eval_ns, st.wake_ns, st.resume_ns,
                           b->pack_ns.load(), b->launch_ns.load(), b->sync_ns.load()};
    std::memcpy(out, v, sizeof(v));
    return AUTHJX_OK;
}

void authjx_batcher_destroy(authjx_batcher* b) {
    if (!b) return;
    {
        std::lock_guard<std::mutex> g(b->ctx->mu);
        auto& v = b->ctx->batchers;
        v.erase(std::remove(v.begin(), v.end(), b), v.end());
    }
    delete b->core;  // evaluates what is queued, joins the workers
    (void)hipSetDevice(b->ctx->device);
    for (auto& L : b->lanes) {
        if (!L.stream) continue;
        (void)hipStreamSynchronize(L.stream);
        retire_stream(b->ctx, L.stream);  // (only the joined workers used it)
        (void)hipStreamDestroy(L.stream);
    }
    delete b;  // (the lanes' buffers, idle since the synchronize)
}

int authjx_batcher_eval(authjx_batcher* b, const authjx_ruleset* rs, const uint8_t* doc, size_t len,
                        uint64_t timeout_us, uint8_t* out_tristate, int32_t* out_err_idx) {
    if (!b || !rs || (!doc && len) || !out_tristate || len >= (1ull << 32)) return AUTHJX_EINVAL;
    if (rs->device != b->ctx->device) return AUTHJX_EINVAL;
    ajx::BatchReq r;
    r.rs = rs;
    r.n_out = rs->c.n_trees;
    r.doc = doc;
    r.len = len;
    r.deadline_ns = timeout_us ? ajx::mono_ns() + timeout_us * 1000ull : 0;
    r.out_tri = out_tristate;
    r.out_err = out_err_idx;
    return b->core->submit(r);
}

int authjx_batcher_phase(authjx_batcher* b, const authjx_phase* ph, const uint8_t* doc, size_t len,
                         uint64_t timeout_us, uint8_t* out_tristate, int32_t* out_err_idx, uint8_t* out_text,
                         authjx_rendered* out) {
    if (!b || !ph || (!doc && len) || !out_tristate || len >= (1ull << 32)) return AUTHJX_EINVAL;
    if (!out_text || (ph->f.n_outputs && !out) || ph->device != b->ctx->device || !ph->f.render)
        return AUTHJX_EINVAL;
    ajx::BatchReq r;
    r.rs = ph->rules;
    r.n_out = ph->rules->c.n_trees;
    r.doc = doc;
    r.len = len;
    r.deadline_ns = timeout_us ? ajx::mono_ns() + timeout_us * 1000ull : 0;
    r.out_tri = out_tristate;
    r.out_err = out_err_idx;
    r.phase = &ph->f;
    r.out_text = out_text;
    r.out_rec = out;
    return b->core->submit(r);
}

int authjx_batcher_phase_gated(authjx_batcher* b, const authjx_phase* ph, const uint8_t* doc, size_t len,
                               uint64_t timeout_us, uint8_t* out_tristate, int32_t* out_err_idx, uint8_t* out_text,
                               authjx_rendered* out, authjx_verdict* out_verdict) {
    if (!b || !ph || (!doc && len) || !out_tristate || len >= (1ull << 32)) return AUTHJX_EINVAL;
    if (!out_text || (ph->f.n_outputs && !out) || ph->device != b->ctx->device) return AUTHJX_EINVAL;
    if (!ph->f.gates || !ph->f.render_gated) return AUTHJX_EINVAL;  // (an ungated phase)
    ajx::BatchReq r;
    r.rs = ph->rules;
    r.n_out = ph->rules->c.n_trees;
    r.doc = doc;
    r.len = len;
    r.deadline_ns = timeout_us ? ajx::mono_ns() + timeout_us * 1000ull : 0;
    r.out_tri = out_tristate;
    r.out_err = out_err_idx;
    r.phase = &ph->f;
    r.out_text = out_text;
    r.out_rec = out;
    r.out_verdict = out_verdict;
    return b->core->submit(r);
}

// Profiling only (not in authjx.h): authjx_debug_loadgen for phase requests. Thread t
// submits requests i = t, t + threads, ... as authjx_batcher_phase(phases[por[i]], ...);
// lat_ns[i] = that call's latency, out_tri[i] its first result, out_hash[i] the 64-bit
// FNV-1a of its rendered outputs (each output's status byte, then its bytes when rendered).
int authjx_debug_phase_loadgen(authjx_batcher* b, const authjx_phase* const* phases, const uint32_t* por,
                               const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                               uint32_t threads, uint64_t* lat_ns, uint8_t* out_tri, uint64_t* out_hash,
                               uint64_t* wall_ns) {
    if (!b || !phases || !por || !arena || !offs || !lens || !lat_ns || !out_tri || !out_hash || !wall_ns ||
        threads == 0)
        return AUTHJX_EINVAL;
    std::atomic<int> first_rc{AUTHJX_OK};
    const uint64_t t0 = ajx::mono_ns();
    std::vector<std::thread> ts;
    for (uint32_t t = 0; t < threads; t++)
        ts.emplace_back([&, t] {
            uint8_t tri[64];
            std::vector<uint8_t> text;
            std::vector<authjx_rendered> rec;
            for (uint32_t i = t; i < n; i += threads) {
                const authjx_phase* ph = phases[por[i]];
                if (!ph || ph->rules->c.n_trees > 64) {
                    first_rc.store(AUTHJX_EINVAL);
                    return;
                }
                text.resize(ph->f.out_stride);
                rec.resize(ph->f.n_outputs + 1);
                const uint64_t a = ajx::mono_ns();
                const int rc = authjx_batcher_phase(b, ph, arena + offs[i], lens[i], 0, tri, nullptr, text.data(),
                                                    rec.data());
                lat_ns[i] = ajx::mono_ns() - a;
                out_tri[i] = tri[0];
                uint64_t hsh = 0xcbf29ce484222325ull;
                for (uint32_t k = 0; rc == AUTHJX_OK && k < ph->f.n_outputs; k++) {
                    hsh = (hsh ^ rec[k].status) * 0x100000001b3ull;
                    for (uint32_t q = 0; rec[k].status == AUTHJX_RENDER_OK && q < rec[k].len; q++)
                        hsh = (hsh ^ text[rec[k].start + q]) * 0x100000001b3ull;
                }
                out_hash[i] = hsh;
                if (rc != AUTHJX_OK) {
                    int ok = AUTHJX_OK;
                    first_rc.compare_exchange_strong(ok, rc);
                }
            }
        });
    for (auto& th : ts) th.join();
    *wall_ns = ajx::mono_ns() - t0;
    return first_rc.load();
}

// Profiling only (not in authjx.h): the serving path under load. `threads` producer threads
// each submit their share of the n requests (request i: sets[sor[i]] on arena[offs[i] ..
// offs[i] + lens[i]); thread t takes i = t, t + threads, ...) one at a time through the
// batcher (authjx_batcher_eval, blocking, as a serving goroutine would); lat_ns[i] = that
// call's latency, out_tri[i] its first result; *wall_ns = the whole run.
int authjx_debug_loadgen(authjx_batcher* b, const authjx_ruleset* const* sets, const uint32_t* sor,
                         const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                         uint32_t threads, uint64_t* lat_ns, uint8_t* out_tri, uint64_t* wall_ns) {
    if (!b || !sets || !sor || !arena || !offs || !lens || !lat_ns || !out_tri || !wall_ns || threads == 0)
        return AUTHJX_EINVAL;
    std::atomic<int> first_rc{AUTHJX_OK};
    const uint64_t t0 = ajx::mono_ns();
    std::vector<std::thread> ts;
    for (uint32_t t = 0; t < threads; t++)
        ts.emplace_back([&, t] {
            uint8_t tri[64];
            for (uint32_t i = t; i < n; i += threads) {
                const authjx_ruleset* rs = sets[sor[i]];
                if (rs->c.n_trees > 64) {
                    first_rc.store(AUTHJX_EINVAL);
                    return;
                }
                const uint64_t a = ajx::mono_ns();
                const int rc = authjx_batcher_eval(b, rs, arena + offs[i], lens[i], 0, tri, nullptr);
                lat_ns[i] = ajx::mono_ns() - a;
                out_tri[i] = tri[0];
                if (rc != AUTHJX_OK) {
                    int ok = AUTHJX_OK;
                    first_rc.compare_exchange_strong(ok, rc);
                }
            }
        });
    for (auto& th : ts) th.join();
    *wall_ns = ajx::mono_ns() - t0;
    return first_rc.load();
}

int authjx_batcher_stats(authjx_batcher* b, uint64_t* batches, uint64_t* requests, uint64_t* expired,
                         uint64_t* max_batch_seen) {
    if (!b) return AUTHJX_EINVAL;
    const ajx::BatchStats st = b->core->stats();
    if (batches) *batches = st.batches;
    if (requests) *requests = st.requests;
    if (expired) *expired = st.expired;
    if (max_batch_seen) *max_batch_seen = st.max_batch_seen;
    return AUTHJX_OK;
}

}  // extern "C"
