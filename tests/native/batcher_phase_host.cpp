// batcher_phase_host.cpp — TEST-ONLY: the micro-batcher's queue (ajx_batcher.h) with phase
// requests, and the phase plan and delivery the device batcher runs (ajx_phase.h:
// plan_phases, deliver_phase), driven on the CPU with a stand-in for the device work. The
// stand-in "evaluates" every request as batcher_host.cpp does and "renders" each phase
// request into a staging buffer laid out by the plan's groups, from the request's document
// byte and its phase's program id, so the tests can check that every caller gets its own
// outputs through the plan's index mapping.
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>

#include "../../authorino_amd/csrc/ajx_phase.h"

using namespace ajx;

namespace {
struct Host {
    BatchCore* core = nullptr;
    uint32_t delay_us = 0;
    std::atomic<uint64_t> plan_violations{0}, groups{0}, mixed_batches{0}, phase_requests{0};
};

// output q of a phase request: 1 + (byte + q) % 5 bytes of value byte ^ q ^ program id
void fake_render(const PhaseFacts& f, uint8_t byte, uint8_t* slot, uint32_t* rec) {
    uint32_t pos = 0;
    for (uint32_t q = 0; q < f.n_outputs; q++) {
        const uint32_t len = 1 + (byte + q) % 5;
        rec[3 * q] = pos;
        if (pos + len > f.out_stride) {  // (declined: appends nothing)
            rec[3 * q + 1] = 0;
            rec[3 * q + 2] = 1;
            continue;
        }
        std::memset(slot + pos, (uint8_t)(byte ^ q ^ (uintptr_t)f.prog), len);
        rec[3 * q + 1] = len;
        rec[3 * q + 2] = 0;
        pos += len;
    }
}

int evaluate(Host* h, std::vector<BatchReq*>& reqs) {
    const PhasePlan plan = plan_phases(reqs);
    const uint32_t rs = plan.records_stride;
    std::vector<uint32_t> rec((size_t)plan.n() * rs * 3 + 1, 0xA5A5A5A5u);
    std::vector<std::vector<uint8_t>> slots(plan.groups.size());
    uint32_t covered = 0;
    for (size_t gi = 0; gi < plan.groups.size(); gi++) {
        const PhaseGroup& g = plan.groups[gi];
        if (g.first != covered || g.set_of.size() != g.count) h->plan_violations++;
        covered += g.count;
        slots[gi].assign((size_t)g.count * g.out_stride, 0xEE);  // (stale bytes: must not reach a caller)
        for (uint32_t j = 0; j < g.count; j++) {
            const BatchReq& r = *reqs[plan.req[g.first + j]];
            const PhaseFacts& f = *r.phase;
            if (f.text_stride != g.text_stride || f.out_stride != g.out_stride || g.sets[g.set_of[j]] != f.selectors ||
                plan.progs[plan.prog_of[g.first + j]] != f.prog || f.n_outputs > rs || f.n_patterns > plan.values_stride)
                h->plan_violations++;
            fake_render(f, r.doc[0], slots[gi].data() + (size_t)j * g.out_stride,
                        rec.data() + (size_t)(g.first + j) * rs * 3);
        }
    }
    if (covered != plan.n()) h->plan_violations++;
    h->groups += plan.groups.size();
    h->phase_requests += plan.n();
    if (plan.n() && plan.n() < reqs.size()) h->mixed_batches++;
    if (h->delay_us) std::this_thread::sleep_for(std::chrono::microseconds(h->delay_us));
    for (BatchReq* r : reqs)
        for (uint32_t k = 0; k < r->n_out; k++)
            r->out_tri[k] = (uint8_t)(r->doc[0] ^ (uint8_t)(uintptr_t)r->rs ^ (uint8_t)k);
    for (size_t gi = 0; gi < plan.groups.size(); gi++) {
        const PhaseGroup& g = plan.groups[gi];
        for (uint32_t j = 0; j < g.count; j++)
            deliver_phase(*reqs[plan.req[g.first + j]], slots[gi].data() + (size_t)j * g.out_stride,
                          rec.data() + (size_t)(g.first + j) * rs * 3);
    }
    return 0;
}
}  // namespace

extern "C" {

void* hbp_create(uint32_t max_batch, uint32_t window_us, uint32_t delay_us, uint32_t workers, uint32_t wake) {
    Host* h = new Host();
    h->delay_us = delay_us;
    h->core = new BatchCore(max_batch, (uint64_t)window_us * 1000ull, 0,
                            [h](std::vector<BatchReq*>& reqs, uint32_t) { return evaluate(h, reqs); }, workers, wake);
    return h;
}

// a phase: selector ruleset id and program id (nonzero, opaque), the facts the plan reads
void* hbp_phase_new(uint64_t selectors, uint64_t prog, uint32_t n_patterns, uint32_t n_outputs, uint32_t text_stride,
                    uint32_t out_stride) {
    PhaseFacts* f = new PhaseFacts();
    f->selectors = (const void*)(uintptr_t)selectors;
    f->prog = (const void*)(uintptr_t)prog;
    f->n_patterns = n_patterns;
    f->n_outputs = n_outputs;
    f->text_stride = text_stride;
    f->out_stride = out_stride;
    return f;
}
void hbp_phase_free(void* f) { delete (PhaseFacts*)f; }

// one request: ruleset id `rs` (nonzero), result shape n_out, one document byte; phase (or
// null: an eval-only request) with the caller's out_text / out_rec
int hbp_call(void* hv, uint64_t rs, uint32_t n_out, uint8_t byte, const void* phase, uint64_t timeout_us,
             uint8_t* out_tri, uint8_t* out_text, uint32_t* out_rec) {
    Host* h = (Host*)hv;
    BatchReq r;
    r.rs = (const void*)(uintptr_t)rs;
    r.n_out = n_out;
    r.doc = &byte;
    r.len = 1;
    r.deadline_ns = timeout_us ? mono_ns() + timeout_us * 1000ull : 0;
    r.out_tri = out_tri;
    r.phase = (const PhaseFacts*)phase;
    r.out_text = out_text;
    r.out_rec = out_rec;
    return h->core->submit(r);
}

void hbp_stats(void* hv, uint64_t* out) {
    Host* h = (Host*)hv;
    const BatchStats st = h->core->stats();
    out[0] = st.batches;
    out[1] = st.requests;
    out[2] = st.expired;
    out[3] = st.max_batch_seen;
    out[4] = h->plan_violations.load();
    out[5] = h->groups.load();
    out[6] = h->mixed_batches.load();
    out[7] = h->phase_requests.load();
}

void hbp_destroy(void* hv) {
    Host* h = (Host*)hv;
    delete h->core;
    delete h;
}
}
