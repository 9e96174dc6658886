// ajx_phase.h — the phase requests of a micro-batch (host C++, no HIP): which of a batch's
// requests also want their AuthConfig's response outputs (authjx_batcher_phase), in what
// order the select and the render see them, and how a finished request's outputs reach its
// caller. Evaluator-agnostic like ajx_batcher.h: ajx_batcher_api.cpp queues the device
// work this plan describes, the CPU tests run the plan with a stand-in
// (tests/native/batcher_phase_host.cpp).
//
// The select and render kernels take one text_stride and one out_stride per launch, and a
// phase has its own: the phase requests are ordered by (text_stride, out_stride), and each
// run of one pair is a group with its own select and render launch over a slice of the
// subset's arrays. One pair per deployment is the common case: one group, two launches.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ajx_batcher.h"

namespace ajx {

// The multi-program render launch (ajx::launch_render_multi, ajx_render_api.h) in plain types
// (stream: a hipStream_t; the result: a hipError_t). A phase carries it, so the batcher's
// translation unit queues the render without linking the kernel's: authjx_phase_create
// (ajx_phase_api.cpp) sets it, the CPU tests' stand-in leaves it null.
using PhaseRender = int (*)(const uint8_t* const* progs, uint32_t n_progs, const uint32_t* prog_of_req,
                            const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                            const uint32_t* values, uint32_t values_stride, const uint8_t* text, uint32_t text_stride,
                            uint8_t* out_text, uint32_t out_stride, uint32_t* out, uint32_t records_stride,
                            void* stream);

// The gated render launch (ajx::launch_render_gated) in plain types: tables holds the
// n_progs program blobs, then their n_progs gates blobs (null: ungated); tri / tri_stride /
// tri_of_req: the batch's tri-states and each request's row; verdicts: two words per request.
using PhaseRenderGated = int (*)(const uint8_t* const* tables, uint32_t n_progs, const uint32_t* prog_of_req,
                                 const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                                 const uint32_t* values, uint32_t values_stride, const uint8_t* text,
                                 uint32_t text_stride, uint8_t* out_text, uint32_t out_stride, uint32_t* out,
                                 uint32_t records_stride, const uint8_t* tri, uint32_t tri_stride,
                                 const uint32_t* tri_of_req, uint32_t* verdicts, void* stream);

// what the plan reads of a phase (authjx_phase holds one)
struct PhaseFacts {
    const void* selectors = nullptr;  // the selector ruleset
    const void* prog = nullptr;       // the render program's blob in device memory
    PhaseRender render = nullptr;
    uint32_t n_patterns = 0;          // of the selector ruleset: the values the select writes per request
    uint32_t n_outputs = 0;           // of the program
    uint32_t text_stride = 0, out_stride = 0;
    // a gated phase (authjx_phase_create_gated): its gates' blob in device memory and the
    // gated launch; null for an ungated one
    const void* gates = nullptr;
    PhaseRenderGated render_gated = nullptr;
};

struct PhaseGroup {
    uint32_t first = 0, count = 0;  // subset positions [first, first + count)
    uint32_t text_stride = 0, out_stride = 0;
    std::vector<const void*> sets;  // the group's selector rulesets as runs
    std::vector<uint32_t> set_of;   // per request of the group: index into sets
};

struct PhasePlan {
    std::vector<uint32_t> req;       // subset position j -> index in the batch
    std::vector<const void*> progs;  // the batch's distinct {program, gates} pairs: the programs
    std::vector<const void*> gates;  // ... and their gates (null: ungated), entry for entry
    std::vector<uint32_t> prog_of;   // per subset position: index into progs / gates
    std::vector<uint32_t> tri_row;   // per subset position: its row in the batch's tri-state array
    PhaseRenderGated render_gated = nullptr;  // set when a request of the batch is gated: every
                                              // group then takes the gated launch
    std::vector<PhaseGroup> groups;
    uint32_t values_stride = 0, records_stride = 0;  // the largest n_patterns / n_outputs
    uint32_t n() const { return (uint32_t)req.size(); }
};

inline PhasePlan plan_phases(const std::vector<BatchReq*>& reqs) {
    PhasePlan p;
    for (uint32_t i = 0; i < (uint32_t)reqs.size(); i++)
        if (reqs[i]->phase) p.req.push_back(i);
    if (p.req.empty()) return p;
    // (stable: the batch's ruleset order, and arrival order in it, hold inside a group)
    std::stable_sort(p.req.begin(), p.req.end(), [&](uint32_t a, uint32_t b) {
        const PhaseFacts &x = *reqs[a]->phase, &y = *reqs[b]->phase;
        return x.text_stride != y.text_stride ? x.text_stride < y.text_stride : x.out_stride < y.out_stride;
    });
    p.prog_of.resize(p.req.size());
    p.tri_row = p.req;  // (the evaluation writes request i's tri-states at row i)
    for (uint32_t j = 0; j < p.n(); j++) {
        const PhaseFacts& f = *reqs[p.req[j]]->phase;
        p.values_stride = std::max(p.values_stride, f.n_patterns);
        p.records_stride = std::max(p.records_stride, f.n_outputs);
        uint32_t k = 0;
        while (k < p.progs.size() && !(p.progs[k] == f.prog && p.gates[k] == f.gates)) k++;
        p.prog_of[j] = k;
        if (k == p.progs.size()) {
            p.progs.push_back(f.prog);
            p.gates.push_back(f.gates);
        }
        if (f.gates && !p.render_gated) p.render_gated = f.render_gated;
        if (p.groups.empty() || p.groups.back().text_stride != f.text_stride ||
            p.groups.back().out_stride != f.out_stride) {
            PhaseGroup g;
            g.first = j;
            g.text_stride = f.text_stride;
            g.out_stride = f.out_stride;
            p.groups.push_back(g);
        }
        PhaseGroup& g = p.groups.back();
        if (g.sets.empty() || g.sets.back() != f.selectors) g.sets.push_back(f.selectors);
        g.set_of.push_back((uint32_t)g.sets.size() - 1);
        g.count++;
    }
    return p;
}

// A finished phase request's outputs to its caller: the program's records, and the output
// slot up to the end of its last rendered output (the slot's bytes past it are unspecified
// on the device and may be an earlier batch's: they are not handed on). rec: three words
// per record {start, len, status}.
inline void deliver_phase(const BatchReq& r, const uint8_t* slot, const uint32_t* rec) {
    const PhaseFacts& f = *r.phase;
    uint32_t end = 0;
    for (uint32_t k = 0; k < f.n_outputs; k++) {
        const uint32_t s = rec[3 * k], len = rec[3 * k + 1];
        if (s <= f.out_stride && len <= f.out_stride - s) end = std::max(end, s + len);
    }
    if (end && r.out_text) std::memcpy(r.out_text, slot, end);
    if (f.n_outputs && r.out_rec) std::memcpy(r.out_rec, rec, 12u * (size_t)f.n_outputs);
}

// A gated phase request's verdict (two words: verdict, denied_by) to its caller.
inline void deliver_verdict(const BatchReq& r, const uint32_t* verdict) {
    if (r.phase->gates && r.out_verdict) std::memcpy(r.out_verdict, verdict, 8);
}

}  // namespace ajx
