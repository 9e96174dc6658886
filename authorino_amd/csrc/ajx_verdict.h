// ajx_verdict.h — the verdict fold: auth_pipeline.go's `when` gates and authorization
// phase (AuthConfig `when`, evaluator `when`, rules by priority, per-response `when`) over
// one request's tri-states, and which outputs of a render program apply under the verdict
// (include/authjx.h has the rule; authorino_amd/pipeline.py verdict_of restates it). One
// function for the gated render kernel (ajx_render.hip), authjx_verdict_of and the CPU
// tests: plain loops over the gates blob, a handful of bytes per request, no memory of its
// own.
//
// Gates blob (build_gates): GatesHdr | authjx_gate_evaluator[n_evals] | GateOutput[n_outputs].
#pragma once
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/authjx.h"

#ifndef AJX_VERDICT_HD
#if defined(__HIPCC__)
#define AJX_VERDICT_HD __host__ __device__ __forceinline__
#else
#define AJX_VERDICT_HD inline
#endif
#endif

namespace ajx {

constexpr uint32_t kGatesMagic = 0x53544147u;

struct GatesHdr {
    uint32_t magic, n_trees, n_evals, n_outputs;
    int32_t top;
    uint32_t off_evals, off_outputs, total;
};
struct GateOutput {
    uint32_t on;
    int32_t when;
};

// the tri-state of tree `tree`, a missing one (-1) standing for T
AJX_VERDICT_HD uint32_t gate_tri(const uint8_t* t, int32_t tree) { return tree < 0 ? (uint32_t)AUTHJX_T : t[tree]; }

// The verdict of tri-states t[0, n_trees) under `gates`; *denied_by: the denying evaluator or -1.
AJX_VERDICT_HD uint32_t verdict_fold(const uint8_t* gates, const uint8_t* t, int32_t* denied_by) {
    const GatesHdr* h = reinterpret_cast<const GatesHdr*>(gates);
    const authjx_gate_evaluator* ev = reinterpret_cast<const authjx_gate_evaluator*>(gates + h->off_evals);
    *denied_by = -1;
    const uint32_t top = gate_tri(t, h->top);
    if (top == AUTHJX_UNDECIDED) return AUTHJX_V_UNDECIDED;
    if (top != AUTHJX_T) return AUTHJX_V_SKIPPED;
    for (uint32_t i = 0; i < h->n_evals;) {
        const int32_t prio = ev[i].priority;
        bool undecided = false;
        int32_t deny = -1;
        for (; i < h->n_evals && ev[i].priority == prio; i++) {
            const uint32_t w = gate_tri(t, ev[i].when_tree), r = gate_tri(t, ev[i].rules_tree);
            undecided = undecided || w == AUTHJX_UNDECIDED || r == AUTHJX_UNDECIDED;
            if (deny < 0 && w == AUTHJX_T && r != AUTHJX_T) deny = (int32_t)i;
        }
        if (undecided) return AUTHJX_V_UNDECIDED;
        if (deny >= 0) {
            *denied_by = deny;
            return AUTHJX_V_DENIED;
        }
    }
    return AUTHJX_V_GRANTED;
}

// Output k under `verdict`: AUTHJX_RENDER_OK (it renders), _UNRENDERED or _SKIPPED.
AJX_VERDICT_HD uint32_t gate_output(const uint8_t* gates, const uint8_t* t, uint32_t verdict, uint32_t k) {
    const GatesHdr* h = reinterpret_cast<const GatesHdr*>(gates);
    const GateOutput g = reinterpret_cast<const GateOutput*>(gates + h->off_outputs)[k];
    if (g.on == AUTHJX_GATE_ALWAYS) return AUTHJX_RENDER_OK;
    if (verdict == AUTHJX_V_UNDECIDED) return AUTHJX_RENDER_UNRENDERED;
    if (g.on == AUTHJX_GATE_DENIED) return verdict == AUTHJX_V_DENIED ? AUTHJX_RENDER_OK : AUTHJX_RENDER_SKIPPED;
    if (verdict != AUTHJX_V_GRANTED) return AUTHJX_RENDER_SKIPPED;
    const uint32_t w = gate_tri(t, g.when);
    return w == AUTHJX_T ? AUTHJX_RENDER_OK : w == AUTHJX_UNDECIDED ? AUTHJX_RENDER_UNRENDERED : AUTHJX_RENDER_SKIPPED;
}

// authjx_gates_compile's checks and the blob's layout
inline int build_gates(int32_t top, const authjx_gate_evaluator* evals, uint32_t n_evals,
                       const authjx_gate_output* outs, uint32_t n_outputs, uint32_t n_trees,
                       std::vector<uint8_t>* blob, std::string* err) {
    if ((!evals && n_evals) || (!outs && n_outputs)) { *err = "no evaluators or outputs"; return AUTHJX_EINVAL; }
    const auto tree_ok = [&](int32_t t) { return t >= -1 && (t < 0 || (uint32_t)t < n_trees); };
    if (!tree_ok(top)) { *err = "top when_tree out of range"; return AUTHJX_EINVAL; }
    for (uint32_t i = 0; i < n_evals; i++) {
        const std::string at = "evaluator " + std::to_string(i);
        if (!tree_ok(evals[i].when_tree) || !tree_ok(evals[i].rules_tree)) {
            *err = at + ": tree out of range";
            return AUTHJX_EINVAL;
        }
        if (i && evals[i].priority < evals[i - 1].priority) {
            *err = at + ": priorities must not decrease";
            return AUTHJX_EINVAL;
        }
    }
    std::vector<GateOutput> go(n_outputs);
    for (uint32_t k = 0; k < n_outputs; k++) {
        const std::string at = "output " + std::to_string(k);
        if (outs[k].on > AUTHJX_GATE_DENIED) { *err = at + ": unknown `on`"; return AUTHJX_EINVAL; }
        if (!tree_ok(outs[k].when_tree)) { *err = at + ": tree out of range"; return AUTHJX_EINVAL; }
        if (outs[k].on != AUTHJX_GATE_GRANTED && outs[k].when_tree >= 0) {
            *err = at + ": only a GRANTED output has a when_tree";
            return AUTHJX_EINVAL;
        }
        go[k] = {outs[k].on, outs[k].when_tree};
    }
    GatesHdr h;
    h.magic = kGatesMagic;
    h.n_trees = n_trees;
    h.n_evals = n_evals;
    h.n_outputs = n_outputs;
    h.top = top;
    h.off_evals = sizeof(GatesHdr);
    h.off_outputs = h.off_evals + n_evals * (uint32_t)sizeof(authjx_gate_evaluator);
    h.total = (h.off_outputs + n_outputs * (uint32_t)sizeof(GateOutput) + 15u) & ~15u;
    blob->assign(h.total, 0);
    std::memcpy(blob->data(), &h, sizeof h);
    if (n_evals) std::memcpy(blob->data() + h.off_evals, evals, n_evals * sizeof(authjx_gate_evaluator));
    if (n_outputs) std::memcpy(blob->data() + h.off_outputs, go.data(), n_outputs * sizeof(GateOutput));
    return AUTHJX_OK;
}

// authjx_verdict_of over a gates blob
inline int gates_verdict_of(const uint8_t* gates, const uint8_t* tristate, uint32_t n_trees, authjx_verdict* out) {
    if (!gates || !out || reinterpret_cast<const GatesHdr*>(gates)->n_trees > n_trees || (n_trees && !tristate))
        return AUTHJX_EINVAL;
    int32_t by;
    const uint32_t v = verdict_fold(gates, tristate, &by);
    *out = authjx_verdict{(uint8_t)v, {0, 0, 0}, by};
    return AUTHJX_OK;
}

}  // namespace ajx
