// ajx_render_gated.h — a request of the gated render kernel: the verdict fold
// (ajx_verdict.h) over the request's tri-states, then its program's outputs
// (ajx_render.h), each one asked of the fold before its first op is read. AJX_HD code:
// __device__ in ajx_render.hip, plain inline functions in the test-only host build
// (tests/native/gated_host.cpp).
#pragma once
#include "ajx_render.h"
#include "ajx_verdict.h"

namespace ajx {

struct RenderGated {
    const uint8_t* gates;  // nullptr: every output renders
    const uint8_t* tri;
    uint32_t verdict;
    AJX_HD uint32_t operator()(uint32_t k) const { return gates ? gate_output(gates, tri, verdict, k) : kRenderOk; }
};

// render_request_multi under gates[prog] (a table beside progs; a null entry: ungated, no
// verdict written). tri: the request's tri-states; verdict: where its two words {verdict,
// denied_by} go, or nullptr. A request without a program reads and writes nothing.
AJX_HD void render_request_gated(const uint8_t* const* progs, const uint8_t* const* gates, uint32_t n_progs,
                                 uint32_t prog, const uint8_t* tri, const uint8_t* doc, uint32_t doc_len,
                                 const uint32_t* vals, const uint8_t* text, uint32_t text_cap, uint8_t* out,
                                 uint32_t out_cap, uint32_t* res, uint32_t* verdict, const RenderStack& st) {
    if (prog >= n_progs) return;
    RenderGated g{gates[prog], tri, AUTHJX_V_GRANTED};
    if (g.gates) {
        int32_t by;
        g.verdict = verdict_fold(g.gates, tri, &by);
        if (verdict) {
            verdict[0] = g.verdict;
            verdict[1] = (uint32_t)by;
        }
    }
    render_request_under(progs[prog], doc, doc_len, vals, text, text_cap, out, out_cap, res, st, g);
}

}  // namespace ajx
