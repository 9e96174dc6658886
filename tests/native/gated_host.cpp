// gated_host.cpp — TEST-ONLY host build of the verdict fold (authorino_amd/csrc/ajx_verdict.h)
// and of the gated render kernel's per-request body (render_request_gated,
// ajx_render_gated.h) on top of render_multi_host.cpp's program builder and ungated calls,
// for tests/test_gated_host.py, tests/test_gpu_render_gated.py (its oracle) and san_gated.
// Not part of libauthjx.so.
#include "render_multi_host.cpp"

#include "../../authorino_amd/csrc/ajx_render_gated.h"

struct GtGates {
    std::vector<uint8_t> blob;
    uint32_t n_outputs = 0, n_trees = 0;
};

extern "C" {

// authjx_gates_compile's checks and layout (build_gates); nullptr and *rc on error
void* gt_gates_compile(int32_t top, const authjx_gate_evaluator* evals, uint32_t n_evals,
                       const authjx_gate_output* outs, uint32_t n_outputs, uint32_t n_trees, char* err, size_t cap,
                       int* rc) {
    GtGates* g = new GtGates();
    std::string e;
    *rc = build_gates(top, evals, n_evals, outs, n_outputs, n_trees, &g->blob, &e);
    if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
    if (*rc != AUTHJX_OK) { delete g; return nullptr; }
    g->n_outputs = n_outputs;
    g->n_trees = n_trees;
    return g;
}

void gt_gates_free(void* h) { delete (GtGates*)h; }

// authjx_verdict_of's body
int gt_verdict_of(void* h, const uint8_t* tri, uint32_t n_trees, authjx_verdict* out) {
    return h ? gates_verdict_of(((GtGates*)h)->blob.data(), tri, n_trees, out) : AUTHJX_EINVAL;
}

// the status of output k under a verdict (gate_output)
uint32_t gt_output_status(void* h, const uint8_t* tri, uint32_t verdict, uint32_t k) {
    return gate_output(((GtGates*)h)->blob.data(), tri, verdict, k);
}

// authjx_render_batch_gated_device on the CPU, with its argument checks: request r renders
// progs[prog_of_req[r]] under gates[prog_of_req[r]] over exact-size heap copies of its
// document, values, text slot, output slot, records and of the n_trees tri-states its gates
// name (none without gates), so that a sanitizer build sees any access outside them. A
// request without a program gets no buffer at all.
int gtm_render(void* const* progs, void* const* gates, uint32_t n_progs, const uint32_t* prog_of_req,
               const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n, const uint32_t* values,
               uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
               uint32_t out_stride, uint32_t* out, uint32_t records_stride, const uint8_t* tri, uint32_t tri_stride,
               const uint32_t* tri_of_req, uint32_t* verdicts) {
    if (!progs || !gates || n_progs == 0 || out_stride == 0 || out_stride % 16u || (n_progs > 1 && !prog_of_req))
        return AUTHJX_EINVAL;
    std::vector<const uint8_t*> blobs(n_progs), gblobs(n_progs);
    for (uint32_t i = 0; i < n_progs; i++) {
        const RtProgram* p = (const RtProgram*)progs[i];
        if (!p || values_stride < p->n_slots || records_stride < p->n_outputs) return AUTHJX_EINVAL;
        const GtGates* g = (const GtGates*)gates[i];
        if (g && (g->n_outputs != p->n_outputs || g->n_trees > tri_stride || !tri)) return AUTHJX_EINVAL;
        blobs[i] = p->blob.data();
        gblobs[i] = g ? g->blob.data() : nullptr;
    }
    uint32_t levels[kMaxRenderDepth * kRenderLevelWords];
    const RenderStack st{levels, 1};
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t pi = prog_of_req ? prog_of_req[r] : 0u;
        if (pi >= n_progs) {
            render_request_gated(blobs.data(), gblobs.data(), n_progs, pi, nullptr, nullptr, lens[r], nullptr, nullptr,
                                 text_stride, nullptr, out_stride, nullptr, nullptr, st);
            continue;
        }
        const RtProgram* p = (const RtProgram*)progs[pi];
        const GtGates* g = (const GtGates*)gates[pi];
        std::vector<uint8_t> doc(arena + offs[r], arena + offs[r] + lens[r]);
        std::vector<uint8_t> txt, row;
        if (text) txt.assign(text + (size_t)r * text_stride, text + (size_t)(r + 1) * text_stride);
        if (g) {
            const uint8_t* t0 = tri + (size_t)(tri_of_req ? tri_of_req[r] : r) * tri_stride;
            row.assign(t0, t0 + g->n_trees);
        }
        uint8_t* slot = (uint8_t*)std::aligned_alloc(16, out_stride);
        std::memcpy(slot, out_text + (size_t)r * out_stride, out_stride);
        const uint32_t* v0 = values + (size_t)r * values_stride * 3;
        std::vector<uint32_t> vals(v0, v0 + (size_t)p->n_slots * 3);
        std::vector<uint32_t> res(3 * (size_t)p->n_outputs);
        uint32_t ver[2] = {0, 0};
        render_request_gated(blobs.data(), gblobs.data(), n_progs, pi, g ? row.data() : nullptr, doc.data(), lens[r],
                             vals.data(), text ? txt.data() : nullptr, text_stride, slot, out_stride, res.data(),
                             verdicts ? ver : nullptr, st);
        std::memcpy(out_text + (size_t)r * out_stride, slot, out_stride);
        if (!res.empty()) std::memcpy(out + (size_t)r * records_stride * 3, res.data(), 4 * res.size());
        if (verdicts && g) std::memcpy(verdicts + (size_t)r * 2, ver, 8);
        std::free(slot);
    }
    return AUTHJX_OK;
}

}  // extern "C"
