// ajx_render_gated_api.cpp — the gated render entry points of the C-ABI (include/authjx.h):
// gates objects (ajx_verdict.h's blob, resident in HBM and kept on the host), the verdict
// fold on the host and the batch calls that run the gated kernel (ajx_render.hip). A
// translation unit of its own: ajx_render_api.cpp does not reference it.
#include <cstdio>
#include <string>

#include "ajx_host.h"
#include "ajx_phase_api.h"
#include "ajx_render_api.h"
#include "ajx_verdict.h"

static_assert(sizeof(authjx_verdict) == 8, "authjx_verdict is two u32 words on the device");
static_assert(sizeof(authjx_gate_evaluator) == 12, "authjx_gate_evaluator is three i32 words in the blob");

int authjx_gates_compile(authjx_ctx* ctx, int32_t top_when_tree, const authjx_gate_evaluator* evaluators,
                         uint32_t n_evaluators, const authjx_gate_output* outputs, uint32_t n_outputs,
                         uint32_t n_trees, authjx_gates** out, char* errbuf, size_t errcap) {
    if (errbuf && errcap) errbuf[0] = 0;
    if (!ctx || !out) return AUTHJX_EINVAL;
    *out = nullptr;
    authjx_gates* g = new authjx_gates();
    std::string err;
    const int rc = ajx::build_gates(top_when_tree, evaluators, n_evaluators, outputs, n_outputs, n_trees, &g->blob, &err);
    if (rc != AUTHJX_OK) {
        if (errbuf && errcap) std::snprintf(errbuf, errcap, "%s", err.c_str());
        delete g;
        return rc;
    }
    g->device = ctx->device;
    g->n_outputs = n_outputs;
    g->n_trees = n_trees;
    if (hipSetDevice(g->device) != hipSuccess || g->d_blob.reserve(g->blob.size()) != hipSuccess ||
        hipMemcpy(g->d_blob.data(), g->blob.data(), g->blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        delete g;
        return AUTHJX_EDEVICE;
    }
    *out = g;
    return AUTHJX_OK;
}

void authjx_gates_free(authjx_gates* gates) {
    if (!gates) return;
    if (gates->d_blob.data()) (void)hipSetDevice(gates->device);
    delete gates;  // (freeing the blob waits for the kernels that read it)
}

int authjx_verdict_of(const authjx_gates* gates, const uint8_t* tristate, uint32_t n_trees, authjx_verdict* out) {
    if (!gates) return AUTHJX_EINVAL;
    return ajx::gates_verdict_of(gates->blob.data(), tristate, n_trees, out);
}

int authjx_render_batch_gated_device(authjx_ctx* ctx, const authjx_render* const* progs, uint32_t n_progs,
                                     const uint32_t* d_prog_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                                     const uint32_t* d_lens, uint32_t n, const authjx_value* d_values,
                                     uint32_t values_stride, const uint8_t* d_text, uint32_t text_stride,
                                     uint8_t* d_out_text, uint32_t out_stride, authjx_rendered* d_out,
                                     uint32_t records_stride, const authjx_gates* const* gates,
                                     const uint8_t* d_tristate, uint32_t tri_stride, const uint32_t* d_tri_of_req,
                                     authjx_verdict* d_out_verdict, void* stream) {
    if (!ctx || !progs || !gates || n_progs == 0) return AUTHJX_EINVAL;
    if (out_stride == 0 || out_stride % 16u != 0 || (n_progs > 1 && !d_prog_of_req)) return AUTHJX_EINVAL;
    std::vector<const uint8_t*> tables(2 * (size_t)n_progs);  // the programs, then their gates
    uint32_t slots = 0;
    for (uint32_t i = 0; i < n_progs; i++) {
        const authjx_render* p = progs[i];
        if (!p || p->device != ctx->device || values_stride < p->n_slots || records_stride < p->n_outputs)
            return AUTHJX_EINVAL;
        const authjx_gates* g = gates[i];
        if (g && (g->device != ctx->device || g->n_outputs != p->n_outputs || g->n_trees > tri_stride || !d_tristate))
            return AUTHJX_EINVAL;
        tables[i] = p->d_prog.data();
        tables[n_progs + i] = g ? g->d_blob.data() : nullptr;
        slots = std::max(slots, p->n_slots);
    }
    if (n && (!d_arena || !d_offs || !d_lens || !d_out_text || !d_out || (slots && !d_values)))
        return AUTHJX_EINVAL;
    if (((uintptr_t)d_out_text & 15u) != 0) return AUTHJX_EINVAL;
    if (n == 0) return AUTHJX_OK;
    return with_ptr_table(ctx, stream, tables.data(), 2 * n_progs, [&](const uint8_t* const* d_tables, hipStream_t s) {
        return ajx::launch_render_gated(d_tables, n_progs, d_prog_of_req, d_arena, d_offs, d_lens, n,
                                        reinterpret_cast<const uint32_t*>(d_values), values_stride, d_text,
                                        text_stride, d_out_text, out_stride, reinterpret_cast<uint32_t*>(d_out),
                                        records_stride, d_tristate, tri_stride, d_tri_of_req,
                                        reinterpret_cast<uint32_t*>(d_out_verdict), s);
    });
}

int authjx_render_batch_gated(authjx_ctx* ctx, const authjx_render* const* progs, uint32_t n_progs,
                              const uint32_t* prog_of_req, const uint8_t* arena, uint64_t arena_len,
                              const uint64_t* offs, const uint32_t* lens, uint32_t n, const authjx_value* values,
                              uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
                              uint32_t out_stride, authjx_rendered* out, uint32_t records_stride,
                              const authjx_gates* const* gates, const uint8_t* tristate, uint32_t tri_stride,
                              const uint32_t* tri_of_req, authjx_verdict* out_verdict) {
    if (!ctx || !progs || !gates || n_progs == 0) return AUTHJX_EINVAL;
    if (out_stride == 0 || out_stride % 16u != 0 || (n_progs > 1 && !prog_of_req)) return AUTHJX_EINVAL;
    uint32_t slots = 0;
    for (uint32_t i = 0; i < n_progs; i++) {  // (the device call's table, before anything is staged)
        const authjx_render* p = progs[i];
        const authjx_gates* g = gates[i];
        if (!p || p->device != ctx->device || values_stride < p->n_slots || records_stride < p->n_outputs)
            return AUTHJX_EINVAL;
        if (g && (g->device != ctx->device || g->n_outputs != p->n_outputs || g->n_trees > tri_stride || !tristate))
            return AUTHJX_EINVAL;
        slots = std::max(slots, p->n_slots);
    }
    if (n == 0) return AUTHJX_OK;
    if (!arena || !offs || !lens || !out_text || !out || (slots && !values)) return AUTHJX_EINVAL;
    if (!ajx::spans_in_arena(offs, lens, n, arena_len)) return AUTHJX_EINVAL;
    size_t tri_rows = tristate ? n : 0;
    if (tristate && tri_of_req) {
        tri_rows = 0;
        for (uint32_t r = 0; r < n; r++) tri_rows = std::max(tri_rows, (size_t)tri_of_req[r] + 1);
    }
    const size_t val_bytes = (size_t)n * values_stride * sizeof(authjx_value);
    const size_t text_bytes = text ? (size_t)n * text_stride : 0;
    const size_t outt_bytes = (size_t)n * out_stride, out_bytes = (size_t)n * records_stride * sizeof(authjx_rendered);
    const size_t tri_bytes = tri_rows * tri_stride, ver_bytes = out_verdict ? (size_t)n * sizeof(authjx_verdict) : 0;
    ajx::StageLayout lay;
    lay.add(arena_len);  // (the arena at 0)
    const size_t o_offs = lay.add((size_t)n * 8), o_lens = lay.add((size_t)n * 4);
    const size_t o_por = lay.add(prog_of_req ? (size_t)n * 4 : 0), o_tor = lay.add(tri_of_req ? (size_t)n * 4 : 0);
    const size_t o_val = lay.add(val_bytes), o_text = lay.add(text_bytes), o_tri = lay.add(tri_bytes);
    const size_t o_outt = lay.add(outt_bytes), o_out = lay.add(out_bytes), o_ver = lay.add(ver_bytes);
    HIP_OK(hipSetDevice(ctx->device));
    ajx::DeviceBuf buf;  // (a buffer per call: freed on every return)
    HIP_OK(buf.reserve(lay.total() + 256));
    uint8_t* b = buf.data();
    hipStream_t s = ctx->stream;
    const auto up = [&](size_t at, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(b + at, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIP_OK(up(0, arena, arena_len));
    HIP_OK(up(o_offs, offs, (size_t)n * 8));
    HIP_OK(up(o_lens, lens, (size_t)n * 4));
    HIP_OK(up(o_por, prog_of_req, prog_of_req ? (size_t)n * 4 : 0));
    HIP_OK(up(o_tor, tri_of_req, tri_of_req ? (size_t)n * 4 : 0));
    HIP_OK(up(o_val, values, val_bytes));
    HIP_OK(up(o_text, text, text_bytes));
    HIP_OK(up(o_tri, tristate, tri_bytes));
    // (what the kernel does not write comes back as the caller's own: the host copies keep it)
    HIP_OK(up(o_outt, out_text, outt_bytes));
    HIP_OK(up(o_out, out, out_bytes));
    HIP_OK(up(o_ver, out_verdict, ver_bytes));
    const int rc = authjx_render_batch_gated_device(
        ctx, progs, n_progs, prog_of_req ? (const uint32_t*)(b + o_por) : nullptr, b, (const uint64_t*)(b + o_offs),
        (const uint32_t*)(b + o_lens), n, (const authjx_value*)(b + o_val), values_stride,
        text ? b + o_text : nullptr, text_stride, b + o_outt, out_stride, (authjx_rendered*)(b + o_out),
        records_stride, gates, tristate ? b + o_tri : nullptr, tri_stride,
        tri_of_req ? (const uint32_t*)(b + o_tor) : nullptr, out_verdict ? (authjx_verdict*)(b + o_ver) : nullptr, s);
    if (rc != AUTHJX_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    HIP_OK(hipMemcpyAsync(out_text, b + o_outt, outt_bytes, hipMemcpyDeviceToHost, s));
    if (out_bytes) HIP_OK(hipMemcpyAsync(out, b + o_out, out_bytes, hipMemcpyDeviceToHost, s));
    if (ver_bytes) HIP_OK(hipMemcpyAsync(out_verdict, b + o_ver, ver_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return AUTHJX_OK;
}

namespace {

int render_gated_launch(const uint8_t* const* tables, uint32_t n_progs, const uint32_t* prog_of_req,
                        const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                        const uint32_t* values, uint32_t values_stride, const uint8_t* text, uint32_t text_stride,
                        uint8_t* out_text, uint32_t out_stride, uint32_t* out, uint32_t records_stride,
                        const uint8_t* tri, uint32_t tri_stride, const uint32_t* tri_of_req, uint32_t* verdicts,
                        void* stream) {
    return (int)ajx::launch_render_gated(tables, n_progs, prog_of_req, arena, offs, lens, n, values, values_stride,
                                         text, text_stride, out_text, out_stride, out, records_stride, tri, tri_stride,
                                         tri_of_req, verdicts, (hipStream_t)stream);
}

}  // namespace

// (here, not in ajx_phase_api.cpp: this translation unit is the one that links the gated launch)
int authjx_phase_create_gated(authjx_ctx* ctx, const authjx_ruleset* rules, const authjx_ruleset* selectors,
                              const authjx_render* prog, const authjx_gates* gates, uint32_t text_stride,
                              uint32_t out_stride, authjx_phase** out) {
    if (out) *out = nullptr;
    if (!gates || !prog || !rules || !ctx) return AUTHJX_EINVAL;
    if (gates->device != ctx->device || gates->n_outputs != prog->n_outputs || gates->n_trees > rules->c.n_trees)
        return AUTHJX_EINVAL;
    const int rc = authjx_phase_create(ctx, rules, selectors, prog, text_stride, out_stride, out);
    if (rc != AUTHJX_OK) return rc;
    (*out)->f.gates = gates->d_blob.data();
    (*out)->f.render_gated = render_gated_launch;
    return AUTHJX_OK;
}
