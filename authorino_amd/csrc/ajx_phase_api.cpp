// ajx_phase_api.cpp — the phase object of the C-ABI (include/authjx.h): one AuthConfig's rules,
// response selectors and render program as authjx_batcher_phase (ajx_batcher_api.cpp) takes
// them. A translation unit of its own: it ties a phase to the render kernel
// (ajx_render.hip), which the batcher's translation unit does not reference.
#include "ajx_phase_api.h"
#include "ajx_render_api.h"

namespace {

int render_launch(const uint8_t* const* progs, uint32_t n_progs, const uint32_t* prog_of_req, const uint8_t* arena,
                  const uint64_t* offs, const uint32_t* lens, uint32_t n, const uint32_t* values,
                  uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
                  uint32_t out_stride, uint32_t* out, uint32_t records_stride, void* stream) {
    return (int)ajx::launch_render_multi(progs, n_progs, prog_of_req, arena, offs, lens, n, values, values_stride, text,
                                         text_stride, out_text, out_stride, out, records_stride, (hipStream_t)stream);
}

}  // namespace

int authjx_phase_create(authjx_ctx* ctx, const authjx_ruleset* rules, const authjx_ruleset* selectors,
                        const authjx_render* prog, uint32_t text_stride, uint32_t out_stride, authjx_phase** out) {
    if (out) *out = nullptr;
    if (!ctx || !rules || !selectors || !prog || !out) return AUTHJX_EINVAL;
    // (no patterns: the select would have no value to write; such a ruleset selects nothing)
    if (selectors->c.n_trees > 1 || selectors->c.n_patterns == 0 || selectors->c.n_patterns < prog->n_slots)
        return AUTHJX_EINVAL;
    if (out_stride == 0 || out_stride % 16u != 0) return AUTHJX_EINVAL;
    if (rules->device != ctx->device || selectors->device != ctx->device || prog->device != ctx->device)
        return AUTHJX_EINVAL;
    if (out_stride > 65536u || text_stride > 65536u) return AUTHJX_ELIMIT;  // (pinned staging per request)
    authjx_phase* ph = new authjx_phase();
    ph->device = ctx->device;
    ph->rules = rules;
    ph->selectors = selectors;
    ph->prog = prog;
    ph->f.selectors = selectors;
    ph->f.prog = prog->d_prog.data();
    ph->f.render = render_launch;
    ph->f.n_patterns = selectors->c.n_patterns;
    ph->f.n_outputs = prog->n_outputs;
    ph->f.text_stride = text_stride;
    ph->f.out_stride = out_stride;
    *out = ph;
    return AUTHJX_OK;
}

void authjx_phase_free(authjx_phase* ph) { delete ph; }  // (host memory only: no kernel reads it)

uint32_t authjx_phase_outputs(const authjx_phase* ph) { return ph ? ph->f.n_outputs : 0u; }
