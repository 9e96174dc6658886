// render_host.cpp — TEST-ONLY host build of the render logic (authorino_amd/csrc/ajx_render.h)
// and of the program builder (ajx_render_prog.h), so that the CPU suite checks them against
// the Python mirror (authorino_amd/response.py) without a GPU. Not part of libauthjx.so.
#define AJX_HD inline
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../authorino_amd/csrc/ajx_render.h"
#include "../../authorino_amd/csrc/ajx_render_prog.h"

using namespace ajx;

struct RtProgram {
    std::vector<uint8_t> blob;
    uint32_t n_outputs = 0, n_slots = 0;
};

extern "C" {

// authjx_render_compile's checks and layout (build_render_program); nullptr and *rc on error
void* rt_compile(const authjx_render_output* outs, uint32_t n_outputs, uint32_t n_slots, char* err, size_t cap,
                 int* rc) {
    RtProgram* p = new RtProgram();
    std::string e;
    *rc = build_render_program(outs, n_outputs, n_slots, &p->blob, &e);
    if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
    if (*rc != AUTHJX_OK) { delete p; return nullptr; }
    p->n_outputs = n_outputs;
    p->n_slots = n_slots;
    return p;
}

void rt_free(void* h) { delete (RtProgram*)h; }

int rt_max_depth(void) { return kMaxRenderDepth; }

// authjx_render_batch on the CPU: one render_request per request, each over exact-size heap
// copies of its document, text slot and output slot (so that a sanitizer build sees any
// access outside them). The output slot's bytes are copied in and out: what the code does
// not write stays the caller's.
int rt_render(void* h, const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
              const uint32_t* values, uint32_t values_stride, const uint8_t* text, uint32_t text_stride,
              uint8_t* out_text, uint32_t out_stride, uint32_t* out) {
    RtProgram* p = (RtProgram*)h;
    if (!p || values_stride < p->n_slots || out_stride == 0 || out_stride % 16u) return AUTHJX_EINVAL;
    uint32_t levels[kMaxRenderDepth * kRenderLevelWords];
    const RenderStack st{levels, 1};
    for (uint32_t r = 0; r < n; r++) {
        std::vector<uint8_t> doc(arena + offs[r], arena + offs[r] + lens[r]);
        std::vector<uint8_t> txt;
        if (text) txt.assign(text + (size_t)r * text_stride, text + (size_t)(r + 1) * text_stride);
        uint8_t* slot = (uint8_t*)std::aligned_alloc(16, out_stride);
        std::memcpy(slot, out_text + (size_t)r * out_stride, out_stride);
        std::vector<uint32_t> vals(values + (size_t)r * values_stride * 3, values + (size_t)(r + 1) * values_stride * 3);
        std::vector<uint32_t> res(3 * (size_t)p->n_outputs + 1);
        render_request(p->blob.data(), doc.data(), lens[r], vals.data(), text ? txt.data() : nullptr, text_stride,
                       slot, out_stride, res.data(), st);
        std::memcpy(out_text + (size_t)r * out_stride, slot, out_stride);
        std::memcpy(out + (size_t)r * p->n_outputs * 3, res.data(), 12 * (size_t)p->n_outputs);
        std::free(slot);
    }
    return AUTHJX_OK;
}

}  // extern "C"
