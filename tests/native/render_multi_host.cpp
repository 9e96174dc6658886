// render_multi_host.cpp — TEST-ONLY host build of the multi-program render kernel's
// per-request body (render_request_multi, authorino_amd/csrc/ajx_render.h) on top of
// render_host.cpp's program builder and one-program call, for tests/test_render_multi_host.py
// and san_render_multi. Not part of libauthjx.so.
#include "render_host.cpp"

extern "C" {

// authjx_render_batch_multi_device on the CPU: request r renders progs[prog_of_req[r]]
// (prog_of_req nullptr: progs[0]) over exact-size heap copies of its document, values, text
// slot, output slot and its program's records, so that a sanitizer build sees any access
// outside them. A request whose entry is not below n_progs gets no buffer at all (null
// pointers): whatever the body read or wrote for it would fault.
int rtm_render(void* const* progs, uint32_t n_progs, const uint32_t* prog_of_req, const uint8_t* arena,
               const uint64_t* offs, const uint32_t* lens, uint32_t n, const uint32_t* values,
               uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
               uint32_t out_stride, uint32_t* out, uint32_t records_stride) {
    if (!progs || n_progs == 0 || out_stride == 0 || out_stride % 16u || (n_progs > 1 && !prog_of_req))
        return AUTHJX_EINVAL;
    std::vector<const uint8_t*> blobs(n_progs);
    for (uint32_t i = 0; i < n_progs; i++) {
        const RtProgram* p = (const RtProgram*)progs[i];
        if (!p || values_stride < p->n_slots || records_stride < p->n_outputs) return AUTHJX_EINVAL;
        blobs[i] = p->blob.data();
    }
    uint32_t levels[kMaxRenderDepth * kRenderLevelWords];
    const RenderStack st{levels, 1};
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t pi = prog_of_req ? prog_of_req[r] : 0u;
        if (pi >= n_progs) {
            render_request_multi(blobs.data(), n_progs, pi, nullptr, lens[r], nullptr, nullptr, text_stride, nullptr,
                                 out_stride, nullptr, st);
            continue;
        }
        const RtProgram* p = (const RtProgram*)progs[pi];
        std::vector<uint8_t> doc(arena + offs[r], arena + offs[r] + lens[r]);
        std::vector<uint8_t> txt;
        if (text) txt.assign(text + (size_t)r * text_stride, text + (size_t)(r + 1) * text_stride);
        uint8_t* slot = (uint8_t*)std::aligned_alloc(16, out_stride);
        std::memcpy(slot, out_text + (size_t)r * out_stride, out_stride);
        const uint32_t* v0 = values + (size_t)r * values_stride * 3;
        std::vector<uint32_t> vals(v0, v0 + (size_t)p->n_slots * 3);
        std::vector<uint32_t> res(3 * (size_t)p->n_outputs);
        render_request_multi(blobs.data(), n_progs, pi, doc.data(), lens[r], vals.data(), text ? txt.data() : nullptr,
                             text_stride, slot, out_stride, res.data(), st);
        std::memcpy(out_text + (size_t)r * out_stride, slot, out_stride);
        if (!res.empty()) std::memcpy(out + (size_t)r * records_stride * 3, res.data(), 4 * res.size());
        std::free(slot);
    }
    return AUTHJX_OK;
}

}  // extern "C"
