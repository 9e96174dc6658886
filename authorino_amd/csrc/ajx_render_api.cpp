// ajx_render_api.cpp — the render entry points of the C-ABI (include/authjx.h): render
// programs resident in HBM and the batch calls that run them (ajx_render.hip). A
// translation unit of its own: ajx_api.cpp does not reference it.
#include <cstdio>
#include <string>

#include "ajx_host.h"
#include "ajx_render_api.h"
#include "ajx_render_prog.h"

static_assert(sizeof(authjx_rendered) == 12, "authjx_rendered is three u32 words on the device");

int authjx_render_compile(authjx_ctx* ctx, const authjx_render_output* outs, uint32_t n_outputs, uint32_t n_slots,
                          authjx_render** out, char* errbuf, size_t errcap) {
    if (errbuf && errcap) errbuf[0] = 0;
    if (!ctx || !out) return AUTHJX_EINVAL;
    *out = nullptr;
    std::vector<uint8_t> blob;
    std::string err;
    const int rc = ajx::build_render_program(outs, n_outputs, n_slots, &blob, &err);
    if (rc != AUTHJX_OK) {
        if (errbuf && errcap) std::snprintf(errbuf, errcap, "%s", err.c_str());
        return rc;
    }
    authjx_render* p = new authjx_render();
    p->device = ctx->device;
    p->n_outputs = n_outputs;
    p->n_slots = n_slots;
    if (hipSetDevice(p->device) != hipSuccess || p->d_prog.reserve(blob.size()) != hipSuccess ||
        hipMemcpy(p->d_prog.data(), blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        return AUTHJX_EDEVICE;
    }
    *out = p;
    return AUTHJX_OK;
}

void authjx_render_free(authjx_render* prog) {
    if (!prog) return;
    if (prog->d_prog.data()) (void)hipSetDevice(prog->device);
    delete prog;  // (freeing the program waits for the kernels that read it)
}

uint32_t authjx_render_outputs(const authjx_render* prog) { return prog ? prog->n_outputs : 0u; }

int authjx_render_batch_device(authjx_ctx* ctx, const authjx_render* prog, const uint8_t* d_arena,
                               const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n,
                               const authjx_value* d_values, uint32_t values_stride, const uint8_t* d_text,
                               uint32_t text_stride, uint8_t* d_out_text, uint32_t out_stride,
                               authjx_rendered* d_out, void* stream) {
    if (!ctx || !prog) return AUTHJX_EINVAL;
    if (values_stride < prog->n_slots || out_stride == 0 || out_stride % 16u != 0) return AUTHJX_EINVAL;
    if (n && (!d_arena || !d_offs || !d_lens || !d_out_text || !d_out || (prog->n_slots && !d_values)))
        return AUTHJX_EINVAL;
    if (((uintptr_t)d_out_text & 15u) != 0 || prog->device != ctx->device) return AUTHJX_EINVAL;
    HIP_OK(hipSetDevice(prog->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    HIP_OK(ajx::launch_render(prog->d_prog.data(), prog->n_outputs, d_arena, d_offs, d_lens, n,
                              reinterpret_cast<const uint32_t*>(d_values), values_stride, d_text, text_stride,
                              d_out_text, out_stride, reinterpret_cast<uint32_t*>(d_out), s));
    return AUTHJX_OK;
}

int authjx_render_batch_multi_device(authjx_ctx* ctx, const authjx_render* const* progs, uint32_t n_progs,
                                     const uint32_t* d_prog_of_req, const uint8_t* d_arena, const uint64_t* d_offs,
                                     const uint32_t* d_lens, uint32_t n, const authjx_value* d_values,
                                     uint32_t values_stride, const uint8_t* d_text, uint32_t text_stride,
                                     uint8_t* d_out_text, uint32_t out_stride, authjx_rendered* d_out,
                                     uint32_t records_stride, void* stream) {
    if (!ctx || !progs || n_progs == 0) return AUTHJX_EINVAL;
    if (out_stride == 0 || out_stride % 16u != 0 || (n_progs > 1 && !d_prog_of_req)) return AUTHJX_EINVAL;
    std::vector<const uint8_t*> blobs(n_progs);
    uint32_t slots = 0;
    for (uint32_t i = 0; i < n_progs; i++) {
        const authjx_render* p = progs[i];
        if (!p || p->device != ctx->device || values_stride < p->n_slots || records_stride < p->n_outputs)
            return AUTHJX_EINVAL;
        blobs[i] = p->d_prog.data();
        slots = std::max(slots, p->n_slots);
    }
    if (n && (!d_arena || !d_offs || !d_lens || !d_out_text || !d_out || (slots && !d_values)))
        return AUTHJX_EINVAL;
    if (((uintptr_t)d_out_text & 15u) != 0) return AUTHJX_EINVAL;
    if (n == 0) return AUTHJX_OK;
    return with_ptr_table(ctx, stream, blobs.data(), n_progs, [&](const uint8_t* const* d_progs, hipStream_t s) {
        return ajx::launch_render_multi(d_progs, n_progs, d_prog_of_req, d_arena, d_offs, d_lens, n,
                                        reinterpret_cast<const uint32_t*>(d_values), values_stride, d_text,
                                        text_stride, d_out_text, out_stride, reinterpret_cast<uint32_t*>(d_out),
                                        records_stride, s);
    });
}

int authjx_render_batch(authjx_ctx* ctx, const authjx_render* prog, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* offs, const uint32_t* lens, uint32_t n, const authjx_value* values,
                        uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
                        uint32_t out_stride, authjx_rendered* out) {
    if (!ctx || !prog) return AUTHJX_EINVAL;
    if (values_stride < prog->n_slots || out_stride == 0 || out_stride % 16u != 0) return AUTHJX_EINVAL;
    if (n == 0) return AUTHJX_OK;
    if (!arena || !offs || !lens || !out_text || !out || (prog->n_slots && !values)) return AUTHJX_EINVAL;
    if (!ajx::spans_in_arena(offs, lens, n, arena_len)) return AUTHJX_EINVAL;
    const size_t val_bytes = (size_t)n * values_stride * sizeof(authjx_value);
    const size_t text_bytes = text ? (size_t)n * text_stride : 0;
    const size_t outt_bytes = (size_t)n * out_stride, out_bytes = (size_t)n * prog->n_outputs * sizeof(authjx_rendered);
    ajx::StageLayout lay;
    lay.add(arena_len);  // (the arena at 0)
    const size_t o_offs = lay.add((size_t)n * 8), o_lens = lay.add((size_t)n * 4);
    const size_t o_val = lay.add(val_bytes), o_text = lay.add(text_bytes);
    const size_t o_outt = lay.add(outt_bytes), o_out = lay.add(out_bytes);
    HIP_OK(hipSetDevice(prog->device));
    ajx::DeviceBuf buf;  // (a buffer per call: freed on every return)
    HIP_OK(buf.reserve(lay.total() + 256));
    uint8_t* b = buf.data();
    hipStream_t s = ctx->stream;
    if (arena_len) HIP_OK(hipMemcpyAsync(b, arena, arena_len, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(b + o_offs, offs, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(b + o_lens, lens, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (val_bytes) HIP_OK(hipMemcpyAsync(b + o_val, values, val_bytes, hipMemcpyHostToDevice, s));
    if (text_bytes) HIP_OK(hipMemcpyAsync(b + o_text, text, text_bytes, hipMemcpyHostToDevice, s));
    // (the slots' unspecified bytes come back as the caller's own: the host copy keeps them)
    HIP_OK(hipMemcpyAsync(b + o_outt, out_text, outt_bytes, hipMemcpyHostToDevice, s));
    const int rc = authjx_render_batch_device(
        ctx, prog, b, (const uint64_t*)(b + o_offs), (const uint32_t*)(b + o_lens), n,
        (const authjx_value*)(b + o_val), values_stride, text ? b + o_text : nullptr, text_stride, b + o_outt,
        out_stride, (authjx_rendered*)(b + o_out), s);
    if (rc != AUTHJX_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    HIP_OK(hipMemcpyAsync(out_text, b + o_outt, outt_bytes, hipMemcpyDeviceToHost, s));
    if (out_bytes) HIP_OK(hipMemcpyAsync(out, b + o_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return AUTHJX_OK;
}
