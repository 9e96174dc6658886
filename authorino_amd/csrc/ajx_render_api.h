// ajx_render_api.h — private: what the render entry points (ajx_render_api.cpp, a
// translation unit of its own) need from the rest of the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/authjx.h"
#include "ajx_hostbuf.h"

// a render program resident in device memory (authjx_render_compile)
struct authjx_render {
    int device = 0;
    ajx::DeviceBuf d_prog;
    uint32_t n_outputs = 0, n_slots = 0;
};

// the gates of a render program (authjx_gates_compile): the blob on the device for the gated
// kernel and on the host for authjx_verdict_of
struct authjx_gates {
    int device = 0;
    ajx::DeviceBuf d_blob;
    std::vector<uint8_t> blob;
    uint32_t n_outputs = 0, n_trees = 0;
};

// the context's device and its own stream (ajx_api.cpp)
int ajx_ctx_device(const authjx_ctx* ctx);
hipStream_t ajx_ctx_stream(const authjx_ctx* ctx);

namespace ajx {

// The render kernel (ajx_render.hip): request r renders the program's outputs from
// values[r * values_stride ...] into out_text[r * out_stride ...] and writes n_outputs
// records {start, len, status} at out[r * n_outputs ...]. text: the requests' text slots or
// nullptr. out_text 16-byte aligned, out_stride a multiple of 16.
hipError_t launch_render(const uint8_t* d_prog, uint32_t n_outputs, const uint8_t* arena, const uint64_t* offs,
                         const uint32_t* lens, uint32_t n, const uint32_t* values, uint32_t values_stride,
                         const uint8_t* text, uint32_t text_stride, uint8_t* out_text, uint32_t out_stride,
                         uint32_t* out, hipStream_t stream);

// The same kernel's multi-program instance: request r renders d_progs[prog_of_req[r]]
// (prog_of_req nullptr: d_progs[0]) and writes that program's records at
// out[r * records_stride ...]; an entry that is not below n_progs (0xFFFFFFFF: "no program")
// reads and writes nothing. d_progs: a device table of n_progs program blobs.
hipError_t launch_render_multi(const uint8_t* const* d_progs, uint32_t n_progs, const uint32_t* prog_of_req,
                               const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                               const uint32_t* values, uint32_t values_stride, const uint8_t* text,
                               uint32_t text_stride, uint8_t* out_text, uint32_t out_stride, uint32_t* out,
                               uint32_t records_stride, hipStream_t stream);

// The gated kernel: d_tables holds the n_progs program blobs, then their n_progs gates
// blobs (nullptr: ungated). tri: u8 tri-states, row (tri_of_req ? tri_of_req[r] : r) of
// tri_stride bytes for request r; verdicts: two words per request or nullptr.
hipError_t launch_render_gated(const uint8_t* const* d_tables, uint32_t n_progs, const uint32_t* prog_of_req,
                               const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                               const uint32_t* values, uint32_t values_stride, const uint8_t* text,
                               uint32_t text_stride, uint8_t* out_text, uint32_t out_stride, uint32_t* out,
                               uint32_t records_stride, const uint8_t* tri, uint32_t tri_stride,
                               const uint32_t* tri_of_req, uint32_t* verdicts, hipStream_t stream);

}  // namespace ajx
