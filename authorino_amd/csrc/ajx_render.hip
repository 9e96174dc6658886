// ajx_render.hip — the render kernel: selected values -> final response header bytes
// (ajx_render.h). One work-item per request, in request order, 256-thread workgroups; the
// container walk's level stack lives in LDS (kMaxRenderDepth levels of three words per
// lane, 24 KiB per workgroup), never in a runtime-indexed register array.
#include <hip/hip_runtime.h>

#include "ajx_render.h"
#include "ajx_render_api.h"
#include "ajx_render_gated.h"

namespace ajx {

constexpr uint32_t kRenderBlock = 256;

__global__ __launch_bounds__(256) void ajx_render_values(const uint8_t* __restrict__ prog,
                                                         const uint8_t* __restrict__ arena,
                                                         const uint64_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ lens, uint32_t n,
                                                         const uint32_t* __restrict__ values, uint32_t values_stride,
                                                         const uint8_t* __restrict__ text, uint32_t text_stride,
                                                         uint8_t* __restrict__ out_text, uint32_t out_stride,
                                                         uint32_t* __restrict__ out, uint32_t n_outputs) {
    __shared__ uint32_t levels[kMaxRenderDepth * kRenderLevelWords * kRenderBlock];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const RenderStack st{levels + threadIdx.x, kRenderBlock};
    render_request(prog, arena + offs[r], lens[r], values + (size_t)r * values_stride * 3u,
                   text ? text + (size_t)r * text_stride : nullptr, text_stride, out_text + (size_t)r * out_stride,
                   out_stride, out + (size_t)r * n_outputs * 3u, st);
}

// The multi-program instance: request r renders progs[prog_of_req[r]] (prog_of_req nullptr:
// progs[0]) and writes that program's records at out[r * records_stride ...]. A kernel of
// its own: the one above keeps its program pointer as a kernel argument and its code.
__global__ __launch_bounds__(256) void ajx_render_values_multi(
    const uint8_t* const* __restrict__ progs, uint32_t n_progs, const uint32_t* __restrict__ prog_of_req,
    const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs, const uint32_t* __restrict__ lens, uint32_t n,
    const uint32_t* __restrict__ values, uint32_t values_stride, const uint8_t* __restrict__ text, uint32_t text_stride,
    uint8_t* __restrict__ out_text, uint32_t out_stride, uint32_t* __restrict__ out, uint32_t records_stride) {
    __shared__ uint32_t levels[kMaxRenderDepth * kRenderLevelWords * kRenderBlock];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const RenderStack st{levels + threadIdx.x, kRenderBlock};
    render_request_multi(progs, n_progs, prog_of_req ? prog_of_req[r] : 0u, arena + offs[r], lens[r],
                         values + (size_t)r * values_stride * 3u, text ? text + (size_t)r * text_stride : nullptr,
                         text_stride, out_text + (size_t)r * out_stride, out_stride,
                         out + (size_t)r * records_stride * 3u, st);
}

// The gated instance: the multi-program kernel with a table of gates beside the programs
// (tables[n_progs + i] = the gates of program i, or nullptr). Each lane folds its request's
// tri-states tri[(tri_of_req ? tri_of_req[r] : r) * tri_stride ...] into a verdict
// (ajx_verdict.h: registers only) and asks it about each output before that output's first
// op is read: a lane whose output does not apply waits for its wave, and loads nothing but
// the gate's own {on, when} pair and tri-state byte: no op, no value, no source byte.
// verdicts: two words {verdict, denied_by} per request, or nullptr.
__global__ __launch_bounds__(256) void ajx_render_values_gated(
    const uint8_t* const* __restrict__ tables, uint32_t n_progs, const uint32_t* __restrict__ prog_of_req,
    const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs, const uint32_t* __restrict__ lens, uint32_t n,
    const uint32_t* __restrict__ values, uint32_t values_stride, const uint8_t* __restrict__ text, uint32_t text_stride,
    uint8_t* __restrict__ out_text, uint32_t out_stride, uint32_t* __restrict__ out, uint32_t records_stride,
    const uint8_t* __restrict__ tri, uint32_t tri_stride, const uint32_t* __restrict__ tri_of_req,
    uint32_t* __restrict__ verdicts) {
    __shared__ uint32_t levels[kMaxRenderDepth * kRenderLevelWords * kRenderBlock];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const RenderStack st{levels + threadIdx.x, kRenderBlock};
    const uint32_t row = tri_of_req ? tri_of_req[r] : r;
    render_request_gated(tables, tables + n_progs, n_progs, prog_of_req ? prog_of_req[r] : 0u,
                         tri ? tri + (size_t)row * tri_stride : nullptr, arena + offs[r], lens[r],
                         values + (size_t)r * values_stride * 3u, text ? text + (size_t)r * text_stride : nullptr,
                         text_stride, out_text + (size_t)r * out_stride, out_stride,
                         out + (size_t)r * records_stride * 3u, verdicts ? verdicts + (size_t)r * 2u : nullptr, st);
}

hipError_t launch_render_gated(const uint8_t* const* d_tables, uint32_t n_progs, const uint32_t* prog_of_req,
                               const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                               const uint32_t* values, uint32_t values_stride, const uint8_t* text,
                               uint32_t text_stride, uint8_t* out_text, uint32_t out_stride, uint32_t* out,
                               uint32_t records_stride, const uint8_t* tri, uint32_t tri_stride,
                               const uint32_t* tri_of_req, uint32_t* verdicts, hipStream_t stream) {
    if (n == 0 || n_progs == 0) return hipSuccess;
    const uint32_t grid = (n + kRenderBlock - 1) / kRenderBlock;
    hipLaunchKernelGGL(ajx_render_values_gated, dim3(grid), dim3(kRenderBlock), 0, stream, d_tables, n_progs,
                       prog_of_req, arena, offs, lens, n, values, values_stride, text, text_stride, out_text,
                       out_stride, out, records_stride, tri, tri_stride, tri_of_req, verdicts);
    return hipGetLastError();
}

hipError_t launch_render_multi(const uint8_t* const* d_progs, uint32_t n_progs, const uint32_t* prog_of_req,
                               const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                               const uint32_t* values, uint32_t values_stride, const uint8_t* text,
                               uint32_t text_stride, uint8_t* out_text, uint32_t out_stride, uint32_t* out,
                               uint32_t records_stride, hipStream_t stream) {
    if (n == 0 || n_progs == 0) return hipSuccess;
    const uint32_t grid = (n + kRenderBlock - 1) / kRenderBlock;
    hipLaunchKernelGGL(ajx_render_values_multi, dim3(grid), dim3(kRenderBlock), 0, stream, d_progs, n_progs,
                       prog_of_req, arena, offs, lens, n, values, values_stride, text, text_stride, out_text,
                       out_stride, out, records_stride);
    return hipGetLastError();
}

hipError_t launch_render(const uint8_t* d_prog, uint32_t n_outputs, const uint8_t* arena, const uint64_t* offs,
                         const uint32_t* lens, uint32_t n, const uint32_t* values, uint32_t values_stride,
                         const uint8_t* text, uint32_t text_stride, uint8_t* out_text, uint32_t out_stride,
                         uint32_t* out, hipStream_t stream) {
    if (n == 0 || n_outputs == 0) return hipSuccess;
    const uint32_t grid = (n + kRenderBlock - 1) / kRenderBlock;
    hipLaunchKernelGGL(ajx_render_values, dim3(grid), dim3(kRenderBlock), 0, stream, d_prog, arena, offs, lens, n,
                       values, values_stride, text, text_stride, out_text, out_stride, out, n_outputs);
    return hipGetLastError();
}

}  // namespace ajx
