// ajx_host.h — private: what the C-ABI's translation units (ajx_api.cpp, ajx_batcher_api.cpp,
// ajx_render_api.cpp) share: the context, the ruleset, the HIP error check, the staging
// layout and the span check of the host-buffer entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/authjx.h"
#include "ajx_compiler.h"
#include "ajx_hostbuf.h"
#include "ajx_plan.h"

struct authjx_ruleset {
    int device = 0;
    ajx::DeviceBuf d_blob;
    ajx::CompiledRuleset c;
    // what the choice of kernels reads of the blob (ajx_plan.h PlanIn), set once by the compile
    bool stream_ok = false;   // the streaming kernel takes it (ajx::stream_eligible)
    uint32_t stream_rec = 0;  // its capture records there (ajx::stream_records)
    bool mods = false;        // modifier chains or text buffers: the exact scan's instance with buffers
    uint32_t lean_feat = 0, hdr_trees = 0;  // RulesetHdr lean_feat, pad1[0] (0: no forest)
    uint32_t blob_bytes = 0;
    // workspaces (by registry id) whose stream has run a batch over this ruleset:
    // authjx_free waits for their last batch instead of the whole device
    std::mutex mu;
    std::vector<uint64_t> users;
    void note_use(uint64_t ws_id) {
        std::lock_guard<std::mutex> lock(mu);
        if (std::find(users.begin(), users.end(), ws_id) == users.end()) users.push_back(ws_id);
    }
};

struct Workspace;  // per-stream scratch (ajx_api.cpp)

struct authjx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // the context's own stream (host-buffer entry points)
    std::mutex mu;                 // workspace list and settings
    std::mutex batch_mu;           // serialises the host-buffer entry points (staging buffer)
    std::vector<Workspace*> ws;
    Workspace* last_ws = nullptr;  // of the last device call (last_kernel_ms / last_exact_count)
    std::vector<authjx_batcher*> batchers;  // alive on this context (shutdown destroys them first)
    ajx::DeviceBuf stage;  // staging for the host-buffer entry points (batch_mu)
    int len_sort = 1;         // order requests by length class before the single-pass kernel
    int no_tenant_stage = 0;  // profiling: multi-tenant batches read tables from global memory
    int force_scan = 0;
    // batches of up to this many requests go to the streaming kernel (latency: several
    // waves per document span), larger ones to the lean / multi-tenant kernels
    uint32_t stream_max_n = 4096;
    int mode = ajx::kModeDefault;  // profiling / comparison only: an ajx::KernelMode (ajx_plan.h)
};

// the last HIP error an entry point returned AUTHJX_EDEVICE for, on this thread, and where
// it was seen (authjx_debug_last_error); the runtime's own last-error slot is cleared, so
// the caller's next HIP call does not report it again
struct AjxLastError {
    hipError_t err = hipSuccess;
    const char* file = "";
    int line = 0;
};
extern thread_local AjxLastError ajx_last_error;

#define HIP_OK(x)                                        \
    do {                                                 \
        hipError_t e_ = (x);                             \
        if (e_ != hipSuccess) {                          \
            ajx_last_error = {e_, __FILE__, __LINE__};   \
            (void)hipGetLastError();                     \
            return AUTHJX_EDEVICE;                       \
        }                                                \
    } while (0)

// authjx_eval_batch_device; d_sets_pre: the blob pointers already on the device (the
// micro-batcher's one staging copy), else this stream's table is filled from sets
int eval_device(authjx_ctx* ctx, const authjx_ruleset* const* sets, uint32_t n_sets, const uint32_t* d_set_of_req,
                const uint8_t* d_arena, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n,
                uint8_t* d_out_tristate, int32_t* d_out_err_idx, uint64_t* d_out_bitmap, uint32_t bitmap_stride_words,
                void* stream, const uint8_t* const* d_sets_pre);

// Queues launch(table, s) on `stream` (NULL: the context's), `table` being ptrs[0, n), n > 0,
// as a device table of that stream's workspace, uploaded on the stream when it differs from
// the last call's. AUTHJX_EDEVICE when an upload or the launch fails.
int with_ptr_table(authjx_ctx* ctx, void* stream, const uint8_t* const* ptrs, uint32_t n,
                   const std::function<hipError_t(const uint8_t* const*, hipStream_t)>& launch);

// retires the workspace of stream s (the caller holds no lock)
void retire_stream(authjx_ctx* ctx, hipStream_t s);

namespace ajx {

// A staging buffer's parts, each at a multiple of 256 bytes: add() answers the part's offset,
// total() the bytes to allocate.
struct StageLayout {
    size_t end = 0;
    size_t add(size_t bytes) {
        const size_t at = end;
        end = (at + bytes + 255u) & ~(size_t)255u;
        return at;
    }
    size_t total() const { return end; }
};

// A table of device pointers that kernels index, kept per stream: two slots (device + pinned
// source each), so a call with another list fills the slot the call before the last one
// used; that call's event, not a stream synchronize, guards the reuse.
struct PtrTable {
    DeviceBuf dev;
    PinnedBuf host;
    uint32_t cap = 0;  // entries per slot
    uint32_t slot = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool rec[2] = {false, false};
    std::vector<const uint8_t*> last;  // the current slot's entries (empty: none uploaded)
};

// every request's span lies in the arena (written so that offs + lens cannot wrap)
inline bool spans_in_arena(const uint64_t* offs, const uint32_t* lens, uint32_t n, uint64_t arena_len) {
    for (uint32_t r = 0; r < n; r++)
        if (offs[r] > arena_len || lens[r] > arena_len - offs[r]) return false;
    return true;
}

}  // namespace ajx
