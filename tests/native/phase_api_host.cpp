// phase_api_host.cpp — TEST-ONLY: a stand-alone ASan + UBSan driver (phase_api.mk) for the
// phase object and the batcher's phase staging (authorino_amd/csrc/ajx_phase_api.cpp,
// ajx_batcher_api.cpp, ajx_render_api.cpp) on the host stand-in of the HIP runtime
// (hipstub/, hip_stub.cpp: its hipMalloc is an exact-size calloc, so an undersized staging
// part is a report; its select writes every value as a missing path). The render launches
// are stand-ins here that run the kernels' per-request bodies (ajx_render.h) on the host, so
// a packed batch comes back with real records and bytes. It runs authjx_phase_create's
// argument table, batches of phase requests of two phases with different strides next to
// eval-only requests from 6 threads (zero-copy on and off), a deadline that expires, and
// authjx_shutdown with a batcher alive. Prints "ok ..." when every check held.
#define AJX_HD inline
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../authorino_amd/csrc/ajx_render.h"
#include "../../authorino_amd/csrc/ajx_render_api.h"

extern "C" int authjx_debug_batcher_modes(uint32_t wake, uint32_t sync, uint32_t zcopy);

namespace ajx {

hipError_t launch_render(const uint8_t* d_prog, uint32_t n_outputs, const uint8_t* arena, const uint64_t* offs,
                         const uint32_t* lens, uint32_t n, const uint32_t* values, uint32_t values_stride,
                         const uint8_t* text, uint32_t text_stride, uint8_t* out_text, uint32_t out_stride,
                         uint32_t* out, hipStream_t) {
    uint32_t levels[kMaxRenderDepth * kRenderLevelWords];
    const RenderStack st{levels, 1};
    for (uint32_t r = 0; r < n; r++)
        render_request(d_prog, arena + offs[r], lens[r], values + (size_t)r * values_stride * 3u,
                       text ? text + (size_t)r * text_stride : nullptr, text_stride,
                       out_text + (size_t)r * out_stride, out_stride, out + (size_t)r * n_outputs * 3u, st);
    return hipSuccess;
}

hipError_t launch_render_multi(const uint8_t* const* d_progs, uint32_t n_progs, const uint32_t* prog_of_req,
                               const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                               const uint32_t* values, uint32_t values_stride, const uint8_t* text,
                               uint32_t text_stride, uint8_t* out_text, uint32_t out_stride, uint32_t* out,
                               uint32_t records_stride, hipStream_t) {
    uint32_t levels[kMaxRenderDepth * kRenderLevelWords];
    const RenderStack st{levels, 1};
    for (uint32_t r = 0; r < n; r++)
        render_request_multi(d_progs, n_progs, prog_of_req ? prog_of_req[r] : 0u, arena + offs[r], lens[r],
                             values + (size_t)r * values_stride * 3u, text ? text + (size_t)r * text_stride : nullptr,
                             text_stride, out_text + (size_t)r * out_stride, out_stride,
                             out + (size_t)r * records_stride * 3u, st);
    return hipSuccess;
}

}  // namespace ajx

namespace {

std::atomic<int> g_fail{0}, g_checks{0};
#define CHECK(c)                                                      \
    do {                                                              \
        g_checks++;                                                   \
        if (!(c)) {                                                   \
            g_fail++;                                                 \
            std::fprintf(stdout, "FAIL line %d: %s\n", __LINE__, #c); \
        }                                                             \
    } while (0)

authjx_ruleset* compile_rules(authjx_ctx* ctx, const char* val) {
    authjx_pattern p{"a", 1, AUTHJX_OP_EQ, val, (uint32_t)std::strlen(val)};
    authjx_node nd{AUTHJX_NODE_PATTERN, -1, -1, 0};
    authjx_tree t{&p, 1, &nd, 1, 0};
    authjx_ruleset* rs = nullptr;
    return authjx_compile(ctx, &t, &rs, nullptr, nullptr, 0) == AUTHJX_OK ? rs : nullptr;
}

authjx_ruleset* compile_selectors(authjx_ctx* ctx, uint32_t n) {
    authjx_pattern sel[3] = {{"a", 1, AUTHJX_OP_EQ, "", 0}, {"b", 1, AUTHJX_OP_EQ, "", 0}, {"c", 1, AUTHJX_OP_EQ, "", 0}};
    authjx_tree t{sel, n, nullptr, 0, -1};
    authjx_ruleset* rs = nullptr;
    return authjx_compile(ctx, &t, &rs, nullptr, nullptr, 0) == AUTHJX_OK ? rs : nullptr;
}

// outputs: LIT(lit), SPRINT(slot 0) -> "<nil>" of the stand-in's missing values, LIT(lit) STRING(slot 1)
authjx_render* compile_program(authjx_ctx* ctx, const char* lit, uint32_t n_slots) {
    const uint32_t len = (uint32_t)std::strlen(lit);
    authjx_render_op o0[1] = {{AUTHJX_R_LIT, 0, (const uint8_t*)lit, len}};
    authjx_render_op o1[1] = {{AUTHJX_R_SPRINT, 0, nullptr, 0}};
    authjx_render_op o2[2] = {{AUTHJX_R_LIT, 0, (const uint8_t*)lit, len}, {AUTHJX_R_STRING, 1, nullptr, 0}};
    authjx_render_output outs[3] = {{o0, 1}, {o1, 1}, {o2, 2}};
    authjx_render* p = nullptr;
    return authjx_render_compile(ctx, outs, 3, n_slots, &p, nullptr, 0) == AUTHJX_OK ? p : nullptr;
}

// one phase request: its records and bytes are the program's over missing values, the
// buffers' bytes past them the caller's guard
void phase_call(authjx_batcher* b, const authjx_phase* ph, const char* lit, uint32_t out_stride, uint32_t i) {
    const std::string doc = "{\"a\":" + std::to_string(i) + ",\"b\":\"y\"}";
    std::vector<uint8_t> text(out_stride, 0xA5);
    authjx_rendered rec[4];
    std::memset(rec, 0xA5, sizeof rec);
    uint8_t tri = 0xA5;
    int32_t err = 7;
    const int rc = authjx_batcher_phase(b, ph, (const uint8_t*)doc.data(), doc.size(), 0, &tri, &err, text.data(), rec);
    CHECK(rc == AUTHJX_OK && tri == 1 && err == -1);
    const std::string l(lit), want = l + "<nil>" + l;
    if (want.size() <= out_stride) {
        CHECK(rec[0].start == 0 && rec[0].len == l.size() && rec[0].status == AUTHJX_RENDER_OK);
        CHECK(rec[1].start == l.size() && rec[1].len == 5 && rec[1].status == AUTHJX_RENDER_OK);
        CHECK(rec[2].start == l.size() + 5 && rec[2].len == l.size() && rec[2].status == AUTHJX_RENDER_OK);
        CHECK(std::memcmp(text.data(), want.data(), want.size()) == 0);
        for (size_t k = want.size(); k < out_stride; k++) CHECK(text[k] == 0xA5);
    } else {  // (out_stride 16: the literal and "<nil>" fit, the third output does not)
        CHECK(rec[0].status == AUTHJX_RENDER_OK && rec[1].status == AUTHJX_RENDER_OK);
        CHECK(rec[2].status == AUTHJX_RENDER_UNRENDERED && rec[2].len == 0);
        CHECK(std::memcmp(text.data(), want.data(), l.size() + 5) == 0);
        for (size_t k = l.size() + 5; k < out_stride; k++) CHECK(text[k] == 0xA5);
    }
    const uint8_t* tail = reinterpret_cast<const uint8_t*>(&rec[3]);
    for (size_t k = 0; k < sizeof rec[3]; k++) CHECK(tail[k] == 0xA5);
}

}  // namespace

int main() {
    authjx_ctx* ctx = nullptr;
    CHECK(authjx_init(0, &ctx) == AUTHJX_OK);
    authjx_ruleset *r1 = compile_rules(ctx, "1"), *r2 = compile_rules(ctx, "2");
    authjx_ruleset *s3 = compile_selectors(ctx, 3), *s1 = compile_selectors(ctx, 1);
    authjx_render *pa = compile_program(ctx, "hello ", 2), *pb = compile_program(ctx, "0123456789", 3);
    CHECK(r1 && r2 && s3 && s1 && pa && pb);

    // authjx_phase_create's argument table
    authjx_phase* ph = nullptr;
    CHECK(authjx_phase_create(nullptr, r1, s3, pa, 64, 64, &ph) == AUTHJX_EINVAL && !ph);
    CHECK(authjx_phase_create(ctx, nullptr, s3, pa, 64, 64, &ph) == AUTHJX_EINVAL);
    CHECK(authjx_phase_create(ctx, r1, nullptr, pa, 64, 64, &ph) == AUTHJX_EINVAL);
    CHECK(authjx_phase_create(ctx, r1, s3, nullptr, 64, 64, &ph) == AUTHJX_EINVAL);
    CHECK(authjx_phase_create(ctx, r1, s3, pa, 64, 64, nullptr) == AUTHJX_EINVAL);
    CHECK(authjx_phase_create(ctx, r1, s1, pa, 64, 64, &ph) == AUTHJX_EINVAL);  // 1 pattern, 2 slots
    authjx_ruleset* s0 = compile_selectors(ctx, 0);  // (a nil expression: no pattern to select)
    CHECK(s0 && authjx_phase_create(ctx, r1, s0, pa, 64, 64, &ph) == AUTHJX_EINVAL);
    CHECK(authjx_phase_create(ctx, r1, s3, pa, 64, 0, &ph) == AUTHJX_EINVAL);
    CHECK(authjx_phase_create(ctx, r1, s3, pa, 64, 40, &ph) == AUTHJX_EINVAL);
    CHECK(authjx_phase_create(ctx, r1, s3, pa, 64, 65552, &ph) == AUTHJX_ELIMIT);
    CHECK(authjx_phase_create(ctx, r1, s3, pa, 65537, 64, &ph) == AUTHJX_ELIMIT && !ph);
    CHECK(authjx_phase_outputs(nullptr) == 0);
    authjx_phase_free(nullptr);
    authjx_phase *pha = nullptr, *phb = nullptr;
    CHECK(authjx_phase_create(ctx, r1, s3, pa, 0, 64, &pha) == AUTHJX_OK && authjx_phase_outputs(pha) == 3);
    CHECK(authjx_phase_create(ctx, r2, s3, pb, 128, 16, &phb) == AUTHJX_OK);

    for (uint32_t zcopy = 0; zcopy < 2; zcopy++) {
        CHECK(authjx_debug_batcher_modes(0, 0, zcopy) == AUTHJX_OK);
        authjx_batcher* b = nullptr;
        CHECK(authjx_batcher_create(ctx, 16, 2000, 0, &b) == AUTHJX_OK);
        std::vector<std::thread> ts;
        for (uint32_t t = 0; t < 6; t++)
            ts.emplace_back([&, t] {
                for (uint32_t i = 0; i < 20; i++) {
                    const uint32_t kind = (t * 5 + i * 3 + i / 7) % 3;
                    if (kind == 0) phase_call(b, pha, "hello ", 64, t * 100 + i);
                    else if (kind == 1) phase_call(b, phb, "0123456789", 16, t * 100 + i);
                    else {
                        uint8_t tri = 0;
                        CHECK(authjx_batcher_eval(b, r2, (const uint8_t*)"{\"a\":2}", 7, 0, &tri, nullptr) == AUTHJX_OK);
                        CHECK(tri == 1);
                    }
                }
            });
        for (auto& th : ts) th.join();
        uint64_t batches = 0, requests = 0, expired = 0, max_seen = 0;
        CHECK(authjx_batcher_stats(b, &batches, &requests, &expired, &max_seen) == AUTHJX_OK);
        CHECK(requests == 120 && max_seen > 1);
        // a deadline shorter than the window: untouched buffers
        uint8_t text[64], tri = 0xA5;
        authjx_rendered rec[3];
        std::memset(text, 0xA5, sizeof text);
        std::memset(rec, 0xA5, sizeof rec);
        CHECK(authjx_batcher_phase(b, pha, (const uint8_t*)"{}", 2, 100, &tri, nullptr, text, rec) == AUTHJX_ETIMEDOUT);
        CHECK(tri == 0xA5);
        for (uint8_t x : text) CHECK(x == 0xA5);
        for (size_t k = 0; k < sizeof rec; k++) CHECK(reinterpret_cast<const uint8_t*>(rec)[k] == 0xA5);
        CHECK(authjx_batcher_phase(b, pha, (const uint8_t*)"{}", 2, 0, &tri, nullptr, nullptr, rec) == AUTHJX_EINVAL);
        CHECK(authjx_batcher_phase(b, nullptr, (const uint8_t*)"{}", 2, 0, &tri, nullptr, text, rec) == AUTHJX_EINVAL);
        if (zcopy == 0) authjx_batcher_destroy(b);  // (the second one is left to authjx_shutdown)
    }
    CHECK(authjx_debug_batcher_modes(0, 0, 1) == AUTHJX_OK);
    authjx_phase_free(pha);
    authjx_phase_free(phb);
    authjx_shutdown(ctx);
    authjx_render_free(pa);
    authjx_render_free(pb);
    for (authjx_ruleset* r : {r1, r2, s3, s1, s0}) authjx_free(r);
    std::printf("%s %d checks, %d failed\n", g_fail.load() ? "FAILED" : "ok", g_checks.load(), g_fail.load());
    return g_fail.load() ? 1 : 0;
}
