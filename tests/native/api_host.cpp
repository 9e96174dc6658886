// api_host.cpp — TEST-ONLY: a sequential ASan + UBSan driver for the C-ABI's ownership code
// (authorino_amd/csrc/ajx_api.cpp, ajx_batcher_api.cpp) on the host stand-in of the HIP
// runtime (hipstub/, hip_stub.cpp; its hipMalloc is an exact-size calloc, so an undersized
// buffer is a report). One context and one stream grow their buffers through batches of
// 3, 64, 65, 4097 and 130 requests on every entry point; the staged copies of the
// host-buffer entry points must land where the caller's outputs are; bad spans and stale
// capture rows are refused; batchers are destroyed by hand and by authjx_shutdown. Prints
// "ok ..." when every check held; LeakSanitizer speaks at exit.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/authjx.h"

namespace {

int g_fail = 0, g_checks = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        g_checks++;                                                         \
        if (!(c)) {                                                         \
            g_fail++;                                                       \
            std::fprintf(stdout, "FAIL line %d: %s\n", __LINE__, #c);       \
        }                                                                   \
    } while (0)

constexpr uint8_t kGuard = 0xA5;
constexpr size_t kTail = 64;  // guard bytes after every output

authjx_ruleset* compile(authjx_ctx* ctx, const char* val) {
    authjx_pattern p[2] = {{"a", 1, AUTHJX_OP_EQ, val, (uint32_t)std::strlen(val)},
                           {"b", 1, AUTHJX_OP_NEQ, "x", 1}};
    authjx_node nd[3] = {{AUTHJX_NODE_PATTERN, -1, -1, 0}, {AUTHJX_NODE_PATTERN, -1, -1, 1}, {AUTHJX_NODE_AND, 0, 1, -1}};
    authjx_tree t{p, 2, nd, 3, 2};
    authjx_ruleset* rs = nullptr;
    return authjx_compile(ctx, &t, &rs, nullptr, nullptr, 0) == AUTHJX_OK ? rs : nullptr;
}

// one rule tree and a root-less tree of two response selectors (the last two patterns)
authjx_ruleset* compile_forest(authjx_ctx* ctx) {
    authjx_pattern p{"a", 1, AUTHJX_OP_EQ, "1", 1};
    authjx_node nd{AUTHJX_NODE_PATTERN, -1, -1, 0};
    authjx_pattern sel[2] = {{"a", 1, AUTHJX_OP_EQ, "", 0}, {"b", 1, AUTHJX_OP_EQ, "", 0}};
    authjx_tree trees[2] = {{&p, 1, &nd, 1, 0}, {sel, 2, nullptr, 0, -1}};
    authjx_ruleset* rs = nullptr;
    return authjx_compile_forest(ctx, trees, 2, &rs, nullptr, nullptr, 0) == AUTHJX_OK ? rs : nullptr;
}

struct Docs {  // n documents; "device" memory is host memory under the stub
    std::string arena;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens, sor;
    explicit Docs(uint32_t n, uint32_t n_sets = 2) {
        for (uint32_t i = 0; i < n; i++) {
            const std::string d = "{\"a\":" + std::to_string(i) + ",\"b\":\"y\"}";
            offs.push_back(arena.size());
            lens.push_back((uint32_t)d.size());
            sor.push_back(i % n_sets);
            arena += d;
        }
    }
    const uint8_t* a() const { return (const uint8_t*)arena.data(); }
};

// an output of `bytes` bytes followed by guard bytes, all preset to the guard value
struct Out {
    std::vector<uint8_t> v;
    size_t bytes;
    explicit Out(size_t b) : v(b + kTail, kGuard), bytes(b) {}
    template <class T>
    T* as() {
        return reinterpret_cast<T*>(v.data());
    }
    bool tail_kept() const {
        for (size_t i = bytes; i < v.size(); i++)
            if (v[i] != kGuard) return false;
        return true;
    }
    bool all(uint8_t x, size_t upto) const {
        for (size_t i = 0; i < upto; i++)
            if (v[i] != x) return false;
        return true;
    }
};

bool all_i32(const int32_t* p, size_t n, int32_t x) {
    for (size_t i = 0; i < n; i++)
        if (p[i] != x) return false;
    return true;
}
bool all_u64(const uint64_t* p, size_t n, uint64_t x) {
    for (size_t i = 0; i < n; i++)
        if (p[i] != x) return false;
    return true;
}

// the stub's slow count for the plan a one-ruleset batch of n takes (hip_stub.cpp)
int64_t stub_count(uint32_t n) { return n <= 4096 ? n / 5 : n / 7; }

void eval_checks(Out& tri, Out* err, Out* bm, uint32_t n, uint32_t stride) {
    CHECK(tri.all(1, n) && tri.tail_kept());
    if (err) CHECK(all_i32(err->as<int32_t>(), n, -1) && err->tail_kept());
    if (bm) CHECK(all_u64(bm->as<uint64_t>(), (size_t)n * stride, 1) && bm->tail_kept());
}

// every entry point at one batch size, on stream s and on the context's own stream
void run_size(authjx_ctx* ctx, hipStream_t s, uint32_t n, const authjx_ruleset* const* two,
              const authjx_ruleset* forest) {
    const Docs d(n);
    const authjx_ruleset* const* one = two;
    const uint32_t vs = 2, ts = 16, bs = 2;  // values, text and bitmap strides
    {  // device buffers: results only, then with error indices and bitmaps
        Out tri(n);
        CHECK(authjx_eval_batch_device(ctx, one, 1, nullptr, d.a(), d.offs.data(), d.lens.data(), n, tri.as<uint8_t>(),
                                       nullptr, nullptr, 0, s) == AUTHJX_OK);
        eval_checks(tri, nullptr, nullptr, n, 0);
        CHECK(authjx_last_exact_count(ctx) == stub_count(n));
        CHECK(authjx_last_kernel_ms(ctx) > 0.f);
        Out tri2(n), err(n * 4), bm((size_t)n * bs * 8);
        CHECK(authjx_eval_batch_device(ctx, one, 1, nullptr, d.a(), d.offs.data(), d.lens.data(), n,
                                       tri2.as<uint8_t>(), err.as<int32_t>(), bm.as<uint64_t>(), bs, s) == AUTHJX_OK);
        eval_checks(tri2, &err, &bm, n, bs);
        Out tri3(n), err3(n * 4);
        CHECK(authjx_eval_batch_device(ctx, two, 2, d.sor.data(), d.a(), d.offs.data(), d.lens.data(), n,
                                       tri3.as<uint8_t>(), err3.as<int32_t>(), nullptr, 0, s) == AUTHJX_OK);
        eval_checks(tri3, &err3, nullptr, n, 0);
    }
    {  // selector values, with and without text
        Out val((size_t)n * vs * sizeof(authjx_value)), val2(val.bytes), text((size_t)n * ts);
        CHECK(authjx_select_batch_device(ctx, one, 1, nullptr, d.a(), d.offs.data(), d.lens.data(), n,
                                         val.as<authjx_value>(), vs, s) == AUTHJX_OK);
        CHECK(val.all(0, val.bytes) && val.tail_kept());
        CHECK(authjx_select_text_batch_device(ctx, two, 2, d.sor.data(), d.a(), d.offs.data(), d.lens.data(), n,
                                              val2.as<authjx_value>(), vs, text.as<uint8_t>(), ts, s) == AUTHJX_OK);
        CHECK(val2.all(0, val2.bytes) && val2.tail_kept() && text.tail_kept());
    }
    {  // a forest: its kept capture rows resolve the response selectors
        const uint32_t nt = authjx_ruleset_trees(forest), np = authjx_ruleset_patterns(forest);
        CHECK(nt == 2 && np == 3);
        Out tri((size_t)n * nt), err((size_t)n * nt * 4), val((size_t)n * 2 * sizeof(authjx_value));
        CHECK(authjx_eval_batch_device(ctx, &forest, 1, nullptr, d.a(), d.offs.data(), d.lens.data(), n,
                                       tri.as<uint8_t>(), err.as<int32_t>(), nullptr, 0, s) == AUTHJX_OK);
        eval_checks(tri, &err, nullptr, n, 0);  // (the stub writes one result per request)
        CHECK(authjx_last_exact_count(ctx) == stub_count(n));
        CHECK(authjx_select_from_eval_device(ctx, forest, np - 2, d.a(), d.offs.data(), d.lens.data(), n,
                                             val.as<authjx_value>(), 2, s) == AUTHJX_OK);
        bool rows = true;
        for (uint32_t r = 0; r < n; r++) rows = rows && val.as<authjx_value>()[(size_t)r * 2].start == r;
        CHECK(rows && val.tail_kept());
    }
    {  // host buffers, staged on the context's stream and copied back
        Out tri(n), err(n * 4), bm((size_t)n * bs * 8);
        CHECK(authjx_eval_batch(ctx, one, 1, nullptr, d.a(), d.arena.size(), d.offs.data(), d.lens.data(), n,
                                tri.as<uint8_t>(), err.as<int32_t>(), bm.as<uint64_t>(), bs) == AUTHJX_OK);
        eval_checks(tri, &err, &bm, n, bs);
        Out tri2(n);
        CHECK(authjx_eval_batch(ctx, two, 2, d.sor.data(), d.a(), d.arena.size(), d.offs.data(), d.lens.data(), n,
                                tri2.as<uint8_t>(), nullptr, nullptr, 0) == AUTHJX_OK);
        eval_checks(tri2, nullptr, nullptr, n, 0);
        Out val((size_t)n * vs * sizeof(authjx_value)), text((size_t)n * ts);
        CHECK(authjx_select_text_batch(ctx, two, 2, d.sor.data(), d.a(), d.arena.size(), d.offs.data(), d.lens.data(),
                                       n, val.as<authjx_value>(), vs, text.as<uint8_t>(), ts) == AUTHJX_OK);
        CHECK(val.all(0, val.bytes) && val.tail_kept() && text.tail_kept());
        Out val2(val.bytes);
        CHECK(authjx_select_batch(ctx, one, 1, nullptr, d.a(), d.arena.size(), d.offs.data(), d.lens.data(), n,
                                  val2.as<authjx_value>(), vs) == AUTHJX_OK);
        CHECK(val2.all(0, val2.bytes) && val2.tail_kept());
    }
}

void refusals(authjx_ctx* ctx, hipStream_t s, const authjx_ruleset* const* two, const authjx_ruleset* forest) {
    const uint32_t n = 8;
    const Docs d(n);
    Out tri(n), val((size_t)n * 2 * sizeof(authjx_value));
    auto eval_host = [&](const std::vector<uint64_t>& offs, const std::vector<uint32_t>& lens,
                         const std::vector<uint32_t>& sor) {
        return authjx_eval_batch(ctx, two, 2, sor.data(), d.a(), d.arena.size(), offs.data(), lens.data(), n,
                                 tri.as<uint8_t>(), nullptr, nullptr, 0);
    };
    auto select_host = [&](const std::vector<uint64_t>& offs, const std::vector<uint32_t>& lens) {
        return authjx_select_text_batch(ctx, two, 1, nullptr, d.a(), d.arena.size(), offs.data(), lens.data(), n,
                                        val.as<authjx_value>(), 2, nullptr, 0);
    };
    std::vector<uint64_t> offs = d.offs;
    std::vector<uint32_t> lens = d.lens, sor = d.sor;
    lens[n - 1] += 1;  // one byte past the arena
    CHECK(eval_host(offs, lens, sor) == AUTHJX_EINVAL);
    CHECK(select_host(offs, lens) == AUTHJX_EINVAL);
    offs[3] = d.arena.size() + 1;  // starts past the arena
    lens = d.lens;
    lens[3] = 0;
    CHECK(eval_host(offs, lens, sor) == AUTHJX_EINVAL);
    offs = d.offs;  // offs + lens wraps
    lens = d.lens;
    offs[2] = ~0ull - 7;
    lens[2] = 16;
    CHECK(eval_host(offs, lens, sor) == AUTHJX_EINVAL);
    CHECK(select_host(offs, lens) == AUTHJX_EINVAL);
    sor[5] = 2;  // no such ruleset
    CHECK(eval_host(d.offs, d.lens, sor) == AUTHJX_EINVAL);
    CHECK(tri.all(kGuard, n) && val.all(kGuard, val.bytes));  // (nothing was written)
    CHECK(eval_host(d.offs, d.lens, d.sor) == AUTHJX_OK);  // the context still evaluates
    eval_checks(tri, nullptr, nullptr, n, 0);
    CHECK(select_host(d.offs, d.lens) == AUTHJX_OK);
    // capture rows of another batch size, then of another ruleset, on this stream
    auto eval_dev = [&](const authjx_ruleset* rs, uint32_t m) {
        return authjx_eval_batch_device(ctx, &rs, 1, nullptr, d.a(), d.offs.data(), d.lens.data(), m,
                                        tri.as<uint8_t>(), nullptr, nullptr, 0, s);
    };
    auto from_eval = [&](uint32_t m) {
        return authjx_select_from_eval_device(ctx, forest, 1, d.a(), d.offs.data(), d.lens.data(), m,
                                              val.as<authjx_value>(), 2, s);
    };
    CHECK(eval_dev(forest, n) == AUTHJX_OK);
    CHECK(from_eval(n - 1) == AUTHJX_EINVAL);
    CHECK(from_eval(n) == AUTHJX_OK);
    CHECK(eval_dev(two[0], n) == AUTHJX_OK);
    CHECK(from_eval(n) == AUTHJX_EINVAL);
    CHECK(eval_dev(forest, n) == AUTHJX_OK && from_eval(n) == AUTHJX_OK);
}

// a handful of requests through a batcher from this thread
void batcher_requests(authjx_batcher* b, const authjx_ruleset* rs, const authjx_ruleset* forest) {
    for (int k = 0; k < 6; k++) {
        const std::string d = "{\"a\":" + std::to_string(k) + "}";
        uint8_t tri[2] = {kGuard, kGuard};
        int32_t err[2] = {7, 7};
        const bool f = (k & 1) != 0;
        CHECK(authjx_batcher_eval(b, f ? forest : rs, (const uint8_t*)d.data(), d.size(), 0, tri, f ? nullptr : err) ==
              AUTHJX_OK);
        CHECK(tri[0] == 1 && (f || (err[0] == -1 && tri[1] == kGuard && err[1] == 7)));
    }
    uint64_t batches = 0, requests = 0;
    CHECK(authjx_batcher_stats(b, &batches, &requests, nullptr, nullptr) == AUTHJX_OK && requests == 6);
}

}  // namespace

int main() {
    authjx_ctx* ctx = nullptr;
    if (authjx_init(0, &ctx) != AUTHJX_OK) return 2;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return 2;
    authjx_ruleset* a = compile(ctx, "1");
    authjx_ruleset* b = compile(ctx, "2");
    authjx_ruleset* forest = compile_forest(ctx);
    if (!a || !b || !forest) return 2;
    const authjx_ruleset* two[2] = {a, b};
    for (uint32_t n : {3u, 64u, 65u, 4097u, 130u}) run_size(ctx, s, n, two, forest);
    {  // the set table past its 64 entries: 65 rulesets, then the two again
        std::vector<authjx_ruleset*> many;
        for (int i = 0; i < 65; i++) many.push_back(compile(ctx, std::to_string(i).c_str()));
        const uint32_t n = 130;
        const Docs d(n, 65);
        Out tri(n);
        CHECK(authjx_eval_batch_device(ctx, many.data(), 65, d.sor.data(), d.a(), d.offs.data(), d.lens.data(), n,
                                       tri.as<uint8_t>(), nullptr, nullptr, 0, s) == AUTHJX_OK);
        eval_checks(tri, nullptr, nullptr, n, 0);
        Out tri2(n);
        CHECK(authjx_eval_batch(ctx, many.data(), 65, d.sor.data(), d.a(), d.arena.size(), d.offs.data(), d.lens.data(),
                                n, tri2.as<uint8_t>(), nullptr, nullptr, 0) == AUTHJX_OK);
        eval_checks(tri2, nullptr, nullptr, n, 0);
        run_size(ctx, s, 3, two, forest);
        for (authjx_ruleset* rs : many) authjx_free(rs);
    }
    refusals(ctx, s, two, forest);
    CHECK(authjx_release_stream(ctx, s) == AUTHJX_OK);
    CHECK(authjx_release_stream(ctx, nullptr) == AUTHJX_EINVAL);
    (void)hipStreamDestroy(s);
    authjx_batcher *b1 = nullptr, *b2 = nullptr;
    CHECK(authjx_batcher_create(ctx, 16, 50, 0, &b1) == AUTHJX_OK && b1);
    if (b1) batcher_requests(b1, a, forest);
    authjx_batcher_destroy(b1);
    CHECK(authjx_batcher_create(ctx, 4, 0, 0, &b2) == AUTHJX_OK && b2);  // left for authjx_shutdown
    if (b2) batcher_requests(b2, b, forest);
    authjx_free(a);
    authjx_free(b);
    authjx_free(forest);
    authjx_shutdown(ctx);
    if (g_fail) {
        std::printf("failed %d of %d checks\n", g_fail, g_checks);
        return 1;
    }
    std::printf("ok checks %d\n", g_checks);
    return 0;
}
