// san_render.cpp — TEST-ONLY stand-alone driver (built with ASan + UBSan by render.mk): runs
// the host build of the render logic (render_host.cpp) over the cases of a file that
// tests/test_render_host.py writes — render programs, batches of documents with their
// selected values, and the bytes and statuses the Python mirror expects — and exits 0 when
// every output matches and no sanitizer report ended the run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/authjx.h"

extern "C" {
void* rt_compile(const authjx_render_output* outs, uint32_t n_outputs, uint32_t n_slots, char* err, size_t cap,
                 int* rc);
void rt_free(void* h);
int rt_render(void* h, const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
              const uint32_t* values, uint32_t values_stride, const uint8_t* text, uint32_t text_stride,
              uint8_t* out_text, uint32_t out_stride, uint32_t* out);
}

struct Reader {
    std::vector<uint8_t> buf;
    size_t i = 0;
    bool bad = false;
    const uint8_t* take(size_t n) {
        if (n > buf.size() - i) { bad = true; i = buf.size(); return nullptr; }
        const uint8_t* p = buf.data() + i;
        i += n;
        return p;
    }
    uint32_t u32() {
        uint32_t v = 0;
        const uint8_t* p = take(4);
        if (p) std::memcpy(&v, p, 4);
        return v;
    }
    uint64_t u64() {
        uint64_t v = 0;
        const uint8_t* p = take(8);
        if (p) std::memcpy(&v, p, 8);
        return v;
    }
    template <class T>
    std::vector<T> vec(size_t n) {
        std::vector<T> v(n);
        const uint8_t* p = take(n * sizeof(T));
        if (p && n) std::memcpy(v.data(), p, n * sizeof(T));
        return v;
    }
};

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: san_render CASES\n"); return 2; }
    Reader rd;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::perror(argv[1]); return 2; }
        uint8_t tmp[65536];
        for (size_t k; (k = std::fread(tmp, 1, sizeof tmp, f)) > 0;) rd.buf.insert(rd.buf.end(), tmp, tmp + k);
        std::fclose(f);
    }
    const uint32_t n_cases = rd.u32();
    uint64_t outputs = 0, declined = 0;
    for (uint32_t c = 0; c < n_cases && !rd.bad; c++) {
        const uint32_t n_outputs = rd.u32(), n_slots = rd.u32();
        std::vector<std::vector<authjx_render_op>> ops(n_outputs);
        std::vector<std::vector<uint8_t>> lits;
        std::vector<authjx_render_output> outs(n_outputs);
        for (uint32_t k = 0; k < n_outputs && !rd.bad; k++) {
            const uint32_t n_ops = rd.u32();
            for (uint32_t q = 0; q < n_ops && !rd.bad; q++) {
                authjx_render_op op{};
                op.op = (uint8_t)rd.u32();
                op.slot = rd.u32();
                op.lit_len = rd.u32();
                lits.push_back(rd.vec<uint8_t>(op.lit_len));
                ops[k].push_back(op);
            }
        }
        if (rd.bad) break;
        size_t li = 0;  // (the literal pointers, once `lits` no longer grows)
        for (uint32_t k = 0; k < n_outputs; k++) {
            for (auto& op : ops[k]) op.lit = lits[li++].data();
            outs[k].ops = ops[k].data();
            outs[k].n_ops = (uint32_t)ops[k].size();
        }
        const uint32_t n = rd.u32(), vs = rd.u32(), ts = rd.u32(), os = rd.u32(), has_text = rd.u32();
        const uint64_t arena_len = rd.u64();
        const std::vector<uint8_t> arena = rd.vec<uint8_t>(arena_len);
        const std::vector<uint64_t> offs = rd.vec<uint64_t>(n);
        const std::vector<uint32_t> lens = rd.vec<uint32_t>(n);
        const std::vector<uint32_t> values = rd.vec<uint32_t>((size_t)n * vs * 3);
        const std::vector<uint8_t> text = rd.vec<uint8_t>(has_text ? (size_t)n * ts : 0);
        if (rd.bad) break;
        char err[256];
        int rc = 0;
        void* h = rt_compile(outs.data(), n_outputs, n_slots, err, sizeof err, &rc);
        if (!h) { std::fprintf(stderr, "case %u: compile failed (%d): %s\n", c, rc, err); return 1; }
        std::vector<uint8_t> out_text((size_t)n * os, 0xA5);
        std::vector<uint32_t> out((size_t)n * n_outputs * 3 + 1);
        rc = rt_render(h, arena.data(), offs.data(), lens.data(), n, values.data(), vs, has_text ? text.data() : nullptr,
                       ts, out_text.data(), os, out.data());
        rt_free(h);
        if (rc != 0) { std::fprintf(stderr, "case %u: render failed (%d)\n", c, rc); return 1; }
        for (uint32_t r = 0; r < n && !rd.bad; r++)
            for (uint32_t k = 0; k < n_outputs && !rd.bad; k++) {
                const uint32_t status = rd.u32(), len = rd.u32();
                const std::vector<uint8_t> want = rd.vec<uint8_t>(len);
                const uint32_t* o = &out[((size_t)r * n_outputs + k) * 3];
                outputs++;
                declined += status != 0;
                const bool same = (o[2] & 0xFFu) == status && o[1] == len && o[0] + o[1] <= os &&
                                  (len == 0 || std::memcmp(&out_text[(size_t)r * os + o[0]], want.data(), len) == 0);
                if (!same) {
                    std::fprintf(stderr, "case %u request %u output %u: status %u len %u, expected status %u len %u\n", c,
                                 r, k, o[2] & 0xFFu, o[1], status, len);
                    return 1;
                }
            }
    }
    if (rd.bad) { std::fprintf(stderr, "truncated case file\n"); return 2; }
    std::printf("san_render: %u cases, %llu outputs (%llu declined as expected)\n", n_cases,
                (unsigned long long)outputs, (unsigned long long)declined);
    return 0;
}
