// san_render_multi.cpp — TEST-ONLY stand-alone driver (built with ASan + UBSan by
// render_multi.mk): runs the host build of the multi-program render body
// (render_multi_host.cpp) over the batches of a file that tests/test_render_multi_host.py
// writes — several programs, a batch with each request's program index, and the output
// slots and records expected for the whole batch (the one-program body's, guard bytes where
// a request has no program) — and exits 0 when every byte matches and no sanitizer report
// ended the run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/authjx.h"

extern "C" {
void* rt_compile(const authjx_render_output* outs, uint32_t n_outputs, uint32_t n_slots, char* err, size_t cap,
                 int* rc);
void rt_free(void* h);
int rtm_render(void* const* progs, uint32_t n_progs, const uint32_t* prog_of_req, const uint8_t* arena,
               const uint64_t* offs, const uint32_t* lens, uint32_t n, const uint32_t* values,
               uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
               uint32_t out_stride, uint32_t* out, uint32_t records_stride);
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

// one program of the file: its op lists, compiled
static void* read_program(Reader& rd) {
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
    if (rd.bad) return nullptr;
    size_t li = 0;  // (the literal pointers, once `lits` no longer grows)
    for (uint32_t k = 0; k < n_outputs; k++) {
        for (auto& op : ops[k]) op.lit = lits[li++].data();
        outs[k].ops = ops[k].data();
        outs[k].n_ops = (uint32_t)ops[k].size();
    }
    char err[256];
    int rc = 0;
    void* h = rt_compile(outs.data(), n_outputs, n_slots, err, sizeof err, &rc);
    if (!h) std::fprintf(stderr, "compile failed (%d): %s\n", rc, err);
    return h;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: san_render_multi CASES\n"); return 2; }
    Reader rd;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::perror(argv[1]); return 2; }
        uint8_t tmp[65536];
        for (size_t k; (k = std::fread(tmp, 1, sizeof tmp, f)) > 0;) rd.buf.insert(rd.buf.end(), tmp, tmp + k);
        std::fclose(f);
    }
    const uint32_t n_cases = rd.u32();
    uint64_t requests = 0, idle = 0;
    for (uint32_t c = 0; c < n_cases && !rd.bad; c++) {
        const uint32_t n_progs = rd.u32();
        std::vector<void*> progs;
        for (uint32_t i = 0; i < n_progs && !rd.bad; i++) {
            void* h = read_program(rd);
            if (!h) return rd.bad ? 2 : 1;
            progs.push_back(h);
        }
        const uint32_t n = rd.u32(), vs = rd.u32(), ts = rd.u32(), os = rd.u32(), has_text = rd.u32(), rs = rd.u32();
        const uint64_t arena_len = rd.u64();
        const std::vector<uint8_t> arena = rd.vec<uint8_t>(arena_len);
        const std::vector<uint64_t> offs = rd.vec<uint64_t>(n);
        const std::vector<uint32_t> lens = rd.vec<uint32_t>(n);
        const std::vector<uint32_t> por = rd.vec<uint32_t>(n);
        const std::vector<uint32_t> values = rd.vec<uint32_t>((size_t)n * vs * 3);
        const std::vector<uint8_t> text = rd.vec<uint8_t>(has_text ? (size_t)n * ts : 0);
        const std::vector<uint8_t> want_text = rd.vec<uint8_t>((size_t)n * os);
        const std::vector<uint32_t> want = rd.vec<uint32_t>((size_t)n * rs * 3);
        if (rd.bad) break;
        std::vector<uint8_t> out_text((size_t)n * os, 0xA5);
        std::vector<uint32_t> out((size_t)n * rs * 3, 0xA5A5A5A5u);
        const int rc = rtm_render(progs.data(), n_progs, por.data(), arena.data(), offs.data(), lens.data(), n,
                                  values.data(), vs, has_text ? text.data() : nullptr, ts, out_text.data(), os,
                                  out.data(), rs);
        for (void* h : progs) rt_free(h);
        if (rc != 0) { std::fprintf(stderr, "case %u: render failed (%d)\n", c, rc); return 1; }
        for (uint32_t r = 0; r < n; r++) {
            requests++;
            idle += por[r] >= n_progs;
            const bool same = std::memcmp(&out_text[(size_t)r * os], &want_text[(size_t)r * os], os) == 0 &&
                              (rs == 0 || std::memcmp(&out[(size_t)r * rs * 3], &want[(size_t)r * rs * 3], 12u * rs) == 0);
            if (!same) {
                std::fprintf(stderr, "case %u request %u (program %u): slot or records differ\n", c, r, por[r]);
                return 1;
            }
        }
    }
    if (rd.bad) { std::fprintf(stderr, "truncated case file\n"); return 2; }
    std::printf("san_render_multi: %u cases, %llu requests (%llu without a program)\n", n_cases,
                (unsigned long long)requests, (unsigned long long)idle);
    return 0;
}
