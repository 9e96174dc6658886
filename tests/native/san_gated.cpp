// san_gated.cpp — TEST-ONLY stand-alone driver (built with ASan + UBSan by gated.mk): runs
// the host build of the gated render body and of the verdict fold (gated_host.cpp) over the
// file tests/test_gated_host.py writes — the programs with their gates, then batches with
// each request's program index and tri-states and the output slots, records and verdicts
// expected for the whole batch (composed from ungated renders and pipeline.verdict_of, guard
// bytes where nothing is written) — and exits 0 when every byte matches and no sanitizer
// report ended the run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/authjx.h"

extern "C" {
void* rt_compile(const authjx_render_output* outs, uint32_t n_outputs, uint32_t n_slots, char* err, size_t cap,
                 int* rc);
void rt_free(void* h);
void* gt_gates_compile(int32_t top, const authjx_gate_evaluator* evals, uint32_t n_evals,
                       const authjx_gate_output* outs, uint32_t n_outputs, uint32_t n_trees, char* err, size_t cap,
                       int* rc);
void gt_gates_free(void* h);
int gt_verdict_of(void* h, const uint8_t* tri, uint32_t n_trees, authjx_verdict* out);
int gtm_render(void* const* progs, void* const* gates, uint32_t n_progs, const uint32_t* prog_of_req,
               const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n, const uint32_t* values,
               uint32_t values_stride, const uint8_t* text, uint32_t text_stride, uint8_t* out_text,
               uint32_t out_stride, uint32_t* out, uint32_t records_stride, const uint8_t* tri, uint32_t tri_stride,
               const uint32_t* tri_of_req, uint32_t* verdicts);
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

// one program of the file: its op lists, compiled; *gates: its gates or nullptr
static void* read_program(Reader& rd, void** gates, uint32_t* n_trees) {
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
    *gates = nullptr;
    *n_trees = 0;
    const uint32_t has_plan = rd.u32();
    std::vector<authjx_gate_evaluator> evals;
    std::vector<authjx_gate_output> gouts;
    int32_t top = -1;
    if (has_plan && !rd.bad) {
        top = (int32_t)rd.u32();
        const uint32_t n_evals = rd.u32();
        *n_trees = rd.u32();
        for (uint32_t i = 0; i < n_evals && !rd.bad; i++) {
            authjx_gate_evaluator e;
            e.when_tree = (int32_t)rd.u32();
            e.rules_tree = (int32_t)rd.u32();
            e.priority = (int32_t)rd.u32();
            evals.push_back(e);
        }
        for (uint32_t k = 0; k < n_outputs && !rd.bad; k++) {
            authjx_gate_output g{};
            g.on = (uint8_t)rd.u32();
            g.when_tree = (int32_t)rd.u32();
            gouts.push_back(g);
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
    if (!h) { std::fprintf(stderr, "compile failed (%d): %s\n", rc, err); return nullptr; }
    if (has_plan) {
        *gates = gt_gates_compile(top, evals.data(), (uint32_t)evals.size(), gouts.data(), n_outputs, *n_trees, err,
                                  sizeof err, &rc);
        if (!*gates) { std::fprintf(stderr, "gates compile failed (%d): %s\n", rc, err); rt_free(h); return nullptr; }
    }
    return h;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: san_gated CASES\n"); return 2; }
    Reader rd;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::perror(argv[1]); return 2; }
        uint8_t tmp[65536];
        for (size_t k; (k = std::fread(tmp, 1, sizeof tmp, f)) > 0;) rd.buf.insert(rd.buf.end(), tmp, tmp + k);
        std::fclose(f);
    }
    const uint32_t n_progs = rd.u32();
    std::vector<void*> progs, gates;
    std::vector<uint32_t> trees;
    for (uint32_t i = 0; i < n_progs && !rd.bad; i++) {
        void* g = nullptr;
        uint32_t nt = 0;
        void* h = read_program(rd, &g, &nt);
        if (!h) return rd.bad ? 2 : 1;
        progs.push_back(h);
        gates.push_back(g);
        trees.push_back(nt);
    }
    const uint32_t n_cases = rd.u32();
    uint64_t requests = 0, folded = 0;
    int status = 0;
    for (uint32_t c = 0; c < n_cases && !rd.bad && !status; c++) {
        const uint32_t n = rd.u32(), vs = rd.u32(), ts = rd.u32(), os = rd.u32(), rs = rd.u32(), tst = rd.u32();
        const uint64_t arena_len = rd.u64();
        const std::vector<uint8_t> arena = rd.vec<uint8_t>(arena_len);
        const std::vector<uint64_t> offs = rd.vec<uint64_t>(n);
        const std::vector<uint32_t> lens = rd.vec<uint32_t>(n);
        const std::vector<uint32_t> por = rd.vec<uint32_t>(n);
        const std::vector<uint32_t> values = rd.vec<uint32_t>((size_t)n * vs * 3);
        const std::vector<uint8_t> text = rd.vec<uint8_t>((size_t)n * ts);
        const std::vector<uint8_t> tri = rd.vec<uint8_t>((size_t)n * tst);
        const std::vector<uint8_t> want_text = rd.vec<uint8_t>((size_t)n * os);
        const std::vector<uint32_t> want = rd.vec<uint32_t>((size_t)n * rs * 3);
        const std::vector<uint32_t> want_ver = rd.vec<uint32_t>((size_t)n * 2);
        if (rd.bad) break;
        std::vector<uint8_t> out_text((size_t)n * os, 0xA5);
        std::vector<uint32_t> out((size_t)n * rs * 3, 0xA5A5A5A5u), ver((size_t)n * 2, 0xA5A5A5A5u);
        const int rc = gtm_render(progs.data(), gates.data(), n_progs, por.data(), arena.data(), offs.data(),
                                  lens.data(), n, values.data(), vs, text.data(), ts, out_text.data(), os, out.data(),
                                  rs, tri.data(), tst, nullptr, ver.data());
        if (rc != 0) { std::fprintf(stderr, "case %u: render failed (%d)\n", c, rc); status = 1; break; }
        for (uint32_t r = 0; r < n; r++) {
            requests++;
            const bool same = std::memcmp(&out_text[(size_t)r * os], &want_text[(size_t)r * os], os) == 0 &&
                              std::memcmp(&out[(size_t)r * rs * 3], &want[(size_t)r * rs * 3], 12u * rs) == 0 &&
                              std::memcmp(&ver[(size_t)r * 2], &want_ver[(size_t)r * 2], 8) == 0;
            if (!same) {
                std::fprintf(stderr, "case %u request %u (program %u): slot, records or verdict differ\n", c, r, por[r]);
                status = 1;
                break;
            }
            if (por[r] < n_progs && gates[por[r]]) {  // authjx_verdict_of's body over an exact-size row
                std::vector<uint8_t> row(tri.begin() + (size_t)r * tst, tri.begin() + (size_t)r * tst + trees[por[r]]);
                authjx_verdict v;
                if (gt_verdict_of(gates[por[r]], row.data(), trees[por[r]], &v) != 0 || v.verdict != want_ver[r * 2] ||
                    (uint32_t)v.denied_by != want_ver[r * 2 + 1]) {
                    std::fprintf(stderr, "case %u request %u: verdict_of differs\n", c, r);
                    status = 1;
                    break;
                }
                folded++;
            }
        }
    }
    for (void* h : progs) rt_free(h);
    for (void* g : gates) gt_gates_free(g);
    if (status) return status;
    if (rd.bad) { std::fprintf(stderr, "truncated case file\n"); return 2; }
    std::printf("san_gated: %u cases, %llu requests (%llu folded)\n", n_cases, (unsigned long long)requests,
                (unsigned long long)folded);
    return 0;
}
