// tsan_phase.cpp — TEST-ONLY stand-alone driver (built with ThreadSanitizer by
// batcher_phase.mk): 8 producer threads push phase requests of four phases (two stride
// shapes) and eval-only requests through batcher_phase_host.cpp's batcher, two workers;
// every caller checks its own decision, records and bytes, and that a timed-out request's
// buffers keep their guard bytes. Exits 0 when all match and no race report ended the run.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

extern "C" {
void* hbp_create(uint32_t max_batch, uint32_t window_us, uint32_t delay_us, uint32_t workers, uint32_t wake);
void* hbp_phase_new(uint64_t selectors, uint64_t prog, uint32_t n_patterns, uint32_t n_outputs, uint32_t text_stride,
                    uint32_t out_stride);
void hbp_phase_free(void* f);
int hbp_call(void* hv, uint64_t rs, uint32_t n_out, uint8_t byte, const void* phase, uint64_t timeout_us,
             uint8_t* out_tri, uint8_t* out_text, uint32_t* out_rec);
void hbp_stats(void* hv, uint64_t* out);
void hbp_destroy(void* hv);
}

struct Ph {
    void* h;
    uint64_t rs, prog;
    uint32_t n_outputs, out_stride;
};

// what a caller of phase p with document byte b must see (batcher_phase_host.cpp fake_render)
static bool outputs_ok(const Ph& p, uint8_t b, const uint8_t* text, const uint32_t* rec) {
    uint32_t pos = 0;
    for (uint32_t q = 0; q < p.n_outputs; q++) {
        const uint32_t len = 1 + (b + q) % 5;
        if (pos + len > p.out_stride) {
            if (rec[3 * q] != pos || rec[3 * q + 1] != 0 || rec[3 * q + 2] != 1) return false;
            continue;
        }
        if (rec[3 * q] != pos || rec[3 * q + 1] != len || rec[3 * q + 2] != 0) return false;
        for (uint32_t i = 0; i < len; i++)
            if (text[pos + i] != (uint8_t)(b ^ q ^ p.prog)) return false;
        pos += len;
    }
    for (uint32_t i = pos; i < p.out_stride; i++)
        if (text[i] != 0xA5) return false;  // (nothing past the last output is handed on)
    return true;
}

int main() {
    std::vector<Ph> phases;
    const uint32_t shape[4][3] = {{4, 64, 128}, {18, 64, 128}, {0, 0, 16}, {6, 0, 16}};  // outputs, text, out stride
    for (uint32_t i = 0; i < 4; i++)
        phases.push_back({hbp_phase_new(100 + i, 200 + i, 8, shape[i][0], shape[i][1], shape[i][2]), 1 + i % 2, 200 + i,
                          shape[i][0], shape[i][2]});
    std::atomic<uint64_t> bad{0}, timed_out{0};
    for (int round = 0; round < 2; round++) {
        // round 1: a slow evaluator and short deadlines, so that requests expire in the queue
        void* h = hbp_create(64, 300, round ? 20000 : 50, 2, 0);
        std::vector<std::thread> ts;
        for (uint32_t t = 0; t < 8; t++)
            ts.emplace_back([&, t] {
                uint32_t x = 12345u + t;  // (the kinds by a generator of the thread's own: threads that
                                          // fall into step, one request apart, would otherwise batch by kind)
                for (uint32_t i = 0; i < (round ? 12u : 400u); i++) {
                    const uint8_t b = (uint8_t)(t * 31 + i * 7);
                    uint8_t tri[2] = {0xA5, 0xA5}, text[128];
                    uint32_t rec[18 * 3];
                    std::memset(text, 0xA5, sizeof text);
                    std::memset(rec, 0xA5, sizeof rec);
                    x = x * 1103515245u + 12345u;
                    const uint32_t kind = (x >> 16) % 5;
                    const Ph* p = kind < 4 ? &phases[kind] : nullptr;
                    const uint64_t rs = p ? p->rs : 2;
                    const int rc = hbp_call(h, rs, 1, b, p ? p->h : nullptr, round ? 5000 : 0, tri, text, rec);
                    if (rc == -5) {
                        timed_out++;
                        bool clean = tri[0] == 0xA5;
                        for (uint8_t x : text) clean = clean && x == 0xA5;
                        for (uint32_t x : rec) clean = clean && x == 0xA5A5A5A5u;
                        if (!clean) bad++;
                        continue;
                    }
                    bool ok = rc == 0 && tri[0] == (uint8_t)(b ^ rs) && (!p || outputs_ok(*p, b, text, rec));
                    for (uint32_t k = p ? 3 * p->n_outputs : 0; k < 18 * 3; k++) ok = ok && rec[k] == 0xA5A5A5A5u;
                    if (!ok) {
                        std::fprintf(stderr, "round %d thread %u request %u (kind %u): rc %d, wrong result\n", round, t, i,
                                     kind, rc);
                        bad++;
                    }
                }
            });
        for (auto& th : ts) th.join();
        uint64_t st[8];
        hbp_stats(h, st);
        hbp_destroy(h);
        std::printf("round %d: %llu batches, %llu requests, %llu expired, %llu groups, %llu mixed batches, "
                    "%llu plan violations\n", round, (unsigned long long)st[0], (unsigned long long)st[1],
                    (unsigned long long)st[2], (unsigned long long)st[5], (unsigned long long)st[6],
                    (unsigned long long)st[4]);
        if (st[4] || (round == 0 && (st[1] != 8 * 400 || st[6] == 0)) ||
            (round == 1 && (timed_out.load() == 0 || st[2] != timed_out.load()))) {
            std::fprintf(stderr, "round %d: unexpected counts\n", round);
            bad++;
        }
    }
    for (Ph& p : phases) hbp_phase_free(p.h);
    std::printf("tsan_phase: %llu mismatches, %llu timed out\n", (unsigned long long)bad.load(),
                (unsigned long long)timed_out.load());
    return bad.load() ? 1 : 0;
}
