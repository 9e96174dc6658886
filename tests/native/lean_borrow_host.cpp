// lean_borrow_host.cpp — TEST-ONLY: the host harness (host_eval.cpp) plus the setters of
// the lean walk's spare budget (ajx_lean.h: the iterations in which a lane whose own
// tokens are gone takes the next sub-window's; on the device they come from the wave's
// busiest lane, a host lane gets them from the policy set here). Built by lean_borrow.mk
// into libajx_leanborrow.so; tests/test_lean_borrow.py loads it through AJX_HOSTTEST_LIB.
#include "host_eval.cpp"

extern "C" {
// policy 0: no spare iterations (the walk of a lane alone); 1: k per walk() call;
// 2: unlimited; 3: 0..4 per call, drawn from seed
void ht_lean_spare(uint32_t policy, uint32_t k, uint64_t seed) {
    lean::g_lean_spare_policy = policy;
    lean::g_lean_spare_k = k;
    lean::g_lean_spare_rng = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
    if (!lean::g_lean_spare_rng) lean::g_lean_spare_rng = 1;
}
// tokens taken early so far
uint64_t ht_lean_early(void) { return lean::g_lean_early; }
// the trace's second word per iteration (position | kTraceElig | kTraceStop | kTraceEarly),
// beside ht_lean_trace's buffer (same capacity; null: off)
void ht_lean_trace_pos(uint32_t* buf) { lean::g_lean_trace_pos = buf; }
}
