// host_eval.cpp — TEST-ONLY harness. Compiles the kernels' per-document logic
// (authorino_amd/csrc/ajx_device.h) and the reconcile-time compiler for the host CPU so
// the CPU test suite can check them against the oracle without a GPU. It is not part
// of libauthjx.so and is never used by the product path (which has no CPU fallback).
#define AJX_HD inline
#include <cstring>
#include <string>
#include <vector>

#include "../../authorino_amd/csrc/ajx_compiler.h"
#include "../../authorino_amd/csrc/ajx_fast.h"
#define AJX_LEAN_COUNT 1
#include "../../authorino_amd/csrc/ajx_lean.h"
#include "../../authorino_amd/csrc/ajx_modifiers.h"
#include "../../authorino_amd/csrc/ajx_regex.h"

using namespace ajx;

struct HtRuleset {
    CompiledRuleset c;
};

extern "C" {

void* ht_compile(const authjx_tree* tree, int32_t* status, char* err, size_t cap, int* rc) {
    HtRuleset* r = new HtRuleset();
    std::string e;
    *rc = compile_tree(tree, &r->c, &e);
    if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
    if (*rc != AUTHJX_OK) { delete r; return nullptr; }
    if (status)
        for (uint32_t i = 0; i < r->c.n_patterns; i++) status[i] = r->c.pattern_status[i];
    return r;
}

// a forest (authjx_compile_forest): trees[n], one fold program each
void* ht_compile_forest(const authjx_tree* trees, uint32_t n, char* err, size_t cap, int* rc) {
    HtRuleset* r = new HtRuleset();
    std::string e;
    *rc = compile_forest(trees, n, &r->c, &e);
    if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
    if (*rc != AUTHJX_OK) { delete r; return nullptr; }
    return r;
}

void ht_free(void* h) { delete (HtRuleset*)h; }

// evaluate one document; res[p] receives each pattern's tri-state
int ht_eval(void* h, const uint8_t* doc_in, uint32_t len, uint8_t* res, int32_t* err) {
    // (the device reads whole aligned blocks around a document: give the copy that slack)
    std::vector<uint8_t> buf(len + 32, 0);
    uint8_t* doc = buf.data() + 16;
    if (len) std::memcpy(doc, doc_in, len);
    const uint8_t* blob = ((HtRuleset*)h)->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    const Selector* sels = (const Selector*)(blob + hd->off_selectors);
    const Component* comps = (const Component*)(blob + hd->off_components);
    const Pattern* pats = (const Pattern*)(blob + hd->off_patterns);
    const uint32_t* code = (const uint32_t*)(blob + hd->off_code);
    const uint8_t* lits = blob + hd->off_literals;
    for (uint32_t p = 0; p < hd->n_patterns; p++) {
        ValueRef v{0, 0, T_NULL, 0};
        if (pats[p].state == P_OK) {
            const Selector& s = sels[pats[p].selector];
            v = gj_get(doc, len, comps + s.comp_begin, s.comp_count, lits);
        }
        if (pats[p].state == P_OK && v.esc == kValList) {  // a "#." list (the kernel's build_list)
            static ModBufs mb;
            const uint8_t* rd;
            ValueRef rv;
            res[p] = build_list(blob, sels[pats[p].selector], doc, v, mb, &rd, &rv)
                         ? eval_pattern<true>(blob, pats[p], rd, rv)
                         : (uint8_t)V_U;
            continue;
        }
        if (pats[p].state == P_OK && sels[pats[p].selector].mod_count) {
            static ModBufs mb;  // (the kernel's work-item scratch)
            const uint8_t* rd;
            ValueRef rv;
            res[p] = apply_modifiers(blob, sels[pats[p].selector], doc, v, mb, &rd, &rv)
                         ? eval_pattern<true>(blob, pats[p], rd, rv)
                         : (uint8_t)V_U;
            continue;
        }
        res[p] = eval_pattern<true>(blob, pats[p], doc, v);
    }
    return run_fold(code, hd->n_code, [&](uint32_t p) { return res[p]; }, err);
}

// fault injection for the checker tests (tests/test_checker_sensitivity.py): 1 drops the
// last byte of every built text value select_value returns, as a kernel bug would
static int g_inject_truncate = 0;
void ht_inject_truncate(int on) { g_inject_truncate = on; }

// select_value (ajx_modifiers.h): the value of pattern p's selector as the select kernel
// resolves it with a text slot; returns 0, or -1 undecided (out = {start, len, type | esc << 8})
int ht_select_value(void* h, uint32_t p, const uint8_t* doc_in, uint32_t len, uint8_t* text, uint32_t cap,
                    uint32_t* used, uint32_t* out) {
    std::vector<uint8_t> buf(len + 32, 0);
    uint8_t* doc = buf.data() + 16;
    if (len) std::memcpy(doc, doc_in, len);
    const uint8_t* blob = ((HtRuleset*)h)->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    const Selector* sels = (const Selector*)(blob + hd->off_selectors);
    const Pattern* pats = (const Pattern*)(blob + hd->off_patterns);
    static ModBufs mb;
    if (!select_value(blob, sels[pats[p].selector], doc, len, mb, text, cap, used, out)) return -1;
    if (g_inject_truncate && ((out[2] >> 8) & kValText) && out[1]) out[1]--;
    return 0;
}

// json_valid (ajx_modifiers.h, gjson Valid): 1 valid, 0 invalid, -1 undecided (depth)
int ht_json_valid(const uint8_t* d, uint32_t n) {
    bool ok;
    if (!json_valid(d, n, &ok)) return -1;
    return ok ? 1 : 0;
}

// value resolution only: type + raw span
int ht_get(const char* path, uint32_t plen, const uint8_t* doc_in, uint32_t len, uint32_t* start, uint32_t* end) {
    std::vector<uint8_t> buf(len + 32, 0);
    uint8_t* doc = buf.data() + 16;
    if (len) std::memcpy(doc, doc_in, len);
    std::vector<PathComponent> pc;
    if (!split_selector(std::string(path, plen), &pc)) return -1;
    std::string lits;
    std::vector<Component> comps;
    for (auto& c : pc) {
        Component k{(uint32_t)lits.size(), (uint32_t)c.key.size(), c.array_index, 0};
        lits += c.key;
        comps.push_back(k);
    }
    ValueRef v = gj_get(doc, len, comps.data(), (uint32_t)comps.size(), (const uint8_t*)lits.data());
    *start = v.start;
    *end = v.end;
    return v.type;
}

// Result.String() of the value at path; returns length or -1 undecided / -2 unsupported
int ht_string(const char* path, uint32_t plen, const uint8_t* doc_in, uint32_t len, uint8_t* out, uint32_t cap) {
    std::vector<uint8_t> buf(len + 32, 0);
    uint8_t* doc = buf.data() + 16;
    if (len) std::memcpy(doc, doc_in, len);
    std::vector<PathComponent> pc;
    if (!split_selector(std::string(path, plen), &pc)) return -2;
    std::string lits;
    std::vector<Component> comps;
    for (auto& c : pc) {
        Component k{(uint32_t)lits.size(), (uint32_t)c.key.size(), c.array_index, 0};
        lits += c.key;
        comps.push_back(k);
    }
    ValueRef v = gj_get(doc, len, comps.data(), (uint32_t)comps.size(), (const uint8_t*)lits.data());
    static ModBufs mb;
    if (v.esc == kValList) {  // a "#." list: its text from build_list
        std::vector<uint8_t> blob(sizeof(RulesetHdr) + comps.size() * sizeof(Component) + lits.size() + 16, 0);
        RulesetHdr* hd = (RulesetHdr*)blob.data();
        hd->off_components = sizeof(RulesetHdr);
        hd->off_literals = (uint32_t)(sizeof(RulesetHdr) + comps.size() * sizeof(Component));
        std::memcpy(blob.data() + hd->off_components, comps.data(), comps.size() * sizeof(Component));
        std::memcpy(blob.data() + hd->off_literals, lits.data(), lits.size());
        Selector sel{0, (uint16_t)comps.size(), 0, 0};
        const uint8_t* rd;
        ValueRef rv;
        if (!build_list(blob.data(), sel, doc, v, mb, &rd, &rv)) return -1;
        uint32_t k = 0;
        for (uint32_t i = rv.start; i < rv.end; i++)
            if (k < cap) out[k++] = rd[i];
        return (int)k;
    }
    StrSrc s;
    if (!string_of<true>(doc, v, &s)) return -1;
    uint32_t k = 0;
    for (int c; (c = s.next()) >= 0;)
        if (k < cap) out[k++] = (uint8_t)c;
    return (int)k;
}

// regex: compile + match (host copy of the device DFA walk)
void* ht_regex(const char* pat, uint32_t n, int* status, char* err, size_t cap) {
    RegexDfa* d = new RegexDfa();
    std::string e;
    *status = compile_go_regex(std::string(pat, n), d, &e);
    if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
    if (*status != RX_OK) { delete d; return nullptr; }
    return d;
}
void ht_regex_free(void* d) { delete (RegexDfa*)d; }
uint32_t ht_regex_states(void* d) { return ((RegexDfa*)d)->n_states; }
int ht_regex_match(void* dv, const uint8_t* s, uint32_t n) {
    RegexDfa* d = (RegexDfa*)dv;
    // lay the DFA out like the blob does
    std::vector<uint8_t> blob(sizeof(DfaHdr));
    DfaHdr h;
    std::memset(&h, 0, sizeof h);
    h.n_states = d->n_states; h.n_classes = d->n_classes; h.start = d->start; h.match_state = d->match_state;
    std::memcpy(h.ascii_class, d->ascii_class, 128);
    h.trans_off = (uint32_t)blob.size();
    blob.insert(blob.end(), (uint8_t*)d->trans.data(), (uint8_t*)(d->trans.data() + d->trans.size()));
    h.eot_off = (uint32_t)blob.size();
    blob.insert(blob.end(), d->eot.begin(), d->eot.end());
    while (blob.size() % 16) blob.push_back(0);
    h.ranges_off = (uint32_t)blob.size();
    h.n_ranges = (uint32_t)d->ranges.size();
    blob.insert(blob.end(), (uint8_t*)d->ranges.data(), (uint8_t*)(d->ranges.data() + d->ranges.size()));
    std::memcpy(blob.data(), &h, sizeof h);
    StrSrc src;
    src.init_raw(s, 0, n);
    return dfa_match(blob.data(), 0, &src) ? 1 : 0;
}

}  // extern "C"

static uint64_t g_flat_folds = 0;  // (lean evaluations whose ruleset took the flat fold)
extern "C" uint64_t ht_flat_folds() { return g_flat_folds; }
static uint64_t g_group_folds = 0;  // (the same for the group fold)
extern "C" uint64_t ht_group_folds() { return g_group_folds; }

// Stage B as the kernels run it (finish_request, ajx_stageb.h) for one request on its capture
// row; dec / ring: the lean scan's decisions and the lane's span buffer, as its kernel passes
// them. res[p] is read back from what it wrote (static E, unsupported, the T bitmap). Returns
// -1 when it hands the request to the exact scan; 99 (no tri-state: the test's comparison
// fails) when a tree's result is not the code interpreter's on res, or a bitmap word past the
// ruleset's two was not zeroed; else the interpreter's tri-state of the fold code.
static int stage_b(const uint8_t* blob, const uint8_t* d, uint64_t* row, const uint64_t* dec, uint8_t* ring,
                   uint8_t* res, int32_t* err, bool count) {
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    const uint32_t nt = hd->pad1[0], slots = nt ? nt : 1u;
    constexpr uint32_t kStride = 4;  // (the ruleset's two words and two the writer must zero)
    uint64_t bm[kStride];
    std::memset(bm, 0xFF, sizeof bm);
    std::vector<uint8_t> tri(slots, 0xEE);
    std::vector<int32_t> ep(slots, -7);
    if (!finish_request(0, blob, d, RowRef(row), tri.data(), ep.data(), bm, kStride, dec, ring)) return -1;
    if (bm[2] | bm[3]) return 99;
    for (uint32_t p = 0; p < hd->n_patterns; p++) {
        const uint64_t bit = 1ull << (p & 63);
        const uint32_t k = p >> 6;
        res[p] = (hd->static_error[k] & bit) ? V_E : (hd->unsupported[k] & bit) ? V_U : (bm[k] & bit) ? V_T : V_F;
    }
    if (count && (hd->flags & kFlagFlatFold)) g_flat_folds++;
    if (count && (hd->flags & kFlagGroupFold)) g_group_folds++;
    const uint32_t* code = (const uint32_t*)(blob + hd->off_code);
    const auto rp = [&](uint32_t p) { return res[p]; };
    const int whole = run_fold(code, hd->n_code, rp, err);
    if (nt == 0) return tri[0] == whole && ep[0] == *err ? whole : 99;
    const uint32_t* rc = (const uint32_t*)(blob + hd->pad1[1]);
    for (uint32_t k = 0; k < nt; k++) {  // (a forest: tree by tree)
        int32_t e;
        if (tri[k] != run_fold(code + rc[2 * k], rc[2 * k + 1], rp, &e) || ep[k] != e) return 99;
    }
    return whole;
}

extern "C" {
// single-pass path: returns -1 when the document is handed to the exact scan, else the
// tri-state; res[p] receives each pattern's value. `mis` places the copy at that
// misalignment (0..15) like an arbitrary arena offset.
static int eval_single_pass(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                            bool ev, uint64_t* row_out);
int ht_eval_fast(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err) {
    return eval_single_pass(h, doc, len, mis, res, err, false, nullptr);
}
// the token scanner with its capture row (row_out: 1 + n_selectors)
int ht_eval_tok(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                uint64_t* row_out) {
    return eval_single_pass(h, doc, len, mis, res, err, false, row_out);
}
static int eval_single_pass(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                            bool ev, uint64_t* row_out) {
    const uint8_t* blob = ((HtRuleset*)h)->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    if (!(hd->flags & kFlagFastOk)) return -2;
    std::vector<uint8_t> buf(len + 64, 0);
    uintptr_t base = ((uintptr_t)buf.data() + 15) & ~(uintptr_t)15;
    uint8_t* d = (uint8_t*)base + (mis & 15);
    std::memcpy(d, doc, len);
    std::vector<uint64_t> row(1 + hd->n_selectors, 0xDEADBEEFDEADBEEFull);
    const uint32_t* a = (const uint32_t*)(d - mis);
    alignas(16) uint8_t ring_mem[128];
    std::memset(ring_mem, 0x5A, sizeof ring_mem);
    WinRing ring{ring_mem, 0u, 16u};
    auto load = [&](uint32_t b, uint32_t nblk) -> Block16 {
        if (b < nblk) return Block16{a[4 * b], a[4 * b + 1], a[4 * b + 2], a[4 * b + 3]};
        return Block16{0, 0, 0, 0};
    };
    (void)ev;
    const bool ok = scan_doc(blob, blob_tables(blob), d, len, row.data(), ring, load);
    if (!ok) return -1;
    if (row_out) std::memcpy(row_out, row.data(), row.size() * sizeof(uint64_t));
    return stage_b(blob, d, row.data(), nullptr, nullptr, res, err, false);
}
}

extern "C" uint32_t ht_blob_size(void* h) { return (uint32_t)((HtRuleset*)h)->c.blob.size(); }
// the ruleset's header (profiling helpers): key table log2 size, probes, hot bytes
extern "C" void ht_blob_keytab(void* h, uint32_t* out) {
    const RulesetHdr* hd = (const RulesetHdr*)((HtRuleset*)h)->c.blob.data();
    out[0] = hd->key_slots_log2;
    out[1] = hd->key_probes;
    out[2] = hd->hot_bytes;
    out[3] = hd->n_trie_nodes;
    out[4] = hd->off_key_slots;
    out[5] = hd->off_eager;
}
extern "C" uint32_t ht_blob_hot_bytes(void* h) { return ((const RulesetHdr*)((HtRuleset*)h)->c.blob.data())->hot_bytes; }



// ---------------------------------------------------------------------------------
// The lean scan (ajx_lean.h) for one document: -1 exact scan, -2 not eligible, else the
// tri-state; res[p] per pattern; row_out (optional, 1 + n_selectors) the capture row.
static uint64_t g_last_dec[2];
extern "C" void ht_lean_last_dec(uint64_t* out) {
    out[0] = g_last_dec[0];
    out[1] = g_last_dec[1];
}
// keep = 0: the lean scan writes only the capture records stage B needs (the kernel's
// default when no caller reads the rows); 1 every record
static uint32_t g_lean_keep = 1;
extern "C" void ht_lean_keep(int keep) { g_lean_keep = keep ? 1u : 0u; }
extern "C" int ht_eval_lean_row(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                                uint64_t* row_out) {
    const uint8_t* blob = ((HtRuleset*)h)->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    if (!(hd->flags & kFlagFastOk)) return -2;
    if (!lean::eligible(hd, len)) return -1;  // (as the kernels: empty or too long, the exact scan)
    std::vector<uint8_t> buf(len + 96, 0x7A);  // (neighbour bytes around the document)
    uintptr_t base = ((uintptr_t)buf.data() + 15) & ~(uintptr_t)15;
    uint8_t* d = (uint8_t*)base + (mis & 15);
    std::memcpy(d, doc, len);
    std::vector<uint64_t> row(1 + hd->n_selectors, 0xDEADBEEFDEADBEEFull);
    const uint32_t* a = (const uint32_t*)(d - (mis & 15));
    const uint32_t nb = (uint32_t)((buf.data() + buf.size() - (const uint8_t*)a) / 16);
    // the wave's ring (chunk-major); this document's lane: mis * 5 (every lane offset used)
    static thread_local std::vector<uint8_t> ring_mem(lean::kRingBytesPerWave);
    std::memset(ring_mem.data(), 0x5A, ring_mem.size());
    const uint32_t nblk = (len + (mis & 15) + 15) / 16;
    lean::CopyLoader ld{(const uint8_t*)a, nblk, nb, ring_mem.data() + ((mis * 5u) & 63u) * 16u};
    uint64_t dec[2] = {0, 0};
    // (the instance the kernel takes for this ruleset: RulesetHdr::lean_feat)
    const uint32_t m15 = (uint32_t)(mis & 15);
    const RowRef rr(row.data());
    const bool ok = (hd->lean_feat & kLeanArr) ? lean::scan_doc<0, true>(blob, len, m15, rr, ld.lane_ring, ld, dec, g_lean_keep)
                                               : lean::scan_doc<0, false>(blob, len, m15, rr, ld.lane_ring, ld, dec, g_lean_keep);
    g_last_dec[0] = dec[0];
    g_last_dec[1] = dec[1];
    if (!ok) return -1;
    if (row_out) std::memcpy(row_out, row.data(), row.size() * sizeof(uint64_t));
    // (values from the lane's span buffer, as the kernel)
    return stage_b(blob, d, row.data(), dec, ld.lane_ring, res, err, true);
}
// tree_fold against the code interpreter for every forest tree with a TreeFold shape, on n
// random 128-bit (T, U, static E) bitmaps: the number of differences (-1: no such tree)
extern "C" int64_t ht_tree_fold_check(void* h, uint64_t seed, uint32_t n) {
    const uint8_t* blob = ((HtRuleset*)h)->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    const uint32_t nt = hd->pad1[0];
    if (!nt || !hd->pad1[2]) return -1;
    const uint32_t* code = (const uint32_t*)(blob + hd->off_code);
    const uint32_t* rc = (const uint32_t*)(blob + hd->pad1[1]);
    const TreeFold* tf = (const TreeFold*)(blob + hd->pad1[2]);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 7ull;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    int64_t bad = 0, shaped = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool dense = (i & 3) == 0;
        const uint64_t t[2] = {dense ? rnd() : (rnd() | rnd() | rnd()), dense ? rnd() : (rnd() | rnd() | rnd())};
        const uint64_t u[2] = {(i & 7) ? (rnd() & rnd() & rnd() & rnd()) : 0ull, (i & 7) ? (rnd() & rnd() & rnd() & rnd()) : 0ull};
        const uint64_t se[2] = {(i & 5) ? (rnd() & rnd() & rnd() & rnd() & rnd()) : 0ull,
                                (i & 5) ? (rnd() & rnd() & rnd() & rnd() & rnd()) : 0ull};
        for (uint32_t k = 0; k < nt; k++) {
            if (!tf[k].shape) continue;
            shaped++;
            int32_t e1, e2;
            const uint8_t a = run_fold_bits(code + rc[2 * k], rc[2 * k + 1], t, u, se, &e1);
            const uint8_t b = tree_fold(tf[k], t, u, se, &e2);
            if (a != b || e1 != e2) bad++;
        }
    }
    return shaped ? bad : -1;
}
// group_fold against the code interpreter on n random (T, U, static E) bitmaps of the
// ruleset's patterns: the number of differences (-1: the ruleset is not kFlagGroupFold)
extern "C" int64_t ht_group_fold_check(void* h, uint64_t seed, uint32_t n) {
    const uint8_t* blob = ((HtRuleset*)h)->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    if (!(hd->flags & kFlagGroupFold)) return -1;
    const uint32_t* code = (const uint32_t*)(blob + hd->off_code);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1ull;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    int64_t bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        // mostly-true T, sparse U and E (bits at 1/16 and 1/64 density), now and then dense
        const uint64_t t[2] = {(i & 3) ? (rnd() | rnd() | rnd()) : rnd(), 0ull};
        const uint64_t u[2] = {(i & 7) ? (rnd() & rnd() & rnd() & rnd()) : 0ull, 0ull};
        const uint64_t se[2] = {(i & 5) ? (rnd() & rnd() & rnd() & rnd() & rnd() & rnd()) : 0ull, 0ull};
        int32_t e1, e2;
        const uint8_t a = run_fold_bits(code, hd->n_code, t, u, se, &e1);
        const uint8_t b = group_fold(hd, code, t, u, se, &e2);
        if (a != b || e1 != e2) bad++;
    }
    return bad;
}
extern "C" int ht_eval_lean(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err) {
    return ht_eval_lean_row(h, doc, len, mis, res, err, nullptr);
}
// the byte-class masks of 32 bytes (LUT + transpose): out[c] = mask of class c
extern "C" void ht_lean_classes(const uint8_t* bytes, uint32_t* out) {
    uint32_t d[8];
    for (int j = 0; j < 8; j++) {
        uint32_t x;
        std::memcpy(&x, bytes + 4 * j, 4);
        d[j] = lean::classify4(x);
    }
    lean::transpose(d);
    for (uint32_t c = 0; c < 8; c++) out[c] = d[lean::creg(c)];
}

// the lean walk's trace of the next scans (sub-window << 8 | token kind per iteration, see
// AJX_LEAN_TRACE) into buf[cap]; returns the entries written so far (buf null: stop)
extern "C" uint32_t ht_lean_trace(uint32_t* buf, uint32_t cap) {
    const uint32_t n = lean::g_lean_trace_n;
    lean::g_lean_trace = buf;
    lean::g_lean_trace_cap = cap;
    lean::g_lean_trace_n = 0;
    lean::g_lean_subs = 0;
    return n;
}
extern "C" void ht_lean_counts(uint64_t* iters, uint64_t* subs) {
    *iters = lean::g_lean_iters;
    *subs = lean::g_lean_subs;
}

// ---- the streaming scan (ajx_stream.h) on 64 host threads per wave (ajx_wave.h) ----
#include "../../authorino_amd/csrc/ajx_stream.h"

// every request of the batch through the stream kernel's code, one span (wave) at a time,
// then stage B (finish_full) for those it hands over; out_slow[r] = 1 where the exact scan
// decides request r (outputs unset), 2 where stage B decided it. mode 1: structure only
// (out_tri[r] = proved). Returns -1 when the ruleset has no stream tables.
extern "C" int ht_eval_stream(void* h, const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                              uint8_t* out_tri, int32_t* out_err, uint64_t* out_bm, uint32_t stride, uint8_t* out_slow,
                              int mode, uint32_t* out_dbg, uint32_t per) {
    const std::vector<uint8_t>& blob_v = ((HtRuleset*)h)->c.blob;
    const RulesetHdr* hd = (const RulesetHdr*)blob_v.data();
    if (!hd->off_stream) return -1;
    // (16-byte aligned copy, as in LDS)
    std::vector<uint64_t> blob_buf((blob_v.size() + 7) / 8 + 2);
    std::memcpy(blob_buf.data(), blob_v.data(), blob_v.size());
    const uint8_t* blob = (const uint8_t*)blob_buf.data();
    const uint32_t ns = reinterpret_cast<const StreamHdr*>(blob_v.data() + hd->off_stream)->n_rec;  // (records)
    if (per == 0 || per > stream::kSpan) per = stream::kSpan;
    const uint32_t spans = (n + per - 1) / per;
    std::vector<uint64_t> wl(stream::lds_bytes(ns) / 8 + 2);
    std::vector<uint64_t> stage_rows((size_t)n * (5 + ns));
    std::vector<uint32_t> stage_list;
    for (uint32_t span = 0; span < spans; span++) {
        std::memset(wl.data(), 0xA5, wl.size() * 8);
        stream::WaveLds& L = *reinterpret_cast<stream::WaveLds*>(wl.data());
        uint64_t* rows = wl.data() + sizeof(stream::WaveLds) / 8;
        std::mutex mu;
        // (as the kernel's LAT instance for small batches: per < 32)
        const bool lat = per < stream::kSpan;
        wave::run_wave([&](uint32_t l) {
            const uint64_t *rowp = nullptr, *dwp = nullptr;
            const uint8_t* lds_doc = nullptr;
            uint32_t res;
            if (mode == 1)
                res = stream::scan_span<1>(L, rows, blob, arena, offs, lens, n, span, per, l, out_tri, out_err,
                                           out_bm, stride, &rowp, &dwp);
            else
                res = stream::scan_span<0>(L, rows, blob, arena, offs, lens, n, span, per, l, out_tri, out_err,
                                           out_bm, stride, &rowp, &dwp, lat ? &lds_doc : nullptr);
            const uint32_t r = span * per + l;
            // (one request per wave: the whole wave runs its stage B, as the kernel does)
            if (lat && per == 1 && wave::readlane(res == stream::R_STAGE_B && lds_doc ? 1u : 0u, 0) != 0) {
                auto bcast = [](const void* q) {
                    const uint64_t v = (uint64_t)(uintptr_t)q;
                    return (uintptr_t)((uint64_t)wave::readlane((uint32_t)v, 0) |
                                       ((uint64_t)wave::readlane((uint32_t)(v >> 32), 0) << 32));
                };
                const uint8_t* d0 = reinterpret_cast<const uint8_t*>(bcast(lds_doc));
                uint64_t* row0 = reinterpret_cast<uint64_t*>(bcast(rowp));
                const uint64_t* dw0 = reinterpret_cast<const uint64_t*>(bcast(dwp));
                const bool ok = stream::finish_full<true>(span, blob, d0, lens[span], RowRef(row0), out_tri, out_err,
                                                          out_bm, stride, dw0);
                if (l == 0) out_slow[span] = ok ? 2 : 1;
                return;
            }
            if (l >= per || r >= n) return;
            out_slow[r] = res == stream::R_SLOW ? 1 : 0;
            if (res == stream::R_STAGE_B && lds_doc) {  // stage B on the ring's copy of the document
                const bool ok = stream::finish_full(r, blob, lds_doc, lens[r], RowRef(const_cast<uint64_t*>(rowp)),
                                                    out_tri, out_err, out_bm, stride, dwp);
                out_slow[r] = ok ? 2 : 1;
                return;
            }
            if (res == stream::R_STAGE_B) {
                uint64_t* o = stage_rows.data() + (size_t)r * (5 + ns);
                std::memcpy(o, rowp, (1 + ns) * 8);
                std::memcpy(o + 1 + ns, dwp, 4 * 8);
                std::lock_guard<std::mutex> g(mu);
                stage_list.push_back(r);
            }
            if (out_dbg) {  // (bad position, root close)
                out_dbg[2 * r] = L.bad[l];
                out_dbg[2 * r + 1] = L.root_end[l];
            }
        });
    }
    for (uint32_t r : stage_list) {
        RowRef row(stage_rows.data() + (size_t)r * (5 + ns));
        const bool ok = stream::finish_full(r, blob, arena + offs[r], lens[r], row, out_tri, out_err, out_bm, stride);
        out_slow[r] = ok ? 2 : 1;
    }
    return 0;
}

// the launch plan (ajx_plan.h): which kernel a batch gets, as the library decides it
#include "../../authorino_amd/csrc/ajx_plan.h"
extern "C" void ht_plan_eval(const ajx::PlanIn* in, ajx::EvalPlan* out) { *out = ajx::plan_eval(*in); }
extern "C" int ht_mode_known(int mode) { return ajx::mode_known(mode) ? 1 : 0; }
