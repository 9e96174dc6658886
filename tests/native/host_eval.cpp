// host_eval.cpp — TEST-ONLY harness. Compiles the kernels' per-document logic
// (authorino_amd/csrc/ajx_device.h) and the reconcile-time compiler for the host CPU so
// the CPU test suite can check them against the oracle without a GPU. It is not part
// of libauthjx.so and is never used by the product path (which has no CPU fallback).
// What the kernels do to one request or one span it calls as the kernels do, from
// ajx_request.h, ajx_lean.h (lean_request) and ajx_stream_body.h: it holds no copy of those
// bodies.
#define AJX_HD inline
#include <cstring>
#include <string>
#include <vector>

#include "../../authorino_amd/csrc/ajx_compiler.h"
#define AJX_LEAN_COUNT 1
#include "../../authorino_amd/csrc/ajx_lean.h"
#include "../../authorino_amd/csrc/ajx_request.h"
#include "../../authorino_amd/csrc/ajx_regex.h"

using namespace ajx;

struct HtRuleset {
    CompiledRuleset c;
    // the same patterns as a forest of one-pattern trees: the exact scan of it writes every
    // pattern's tri-state as a tree's result (ht_eval's res[]). Empty when it did not compile
    // or is not one tree per pattern of c: ht_eval then reads res[] as stage_b() reads a
    // bitmap (T bit, static E, unsupported, else F), which hides runtime U and E
    CompiledRuleset probe;
};

// (pats: the ruleset's patterns in order)
static void build_probe(HtRuleset* r, const std::vector<authjx_pattern>& pats) {
    std::vector<authjx_node> leaf(pats.size());
    std::vector<authjx_tree> trees(pats.size());
    for (size_t p = 0; p < pats.size(); p++) {
        leaf[p] = authjx_node{AUTHJX_NODE_PATTERN, -1, -1, 0};
        trees[p] = authjx_tree{&pats[p], 1, &leaf[p], 1, 0};
    }
    std::string e;
    if (pats.empty() || compile_forest(trees.data(), (uint32_t)trees.size(), &r->probe, &e) != AUTHJX_OK ||
        r->probe.n_patterns != r->c.n_patterns ||
        ((const RulesetHdr*)r->probe.blob.data())->pad1[0] != r->c.n_patterns)  // (one result per pattern)
        r->probe = CompiledRuleset();
}

// the exact scan's body (eval_scan_one, the instance the launcher takes for the ruleset) for
// one document: tri / err per tree, bm (or null) of `stride` words
static void exact_one(const uint8_t* blob, const uint8_t* doc, uint32_t len, int mods, uint8_t* tri, int32_t* err,
                      uint64_t* bm, uint32_t stride) {
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    const uint8_t* sets[1] = {blob};
    const uint64_t offs[1] = {0};
    const uint32_t lens[1] = {len};
    if (mods < 0) mods = hd->n_modifiers != 0 || (hd->flags & kFlagBufs) != 0;
    if (mods) {
        static thread_local ModBufs mb;  // (the kernel's work-item scratch)
        eval_scan_one<true>(0, sets, nullptr, doc, offs, lens, tri, err, bm, stride, &mb);
    } else {
        eval_scan_one<false>(0, sets, nullptr, doc, offs, lens, tri, err, bm, stride, nullptr);
    }
}

extern "C" {

void* ht_compile(const authjx_tree* tree, int32_t* status, char* err, size_t cap, int* rc) {
    HtRuleset* r = new HtRuleset();
    std::string e;
    *rc = compile_tree(tree, &r->c, &e);
    if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
    if (*rc != AUTHJX_OK) { delete r; return nullptr; }
    if (status)
        for (uint32_t i = 0; i < r->c.n_patterns; i++) status[i] = r->c.pattern_status[i];
    build_probe(r, std::vector<authjx_pattern>(tree->patterns, tree->patterns + tree->n_patterns));
    return r;
}

// a forest (authjx_compile_forest): trees[n], one fold program each
void* ht_compile_forest(const authjx_tree* trees, uint32_t n, char* err, size_t cap, int* rc) {
    HtRuleset* r = new HtRuleset();
    std::string e;
    *rc = compile_forest(trees, n, &r->c, &e);
    if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
    if (*rc != AUTHJX_OK) { delete r; return nullptr; }
    std::vector<authjx_pattern> pats;
    for (uint32_t k = 0; k < n; k++) pats.insert(pats.end(), trees[k].patterns, trees[k].patterns + trees[k].n_patterns);
    build_probe(r, pats);
    return r;
}

void ht_free(void* h) { delete (HtRuleset*)h; }

// The exact scan of one document as its kernel runs it (eval_scan_one): the tri-state (a
// forest: of its whole fold code over res[]); res[p] receives each pattern's tri-state, from
// the T bitmap the body wrote and, where that says not T, from the probe forest's results
// (without a probe: static E, unsupported, else F, as stage_b() reads a bitmap).
// 99 (no tri-state): the two disagree on a T bit.
int ht_eval(void* h, const uint8_t* doc_in, uint32_t len, uint8_t* res, int32_t* err) {
    // (the device reads whole aligned blocks around a document: give the copy that slack)
    std::vector<uint8_t> buf(len + 32, 0);
    uint8_t* doc = buf.data() + 16;
    if (len) std::memcpy(doc, doc_in, len);
    const HtRuleset* rs = (const HtRuleset*)h;
    const uint8_t* blob = rs->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    const uint32_t np = hd->n_patterns, slots = hd->pad1[0] ? hd->pad1[0] : 1u, stride = (np + 63u) / 64u + 1u;
    std::vector<uint8_t> tri(slots, 0xEE), ptri(np ? np : 1u, 0xEE);
    std::vector<int32_t> ep(slots, -7);
    std::vector<uint64_t> bm(stride, ~0ull);
    exact_one(blob, doc, len, -1, tri.data(), ep.data(), bm.data(), stride);
    const bool probe = !rs->probe.blob.empty();
    if (probe) exact_one(rs->probe.blob.data(), doc, len, -1, ptri.data(), nullptr, nullptr, 0);
    for (uint32_t p = 0; p < np; p++) {
        const uint64_t bit = 1ull << (p & 63);
        const bool t = (bm[p >> 6] & bit) != 0;
        if (probe) {
            if (t != (ptri[p] == V_T)) return 99;
            res[p] = ptri[p];
        } else {
            res[p] = t ? V_T : p < 128 && (hd->static_error[p >> 6] & bit) ? V_E
                             : p < 128 && (hd->unsupported[p >> 6] & bit)  ? V_U
                                                                           : V_F;
        }
    }
    if (bm[stride - 1]) return 99;  // (a word past the ruleset's patterns: zero)
    if (hd->pad1[0])
        return run_fold((const uint32_t*)(blob + hd->off_code), hd->n_code, [&](uint32_t p) { return res[p]; }, err);
    *err = ep[0];
    return tri[0];
}

// eval_scan_one for one document, the instance and the outputs named: mods 0 / 1 (-1: as the
// launcher, by the ruleset), stride words of bitmap at bm (0: no bitmap), tri / err per tree
void ht_eval_exact(void* h, const uint8_t* doc_in, uint32_t len, int mods, uint32_t stride, uint8_t* tri, int32_t* err,
                   uint64_t* bm) {
    std::vector<uint8_t> buf(len + 32, 0);
    uint8_t* doc = buf.data() + 16;
    if (len) std::memcpy(doc, doc_in, len);
    exact_one(((HtRuleset*)h)->c.blob.data(), doc, len, mods, tri, err, stride ? bm : nullptr, stride);
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

// What a single-pass body (scan_request + finish_request, lean_request) wrote for request 0:
// res[p] is read back from it (static E, unsupported, the T bitmap of kOutStride words).
// Returns 99 (no tri-state: the test's comparison fails) when a tree's result is not the
// code interpreter's on res, or a bitmap word past the ruleset's two was not zeroed; else
// the interpreter's tri-state of the fold code.
constexpr uint32_t kOutStride = 4;  // (the ruleset's two words and two the writer must zero)
struct Outs {
    uint64_t bm[kOutStride];
    std::vector<uint8_t> tri;
    std::vector<int32_t> ep;
    explicit Outs(const RulesetHdr* hd) : tri(hd->pad1[0] ? hd->pad1[0] : 1u, 0xEE), ep(tri.size(), -7) {
        std::memset(bm, 0xFF, sizeof bm);
    }
};
static int read_outs(const uint8_t* blob, const Outs& o, uint8_t* res, int32_t* err, bool count) {
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    const uint32_t nt = hd->pad1[0];
    if (o.bm[2] | o.bm[3]) return 99;
    for (uint32_t p = 0; p < hd->n_patterns; p++) {
        const uint64_t bit = 1ull << (p & 63);
        const uint32_t k = p >> 6;
        res[p] = (hd->static_error[k] & bit) ? V_E : (hd->unsupported[k] & bit) ? V_U : (o.bm[k] & bit) ? V_T : V_F;
    }
    if (count && (hd->flags & kFlagFlatFold)) g_flat_folds++;
    if (count && (hd->flags & kFlagGroupFold)) g_group_folds++;
    const uint32_t* code = (const uint32_t*)(blob + hd->off_code);
    const auto rp = [&](uint32_t p) { return res[p]; };
    const int whole = run_fold(code, hd->n_code, rp, err);
    if (nt == 0) return o.tri[0] == whole && o.ep[0] == *err ? whole : 99;
    const uint32_t* rc = (const uint32_t*)(blob + hd->pad1[1]);
    for (uint32_t k = 0; k < nt; k++) {  // (a forest: tree by tree)
        int32_t e;
        if (o.tri[k] != run_fold(code + rc[2 * k], rc[2 * k + 1], rp, &e) || o.ep[k] != e) return 99;
    }
    return whole;
}

extern "C" {
// single-pass path: returns -1 when the document is handed to the exact scan, else the
// tri-state; res[p] receives each pattern's value. `mis` places the copy at that
// misalignment (0..15) like an arbitrary arena offset.
static int eval_single_pass(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                            uint64_t* row_out);
int ht_eval_fast(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err) {
    return eval_single_pass(h, doc, len, mis, res, err, nullptr);
}
// the token scanner with its capture row (row_out: 1 + n_selectors)
int ht_eval_tok(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                uint64_t* row_out) {
    return eval_single_pass(h, doc, len, mis, res, err, row_out);
}
// (ajx_scan_fused's request: scan_request, then finish_request)
static int eval_single_pass(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                            uint64_t* row_out) {
    const uint8_t* blob = ((HtRuleset*)h)->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    if (!(hd->flags & kFlagFastOk)) return -2;
    std::vector<uint8_t> buf(len + 64, 0);
    uintptr_t base = ((uintptr_t)buf.data() + 15) & ~(uintptr_t)15;
    uint8_t* d = (uint8_t*)base + (mis & 15);
    std::memcpy(d, doc, len);
    std::vector<uint64_t> row(1 + hd->n_selectors, 0xDEADBEEFDEADBEEFull);
    alignas(16) uint8_t ring_mem[128];
    std::memset(ring_mem, 0x5A, sizeof ring_mem);
    WinRing ring{ring_mem, 0u, 16u};
    const RowRef rr(row.data());
    if (!scan_request(blob, d, len, rr, ring)) return row[0] == kRowSlow ? -1 : 99;
    if (row_out) std::memcpy(row_out, row.data(), row.size() * sizeof(uint64_t));
    Outs o(hd);
    if (!finish_request(0, blob, d, rr, o.tri.data(), o.ep.data(), o.bm, kOutStride)) return -1;
    return read_outs(blob, o, res, err, false);
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
// arr = 1: the array-walking instance for every ruleset (the one ajx_scan_lean takes without
// a staged blob, and the tenant kernel); 0: by the ruleset's kLeanArr, as launch_lean
static bool g_lean_arr = false;
extern "C" void ht_lean_arr(int arr) { g_lean_arr = arr != 0; }
extern "C" int ht_eval_lean_row(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                                uint64_t* row_out) {
    const uint8_t* blob = ((HtRuleset*)h)->c.blob.data();
    const RulesetHdr* hd = (const RulesetHdr*)blob;
    if (!(hd->flags & kFlagFastOk)) return -2;
    std::vector<uint8_t> buf(len + 96, 0x7A);  // (neighbour bytes around the document)
    uintptr_t base = ((uintptr_t)buf.data() + 15) & ~(uintptr_t)15;
    uint8_t* d = (uint8_t*)base + (mis & 15);
    std::memcpy(d, doc, len);
    std::vector<uint64_t> row(1 + hd->n_selectors, 0xDEADBEEFDEADBEEFull);
    const uint8_t* a = d - (mis & 15);
    const uint32_t nb = (uint32_t)((buf.data() + buf.size() - a) / 16);
    // the wave's ring (chunk-major); this document's lane: mis * 5 (every lane offset used)
    static thread_local std::vector<uint8_t> ring_mem(lean::kRingBytesPerWave);
    std::memset(ring_mem.data(), 0x5A, ring_mem.size());
    const uint32_t nblk = (len + (mis & 15) + 15) / 16;
    lean::CopyLoader ld{a, nblk, nb, ring_mem.data() + ((mis * 5u) & 63u) * 16u};
    uint64_t dec[2] = {0, 0};
    const RowRef rr(row.data());
    // (the kernels' request, lean_request; the instance launch_lean takes for this ruleset,
    // RulesetHdr::lean_feat, or the array-walking one, ht_lean_arr; stage B's values from the
    // lane's span buffer, as the kernel)
    Outs o(hd);
    uint32_t slow_count = 0, slow_id = ~0u;
    if (g_lean_arr || (hd->lean_feat & kLeanArr))
        lean_request<0, true>(0, 0, blob, d, len, rr, ld.lane_ring, ld.lane_ring, ld, g_lean_keep, &slow_count, &slow_id,
                              o.tri.data(), o.ep.data(), o.bm, kOutStride, dec);
    else
        lean_request<0, false>(0, 0, blob, d, len, rr, ld.lane_ring, ld.lane_ring, ld, g_lean_keep, &slow_count,
                               &slow_id, o.tri.data(), o.ep.data(), o.bm, kOutStride, dec);
    g_last_dec[0] = dec[0];
    g_last_dec[1] = dec[1];
    // handed to the exact scan: one list entry, the row marked
    if (slow_count) return slow_count == 1 && slow_id == 0 && row[0] == kRowSlow ? -1 : 99;
    if (row_out) std::memcpy(row_out, row.data(), row.size() * sizeof(uint64_t));
    return read_outs(blob, o, res, err, true);
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

// ---- the streaming kernels' bodies (ajx_stream_body.h) on 64 host threads per wave (ajx_wave.h) ----
#include "../../authorino_amd/csrc/ajx_stream_body.h"

// a 16-byte aligned copy of a ruleset's blob (as the device's)
static std::vector<uint64_t> aligned_blob(const std::vector<uint8_t>& b) {
    std::vector<uint64_t> v((b.size() + 7) / 8 + 2);
    std::memcpy(v.data(), b.data(), b.size());
    return v;
}

// Every request of the batch through the streaming kernels' code, as launch_eval_stream
// runs them: stream_body per span (wave), the workgroup's LDS laid out as the kernel's; then
// the stage-B list by stream_fin_list (fin) or stream_finish_entry, and, without merge_slow,
// the exact scan over the slow list. out_slow[r] = 0 where the stream decided request r, 2
// where stage B did, 1 where the exact scan did. mode 1: structure only (out_tri[r] = proved,
// no lists).
//   h2, set_of_req: a second ruleset (the MT instance: per = 1, request r under
//     set_of_req[r] ? h2 : h); mt_wave_off: the room of a wave's own blob copy (0: the blob is
//     read in place)
//   keep_rows: every request's row is kept in rows (the wave layout, row_stride >= 5 + n_rec
//     words; null: a buffer of the harness's)
//   merge_slow: -1 as the launcher (per < 32 or MT), else 0 / 1
//   lists (optional, 4 + 2 n words): [0] slow and [1] stage-B counts after the spans, [2] the
//     final slow count, [3] the slow list's length; the stage-B list's entries from [4], the
//     slow ids from [4 + n]
// Returns -1 when a ruleset has no stream tables, -3 for a combination the launcher never makes.
extern "C" int ht_eval_stream(void* h, void* h2, const uint32_t* set_of_req, uint32_t mt_wave_off,
                              const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                              uint8_t* out_tri, int32_t* out_err, uint64_t* out_bm, uint32_t stride, uint8_t* out_slow,
                              int mode, uint32_t* out_dbg, uint32_t per, uint32_t keep_rows, int merge_slow, int fin,
                              uint64_t* rows_io, uint32_t row_stride, uint32_t* lists) {
    const bool mt = h2 != nullptr;
    std::vector<uint64_t> blobs[2] = {aligned_blob(((HtRuleset*)h)->c.blob),
                                      aligned_blob(((HtRuleset*)(mt ? h2 : h))->c.blob)};
    const uint8_t* sets[2] = {(const uint8_t*)blobs[0].data(), (const uint8_t*)blobs[1].data()};
    uint32_t ns = 0, blob_bytes = 0;
    bool mods = false;
    for (const uint8_t* b : sets) {
        const RulesetHdr* hd = (const RulesetHdr*)b;
        if (!hd->off_stream) return -1;
        const uint32_t k = reinterpret_cast<const StreamHdr*>(b + hd->off_stream)->n_rec;  // (records)
        ns = k > ns ? k : ns;
        blob_bytes = hd->total_bytes > blob_bytes ? hd->total_bytes : blob_bytes;
        mods = mods || hd->n_modifiers != 0 || (hd->flags & kFlagBufs) != 0;
    }
    if (mt) per = 1;
    if (per == 0 || per > stream::kSpan) per = stream::kSpan;
    const bool merge = merge_slow < 0 ? (mt || per < stream::kSpan) : merge_slow != 0;
    const bool lat = merge && !keep_rows;  // (the kernel's LAT instance, as the launcher picks it)
    if ((mt && (mode != 0 || !merge)) || (fin && (!lat || mods))) return -3;
    // the workgroup's dynamic LDS: [blob copy] [per wave: WaveLds, rows]; MT: per wave
    // [room for its blob] [WaveLds, rows]
    constexpr uint32_t kWaves = 4;
    uint32_t wave_off = mt ? (mt_wave_off + 15u) & ~15u : (blob_bytes + 15u) & ~15u;
    uint32_t wave_bytes = ((stream::lds_bytes(ns) + 15u) & ~15u) + (mt ? wave_off : 0u);
    std::vector<uint64_t> dyn_mem(((mt ? 0u : wave_off) + kWaves * wave_bytes) / 8 + 2);
    uint8_t* dyn = (uint8_t*)dyn_mem.data();
    if (row_stride == 0) row_stride = 5 + ns;
    if (row_stride < 5 + ns) return -3;
    std::vector<uint64_t> own_rows(rows_io ? 0 : (size_t)((n + 63u) & ~63u) * row_stride);
    uint64_t* rows = rows_io ? rows_io : own_rows.data();
    // the counters and the slow ids in one buffer, the stage-B list in another (the workspace's)
    std::vector<uint32_t> slow_buf(n + kStreamCounterWords, 0), stage_list(n + 1, 0);
    StreamCounters* ctr = stream_counters(slow_buf.data());
    uint32_t* slow_ids = stream_slow_ids(slow_buf.data());
    const uint32_t* sor = mt ? set_of_req : nullptr;
    const uint32_t spans = (n + per - 1) / per;
    const uint32_t keep = keep_rows ? kKeepRows : 0u;
    for (uint32_t span = 0; span < spans; span++) {
        const uint32_t w = span % kWaves;
        std::memset(dyn, 0xA5, dyn_mem.size() * 8);
        if (!mt) std::memcpy(dyn, sets[0], blob_bytes);  // (stage_blob<true>)
        wave::run_wave([&](uint32_t l) {
            uint32_t d;
#define AJX_BODY(M, T, LT)                                                                                          \
    stream_body<M, T, LT>(sets, sor, arena, offs, lens, n, ctr, slow_ids, stage_list.data(), out_tri, out_err, out_bm,  \
                          stride, wave_off, wave_bytes, rows, row_stride, keep, per, merge ? 1u : 0u, dyn, w, l, span,  \
                          mt ? nullptr : dyn, 0ull)
            if (mode == 1) d = AJX_BODY(1, false, false);
            else if (mt) d = lat ? AJX_BODY(0, true, true) : AJX_BODY(0, true, false);
            else d = lat ? AJX_BODY(0, false, true) : AJX_BODY(0, false, false);
#undef AJX_BODY
            const uint32_t r = span * per + l;
            if (d != kDispNone) out_slow[r] = (uint8_t)d;
        });
        if (out_dbg) {  // (bad position, root close)
            const stream::WaveLds& L =
                *reinterpret_cast<const stream::WaveLds*>(mt ? dyn + w * wave_bytes + wave_off : dyn + wave_off + w * wave_bytes);
            for (uint32_t l = 0; l < per && span * per + l < n; l++) {
                out_dbg[2 * (span * per + l)] = L.bad[l];
                out_dbg[2 * (span * per + l) + 1] = L.root_end[l];
            }
        }
    }
    if (lists) {
        lists[0] = ctr->slow;
        lists[1] = ctr->stage_b;
        for (uint32_t i = 0; i < ctr->stage_b; i++) lists[4 + i] = stage_list[i];
    }
    if (mode != 0) return 0;
    // the stage-B list, an entry at a time: where stage B could not decide the request the
    // slow count moved (and, without merge_slow, the slow list got it)
    const uint32_t cnt = ctr->stage_b;
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t before = ctr->slow, e = stage_list[i];
        if (fin) {  // (lane 0's share of a one-entry list)
            if (mt) stream_fin_list<true>(sets, sor, arena, offs, lens, 1u, ctr, &stage_list[i], out_tri, out_err, out_bm, stride, rows, row_stride, 0u);
            else stream_fin_list<false>(sets, sor, arena, offs, lens, 1u, ctr, &stage_list[i], out_tri, out_err, out_bm, stride, rows, row_stride, 0u);
        } else {
#define AJX_ENTRY(T, X)                                                                                             \
    stream_finish_entry<T, X>(e, sets[0], sets, sor, arena, offs, lens, rows, row_stride, ctr, slow_ids, out_tri, out_err, \
                              out_bm, stride)
            if (mt && mods) AJX_ENTRY(true, 2);
            else if (mt) AJX_ENTRY(true, 1);
            else if (merge && mods) AJX_ENTRY(false, 2);
            else if (merge) AJX_ENTRY(false, 1);
            else AJX_ENTRY(false, 0);
#undef AJX_ENTRY
        }
        if ((e & kStageExact) || ctr->slow != before) out_slow[e & ~kStageExact] = 1;
    }
    if (!merge) {  // (ajx_eval_scan_list over the slow list)
        const uint32_t trees = ((const RulesetHdr*)sets[0])->pad1[0];
        const uint32_t nt = trees ? trees : 1u;
        for (uint32_t i = 0; i < ctr->slow; i++) {
            const uint32_t r = slow_ids[i];
            exact_one(sets[0], arena + offs[r], lens[r], mods, out_tri + (size_t)r * nt, out_err + (size_t)r * nt,
                      out_bm ? out_bm + (size_t)r * stride : nullptr, stride);
        }
    }
    if (lists) {
        lists[2] = ctr->slow;
        lists[3] = merge ? 0u : ctr->slow;  // (ids on the slow list: with merge_slow it only counts)
        for (uint32_t i = 0; i < lists[3]; i++) lists[4 + n + i] = slow_ids[i];
    }
    return 0;
}

// select_request (the select kernel's body) for every request of a batch under one ruleset:
// out[n][stride][3]; rows (or null: the exact Get) in the wave layout (wave_rows) or one per
// request; text (or null: the instance without TEXT) of text_stride bytes per request
extern "C" void ht_select_rows(void* h, const uint8_t* arena, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                               uint32_t* out, uint32_t stride, const uint64_t* rows, uint32_t row_stride, uint32_t p0,
                               uint32_t wave_rows, uint8_t* text, uint32_t text_stride) {
    std::vector<uint64_t> blob = aligned_blob(((HtRuleset*)h)->c.blob);
    const uint8_t* sets[1] = {(const uint8_t*)blob.data()};
    for (uint32_t r = 0; r < n; r++) {
        if (text)
            select_request<true>(r, r, sets, nullptr, arena, offs, lens, out, stride, rows, row_stride, p0, wave_rows, text,
                                 text_stride);
        else
            select_request<false>(r, r, sets, nullptr, arena, offs, lens, out, stride, rows, row_stride, p0, wave_rows,
                                  nullptr, 0u);
    }
}

// the launch plan (ajx_plan.h): which kernel a batch gets, as the library decides it
#include "../../authorino_amd/csrc/ajx_plan.h"
extern "C" void ht_plan_eval(const ajx::PlanIn* in, ajx::EvalPlan* out) { *out = ajx::plan_eval(*in); }
extern "C" int ht_mode_known(int mode) { return ajx::mode_known(mode) ? 1 : 0; }
