// ajx_request.h — what the lane-per-request kernels do to one request, from its scan to its
// outputs: the exact scan (eval_scan_one), the token scanner's stage A (scan_request) and the
// select kernel's request (select_request). The kernels (ajx_kernels.hip, ajx_lean.hip) keep
// the indices, the staging and the launch bounds and call these; the test-only host build
// (tests/native/host_eval.cpp) calls the same text. (The lean kernels' request,
// lean_request, stands with its walker in ajx_lean.h, which ajx_kernels.hip does not compile.)
#pragma once
#include "ajx_fast.h"
#include "ajx_modifiers.h"
#include "ajx_wave.h"

namespace ajx {

// keep_rows (the stream and lean kernels' parameter), bit 0: every request's capture row is
// written, for authjx_select_from_eval_device. Each kernel names its own bit 1.
constexpr uint32_t kKeepRows = 1u;

constexpr int kSelCache = 32;  // resolved selector values kept per request
constexpr int kPatCache = 64;  // pattern results kept per request for the fold

// The exact scan (ajx_device.h gj_get; exact for arbitrary bytes) of request r: per selector
// an exact gjson.Get scan, the patterns, the fold.
// MODS: the rulesets of the batch have modifier chains (ajx_modifiers.h; mb: the
// work-item's three text buffers, the caller's scratch)
template <bool MODS>
AJX_HD void eval_scan_one(uint32_t r, const uint8_t* const* __restrict__ sets,
                          const uint32_t* __restrict__ set_of_req,
                          const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                          const uint32_t* __restrict__ lens, uint8_t* __restrict__ out_tri,
                          int32_t* __restrict__ out_err, uint64_t* __restrict__ out_bm,
                          uint32_t stride, [[maybe_unused]] ModBufs* mb) {
    const uint8_t* blob = sets[set_of_req ? set_of_req[r] : 0];
    const RulesetHdr* h = reinterpret_cast<const RulesetHdr*>(blob);
    const Selector* sels = reinterpret_cast<const Selector*>(blob + h->off_selectors);
    const Component* comps = reinterpret_cast<const Component*>(blob + h->off_components);
    const Pattern* pats = reinterpret_cast<const Pattern*>(blob + h->off_patterns);
    const uint32_t* code = reinterpret_cast<const uint32_t*>(blob + h->off_code);
    const uint8_t* lits = blob + h->off_literals;
    const uint8_t* doc = arena + offs[r];
    const uint32_t len = lens[r];

    const uint32_t ns = h->n_selectors, np = h->n_patterns;
    ValueRef vals[kSelCache];
    const bool cache_sel = ns <= (uint32_t)kSelCache;
    if (cache_sel)
        for (uint32_t s = 0; s < ns; s++)
            vals[s] = gj_get(doc, len, comps + sels[s].comp_begin, sels[s].comp_count, lits);

    auto value_of = [&](uint32_t p) -> ValueRef {
        if (cache_sel) return vals[pats[p].selector];
        const Selector& s = sels[pats[p].selector];
        return gj_get(doc, len, comps + s.comp_begin, s.comp_count, lits);
    };
    auto eval = [&](uint32_t p) -> uint8_t {
        const Pattern& pt = pats[p];
        if (pt.state != P_OK) return eval_pattern<true>(blob, pt, doc, ValueRef{0, 0, T_NULL, 0});
        if constexpr (MODS) {
            const Selector& sl = sels[pt.selector];
            const ValueRef v = value_of(p);
            if (v.esc == kValList) {  // a "#." list (no modifier chain after it)
                const uint8_t* rd;
                ValueRef rv;
                if (!build_list(blob, sl, doc, v, *mb, &rd, &rv)) return V_U;
                return eval_pattern<true>(blob, pt, rd, rv);
            }
            if (sl.mod_count) {
                const uint8_t* rd;
                ValueRef rv;
                if (!apply_modifiers(blob, sl, doc, value_of(p), *mb, &rd, &rv)) return V_U;
                return eval_pattern<true>(blob, pt, rd, rv);
            }
        }
        return eval_pattern<true>(blob, pt, doc, value_of(p));
    };

    uint8_t res[kPatCache];
    const bool cache_pat = np <= (uint32_t)kPatCache;
    if (out_bm) {
        uint64_t* row = out_bm + (size_t)r * stride;
        for (uint32_t w = 0; w < stride; w++) {
            uint64_t word = 0;
            for (uint32_t b = 0; b < 64; b++) {
                uint32_t p = w * 64 + b;
                if (p >= np) break;
                uint8_t v = eval(p);
                if (cache_pat) res[p] = v;
                if (v == V_T) word |= 1ull << b;
            }
            row[w] = word;
        }
    }
    if (cache_pat && !out_bm)
        for (uint32_t p = 0; p < np; p++) res[p] = eval(p);
    // one fold program per tree (a forest ruleset writes n_trees results per request)
    const uint32_t nt = h->pad1[0] ? h->pad1[0] : 1u;
    const uint32_t* rc = h->pad1[0] ? reinterpret_cast<const uint32_t*>(blob + h->pad1[1]) : nullptr;
    for (uint32_t k = 0; k < nt; k++) {
        const uint32_t* c = rc ? code + rc[2 * k] : code;
        const uint32_t len = rc ? rc[2 * k + 1] : h->n_code;
        int32_t ep;
        uint8_t t;
        if (cache_pat)
            t = run_fold(c, len, [&](uint32_t p) { return res[p]; }, &ep);
        else
            t = run_fold(c, len, eval, &ep);
        out_tri[(size_t)r * nt + k] = t;
        if (out_err) out_err[(size_t)r * nt + k] = ep;
    }
}

// a document's aligned 16-byte block, as one load
#if defined(__HIPCC__)
using Quad16 = uint4;
#else
struct alignas(16) Quad16 {
    uint32_t x, y, z, w;
};
#endif

// stage A for request r: single-pass scan into its capture row (false: slow list)
AJX_HD bool scan_request(const uint8_t* blob, const uint8_t* d, uint32_t len, RowRef row, const WinRing& ring) {
    const RulesetHdr* h = reinterpret_cast<const RulesetHdr*>(blob);
    if (!(h->flags & kFlagFastOk) || len >= (1u << 24)) {
        row[0] = kRowSlow;
        return false;
    }
    const Quad16* a4 = reinterpret_cast<const Quad16*>(d - ((uintptr_t)d & 15u));
    auto load = [&](uint32_t b, uint32_t nblk) -> Block16 {
        if (b < nblk) {
            const Quad16 v = a4[b];
            return Block16{v.x, v.y, v.z, v.w};
        }
        return Block16{0u, 0u, 0u, 0u};
    };
    return scan_doc(blob, blob_tables(blob), d, len, row, ring, load);
}

// gjson.Get per pattern selector for request r (work-item k): the exact device Get (gj_get)
// for each of the ruleset's patterns [p0, p0 + stride), or its capture record when the
// request has a row that is not slow; out[r * stride + q] = {start (relative to the
// document), len, type | esc << 8}. An UNSUPPORTED selector reports type 0xFF. TEXT: a
// selector with modifiers and a "#." list resolve to built text, copied into the request's
// slot text[r * text_stride ...] (select_value, ajx_modifiers.h; 0xFF when it does not fit);
// without TEXT they report 0xFF (the capture-row path of select_from_eval).
template <bool TEXT>
AJX_HD void select_request(uint32_t r, uint32_t k, const uint8_t* const* sets,
                           const uint32_t* set_of_req, const uint8_t* arena,
                           const uint64_t* offs, const uint32_t* lens,
                           uint32_t* out, uint32_t stride, const uint64_t* rows,
                           uint32_t row_stride, uint32_t p0, uint32_t wave_rows, uint8_t* text,
                           uint32_t text_stride) {
    // the single-pass scan's capture row when it has one (not on the slow list): row k of the
    // wave-interleaved layout (wave_rows: the fused kernels') or row r
    const RowRef row = !rows ? RowRef() : wave_rows ? wave_row(const_cast<uint64_t*>(rows), row_stride, k)
                                                    : RowRef(rows + (size_t)r * row_stride);
    const uint64_t found = rows ? row[0] : kRowSlow;
    const uint8_t* blob = sets[set_of_req ? set_of_req[r] : 0];
    const RulesetHdr* h = reinterpret_cast<const RulesetHdr*>(blob);
    const Selector* sels = reinterpret_cast<const Selector*>(blob + h->off_selectors);
    const Component* comps = reinterpret_cast<const Component*>(blob + h->off_components);
    const Pattern* pats = reinterpret_cast<const Pattern*>(blob + h->off_patterns);
    const uint8_t* lits = blob + h->off_literals;
    const uint8_t* doc = arena + offs[r];
    const uint32_t len = lens[r];
    // patterns [p0, p0 + stride): the whole ruleset (p0 = 0) or, after a forest
    // evaluation, the response selectors compiled as its last tree
    const uint32_t avail = h->n_patterns > p0 ? h->n_patterns - p0 : 0u;
    const uint32_t np = avail < stride ? avail : stride;
    [[maybe_unused]] uint32_t used = 0;  // (TEXT: bytes of the request's text slot taken)
    for (uint32_t q = 0; q < np; q++) {
        const uint32_t p = p0 + q;
        uint32_t* o = out + ((size_t)r * stride + q) * 3;
        const uint32_t si = pats[p].selector;
        if (pats[p].state == P_UNSUPPORTED || (!TEXT && sels[si].mod_count)) {
            o[0] = 0;
            o[1] = 0;
            o[2] = 0xFFu;
            continue;
        }
        if constexpr (TEXT) {
            if (sels[si].mod_count) {
                ModBufs mb;
                if (!select_value(blob, sels[si], doc, len, mb, text + (size_t)r * text_stride, text_stride, &used, o))
                    o[0] = 0, o[1] = 0, o[2] = 0xFFu;
                continue;
            }
        }
        if (!(found & kRowSlow)) {
            if ((found >> si) & 1u) {
                const uint64_t rec = row[1 + si];
                const uint32_t meta = (uint32_t)(rec >> 32);
                o[0] = (uint32_t)rec;
                o[1] = meta & 0xFFFFFFu;
                o[2] = ((meta >> 24) & 7u) | (((meta >> 27) & 1u) << 8);
            } else {
                o[0] = 0;
                o[1] = 0;
                o[2] = T_NULL;
            }
            continue;
        }
        const Selector& sl = sels[si];
        const ValueRef v = gj_get(doc, len, comps + sl.comp_begin, sl.comp_count, lits);
        o[0] = v.start;
        o[1] = v.end - v.start;
        o[2] = (uint32_t)v.type | ((uint32_t)v.esc << 8);
        if (v.esc == kValList) {  // a "#." list: built text (without TEXT: not selectable)
            o[2] = 0xFFu;
            if constexpr (TEXT) {
                ModBufs mb;
                if (!select_value(blob, sl, doc, len, mb, text + (size_t)r * text_stride, text_stride, &used, o))
                    o[0] = 0, o[1] = 0, o[2] = 0xFFu;
            }
        }
    }
}

}  // namespace ajx
