// ajx_stageb.h — stage B, the step after every structural scan (ajx_fast.h, ajx_lean.h,
// ajx_stream.h): the capture-row format the scans write, Pattern.Matches
// (pkg/jsonexp/expressions.go:59-96) for every pattern on its selector's captured value
// (Null when not found), the T bitmap, and the And/Or fold of every tree
// (expressions.go:111-154) into the request's outputs.
//
// One work-item per request: patterns_from_row decides the patterns, write_bitmap and
// fold_outputs write the outputs, finish_request is the three in order. The folds read
// one- and two-level trees off the bitmaps (flat_fold, group_fold, tree_fold) and leave the
// rest to the interpreter (run_fold_bits, ajx_device.h).
//
// No HIP in this header: the kernels compile it as device code, the host test harness
// (tests/native) as plain C++, the same text either way (AJX_HD).
#pragma once
#include "ajx_device.h"

namespace ajx {

// capture row: [0] = header (bit 63: slow, bits 0..62: selector found), then one
// 8-byte record per selector: low = start, high = len (24 bits) | type << 24 | esc << 27
constexpr uint64_t kRowSlow = 1ull << 63;

// A capture row in memory: word j at p[j * es]. es = 1: the row's words are contiguous
// (rows indexed by request); es = 64: the wave-interleaved layout of the fused kernels,
// where word j of the 64 work-items of a wave is one 512-B run, so a wave's record
// stores share cache lines and stage B's row reads are coalesced (wave_row).
struct RowRef {
    uint64_t* p;
    uint32_t es;
    AJX_HD RowRef() : p(nullptr), es(1) {}
    AJX_HD RowRef(uint64_t* q, uint32_t e = 1) : p(q), es(e) {}
    AJX_HD RowRef(const uint64_t* q, uint32_t e = 1) : p(const_cast<uint64_t*>(q)), es(e) {}  // (read-only uses)
    AJX_HD uint64_t& operator[](uint32_t j) const { return p[(size_t)j * es]; }
};
// work-item k's row in the wave-interleaved layout of (1 + n_selectors)-word rows
AJX_HD RowRef wave_row(uint64_t* rows, uint32_t row_stride, uint32_t k) {
    return RowRef(rows + (size_t)(k & ~63u) * row_stride + (k & 63u), 64u);
}

// (bit helpers and the 16-byte block that the scans use as well)
AJX_HD uint32_t eq_bytes(uint32_t w, uint32_t c4) {  // 0x80 in every byte equal to c
    uint32_t t = w ^ c4;
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}
AJX_HD uint32_t le20_bytes(uint32_t w) {  // 0x80 in every byte <= 0x20
    uint32_t t = (w & 0x7F7F7F7Fu) + 0x5F5F5F5Fu;
    return ~(t | w) & 0x80808080u;
}

struct Block16 {
    uint32_t x, y, z, w;
};

AJX_HD uint32_t ctz64f(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }
AJX_HD uint32_t hibit64f(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }
AJX_HD uint32_t popc64f(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
AJX_HD uint64_t below64f(uint32_t i) { return i >= 64 ? ~0ull : ((1ull << i) - 1ull); }
AJX_HD uint64_t lt64(uint32_t i) { return (1ull << i) - 1ull; }  // bits below i, i < 64
AJX_HD uint64_t upto64(uint32_t i) { return ~0ull >> (63u - i); }  // bits 0..i, i < 64

// the 4 bytes at p when only `avail` (>= 1) of them are readable: no aligned dword past
// the one holding p[avail - 1] is touched (bytes past it are garbage)
AJX_HD uint32_t load_u32_upto(const uint8_t* p, uint32_t avail) {
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* q = (const uint32_t*)(p - sh);
    const uint32_t w0 = q[0];
    const uint32_t w1 = (sh && avail > 4u - sh) ? q[1] : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(w1, w0, sh);
#else
    return sh ? (w0 >> (8 * sh)) | (w1 << (32 - 8 * sh)) : w0;
#endif
}

// A JSON number that is its own FormatFloat(f, 'f', -1, 64) (gjson Result.String() of a
// non-integer Number): (0|[1-9][0-9]*)\.[0-9]*[1-9] with at most 15 digits in all — a
// decimal of <= 15 significant digits is the only such decimal that parses to its double,
// so the shortest round-trip digits are its own (the sign is handled by the caller).
AJX_HD bool simple_decimal(const uint8_t* s, uint32_t n) {
    if (n < 3 || n > 16) return false;
    uint32_t i = 0, nd = 0;
    if (s[0] == '0') {
        i = 1;
        nd = 1;
    } else {
        while (i < n && s[i] >= '0' && s[i] <= '9') i++;
        nd = i;
        if (i == 0) return false;
    }
    if (i >= n || s[i] != '.') return false;
    const uint32_t f0 = ++i;
    while (i < n && s[i] >= '0' && s[i] <= '9') i++;
    if (i != n || i == f0 || s[n - 1] == '0') return false;
    return nd + (n - f0) <= 15;
}

struct RawVal {
    uint32_t a, n;  // span in the document
    uint32_t lit;   // 0 span, kLitTrue / kLitFalse / kLitEmpty for the literals
    bool ok;        // false: the general path formats it
};
AJX_HD RawVal raw_value(const uint8_t* doc, const ValueRef& v) {
    RawVal r{v.start, v.end - v.start, 0u, true};
    switch (v.type) {
        case T_STRING:
            r.a = v.start + 1;
            r.n = v.end - v.start - 2;
            r.ok = !v.esc;
            break;
        case T_NUMBER: {
            uint32_t k = v.start;
            if (k < v.end && doc[k] == '-') k++;
            const uint32_t k0 = k;
            for (; k < v.end; k += 4) {  // -?[0-9]* is its own String()
                const uint32_t w = load_u32_upto(doc + k, v.end - k);
                const uint32_t m = v.end - k >= 4 ? 0xFFFFFFFFu : (1u << (8 * (v.end - k))) - 1u;
                const uint32_t d = w ^ 0x30303030u;
                if ((((d + 0x76767676u) | d) & 0x80808080u) & m) { r.ok = false; break; }
            }
            if (!r.ok) r.ok = simple_decimal(doc + k0, v.end - k0);
            break;
        }
        case T_TRUE: r.lit = kLitTrue; r.n = 4; break;
        case T_FALSE: r.lit = kLitFalse; r.n = 5; break;
        case T_JSON: break;
        default: r.lit = kLitEmpty; r.n = 0; break;  // Null: ""
    }
    return r;
}

// `matches` on a raw span: ASCII four bytes at a time, utf8.DecodeRune otherwise (the
// S_RAW branch of dfa_match without a StrSrc)
AJX_HD bool dfa_match_span(const uint8_t* blob, uint32_t dfa_off, const uint8_t* p, uint32_t n) {
    const DfaHdr* h = (const DfaHdr*)(blob + dfa_off);
    const uint16_t* tr = (const uint16_t*)(blob + h->trans_off);
    const uint32_t nc = h->n_classes, ms = h->match_state;
    uint32_t st = h->start;
    if (st == ms) return true;
    uint32_t i = 0;
    // 16 ASCII bytes per step: the five aligned dwords that hold them are loaded together
    // (one memory latency per 16 bytes instead of one per dword: the span was read by stage
    // A long before and has left the caches); every dword loaded holds a byte of the span
    while (i + 16 <= n) {
        const uint32_t sh = (uint32_t)((uintptr_t)(p + i) & 3u);
        const uint32_t* q = (const uint32_t*)(p + i - sh);
        const uint32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = sh ? q[4] : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t w[4] = {__builtin_amdgcn_alignbyte(a1, a0, sh), __builtin_amdgcn_alignbyte(a2, a1, sh),
                               __builtin_amdgcn_alignbyte(a3, a2, sh), __builtin_amdgcn_alignbyte(a4, a3, sh)};
#else
        const uint64_t s8 = 8ull * sh;
        const uint32_t w[4] = {(uint32_t)((((uint64_t)a1 << 32) | a0) >> s8), (uint32_t)((((uint64_t)a2 << 32) | a1) >> s8),
                               (uint32_t)((((uint64_t)a3 << 32) | a2) >> s8), (uint32_t)((((uint64_t)a4 << 32) | a3) >> s8)};
#endif
        if ((w[0] | w[1] | w[2] | w[3]) & 0x80808080u) break;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            st = tr[st * nc + h->ascii_class[(w[k >> 2] >> (8 * (k & 3))) & 0x7Fu]];
            if (st == ms) return true;
        }
        i += 16;
    }
    while (i < n) {
        if (i + 4 <= n) {
            const uint32_t w = load_u32_any(p + i);
            if (!(w & 0x80808080u)) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    st = tr[st * nc + h->ascii_class[(w >> (8 * k)) & 0x7Fu]];
                    if (st == ms) return true;
                }
                i += 4;
                continue;
            }
        }
        const uint32_t b0 = p[i];
        int32_t r = (int32_t)b0;
        uint32_t sz = 1;
        if (b0 >= 0x80) {
            r = 0xFFFD;
            uint32_t need = 0, lo = 0x80, hi = 0xBF, v = 0;
            if (b0 >= 0xC2 && b0 <= 0xDF) { need = 2; v = b0 & 0x1F; }
            else if (b0 >= 0xE0 && b0 <= 0xEF) {
                need = 3; v = b0 & 0x0F;
                if (b0 == 0xE0) lo = 0xA0;
                if (b0 == 0xED) hi = 0x9F;
            } else if (b0 >= 0xF0 && b0 <= 0xF4) {
                need = 4; v = b0 & 0x07;
                if (b0 == 0xF0) lo = 0x90;
                if (b0 == 0xF4) hi = 0x8F;
            }
            if (need && n - i >= need && p[i + 1] >= lo && p[i + 1] <= hi) {
                bool good = true;
                v = (v << 6) | (p[i + 1] & 0x3Fu);
                for (uint32_t k = 2; k < need; k++) {
                    const uint32_t c = p[i + k];
                    if (c < 0x80 || c > 0xBF) { good = false; break; }
                    v = (v << 6) | (c & 0x3Fu);
                }
                if (good) { r = (int32_t)v; sz = need; }
            }
        }
        i += sz;
        st = tr[st * nc + rune_class(h, blob, r)];
        if (st == ms) return true;
    }
    return blob[h->eot_off + st] != 0;
}
// `matches` on a literal's text ("true" / "false" / ""), from registers
AJX_HD bool dfa_match_lit(const uint8_t* blob, uint32_t dfa_off, uint32_t lit) {
    const DfaHdr* h = (const DfaHdr*)(blob + dfa_off);
    const uint16_t* tr = (const uint16_t*)(blob + h->trans_off);
    const uint32_t nc = h->n_classes, ms = h->match_state;
    uint32_t st = h->start;
    if (st == ms) return true;
    const uint64_t text = lit == kLitTrue ? 0x65757274ull : lit == kLitFalse ? 0x65736C6166ull : 0ull;
    const uint32_t n = lit == kLitTrue ? 4u : lit == kLitFalse ? 5u : 0u;
    for (uint32_t k = 0; k < n; k++) {
        st = tr[st * nc + h->ascii_class[(text >> (8 * k)) & 0x7Fu]];
        if (st == ms) return true;
    }
    return blob[h->eot_off + st] != 0;
}

// The gjson unescape of a string's contents as a byte stream (StrSrc::S_UNESC) with
// every byte of state in registers: the UTF-8 bytes of a \u escape wait packed in `pend`.
struct UnescSrc {
    const uint8_t* p;
    uint32_t i, n;
    uint32_t pend, npend;
    bool done;
    AJX_HD void init(const uint8_t* s, uint32_t a, uint32_t b) {
        p = s;
        i = a;
        n = b;
        pend = npend = 0;
        done = false;
    }
    AJX_HD int next() {
        if (npend) {
            const int c = (int)(pend & 0xFFu);
            pend >>= 8;
            npend--;
            return c;
        }
        if (done || i >= n) return -1;
        const uint8_t c = p[i];
        if (c < ' ') { done = true; return -1; }
        if (c != '\\') { i++; return c; }
        i++;
        if (i >= n) { done = true; return -1; }
        const uint8_t e = p[i];
        uint8_t out;
        switch (e) {
            case '\\': out = '\\'; break;
            case '/': out = '/'; break;
            case 'b': out = '\b'; break;
            case 'f': out = '\f'; break;
            case 'n': out = '\n'; break;
            case 'r': out = '\r'; break;
            case 't': out = '\t'; break;
            case '"': out = '"'; break;
            case 'u': {
                if (i + 5 > n) { done = true; return -1; }
                uint32_t r = hexval4(p + i + 1);
                i += 5;
                if (r >= 0xD800 && r < 0xE000) {
                    if (n - i >= 6 && p[i] == '\\' && p[i + 1] == 'u') {
                        const uint32_t r2 = hexval4(p + i + 2);
                        if (r < 0xDC00 && r2 >= 0xDC00 && r2 < 0xE000)
                            r = (((r - 0xD800) << 10) | (r2 - 0xDC00)) + 0x10000;
                        else
                            r = 0xFFFD;
                        i += 6;
                    }
                }
                // utf8_put, packed low byte first
                if (r > 0x10FFFF || (r >= 0xD800 && r <= 0xDFFF)) r = 0xFFFD;
                uint32_t b;
                uint32_t k;
                if (r < 0x80) { b = r; k = 1; }
                else if (r < 0x800) { b = (0xC0 | (r >> 6)) | ((0x80 | (r & 0x3F)) << 8); k = 2; }
                else if (r < 0x10000) {
                    b = (0xE0 | (r >> 12)) | ((0x80 | ((r >> 6) & 0x3F)) << 8) | ((0x80 | (r & 0x3F)) << 16);
                    k = 3;
                } else {
                    b = (0xF0 | (r >> 18)) | ((0x80 | ((r >> 12) & 0x3F)) << 8) | ((0x80 | ((r >> 6) & 0x3F)) << 16) |
                        ((0x80 | (r & 0x3F)) << 24);
                    k = 4;
                }
                pend = b >> 8;
                npend = k - 1;
                return (int)(b & 0xFFu);
            }
            default: done = true; return -1;
        }
        i++;
        return out;
    }
};

// stream == literal (UnescSrc)
AJX_HD bool unesc_equals(UnescSrc* s, const uint8_t* lit, uint32_t len) {
    for (uint32_t k = 0; k < len; k++)
        if (s->next() != (int)lit[k]) return false;
    return s->next() < 0;
}

// `matches` over a UnescSrc: utf8.DecodeRune over the stream with the (up to 4) bytes
// of lookahead packed in a register (RuneReader, without its arrays)
AJX_HD bool dfa_match_unesc(const uint8_t* blob, uint32_t dfa_off, UnescSrc* s) {
    const DfaHdr* h = (const DfaHdr*)(blob + dfa_off);
    const uint16_t* tr = (const uint16_t*)(blob + h->trans_off);
    const uint32_t nc = h->n_classes, ms = h->match_state;
    uint32_t st = h->start;
    if (st == ms) return true;
    uint32_t la = 0, nla = 0;
    for (;;) {
        while (nla < 4) {
            const int c = s->next();
            if (c < 0) break;
            la |= (uint32_t)c << (8 * nla);
            nla++;
        }
        if (nla == 0) break;
        const uint32_t b0 = la & 0xFFu;
        uint32_t sz = 1;
        int32_t r = (int32_t)b0;
        if (b0 >= 0x80) {
            r = 0xFFFD;
            uint32_t need = 0, lo = 0x80, hi = 0xBF, v = 0;
            if (b0 >= 0xC2 && b0 <= 0xDF) { need = 2; v = b0 & 0x1F; }
            else if (b0 >= 0xE0 && b0 <= 0xEF) {
                need = 3; v = b0 & 0x0F;
                if (b0 == 0xE0) lo = 0xA0;
                if (b0 == 0xED) hi = 0x9F;
            } else if (b0 >= 0xF0 && b0 <= 0xF4) {
                need = 4; v = b0 & 0x07;
                if (b0 == 0xF0) lo = 0x90;
                if (b0 == 0xF4) hi = 0x8F;
            }
            const uint32_t b1 = (la >> 8) & 0xFFu;
            if (need && nla >= need && b1 >= lo && b1 <= hi) {
                bool good = true;
                v = (v << 6) | (b1 & 0x3Fu);
                for (uint32_t k = 2; k < need; k++) {
                    const uint32_t c = (la >> (8 * k)) & 0xFFu;
                    if (c < 0x80 || c > 0xBF) { good = false; break; }
                    v = (v << 6) | (c & 0x3Fu);
                }
                if (good) { r = (int32_t)v; sz = need; }
            }
        }
        la = sz == 4 ? 0u : la >> (8 * sz);
        nla -= sz;
        st = tr[st * nc + rune_class(h, blob, r)];
        if (st == ms) return true;
    }
    return blob[h->eot_off + st] != 0;
}

// eq on a raw value
AJX_HD bool raw_equals(const uint8_t* doc, const RawVal& r, const Pattern& pt, const uint8_t* lits) {
    if (r.lit) return (pt.litf & r.lit) != 0;
    return r.n == pt.lit_len && bytes_equal(doc + r.a, lits + pt.lit_off, r.n);
}

// incl / excl of every such pattern of one selector, the array walked once: bit j of the
// result = pattern j of the selector's list found among the elements. Compact arrays of
// unescaped strings / integers / literals only; false sends the selector to the general
// path (whitespace, escapes, nested containers, non-integer numbers, a non-array value).
AJX_HD bool incl_hits(const uint8_t* doc, const ValueRef& v, const Pattern* pats, const uint16_t* plist,
                      uint32_t begin, uint32_t cnt, const uint8_t* lits, uint32_t* hits) {
    uint32_t h = 0;
    if (v.type != T_JSON || v.end - v.start < 2 || doc[v.start] != '[') return false;
    uint32_t i = v.start + 1;
    const uint32_t end = v.end - 1;  // the ']'
    if (doc[end] != ']') return false;
    while (i < end) {
        ValueRef e;
        const uint32_t c = doc[i];
        e.start = i;
        e.esc = 0;
        if (c == '"') {  // the closing quote: the first '"' or '\\' after i
            uint32_t k = i + 1;
            for (;;) {
                if (k >= end) return false;
                const uint32_t w = load_u32_upto(doc + k, end + 1 - k);
                const uint32_t m = end - k >= 4 ? 0xFFFFFFFFu : (1u << (8 * (end - k))) - 1u;
                const uint32_t f = (eq_bytes(w, 0x22222222u) | eq_bytes(w, 0x5C5C5C5Cu)) & m;
                if (f) {
                    k += (uint32_t)__builtin_ctz(f) >> 3;
                    break;
                }
                k += 4;
            }
            if (doc[k] != '"') return false;  // an escape
            e.end = k + 1;
            e.type = T_STRING;
        } else if (c == 't' || c == 'f' || c == 'n') {
            const uint32_t w = load_u32_upto(doc + i, end + 1 - i);
            if (w == 0x65757274u) { e.end = i + 4; e.type = T_TRUE; }
            else if (w == 0x6C6C756Eu) { e.end = i + 4; e.type = T_NULL; }
            else if (w == 0x736C6166u && i + 4 < end && doc[i + 4] == 'e') { e.end = i + 5; e.type = T_FALSE; }
            else return false;
        } else if (c == '-' || (c >= '0' && c <= '9')) {
            uint32_t k = i + 1;
            while (k < end && doc[k] != ',') {
                if (doc[k] <= ' ') return false;  // (gjson's number ends there: the general path)
                k++;
            }
            e.end = k;
            e.type = T_NUMBER;
        } else {
            return false;
        }
        const RawVal r = raw_value(doc, e);
        if (!r.ok) return false;
        if (!r.lit && r.n <= 8) {
            // a short element (the common case: group / role names): its bytes are read
            // from the document once, into two masked dwords, and compared with each
            // literal's dwords (4-byte aligned in the pool, LDS when the blob is staged)
            const uint32_t n0 = r.n < 4 ? r.n : 4u, n1 = r.n - n0;
            const uint32_t m0 = n0 == 4 ? 0xFFFFFFFFu : (1u << (8 * n0)) - 1u;
            const uint32_t m1 = n1 == 4 ? 0xFFFFFFFFu : (1u << (8 * n1)) - 1u;
            const uint32_t w0 = n0 ? load_u32_upto(doc + r.a, n0) & m0 : 0u;
            const uint32_t w1 = n1 ? load_u32_upto(doc + r.a + 4, n1) & m1 : 0u;
            for (uint32_t j = 0; j < cnt; j++) {
                const Pattern pt = pats[plist[begin + j]];
                if ((pt.op != OP_INCL && pt.op != OP_EXCL) || pt.state != P_OK || pt.lit_len != r.n) continue;
                const uint32_t* lw = reinterpret_cast<const uint32_t*>(lits + pt.lit_off);
                if ((lw[0] & m0) == w0 && (n1 == 0 || (lw[1] & m1) == w1)) h |= 1u << j;
            }
        } else {
            for (uint32_t j = 0; j < cnt; j++) {
                const Pattern pt = pats[plist[begin + j]];
                if ((pt.op == OP_INCL || pt.op == OP_EXCL) && pt.state == P_OK && raw_equals(doc, r, pt, lits))
                    h |= 1u << j;
            }
        }
        i = e.end;
        if (i < end) {
            if (doc[i] != ',') return false;
            i++;
            if (i == end) return false;  // "[1,]"
        }
    }
    *hits = h;
    return true;
}

// The fold of a ruleset flagged kFlagFlatFold (one flat All / Any of patterns 0..n - 1 in
// order, n <= 64): the first pattern that is not the group's identity decides, read off the
// bitmaps (run_fold_bits' result, without interpreting the code)
AJX_HD uint8_t flat_fold(const RulesetHdr* h, const uint32_t* code, const uint64_t t[2], const uint64_t u[2],
                         const uint64_t se[2], int32_t* ep) {
    const bool any = (code[0] >> 24) == C_OPEN_OR;
    const uint32_t np = h->n_patterns;
    const uint64_t pm = np >= 64 ? ~0ull : (1ull << np) - 1ull;
    const uint64_t stick = pm & (se[0] | u[0] | (any ? t[0] : ~t[0]));  // (E and U are never the identity)
    *ep = -1;
    if (!stick) return any ? (uint8_t)V_F : (uint8_t)V_T;
    const uint32_t k = (uint32_t)__builtin_ctzll(stick);
    const uint8_t v = ((se[0] >> k) & 1u) ? (uint8_t)V_E : ((u[0] >> k) & 1u) ? (uint8_t)V_U
                    : ((t[0] >> k) & 1u) ? (uint8_t)V_T : (uint8_t)V_F;
    if (v == V_E || v == V_U) *ep = (int32_t)k;
    return v;
}

// The fold of a ruleset flagged kFlagGroupFold (one All / Any over patterns and groups of
// the other kind, patterns 0..n - 1 in code order). A child decides the outer group when
// its value is not the outer identity; a group's value is its first pattern that is not
// the group's identity (or the identity when there is none). The lone patterns that
// decide come off the bitmaps at once; the groups before the first of them are taken in
// order, one bitmap step each (run_fold_bits' result, without interpreting the code).
// (fold_masks: patterns 0..np - 1 of one tree's own bitmaps t0 / u0 / s0 and its group
// masks; *ep is the tree's pattern, from 0)
AJX_HD uint8_t fold_masks(bool any, uint32_t np, uint64_t g_any, uint64_t g_in, uint64_t g_start, uint64_t t0,
                          uint64_t u0, uint64_t s0, int32_t* ep) {
    const uint64_t pm = np >= 64 ? ~0ull : (1ull << np) - 1ull;
    const uint64_t se[1] = {s0}, u[1] = {u0};
    const uint64_t eu = s0 | u0;
    const uint64_t lone = pm & ~g_in & (eu | (any ? t0 : ~t0));   // lone patterns that decide
    const uint64_t inner = g_in & (eu | (g_any & t0) | (~g_any & ~t0));  // not their group's identity
    const uint32_t kl = lone ? (uint32_t)__builtin_ctzll(lone) : 64u;
    const uint8_t ident = any ? (uint8_t)V_F : (uint8_t)V_T;
    auto value = [&](uint32_t k) -> uint8_t {
        return ((se[0] >> k) & 1u) ? (uint8_t)V_E : ((u[0] >> k) & 1u) ? (uint8_t)V_U
             : ((t0 >> k) & 1u) ? (uint8_t)V_T : (uint8_t)V_F;
    };
    *ep = -1;
    uint64_t g = g_start;
    while (g) {
        const uint32_t lo = (uint32_t)__builtin_ctzll(g);
        if (lo > kl) break;
        g &= g - 1ull;
        // the group runs to the next group's first pattern or the next lone pattern
        const uint64_t above = lo >= 63 ? 0ull : ~0ull << (lo + 1);
        const uint64_t ends = (g | ~g_in) & above;
        const uint64_t range = (ends ? ((1ull << __builtin_ctzll(ends)) - 1ull) : ~0ull) & ~((1ull << lo) - 1ull);
        const uint64_t s = inner & range;
        if (!s) {  // the group's identity, the other kind's: it decides
            const uint8_t v = ((g_any >> lo) & 1u) ? (uint8_t)V_F : (uint8_t)V_T;
            if (v != ident) return v;
            continue;
        }
        const uint32_t k = (uint32_t)__builtin_ctzll(s);
        const uint8_t v = value(k);
        if (v != ident) {
            if (v == V_E || v == V_U) *ep = (int32_t)k;
            return v;
        }
    }
    if (kl == 64u) return ident;
    const uint8_t v = value(kl);
    if (v == V_E || v == V_U) *ep = (int32_t)kl;
    return v;
}
AJX_HD uint8_t group_fold(const RulesetHdr* h, const uint32_t* code, const uint64_t t[2], const uint64_t u[2],
                          const uint64_t se[2], int32_t* ep) {
    return fold_masks((code[0] >> 24) == C_OPEN_OR, h->n_patterns, h->fold_grp[0], h->fold_grp[1], h->fold_grp[2],
                      t[0], u[0], se[0], ep);
}
// bits base .. base + n - 1 of a 128-bit bitmap (n <= 64, base + n <= 128)
AJX_HD uint64_t bits_at(const uint64_t w[2], uint32_t base, uint32_t n) {
    const uint64_t lo = base >= 64 ? w[1] >> (base - 64u) : base ? (w[0] >> base) | (w[1] << (64u - base)) : w[0];
    return n >= 64 ? lo : lo & ((1ull << n) - 1ull);
}
// a forest's tree with a TreeFold shape: its fold off its own bits of the bitmaps
AJX_HD uint8_t tree_fold(const TreeFold& f, const uint64_t t[2], const uint64_t u[2], const uint64_t se[2],
                         int32_t* ep) {
    const uint8_t v = fold_masks(f.any != 0, f.n, f.g_any, f.g_in, f.g_start, bits_at(t, f.base, f.n),
                                 bits_at(u, f.base, f.n), bits_at(se, f.base, f.n), ep);
    if (*ep >= 0) *ep += (int32_t)f.base;
    return v;
}

// Stage B's values from LDS. In the lean kernel each lane's 128-byte share of the wave's
// ring is free once stage A is done (and no load of it is in flight), so stage B copies a
// captured value of up to kSpanMax bytes there and reads it from LDS: the value's aligned
// 16-byte blocks (at most eight) are loaded together, one memory latency per value, where
// walking it in memory costs one latency per dependent read (an array: about five per
// element; an escaped string: one per byte; a short literal compare: one per byte). The
// copy is contiguous, lane l's at l * kSpanStride in the wave's ring: 29 dwords, an odd
// count, so the lanes' reads at one offset fall in different banks.
constexpr uint32_t kSpanStride = 116;
constexpr uint32_t kSpanMax = 112;
// copy doc bytes [a, a + n) to buf (4-byte aligned): returns the offset in buf of byte a
// (a's offset in its dword; the dwords that hold the span are copied whole), or ~0u when
// they do not fit (more than kSpanStride bytes, or more than eight 16-byte blocks)
AJX_HD uint32_t stage_span(const uint8_t* src, uint32_t n, uint8_t* buf) {
    const uint32_t m16 = (uint32_t)((uintptr_t)src & 15u), sh = m16 & 3u;
    const uint32_t nb = (m16 + n + 15u) / 16u, nd = (sh + n + 3u) / 4u;
    if (nb > 8 || nd * 4u > kSpanStride || n == 0) return ~0u;
#if defined(__HIPCC__)
    using V16 = uint4;
#else
    using V16 = Block16;
#endif
    const V16* a4 = reinterpret_cast<const V16*>(src - m16);
    V16 blk[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) blk[j] = a4[j < nb ? j : nb - 1u];
    // dword k of block j is the span's dword 4 j + k - m16 / 4
    uint32_t* bw = reinterpret_cast<uint32_t*>(buf);
#if !defined(__HIPCC__)
    // (host test builds: the bytes around the copy are poison, so that a read outside the
    // value's span shows as a wrong answer against the oracle)
    for (uint32_t k = 0; k < kSpanStride; k++) buf[k] = (k & 1u) ? 0x5Cu : 0x22u;
#endif
    const int32_t d0 = -(int32_t)(m16 >> 2);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t x[4] = {blk[j].x, blk[j].y, blk[j].z, blk[j].w};
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const int32_t d = d0 + (int32_t)(4 * j + k);
            if (d >= 0 && d < (int32_t)nd) bw[d] = x[k];
        }
    }
    return sh;
}

// Stage B for one request: patterns on the captured values, bitmap, fold.
// res(p) values are V_T / V_F / V_E / V_U.
// (s0, sstep: the selectors s0, s0 + sstep, ... only — the lanes of a wave sharing one
// request's stage B; their t / u OR together)
// (ring: the lane's span buffer when the kernel has one free (the lean kernel's, see
// stage_span); nullptr: values are read in memory)
AJX_HD void patterns_from_row(const uint8_t* blob, const uint8_t* doc, RowRef row, uint64_t t[2],
                              uint64_t u[2], const uint64_t* dec = nullptr, uint32_t s0 = 0, uint32_t sstep = 1,
                              uint8_t* ring = nullptr) {
    // selector by selector: each captured value is decoded once for all its patterns;
    // when its String() is a byte span or a literal, eq/neq compare a dword at a time,
    // `matches` runs the DFA straight over the span and incl/excl walk a compact array
    // once for all of the selector's patterns; other values take eval_pattern
    const RulesetHdr* h = (const RulesetHdr*)blob;
    const Pattern* pats = (const Pattern*)(blob + h->off_patterns);
    const SelectorPatterns* sps = (const SelectorPatterns*)(blob + h->off_sel_patterns);
    const uint16_t* plist = (const uint16_t*)(blob + h->off_pattern_lists);
    const uint8_t* lits = blob + h->off_literals;
    const uint64_t found = row[0];
    uint64_t t0 = 0, t1 = 0, u0 = h->unsupported[0], u1 = h->unsupported[1];
    const uint64_t nt0 = h->null_true[0], nt1 = h->null_true[1];
    const uint32_t ns = h->n_selectors;
    // first the selectors decided without their record, then the others (needm) in order,
    // each one's record loaded while the one before it is decided (a row read is a memory
    // latency; `found` is one word, so selectors are < 64)
    uint64_t needm = 0;
    for (uint32_t s = s0; s < ns; s += sstep) {
        const uint32_t cnt = sps[s].count;
        if (!cnt) continue;
        if (!((found >> s) & 1)) {  // Null result
            t0 |= sps[s].mask[0] & nt0;
            t1 |= sps[s].mask[1] & nt1;
            continue;
        }
        if (dec && !(sps[s].mask[0] & ~dec[0]) && !sps[s].mask[1]) {  // decided while capturing
            t0 |= sps[s].mask[0] & dec[1];
            continue;
        }
        needm |= 1ull << s;
    }
    uint64_t rec_next = needm ? row[1 + ctz64f(needm)] : 0ull;
    while (needm) {
        const uint32_t s = ctz64f(needm);
        needm &= needm - 1ull;
        const uint64_t rec = rec_next;
        if (needm) rec_next = row[1 + ctz64f(needm)];
        const uint32_t cnt = sps[s].count;
        const uint32_t meta = (uint32_t)(rec >> 32);
        ValueRef v;
        v.start = (uint32_t)rec;
        v.end = v.start + (meta & 0xFFFFFFu);
        v.type = (uint8_t)((meta >> 24) & 7u);
        v.esc = (uint8_t)((meta >> 27) & 1u);
        // (vd: where the value's bytes are read, the document or the lane's copy in LDS)
        const uint8_t* vd = doc;
        if (ring && v.end - v.start <= kSpanMax) {
            const uint32_t at = stage_span(doc + v.start, v.end - v.start, ring);
            if (at != ~0u) {
                vd = ring;
                v.end = at + (v.end - v.start);
                v.start = at;
            }
        }
        const RawVal rv = raw_value(vd, v);
        const uint32_t begin = sps[s].begin;
        uint32_t hits = 0;
        const bool fast_incl = cnt <= 32 && incl_hits(vd, v, pats, plist, begin, cnt, lits, &hits);
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t p = plist[begin + j];
            const Pattern pt = pats[p];
            uint8_t r;
            if (dec && p < 64 && ((dec[0] >> p) & 1u)) {
                r = ((dec[1] >> p) & 1u) ? V_T : V_F;
            } else if (pt.state != P_OK) {
                r = pt.state == P_STATIC_E ? V_E : V_U;
            } else if (rv.ok && (pt.op == OP_EQ || pt.op == OP_NEQ)) {
                r = raw_equals(vd, rv, pt, lits) == (pt.op == OP_EQ) ? V_T : V_F;
            } else if (rv.ok && pt.op == OP_MATCHES) {
                const bool m = rv.lit ? dfa_match_lit(blob, pt.dfa_off, rv.lit)
                                      : dfa_match_span(blob, pt.dfa_off, vd + rv.a, rv.n);
                r = m ? V_T : V_F;
            } else if (fast_incl && (pt.op == OP_INCL || pt.op == OP_EXCL)) {
                r = (((hits >> j) & 1u) != 0) == (pt.op == OP_INCL) ? V_T : V_F;
            } else {
                r = eval_pattern(blob, pt, vd, v);
            }
            const uint64_t bit = 1ull << (p & 63);
            if (r == V_T) {
                if (p < 64) t0 |= bit;
                else t1 |= bit;
            } else if (r == V_U) {
                if (p < 64) u0 |= bit;
                else u1 |= bit;
            }
        }
    }
    t[0] = t0;
    t[1] = t1;
    u[0] = u0;
    u[1] = u1;
}

// the And/Or fold of every tree of the ruleset on the pattern bitmaps; a forest ruleset
// (authjx_compile_forest) writes its n_trees results at r * n_trees + k
AJX_HD void fold_outputs(uint32_t r, const uint8_t* blob, const RulesetHdr* h, const uint64_t t[2],
                         const uint64_t u[2], const uint64_t se[2], uint8_t* __restrict__ out_tri,
                         int32_t* __restrict__ out_err) {
    const uint32_t* code = reinterpret_cast<const uint32_t*>(blob + h->off_code);
    const uint32_t nt = h->pad1[0];
    if (h->flags & kFlagFlatFold) {  // (one tree, [open, pattern 0, ..., pattern n - 1, close])
        int32_t ep;
        out_tri[r] = flat_fold(h, code, t, u, se, &ep);
        if (out_err) out_err[r] = ep;
        return;
    }
    if (h->flags & kFlagGroupFold) {  // (one tree: groups of patterns under one All / Any)
        int32_t ep;
        out_tri[r] = group_fold(h, code, t, u, se, &ep);
        if (out_err) out_err[r] = ep;
        return;
    }
    if (nt == 0) {
        int32_t ep;
        out_tri[r] = run_fold_bits(code, h->n_code, t, u, se, &ep);
        if (out_err) out_err[r] = ep;
        return;
    }
    const uint32_t* rc = reinterpret_cast<const uint32_t*>(blob + h->pad1[1]);
    const TreeFold* tf = h->pad1[2] ? reinterpret_cast<const TreeFold*>(blob + h->pad1[2]) : nullptr;
    for (uint32_t k = 0; k < nt; k++) {
        int32_t ep;
        out_tri[(size_t)r * nt + k] = tf && tf[k].shape ? tree_fold(tf[k], t, u, se, &ep)
                                                        : run_fold_bits(code + rc[2 * k], rc[2 * k + 1], t, u, se, &ep);
        if (out_err) out_err[(size_t)r * nt + k] = ep;
    }
}

// request r's row of the T bitmap (out_bm null: the caller wants none): the ruleset's two
// words, the row's other words zero
AJX_HD void write_bitmap(uint32_t r, const uint64_t t[2], uint64_t* __restrict__ out_bm, uint32_t stride) {
    if (!out_bm) return;
    uint64_t* orow = out_bm + (size_t)r * stride;
    orow[0] = t[0];
    if (stride > 1) orow[1] = t[1];
    for (uint32_t w = 2; w < stride; w++) orow[w] = 0ull;
}

// stage B for request r on its capture row: patterns, T bitmap, And/Or fold, outputs.
// false (nothing written): a value needs the exact scan (a number only ajx_float.h
// decides), the caller hands the request over
AJX_HD bool finish_request(uint32_t r, const uint8_t* blob, const uint8_t* d, RowRef row,
                           uint8_t* __restrict__ out_tri, int32_t* __restrict__ out_err,
                           uint64_t* __restrict__ out_bm, uint32_t stride, const uint64_t* dec = nullptr,
                           uint8_t* ring = nullptr) {
    const RulesetHdr* h = reinterpret_cast<const RulesetHdr*>(blob);
    uint64_t t[2], u[2];
    patterns_from_row(blob, d, row, t, u, dec, 0, 1, ring);
    if ((u[0] & ~h->unsupported[0]) | (u[1] & ~h->unsupported[1])) return false;
    write_bitmap(r, t, out_bm, stride);
    const uint64_t se[2] = {h->static_error[0], h->static_error[1]};
    fold_outputs(r, blob, h, t, u, se, out_tri, out_err);
    return true;
}

}  // namespace ajx
