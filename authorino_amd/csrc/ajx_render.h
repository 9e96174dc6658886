// ajx_render.h — the response phase's last step on the device: a render program turns
// selected values (authjx_value spans of the document or of the request's text slot) into
// the final header bytes of
//   response.Plain        fmt.Sprintf("%v", gjson Result.Value())      (plain.go)
//   templates             ReplaceJSONPlaceholders: Result.String()    (pkg/json/json.go:96-151)
//   response.DynamicJSON  json.Marshal of a map, then StringifyJSON   (dynamic_json.go:20-31,
//                                                                       json.go:153-159)
//   denyWith              StringifyJSON of a resolved value                (auth_pipeline.go:581-608)
// as authorino_amd/response.py restates them (result_string, go_sprint_v, go_json_marshal,
// stringify_json). Per-request logic as AJX_HD functions: __device__ in ajx_render.hip,
// plain inline functions in the test-only host build (tests/native/render_host.cpp).
//
// Program blob (built by ajx_render_prog.h): RenderHdr | u32 begin[n_outputs + 1] |
// RenderOp[n_ops] | literal bytes. Output k runs ops [begin[k], begin[k + 1]).
//
// Nesting: the container walk keeps {opening bracket, cursor or last key span} per level
// in a per-lane stack the caller provides (LDS in the kernel), kMaxRenderDepth levels; a
// value nested deeper is left to the caller (kRenderUnrendered).
#pragma once
#include <stdint.h>

#include "ajx_device.h"

namespace ajx {

constexpr int kMaxRenderDepth = 8;     // container levels a SPRINT / MARSHAL op walks
constexpr int kRenderLevelWords = 3;   // per level: opening bracket, cursor | last key start, last key end | esc << 31
constexpr uint32_t kRenderMagic = 0x52444E52u;
// authjx_value.esc flag of built text in the request's text slot (kValText of
// ajx_modifiers.h, AUTHJX_VALUE_TEXT)
constexpr uint8_t kRenderValText = 4;

// ops (AUTHJX_R_* of include/authjx.h)
enum : uint32_t {
    R_LIT = 0, R_STRING = 1, R_STRING_ESC = 2, R_SPRINT = 3, R_MARSHAL = 4, R_STRINGIFY = 6, R_STRING_UTF8 = 7,
    R_OP_COUNT = 8  // (5 is not assigned)
};
// output status (AUTHJX_RENDER_*)
constexpr uint32_t kRenderOk = 0, kRenderUnrendered = 1, kRenderSkipped = 2;

struct RenderHdr {
    uint32_t magic, n_outputs, n_slots, n_ops;
    uint32_t off_begin, off_ops, off_lits, total;
};
struct RenderOp {
    uint32_t op, slot, lit_off, lit_len;
};

// Per-lane level stack: word w of level l at p[(l * kRenderLevelWords + w) * stride]
// (stride = the workgroup's lanes in LDS, so that a wave's accesses fall on distinct banks)
struct RenderStack {
    uint32_t* p;
    uint32_t stride;
    AJX_HD uint32_t& at(int level, int w) const { return p[(uint32_t)(level * kRenderLevelWords + w) * stride]; }
};

AJX_HD void render_store16(uint8_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint4*>(p) = make_uint4(a, b, c, d);
#else
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = a; q[1] = b; q[2] = c; q[3] = d;
#endif
}

// A request's output slot [base, base + cap), base 16-byte aligned and cap a multiple of
// 16. Bytes gather in registers: a dword under construction and the three dwords before it
// of the current 16-byte block; a complete block is one 16-byte store, and flush() writes
// what is left as whole dwords (the last one zero above the text's end). Every store is an
// aligned dword or block that holds a byte below `pos`, so none leaves the slot.
struct RenderOut {
    uint8_t* base;
    uint32_t cap, pos;
    uint32_t acc, q0, q1, q2;
    bool ok;  // false: a byte did not fit (the output is declined)

    AJX_HD void init(uint8_t* b, uint32_t c) {
        base = b; cap = c; pos = 0; acc = q0 = q1 = q2 = 0; ok = true;
    }
    AJX_HD void put(uint32_t c) {
        if (pos >= cap) { ok = false; return; }
        acc |= (c & 0xFFu) << (8u * (pos & 3u));
        pos++;
        if ((pos & 3u) == 0) {
            const uint32_t k = ((pos - 4u) >> 2) & 3u;
            if (k == 0) q0 = acc;
            else if (k == 1) q1 = acc;
            else if (k == 2) q2 = acc;
            else render_store16(base + (pos - 16u), q0, q1, q2, acc);
            acc = 0;
        }
    }
    AJX_HD void put_bytes(const uint8_t* s, uint32_t n) {
        for (uint32_t i = 0; i < n && ok; i++) put(s[i]);
    }
    AJX_HD void put_str(const char* s) {
        for (; *s; s++) put((uint8_t)*s);
    }
    AJX_HD void flush() {
        const uint32_t blk = pos & ~15u, k = (pos >> 2) & 3u;
        uint32_t* o = reinterpret_cast<uint32_t*>(base + blk);
        if (k > 0) o[0] = q0;
        if (k > 1) o[1] = q1;
        if (k > 2) o[2] = q2;
        if (pos & 3u) o[k] = acc;
    }
};

// where an output began: a declined output appends nothing (the registers of the block
// under construction go back too; bytes already stored above `pos` are unspecified)
struct RenderMark {
    uint32_t pos, acc, q0, q1, q2;
    AJX_HD void take(const RenderOut& w) { pos = w.pos; acc = w.acc; q0 = w.q0; q1 = w.q1; q2 = w.q2; }
    AJX_HD void restore(RenderOut* w) const {
        w->pos = pos; w->acc = acc; w->q0 = q0; w->q1 = q1; w->q2 = q2; w->ok = true;
    }
};

// result of an emit step
enum : int { RR_OK = 0, RR_DECLINE = 1, RR_POISON = 2 };  // POISON: json.Marshal fails (the output is "")

AJX_HD void render_put_uint(RenderOut& w, uint32_t x) {
    uint32_t div = 1;
    while (x / div >= 10u) div *= 10u;
    for (; div; div /= 10u) w.put('0' + (x / div) % 10u);
}

enum : int { NF_G = 0, NF_JSON = 1 };

// float64 text from its shortest digits: NF_G = strconv 'g' as fmt %v uses it (%e when the
// decimal exponent is < -4 or >= 6, exponent of at least two digits); NF_JSON =
// encoding/json ('f' unless |f| < 1e-6 or >= 1e21, then 'e' with e-0X written e-X)
AJX_HD int render_canon(RenderOut& w, const NumCanon& c, int fmt) {
    switch (c.kind) {
        case NumCanon::K_UNDECIDED:
        case NumCanon::K_HARD: return RR_DECLINE;
        case NumCanon::K_ZERO:
            if (c.neg) w.put('-');
            w.put('0');
            return RR_OK;
        case NumCanon::K_PINF:
            if (fmt == NF_JSON) return RR_POISON;
            w.put_str("+Inf");
            return RR_OK;
        case NumCanon::K_NINF:
            if (fmt == NF_JSON) return RR_POISON;
            w.put_str("-Inf");
            return RR_OK;
        case NumCanon::K_NAN:
            if (fmt == NF_JSON) return RR_POISON;
            w.put_str("NaN");
            return RR_OK;
        default: break;
    }
    int nd = c.nd;
    const int dp = c.dp;
    while (nd > 1 && c.dig_at(nd - 1) == '0') nd--;
    const int exp = dp - 1;
    // value in [10^(dp-1), 10^dp): < 1e-6 when dp <= -6, >= 1e21 when dp >= 22
    const bool e = fmt == NF_G ? (exp < -4 || exp >= 6) : (dp <= -6 || dp >= 22);
    if (c.neg) w.put('-');
    if (e) {
        w.put(c.dig_at(0));
        if (nd > 1) {
            w.put('.');
            for (int i = 1; i < nd; i++) w.put(c.dig_at(i));
        }
        w.put('e');
        w.put(exp < 0 ? '-' : '+');
        const uint32_t ae = (uint32_t)(exp < 0 ? -exp : exp);
        if (ae < 10u && !(fmt == NF_JSON && exp < 0)) w.put('0');
        render_put_uint(w, ae);
        return RR_OK;
    }
    if (dp <= 0) {
        w.put('0');
        w.put('.');
        for (int i = 0; i < -dp; i++) w.put('0');
        for (int i = 0; i < nd; i++) w.put(c.dig_at(i));
    } else {
        for (int i = 0; i < dp; i++) w.put(i < nd ? c.dig_at(i) : '0');
        if (nd > dp) {
            w.put('.');
            for (int i = dp; i < nd; i++) w.put(c.dig_at(i));
        }
    }
    return RR_OK;
}

// a number token through float64 (gjson Result.Value(): strconv.ParseFloat)
AJX_HD int render_number(RenderOut& w, const uint8_t* s, uint32_t n, int fmt) {
    NumCanon c;
    num_canon(s, n, &c);
    if (c.kind == NumCanon::K_HARD) num_canon_exact(s, n, &c);
    return render_canon(w, c, fmt);
}

AJX_HD int render_count(RenderOut& w, uint32_t x, int fmt) {
    NumCanon c;
    c.kind = x ? NumCanon::K_DIGITS : NumCanon::K_ZERO;
    c.neg = 0;
    c.dlo = 0;
    c.dhi = 0;
    uint32_t nd = 0;
    for (uint32_t y = x;; y /= 10u) { nd++; if (y < 10u) break; }
    for (int j = (int)nd - 1; j >= 0; j--, x /= 10u) c.set_dig(j, (uint8_t)('0' + x % 10u));
    c.nd = (uint8_t)nd;
    c.dp = (int16_t)nd;
    return render_canon(w, c, fmt);
}

AJX_HD void render_hex4(RenderOut& w, uint32_t r) {
    w.put('\\');
    w.put('u');
    for (int k = 3; k >= 0; k--) {
        const uint32_t x = (r >> (4 * k)) & 0xFu;
        w.put(x < 10u ? '0' + x : 'a' + (x - 10u));
    }
}

// encoding/json string encoding (escapeHTML on) of the stream's bytes, without the quotes.
// False on bytes that are not UTF-8 (Go writes the escape of U+FFFD there; the caller declines).
AJX_HD bool render_escaped(RenderOut& w, StrSrc* s) {
    for (;;) {
        const int c = s->next();
        if (c < 0) return true;
        if (c < 0x80) {
            switch (c) {
                case '"': w.put('\\'); w.put('"'); break;
                case '\\': w.put('\\'); w.put('\\'); break;
                case '\n': w.put('\\'); w.put('n'); break;
                case '\r': w.put('\\'); w.put('r'); break;
                case '\t': w.put('\\'); w.put('t'); break;
                default:
                    if (c < 0x20 || c == '<' || c == '>' || c == '&') render_hex4(w, (uint32_t)c);
                    else w.put((uint32_t)c);
            }
            continue;
        }
        // utf8.DecodeRune's accepted forms
        const uint32_t b0 = (uint32_t)c;
        int need = 0;
        uint32_t lo = 0x80, hi = 0xBF;
        if (b0 >= 0xC2 && b0 <= 0xDF) need = 2;
        else if (b0 >= 0xE0 && b0 <= 0xEF) {
            need = 3;
            if (b0 == 0xE0) lo = 0xA0;
            if (b0 == 0xED) hi = 0x9F;
        } else if (b0 >= 0xF0 && b0 <= 0xF4) {
            need = 4;
            if (b0 == 0xF0) lo = 0x90;
            if (b0 == 0xF4) hi = 0x8F;
        }
        if (!need) return false;
        uint32_t word = b0;
        for (int k = 1; k < need; k++) {
            const int x = s->next();
            if (x < (int)lo || x > (int)hi) return false;
            word |= (uint32_t)x << (8 * k);
            lo = 0x80;
            hi = 0xBF;
        }
        if (word == 0xA880E2u || word == 0xA980E2u) {  // U+2028 / U+2029
            render_hex4(w, word == 0xA880E2u ? 0x2028u : 0x2029u);
            continue;
        }
        for (int k = 0; k < need; k++) w.put((word >> (8 * k)) & 0xFFu);
    }
}

// The stream's bytes as they are. False on bytes that are not UTF-8 (utf8.DecodeRune's
// accepted forms, as render_escaped reads them): under StringifyJSON Go writes U+FFFD there.
AJX_HD bool render_utf8(RenderOut& w, StrSrc* s) {
    for (;;) {
        const int c = s->next();
        if (c < 0) return true;
        if (!w.ok) return false;
        w.put((uint32_t)c);
        if (c < 0x80) continue;
        const uint32_t b0 = (uint32_t)c;
        int need = 0;
        uint32_t lo = 0x80, hi = 0xBF;
        if (b0 >= 0xC2 && b0 <= 0xDF) need = 2;
        else if (b0 >= 0xE0 && b0 <= 0xEF) {
            need = 3;
            if (b0 == 0xE0) lo = 0xA0;
            if (b0 == 0xED) hi = 0x9F;
        } else if (b0 >= 0xF0 && b0 <= 0xF4) {
            need = 4;
            if (b0 == 0xF0) lo = 0x90;
            if (b0 == 0xF4) hi = 0x8F;
        }
        if (!need) return false;
        for (int k = 1; k < need; k++) {
            const int x = s->next();
            if (x < (int)lo || x > (int)hi) return false;
            w.put((uint32_t)x);
            lo = 0x80;
            hi = 0xBF;
        }
    }
}

// a string's contents [a, b) (between the quotes): raw bytes for %v, encoded for json
AJX_HD int render_str(RenderOut& w, const uint8_t* d, uint32_t a, uint32_t b, bool esc, bool js) {
    StrSrc s;
    if (esc) s.init_unesc(d, a, b);
    else s.init_raw(d, a, b);
    if (js) {
        w.put('"');
        if (!render_escaped(w, &s)) return RR_DECLINE;
        w.put('"');
        return RR_OK;
    }
    for (int c; (c = s.next()) >= 0 && w.ok;) w.put((uint32_t)c);
    return RR_OK;
}

// order of two object keys by their unescaped bytes: < 0, 0, > 0
AJX_HD int render_key_cmp(const uint8_t* d, uint32_t as, uint32_t ae, bool aesc, uint32_t bs, uint32_t be,
                          bool besc) {
    StrSrc a, b;
    if (aesc) a.init_unesc(d, as, ae);
    else a.init_raw(d, as, ae);
    if (besc) b.init_unesc(d, bs, be);
    else b.init_raw(d, bs, be);
    for (;;) {
        const int x = a.next(), y = b.next();
        if (x != y) return x < y ? -1 : 1;  // (the end, -1, sorts first)
        if (x < 0) return 0;
    }
}

AJX_HD uint32_t render_skip_value(const uint8_t* d, uint32_t e, uint32_t i) {
    const uint8_t c = d[i];
    if (c == '"') {
        bool esc, ok;
        return scan_string(d, e, i + 1, &esc, &ok);
    }
    if (c == '{' || c == '[') return squash(d, e, i);
    return scan_number(d, e, i);
}

// a scalar token [vs, ve) inside a container: true / false / null, else a number
AJX_HD int render_token(RenderOut& w, const uint8_t* d, uint32_t vs, uint32_t ve, bool js) {
    const uint32_t n = ve - vs;
    const uint8_t c = d[vs];
    if (c == 't' && n == 4) { w.put_str("true"); return RR_OK; }
    if (c == 'f' && n == 5) { w.put_str("false"); return RR_OK; }
    if (c == 'n' && n == 4 && d[vs + 1] == 'u') { w.put_str(js ? "null" : "<nil>"); return RR_OK; }
    return render_number(w, d + vs, n, js ? NF_JSON : NF_G);
}

// gjson Result.Value() of the object / array d[s, e), printed by fmt %v (js false:
// "map[k:v k:v]", "[a b]") or json.Marshal (js true). Object members come out in key order
// without a member table: each step scans the object for the smallest unescaped key above
// the one just written, the last member among equal keys (a Go map keeps the last
// duplicate). O(m^2) scans of the object for m members, two words of state per level.
AJX_HD int render_container(RenderOut& w, const uint8_t* d, uint32_t s, uint32_t e, bool js, const RenderStack& st) {
    int level = 0;
    uint32_t wrote = 0;  // bit l: level l has written a member
    st.at(0, 0) = s;
    st.at(0, 1) = d[s] == '[' ? s + 1 : 0u;
    st.at(0, 2) = 0;
    if (d[s] == '[') w.put('[');
    else if (js) w.put('{');
    else w.put_str("map[");
    for (;;) {
        if (!w.ok) return RR_DECLINE;
        const uint32_t o = st.at(level, 0);
        const bool arr = d[o] == '[';
        bool have = false;
        uint32_t vs = 0, bks = 0, bke = 0;
        bool besc = false;
        if (arr) {
            uint32_t i = st.at(level, 1);
            while (i < e && (d[i] <= ' ' || d[i] == ',')) i++;
            if (i < e && d[i] != ']' && d[i] != '}') { have = true; vs = i; }
        } else {
            const uint32_t lks = st.at(level, 1), l2 = st.at(level, 2);
            const uint32_t lke = l2 & 0x7FFFFFFFu;
            const bool lesc = (l2 >> 31) != 0;
            uint32_t i = o + 1;
            while (i < e) {
                while (i < e && d[i] != '"' && d[i] != '}') i++;
                if (i >= e || d[i] == '}') break;
                bool kesc, ok;
                const uint32_t ks = i + 1;
                i = scan_string(d, e, i + 1, &kesc, &ok);
                if (!ok) break;
                const uint32_t ke = i - 1;
                while (i < e && d[i] != ':') i++;
                i++;
                while (i < e && d[i] <= ' ') i++;
                if (i >= e) break;
                const uint32_t v0 = i;
                i = render_skip_value(d, e, i);
                if (lks && render_key_cmp(d, ks, ke, kesc, lks, lke, lesc) <= 0) continue;
                if (have && render_key_cmp(d, ks, ke, kesc, bks, bke, besc) > 0) continue;
                have = true;
                bks = ks; bke = ke; besc = kesc;
                vs = v0;
            }
            if (have) {
                st.at(level, 1) = bks;
                st.at(level, 2) = bke | (besc ? 0x80000000u : 0u);
            }
        }
        if (!have) {
            w.put(arr ? ']' : js ? '}' : ']');
            if (level == 0) return w.ok ? RR_OK : RR_DECLINE;
            level--;
            continue;
        }
        if ((wrote >> level) & 1u) w.put(js ? ',' : ' ');
        wrote |= 1u << level;
        if (!arr) {
            const int rc = render_str(w, d, bks, bke, besc, js);
            if (rc) return rc;
            w.put(':');
        }
        const uint8_t c = d[vs];
        if (c == '{' || c == '[') {
            if (arr) st.at(level, 1) = squash(d, e, vs);
            if (level + 1 >= kMaxRenderDepth) return RR_DECLINE;
            level++;
            wrote &= ~(1u << level);
            st.at(level, 0) = vs;
            st.at(level, 1) = c == '[' ? vs + 1 : 0u;
            st.at(level, 2) = 0;
            if (c == '[') w.put('[');
            else if (js) w.put('{');
            else w.put_str("map[");
            continue;
        }
        uint32_t ve;
        int rc;
        if (c == '"') {
            bool esc, ok;
            ve = scan_string(d, e, vs + 1, &esc, &ok);
            if (!ok) return RR_DECLINE;
            rc = render_str(w, d, vs + 1, ve - 1, esc, js);
        } else {
            ve = scan_number(d, e, vs);
            rc = render_token(w, d, vs, ve, js);
        }
        if (rc) return rc;
        if (arr) st.at(level, 1) = ve;
    }
}

// One op over one selected value. src: the document or the request's text slot; v: its span
// there (already checked to lie inside src).
AJX_HD int render_value(RenderOut& w, uint32_t op, const uint8_t* src, const ValueRef& v, const RenderStack& st) {
    if (op == R_STRING || op == R_STRING_ESC) {
        StrSrc s;
        if (!string_of<true>(src, v, &s)) return RR_DECLINE;
        if (op == R_STRING_ESC) return render_escaped(w, &s) ? RR_OK : RR_DECLINE;
        for (int c; (c = s.next()) >= 0 && w.ok;) w.put((uint32_t)c);
        return RR_OK;
    }
    if (op == R_STRING_UTF8 || (op == R_STRINGIFY && v.type != T_NULL && v.type != T_JSON)) {
        // StringifyJSON of a scalar: Marshal's text read back by Result.String(). A number goes
        // through float64 whatever its spelling and comes out in eq's 'f' layout (StrSrc)
        StrSrc s;
        if (op == R_STRINGIFY && v.type == T_NUMBER && v.esc != kValCount) {
            if (!s.init_num<true>(src, v.start, v.end)) return RR_DECLINE;
            if (s.num.kind == NumCanon::K_PINF || s.num.kind == NumCanon::K_NINF || s.num.kind == NumCanon::K_NAN)
                return RR_POISON;
        } else if (!string_of<true>(src, v, &s)) {
            return RR_DECLINE;
        }
        return render_utf8(w, &s) ? RR_OK : RR_DECLINE;
    }
    const bool js = op == R_MARSHAL || op == R_STRINGIFY;
    switch (v.type) {
        case T_STRING: return render_str(w, src, v.start + 1, v.end - 1, (v.esc & 1) != 0, js);
        case T_NUMBER:
            if (v.esc == kValCount) return render_count(w, v.start, js ? NF_JSON : NF_G);
            return render_number(w, src + v.start, v.end - v.start, js ? NF_JSON : NF_G);
        case T_TRUE: w.put_str("true"); return RR_OK;
        case T_FALSE: w.put_str("false"); return RR_OK;
        case T_JSON: {
            uint32_t s0 = v.start;
            while (s0 < v.end && src[s0] <= ' ') s0++;
            if (s0 >= v.end || (src[s0] != '{' && src[s0] != '[')) return RR_DECLINE;
            return render_container(w, src, s0, v.end, js, st);
        }
        case T_NULL:
            if (op != R_STRINGIFY) w.put_str(js ? "null" : "<nil>");
            return RR_OK;
        default: return RR_DECLINE;
    }
}

// Every output of one request. vals: the request's values, three words each {start, len,
// type | esc << 8}; text: its text slot or nullptr; out: its output slot (16-byte aligned,
// out_cap a multiple of 16); res: n_outputs records of three words {start, len, status}.
// gate(k): kRenderOk when output k renders, else the status it gets instead
// (kRenderUnrendered, kRenderSkipped): such an output appends nothing, reads none of its ops
// or values (the gate's own reads apart: ajx_verdict.h gate_output loads the output's {on,
// when} pair and at most one tri-state byte) and leaves the writer as it found it.
template <class Gate>
AJX_HD void render_request_under(const uint8_t* prog, const uint8_t* doc, uint32_t doc_len, const uint32_t* vals,
                                 const uint8_t* text, uint32_t text_cap, uint8_t* out, uint32_t out_cap, uint32_t* res,
                                 const RenderStack& st, const Gate& gate) {
    const RenderHdr* h = reinterpret_cast<const RenderHdr*>(prog);
    const uint32_t* begin = reinterpret_cast<const uint32_t*>(prog + h->off_begin);
    const RenderOp* ops = reinterpret_cast<const RenderOp*>(prog + h->off_ops);
    const uint8_t* lits = prog + h->off_lits;
    RenderOut w;
    w.init(out, out_cap);
    for (uint32_t k = 0; k < h->n_outputs; k++) {
        RenderMark mark;
        mark.take(w);
        const uint32_t gated = gate(k);
        int rc = RR_OK;
        // (an output that does not apply reads neither its op range nor an op)
        const uint32_t q0 = gated == kRenderOk ? begin[k] : 0u, q1 = gated == kRenderOk ? begin[k + 1] : 0u;
        for (uint32_t q = q0; q < q1 && rc == RR_OK; q++) {
            const RenderOp op = ops[q];
            if (op.op == R_LIT) {
                w.put_bytes(lits + op.lit_off, op.lit_len);
            } else {
                const uint32_t* val = vals + 3u * op.slot;
                ValueRef v;
                v.start = val[0];
                v.end = val[0] + val[1];
                v.type = (uint8_t)(val[2] & 0xFFu);
                v.esc = (uint8_t)((val[2] >> 8) & 0xFFu);
                const bool in_text = (v.esc & kRenderValText) != 0;
                v.esc &= (uint8_t)~kRenderValText;
                const uint8_t* src = in_text ? text : doc;
                const uint32_t cap = in_text ? text_cap : doc_len;
                const bool span = !(v.type == T_NUMBER && v.esc == kValCount) && v.type != T_NULL;
                if (v.type > T_JSON || (span && (!src || v.end < v.start || v.end > cap)) ||
                    (v.type == T_STRING && val[1] < 2u))
                    rc = RR_DECLINE;
                else
                    rc = render_value(w, op.op, src, v, st);
            }
            if (!w.ok) rc = RR_DECLINE;
        }
        if (rc != RR_OK) mark.restore(&w);
        res[3 * k + 0] = mark.pos;
        res[3 * k + 1] = w.pos - mark.pos;
        res[3 * k + 2] = gated != kRenderOk ? gated : rc == RR_DECLINE ? kRenderUnrendered : kRenderOk;
    }
    w.flush();
}

struct RenderUngated {
    AJX_HD uint32_t operator()(uint32_t) const { return kRenderOk; }
};

AJX_HD void render_request(const uint8_t* prog, const uint8_t* doc, uint32_t doc_len, const uint32_t* vals,
                           const uint8_t* text, uint32_t text_cap, uint8_t* out, uint32_t out_cap, uint32_t* res,
                           const RenderStack& st) {
    render_request_under(prog, doc, doc_len, vals, text, text_cap, out, out_cap, res, st, RenderUngated{});
}

// prog_of_req entry of a request that renders nothing (AUTHJX_RENDER_NO_PROGRAM)
constexpr uint32_t kRenderNoProgram = 0xFFFFFFFFu;

// A request of a multi-program batch: renders progs[prog], its other arguments as
// render_request's (res: room for that program's n_outputs records). prog ==
// kRenderNoProgram, or any index that is not below n_progs: nothing is read and nothing
// written, neither the output slot nor the records.
// On the device every lane holds its own program pointer, and the program's header, op and
// literal reads are vector loads where the one-program kernel has scalar ones. In a wave of
// one program (the common case: batches are ordered by ruleset) all lanes of such a load read
// one address; lanes of different programs run together, not in turns (DESIGN §5.15 has the
// build report and the waterfall that was tried instead).
AJX_HD void render_request_multi(const uint8_t* const* progs, uint32_t n_progs, uint32_t prog, const uint8_t* doc,
                                 uint32_t doc_len, const uint32_t* vals, const uint8_t* text, uint32_t text_cap,
                                 uint8_t* out, uint32_t out_cap, uint32_t* res, const RenderStack& st) {
    if (prog >= n_progs) return;
    render_request(progs[prog], doc, doc_len, vals, text, text_cap, out, out_cap, res, st);
}

}  // namespace ajx
