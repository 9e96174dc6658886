// ajx_fast.h — the token scanner: the single-pass structural scan (stage A) of
// ajx_scan_fast / ajx_scan_fused and of the multi-tenant kernel's mixed waves.
//
// One work-item per request: the document is read once in 64-byte windows of
// aligned dwordx4 loads (the next window prefetched while the current one is
// processed). Each 16-byte block is classified with SWAR byte compares into bitmasks
// (quote, backslash, structural, whitespace); escapes are resolved with the
// branch-free odd-backslash-run rule and string interiors with a prefix-XOR of the
// unescaped quotes, carrying string / escape state from block to block. Only the tokens
// (structural bytes outside strings, string delimiters, scalar runs) go through a JSON
// grammar automaton that follows every selector at once through the ruleset's trie.
// For documents that are valid JSON, gjson v1.14.0 Get returns the first complete path
// match in document order (its scan is a depth-first walk in document order that
// descends only into matching keys and stops at the first hit) — exactly the first key
// or element reached here on the trie node that ends the selector. The value span of
// each selector is written to the request's capture row (ajx_stageb.h: the row format, and
// stage B, which decides the patterns on the captured values).
// Anything the automaton can not prove equivalent to gjson's scan (not valid JSON, a
// non-object/array root, a key with escapes on a selector path, more nesting than
// tracked) marks the row `slow`; the exact per-selector scan (ajx_eval_scan) redoes it.
#pragma once
#include "ajx_stageb.h"

namespace ajx {

AJX_HD uint32_t gather4(uint32_t f) {  // 0x80-per-byte flags -> 4-bit mask
    uint32_t x = f >> 7;
    return (x | (x >> 7) | (x >> 14) | (x >> 21)) & 0xFu;
}
// the 0x80-per-byte flags of 16 bytes (f_i: bytes 4i..4i+3) -> 16-bit mask, bit 4i + j =
// byte j of f_i: the four dwords' flags are merged into one dword (byte j, bit i), its
// nibbles packed into a 4 x 4 bit matrix and transposed with two delta swaps
AJX_HD uint32_t gather16(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t f3) {
    const uint32_t y = (f0 >> 7) | (f1 >> 6) | (f2 >> 5) | (f3 >> 4);
    const uint32_t t0 = (y | (y >> 4)) & 0x00FF00FFu;
    uint32_t z = (t0 | (t0 >> 8)) & 0xFFFFu;  // bit 4j + i
    uint32_t t = (z ^ (z >> 3)) & 0x0A0Au;
    z ^= t ^ (t << 3);
    t = (z ^ (z >> 6)) & 0x00CCu;
    z ^= t ^ (t << 6);
    return z;  // bit 4i + j
}
AJX_HD uint32_t ctz32(uint32_t x) { return (uint32_t)__builtin_ctz(x); }
AJX_HD uint32_t popc32(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
AJX_HD uint32_t hibit32(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }

enum : uint32_t {
    X_ROOT = 0, X_VALUE, X_VALUE_OR_CLOSE, X_KEY_OR_CLOSE, X_KEY, X_COLON, X_COMMA_OR_CLOSE,
    X_IN_KEY, X_IN_VAL, X_DONE, X_SLOW
};

constexpr uint32_t kFastDepth = 16;  // trie tracking depth

// The document window ring of one work-item: the current and the previous 64-byte
// window. Chunk j (16 B) of the ring — j = (A >> 4) & 7 for the position A relative to
// the document's first aligned 16-B block — sits at j * cstride + lane16, so a wave's
// 16-B accesses to one chunk index are contiguous (conflict-free ds_write_b128).
struct WinRing {
    uint8_t* base;
    uint32_t lane16;   // lane * 16
    uint32_t cstride;  // lanes * 16
    AJX_HD uint32_t off(uint32_t a) const { return ((a >> 4) & 7u) * cstride + lane16 + (a & 15u); }
    AJX_HD uint32_t u8(uint32_t a) const { return base[off(a)]; }
    AJX_HD uint32_t u32a(uint32_t a) const { return *reinterpret_cast<const uint32_t*>(base + off(a)); }  // a % 4 == 0
    AJX_HD uint32_t u32(uint32_t a) const {  // the 4 bytes at a, little-endian
        const uint32_t q = a & ~3u, sh = a & 3u;
        const uint32_t w0 = u32a(q), w1 = u32a(q + 4);
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_alignbyte(w1, w0, sh);
#else
        return sh ? (w0 >> (8 * sh)) | (w1 << (32 - 8 * sh)) : w0;
#endif
    }
    AJX_HD uint64_t u64(uint32_t a) const {  // the 8 bytes at a, little-endian
        const uint32_t q = a & ~3u, sh = a & 3u;
        const uint32_t w0 = u32a(q), w1 = u32a(q + 4), w2 = u32a(q + 8);
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh), hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
#else
        const uint32_t lo = sh ? (w0 >> (8 * sh)) | (w1 << (32 - 8 * sh)) : w0;
        const uint32_t hi = sh ? (w1 >> (8 * sh)) | (w2 << (32 - 8 * sh)) : w1;
#endif
        return (uint64_t)lo | ((uint64_t)hi << 32);
    }
    AJX_HD void put(uint32_t a, const Block16& b) {  // a % 16 == 0
#if defined(__HIP_DEVICE_COMPILE__)
        *reinterpret_cast<uint4*>(base + off(a)) = uint4{b.x, b.y, b.z, b.w};
#else
        *reinterpret_cast<Block16*>(base + off(a)) = b;
#endif
    }
};

// Stage-A scanner state (kept in registers; no dynamically indexed arrays). The trie
// tables are read through `tn`/`tc`, which the kernel points at an LDS copy when the
// whole batch uses one ruleset; document bytes a token needs (its byte, a key's last
// 8 bytes, a short scalar) come from the window ring, global memory only on rare paths.
// The document goes by in 64-byte windows: one classification per window and one token
// loop over its 64-bit token mask (a wave runs each loop as long as its busiest lane,
// so wider windows even out the lanes' token counts).
struct Scan {
    const TrieNode* tn;
    const TrieChild* tc;
    const KeySlot* ks;  // key table (1 << (ks_meta & 0xFF) slots)
    uint32_t ks_meta;   // log2 of the slot count | key_probes << 8 (one register for both)
    uint32_t ks_mult;   // key_slot_hash multiplier
    const uint8_t* lits;
    const uint8_t* d;
    RowRef row;     // capture row (header + records)
    uint32_t n;
    WinRing ring;

    uint32_t wa;        // ring position of the current window's byte 0
    int32_t bpos;       // doc position of the current window's byte 0
    uint64_t mbs;       // backslash bits of the current window
    uint32_t carry_bs;  // last backslash before the current window (~0u none)
    uint64_t oq;        // opening-quote bits of the current window
    uint32_t carry_oq;  // last opening quote before the current window
    uint32_t last_oq;

    uint64_t is_arr;    // bit k: container at depth k (1-based) is an array
    uint32_t top_arr;   // (is_arr >> depth) & 1, kept up to date at every push and pop
    uint32_t top_node;  // node_at(depth), kept likewise
    uint64_t nodes_lo;  // trie node per depth 1..8 (kNoNode = none)
    uint64_t nodes_hi;  // depths 9..16
    uint64_t found;     // selectors captured
    uint32_t depth, st, pending, str_open;
    uint32_t gap_first, gap_last, gap_cnt;
    uint32_t last_bs;   // last backslash position (~0u none)
    uint32_t in_str, esc;
    // open container captures (at most 2 nested): sel | depth << 8, start
    uint32_t cap0, cap0_start, cap1, cap1_start, ncap;
    // live arrays on selector paths (at most 2 nested): depth | h << 8
    uint32_t arr0, arr1, narr;

    // (values are selected after they are computed, never by member address: that keeps
    // the scanner state in registers)
    // the 8 document bytes ending just before window offset q (0..64), little-endian
    AJX_HD uint64_t tail8(uint32_t q) const {
        const int32_t a = (int32_t)(wa + q) - 8;
        if (a < 0) return ring.u64(0) << (8 * (uint32_t)(-a));  // (before the first block: zeros)
        return ring.u64((uint32_t)a);
    }
    // window byte i (< 64); wa is a multiple of 64, so its chunk is (wa's half of the
    // ring) | i / 16
    AJX_HD uint32_t byte_at(uint32_t i) const {
        return ring.base[(((wa >> 4) & 4u) | (i >> 4)) * ring.cstride + ring.lane16 + (i & 15u)];
    }
    // opening quote of the string whose closing quote is at window offset i
    AJX_HD uint32_t open_before(uint32_t i) const {
        const uint64_t ob = oq & lt64(i);  // (i < 64: a token's window offset)
        return ob ? (uint32_t)(bpos + (int32_t)hibit64f(ob)) : carry_oq;
    }
    AJX_HD uint32_t last_bs_before(uint32_t i) const {
        const uint64_t mb = mbs & lt64(i);
        return mb ? (uint32_t)(bpos + (int32_t)hibit64f(mb)) : carry_bs;
    }

    AJX_HD uint32_t node_at(uint32_t dd) const {
        if (dd == 0) return 0;
        if (dd > kFastDepth) return kNoNode;
        const uint32_t k = dd - 1;
        const uint64_t lo = nodes_lo, hi = nodes_hi;
        const uint64_t w = k < 8 ? lo : hi;
        return (uint32_t)((w >> ((k & 7) * 8)) & 0xFFu);
    }
    AJX_HD void set_node(uint32_t dd, uint32_t v) {
        if (dd == 0 || dd > kFastDepth) return;
        const uint32_t k = dd - 1;
        const uint64_t m = 0xFFull << ((k & 7) * 8);
        const uint64_t x = ((uint64_t)(v & 0xFF)) << ((k & 7) * 8);
        // (both members stored unconditionally: stores into sibling members from two
        // branches get merged into a store through a selected address, which would push
        // the scanner state out of registers)
        const uint64_t lo = nodes_lo, hi = nodes_hi;
        nodes_lo = k < 8 ? (lo & ~m) | x : lo;
        nodes_hi = k < 8 ? hi : (hi & ~m) | x;
    }
    AJX_HD bool top_is_arr() const { return top_arr != 0; }
    // trie node of the value about to start (key for objects, element index for arrays)
    AJX_HD uint32_t value_node() const {
        if (depth == 0) return 0;
        if (!top_is_arr()) return pending;
        if (!narr) return kNoNode;  // no live array open: the element is off every path
        const uint32_t parent = top_node;
        if (parent == kNoNode || !(tn[parent].flags & 1)) return kNoNode;
        uint32_t h;
        if (narr >= 2 && (arr1 & 0xFF) == depth) h = arr1 >> 8;
        else if (narr >= 1 && (arr0 & 0xFF) == depth) h = arr0 >> 8;
        else return kNoNode;
        const uint32_t cb = tn[parent].child_begin, nc = tn[parent].n_children;
        for (uint32_t c = 0; c < nc; c++)
            if (tc[cb + c].array_index == (int32_t)h) return tc[cb + c].node;
        return kNoNode;
    }
    AJX_HD int32_t leaf_sel(uint32_t node) const {
        if (node == kNoNode) return -1;
        const int32_t s = tn[node].selector;
        if (s < 0 || ((found >> s) & 1)) return -1;
        return s;
    }
    AJX_HD void record(int32_t s, uint32_t start, uint32_t end, uint32_t type, uint32_t esc_) {
        found |= 1ull << s;
        row[1 + s] = (uint64_t)start | ((uint64_t)(((end - start) & 0xFFFFFFu) | (type << 24) | (esc_ << 27)) << 32);
    }
    // a value (scalar, string or container) inside an array completed: next element
    AJX_HD void element_done() {
        if (!narr || !depth || !top_is_arr()) return;
        const uint32_t a0 = arr0, a1 = arr1;
        const bool h1 = narr >= 2 && (a1 & 0xFF) == depth;
        const bool h0 = !h1 && narr >= 1 && (a0 & 0xFF) == depth;
        arr1 = a1 + (h1 ? 0x100u : 0u);
        arr0 = a0 + (h0 ? 0x100u : 0u);
    }
    AJX_HD bool open_container(uint32_t c, uint32_t p) {
        const uint32_t node = value_node();
        if (depth + 1 >= 63) return false;
        depth++;
        const uint64_t bit = 1ull << depth;
        is_arr = c == '[' ? is_arr | bit : is_arr & ~bit;
        top_arr = c == '[' ? 1u : 0u;
        if (node == kNoNode) {  // off every selector path (the common case)
            set_node(depth, kNoNode);
            top_node = kNoNode;
            st = c == '[' ? X_VALUE_OR_CLOSE : X_KEY_OR_CLOSE;
            return true;
        }
        const int32_t s = leaf_sel(node);
        const uint32_t live = tn[node].n_children ? node : kNoNode;
        if (live != kNoNode && depth > kFastDepth) return false;
        set_node(depth, live);
        top_node = live;
        if (s >= 0) {
            found |= 1ull << s;  // first match in document order wins
            if (ncap >= 2) return false;
            const uint32_t v = (uint32_t)s | (depth << 8), c0 = cap0, c1 = cap1, s0 = cap0_start, s1 = cap1_start;
            cap0 = ncap == 0 ? v : c0;
            cap0_start = ncap == 0 ? p : s0;
            cap1 = ncap == 1 ? v : c1;
            cap1_start = ncap == 1 ? p : s1;
            ncap++;
        }
        if (c == '[' && live != kNoNode && (tn[live].flags & 1)) {
            if (narr >= 2) return false;
            const uint32_t a0 = arr0, a1 = arr1;
            arr0 = narr == 0 ? depth : a0;
            arr1 = narr == 1 ? depth : a1;
            narr++;
        }
        st = c == '[' ? X_VALUE_OR_CLOSE : X_KEY_OR_CLOSE;
        return true;
    }
    AJX_HD void close_container(uint32_t p) {
        // (copies first: a conditional over two lvalue members would select their
        // addresses and force the state out of registers)
        if (ncap) {
            const uint32_t c0 = cap0, c1 = cap1, s0 = cap0_start, s1 = cap1_start;
            const uint32_t cs = ncap == 2 ? c1 : c0;
            if ((cs >> 8) == depth) {
                const uint32_t start = ncap == 2 ? s1 : s0;
                row[1 + (cs & 0xFF)] =
                    (uint64_t)start | ((uint64_t)(((p + 1 - start) & 0xFFFFFFu) | ((uint32_t)T_JSON << 24)) << 32);
                ncap--;
            }
        }
        if (narr) {
            const uint32_t a0 = arr0, a1 = arr1;
            const uint32_t at = narr == 2 ? a1 : a0;
            if ((at & 0xFF) == depth) narr--;
        }
        depth--;
        top_arr = (uint32_t)(is_arr >> depth) & 1u;
        top_node = node_at(depth);
        st = depth == 0 ? X_DONE : X_COMMA_OR_CLOSE;
        element_done();  // the container was an element of its parent array
    }
    // a scalar occupying [gap_first, gap_last] completed in a value position
    AJX_HD bool scalar_value() {
        if (gap_last + 1 - gap_first != gap_cnt) return false;  // whitespace inside the run
        const int32_t qend = (int32_t)gap_last + 1 - bpos;
        const uint32_t m = gap_cnt < 8 ? gap_cnt : 8u;
        uint64_t t8 = 0;  // the scalar's last m bytes in the top m bytes
        if (qend >= 0) {
            t8 = tail8((uint32_t)qend);
        } else {  // trailing whitespace ran past a block boundary
            for (uint32_t j = 0; j < m; j++) t8 |= (uint64_t)d[gap_last + 1 - m + j] << (8 * (8 - m + j));
        }
        uint32_t c0, c1;
        if (gap_cnt <= 8) {
            c0 = (uint32_t)(t8 >> (8 * (8 - gap_cnt))) & 0xFFu;
            c1 = gap_cnt >= 2 ? (uint32_t)(t8 >> (8 * (9 - gap_cnt))) & 0xFFu : 0u;
        } else {
            const uint32_t a0 = gap_first + (wa - (uint32_t)bpos);  // ring position of the first byte
            if (a0 + 64u >= wa) {
                const uint32_t w = ring.u32(a0);
                c0 = w & 0xFFu;
                c1 = (w >> 8) & 0xFFu;
            } else {
                c0 = d[gap_first];
                c1 = d[gap_first + 1];
            }
        }
        uint32_t type;
        if (c0 == 't') {
            if (gap_cnt != 4 || (uint32_t)(t8 >> 32) != 0x65757274u) return false;  // "true"
            type = T_TRUE;
        } else if (c0 == 'f') {
            if (gap_cnt != 5 || (t8 >> 24) != 0x65736C6166ull) return false;  // "false"
            type = T_FALSE;
        } else if (c0 == 'n' && c1 == 'u') {
            if (gap_cnt != 4 || (uint32_t)(t8 >> 32) != 0x6C6C756Eu) return false;  // "null"
            type = T_NULL;
        } else if (c0 == '-' || c0 == '+' || (c0 >= '0' && c0 <= '9') || c0 == 'i' || c0 == 'I' || c0 == 'N' ||
                   c0 == 'n') {
            type = T_NUMBER;  // gjson parseNumber: raw runs to whitespace , ] }
        } else {
            return false;
        }
        const int32_t s = leaf_sel(value_node());
        if (s >= 0) record(s, gap_first, gap_last + 1, type, 0);
        element_done();
        st = X_COMMA_OR_CLOSE;
        return true;
    }
    // closing quote of a key at block offset i (doc position p)
    AJX_HD void key_closed(uint32_t p, uint32_t i) {
        pending = kNoNode;
        const uint32_t parent = top_node;
        if (parent == kNoNode) return;
        // (a live node always has children: open_container stores only those)
        str_open = open_before(i);
        const uint32_t lb = last_bs_before(i);
        if (lb != ~0u && lb > str_open) { st = X_SLOW; return; }  // escaped key on a live path
        const uint32_t k0 = str_open + 1, klen = p - k0;
        uint64_t sig = tail8(i);
        if (klen < 8) sig = klen ? sig >> (8 * (8 - klen)) : 0ull;
        if (klen >= kIndexKeyLen) return;
        const uint32_t log2 = ks_meta & 0xFFu, want = klen | (parent << 16), mask = (1u << log2) - 1u;
        const uint32_t at = key_slot_hash(sig, klen, parent, log2, ks_mult);
        // every key of the table sits within key_probes slots of its home (the compiler grows
        // the table for that), so the probe sequence is bounded by it, not by an empty slot
        uint32_t pos = at;
        for (uint32_t probe = 0; probe < (ks_meta >> 8); probe++, pos = (pos + 1) & mask) {
            const KeySlot slot = ks[pos];
            if (slot.meta == kEmptySlot) return;
            if (slot.sig != sig || (slot.meta & 0xFFFFFFu) != want) continue;
            if (klen <= 8 || key_rest_equal(k0, klen, (uint32_t)slot.key_off8 * 8u)) { pending = slot.meta >> 24; return; }
        }
    }
    // the bytes of a key [k0, k0 + klen) before its last 8 equal the literal at key_off
    AJX_HD bool key_rest_equal(uint32_t k0, uint32_t klen, uint32_t key_off) const {
        const uint8_t* kl = lits + key_off;
        const uint32_t a0 = k0 + (wa - (uint32_t)bpos);  // ring position of the key's first byte
        if (a0 + 64u >= wa) {  // the key began in the ring's windows: compare from LDS
            for (uint32_t k = 0; k + 8 < klen; k += 4) {
                const uint32_t r = klen - 8 - k;
                const uint32_t m = r >= 4 ? 0xFFFFFFFFu : (1u << (8 * r)) - 1u;
                if ((ring.u32(a0 + k) ^ load_u32_any(kl + k)) & m) return false;
            }
            return true;
        }
        for (uint32_t k = 0; k + 8 < klen; k++)
            if (d[k0 + k] != kl[k]) return false;
        return true;
    }

    // a string value closed at block offset i (state X_VALUE / X_VALUE_OR_CLOSE)
    AJX_HD void value_string(uint32_t i) {
        const int32_t s = leaf_sel(value_node());
        if (s >= 0) {
            const uint32_t so = open_before(i);
            const uint32_t lb = last_bs_before(i);
            record(s, so, (uint32_t)(bpos + (int32_t)i) + 1, T_STRING, (lb != ~0u && lb > so) ? 1u : 0u);
        }
        element_done();
        st = X_COMMA_OR_CLOSE;
    }

    // one token at block offset i (byte c). Strings arrive as one token, their closing
    // quote (nothing inside a string is a token, so the state before the opening quote
    // still holds there).
    AJX_HD void token(uint32_t c, uint32_t i) {
        const uint32_t p = (uint32_t)(bpos + (int32_t)i);
        if (gap_cnt) {
            if ((st != X_VALUE && st != X_VALUE_OR_CLOSE) || !scalar_value() || (c != ',' && c != ']' && c != '}')) {
                st = X_SLOW;
                return;
            }
            gap_cnt = 0;
        }
        switch (st) {
            case X_ROOT:
                if ((c != '{' && c != '[') || !open_container(c, p)) st = X_SLOW;
                return;
            case X_KEY_OR_CLOSE:
            case X_KEY:
                if (c == '"') {
                    st = X_COLON;
                    key_closed(p, i);
                    return;
                }
                if (c == '}' && st == X_KEY_OR_CLOSE) { close_container(p); return; }
                st = X_SLOW;
                return;
            case X_COLON:
                st = c == ':' ? X_VALUE : X_SLOW;
                return;
            case X_VALUE:
            case X_VALUE_OR_CLOSE:
                if (c == '"') {
                    value_string(i);
                    return;
                }
                if (c == '{' || c == '[') {
                    if (!open_container(c, p)) st = X_SLOW;
                    return;
                }
                if (c == ']' && st == X_VALUE_OR_CLOSE) { close_container(p); return; }
                st = X_SLOW;
                return;
            case X_COMMA_OR_CLOSE:
                if (c == ',') { st = top_is_arr() ? X_VALUE : X_KEY; return; }
                if ((c == '}' && !top_is_arr()) || (c == ']' && top_is_arr())) { close_container(p); return; }
                st = X_SLOW;
                return;
            default:
                return;
        }
    }

    // process the 64 document bytes of window `blk` (ring position of byte 0 = a, a
    // multiple of 64; doc position of byte 0 = bp)
    AJX_HD void window(const Block16* blk, uint32_t a, int32_t bp) {
        wa = a;
        bpos = bp;
        uint64_t valid = ~0ull;
        if (bp < 0) valid &= ~below64f((uint32_t)(-bp));
        if (bp + 64 > (int32_t)n) valid &= below64f((uint32_t)((int32_t)n - bp));
        uint64_t mq = 0, mst = 0, mws = 0, mb = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const Block16 x4 = blk[j];
            ring.put(a + 16u * (uint32_t)j, x4);
            uint32_t qf[4], bf[4], sf[4], wf[4];  // (0x80-per-byte flags; unrolled: registers)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t x = k == 0 ? x4.x : k == 1 ? x4.y : k == 2 ? x4.z : x4.w;
                const uint32_t lx = x | 0x20202020u;
                qf[k] = eq_bytes(x, 0x22222222u);
                bf[k] = eq_bytes(x, 0x5C5C5C5Cu);
                sf[k] = eq_bytes(lx, 0x7B7B7B7Bu) | eq_bytes(lx, 0x7D7D7D7Du) | eq_bytes(x, 0x3A3A3A3Au) |
                        eq_bytes(x, 0x2C2C2C2Cu);
                wf[k] = le20_bytes(x);
            }
            const uint32_t q16 = gather16(qf[0], qf[1], qf[2], qf[3]), b16 = gather16(bf[0], bf[1], bf[2], bf[3]);
            const uint32_t s16 = gather16(sf[0], sf[1], sf[2], sf[3]), w16 = gather16(wf[0], wf[1], wf[2], wf[3]);
            mq |= (uint64_t)q16 << (16 * j);
            mb |= (uint64_t)b16 << (16 * j);
            mst |= (uint64_t)s16 << (16 * j);
            mws |= (uint64_t)w16 << (16 * j);
        }
        mq &= valid;
        mb &= valid;
        mst &= valid;
        mws &= valid;
        mbs = mb;
        // escaped bytes: the byte after an odd-length backslash run
        uint64_t escaped;
        {
            const uint64_t bs = mb & ~(uint64_t)esc;
            const uint64_t follows = (bs << 1) | esc;
            const uint64_t even = 0x5555555555555555ull;
            const uint64_t odd_starts = bs & ~even & ~follows;
            const uint64_t seq = odd_starts + bs;
            esc = seq < bs ? 1u : 0u;  // carry out of the window
            escaped = (even ^ (seq << 1)) & follows;
        }
        carry_bs = last_bs;
        if (mb) last_bs = (uint32_t)(bp + (int32_t)hibit64f(mb));
        const uint64_t qu = mq & ~escaped;
        uint64_t x = qu;
        x ^= x << 1;
        x ^= x << 2;
        x ^= x << 4;
        x ^= x << 8;
        x ^= x << 16;
        x ^= x << 32;
        const uint64_t instr = in_str ? ~x : x;  // inside a string after this byte
        in_str = (uint32_t)(instr >> 63);
        const uint64_t outside = ~instr & ~qu & valid;
        if (mb & outside) { st = X_SLOW; return; }  // backslash outside any string
        const uint64_t ns = outside & ~mst & ~mws;    // scalar bytes
        // tokens: structural bytes outside strings and closing quotes (an opening quote
        // is the quote after which the string is open)
        oq = qu & instr;
        carry_oq = last_oq;
        if (oq) last_oq = (uint32_t)(bp + (int32_t)hibit64f(oq));
        uint64_t toks = (mst & outside) | (qu & ~instr);
        uint64_t below = 0;  // bits already consumed
        while (toks) {
            const uint32_t i = ctz64f(toks);
            toks &= toks - 1;
            const uint64_t g = ns & lt64(i) & ~below;
            if (g) {
                if (gap_cnt == 0) gap_first = (uint32_t)(bp + (int32_t)ctz64f(g));
                gap_last = (uint32_t)(bp + (int32_t)hibit64f(g));
                gap_cnt += popc64f(g);
            }
            below = upto64(i);
            token(byte_at(i), i);
            if (st >= X_DONE) return;
            // compact JSON: the ':' right after a key and the ',' right after a value are
            // taken in the same iteration, and so is a member's string value that opens
            // right after its ':' ("key":"value", — one iteration per member)
            const uint32_t nb = i + 1;
            if (toks & (2ull << i)) {  // (a token at i + 1; none when i = 63)
                const uint32_t c2 = byte_at(nb);
                const bool colon = st == X_COLON && c2 == ':';
                const bool comma = st == X_COMMA_OR_CLOSE && c2 == ',';
                if (colon || comma) {
                    st = (colon || top_is_arr()) ? X_VALUE : X_KEY;
                    toks &= toks - 1;
                    below = upto64(nb);
                    // the opening quote right after the ':' and its closing quote in this
                    // window (nothing inside a string is a token: it is the next token)
                    if (colon && (oq & (4ull << i)) && toks) {
                        const uint32_t j = ctz64f(toks);
                        toks &= toks - 1;
                        below = upto64(j);
                        value_string(j);
                        const uint32_t nb2 = j + 1;
                        if ((toks & (2ull << j)) && byte_at(nb2) == ',') {
                            st = top_is_arr() ? X_VALUE : X_KEY;
                            toks &= toks - 1;
                            below = upto64(nb2);
                        }
                    }
                }
            }
        }
        const uint64_t g = ns & ~below;
        if (g) {
            if (gap_cnt == 0) gap_first = (uint32_t)(bp + (int32_t)ctz64f(g));
            gap_last = (uint32_t)(bp + (int32_t)hibit64f(g));
            gap_cnt += popc64f(g);
            if (st == X_ROOT) st = X_SLOW;  // a scalar (or junk) before the root container
        }
    }
};

// the single-pass path's lookup tables of a ruleset (the blob's own, or an LDS copy)
struct Tables {
    const TrieNode* tn;
    const TrieChild* tc;
    const KeySlot* ks;
};
AJX_HD Tables blob_tables(const uint8_t* blob) {
    const RulesetHdr* h = (const RulesetHdr*)blob;
    return Tables{(const TrieNode*)(blob + h->off_trie_nodes), (const TrieChild*)(blob + h->off_trie_children),
                  (const KeySlot*)(blob + h->off_key_slots)};
}

// Stage A for one request. `row` = capture row (1 + n_selectors u64); `ring` = the
// work-item's window ring (128 B). Returns true when the row is valid (false: the
// request needs the exact scan).
template <class LoadBlock>
AJX_HD bool scan_doc(const uint8_t* blob, const Tables& tab, const uint8_t* d, uint32_t n, RowRef row,
                     const WinRing& ring, LoadBlock load) {
    const RulesetHdr* h = (const RulesetHdr*)blob;
    Scan s;
    s.tn = tab.tn;
    s.tc = tab.tc;
    s.ks = tab.ks;
    s.ks_meta = h->key_slots_log2 | h->key_probes << 8;
    s.ks_mult = h->key_mult;
    s.lits = blob + h->off_literals;
    s.d = d;
    s.row = row;
    s.n = n;
    s.ring = ring;
    s.wa = 0;
    s.bpos = 0;
    s.mbs = 0;
    s.carry_bs = ~0u;
    s.oq = 0;
    s.carry_oq = s.last_oq = 0;
    s.is_arr = 0;
    s.top_arr = 0;
    s.top_node = 0;  // (the root's node)
    s.nodes_lo = s.nodes_hi = ~0ull;
    s.found = 0;
    s.depth = 0;
    s.st = X_ROOT;
    s.pending = kNoNode;
    s.str_open = 0;
    s.gap_first = s.gap_last = s.gap_cnt = 0;
    s.last_bs = ~0u;
    s.in_str = s.esc = 0;
    s.cap0 = s.cap0_start = s.cap1 = s.cap1_start = s.ncap = 0;
    s.arr0 = s.arr1 = s.narr = 0;

    const uint32_t mis = (uint32_t)((uintptr_t)d & 15u);
    const uint32_t nblk = (n + mis + 15) / 16;
    Block16 cur[4], nxt[4];
#pragma unroll
    for (int j = 0; j < 4; j++) cur[j] = load((uint32_t)j, nblk);
#pragma unroll
    for (int j = 0; j < 4; j++) nxt[j] = load((uint32_t)(4 + j), nblk);
    for (uint32_t b0 = 0; b0 < nblk; b0 += 4) {
        s.window(cur, b0 * 16, (int32_t)(b0 * 16) - (int32_t)mis);
        if (s.st >= X_DONE) break;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            cur[j] = nxt[j];
            nxt[j] = load(b0 + 8 + (uint32_t)j, nblk);
        }
    }
    if (s.st != X_DONE) {
        row[0] = kRowSlow;
        return false;
    }
    row[0] = s.found;
    return true;
}

}  // namespace ajx
