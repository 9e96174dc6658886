// ajx_render_prog.h — host side of a render program: checks the caller's op lists
// (authjx_render_output, include/authjx.h) and lays them out as the blob ajx_render.h
// reads. Plain C++ (no HIP): authjx_render_compile uses it, and so does the test-only host
// build of the render logic.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "../../include/authjx.h"

namespace ajx {

// the same layout as RenderHdr / RenderOp of ajx_render.h (eight and four u32 words)
inline int build_render_program(const authjx_render_output* outs, uint32_t n_outputs, uint32_t n_slots,
                                std::vector<uint8_t>* blob, std::string* err) {
    if (!outs && n_outputs) { *err = "no outputs"; return AUTHJX_EINVAL; }
    std::vector<uint32_t> begin(n_outputs + 1, 0), ops;
    std::vector<uint8_t> lits;
    for (uint32_t k = 0; k < n_outputs; k++) {
        begin[k] = (uint32_t)(ops.size() / 4);
        if (!outs[k].ops && outs[k].n_ops) { *err = "output " + std::to_string(k) + ": no ops"; return AUTHJX_EINVAL; }
        for (uint32_t q = 0; q < outs[k].n_ops; q++) {
            const authjx_render_op& op = outs[k].ops[q];
            const std::string at = "output " + std::to_string(k) + " op " + std::to_string(q);
            // (5 is not assigned)
            if (op.op > AUTHJX_R_STRING_UTF8 || op.op == 5) { *err = at + ": unknown op"; return AUTHJX_EINVAL; }
            uint32_t off = 0, len = 0, slot = 0;
            if (op.op == AUTHJX_R_LIT) {
                if (!op.lit && op.lit_len) { *err = at + ": no literal"; return AUTHJX_EINVAL; }
                off = (uint32_t)lits.size();
                len = op.lit_len;
                lits.insert(lits.end(), op.lit, op.lit + op.lit_len);
            } else {
                if (op.slot >= n_slots) { *err = at + ": slot out of range"; return AUTHJX_EINVAL; }
                slot = op.slot;
            }
            ops.insert(ops.end(), {(uint32_t)op.op, slot, off, len});
        }
    }
    begin[n_outputs] = (uint32_t)(ops.size() / 4);
    const uint32_t off_begin = 32, off_ops = off_begin + 4u * (n_outputs + 1);
    const uint32_t off_lits = off_ops + 4u * (uint32_t)ops.size();
    const uint32_t total = (off_lits + (uint32_t)lits.size() + 15u) & ~15u;
    const uint32_t hdr[8] = {0x52444E52u, n_outputs, n_slots, (uint32_t)(ops.size() / 4),
                             off_begin,   off_ops,   off_lits, total};
    blob->assign(total, 0);
    std::memcpy(blob->data(), hdr, sizeof hdr);
    std::memcpy(blob->data() + off_begin, begin.data(), begin.size() * 4);
    if (!ops.empty()) std::memcpy(blob->data() + off_ops, ops.data(), ops.size() * 4);
    if (!lits.empty()) std::memcpy(blob->data() + off_lits, lits.data(), lits.size());
    return AUTHJX_OK;
}

}  // namespace ajx
