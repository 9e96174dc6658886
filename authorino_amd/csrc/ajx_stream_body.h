// ajx_stream_body.h — what the streaming kernels (ajx_kernels.hip: ajx_scan_stream,
// ajx_stream_finish) do to one span and to one stage-B list entry, next to the walk itself
// (ajx_stream.h): stream_body, stream_fin_list, stream_finish_entry. The kernels keep what
// only the device has (the dynamic LDS base, the thread and block indices, the staged blob,
// the last-wave election, the grid-stride loops); the test-only host build
// (tests/native/host_eval.cpp) runs the same text on the 64-thread wave of ajx_wave.h.
#pragma once
#include "ajx_plan.h"
#include "ajx_request.h"
#include "ajx_stream.h"

namespace ajx {

// a stage-B list entry the stream could not prove (merge_slow): the exact scan decides it
constexpr uint32_t kStageExact = 1u << 31;
// keep_rows bit 1 (bit 0: kKeepRows), profiling: the phase clocks of a one-request wave
constexpr uint32_t kKeepTiming = 2u;

// what stream_body answers for its lane's request (the kernel discards it): who decides it
enum StreamDisp : uint32_t {
    kDispStream = 0,  // the stream's eager fold did
    kDispExact = 1,   // the exact scan will (the slow list, or a flagged stage-B list entry)
    kDispStageB = 2,  // stage B did on the LDS copy, or will from the stage-B list
    kDispNone = 3,    // the lane has no request
};

// copies nq 16-byte words with every load unconditional (past the end, word b again): the
// array stays in registers (the streaming kernel's per-wave blob copy: c4 serving 7.8 k ->
// 4.0 k clocks)
AJX_HD void copy_words_reg(stream::V4* __restrict__ dst, const stream::V4* __restrict__ src, uint32_t nq, uint32_t t,
                           uint32_t nt) {
    for (uint32_t b = t; b < nq; b += 8u * nt) {
        stream::V4 v[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t k = b + j * nt;
            v[j] = src[k < nq ? k : b];
        }
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            if (b + j * nt < nq) dst[b + j * nt] = v[j];
    }
}

// The streaming kernel's span (ajx_stream.h): wave w of its workgroup, lane l, takes span
// `span` of stream::kSpan requests in arena order and reads their bytes as one coalesced
// stream; a lane per request then folds the patterns the stream decided. Requests with a
// pattern left (a value to parse or unescape, a regex, a long value) go with their row
// (found word, records, the 4 eager words: row_stride >= 5 + n_rec, StreamHdr) to
// ajx_stream_finish through the stage-B list; requests it can not prove go to the slow list
// (the exact scan). keep_rows (forest rulesets, for authjx_select_from_eval_device): every
// request's row is written (slow ones: kRowSlow), those with an open record through stage B.
// Rows: the wave-interleaved layout at work-item r. Profiling: MODE 1 the structural pass
// only, 2 no fold.
// dyn: the workgroup's dynamic LDS, [blob copy] [per wave: WaveLds, capture rows, eager
// decisions]; blob0: the batch's ruleset staged at its start (not MT).
// MT (multi-tenant latency batches): one request per wave (per = 1) under its own
// ruleset sets[set_of_req[r]], its tables read from global memory (L2) or, when the blob
// fits wave_off bytes, from the wave's own copy.
// LAT (small batches, no kept rows): a span that fit one step has its documents in LDS
// still, and its lanes run stage B there (finish_full on the ring); what that leaves goes
// to the exact scan through the stage-B list.
// c0 (profiling): the kernel's clock before it staged the blob.
template <int MODE, bool MT = false, bool LAT = false>
AJX_HD uint32_t stream_body(const uint8_t* const* __restrict__ sets, const uint32_t* __restrict__ set_of_req,
                            const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                            const uint32_t* __restrict__ lens, uint32_t n, StreamCounters* __restrict__ ctr,
                            uint32_t* __restrict__ slow_ids, uint32_t* __restrict__ stage_ids,
                            uint8_t* __restrict__ out_tri, int32_t* __restrict__ out_err,
                            uint64_t* __restrict__ out_bm, uint32_t stride, uint32_t wave_off, uint32_t wave_bytes,
                            uint64_t* __restrict__ rows_out, uint32_t row_stride, uint32_t keep_rows, uint32_t per,
                            uint32_t merge_slow, uint8_t* dyn, uint32_t w, uint32_t l, uint32_t span,
                            const uint8_t* blob0, uint64_t c0) {
    // (profiling, keep_rows bit 1: lane 0 of a one-request wave writes its phases' clock
    // counts over the request's bitmap word: blob copy | stream | stage B, 21 bits each, x16)
    const bool timing = (keep_rows & kKeepTiming) != 0;
    keep_rows &= kKeepRows;
    uint64_t c1 = 0, c2 = 0;
    const uint8_t* blob;
    uint8_t* base;
    if constexpr (MT) {
        // per wave: [its ruleset's blob, when it fits wave_off bytes] [WaveLds, rows]
        if (span >= n) return kDispNone;  // (wave-uniform; per = 1)
        const uint8_t* g = sets[set_of_req[span]];
        uint8_t* wb = dyn + w * wave_bytes;
        const uint32_t tb = lean::uni(reinterpret_cast<const RulesetHdr*>(g)->total_bytes);  // (x16)
        if (tb <= wave_off) {
            copy_words_reg(reinterpret_cast<stream::V4*>(wb), reinterpret_cast<const stream::V4*>(g), tb / 16u, l,
                           64u);
            wave::sync();
            blob = wb;
        } else {
            blob = g;
        }
        base = wb + wave_off;
    } else {
        blob = blob0;
        base = dyn + wave_off + w * wave_bytes;
    }
    stream::WaveLds& L = *reinterpret_cast<stream::WaveLds*>(base);
    uint64_t* rows = reinterpret_cast<uint64_t*>(base + sizeof(stream::WaveLds));
    if (span * per >= n) return kDispNone;  // (wave-uniform)
    if (timing) c1 = stream::clk_now();
    const uint64_t *rowp = nullptr, *dwp = nullptr;
    const uint8_t* lds_doc = nullptr;
    uint64_t* ck = L.clk;  // (timing: the step's and stage B's phase clocks)
    if (timing) {
        if (l < 9) ck[l] = 0;
        wave::sync();
    }
    const uint32_t res = stream::scan_span<MODE>(L, rows, blob, arena, offs, lens, n, span, per, l, out_tri, out_err,
                                                 out_bm, stride, &rowp, &dwp, LAT ? &lds_doc : nullptr,
                                                 timing ? ck : nullptr);
    const uint32_t r = span * per + l;
    if (timing) c2 = stream::clk_now();
    auto times = [&](uint32_t rq) {
        if (!timing || l != 0 || !out_bm) return;
        const uint64_t c3 = stream::clk_now();
        auto f = [](uint64_t a, uint64_t b) { return ((b - a) >> 4) & 0x1FFFFFull; };
        uint64_t* o = out_bm + (size_t)rq * stride;
        o[0] = f(c0, c1) | (f(c1, c2) << 21) | (f(c2, c3) << 42);
        if (stride >= 4 && ck[0] && ck[8]) {  // (the sub-phases: step 0..3, stage B 5..8)
            o[1] = f(c1, ck[0]) | (f(ck[0], ck[1]) << 21) | (f(ck[1], ck[2]) << 42);
            o[2] = f(ck[2], ck[3]) | (f(ck[3], c2) << 21) | (f(c2, ck[5]) << 42);
            o[3] = f(ck[5], ck[6]) | (f(ck[6], ck[7]) << 21) | (f(ck[7], ck[8]) << 42);
        }
    };
    if constexpr (LAT) {
        // one request per wave: every lane takes part in its stage B (finish_full<true>)
        if (per == 1 && wave::readlane(res == stream::R_STAGE_B && lds_doc ? 1u : 0u, 0) != 0) {
            auto bcast = [](const void* q) {  // lane 0's pointer
                const uint64_t v = (uint64_t)(uintptr_t)q;
                return (uintptr_t)((uint64_t)wave::readlane((uint32_t)v, 0) |
                                   ((uint64_t)wave::readlane((uint32_t)(v >> 32), 0) << 32));
            };
            const uint8_t* d0 = reinterpret_cast<const uint8_t*>(bcast(lds_doc));
            const uint64_t* row0 = reinterpret_cast<const uint64_t*>(bcast(rowp));
            const uint64_t* dw0 = reinterpret_cast<const uint64_t*>(bcast(dwp));
            const uint32_t r0 = span;
            const bool ok = stream::finish_full<true>(r0, blob, d0, lens[r0], RowRef(row0), out_tri, out_err, out_bm,
                                                      stride, dw0, timing ? ck : nullptr);
            if (!ok && l == 0) {
                wave::global_add(&ctr->slow, 1u);
                stage_ids[wave::global_add(&ctr->stage_b, 1u)] = r0 | kStageExact;
            }
            times(r0);
            return l != 0 ? kDispNone : ok ? kDispStageB : kDispExact;
        }
    }
    if (l >= per || r >= n) return kDispNone;
    if (MODE != 0) return res == stream::R_SLOW ? kDispExact : kDispStream;
    if constexpr (LAT) {
        if (res == stream::R_STAGE_B && lds_doc) {
            if (!stream::finish_full(r, blob, lds_doc, lens[r], RowRef(rowp), out_tri, out_err, out_bm, stride,
                                     dwp)) {
                wave::global_add(&ctr->slow, 1u);
                stage_ids[wave::global_add(&ctr->stage_b, 1u)] = r | kStageExact;
                return kDispExact;
            }
            return kDispStageB;
        }
    }
    const RowRef o = wave_row(rows_out, row_stride, r);
    if (res == stream::R_SLOW) {
        // (merge_slow: the stage-B kernel runs its exact scan, flagged on the stage-B list)
        if (merge_slow) {
            wave::global_add(&ctr->slow, 1u);
            stage_ids[wave::global_add(&ctr->stage_b, 1u)] = r | kStageExact;
        } else {
            slow_ids[wave::global_add(&ctr->slow, 1u)] = r;
        }
        if (keep_rows) o[0] = kRowSlow;
        return kDispExact;
    }
    // (the records: the selectors', then exact selectors' prefixes')
    const RulesetHdr* hb = reinterpret_cast<const RulesetHdr*>(blob);
    const uint32_t ns = reinterpret_cast<const StreamHdr*>(blob + hb->off_stream)->n_rec;
    bool open = false;
    if (keep_rows)
        for (uint32_t s = 0; s < ns; s++) open = open || ((rowp[1u + s] >> 32) & stream::kOpenEnd);
    if (res == stream::R_STAGE_B || open) {
        for (uint32_t s = 0; s <= ns; s++) o[s] = rowp[s];
        for (uint32_t k = 0; k < 4; k++) o[1u + ns + k] = dwp[k];
        stage_ids[wave::global_add(&ctr->stage_b, 1u)] = r;
        return kDispStageB;
    } else if (keep_rows) {
        for (uint32_t s = 0; s <= ns; s++) o[s] = rowp[s];
    }
    return kDispStream;
}

// One stage-B list entry e, on its row in HBM (stream::finish_full); what stage B can not
// decide goes to the slow list. blob0: the batch's ruleset, staged (not MT); MT: the
// request's own, read from global memory. EXACT (small batches, one launch fewer): the exact
// scan runs here, for the requests the stream flagged (kStageExact) and for those stage B can
// not decide; 1 without, 2 with modifier buffers.
template <bool MT, int EXACT>
AJX_HD void stream_finish_entry(uint32_t e, const uint8_t* blob0, const uint8_t* const* sets,
                                const uint32_t* set_of_req, const uint8_t* arena,
                                const uint64_t* offs, const uint32_t* lens,
                                uint64_t* rows, uint32_t row_stride, StreamCounters* ctr,
                                uint32_t* slow_ids, uint8_t* out_tri,
                                int32_t* out_err, uint64_t* out_bm, uint32_t stride) {
    const uint32_t r = e & ~kStageExact;
    const uint8_t* blob = MT ? sets[set_of_req[r]] : blob0;
    bool ok = false;
    if (!(e & kStageExact))
        ok = stream::finish_full(r, blob, arena + offs[r], lens[r], wave_row(rows, row_stride, r), out_tri, out_err,
                                 out_bm, stride);
    if (ok) return;
    if constexpr (EXACT == 0) {
        slow_ids[wave::global_add(&ctr->slow, 1u)] = r;
    } else {
        if (!(e & kStageExact)) wave::global_add(&ctr->slow, 1u);
        if constexpr (EXACT == 2) {
            ModBufs mb;
            eval_scan_one<true>(r, sets, set_of_req, arena, offs, lens, out_tri, out_err, out_bm, stride, &mb);
        } else {
            eval_scan_one<false>(r, sets, set_of_req, arena, offs, lens, out_tri, out_err, out_bm, stride, nullptr);
        }
    }
}

// The stage-B list of a small batch, lane l's share of its cnt entries (the wave that
// finished last runs it): the requests left to the exact scan and those whose stage B could
// not run on the LDS copy. The rulesets are read from global memory.
template <bool MT>
AJX_HD void stream_fin_list(const uint8_t* const* __restrict__ sets, const uint32_t* __restrict__ set_of_req,
                            const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                            const uint32_t* __restrict__ lens, uint32_t cnt, StreamCounters* __restrict__ ctr,
                            const uint32_t* __restrict__ stage_ids, uint8_t* __restrict__ out_tri,
                            int32_t* __restrict__ out_err, uint64_t* __restrict__ out_bm, uint32_t stride,
                            uint64_t* __restrict__ rows_out, uint32_t row_stride, uint32_t l) {
    for (uint32_t i = l; i < cnt; i += 64u) {
        const uint32_t e = stage_ids[i];
        const uint32_t r = e & ~kStageExact;
        const uint8_t* blob = sets[MT ? set_of_req[r] : 0];
        bool ok = false;
        if (!(e & kStageExact)) {
            ok = stream::finish_full(r, blob, arena + offs[r], lens[r], wave_row(rows_out, row_stride, r), out_tri,
                                     out_err, out_bm, stride);
            if (!ok) wave::global_add(&ctr->slow, 1u);
        }
        if (!ok)
            eval_scan_one<false>(r, sets, MT ? set_of_req : nullptr, arena, offs, lens, out_tri, out_err, out_bm,
                                 stride, nullptr);
    }
}

}  // namespace ajx
