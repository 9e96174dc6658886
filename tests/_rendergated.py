"""TEST-ONLY helpers of the gated render tests (tests/test_gated_host.py,
tests/test_gpu_render_gated.py): a ctypes binding of tests/native/libajx_gatedtest.so (host
build of authorino_amd/csrc/ajx_verdict.h and ajx_render_gated.h), the four programs and
three gate plans both files use, each request's document and values by its own program, the
tri-state shapes, and what a gated call must give composed from UNGATED one-program renders
of the sub-program that holds only the applicable outputs. Not product code."""
from __future__ import annotations

import ctypes as C
import functools
import os
import random
import struct
import subprocess

import numpy as np

import _rendermulti as M
import _rendertest as T
import render_gen as G
from authorino_amd import pipeline as P
from authorino_amd import response as R
from authorino_amd.runtime import _GateEvaluator, _GateOutput, _RenderOutput, _Verdict

NONE, GUARD, GUARD32 = M.NONE, M.GUARD, M.GUARD32
OK, UNRENDERED, SKIPPED = R.RENDER_OK, R.RENDER_UNRENDERED, R.RENDER_SKIPPED
F, T_, E, U = range(4)  # AUTHJX_F / T / E / UNDECIDED
N_TREES = 8
TEXT_STRIDE = M.TEXT_STRIDE
_L = None


def make(target: str) -> str:
    subprocess.run(["make", "-s", "-C", T.NATIVE, "-f", "gated.mk", target], check=True)
    return os.path.join(T.NATIVE, target)


def load(path: str):
    L = C.CDLL(path)
    L.rt_compile.argtypes = [C.POINTER(_RenderOutput), C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t,
                             C.POINTER(C.c_int)]
    L.rt_compile.restype = C.c_void_p
    L.rt_free.argtypes = [C.c_void_p]
    L.rt_render.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                               C.c_void_p, C.c_uint32, C.c_void_p]
    L.rt_render.restype = C.c_int
    L.gt_gates_compile.argtypes = [C.c_int32, C.POINTER(_GateEvaluator), C.c_uint32, C.POINTER(_GateOutput),
                                   C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]
    L.gt_gates_compile.restype = C.c_void_p
    L.gt_gates_free.argtypes = [C.c_void_p]
    L.gt_verdict_of.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_Verdict)]
    L.gt_verdict_of.restype = C.c_int
    L.gt_output_status.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.gt_output_status.restype = C.c_uint32
    L.gtm_render.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                             C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                             C.c_void_p]
    L.gtm_render.restype = C.c_int
    return L


def lib():
    global _L
    if _L is None:
        _L = load(make("libajx_gatedtest.so"))
    return _L


# ---- the plan the fold is enumerated over: a top `when`, two levels of two evaluators each (one
# without `when`, one without rules) and one response `when`: 8 trees ----
FOLD_PLAN = P.GatePlan(top=0, evaluators=[(-1, 1, 0), (2, -1, 0), (3, 4, 5), (5, 6, 5)],
                       outputs=[(P.GATE_ALWAYS, -1), (P.GATE_GRANTED, 7), (P.GATE_GRANTED, -1), (P.GATE_DENIED, -1)],
                       n_trees=N_TREES)


class HostGates:
    """build_gates (what authjx_gates_compile runs) on the CPU."""

    def __init__(self, plan: P.GatePlan, L=None):
        self._L = L if L is not None else lib()
        ev = (_GateEvaluator * max(len(plan.evaluators), 1))(*[_GateEvaluator(*e) for e in plan.evaluators])
        out = (_GateOutput * max(len(plan.outputs), 1))(*[_GateOutput(on, w) for on, w in plan.outputs])
        err = C.create_string_buffer(256)
        rc = C.c_int(0)
        self._h = self._L.gt_gates_compile(plan.top, ev, len(plan.evaluators), out, len(plan.outputs), plan.n_trees,
                                           err, 256, C.byref(rc))
        self.rc, self.error, self.plan = rc.value, err.value.decode(), plan

    def verdict_of(self, row):
        row = np.ascontiguousarray(row, dtype=np.uint8)
        v = _Verdict()
        rc = self._L.gt_verdict_of(self._h, row.ctypes.data, len(row), C.byref(v))
        assert rc == 0, rc
        return int(v.verdict), int(v.denied_by)

    def output_status(self, row, verdict, k):
        row = np.ascontiguousarray(row, dtype=np.uint8)
        return int(self._L.gt_output_status(self._h, row.ctypes.data, verdict, k))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.gt_gates_free(self._h)
            self._h = None


# ---- programs and gates ----
def _cycle(n, gates):
    return [gates[k % len(gates)] for k in range(n)]


@functools.lru_cache(maxsize=None)
def programs():
    """[(outputs, n_slots, paths, plan or None, docs(n, seed))]:
    0  c5's four response headers (GRANTED; two under a response `when`) and a three-output
       denyWith (a static, a template, a pattern) over c5's selectors and documents, under
       FOLD_PLAN's evaluators;
    1  every value of a generated document (render_gen) under STRINGIFY and LIT +
       STRING_UTF8, the gates in turn ALWAYS / GRANTED under a `when` / DENIED / GRANTED;
       no top `when`, one level;
    2  the 18 store-alignment templates over a fuzz string, GRANTED and DENIED in turn;
       a top `when`, two levels;
    3  c5's four headers without gates (a NULL gates entry)."""
    from authorino_amd import workloads

    c5 = M.programs()[0]
    w = lambda n, seed: [workloads.make("c5", n=n, seed=seed).doc(i) for i in range(n)]  # noqa: E731
    deny = [[(R.R_LIT, b"denied by policy")],
            [(R.R_LIT, b"user "), (R.R_STRING_UTF8, 0), (R.R_LIT, b" may not "), (R.R_STRING_UTF8, 1)],
            [(R.R_STRINGIFY, 2)], [(R.R_STRINGIFY, 3)]]
    p0 = c5[0] + deny
    plan0 = P.GatePlan(0, FOLD_PLAN.evaluators,
                       [(P.GATE_GRANTED, -1), (P.GATE_GRANTED, 7), (P.GATE_GRANTED, -1), (P.GATE_GRANTED, 7)]
                       + [(P.GATE_DENIED, -1)] * 4, N_TREES)
    p1 = [o for s in range(G.N_SLOTS) for o in ([(R.R_STRINGIFY, s)], [(R.R_LIT, b"t="), (R.R_STRING_UTF8, s)])]
    plan1 = P.GatePlan(-1, [(-1, 0, 0), (1, 2, 0)],
                       _cycle(len(p1), [(P.GATE_ALWAYS, -1), (P.GATE_GRANTED, 3), (P.GATE_DENIED, -1),
                                        (P.GATE_GRANTED, -1)]), 4)
    p2 = M.programs()[1][0]
    plan2 = P.GatePlan(7, [(6, 5, 1), (-1, 4, 2), (-1, 3, 2)],
                       _cycle(len(p2), [(P.GATE_GRANTED, -1), (P.GATE_DENIED, -1)]), N_TREES)
    return [(p0, c5[1], c5[2], plan0, w),
            (p1, G.N_SLOTS, list(G.PATHS), plan1, lambda n, seed: G.corpus(random.Random(seed), n)),
            (p2, 1, ["x.s0"], plan2, lambda n, seed: T.fuzz_docs(n, seed=seed)),
            (c5[0], c5[1], c5[2], None, w)]


def plans():
    return [p[3] for p in programs()]


@functools.lru_cache(maxsize=None)
def batch(n: int, shape: str = "alternating"):
    """(por, docs, values, text): request r's program by _rendermulti.interleaving over the
    four programs and no program, its document from its program's generator and its values
    from the oracle."""
    progs = programs()
    por = M.interleaving(n, shape, n_progs=len(progs))
    docs = [b"{}"] * n
    for i, p in enumerate(progs):
        idx = np.flatnonzero(por == i)
        for j, d in zip(idx, p[4](len(idx), 700 + i)):
            docs[j] = d
    values, text = M.batch_values([(p[0], p[1], p[2]) for p in progs], por, docs)
    return por, docs, values, text


def tri_rows(por, shape: str, seed: int = 41) -> np.ndarray:
    """u8[n][N_TREES]: "granted" (every tree T), "denied" (the first evaluator with rules
    fails them), "alternating" (granted and denied per lane), "random" (seeded over the four
    values, T at 0.7)."""
    n = len(por)
    tri = np.full((n, N_TREES), T_, dtype=np.uint8)
    if shape == "random":
        rng = np.random.default_rng(seed)
        return rng.choice(np.array([F, T_, E, U], dtype=np.uint8), size=(n, N_TREES), p=[0.1, 0.7, 0.1, 0.1])
    for r in range(n):
        plan = plans()[por[r]] if por[r] != NONE else None
        if plan is None or shape == "granted" or (shape == "alternating" and r % 2 == 0):
            continue
        assert shape in ("denied", "alternating")
        tri[r, next(rt for _, rt, _ in plan.evaluators if rt >= 0)] = F
    return tri


def verdicts_of(por, tri, tri_of_req=None):
    """i32[n][2] by pipeline.verdict_of: {verdict, denied_by}, the guard where a request has
    no program or no gates."""
    out = np.full((len(por), 2), GUARD32, dtype=np.uint32).view(np.int32)
    for r in range(len(por)):
        plan = plans()[por[r]] if por[r] != NONE else None
        if plan is not None:
            out[r] = P.verdict_of(tri[r if tri_of_req is None else tri_of_req[r]], plan)
    return out


def statuses_of(por, tri, r, tri_of_req=None):
    """The gate's answer for every output of request r (pipeline.output_status_of)."""
    outputs, _, _, plan, _ = programs()[por[r]]
    if plan is None:
        return (OK,) * len(outputs)
    row = tri[r if tri_of_req is None else tri_of_req[r]]
    v, _ = P.verdict_of(row, plan)
    return tuple(P.output_status_of(row, plan, v, k) for k in range(len(outputs)))


class HostBatch:
    """The four programs and their gates compiled by the host build `L`."""

    def __init__(self, L=None):
        self._L = L if L is not None else lib()
        self.progs = [T.HostProgram(p[0], p[1], self._L) for p in programs()]
        self.gates = [HostGates(p[3], self._L) if p[3] is not None else None for p in programs()]
        assert all(p.rc == 0 for p in self.progs) and all(g is None or g.rc == 0 for g in self.gates)

    def one(self, outputs, n_slots, docs, values, text, out_text):
        """An ungated one-program render (rt_render: render_request) into the slots given."""
        prog = T.HostProgram(outputs, n_slots, self._L)
        assert prog.rc == 0, prog.error
        rec, out = T.host_render(prog, docs, values[:, :max(n_slots, 1)], text, out_text.shape[1], out_text=out_text)
        return rec, out

    def gated(self, por, docs, values, text, out_stride, tri, tri_of_req=None, records_stride=None, progs=None,
              gates=None, want_verdicts=True):
        """gtm_render (render_request_gated) into guard-filled buffers: (rc, records,
        out_text u8[n + 1][out_stride], verdicts i32[n + 1][2])."""
        arena, offs, lens = T.pack(docs)
        n = len(docs)
        rs = max(len(p[0]) for p in programs()) if records_stride is None else records_stride
        rec = np.full((n + 1, max(rs, 1), 3), GUARD32, dtype=np.uint32)
        out = np.full((n + 1, out_stride), GUARD, dtype=np.uint8)
        ver = np.full((n + 1, 2), GUARD32, dtype=np.uint32)
        rc = gtm_render(self._L, self.progs if progs is None else progs, self.gates if gates is None else gates, por,
                        arena, offs, lens, values, text, out, rec, tri, tri_of_req, ver if want_verdicts else None)
        M.mask_status(rec)
        mask_verdicts(ver)
        return rc, rec, out, ver.view(np.int32)


def gtm_render(L, progs, gates, por, arena, offs, lens, values, text, out, rec, tri, tri_of_req, ver):
    """The host build's gated batch call over the caller's out / rec / ver arrays: its rc."""
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    values, text = np.ascontiguousarray(values, dtype=np.uint32), opt(text, np.uint8)
    por, tri, tor = opt(por, np.uint32), opt(tri, np.uint8), opt(tri_of_req, np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    parr = (C.c_void_p * max(len(progs), 1))(*[p._h if p is not None else None for p in progs])
    garr = (C.c_void_p * max(len(gates), 1))(*[g._h if g is not None else None for g in gates])
    return L.gtm_render(parr, garr, len(progs), ptr(por), ptr(arena), ptr(offs), ptr(lens), len(lens), ptr(values),
                        values.shape[1], ptr(text), text.shape[1] if text is not None else 0, ptr(out), out.shape[1],
                        ptr(rec), rec.shape[1], ptr(tri), tri.shape[1] if tri is not None else 0, ptr(tor), ptr(ver))


class GatedOracleCtx(T.OracleCtx):
    """The oracle's stand-in for runtime.Context (tests/test_pipeline_host.py) with the gated
    entry points on the host build: what AuthPipelineBatch(gated=True) calls."""

    def compile_render(self, outputs, n_slots):
        prog = T.HostProgram(outputs, n_slots, lib())
        assert prog.rc == 0, prog.error
        return prog

    def compile_gates(self, top, evaluators, outputs, n_trees):
        g = HostGates(P.GatePlan(top, list(evaluators), list(outputs), n_trees))
        assert g.rc == 0, g.error
        return g

    def render_gated_host_arena(self, progs, gates, prog_of_req, arena, offs, lens, values, tristate, text=None,
                                tri_of_req=None, out_stride=4096):
        n = len(lens)
        rec = np.zeros((max(n, 1), max([p.n_outputs for p in progs] + [1]), 3), dtype=np.uint32)
        out = np.zeros((max(n, 1), out_stride), dtype=np.uint8)
        ver = np.zeros((max(n, 1), 2), dtype=np.uint32)
        rc = gtm_render(lib(), progs, gates, prog_of_req, np.ascontiguousarray(arena), np.ascontiguousarray(offs),
                        np.ascontiguousarray(lens), values, text, out, rec, tristate, tri_of_req, ver)
        assert rc == 0, rc
        return rec, out, ver.view(np.int32)


def mask_verdicts(ver):
    """authjx_verdict.verdict is a byte (the three after it are reserved): masked where a
    verdict was written."""
    written = ver[:, 0] != GUARD32
    ver[:, 0] = np.where(written, ver[:, 0] & 0xFF, ver[:, 0])


def expected(por, docs, values, text, out_stride, tri, one, tri_of_req=None, records_stride=None):
    """What a gated call must leave in guard-filled buffers, from ungated renders: the
    requests of a program whose gates answer alike render, in one ungated one-program call
    `one(outputs, n_slots, docs, values, text, out_text)`, the sub-program of the outputs
    that apply; an output that does not apply is {the write position, 0, its status}.
    (records u32[n][rs][3], out_text u8[n][out_stride])."""
    n = len(docs)
    rs = max(len(p[0]) for p in programs()) if records_stride is None else records_stride
    rec = np.full((n, rs, 3), GUARD32, dtype=np.uint32)
    out = np.full((n, out_stride), GUARD, dtype=np.uint8)
    groups = {}
    for r in range(n):
        if por[r] != NONE:
            groups.setdefault((int(por[r]), statuses_of(por, tri, r, tri_of_req)), []).append(r)
    for (i, sts), idx in groups.items():
        outputs, n_slots = programs()[i][0], programs()[i][1]
        sub = [o for o, s in zip(outputs, sts) if s == OK]
        r1, o1 = one(sub, n_slots, [docs[j] for j in idx], values[idx], text[idx],
                     np.full((len(idx), out_stride), GUARD, dtype=np.uint8))
        out[idx] = o1[:len(idx)]
        for m, j in enumerate(idx):
            pos = q = 0
            for k, s in enumerate(sts):
                if s == OK:
                    rec[j, k] = r1[m, q]
                    pos = int(r1[m, q, 0]) + int(r1[m, q, 1])
                    q += 1
                else:
                    rec[j, k] = (pos, 0, s)
    return rec, out


# ---- the case file of tests/native/san_gated ----
def write_cases(path, cases):
    """cases = [(por, docs, values, text, out_stride, tri, records u32[n][rs][3], out_text
    u8[n][out_stride], verdicts i32[n][2])] over programs() and plans()."""
    b = bytearray(struct.pack("<I", len(programs())))
    for outputs, n_slots, _, plan, _ in programs():
        b += struct.pack("<II", len(outputs), n_slots)
        for ops in outputs:
            b += struct.pack("<I", len(ops))
            for op, arg in ops:
                lit = bytes(arg) if op == R.R_LIT else b""
                b += struct.pack("<III", op, 0 if op == R.R_LIT else int(arg), len(lit)) + lit
        b += struct.pack("<I", 0 if plan is None else 1)
        if plan is not None:
            b += struct.pack("<iII", plan.top, len(plan.evaluators), plan.n_trees)
            for e in plan.evaluators:
                b += struct.pack("<iii", *e)
            for on, w in plan.outputs:
                b += struct.pack("<Ii", on, w)
    b += struct.pack("<I", len(cases))
    for por, docs, values, text, out_stride, tri, rec, out, ver in cases:
        arena, offs, lens = T.pack(docs)
        b += struct.pack("<IIIIII", len(docs), values.shape[1], text.shape[1], out_stride, rec.shape[1], tri.shape[1])
        b += struct.pack("<Q", arena.nbytes) + arena.tobytes() + offs.tobytes() + lens.tobytes()
        for a, dt in ((por, np.uint32), (values, np.uint32), (text, np.uint8), (tri, np.uint8), (out, np.uint8),
                      (rec, np.uint32), (ver, np.int32)):
            b += np.ascontiguousarray(a, dtype=dt).tobytes()
    with open(path, "wb") as f:
        f.write(bytes(b))
