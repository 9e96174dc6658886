"""TEST-ONLY helpers of the multi-program render tests (tests/test_render_multi_host.py,
tests/test_gpu_render_multi.py): the three programs and the request interleavings both files
use, each request's values from the oracle by its own program's paths, the batch a
one-program call expects composed into what the multi-program call must give, and a ctypes
binding of tests/native/libajx_rendermulti.so (host build of render_request_multi,
authorino_amd/csrc/ajx_render.h). Not product code."""
from __future__ import annotations

import ctypes as C
import os
import struct
import subprocess

import numpy as np

import _rendertest as T
from authorino_amd import response as R
from test_pipeline_host import OracleCtx

NONE = 0xFFFFFFFF           # AUTHJX_RENDER_NO_PROGRAM
GUARD, GUARD32 = 0xA5, 0xA5A5A5A5
TEXT_STRIDE = 256
_L = None


def make(target: str) -> str:
    subprocess.run(["make", "-s", "-C", T.NATIVE, "-f", "render_multi.mk", target], check=True)
    return os.path.join(T.NATIVE, target)


def lib():
    global _L
    if _L is None:
        from authorino_amd.runtime import _RenderOutput

        L = C.CDLL(make("libajx_rendermulti.so"))
        L.rt_compile.argtypes = [C.POINTER(_RenderOutput), C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t,
                                 C.POINTER(C.c_int)]
        L.rt_compile.restype = C.c_void_p
        L.rt_free.argtypes = [C.c_void_p]
        L.rt_render.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                   C.c_void_p, C.c_uint32, C.c_void_p]
        L.rt_render.restype = C.c_int
        L.rtm_render.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                 C.c_void_p, C.c_uint32]
        L.rtm_render.restype = C.c_int
        _L = L
    return _L


def programs():
    """[(outputs, n_slots, paths)]: c5's four response headers over its 8 selectors; the 18
    templates LIT(a) STRING LIT("x"), a = 0..17, of test_gpu_render's store-alignment test,
    over one fuzz string; a program without outputs."""
    from authorino_amd import workloads

    cfg = workloads.make("c5", n=1, seed=51).auth_config
    sel = R.ResponseSelectors(cfg.response, OracleCtx())
    ops, keys = R.compile_render(cfg.response, sel)
    assert len(keys) == 4 and ops.n_slots == len(sel.paths) == 8
    lit = b"ABCDEFGHIJKLMNOPQR"
    tmpl = [([(R.R_LIT, lit[:a])] if a else []) + [(R.R_STRING, 0), (R.R_LIT, b"x")] for a in range(18)]
    return [(ops.outputs, ops.n_slots, list(sel.paths)), (tmpl, 1, ["x.s0"]), ([], 0, [])]


def interleaving(n: int, shape: str, n_progs: int = 3) -> np.ndarray:
    """prog_of_req of n requests. "runs": a quarter of the batch per program, then a
    quarter without one (whole waves of one program once n is large enough);
    "alternating": 0, 1, 2, none, 0, ... (every wave holds all of them); "none"."""
    r = np.arange(n, dtype=np.uint64)
    if shape == "runs":
        por = (r * np.uint64(n_progs + 1)) // np.uint64(max(n, 1))
    elif shape == "alternating":
        por = r % np.uint64(n_progs + 1)
    else:
        assert shape == "none"
        por = np.full(n, n_progs, dtype=np.uint64)
    por = por.astype(np.uint32)
    por[por == n_progs] = NONE
    return por


def batch_values(progs, por, docs):
    """(values u32[n][max n_slots][3], text u8[n][TEXT_STRIDE]): each request's row holds
    the oracle's values of its own program's paths (zeros where it has none)."""
    n = len(docs)
    vs = max(1, max(p[1] for p in progs))
    values = np.zeros((n, vs, 3), dtype=np.uint32)
    text = np.zeros((n, TEXT_STRIDE), dtype=np.uint8)
    for i, (_, n_slots, paths) in enumerate(progs):
        idx = np.flatnonzero(por == i)
        if n_slots == 0 or len(idx) == 0:
            continue
        v, t = T.oracle_values([docs[j] for j in idx], paths, text_stride=TEXT_STRIDE)
        values[idx, :n_slots] = v
        text[idx] = t
    return values, text


def expected(progs, por, docs, values, text, out_stride, one):
    """What the multi-program call must leave in guard-filled buffers: (records
    u32[n][max n_outputs][3], out_text u8[n][out_stride]). one(i, docs, values, text,
    out_text) is a one-program call of program i over a subset of the batch, rendering
    into the guard-filled slots it is given: (records u32[m][n_outputs][3] with the status
    word masked to its byte, out_text)."""
    n = len(docs)
    rs = max(1, max(len(p[0]) for p in progs))
    rec = np.full((n, rs, 3), GUARD32, dtype=np.uint32)
    out = np.full((n, out_stride), GUARD, dtype=np.uint8)
    for i, (outputs, _, _) in enumerate(progs):
        idx = np.flatnonzero(por == i)
        if len(idx) == 0:
            continue
        r1, o1 = one(i, [docs[j] for j in idx], values[idx], text[idx],
                     np.full((len(idx), out_stride), GUARD, dtype=np.uint8))
        rec[idx, :len(outputs)] = r1
        out[idx] = o1[:len(idx)]
    return rec, out


class HostPrograms:
    """The programs compiled by the host build (build_render_program, what
    authjx_render_compile runs)."""

    def __init__(self, progs):
        self.progs = progs
        self.h = []
        for outputs, n_slots, _ in progs:
            oarr, keep = T.c_outputs(outputs)
            err = C.create_string_buffer(256)
            rc = C.c_int(0)
            h = lib().rt_compile(oarr, len(outputs), n_slots, err, 256, C.byref(rc))
            assert rc.value == 0 and h, err.value
            self.h.append(h)

    def __del__(self):
        for h in getattr(self, "h", []):
            lib().rt_free(h)
        self.h = []

    def one(self, i, docs, values, text, out_text):
        """The one-program body (rt_render: render_request) of program i."""
        arena, offs, lens = T.pack(docs)
        n = len(docs)
        values = np.ascontiguousarray(values, dtype=np.uint32)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        k = len(self.progs[i][0])
        rec = np.zeros((n, max(k, 1), 3), dtype=np.uint32)
        rc = lib().rt_render(self.h[i], arena.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, values.ctypes.data,
                             values.shape[1], text.ctypes.data, text.shape[1], out_text.ctypes.data,
                             out_text.shape[1], rec.ctypes.data)
        assert rc == 0, rc
        rec[:, :, 2] &= 0xFF
        return rec[:, :k], out_text

    def multi(self, por, docs, values, text, out_stride, records_stride=None, handles=None):
        """The multi-program body (rtm_render: render_request_multi) into guard-filled
        buffers: (rc, records with the status word masked where a record was written, out_text)."""
        arena, offs, lens = T.pack(docs)
        n = len(docs)
        handles = self.h if handles is None else handles
        rs = max(1, max(len(p[0]) for p in self.progs)) if records_stride is None else records_stride
        rec = np.full((n, max(rs, 1), 3), GUARD32, dtype=np.uint32)
        out = np.full((n, out_stride), GUARD, dtype=np.uint8)
        values = np.ascontiguousarray(values, dtype=np.uint32)
        text = np.ascontiguousarray(text, dtype=np.uint8)
        harr = (C.c_void_p * max(len(handles), 1))(*handles)
        por = None if por is None else np.ascontiguousarray(por, dtype=np.uint32)
        rc = lib().rtm_render(harr, len(handles), por.ctypes.data if por is not None else None, arena.ctypes.data,
                              offs.ctypes.data, lens.ctypes.data, n, values.ctypes.data, values.shape[1],
                              text.ctypes.data, text.shape[1], out.ctypes.data, out_stride, rec.ctypes.data, rs)
        mask_status(rec)
        return rc, rec, out


def mask_status(rec):
    """authjx_rendered.status is a byte (the three after it are reserved): masked in every
    record that was written, the guard words left as they are."""
    written = rec[:, :, 0] != GUARD32
    rec[:, :, 2] = np.where(written, rec[:, :, 2] & 0xFF, rec[:, :, 2])


def write_cases(path, cases):
    """The case file of tests/native/san_render_multi: cases = [(progs, por, docs, values,
    text, out_stride, records u32[n][rs][3], out_text u8[n][out_stride])]."""
    b = bytearray(struct.pack("<I", len(cases)))
    for progs, por, docs, values, text, out_stride, rec, out in cases:
        b += struct.pack("<I", len(progs))
        for outputs, n_slots, _ in progs:
            b += struct.pack("<II", len(outputs), n_slots)
            for ops in outputs:
                b += struct.pack("<I", len(ops))
                for op, arg in ops:
                    lit = bytes(arg) if op == R.R_LIT else b""
                    b += struct.pack("<III", op, 0 if op == R.R_LIT else int(arg), len(lit)) + lit
        arena, offs, lens = T.pack(docs)
        b += struct.pack("<IIIIII", len(docs), values.shape[1], text.shape[1], out_stride, 1, rec.shape[1])
        b += struct.pack("<Q", arena.nbytes) + arena.tobytes() + offs.tobytes() + lens.tobytes()
        b += np.ascontiguousarray(por, dtype=np.uint32).tobytes()
        b += np.ascontiguousarray(values, dtype=np.uint32).tobytes()
        b += np.ascontiguousarray(text, dtype=np.uint8).tobytes()
        b += np.ascontiguousarray(out, dtype=np.uint8).tobytes()
        b += np.ascontiguousarray(rec, dtype=np.uint32).tobytes()
    with open(path, "wb") as f:
        f.write(bytes(b))
