"""TEST-ONLY helpers of the render tests (tests/test_render_host.py, tests/test_gpu_render.py,
tests/_rendervalues.py): a ctypes binding of tests/native/libajx_rendertest.so (host build of
authorino_amd/csrc/ajx_render.h) or of such a library at another path, the Python mirror of a render program (response.py's host
functions per op: the expected bytes), selected values from the oracle, and the fuzz and
decline inputs both test files share. Not product code."""
from __future__ import annotations

import ctypes as C
import os
import struct
import subprocess

import numpy as np

from authorino_amd import response as R
from authorino_amd.runtime import _RenderOp, _RenderOutput
from test_pipeline_host import OracleCtx
from test_response_host import _rand_doc

_HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(_HERE, "native")
_L = None

OPS = (R.R_STRING, R.R_STRING_ESC, R.R_SPRINT, R.R_MARSHAL)
UNRENDERED = R.RENDER_UNRENDERED


def make(target: str) -> str:
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "render.mk", target], check=True)
    return os.path.join(NATIVE, target)


def load(path: str):
    """The ctypes binding of a host build of render_host.cpp (the one render.mk makes, or a
    library a test compiled itself)."""
    L = C.CDLL(path)
    L.rt_compile.argtypes = [C.POINTER(_RenderOutput), C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t,
                             C.POINTER(C.c_int)]
    L.rt_compile.restype = C.c_void_p
    L.rt_free.argtypes = [C.c_void_p]
    L.rt_max_depth.restype = C.c_int
    L.rt_render.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                               C.c_void_p, C.c_uint32, C.c_void_p]
    L.rt_render.restype = C.c_int
    return L


def lib():
    global _L
    if _L is None:
        _L = load(make("libajx_rendertest.so"))
    return _L


def c_outputs(outputs):
    """The authjx_render_output array of op lists [(R_LIT, bytes) | (op, slot)] (+ what
    keeps its pointers alive). An op number above the known ones passes through as is."""
    keep = []
    oarr = (_RenderOutput * max(len(outputs), 1))()
    for k, ops in enumerate(outputs):
        arr = (_RenderOp * max(len(ops), 1))()
        for q, (op, arg) in enumerate(ops):
            if op == R.R_LIT:
                keep.append(bytes(arg))
                arr[q] = _RenderOp(op, 0, keep[-1], len(keep[-1]))
            else:
                arr[q] = _RenderOp(op, int(arg), None, 0)
        keep.append(arr)
        oarr[k] = _RenderOutput(arr, len(ops))
    return oarr, keep


class HostProgram:
    """build_render_program (what authjx_render_compile runs) on the CPU, by the library
    `L` (load()) or the tree's own."""

    def __init__(self, outputs, n_slots, L=None):
        oarr, keep = c_outputs(outputs)
        err = C.create_string_buffer(256)
        rc = C.c_int(0)
        self._L = L if L is not None else lib()
        self._h = self._L.rt_compile(oarr, len(outputs), n_slots, err, 256, C.byref(rc))
        self.rc, self.error = rc.value, err.value.decode()
        self.n_outputs, self.n_slots = len(outputs), n_slots

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.rt_free(self._h)
            self._h = None


def pack(docs):
    lens = np.fromiter((len(d) for d in docs), dtype=np.uint32, count=len(docs))
    offs = np.zeros(len(docs), dtype=np.uint64)
    if len(docs):
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(docs) + b"\0", dtype=np.uint8), offs, lens


def host_render(prog: HostProgram, docs, values, text, out_stride, out_text=None):
    """authjx_render_batch's contract on the host build: (records u32[n][n_outputs][3],
    out_text u8[n][out_stride])."""
    arena, offs, lens = pack(docs)
    n = len(docs)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    if out_text is None:
        out_text = np.full((n, out_stride), 0xA5, dtype=np.uint8)
    rec = np.zeros((n, max(prog.n_outputs, 1), 3), dtype=np.uint32)
    if text is not None:
        text = np.ascontiguousarray(text, dtype=np.uint8)
    rc = prog._L.rt_render(prog._h, arena.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, values.ctypes.data,
                         values.shape[1], text.ctypes.data if text is not None else None,
                         text.shape[1] if text is not None else 0, out_text.ctypes.data, out_stride,
                         rec.ctypes.data)
    assert rc == 0, rc
    rec[:, :, 2] &= 0xFF
    return rec[:, :prog.n_outputs], out_text


class _Sel:
    def __init__(self, paths):
        self.paths, self.n_patterns = list(paths), len(paths)


def oracle_values(docs, paths, text_stride=4096):
    """The authjx_value rows a select_text call writes, from the oracle's gjson: (u32[n][k][3],
    text u8[n][text_stride]). A string's esc bit (a backslash in its raw text) is set as
    the device's scan sets it."""
    arena, offs, lens = pack(docs)
    vals, text = OracleCtx().select_text_host_arena([_Sel(paths)], arena, offs, lens, text_stride=text_stride)
    for r, doc in enumerate(docs):
        for p in range(len(paths)):
            st, ln, t = (int(x) for x in vals[r, p])
            if (t & 0xFF) == R.STRING:
                src = text[r].tobytes() if (t >> 8) & R.VAL_TEXT else doc
                if b"\\" in src[st:st + ln]:
                    vals[r, p, 2] = t | (1 << 8)
    return vals, text


def mirror(outputs, doc: bytes, vals_r, text_r=None):
    """The expected text of every output of one request: response.py's host functions per
    op (result_string, _json_string, go_sprint_v / go_json_marshal of result_value)."""
    out = []
    for ops in outputs:
        parts, failed = [], False
        for op, arg in ops:
            if op == R.R_LIT:
                parts.append(bytes(arg).decode("utf-8", "replace"))
                continue
            st, ln, t = (int(x) for x in vals_r[arg])
            src = text_r.tobytes() if (t >> 8) & R.VAL_TEXT else doc
            count = (t >> 8) == R.VAL_COUNT
            if op in (R.R_STRING, R.R_STRING_ESC):
                s = str(st) if count else R.result_string(src, st, ln, t & 0xFF)
                parts.append(s if op == R.R_STRING else R._json_string(s)[1:-1])
            else:
                v = float(st) if count else R.result_value(src, st, ln, t & 0xFF)
                if op == R.R_SPRINT:
                    parts.append(R.go_sprint_v(v))
                else:
                    try:
                        parts.append(R.go_json_marshal(v))
                    except R._UnsupportedValue:  # Marshal fails: StringifyJSON gives ""
                        failed = True
        out.append("" if failed else "".join(parts))
    return out


def rendered(rec, out_text, r, k):
    """(status, bytes) of output k of request r."""
    s, ln, st = (int(x) for x in rec[r, k])
    return st, out_text[r, s:s + ln].tobytes()


# ---- the fuzz of tests/test_response_host.py::_rand_doc as one program for every document ----
# every path _rand_doc can produce, one slot each, and each slot under each of the four value
# ops (a LIT in front of the first, so that the fifth op is covered too)
FUZZ_PATHS = ["x.%s%d" % (p, k) for k in range(10) for p in "nsbao"] + ["x.missing", "pad"]
FUZZ_OUTPUTS = [([(R.R_LIT, b"v=")] if op == R.R_STRING else []) + [(op, s)]
                for s in range(len(FUZZ_PATHS)) for op in OPS]
FUZZ_STRIDE = 8192


def fuzz_docs(n, seed=11):
    rng = np.random.default_rng(seed)
    return [_rand_doc(rng)[0] for _ in range(n)]


def check_all(rec, out_text, outputs, docs, vals, text, out_stride):
    """Every output OK and byte-equal to the mirror; outputs packed back to back from the
    slot's start. Returns the end of each request's last output."""
    ends = []
    for r, doc in enumerate(docs):
        want = mirror(outputs, doc, vals[r], None if text is None else text[r])
        pos = 0
        for k, w in enumerate(want):
            st, got = rendered(rec, out_text, r, k)
            assert st == R.RENDER_OK, (r, k, outputs[k], doc)
            assert got == w.encode("utf-8"), (r, k, outputs[k], got, w, doc)
            assert int(rec[r, k, 0]) == pos, (r, k)
            pos += len(got)
        assert pos <= out_stride
        ends.append(pos)
    return ends


# ---- the decline reasons (one request; the other outputs of the request stay correct) ----
def nested(depth: int) -> str:
    """A value of `depth` container levels, objects and arrays in turn, keys out of order."""
    s = "1"
    for d in range(depth):
        s = '{"b":%s,"a":null}' % s if d % 2 else "[%s,true]" % s
    return s


def decline_case(max_depth: int):
    """(outputs, n_slots, docs, values, text, expected): expected[k] = (status, text or
    None when the mirror decides it). Slot 5 is a value of type 255."""
    doc = ('{"x":{"ok":"fine","n":1685557675,"dmax":%s,"dover":%s,"ff":"a\xffb\\n"}}'
           % (nested(max_depth), nested(max_depth + 1))).encode("latin-1")
    paths = ["x.ok", "x.n", "x.dmax", "x.dover", "x.ff", "x.ok"]
    vals, text = oracle_values([doc], paths)
    vals[0, 5] = (0, 0, 255)
    U = (UNRENDERED, "")
    cases = [([(R.R_SPRINT, 2)], None), ([(R.R_MARSHAL, 2)], None),
             ([(R.R_SPRINT, 3)], U), ([(R.R_MARSHAL, 3)], U),
             ([(R.R_LIT, b"a="), (R.R_STRING, 0)], None),
             ([(R.R_LIT, b'{"p":'), (R.R_MARSHAL, 4), (R.R_LIT, b"}")], U),
             ([(R.R_LIT, b'"'), (R.R_STRING_ESC, 4)], U),
             ([(R.R_STRING, 4)], None), ([(R.R_SPRINT, 4)], None),
             ([(R.R_LIT, b"k"), (R.R_STRING, 5)], U), ([(R.R_SPRINT, 5)], U), ([(R.R_MARSHAL, 5)], U),
             ([(R.R_SPRINT, 1)], None), ([(R.R_MARSHAL, 0)], None)]
    outputs = [c[0] for c in cases]
    want = mirror(outputs, doc, vals[0], text[0])
    expected = [e if e is not None else (R.RENDER_OK, w) for (_, e), w in zip(cases, want)]
    return outputs, len(paths), [doc], vals, text, expected


def overflow_case():
    """out_stride 16: 10 bytes, then an output one byte longer than the 6 left, then one that
    fills them exactly."""
    doc = b'{"s":"abcde"}'
    vals, text = oracle_values([doc], ["s"])
    outputs = [[(R.R_LIT, b"0123456789")], [(R.R_LIT, b"xy"), (R.R_STRING, 0)], [(R.R_LIT, b"z"), (R.R_STRING, 0)]]
    expected = [(R.RENDER_OK, "0123456789"), (UNRENDERED, ""), (R.RENDER_OK, "zabcde")]
    return outputs, 1, [doc], vals, text, expected


def check_expected(rec, out_text, expected, r=0):
    for k, (st, w) in enumerate(expected):
        got_st, got = rendered(rec, out_text, r, k)
        assert got_st == st, (k, got_st, st, got)
        # (bytes that are not UTF-8 pass through STRING / SPRINT; the mirror's str has U+FFFD)
        assert got.decode("utf-8", "replace") == w, (k, got, w)


# ---- the case file of tests/native/san_render ----
def write_cases(path, cases):
    """cases: [(outputs, n_slots, docs, values, text, out_stride, expected)], expected[r][k] =
    (status, bytes)."""
    b = bytearray(struct.pack("<I", len(cases)))
    for outputs, n_slots, docs, vals, text, out_stride, expected in cases:
        b += struct.pack("<II", len(outputs), n_slots)
        for ops in outputs:
            b += struct.pack("<I", len(ops))
            for op, arg in ops:
                lit = bytes(arg) if op == R.R_LIT else b""
                b += struct.pack("<III", op, 0 if op == R.R_LIT else int(arg), len(lit)) + lit
        arena, offs, lens = pack(docs)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        b += struct.pack("<IIIII", len(docs), vals.shape[1], 0 if text is None else text.shape[1], out_stride,
                         0 if text is None else 1)
        b += struct.pack("<Q", arena.nbytes) + arena.tobytes() + offs.tobytes() + lens.tobytes() + vals.tobytes()
        if text is not None:
            b += np.ascontiguousarray(text, dtype=np.uint8).tobytes()
        for row in expected:
            for st, w in row:
                b += struct.pack("<II", st, len(w)) + w
    with open(path, "wb") as f:
        f.write(bytes(b))
