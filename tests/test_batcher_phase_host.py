"""Phase requests through the micro-batcher's queue (authorino_amd/csrc/ajx_batcher.h) and
the phase plan and delivery the device batcher runs (ajx_phase.h plan_phases /
deliver_phase), on the CPU with a stand-in for the device work
(tests/native/batcher_phase_host.cpp): phase requests of phases with different strides and
eval-only requests share batches, every caller gets its own decision, records and bytes
through the plan's index mapping, nothing of a staging slot past a request's last output
reaches its caller, and a timed-out request's buffers are untouched. The device-backed call
is tested in tests/test_gpu_batcher_phase.py."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
ETIMEDOUT = -5
GUARD, GUARD32 = 0xA5, 0xA5A5A5A5
# (n_outputs, text_stride, out_stride, ruleset id): c5-like, the 18 templates, no outputs, and
# six outputs in a slot of 16 bytes (some do not fit); two stride shapes, two rulesets
SHAPES = [(4, 64, 128, 1), (18, 64, 128, 2), (0, 0, 16, 1), (6, 0, 16, 2)]


def _make(target):
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "batcher_phase.mk", target], check=True, timeout=600)
    return os.path.join(_NATIVE, target)


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(_make("libajx_batchphase.so"))
    L.hbp_create.argtypes = [C.c_uint32] * 5
    L.hbp_create.restype = C.c_void_p
    L.hbp_phase_new.argtypes = [C.c_uint64, C.c_uint64] + [C.c_uint32] * 4
    L.hbp_phase_new.restype = C.c_void_p
    L.hbp_phase_free.argtypes = [C.c_void_p]
    L.hbp_call.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint8, C.c_void_p, C.c_uint64, C.c_void_p,
                           C.c_void_p, C.c_void_p]
    L.hbp_call.restype = C.c_int
    L.hbp_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.hbp_destroy.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def phases(lib):
    hs = [lib.hbp_phase_new(100 + i, 200 + i, 8, k, ts, os_) for i, (k, ts, os_, _) in enumerate(SHAPES)]
    yield hs
    for h in hs:
        lib.hbp_phase_free(h)


def _stats(L, h):
    out = (C.c_uint64 * 8)()
    L.hbp_stats(h, out)
    return dict(zip(("batches", "requests", "expired", "max_batch", "plan_violations", "groups", "mixed_batches",
                     "phase_requests"), out))


def _expected(i, byte):
    """(records [n_outputs][3], text) of phase i on a document byte (the stand-in's render)."""
    k, _, os_, _ = SHAPES[i]
    rec, text, pos = [], b"", 0
    for q in range(k):
        ln = 1 + (byte + q) % 5
        if pos + ln > os_:
            rec.append([pos, 0, 1])
            continue
        rec.append([pos, ln, 0])
        text += bytes([(byte ^ q ^ (200 + i)) & 0xFF]) * ln
        pos += ln
    return rec, text


def _call(L, h, phases, i, byte, timeout_us=0):
    """One request of phase i (None: eval only): (rc, tri, text u8[128], rec u32[18][3]),
    the output buffers guard-filled before the call."""
    tri = np.full(2, GUARD, dtype=np.uint8)
    text = np.full(128, GUARD, dtype=np.uint8)
    rec = np.full((18, 3), GUARD32, dtype=np.uint32)
    rs = SHAPES[i][3] if i is not None else 2
    rc = L.hbp_call(h, rs, 1, byte, phases[i] if i is not None else None, timeout_us, tri.ctypes.data,
                    text.ctypes.data, rec.ctypes.data)
    return rc, rs, tri, text, rec


def _check(i, byte, rs, tri, text, rec):
    assert tri[0] == (byte ^ rs) & 0xFF and tri[1] == GUARD
    if i is None:
        assert (text == GUARD).all() and (rec == GUARD32).all()
        return
    want_rec, want_text = _expected(i, byte)
    assert rec[:len(want_rec)].tolist() == want_rec and (rec[len(want_rec):] == GUARD32).all()
    assert text[:len(want_text)].tobytes() == want_text and (text[len(want_text):] == GUARD).all()


def test_eight_producers_get_their_own_outputs(lib, phases):
    h = lib.hbp_create(64, 500, 100, 2, 0)
    errors = []

    def producer(t):
        kinds = np.random.default_rng(t).integers(0, 5, 400)  # (4: an eval-only request)
        try:
            for j in range(400):
                i = None if kinds[j] == 4 else int(kinds[j])
                byte = (t * 31 + j * 7) & 0xFF
                rc, rs, tri, text, rec = _call(lib, h, phases, i, byte)
                assert rc == 0
                _check(i, byte, rs, tri, text, rec)
        except AssertionError as e:
            errors.append(repr(e))

    ts = [threading.Thread(target=producer, args=(t,)) for t in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    st = _stats(lib, h)
    lib.hbp_destroy(h)
    assert not errors, errors[:3]
    print(st)
    assert st["requests"] == 3200 and 2200 < st["phase_requests"] < 2900 and st["plan_violations"] == 0
    # phase and eval-only requests shared batches, and batches held both stride shapes
    assert st["mixed_batches"] > 0 and st["max_batch"] > 2 and st["groups"] > st["batches"] // 2
    # a declined output was among them (six outputs in 16 bytes), and one that fits exactly
    assert any(r[2] for b in range(256) for r in _expected(3, b)[0])


def test_timed_out_request_keeps_its_buffers(lib, phases):
    """20 ms per batch of at most 2 and a 5 ms deadline: most requests expire in the queue,
    with AUTHJX_ETIMEDOUT and guard-filled buffers; the others are right."""
    h = lib.hbp_create(2, 200, 20000, 1, 0)
    results = [None] * 24

    def call(k):
        results[k] = _call(lib, h, phases, k % 4, k, timeout_us=5000)

    ts = [threading.Thread(target=call, args=(k,)) for k in range(24)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    st = _stats(lib, h)
    lib.hbp_destroy(h)
    late = [k for k in range(24) if results[k][0] == ETIMEDOUT]
    done = [k for k in range(24) if results[k][0] == 0]
    assert len(late) + len(done) == 24 and len(late) >= 12 and done and st["expired"] == len(late)
    for k in late:
        _, _, tri, text, rec = results[k]
        assert (tri == GUARD).all() and (text == GUARD).all() and (rec == GUARD32).all()
    for k in done:
        _check(k % 4, k, *results[k][1:])


def test_tsan_program():
    """tests/native/tsan_phase (ThreadSanitizer, its own main): the same producers, two
    workers, deadlines; exit 0 and no report."""
    p = subprocess.run([_make("tsan_phase")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "tsan_phase: 0 mismatches" in p.stdout and "ThreadSanitizer" not in p.stderr


def test_phase_api_sanitizer_program():
    """tests/native/phase_api_host (ASan + UBSan, its own main): authjx_phase_create's
    argument table and packed batches of two phases with different strides next to
    eval-only requests through authjx_batcher_phase, zero-copy on and off, on the host
    stand-in of the HIP runtime (exact-size allocations; the render launches run the
    kernels' per-request bodies on the host)."""
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "phase_api.mk", "phase_api_host"], check=True, timeout=600)
    p = subprocess.run([os.path.join(_NATIVE, "phase_api_host")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok ") and "0 failed" in p.stdout
