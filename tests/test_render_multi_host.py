"""The multi-program render kernel's per-request body (render_request_multi,
authorino_amd/csrc/ajx_render.h) on the CPU, as built (tests/native/render_multi_host.cpp):
a batch whose requests render different programs, or none, must give what one-program
calls over each program's requests give (render_request, pinned to the Python mirror by
tests/test_render_host.py), and leave the requests without a program alone. The kernel runs
the same body on the GPU in tests/test_gpu_render_multi.py."""
import subprocess

import numpy as np
import pytest

import _rendermulti as M
import _rendertest as T
from authorino_amd import response as R


@pytest.fixture(scope="module")
def setup():
    progs = M.programs()
    return progs, M.HostPrograms(progs), T.fuzz_docs(300)


def _case(setup, shape, out_stride):
    progs, host, docs = setup
    por = M.interleaving(len(docs), shape)
    values, text = M.batch_values(progs, por, docs)
    want_rec, want_out = M.expected(progs, por, docs, values, text, out_stride, host.one)
    return por, values, text, want_rec, want_out


@pytest.mark.parametrize("shape", ["alternating", "runs", "none"])
@pytest.mark.parametrize("out_stride", [16, 4096])
def test_interleaved_programs_equal_one_program_calls(setup, shape, out_stride):
    """Three programs and "no program" over 300 fuzz documents: every record and every byte
    of every output slot equals the one-program body's; a request without a program keeps
    its guard bytes in its slot and its records, and so do the records past a program's own
    outputs."""
    progs, host, docs = setup
    por, values, text, want_rec, want_out = _case(setup, shape, out_stride)
    rc, rec, out = host.multi(por, docs, values, text, out_stride)
    assert rc == 0
    assert np.array_equal(rec, want_rec)
    assert np.array_equal(out, want_out)
    idle = por == M.NONE
    assert (out[idle] == M.GUARD).all() and (rec[idle] == M.GUARD32).all()
    assert idle.sum() == (len(docs) if shape == "none" else len(docs) // 4)
    for i, (outputs, _, _) in enumerate(progs):
        assert (rec[por == i][:, len(outputs):] == M.GUARD32).all()
    if shape != "none" and out_stride == 4096:
        # the comparison is not of empty things: the 18 templates render the fuzz string
        # (the mirror's text of the first and the last one), c5's headers come out whole
        assert not (rec[por == 1][:, :18, 2] != R.RENDER_OK).any()
        r = int(np.flatnonzero(por == 1)[0])
        want = T.mirror(progs[1][0], docs[r], values[r], text[r])
        assert T.rendered(rec, out, r, 0)[1].decode("utf-8", "replace") == want[0] and want[0].endswith("x")
        assert T.rendered(rec, out, r, 17)[1].decode("utf-8", "replace") == want[17]
        assert want[17].startswith("ABCDEFGHIJKLMNOPQ")
        assert not (rec[por == 0][:, :4, 2] != R.RENDER_OK).any() and (rec[por == 0][:, 2, 1] > 2).all()


def test_an_implementation_that_renders_its_first_program_differs(setup):
    """The expectation tells the programs apart: the batch rendered with program 0 for every
    request is not what the interleaved batch must give."""
    progs, host, docs = setup
    por, values, text, want_rec, want_out = _case(setup, "alternating", 4096)
    rc, rec, out = host.multi(np.zeros(len(docs), dtype=np.uint32), docs, values, text, 4096)
    assert rc == 0 and not np.array_equal(rec, want_rec) and not np.array_equal(out, want_out)


def test_one_program_without_indices_and_argument_checks(setup):
    """prog_of_req NULL with one program renders it for every request; the harness keeps the
    entry point's argument table (strides below a program's need, a NULL program, several
    programs without indices); an index that is not below n_progs is "no program"."""
    progs, host, docs = setup
    docs = docs[:40]
    por = np.ones(len(docs), dtype=np.uint32)
    values, text = M.batch_values(progs, por, docs)
    want_rec, want_out = M.expected(progs, por, docs, values, text, 256, host.one)
    rc, rec, out = host.multi(None, docs, values, text, 256, handles=[host.h[1]])
    assert rc == 0 and np.array_equal(rec, want_rec) and np.array_equal(out, want_out)
    EINVAL = -1
    assert host.multi(None, docs, values, text, 256)[0] == EINVAL                    # 3 programs, no indices
    assert host.multi(por, docs, values, text, 24)[0] == EINVAL                      # out_stride % 16
    assert host.multi(por, docs, values, text, 0)[0] == EINVAL
    assert host.multi(por, docs, values, text, 256, records_stride=17)[0] == EINVAL  # below 18 outputs
    assert host.multi(por, docs, values[:, :7], text, 256)[0] == EINVAL              # below 8 slots
    assert host.multi(por, docs, values, text, 256, handles=[host.h[0], None, host.h[2]])[0] == EINVAL
    por[::3] = 3  # (not below n_progs = 3, and not 0xFFFFFFFF)
    want_rec, want_out = M.expected(progs, por, docs, values, text, 256, host.one)
    rc, rec, out = host.multi(por, docs, values, text, 256)
    assert rc == 0 and np.array_equal(rec, want_rec) and np.array_equal(out, want_out)
    assert (out[::3] == M.GUARD).all()


def test_sanitizer_program(setup, tmp_path):
    """tests/native/san_render_multi (ASan + UBSan, its own main) over the alternating and
    the run-wise interleavings at out_stride 4096 and 16 and the batch without programs:
    exit 0. A request without a program gets null buffers there."""
    progs, host, docs = setup
    cases = []
    for shape, out_stride in (("alternating", 4096), ("runs", 16), ("alternating", 16), ("none", 4096)):
        por, values, text, want_rec, want_out = _case(setup, shape, out_stride)
        cases.append((progs, por, docs, values, text, out_stride, want_rec, want_out))
    path = tmp_path / "cases.bin"
    M.write_cases(str(path), cases)
    p = subprocess.run([M.make("san_render_multi"), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "4 cases, 1200 requests (525 without a program)" in p.stdout
