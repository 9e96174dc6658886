"""GPU parity of the lean kernel on the documents of tests/lean_reads_gen.py (the walker's
grouped ring reads at their edges, the key slots' child facts) against the oracle, through
the C-ABI: 193 requests (three waves and one lane: a partial wave), every document
misalignment 0..15, both walker instances (without and with an array-index selector). The
batch is forced onto the lean kernel (the streaming kernel would take one this small)."""
import numpy as np
import pytest

import lean_reads_gen as G
import pyoracle as O

pytestmark = pytest.mark.gpu

N = 193


@pytest.fixture(scope="module")
def ctx():
    from authorino_amd import runtime

    c = runtime.Context(0)
    c.set_kernel_mode(0)
    c.set_stream_max(0)  # every batch to the lean kernel
    yield c
    c.set_stream_max(4096)


def _pack_misaligned(docs):
    """Request r at arena offset = r mod 16 (mod 16): every misalignment, several times."""
    parts, offs, at = [], [], 0
    for r, d in enumerate(docs):
        gap = (r % 16 - at) % 16
        parts.append(b"\x7a" * gap)  # (neighbour bytes: not zeros)
        at += gap
        offs.append(at)
        parts.append(d)
        at += len(d)
    arena = np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8)
    return arena, np.array(offs, dtype=np.uint64), np.array([len(d) for d in docs], dtype=np.uint32)


@pytest.mark.parametrize("arr", [False, True], ids=["no_array_selector", "array_selector"])
def test_lean_kernel_matches_oracle_request_by_request(ctx, arr):
    pats = G.patterns(arr)
    nodes, root = G.chain(len(pats))
    docs = G.sample(N)
    arena, offs, lens = _pack_misaligned(docs)
    assert {int(o) % 16 for o in offs} == set(range(16))
    rs = ctx.compile(pats, nodes, root)
    tri, err, bm = ctx.eval_host_arena([rs], arena, offs, lens)
    otri, oerr, obm = O.eval_batch([O.Ruleset(pats, nodes, root)], arena, offs, lens, nthreads=4)
    bad = np.nonzero((tri != otri) | (err != oerr) | (bm[:, :obm.shape[1]] != obm).any(axis=1))[0]
    assert bad.size == 0, [(int(r), docs[r], int(tri[r]), int(otri[r]), int(err[r]), int(oerr[r]),
                            hex(int(bm[r, 0])), hex(int(obm[r, 0]))) for r in bad[:5]]
    assert len(set(otri.tolist())) > 1 or len({int(x) for x in obm[:, 0]}) > 8  # (the results vary)
