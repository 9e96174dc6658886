"""GPU: the host layer's buffers growing under a runtime that completes work asynchronously
(ajx_api.cpp's workspaces and staging buffer, ajx_hostbuf.h): one context and one stream
take batches of 3, 64, 65, 4097 and 130 requests in that order — across the 64-request row
rounding, the streaming / lean boundary (length order and work-item-ordered outputs come
into use) and back to a smaller batch — through eval_device, select_device,
select_from_eval_device and, at 65 and 4097, eval_host; every result against the oracle.
A buffer freed while the stream's earlier batch still used it would show as a wrong result."""
import numpy as np
import pytest

import pyoracle as O
from test_gpu_parity import _oracle

pytestmark = pytest.mark.gpu

SIZES = [3, 64, 65, 4097, 130]
SEL = ["a", "n"]


def test_buffers_grow_across_batch_sizes():
    import torch

    from authorino_amd import runtime
    from authorino_amd.jsonexp import All, Any, Pattern

    n_max = max(SIZES)
    docs = [b'{"a":"%s","n":%d,"b":"%d","id":%d}' % (b"y" if i % 3 == 0 else b"x", i % 11, i % 2, 1000 + i)
            for i in range(n_max)]
    lens = np.array([len(d) for d in docs], dtype=np.uint32)
    offs = np.zeros(n_max, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1])
    arena = np.frombuffer(b"".join(docs) + b"\0" * 64, dtype=np.uint8)
    sor = (np.arange(n_max, dtype=np.uint32) // 5) % 2
    ea = All(Pattern("a", "eq", "x"), Pattern("n", "neq", "7"))
    eb = Any(Pattern("a", "eq", "y"), Pattern("b", "eq", "1"))
    # the oracle once, over all documents: a batch of n is their first n
    oa = _oracle(ea, arena, offs, lens)
    osets = [O.Ruleset.from_expression(ea), O.Ruleset.from_expression(eb)]
    oab = _oracle(None, arena, offs, lens, set_of_req=sor, sets=osets)
    ospan = np.array([[O.gjson_span(d, p) for p in SEL] for d in docs], dtype=np.int64)  # (type, start, len)
    assert 0 < (oa[0] == runtime.T).sum() < n_max and 0 < (oab[0] == runtime.T).sum() < n_max

    ctx = runtime.Context(0)
    ra, rb = ctx.compile_expression(ea), ctx.compile_expression(eb)
    forest = ctx.compile_forest([ea], extra_selectors=SEL)
    rsel = ctx.compile([(p, 1, "") for p in SEL], [], -1)
    assert ra.n_patterns == 2 and forest.n_trees == 2 and forest.n_patterns == 4
    dev = torch.device("cuda", 0)
    A = torch.from_numpy(arena.copy()).to(dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream

    def same(got, want, n):
        for g, w in zip(got, want):
            assert np.array_equal(np.asarray(g).reshape(n, -1), np.asarray(w)[:n].reshape(n, -1))

    def spans(v, n):
        v = v.cpu().numpy()
        assert np.array_equal(v[:, :, 2] & 0xFF, ospan[:n, :, 0])
        assert np.array_equal(v[:, :, :2], ospan[:n, :, 1:])

    for n in SIZES:
        Of = torch.from_numpy(offs[:n].view(np.int64).copy()).to(dev)
        Ln = torch.from_numpy(lens[:n].view(np.int32).copy()).to(dev)
        Sr = torch.from_numpy(sor[:n].view(np.int32).copy()).to(dev)
        tri = torch.empty(n, dtype=torch.uint8, device=dev)
        err = torch.empty(n, dtype=torch.int32, device=dev)
        bm = torch.empty((n, 1), dtype=torch.int64, device=dev)
        tri2, err2, bm2 = torch.empty_like(tri), torch.empty_like(err), torch.empty_like(bm)
        trif = torch.empty(n * 2, dtype=torch.uint8, device=dev)
        vals = torch.empty((n, 2, 3), dtype=torch.int32, device=dev)
        vals2 = torch.empty_like(vals)
        torch.cuda.synchronize()
        ctx.eval_device([ra], A, Of, Ln, tri, err, bm, stream=s)
        ctx.eval_device([ra, rb], A, Of, Ln, tri2, err2, bm2, set_of_req=Sr, stream=s)
        ctx.select_device([rsel], A, Of, Ln, vals2, stream=s)
        ctx.eval_device([forest], A, Of, Ln, trif, stream=s)
        ctx.select_from_eval_device(forest, forest.n_patterns - 2, A, Of, Ln, vals, stream=s)
        stream.synchronize()
        same((tri.cpu(), err.cpu(), bm.cpu().numpy().view(np.uint64)), oa, n)
        same((tri2.cpu(), err2.cpu(), bm2.cpu().numpy().view(np.uint64)), oab, n)
        tf = trif.cpu().numpy().reshape(n, 2)
        assert np.array_equal(tf[:, 0], oa[0][:n]) and (tf[:, 1] == runtime.T).all()
        spans(vals, n)
        spans(vals2, n)
        if n in (65, 4097):
            same(ctx.eval_host_arena([ra], arena, offs[:n], lens[:n]), oa, n)
            same(ctx.eval_host_arena([ra, rb], arena, offs[:n], lens[:n], set_of_req=sor[:n]), oab, n)
    ctx.release_stream(s)
    ctx.close()
    other = runtime.Context(0)
    other.close()
