"""GPU parity of the lean kernels with lanes taking the next sub-window's tokens early
(ajx_lean.h, Walk::walk) against the oracle, through the C-ABI: waves whose
lanes finish a sub-window at different times (that is when a lane takes tokens early), a
partial wave (inactive lanes in the loop's ballot), the edge family of
tests/lean_borrow_gen.py on both walker instances, a forest with kept rows read back by
select_from_eval_device, and a two-ruleset batch through the multi-tenant kernel. Small
batches are forced onto the lean kernel (the streaming kernel would take them)."""
import numpy as np
import pytest

import fuzz_util as FU
import lean_borrow_gen as B
import pyoracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from authorino_amd import runtime

    c = runtime.Context(0)
    c.set_kernel_mode(0)
    c.set_stream_max(0)  # every batch to the lean kernel
    yield c
    c.set_stream_max(4096)


def _pack(docs, misalign=True):
    """Request r at arena offset = r mod 16 (mod 16): every misalignment."""
    parts, offs, at = [], [], 0
    for r, d in enumerate(docs):
        gap = ((r % 16 if misalign else 0) - at) % 16
        parts.append(b"\x7a" * gap)  # (neighbour bytes: not zeros)
        at += gap
        offs.append(at)
        parts.append(d)
        at += len(d)
    arena = np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8)
    return arena, np.array(offs, dtype=np.uint64), np.array([len(d) for d in docs], dtype=np.uint32)


def _same_as_oracle(ctx, pats, docs, valid, misalign=True):
    """Bit-exact tri-state, error index and bitmap; no request undecided; none on the exact
    path when every document is valid."""
    from authorino_amd import runtime

    nodes, root = FU.chain(len(pats))
    arena, offs, lens = _pack(docs, misalign)
    rs = ctx.compile(pats, nodes, root)
    tri, err, bm = ctx.eval_host_arena([rs], arena, offs, lens)
    exact = ctx.last_exact_count()
    otri, oerr, obm = O.eval_batch([O.Ruleset(pats, nodes, root)], arena, offs, lens, nthreads=4)
    bad = np.nonzero((tri != otri) | (err != oerr) | (bm[:, :obm.shape[1]] != obm).any(axis=1))[0]
    assert bad.size == 0, [(int(r), docs[r], int(tri[r]), int(otri[r]), int(err[r]), int(oerr[r]),
                            hex(int(bm[r, 0])), hex(int(obm[r, 0]))) for r in bad[:5]]
    assert (tri == runtime.UNDECIDED).sum() == 0
    if valid:
        assert exact == 0
    return otri, obm


def test_one_wave_dense_and_sparse_lanes(ctx):
    """64 requests, one wave: documents of many short members alternate with documents of a
    few long strings of the same length, so half the lanes are done with each sub-window
    while the others work."""
    docs = [(B.dense_doc if r % 2 else B.sparse_doc)(700 + 8 * (r // 2 % 4)) for r in range(64)]
    pats = B.EDGE_PATS + [("a3", 1, "3"), ("a7", 2, "0"), ("pad", 2, "")]
    _same_as_oracle(ctx, pats, docs, valid=True, misalign=False)
    _same_as_oracle(ctx, pats, docs, valid=True)


@pytest.mark.parametrize("arr", [False, True], ids=["no_array_selector", "array_selector"])
def test_partial_wave_every_misalignment(ctx, arr):
    """193 requests (three waves and one lane) of the edge family, every misalignment."""
    valid = [d for d, ok in B.edge_docs() if ok]
    docs = [valid[(i * 37) % len(valid)] for i in range(193)]
    otri, obm = _same_as_oracle(ctx, B.EDGE_ARR_PATS if arr else B.EDGE_PATS, docs, valid=True)
    assert len({int(x) for x in obm[:, 0]}) > 8  # (the results vary)


@pytest.mark.parametrize("arr", [False, True], ids=["no_array_selector", "array_selector"])
def test_edge_family(ctx, arr):
    """Every document of the edge family: the unbroken ones all decided by the lean kernel,
    then those mixed with the broken and cut ones (the exact scan may take these)."""
    pats = B.EDGE_ARR_PATS if arr else B.EDGE_PATS
    every = list(B.edge_docs())
    _same_as_oracle(ctx, pats, [d for d, ok in every if ok], valid=True)
    _same_as_oracle(ctx, pats, [d for d, _ in every], valid=False)


def test_forest_kept_rows_and_select_from_eval(ctx):
    """c5's forest with its response selectors as the last tree: the spans read from the
    evaluation's kept capture rows equal select_device's own scan, the trees' results those
    of the forest without the selectors, and the first tree's the oracle's."""
    import torch

    from authorino_amd import runtime, workloads
    from authorino_amd.response import ResponseSelectors

    w = workloads.make("c5", n=2048, seed=58)
    cfg = w.auth_config
    exprs = [cfg.conditions] + [e for c in cfg.authorization for e in (c.conditions, c.rules)]
    sel = ResponseSelectors(cfg.response, ctx)
    plain = ctx.compile_forest(exprs)
    fused = ctx.compile_forest(exprs, extra_selectors=sel.paths)
    k = len(sel.paths)
    dev = torch.device("cuda", 0)
    A = torch.from_numpy(w.arena).to(dev)
    Of = torch.from_numpy(w.offs.view(np.int64)).to(dev)
    Ln = torch.from_numpy(w.lens.view(np.int32)).to(dev)

    def run(rs):
        tri = torch.empty(w.n * rs.n_trees, dtype=torch.uint8, device=dev)
        bm = torch.empty((w.n, (rs.n_patterns + 63) // 64), dtype=torch.int64, device=dev)
        ctx.eval_device([rs], A, Of, Ln, tri, None, bm)
        return tri

    tri_f = run(fused)
    got = torch.empty((w.n, k, 3), dtype=torch.int32, device=dev)
    ctx.select_from_eval_device(fused, fused.n_patterns - k, A, Of, Ln, got)
    torch.cuda.synchronize()
    assert ctx.last_exact_count() == 0
    want = torch.empty((w.n, k, 3), dtype=torch.int32, device=dev)
    ctx.select_device([sel.ruleset], A, Of, Ln, want)
    tri_p = run(plain)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    tf = tri_f.cpu().numpy().reshape(w.n, fused.n_trees)
    assert np.array_equal(tf[:, :plain.n_trees], tri_p.cpu().numpy().reshape(w.n, plain.n_trees))
    assert (tf != runtime.UNDECIDED).all()
    otri, _, _ = O.eval_batch([O.Ruleset.from_expression(exprs[0])], w.arena, w.offs, w.lens, nthreads=4)
    assert np.array_equal(tf[:, 0], otri)


def test_two_rulesets_through_the_tenant_kernel(ctx):
    """4160 requests (65 waves) of two rulesets, bucketed by ruleset: uniform waves of
    either, and the one wave where they meet."""
    from authorino_amd import runtime, workloads

    w = workloads.make("c2", n=4160, seed=59)
    exprs = [w.expr, workloads.c3_expression()]
    sor = (np.arange(w.n) >= 2080).astype(np.uint32)
    rss = [ctx.compile_expression(e) for e in exprs]
    tri, err, bm = ctx.eval_host_arena(rss, w.arena, w.offs, w.lens, set_of_req=sor)
    assert ctx.last_exact_count() == 0
    otri, oerr, obm = O.eval_batch([O.Ruleset.from_expression(e) for e in exprs], w.arena, w.offs, w.lens,
                                   set_of_req=sor, nthreads=4)
    assert np.array_equal(tri, otri) and np.array_equal(err, oerr) and np.array_equal(bm[:, :obm.shape[1]], obm)
    assert (tri == runtime.UNDECIDED).sum() == 0
    assert len(set(otri[:2080].tolist())) > 1 or len(set(otri[2080:].tolist())) > 1
