"""Every writer of stage B's outputs against the oracle, through Context.eval_device on tensors
the test fills itself: tri-states 0xEE, error indices -7, a T bitmap of all-ones whose rows
are two words wider than the rulesets need (a word the kernels must zero shows when they do
not). One request per wave (the streaming kernel's wave-cooperative stage B), two per wave
(its per-lane stage B and the fold of the requests the stream decides alone), the lean
kernel in length order with the outputs gathered back, and the streaming and multi-tenant
kernels on two-ruleset batches (csrc/ajx_plan.h has the cut-offs; the writers are
write_bitmap / fold_outputs in csrc/ajx_stageb.h and fold_outputs_wave in csrc/ajx_stream.h).
Reference: pkg/jsonexp/expressions.go:59-154."""
import numpy as np
import pytest

import fuzz_util as FU
import pyoracle as O
from authorino_amd import jsonexp as J

pytestmark = pytest.mark.gpu

N_DOCS = 300
# the smallest batches that reach each writer under plan_eval's cut-offs (csrc/ajx_plan.h: the
# stream takes n <= 4096 at ceil(n / 2048) requests per wave; tests/test_plan.py pins that
# table): if the cut-offs move, move these with them
SIZES = [1, 2100, 4500]
T, F = 1, 0


def _p(sel, op, val):
    return J.Pattern(sel, J.Operator(op), val)


EQ, NEQ, INCL, EXCL, RX = 1, 2, 3, 4, 5
NO_V = "^[^v]*$"  # (true of a selector that is not found: Null's String() is "")


def _flat():
    return J.All(_p("a", RX, NO_V), _p("b", NEQ, "x"), _p("c", EQ, ""))


def _group():
    return J.All(J.Any(_p("a", RX, NO_V), _p("b", EQ, "hello")), J.Any(_p("c", EQ, ""), _p("n", NEQ, "")),
                 _p("ab", NEQ, "x"))


def _deep():
    return J.All(J.Any(J.All(_p("a", RX, NO_V), _p("b", NEQ, "x")), _p("c", EQ, "1")), _p("n", EQ, ""))


def _forest():
    """a flat tree (base 0), a two-level tree (base 40: it straddles bit 64) and a three-level
    tree (base 70)"""
    keys = ["a", "b", "c", "ab", "n", "0", "1", "long-key-name"]
    flat = J.All(*[_p(keys[i % 8], RX, NO_V) if i % 5 == 0 else _p(keys[i % 8], NEQ, "v%d" % i) for i in range(40)])
    groups = [J.Any(*[_p(keys[(5 * g + j) % 8], RX, NO_V) if j == 0 else _p(keys[(5 * g + j) % 8], EQ, "v%d" % j)
                      for j in range(5)]) for g in range(5)]
    two = J.All(*groups, *[_p(keys[i], NEQ, "hello") for i in range(5)])
    return [flat, two, _deep()]


def _eager():
    return J.Any(_p("a", EQ, "x"), _p("b", EQ, "v1"), _p("c", EQ, ""))


RULESETS = {"flat": _flat, "group": _group, "deep": _deep, "eager": _eager}


@pytest.fixture(scope="module")
def ctx():
    from authorino_amd import runtime

    yield runtime.Context(0)


@pytest.fixture(scope="module")
def docs():
    rng = np.random.default_rng(5100)
    seen, out = set(), []
    while len(out) < N_DOCS:
        d = FU.rand_doc(rng)
        if d not in seen:
            seen.add(d)
            out.append(d)
    return out


def _pack(ds):
    lens = np.array([len(d) for d in ds], dtype=np.uint32)
    offs = np.zeros(len(ds), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(ds) + b"\0" * 64, dtype=np.uint8), offs, lens


def _spec(expr):
    pats, nodes, root = expr.flatten()
    return [(p.selector, int(p.operator), p.value) for p in pats], nodes, root


@pytest.fixture(scope="module")
def oracle(docs):
    """name -> (tri, err, bm) of the N_DOCS distinct documents, computed once; a forest's per
    tree, its trees' bitmaps joined at their pattern bases"""
    arena, offs, lens = _pack(docs)
    out = {}
    for name, make in RULESETS.items():
        out[name] = O.eval_batch([O.Ruleset(*_spec(make()))], arena, offs, lens, nthreads=8)
    tris, errs, base = [], [], 0
    bits = np.zeros((N_DOCS, 128), dtype=bool)
    for e in _forest():
        spec = _spec(e)
        tri, err, bm = O.eval_batch([O.Ruleset(*spec)], arena, offs, lens, nthreads=8)
        n = len(spec[0])
        tris.append(tri)
        errs.append(np.where(err >= 0, err + base, -1))
        for p in range(n):
            bits[:, base + p] = (bm[:, p >> 6] >> np.uint64(p & 63)) & np.uint64(1) != 0
        base += n
    assert 64 < base <= 128
    words = np.zeros((N_DOCS, 2), dtype=np.uint64)
    for p in range(base):
        words[:, p >> 6] |= bits[:, p].astype(np.uint64) << np.uint64(p & 63)
    out["forest"] = (np.stack(tris, axis=1), np.stack(errs, axis=1).astype(np.int32), words)
    for name, (tri, _, _) in out.items():  # (both outcomes occur, in every tree)
        assert (tri == T).any(axis=0).all() and (tri == F).any(axis=0).all(), name
    return out


def _run(ctx, sets, ds, sor=None):
    """the batch on poisoned outputs: (tri [n, trees], err [n, trees], bm [n, words + 2])"""
    import torch

    dev = torch.device("cuda", 0)
    arena, offs, lens = _pack(ds)
    n, nt = len(ds), sets[0].n_trees
    words = max((s.n_patterns + 63) // 64 for s in sets)
    A = torch.from_numpy(arena.copy()).to(dev)
    Of = torch.from_numpy(offs.view(np.int64)).to(dev)
    Ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    S = torch.from_numpy(sor.astype(np.int32)).to(dev) if sor is not None else None
    tri = torch.full((n * nt,), 0xEE, dtype=torch.uint8, device=dev)
    err = torch.full((n * nt,), -7, dtype=torch.int32, device=dev)
    bm = torch.full((n, words + 2), -1, dtype=torch.int64, device=dev)
    ctx.eval_device(sets, A, Of, Ln, tri, err, bm, set_of_req=S)
    torch.cuda.synchronize()
    return (tri.cpu().numpy().reshape(n, nt), err.cpu().numpy().reshape(n, nt),
            bm.cpu().numpy().view(np.uint64))


def _check(got, want, idx):
    """got against the oracle's rows idx (want: tri, err, bm of the distinct documents)"""
    tri, err, bm = got
    otri, oerr, obm = (np.asarray(x)[idx] for x in want)
    n = len(idx)
    assert np.array_equal(tri, otri.reshape(n, -1))
    assert np.array_equal(err, oerr.reshape(n, -1))
    w = obm.shape[1]
    assert np.array_equal(bm[:, :w], obm)
    assert not bm[:, w:].any()  # (the words beyond the ruleset's are zero)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["flat", "group", "deep", "forest", "eager"])
def test_outputs(ctx, docs, oracle, name, n):
    rs = ctx.compile_forest(_forest()) if name == "forest" else ctx.compile_expression(RULESETS[name]())
    assert rs.n_trees == (3 if name == "forest" else 1)
    if n == 1:  # (one launch per document: a few that are T and a few that are F)
        tri0 = np.asarray(oracle[name][0]).reshape(N_DOCS, -1)[:, 0]
        picks = list(np.nonzero(tri0 == T)[0][:3]) + list(np.nonzero(tri0 == F)[0][:3])
        for i in picks:
            _check(_run(ctx, [rs], [docs[i]]), oracle[name], np.array([i]))
        return
    idx = np.arange(n) % N_DOCS
    _check(_run(ctx, [rs], [docs[i] for i in idx]), oracle[name], idx)


@pytest.mark.parametrize("n", [2, 4500])
def test_outputs_two_rulesets(ctx, docs, oracle, n):
    """set_of_req over two rulesets: the streaming kernel's multi-tenant instance (n = 2) and
    the multi-tenant kernel (runs of 100 requests per ruleset: waves of one ruleset and of both)"""
    sets = [ctx.compile_expression(_flat()), ctx.compile_expression(_group())]
    idx = np.arange(n) % N_DOCS
    sor = (np.arange(n) // 100) % 2 if n > 2 else np.array([0, 1])
    tri, err, bm = _run(ctx, sets, [docs[i] for i in idx], sor.astype(np.uint32))
    for k, name in enumerate(["flat", "group"]):
        m = sor == k
        _check((tri[m], err[m], bm[m]), oracle[name], idx[m])
