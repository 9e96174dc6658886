"""GPU tests of response header values rendered on the device (authjx_render_*,
authorino_amd/csrc/ajx_render.hip): the kernel's outputs against the Python mirror
(authorino_amd/response.py's host functions over the oracle's gjson; tests/_rendertest.py),
never against another run of the same code. The per-request logic's CPU checks are
tests/test_render_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from authorino_amd import runtime

    return runtime.Context(0)


@pytest.fixture(scope="module")
def fuzz(ctx):
    """258 fuzz documents, their values from the select kernel (one ruleset of every fuzz
    path) and the render program of every value under every op."""
    import _rendertest as T

    docs = T.fuzz_docs(258, seed=23)
    rs = ctx.compile([(p, 1, "") for p in T.FUZZ_PATHS], [], -1)
    assert all(s == 0 for s in rs.status)
    prog = ctx.compile_render(T.FUZZ_OUTPUTS, len(T.FUZZ_PATHS))
    assert prog.n_outputs == len(T.FUZZ_OUTPUTS)
    return docs, rs, prog


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_block_edges(ctx, fuzz, n):
    """n requests through select_text_host_arena then render_host_arena: every output equals
    the mirror, none declined, and neither the slot bytes past a request's last output nor
    the slot after the batch's last are touched (0xA5 pre-fill)."""
    import _rendertest as T
    from authorino_amd import response as R

    docs, rs, prog = fuzz
    docs = docs[:n]
    arena, offs, lens = T.pack(docs)
    vals, text = ctx.select_text_host_arena([rs], arena, offs, lens)
    assert not ((vals[:, :, 2] & 0xFF) == 255).any()
    slots = np.full((n + 1, T.FUZZ_STRIDE), 0xA5, dtype=np.uint8)
    rec, out = ctx.render_host_arena(prog, arena, offs, lens, vals, text, out_text=slots)
    assert out is slots and rec.shape == (n, len(T.FUZZ_OUTPUTS), 3)
    assert not (rec[:, :, 2] != R.RENDER_OK).any()
    ends = T.check_all(rec, out, T.FUZZ_OUTPUTS, docs, vals, text, T.FUZZ_STRIDE)
    for r, e in enumerate(ends):
        assert (out[r, (e + 3) // 4 * 4:] == 0xA5).all(), r
    assert (out[n] == 0xA5).all()


def test_store_alignment(ctx):
    """LIT(a) STRING LIT(b) for a = 0..17, b = 0..3 over strings of 0..33 bytes: every start
    alignment and tail length of the packed stores. One output per program at out_stride 256
    (all exact) and 16 (exact when it fits, UNRENDERED when not); and the 18 templates of
    each b as one program, so that outputs also start where the one before ended."""
    import _rendertest as T
    from authorino_amd import response as R

    docs = [('{"s":"%s"}' % "abcdefghijklmnopqrstuvwxyz0123456"[:k]).encode() for k in range(34)]
    arena, offs, lens = T.pack(docs)
    rs = ctx.compile([("s", 1, "")], [], -1)
    vals, text = ctx.select_text_host_arena([rs], arena, offs, lens)
    shapes = [(a, b) for a in range(18) for b in range(4)]
    lit = b"ABCDEFGHIJKLMNOPQR"
    outputs = [[(R.R_LIT, lit[:a]), (R.R_STRING, 0), (R.R_LIT, b"xyz"[:b])] for a, b in shapes]
    outputs = [[op for op in o if op[0] != R.R_LIT or op[1]] for o in outputs]
    for b in range(4):
        sub = [o for o, (_, bb) in zip(outputs, shapes) if bb == b]
        prog = ctx.compile_render(sub, 1)
        slots = np.full((len(docs) + 1, 1024), 0xA5, dtype=np.uint8)
        rec, out = ctx.render_host_arena(prog, arena, offs, lens, vals, text, out_text=slots)
        ends = T.check_all(rec, out, sub, docs, vals, text, 1024)
        for r, e in enumerate(ends):
            assert (out[r, (e + 3) // 4 * 4:] == 0xA5).all(), (b, r)
        assert (out[len(docs)] == 0xA5).all()
    for stride in (256, 16):
        for (a, b), o in zip(shapes, outputs):
            prog = ctx.compile_render([o], 1)
            slots = np.full((len(docs) + 1, stride), 0xA5, dtype=np.uint8)
            rec, out = ctx.render_host_arena(prog, arena, offs, lens, vals, text, out_text=slots)
            for r in range(len(docs)):
                want = lit[:a] + docs[r][6:-2] + b"xyz"[:b]
                st, got = T.rendered(rec, out, r, 0)
                if len(want) <= stride:
                    assert (st, got) == (R.RENDER_OK, want), (stride, a, b, r)
                    assert (out[r, (len(want) + 3) // 4 * 4:] == 0xA5).all()
                else:
                    assert (st, got) == (R.RENDER_UNRENDERED, b""), (stride, a, b, r)
            assert (out[len(docs)] == 0xA5).all()


def test_device_resident_c5_headers(ctx):
    """eval_device on a forest whose last tree is the response selectors, then
    select_from_eval_device, then render_device, one stream, 2048 c5 requests: the four
    headers of every granted request equal the oracle pipeline's."""
    import torch

    import _rendertest as T
    from authorino_amd import pipeline as P, response as R, workloads
    from test_pipeline_host import OracleCtx

    w = workloads.make("c5", n=2048)
    cfg = w.auth_config
    docs = [w.doc(i) for i in range(w.n)]
    exprs = [cfg.conditions] + [e for c in cfg.authorization for e in (c.conditions, c.rules)]
    sel = R.ResponseSelectors(cfg.response, ctx)
    ops, keys = R.compile_render(cfg.response, sel)
    prog = ctx.compile_render(ops.outputs, ops.n_slots)
    k = len(sel.paths)
    fused = ctx.compile_forest(exprs, extra_selectors=sel.paths)
    dev = torch.device("cuda", 0)
    A = torch.from_numpy(w.arena).to(dev)
    Of = torch.from_numpy(w.offs.view(np.int64)).to(dev)
    Ln = torch.from_numpy(w.lens.view(np.int32)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    stride = 512
    with torch.cuda.stream(stream):
        tri = torch.empty(w.n * fused.n_trees, dtype=torch.uint8, device=dev)
        vals = torch.empty((w.n, k, 3), dtype=torch.int32, device=dev)
        out_text = torch.empty((w.n, stride), dtype=torch.uint8, device=dev)
        rec = torch.empty((w.n, prog.n_outputs, 3), dtype=torch.int32, device=dev)
        s = stream.cuda_stream
        ctx.eval_device([fused], A, Of, Ln, tri, stream=s)
        ctx.select_from_eval_device(fused, fused.n_patterns - k, A, Of, Ln, vals, stream=s)
        ctx.render_device(prog, A, Of, Ln, vals, out_text, rec, stream=s)
    stream.synchronize()
    ctx.release_stream(stream.cuda_stream)
    rec = rec.cpu().numpy().view(np.uint32)
    rec[:, :, 2] &= 0xFF
    text = out_text.cpu().numpy()
    assert not rec[:, :, 2].any()
    want = P.AuthPipelineBatch(cfg, ctx=OracleCtx()).evaluate(docs)
    granted = 0
    for r, res in enumerate(want):
        if res.code != P.CODE_OK or res.skipped:
            continue
        granted += 1
        got = {key: T.rendered(rec, text, r, j)[1].decode("utf-8", "replace") for j, key in enumerate(keys)}
        assert got == res.headers, r
        assert "e+09" in got["x-auth-exp"]
    assert 0 < granted < w.n


def test_pipeline_headers_from_device(ctx):
    """AuthPipelineBatch on the real context takes header text from the device (rendered > 0,
    no fallback) and equals the oracle run; a depth-9 value under a MARSHAL property falls
    back for that header alone, with the same result."""
    from authorino_amd import jsonexp as J, pipeline as P, response as R
    from test_pipeline_host import OracleCtx, _doc
    import _rendertest as T

    def cfg():
        resp = [R.ResponseConfig("p", plain=R.JSONValue(pattern="auth.identity.sub"), wrapper_key="x-sub"),
                R.ResponseConfig("j", json_properties=[("g", R.JSONValue(pattern="auth.identity.groups")),
                                                       ("s", R.JSONValue(static="k")),
                                                       ("t", R.JSONValue(pattern="{context.request.http.method} "
                                                                                 "{auth.identity.sub}"))],
                                 wrapper_key="x-json"),
                R.ResponseConfig("w", plain=R.JSONValue(pattern="auth.identity.groups"), wrapper_key="x-when",
                                 conditions=J.All(J.Pattern("auth.identity.sub", J.EqualOperator, "bob")), priority=1),
                R.ResponseConfig("m", plain=R.JSONValue(pattern="auth.identity.sub"),
                                 wrapper=R.ENVOY_DYNAMIC_METADATA_WRAPPER, wrapper_key="meta"),
                R.ResponseConfig("d", json_properties=[("deep", R.JSONValue(pattern="auth.metadata.deep"))],
                                 wrapper_key="x-deep")]
        return P.AuthConfig(authorization=[P.AuthorizationConfig(
            "a", rules=J.All(J.Pattern("auth.identity.groups", J.IncludesOperator, "users")))], response=resp)

    docs = [_doc(sub="alice", groups=("users", "devs")), _doc(sub="bob", groups=("users",)),
            _doc(sub="carol", groups=("admins",))]
    want = P.AuthPipelineBatch(cfg(), ctx=OracleCtx()).evaluate(docs)
    batch = P.AuthPipelineBatch(cfg(), ctx=ctx)
    got = batch.evaluate(docs)
    assert [(r.code, r.headers, r.metadata) for r in got] == [(r.code, r.headers, r.metadata) for r in want]
    assert got[0].headers["x-json"] == '{"g":["users","devs"],"s":"k","t":"GET alice"}'
    assert got[1].headers["x-when"] == "[users]" and got[0].headers["x-deep"] == '{"deep":null}'
    assert batch.selectors.rendered == 7 and batch.selectors.fallbacks == 0
    deep = _doc(sub="dan", groups=("users",)).replace(b'"metadata":{}', b'"metadata":{"deep":%s}'
                                                      % T.nested(9).encode())
    assert b'"deep":[' in deep
    want = P.AuthPipelineBatch(cfg(), ctx=OracleCtx()).evaluate(docs + [deep])
    batch = P.AuthPipelineBatch(cfg(), ctx=ctx)
    got = batch.evaluate(docs + [deep])
    assert [(r.code, r.headers, r.metadata) for r in got] == [(r.code, r.headers, r.metadata) for r in want]
    assert got[3].headers["x-deep"].startswith('{"deep":[{"a":null,"b":[')
    assert batch.selectors.fallbacks == 1 and batch.selectors.rendered == 7 + 2


def test_decline_reasons_on_device(ctx):
    """tests/test_render_host.py's decline cases through the kernel, and the entry points'
    argument checks."""
    import _rendertest as T
    from authorino_amd import response as R, runtime

    outputs, n_slots, docs, vals, text, expected = T.decline_case(8)
    arena, offs, lens = T.pack(docs)
    prog = ctx.compile_render(outputs, n_slots)
    rec, out = ctx.render_host_arena(prog, arena, offs, lens, vals, text)
    T.check_expected(rec, out, expected)
    assert T.rendered(rec, out, 0, 7)[1] == b"a\xffb\n"
    outputs, n_slots, docs, vals, text, expected = T.overflow_case()
    arena, offs, lens = T.pack(docs)
    prog = ctx.compile_render(outputs, n_slots)
    slots = np.full((2, 16), 0xA5, dtype=np.uint8)
    rec, out = ctx.render_host_arena(prog, arena, offs, lens, vals, text, out_text=slots)
    T.check_expected(rec, out, expected)
    assert out[0].tobytes() == b"0123456789zabcde" and (out[1] == 0xA5).all()
    with pytest.raises(runtime.AuthjxError):  # out_stride no multiple of 16
        ctx.render_host_arena(prog, arena, offs, lens, vals, text, out_stride=24)
    with pytest.raises(runtime.AuthjxError):  # values_stride < n_slots
        ctx.render_host_arena(ctx.compile_render([[(R.R_STRING, 1)]], 2), arena, offs, lens, vals, text)
    with pytest.raises(runtime.AuthjxError):  # slot >= n_slots
        ctx.compile_render([[(R.R_STRING, 2)]], 2)
    with pytest.raises(runtime.AuthjxError):  # unknown op
        ctx.compile_render([[(5, 0)]], 2)
