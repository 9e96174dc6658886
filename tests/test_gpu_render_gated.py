"""GPU tests of the gated render (authjx_render_batch_gated_device / authjx_render_batch_gated,
authorino_amd/csrc/ajx_render.hip ajx_render_values_gated): the verdict folded per lane and
the outputs chosen by it, against the host build of the same per-request body
(tests/native/gated_host.cpp, which tests/test_gated_host.py pins to ungated renders and to
the Python mirror), pipeline.verdict_of, and AuthPipelineBatch's default path."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ("granted", "denied", "alternating", "random")


@pytest.fixture(scope="module")
def setup():
    """The context, the four programs of tests/_rendergated.py and their gates (one entry
    NULL) compiled for the device, and the host build of the same."""
    import _rendergated as GT
    from authorino_amd import runtime

    ctx = runtime.Context(0)
    dev = [ctx.compile_render(p[0], p[1]) for p in GT.programs()]
    gates = [ctx.compile_gates(pl.top, pl.evaluators, pl.outputs, pl.n_trees) if pl is not None else None
             for pl in GT.plans()]
    return ctx, dev, gates, GT.HostBatch()


def _device(ctx, dev, gates, por, docs, values, text, out_stride, tri, tri_of_req=None, records_stride=None,
            want_verdicts=True):
    """authjx_render_batch_gated_device into guard-filled device buffers with one more row
    than requests: (records, out_text, verdicts) as numpy, status / verdict masked where written."""
    import torch

    import _rendergated as GT
    import _rendermulti as M
    import _rendertest as T

    d = torch.device("cuda", 0)
    arena, offs, lens = T.pack(docs)
    n = len(docs)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
    A, Of, Ln = up(arena), up(offs.view(np.int64)), up(lens.view(np.int32))
    Pr = up(por.view(np.int32)) if por is not None else None
    Vv, X, Tr = up(values.view(np.int32)), up(text), up(tri)
    To = up(np.ascontiguousarray(tri_of_req, dtype=np.uint32).view(np.int32)) if tri_of_req is not None else None
    rs = max(len(p[0]) for p in GT.programs()) if records_stride is None else records_stride
    guard = M.GUARD32 - (1 << 32)
    out = torch.full((n + 1, out_stride), M.GUARD, dtype=torch.uint8, device=d)
    rec = torch.full((n + 1, max(rs, 1), 3), guard, dtype=torch.int32, device=d)
    ver = torch.full((n + 1, 2), guard, dtype=torch.int32, device=d)
    torch.cuda.synchronize()
    ctx.render_gated_device(dev, gates, Pr, A, Of, Ln, Vv, out, rec, Tr, text=X, tri_of_req=To,
                            verdicts=ver if want_verdicts else None)
    torch.cuda.synchronize()
    r = rec.cpu().numpy().view(np.uint32).copy()
    M.mask_status(r)
    v = ver.cpu().numpy().view(np.uint32).copy()
    GT.mask_verdicts(v)
    return r, out.cpu().numpy(), v.view(np.int32)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_gated_kernel_equals_the_host_build(setup, n):
    """n requests (one lane; a full wave; a wave plus one; the 256-lane workgroup boundary of
    the LDS level stack) strictly alternating over three gated programs, one with a NULL gates
    entry and no program, the tri-states all granted, all denied, alternating per lane
    (divergence inside a wave) and seeded random over all four values (through the row
    indirection), at out_stride 16 and 4096: records and whole output slots equal the host
    build's, verdicts equal verdict_of; requests without a program, records past a program's
    outputs, verdicts of ungated requests and the row after the batch keep their guards."""
    import _rendergated as GT

    ctx, dev, gates, hb = setup
    por, docs, values, text = GT.batch(n)
    seen = set()
    for shape in SHAPES:
        tri = GT.tri_rows(por, shape)
        tor = np.arange(n - 1, -1, -1, dtype=np.uint32) if shape == "random" else None
        want_ver = GT.verdicts_of(por, tri, tor)
        seen.update(int(v) for v in want_ver[:, 0])
        for out_stride in (16, 4096):
            rc, want_rec, want_out, host_ver = hb.gated(por, docs, values, text, out_stride, tri, tri_of_req=tor)
            assert rc == 0 and np.array_equal(host_ver[:n], want_ver)
            rec, out, ver = _device(ctx, dev, gates, por, docs, values, text, out_stride, tri, tri_of_req=tor)
            assert np.array_equal(ver, host_ver), (shape, out_stride)
            assert np.array_equal(rec, want_rec), (shape, out_stride)
            assert np.array_equal(out, want_out), (shape, out_stride)
            assert (out[n] == GT.GUARD).all() and (rec[n] == GT.GUARD32).all()
            idle = por == GT.NONE
            assert (out[:n][idle] == GT.GUARD).all() and (rec[:n][idle] == GT.GUARD32).all()
            ungated = idle | (por == 3)
            assert (ver[:n][ungated].view(np.uint32) == GT.GUARD32).all()
            if n >= 64 and out_stride == 4096:  # (not a comparison of empty things)
                sts = rec[:n][por == 1][:, :16, 2]
                assert (sts == GT.OK).any() and (sts == GT.SKIPPED).any()
                assert shape != "random" or (sts == GT.UNRENDERED).any()
    if n >= 64:
        assert seen >= {0, 1, 2, 3}  # every verdict occurred


def test_verdict_of_runs_the_fold_on_the_host(setup):
    """authjx_verdict_of over all 4^8 tri-state rows of FOLD_PLAN equals
    pipeline.verdict_of; a row shorter than the gates' n_trees is EINVAL."""
    import _rendergated as GT
    from authorino_amd import pipeline as P, runtime

    ctx = setup[0]
    plan = GT.FOLD_PLAN
    g = ctx.compile_gates(plan.top, plan.evaluators, plan.outputs, plan.n_trees)
    for row in itertools.product(range(4), repeat=GT.N_TREES):
        assert g.verdict_of(row) == P.verdict_of(row, plan), row
    with pytest.raises(runtime.AuthjxError, match="EINVAL"):
        g.verdict_of([1] * 7)
    for bad in (P.GatePlan(8, plan.evaluators, plan.outputs, 8), P.GatePlan(0, [(-1, 1, 1), (2, 3, 0)], [], 8),
                P.GatePlan(0, [], [(P.GATE_ALWAYS, 2)], 8), P.GatePlan(0, [], [(3, -1)], 8)):
        with pytest.raises(runtime.AuthjxError, match="EINVAL"):
            ctx.compile_gates(bad.top, bad.evaluators, bad.outputs, bad.n_trees)


def test_pipeline_gated_equals_the_default_path(setup):
    """An AuthConfig with a top `when`, two priorities, response `when`s and a denyWith with a
    static, a template and pattern values over 257 documents in which every verdict occurs
    (tests/test_gated_host.py asserts that with the oracle): AuthPipelineBatch(gated=True)
    equals the default path field by field, from one evaluation, one select and one render."""
    from authorino_amd import pipeline as P
    from test_gated_host import _fields, _fold_config, fold_docs

    ctx = setup[0]
    cfg, docs = _fold_config(), fold_docs(257)
    want = P.AuthPipelineBatch(cfg, ctx=ctx).evaluate(docs)
    gated = P.AuthPipelineBatch(cfg, ctx=ctx, gated=True)
    assert gated._gated is not None
    got = gated.evaluate(docs)
    for j, (a, b) in enumerate(zip(got, want)):
        assert _fields(a) == _fields(b), (j, docs[j], _fields(a), _fields(b))
    kinds = {(r.code, r.skipped, r.undecided) for r in want}
    assert kinds == {(P.CODE_OK, False, False), (P.CODE_OK, True, False), (P.CODE_PERMISSION_DENIED, False, False),
                     (P.CODE_UNKNOWN, False, True)}
    assert any(r.deny_headers and r.deny_headers[0] == {"x-quota": "12345678901234568000000"} for r in want)


def test_host_buffer_call_and_einval_table(setup):
    """authjx_render_batch_gated (host buffers) gives the device-buffer call's result.
    AUTHJX_EINVAL: the multi call's table (several programs without indices, no programs,
    out_stride no multiple of 16, values_stride or records_stride below a program's need, a
    NULL program, a NULL output buffer, an output buffer that is not 16-byte aligned) and a
    gates object whose n_outputs differs from its program's, whose n_trees exceeds tri_stride,
    or gates without tri-states; a refused call writes nothing."""
    import torch

    import _rendergated as GT
    import _rendermulti as M
    from authorino_amd import runtime

    ctx, dev, gates, hb = setup
    n = 40
    por, docs, values, text = GT.batch(n)
    tri = GT.tri_rows(por, "alternating")
    rc, want_rec, want_out, want_ver = hb.gated(por, docs, values, text, 256, tri)
    import _rendertest as T

    arena, offs, lens = T.pack(docs)
    rs = want_rec.shape[1]
    rec = np.full((n + 1, rs, 3), GT.GUARD32, dtype=np.uint32)
    out = np.full((n + 1, 256), GT.GUARD, dtype=np.uint8)
    ver = np.full((n + 1, 2), GT.GUARD32, dtype=np.uint32).view(np.int32)
    ctx.render_gated_host_arena(dev, gates, por, arena, offs, lens, values, tri, text=text, out_text=out,
                                records=rec, verdicts=ver)
    M.mask_status(rec)
    v = ver.view(np.uint32).copy()
    GT.mask_verdicts(v)
    assert np.array_equal(rec, want_rec) and np.array_equal(out, want_out) and np.array_equal(v.view(np.int32), want_ver)

    def refused(**kw):
        a = dict(por=por, docs=docs, values=values, text=text, out_stride=256, tri=tri)
        a.update(kw)
        devs, gts = a.pop("dev", dev), a.pop("gates", gates)
        with pytest.raises(runtime.AuthjxError, match="EINVAL"):
            _device(ctx, devs, gts, **a)

    refused(por=None)                                   # four programs, no indices
    refused(dev=[], gates=[])                           # no programs
    refused(out_stride=24)                              # no multiple of 16
    refused(records_stride=len(GT.programs()[2][0]) - 1)
    refused(values=values[:, :7].copy())                # below the 8 slots of program 0
    refused(dev=[dev[0], None] + dev[2:])               # a NULL program
    refused(gates=[gates[1]] + gates[1:])               # gates of another n_outputs
    refused(tri=tri[:, :7].copy())                      # n_trees 8 above tri_stride 7
    d = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
    A, Of, Ln, Pr = up(arena), up(offs.view(np.int64)), up(lens.view(np.int32)), up(por.view(np.int32))
    Vv, X, Tr = up(values.view(np.int32)), up(text), up(tri)
    slots = torch.full((n * 256 + 16,), M.GUARD, dtype=torch.uint8, device=d)
    recd = torch.full((n, rs, 3), -1, dtype=torch.int32, device=d)
    verd = torch.full((n, 2), -1, dtype=torch.int32, device=d)
    ok = slots[:n * 256].view(n, 256)
    with pytest.raises(runtime.AuthjxError, match="EINVAL"):  # gates without tri-states
        ctx.render_gated_device(dev, gates, Pr, A, Of, Ln, Vv, ok, recd, None, text=X, verdicts=verd)
    with pytest.raises(runtime.AuthjxError, match="EINVAL"):  # out_stride 0
        ctx.render_gated_device(dev, gates, Pr, A, Of, Ln, Vv, ok[:, :0], recd, Tr, text=X, verdicts=verd)
    with pytest.raises(runtime.AuthjxError, match="EINVAL"):  # not 16-byte aligned
        ctx.render_gated_device(dev, gates, Pr, A, Of, Ln, Vv, slots[8:8 + n * 256].view(n, 256), recd, Tr, text=X,
                                verdicts=verd)
    with pytest.raises(runtime.AuthjxError, match="EINVAL"):  # a NULL output buffer
        ctx.render_gated_device(dev, gates, Pr, A, Of, Ln, Vv, ok, None, Tr, text=X, verdicts=verd)
    torch.cuda.synchronize()
    assert bool((slots == M.GUARD).all()) and bool((recd == -1).all()) and bool((verd == -1).all())
    # a NULL gates entry for every program needs no tri-states: the multi call's result
    ctx.render_gated_device([dev[3]], [None], None, A, Of, Ln, Vv, ok, recd, None, text=X, verdicts=verd)
    torch.cuda.synchronize()
    assert bool((verd == -1).all()) and bool((recd[:, :4, 2] & 0xFF <= 1).all())


def test_batcher_gated_phases_from_64_producers(setup):
    """64 concurrent producers over two gated phases (different AuthConfigs and strides) and one
    ungated phase that shares the first one's rules, program and stride group, 257 documents
    in turn through one batcher: each answer — tri-states, verdict, every output's status and
    bytes — equals the batch calls' (authjx_eval_batch, authjx_select_text_batch, then
    authjx_render_batch_gated for the gated phases and authjx_render_batch for the ungated
    one). authjx_batcher_phase_gated on the ungated phase and authjx_phase_create_gated with
    another program's gates are EINVAL."""
    import threading

    import _rendertest as T
    from authorino_amd import pipeline as P, response as R, runtime
    from test_gated_host import _fold_config, fold_docs

    ctx = setup[0]
    docs = fold_docs(257)
    arena, offs, lens = T.pack(docs)
    cfg_a, cfg_b = _fold_config(), _fold_config()
    cfg_b.unauthorized = P.DenyWithValues(code=401, message=R.JSONValue(pattern="auth.identity.groups"),
                                          headers=[("x-sub", R.JSONValue(pattern="sub={auth.identity.sub}"))])
    cfg_b.response = cfg_b.response[:1]
    pa, pb = (P.AuthPipelineBatch(c, ctx=ctx, gated=True)._gated for c in (cfg_a, cfg_b))
    stride = {0: 2048, 1: 1024, 2: 2048}
    mk = lambda g, s, gates: runtime.Phase(ctx, g.b._forest, g.sel.ruleset, g.prog, text_stride=g.sel.TEXT_STRIDE,  # noqa: E731
                                           out_stride=s, gates=gates)
    phases = [mk(pa, 2048, pa.gates), mk(pb, 1024, pb.gates), mk(pa, 2048, None)]
    owner = [pa, pb, pa]
    want = []
    for k, g in enumerate(owner):  # the batch calls
        tri, err, _ = ctx.eval_host_arena([g.b._forest], arena, offs, lens, with_bitmap=False)
        tri = np.ascontiguousarray(tri.reshape(len(docs), -1), dtype=np.uint8)
        spans = g.sel.resolve(docs, arena, offs, lens)
        if k < 2:
            rec, text, ver = ctx.render_gated_host_arena([g.prog], [g.gates], None, arena, offs, lens, spans.spans, tri,
                                                         text=spans.text, out_stride=stride[k])
        else:
            rec, text = ctx.render_host_arena(g.prog, arena, offs, lens, spans.spans, spans.text, out_stride=stride[k])
            ver = None
        want.append((tri, err.reshape(len(docs), -1), rec, text, ver))
    batcher = runtime.Batcher(ctx, max_batch=64, window_us=300)
    got, errors = {}, []

    def producer(t):
        try:
            for i in range(t, len(docs), 64):
                k = i % 3
                got[i] = batcher.phase_gated(phases[k], docs[i]) if k < 2 else batcher.phase(phases[k], docs[i]) + (None,)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    try:
        ts = [threading.Thread(target=producer, args=(t,)) for t in range(64)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert batcher.stats()["max_batch_seen"] > 1
        with pytest.raises(runtime.AuthjxError, match="EINVAL"):
            batcher.phase_gated(phases[2], docs[0])
    finally:
        batcher.close()
    assert not errors, errors[:3]
    verdicts, statuses = set(), set()
    for i in range(len(docs)):
        k = i % 3
        tri, err, rec, text, ver = want[k]
        g_tri, g_err, vals, g_ver = got[i]
        assert g_tri == [int(x) for x in tri[i]] and g_err == [int(x) for x in err[i]], i
        for j in range(owner[k].prog.n_outputs):
            s, ln, st = (int(x) for x in rec[i, j])
            st &= 0xFF
            wbytes = text[i, s:s + ln].tobytes()
            if k < 2:
                assert vals[j] == (st, wbytes), (i, j, vals[j], st, wbytes)
                statuses.add(st)
            else:
                assert vals[j] == (wbytes if st == R.RENDER_OK else None), (i, j)
        if k < 2:
            assert g_ver == (int(ver[i, 0]) & 0xFF, int(ver[i, 1])), (i, g_ver, ver[i])
            assert g_ver == P.verdict_of(tri[i], owner[k].plan), i
            verdicts.add(g_ver[0])
    assert verdicts == {P.V_SKIPPED, P.V_GRANTED, P.V_DENIED, P.V_UNDECIDED}
    assert {R.RENDER_OK, R.RENDER_SKIPPED, R.RENDER_UNRENDERED} <= statuses
    with pytest.raises(runtime.AuthjxError, match="EINVAL"):  # pb's gates: another n_outputs
        runtime.Phase(ctx, pa.b._forest, pa.sel.ruleset, pa.prog, out_stride=2048, gates=pb.gates)
