"""GPU: a phase's response headers with each decision through the micro-batcher
(authjx_batcher_phase, ajx_batcher_api.cpp): phase requests of three AuthConfigs and plain
authjx_batcher_eval requests of a fourth ruleset from concurrent callers through one
batcher. Decisions and error indices against the oracle (oracle/), as
tests/test_gpu_batcher.py checks them; header bytes against the Python mirror
(authorino_amd/response.py over the oracle's gjson) and against the one-program
authjx_select_text_batch + authjx_render_batch calls that tests/test_gpu_render.py pins to
that mirror."""
import threading

import numpy as np
import pytest

import pyoracle as O

pytestmark = pytest.mark.gpu

GUARD = 0xA5


class _Config:
    """One AuthConfig of the test: its rules on the device, its phase, documents, and what
    every request must give: oracle decisions, mirror headers, one-program device headers."""

    def __init__(self, ctx, name, rules, exprs, cfgs, docs, text_stride=None, out_stride=None, phase=None):
        import _rendertest as T
        from authorino_amd import response as R
        from test_pipeline_host import OracleCtx

        self.name, self.rules, self.docs, self.cfgs = name, rules, docs, cfgs
        arena, offs, lens = T.pack(docs)
        outs = [O.eval_batch([O.Ruleset.from_expression(e)], arena, offs, lens, nthreads=4) for e in exprs]
        self.tri = np.stack([o[0] for o in outs], axis=1)
        # (forest numbering: tree k's pattern j is rules.offsets[k] + j)
        self.err = np.stack([np.where(o[1] >= 0, o[1] + rules.offsets[k], -1) for k, o in enumerate(outs)], axis=1)
        self.phase, self.keys, self.mirror, self.device = phase, [], None, None
        if cfgs is None:
            return
        self.sel = R.ResponseSelectors(cfgs, ctx)
        if phase is None:
            self.phase, self.keys = self.sel.phase(rules, text_stride=text_stride, out_stride=out_stride)
        so = R.ResponseSelectors(cfgs, OracleCtx())
        spans = so.resolve(docs, arena, offs, lens)
        self.mirror = [[c.wrap_object_as_header_value(so.call(c, d, spans[r])).encode("utf-8") for c in cfgs]
                       for r, d in enumerate(docs)]
        self.device = self.one_program(docs, self.phase.out_stride)

    def one_program(self, docs, out_stride):
        """authjx_select_text_batch + authjx_render_batch (ResponseSelectors.resolve / render)."""
        import _rendertest as T

        arena, offs, lens = T.pack(docs)
        vals, _ = self.sel.render(arena, offs, lens, self.sel.resolve(docs, arena, offs, lens), out_stride=out_stride)
        return vals

    def check(self, r, got):
        tri, err, vals = got
        assert list(tri) == [int(x) for x in self.tri[r]], (self.name, r, tri, self.tri[r])
        assert list(err) == [int(x) for x in self.err[r]], (self.name, r, err, self.err[r])
        if self.device is not None:
            assert vals == self.device[r], (self.name, r, vals, self.device[r])


@pytest.fixture(scope="module")
def world():
    from authorino_amd import jsonexp as J, response as R, runtime, workloads
    from test_denywith_cache_host import _req

    ctx = runtime.Context(0)
    w = workloads.make("c5", n=80)
    cfg = w.auth_config
    exprs = [cfg.conditions] + [e for c in cfg.authorization for e in (c.conditions, c.rules)]
    a = _Config(ctx, "c5", ctx.compile_forest(exprs), exprs, cfg.response, [w.doc(i) for i in range(w.n)],
                out_stride=1024)
    assert len(a.sel.paths) == 8 and a.keys == ["x-auth-user", "x-auth-exp", "x-auth-claims", "x-auth-ctx"]
    docs = [_req(sub=("alice", "s%d" % i, "bob")[i % 3], tenant="t%d" % (i % 7), roles=("r%d" % i, "x"))
            for i in range(80)]
    eb = J.All(J.Pattern("auth.identity.sub", J.EqualOperator, "alice"))
    mods = [R.ResponseConfig("b1", plain=R.JSONValue(pattern='{auth.identity.sub|@extract:{"sep":"i","pos":0}}-'
                                                             '{auth.identity.roles.#.x}'), wrapper_key="x-b1"),
            R.ResponseConfig("b2", plain=R.JSONValue(pattern="T={auth.identity.tenant.@case:upper} "
                                                             "R={auth.identity.roles|@case:upper}"),
                             wrapper_key="x-b2")]
    b = _Config(ctx, "modifiers", ctx.compile_expression(eb), [eb], mods, docs, text_stride=512, out_stride=256)
    ec = J.Any(J.Pattern("auth.identity.tenant", J.EqualOperator, "t3"),
               J.Pattern("auth.identity.sub", J.RegexOperator, "^s[0-9]+$"))
    rc = ctx.compile_expression(ec)
    selc = ctx.compile([("auth.identity.sub", 1, "")], [], -1)
    c = _Config(ctx, "no outputs", rc, [ec], None, docs,
                phase=runtime.Phase(ctx, rc, selc, ctx.compile_render([], 0), 0, 16))
    ed = J.All(J.Pattern("auth.identity.roles", J.IncludesOperator, "x"),
               J.Pattern("auth.identity.sub", J.NotEqualOperator, "bob"))
    d = _Config(ctx, "eval only", ctx.compile_expression(ed), [ed], None, docs)
    for k in (a, b):  # the one-program device result is the mirror's, nothing declined
        assert [[v for v in row] for row in k.device] == k.mirror
    assert b.mirror[0] == [b"al-[]", b'T=T0 R=["R0","X"]']
    yield ctx, a, b, c, d
    ctx.close()


def _call(batcher, cfg, r):
    if cfg.phase is None:
        return batcher.eval(cfg.rules, cfg.docs[r]) + (None,)
    return batcher.phase(cfg.phase, cfg.docs[r])


@pytest.mark.parametrize("zero_copy", [1, 0])
def test_mixed_batches_from_eight_producers(world, zero_copy):
    """8 producer threads x 40 requests, the four configs in turn, through one batcher of
    max_batch 64 with zero-copy on and off: every caller gets its own decision, error
    indices and header bytes; several batches formed and held more than one request."""
    from authorino_amd import runtime

    ctx, a, b, c, d = world
    kinds = (a, b, c, d)
    batcher = runtime.Batcher(ctx, max_batch=64, window_us=300, modes=(0, 0, zero_copy))
    got, errors = {}, []

    def producer(t):
        try:
            for i in range(t, 320, 8):
                got[i] = _call(batcher, kinds[i % 4], i // 4)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    try:
        ts = [threading.Thread(target=producer, args=(t,)) for t in range(8)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        st = batcher.stats()
    finally:
        batcher.close()
    assert not errors, errors[:3]
    rendered = unrendered = 0
    for i in range(320):
        kinds[i % 4].check(i // 4, got[i])
        vals = got[i][2] or []
        rendered += sum(v is not None for v in vals)
        unrendered += sum(v is None for v in vals)
    print({"zero_copy": zero_copy, "rendered by the device": rendered, "UNRENDERED": unrendered, **st})
    assert unrendered == 0 and rendered == 80 * 4 + 80 * 2
    assert st["requests"] == 320 and st["batches"] < 320 and st["max_batch_seen"] > 1


def test_one_request_alone(world):
    """A batch of one (the small-batch streaming path) for each config."""
    from authorino_amd import runtime

    ctx, a, b, c, d = world
    batcher = runtime.Batcher(ctx, max_batch=64, window_us=50)
    try:
        for cfg in (a, b, c, d, b, a):
            cfg.check(5, _call(batcher, cfg, 5))
        assert batcher.stats()["max_batch_seen"] == 1
        assert batcher.phase(c.phase, c.docs[0])[2] == []
    finally:
        batcher.close()


def test_decline_and_text_stride_zero_share_batches(world):
    """c5 with an out_stride of 32 (its claims header needs more: UNRENDERED, the headers
    that fit are right), the modifier config with text_stride 0 (its modifier values are
    UNSUPPORTED, so both headers are UNRENDERED; a third header without modifiers renders;
    the decision is unaffected), next to the same configs with room, in the same batches."""
    from authorino_amd import response as R, runtime

    ctx, a, b, c, d = world
    a32, _ = a.sel.phase(a.rules, out_stride=32)
    want32 = a.one_program(a.docs, 32)
    assert all(row[2] is None and row[0] is not None for row in want32)
    plain = b.cfgs + [R.ResponseConfig("b3", plain=R.JSONValue(pattern="auth.identity.sub"), wrapper_key="x-b3")]
    sel3 = R.ResponseSelectors(plain, ctx)
    b0, _ = sel3.phase(b.rules, text_stride=0, out_stride=256)
    batcher = runtime.Batcher(ctx, max_batch=64, window_us=300)
    got, errors = {}, []

    def producer(t):
        try:
            for i in range(t, 160, 8):
                r = i // 4
                if i % 4 == 0:
                    got[i] = batcher.phase(a32, a.docs[r])
                elif i % 4 == 1:
                    got[i] = batcher.phase(b0, b.docs[r])
                else:
                    got[i] = _call(batcher, (a, b)[i % 2], r)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    try:
        ts = [threading.Thread(target=producer, args=(t,)) for t in range(8)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert batcher.stats()["max_batch_seen"] > 1
    finally:
        batcher.close()
    assert not errors, errors[:3]
    for i in range(160):
        r = i // 4
        tri, err, vals = got[i]
        if i % 4 == 0:
            assert (list(tri), list(err)) == ([int(x) for x in a.tri[r]], [int(x) for x in a.err[r]])
            assert vals == want32[r] and vals[0] == a.mirror[r][0], (r, vals, want32[r])
        elif i % 4 == 1:
            assert (list(tri), list(err)) == ([int(x) for x in b.tri[r]], [int(x) for x in b.err[r]])
            sub = b.docs[r].split(b'"sub":"')[1].split(b'"')[0]
            assert vals == [None, None, sub], (r, vals)
        else:
            (a, b)[i % 2].check(r, got[i])


def test_expired_deadline_leaves_the_buffers(world):
    """A lone request whose deadline is shorter than the batcher's window: AUTHJX_ETIMEDOUT,
    the guard-filled out_text / out unchanged."""
    from authorino_amd import runtime

    ctx, a, b, c, d = world
    batcher = runtime.Batcher(ctx, max_batch=64, window_us=3000)
    try:
        text = np.full(a.phase.out_stride, GUARD, dtype=np.uint8)
        rec = np.full((4, 3), 0xA5A5A5A5, dtype=np.uint32)
        with pytest.raises(runtime.BatchTimeout):
            batcher.phase(a.phase, a.docs[0], timeout_s=100e-6, out_text=text, out=rec)
        assert (text == GUARD).all() and (rec == 0xA5A5A5A5).all()
        assert batcher.stats()["expired"] == 1
        # (and the same buffers are written by a call that has the time)
        a.check(0, batcher.phase(a.phase, a.docs[0], out_text=text, out=rec))
        end = int((rec[:, 0] + rec[:, 1]).max())
        assert 0 < end <= 1024 and (text[end:] == GUARD).all() and text[:end].tobytes() == b"".join(a.mirror[0])
    finally:
        batcher.close()


def test_phase_loadgen_hashes(world):
    """authjx_debug_phase_loadgen (what scripts/serve_phase.py drives): the FNV-1a of each
    request's status bytes and rendered bytes is the expected headers'."""
    from authorino_amd import runtime
    import _rendertest as T

    ctx, a, b, c, d = world
    docs = a.docs + b.docs
    arena, offs, lens = T.pack(docs)
    por = np.array([0] * len(a.docs) + [1] * len(b.docs), dtype=np.uint32)

    def fnv(vals):
        h = 0xcbf29ce484222325
        for v in vals:
            h = ((h ^ 0) * 0x100000001b3) & (2 ** 64 - 1)
            for x in v:
                h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
        return h

    batcher = runtime.Batcher(ctx, max_batch=64, window_us=200)
    try:
        lat, tri, hsh, wall = batcher.phase_loadgen([a.phase, b.phase], por, arena, offs, lens, threads=16)
    finally:
        batcher.close()
    want = [fnv(row) for row in a.mirror + b.mirror]
    assert [int(x) for x in hsh] == want
    assert [int(x) for x in tri] == [int(x) for x in np.concatenate([a.tri[:, 0], b.tri[:, 0]])]
    assert (lat > 0).all() and wall > 0


def test_phase_create_argument_table(world):
    from authorino_amd import runtime

    ctx, a, b, c, d = world
    rules, sel, prog = b.rules, b.sel.ruleset, b.phase.prog

    def rc(*args):
        try:
            runtime.Phase(*args)
        except runtime.AuthjxError as e:
            return str(e).split("failed: ")[1].split(" ")[0]
        return "OK"

    assert rc(ctx, rules, sel, prog, 512, 256) == "OK"
    assert rc(ctx, rules, sel, prog, 0, 16) == "OK" and rc(ctx, rules, sel, prog, 65536, 65536) == "OK"
    assert rc(None, rules, sel, prog, 512, 256) == "EINVAL"
    assert rc(ctx, None, sel, prog, 512, 256) == "EINVAL"
    assert rc(ctx, rules, None, prog, 512, 256) == "EINVAL"
    assert rc(ctx, rules, sel, None, 512, 256) == "EINVAL"
    assert rc(ctx, rules, a.rules, prog, 512, 256) == "EINVAL"        # selectors with more than one tree
    assert rc(ctx, rules, c.phase.selectors, prog, 512, 256) == "EINVAL"  # 1 pattern, the program has more slots
    assert rc(ctx, rules, sel, prog, 512, 0) == "EINVAL" and rc(ctx, rules, sel, prog, 512, 24) == "EINVAL"
    assert rc(ctx, rules, sel, prog, 512, 65552) == "ELIMIT" and rc(ctx, rules, sel, prog, 65537, 256) == "ELIMIT"
    L = runtime.load_library()
    assert L.authjx_phase_create(ctx._h, rules._h, sel._h, prog._h, 512, 256, None) == -1  # no place for the handle
    assert L.authjx_phase_outputs(None) == 0
    if L.authjx_device_count() > 1:  # the objects' devices differ
        other = runtime.Context(1)
        try:
            assert rc(other, rules, sel, prog, 512, 256) == "EINVAL"
        finally:
            other.close()
