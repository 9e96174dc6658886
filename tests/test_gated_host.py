"""The gated render on the CPU: the verdict fold (authorino_amd/csrc/ajx_verdict.h) against its
executable specification (pipeline.verdict_of) and the default AuthPipelineBatch path, the
two denyWith ops (STRINGIFY, STRING_UTF8) against response.stringify_json, and the gated
kernel's per-request body (ajx_render_gated.h) against UNGATED renders, all on the host build
tests/native/gated_host.cpp (tests/_rendergated.py has the programs, gates and batches;
tests/test_gpu_render_gated.py runs them through the kernel). test_mutants_are_caught shows
that the checks bite.

authjx_verdict_of itself (libauthjx.so needs a device to compile gates) is compared with
verdict_of in the GPU file; here its body, gates_verdict_of, runs through gt_verdict_of."""
import itertools
import json
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _rendergated as GT
import _rendertest as T
import _rendervalues as V
import render_gen as G
from authorino_amd import jsonexp as J
from authorino_amd import pipeline as P
from authorino_amd import response as R

OK, UNRENDERED, SKIPPED = GT.OK, GT.UNRENDERED, GT.SKIPPED
EINVAL = -1


# ---- the fold ----
def check_fold(L=None):
    """All 4^8 tri-state rows of FOLD_PLAN: the header's verdict, denied_by and the
    status of each output equal the specification's. Returns the verdicts' counts."""
    g = GT.HostGates(GT.FOLD_PLAN, L)
    assert g.rc == 0, g.error
    counts = [0, 0, 0, 0]
    for row in itertools.product(range(4), repeat=GT.N_TREES):
        row = np.array(row, dtype=np.uint8)
        want = P.verdict_of(row, GT.FOLD_PLAN)
        assert g.verdict_of(row) == want, (row, want)
        counts[want[0]] += 1
        for k in range(len(GT.FOLD_PLAN.outputs)):
            assert g.output_status(row, want[0], k) == P.output_status_of(row, GT.FOLD_PLAN, want[0], k), (row, k)
    return counts


def test_fold_exhaustive():
    counts = check_fold()
    assert sum(counts) == 4 ** 8 and all(c > 0 for c in counts)
    # what the specification must say of a few rows, so that it is not judged by itself alone
    t = lambda **kw: np.array([kw.get("t%d" % i, 1) for i in range(8)], dtype=np.uint8)  # noqa: E731
    assert P.verdict_of(t(), GT.FOLD_PLAN) == (P.V_GRANTED, -1)
    assert P.verdict_of(t(t0=0), GT.FOLD_PLAN) == (P.V_SKIPPED, -1)
    assert P.verdict_of(t(t0=2), GT.FOLD_PLAN) == (P.V_SKIPPED, -1)      # an error in `when`: not met
    assert P.verdict_of(t(t0=3, t1=0), GT.FOLD_PLAN) == (P.V_UNDECIDED, -1)
    assert P.verdict_of(t(t1=0, t4=0), GT.FOLD_PLAN) == (P.V_DENIED, 0)  # the first level decides
    assert P.verdict_of(t(t1=2), GT.FOLD_PLAN) == (P.V_DENIED, 0)        # an error in the rules denies
    assert P.verdict_of(t(t2=0), GT.FOLD_PLAN) == (P.V_GRANTED, -1)      # no rules: nothing to fail
    assert P.verdict_of(t(t3=0, t4=0), GT.FOLD_PLAN) == (P.V_GRANTED, -1)  # `when` not met: ignored
    assert P.verdict_of(t(t3=0, t4=3), GT.FOLD_PLAN) == (P.V_UNDECIDED, -1)  # ... but its rules are named
    assert P.verdict_of(t(t1=0, t4=3), GT.FOLD_PLAN) == (P.V_DENIED, 0)  # a level after the denial is not read
    assert P.verdict_of(t(t4=0, t6=0), GT.FOLD_PLAN) == (P.V_DENIED, 2)
    assert P.verdict_of(t(t6=0), GT.FOLD_PLAN) == (P.V_DENIED, 3)
    assert P.verdict_of(t(t7=3), GT.FOLD_PLAN) == (P.V_GRANTED, -1)      # a response `when` is no part of it
    assert P.output_status_of(t(t7=3), GT.FOLD_PLAN, P.V_GRANTED, 1) == UNRENDERED
    assert P.output_status_of(t(t7=0), GT.FOLD_PLAN, P.V_GRANTED, 1) == SKIPPED
    assert [P.output_status_of(t(), GT.FOLD_PLAN, P.V_UNDECIDED, k) for k in range(4)] == [OK] + [UNRENDERED] * 3
    assert [P.output_status_of(t(), GT.FOLD_PLAN, P.V_DENIED, k) for k in range(4)] == [OK, SKIPPED, SKIPPED, OK]
    assert [P.output_status_of(t(), GT.FOLD_PLAN, P.V_SKIPPED, k) for k in range(4)] == [OK] + [SKIPPED] * 3


def test_gates_compile_einval_table():
    """A tree index >= n_trees (or below -1), priorities that decrease, an ALWAYS (or DENIED)
    output with a when_tree, an unknown `on`; authjx_verdict_of's n_trees below the gates'."""
    ev, out = [(-1, 1, 0), (2, 3, 1)], [(P.GATE_GRANTED, 3)]
    ok = GT.HostGates(P.GatePlan(0, ev, out, 4))
    assert ok.rc == 0 and ok.error == ""
    bad = [P.GatePlan(4, ev, out, 4), P.GatePlan(-2, ev, out, 4), P.GatePlan(0, [(-1, 4, 0)], out, 4),
           P.GatePlan(0, [(4, 1, 0)], out, 4), P.GatePlan(0, ev, [(P.GATE_GRANTED, 4)], 4),
           P.GatePlan(0, [(-1, 1, 1), (2, 3, 0)], out, 4), P.GatePlan(0, ev, [(P.GATE_ALWAYS, 1)], 4),
           P.GatePlan(0, ev, [(P.GATE_DENIED, 1)], 4), P.GatePlan(0, ev, [(3, -1)], 4)]
    for plan in bad:
        g = GT.HostGates(plan)
        assert g.rc == EINVAL and g._h is None and g.error, plan
    row = np.ones(3, dtype=np.uint8)
    v = GT._Verdict()
    assert GT.lib().gt_verdict_of(ok._h, row.ctypes.data, 3, v) == EINVAL


# ---- the fold against the default path ----
def _fold_config():
    """An AuthConfig of FOLD_PLAN's shape: a top `when`, two priorities of two evaluators each
    (one without `when`, one without rules), a response under a `when`, and a denyWith with a
    static, a template and a pattern value."""
    pat = lambda s, op, v: J.All(J.Pattern(s, op, v))  # noqa: E731
    JV = R.JSONValue
    authz = [
        P.AuthorizationConfig("a0", rules=pat("auth.identity.sub", J.NotEqualOperator, "mallory"), priority=0),
        P.AuthorizationConfig("a1", conditions=pat("context.request.http.method", J.EqualOperator, "GET"), priority=0),
        P.AuthorizationConfig("b0", conditions=pat("context.request.http.path", J.RegexOperator, "^/adm"),
                              rules=pat("auth.identity.groups", J.IncludesOperator, "admin"), priority=5),
        # (undecided requests: the oracle leaves @case over non-ASCII text undecided, the device
        # a comparison with a hex number literal)
        P.AuthorizationConfig("b1", conditions=pat("auth.identity.sub.@case:upper", J.NotEqualOperator, "BOB"),
                              rules=J.All(J.Pattern("auth.identity.quota", J.NotEqualOperator, "0"),
                                          J.Pattern("auth.identity.n", J.NotEqualOperator, "16")), priority=5),
    ]
    response = [
        R.ResponseConfig(name="user", wrapper=R.HTTP_HEADER_WRAPPER, wrapper_key="x-user",
                         plain=JV(pattern="auth.identity.sub"),
                         conditions=pat("auth.identity.groups", J.ExcludesOperator, "anon")),
        R.ResponseConfig(name="ctx", wrapper=R.HTTP_HEADER_WRAPPER, wrapper_key="x-ctx",
                         json_properties=[("quota", JV(pattern="auth.identity.quota")),
                                          ("who", JV(pattern="{auth.identity.sub}@{context.request.http.method}"))]),
    ]
    deny = P.DenyWithValues(code=403, message=JV(static="denied by policy"),
                            body=JV(pattern="no {context.request.http.method} on {context.request.http.path}"),
                            headers=[("x-quota", JV(pattern="auth.identity.quota")),
                                     ("x-groups", JV(pattern="auth.identity.groups"))])
    return P.AuthConfig(conditions=pat("context.request.http.path", J.NotEqualOperator, "/healthz"),
                        authorization=authz, response=response, unauthorized=deny)


def fold_docs(n=257):
    """Documents that reach every verdict (test_fold_against_the_default_path asserts it)."""
    docs = []
    for i in range(n):
        ident = {"sub": ["alice", "bob", "mallory", "café <o>"][i % 4],
                 "groups": [["users"], ["admin", "users"], ["anon"], []][(i // 4) % 4],
                 "quota": [0, 12345678901234567890123, 1.5, None, {"b": 1, "a": [1.0, "<"]}][i % 5]}
        if i % 7 == 3:
            ident["n"] = "?"
        d = {"context": {"request": {"http": {"method": ["GET", "POST"][(i // 2) % 2],
                                              "path": ["/adm/x", "/api", "/healthz", "/adm"][(i // 3) % 4]}}},
             "auth": {"identity": ident}}
        raw = json.dumps(d, separators=(",", ":"), ensure_ascii=False).encode()
        docs.append(raw.replace(b'"n":"?"', b'"n":0x1F'))
    return docs


def _fields(r):
    return (r.code, r.message, r.skipped, r.denied_by, r.undecided, r.authorization, r.status, r.body,
            r.deny_headers, r.headers, r.metadata)


def test_fold_against_the_default_path():
    """Over real documents the default AuthPipelineBatch.evaluate path's code, denied_by and
    undecided agree with the fold of the forest's tri-states, and AuthPipelineBatch(gated=True)
    over the host build gives the default path's results field by field."""
    cfg = _fold_config()
    docs = fold_docs()
    ctx = GT.GatedOracleCtx()
    base = P.AuthPipelineBatch(cfg, ctx=ctx)
    want = base.evaluate(docs)
    gated = P.AuthPipelineBatch(cfg, ctx=ctx, gated=True)
    assert gated._gated is not None and base._gated is None
    plan = gated._gated.plan
    assert plan.top == 0 and [p for _, _, p in plan.evaluators] == [0, 0, 1, 1]
    assert [(w < 0, r < 0) for w, r, _ in plan.evaluators] == [(True, False), (False, True), (False, False), (False, False)]
    arena, offs, lens = T.pack(docs)
    tri, _, _ = ctx.eval_host_arena([base._forest], arena, offs, lens, with_bitmap=False)
    seen = set()
    names = [c.name for level in base.levels for c in level]
    for j, r in enumerate(want):
        v, by = P.verdict_of(tri[j], plan)
        seen.add(v)
        assert r.undecided == (v == P.V_UNDECIDED) and r.skipped == (v == P.V_SKIPPED), (j, docs[j])
        assert (r.code == P.CODE_PERMISSION_DENIED) == (v == P.V_DENIED), (j, docs[j])
        assert r.denied_by == (names[by] if v == P.V_DENIED else None), (j, docs[j])
        assert r.code == {P.V_UNDECIDED: P.CODE_UNKNOWN, P.V_DENIED: P.CODE_PERMISSION_DENIED}.get(v, P.CODE_OK)
    assert seen == {P.V_SKIPPED, P.V_GRANTED, P.V_DENIED, P.V_UNDECIDED}
    launches = ctx.launches
    got = gated.evaluate(docs)
    assert ctx.launches == launches + 1  # one forest evaluation
    for j, (a, b) in enumerate(zip(got, want)):
        assert _fields(a) == _fields(b), (j, docs[j], _fields(a), _fields(b))
    denied = [r for r in want if r.code == P.CODE_PERMISSION_DENIED]
    assert any(r.deny_headers[0] == {"x-quota": "12345678901234568000000"} for r in denied)
    assert any(r.deny_headers[0] == {"x-quota": '{"a":[1,"\\u003c"],"b":1}'} for r in denied)
    assert any(r.deny_headers[0] == {"x-quota": ""} for r in denied) and denied[0].status == 403
    assert {r.denied_by for r in denied} == {"a0", "b0", "b1"}
    assert any(r.body == "no POST on /adm" for r in denied) and all(r.message == "denied by policy" for r in denied)
    assert any("x-user" in r.headers and "x-ctx" in r.headers for r in want)
    assert any("x-ctx" in r.headers and "x-user" not in r.headers for r in want)
    # a producer regenerates documents between levels: evaluate() takes the default path
    producer = lambda i, objs: docs[i]  # noqa: E731
    with_p = gated.evaluate(docs, producer=producer)
    assert ctx.launches > launches + 2  # (level by level, not the one gated evaluation)
    assert [_fields(r) for r in with_p] == [_fields(r) for r in base.evaluate(docs, producer=producer)]
    # a cache on an evaluator, or a context without the entry points: the default path
    cached = _fold_config()
    from authorino_amd.cache import EvaluatorCache

    cached.authorization[0].cache = EvaluatorCache(R.JSONValue(pattern="auth.identity.sub"), ttl=60)
    assert P.AuthPipelineBatch(cached, ctx=ctx, gated=True)._gated is None
    assert P.AuthPipelineBatch(cfg, ctx=T.OracleCtx(), gated=True)._gated is None


# ---- STRINGIFY / STRING_UTF8 ----
DENY_OPS = (R.R_STRINGIFY, R.R_STRING_UTF8)
DENY_OUTPUTS = [[(R.R_LIT, b"v=")] * (op == R.R_STRING_UTF8) + [(op, s)] for s in range(G.N_SLOTS) for op in DENY_OPS]


def deny_mirror(outputs, doc, vals_r, text_r=None):
    """The expected bytes of STRINGIFY (response.stringify_json of result_value) and
    STRING_UTF8 (result_string) outputs, None where the value's bytes are not UTF-8."""
    out = []
    for ops in outputs:
        parts = []
        for op, arg in ops:
            if op == R.R_LIT:
                parts.append(bytes(arg).decode())
                continue
            st, ln, t = (int(x) for x in vals_r[arg])
            src = text_r.tobytes() if (t >> 8) & R.VAL_TEXT else doc
            count = (t >> 8) == R.VAL_COUNT
            if (t & 0xFF) in (R.STRING, R.JSON) and not V._is_utf8(src[st:st + ln]):
                parts = None
                break
            if op == R.R_STRINGIFY:
                parts.append(R.stringify_json(float(st) if count else R.result_value(src, st, ln, t & 0xFF)))
            else:
                parts.append(str(st) if count else R.result_string(src, st, ln, t & 0xFF))
        out.append(None if parts is None else "".join(parts).encode("utf-8"))
    return out


def check_deny_corpus(render, seeds=V.SEEDS):
    """The generated corpus under both ops at an ample stride: byte equality with the
    mirror. A value declines only when it nests deeper than the walk's 8 levels (STRINGIFY
    of a container; STRING_UTF8 copies it as it stands). Returns (outputs, declined)."""
    total = declined = 0
    for seed in seeds:
        c = V.corpus(seed)
        rec, out = render(DENY_OUTPUTS, G.N_SLOTS, c.docs, c.vals, c.text, 16384)
        for r, doc in enumerate(c.docs):
            want = deny_mirror(DENY_OUTPUTS, doc, c.vals[r])
            pos = 0
            for k, w in enumerate(want):
                st, got = T.rendered(rec, out, r, k)
                op, slot = DENY_OUTPUTS[k][-1]
                s0, ln, t = (int(x) for x in c.vals[r, slot])
                total += 1
                assert w is not None  # (the generator writes UTF-8 only)
                if st == UNRENDERED:
                    assert op == R.R_STRINGIFY and (t & 0xFF) == R.JSON and G.nesting(doc[s0:s0 + ln]) > G.MAX_DEPTH, \
                        (seed, r, k, doc[s0:s0 + ln])
                    assert got == b""
                    declined += 1
                    continue
                assert (st, got) == (OK, w), (seed, r, k, DENY_OUTPUTS[k], got, w, doc[s0:s0 + ln])
                assert int(rec[r, k, 0]) == pos
                pos += len(got)
        assert (out[len(c.docs)] == V.GUARD).all()
    return total, declined


def test_stringify_on_generated_values():
    total, declined = check_deny_corpus(V.host_render(GT.lib()))
    print("denyWith ops: %d outputs, %d declined" % (total, declined))
    assert total == len(V.SEEDS) * V.DOCS_PER_SEED * len(DENY_OUTPUTS) and declined == 0
    # counts and the UTF-8 table (STRING_UTF8 and STRINGIFY decline exactly what STRING_ESC declines)
    c = V.counts_case()
    outputs = [[(op, s)] for s in range(len(V.COUNTS)) for op in DENY_OPS]
    rec, out = V.host_render(GT.lib())(outputs, c.n_slots, c.docs, c.vals, c.text, 512)
    assert [T.rendered(rec, out, 0, k) for k in range(len(outputs))] == [(OK, str(x).encode()) for x in V.COUNTS for _ in DENY_OPS]
    u, valid = V.utf8_table()
    rec, out = V.host_render(GT.lib())([[(op, 0)] for op in DENY_OPS], 1, u.docs, u.vals, u.text, 64)
    for r, doc in enumerate(u.docs):
        s0, ln, t = (int(x) for x in u.vals[r, 0])
        for k, op in enumerate(DENY_OPS):
            st, got = T.rendered(rec, out, r, k)
            if valid[r]:
                src = doc[s0:s0 + ln]
                w = (R.stringify_json(R.result_value(doc, s0, ln, t & 0xFF)) if op == R.R_STRINGIFY
                     else R.result_string(doc, s0, ln, t & 0xFF))
                assert (st, got) == (OK, w.encode("utf-8")), (doc, op, got, src)
            else:
                assert (st, got) == (UNRENDERED, b""), (doc, op, got)


KNOWN = [(b"1e21", "1000000000000000000000"), (b"12345678901234567890123", "12345678901234568000000"), (b"-0", "-0"),
         (b"1.0", "1"), (b"1e-7", "0.0000001"), (b"1e400", ""), (b"null", ""), (b"true", "true"),
         (b'"a\\u003cb"', "a<b"), (b'{"b":1,"a":[1.0,"<"]}', '{"a":[1,"\\u003c"],"b":1}')]


def check_known_answers(render):
    docs = [b'{"v":' + raw + b"}" for raw, _ in KNOWN] + [b'{"v":"a\xffb"}']
    vals, text = T.oracle_values(docs, ["v"], text_stride=16)
    rec, out = render([[(R.R_STRINGIFY, 0)], [(R.R_LIT, b"x"), (R.R_STRING_UTF8, 0)]], 1, docs, vals, text, 64)
    for r, (raw, want) in enumerate(KNOWN):
        assert T.rendered(rec, out, r, 0) == (OK, want.encode()), (raw, T.rendered(rec, out, r, 0))
        assert R.stringify_json(R.result_value(docs[r], *(int(x) for x in vals[r, 0][:2]), int(vals[r, 0][2]) & 0xFF)) == want
    assert T.rendered(rec, out, 5, 1) == (OK, b"x+Inf") and T.rendered(rec, out, 8, 1) == (OK, b"xa<b")
    lone = len(KNOWN)
    assert T.rendered(rec, out, lone, 0) == (UNRENDERED, b"") and T.rendered(rec, out, lone, 1) == (UNRENDERED, b"")
    assert int(rec[lone, 1, 0]) == 0  # (the literal before the declined value went back too)
    return len(docs)


def test_stringify_known_answers():
    assert check_known_answers(V.host_render(GT.lib())) == 11
    # depth > 8 and a value of type 255 decline as they do for MARSHAL
    outputs, n_slots, docs, vals, text, _ = T.decline_case(8)
    prog = T.HostProgram([[(R.R_STRINGIFY, 2)], [(R.R_STRINGIFY, 3)], [(R.R_STRINGIFY, 5)], [(R.R_STRING_UTF8, 5)],
                          [(R.R_STRINGIFY, 4)], [(R.R_STRINGIFY, 1)]], n_slots, GT.lib())
    rec, out = T.host_render(prog, docs, vals, text, 4096)
    got = [T.rendered(rec, out, 0, k) for k in range(6)]
    assert got[0][0] == OK and got[0][1] == R.go_json_marshal(json.loads(T.nested(8), parse_int=float)).encode()
    assert got[1:5] == [(UNRENDERED, b"")] * 4 and got[5] == (OK, b"1685557675")
    # the op numbers: 6 and 7 are accepted, 5 (not assigned) and 8 stay unknown ops
    assert (R.R_STRINGIFY, R.R_STRING_UTF8) == (6, 7)
    assert T.HostProgram([[(5, 0)]], 1, GT.lib()).rc == EINVAL and T.HostProgram([[(8, 0)]], 1, GT.lib()).rc == EINVAL


# ---- the gated body against the ungated one ----
SHAPES = ("granted", "denied", "alternating", "random")


def check_gated_body(L=None, n=130, shapes=SHAPES):
    """At an ample stride each rendered output's status and bytes equal the FULL ungated
    render's for that output, starts are the running sum of the rendered lengths, an output
    is UNRENDERED exactly where the ungated render declined it or the gate says so, and
    SKIPPED exactly where the gate says so; verdicts equal verdict_of; requests without a
    program, the records past n_outputs and the row after the batch keep their guards. At
    stride 16 the records and whole slots equal the ungated render of the sub-program that
    holds only the applicable outputs. Returns the statuses' counts at the ample stride."""
    hb = GT.HostBatch(L)
    por, docs, values, text = GT.batch(n)
    progs = GT.programs()
    counts = {OK: 0, UNRENDERED: 0, SKIPPED: 0}
    for shape in shapes:
        tri = GT.tri_rows(por, shape)
        tor = None
        if shape == "random":  # (through the row indirection: request r reads row n - 1 - r)
            tor = np.arange(n - 1, -1, -1, dtype=np.uint32)
        ample = 8192
        rc, rec, out, ver = hb.gated(por, docs, values, text, ample, tri, tri_of_req=tor)
        assert rc == 0
        assert np.array_equal(ver[:n], GT.verdicts_of(por, tri, tor)), shape
        assert (out[n] == GT.GUARD).all() and (rec[n] == GT.GUARD32).all() and (ver[n].view(np.uint32) == GT.GUARD32).all()
        for i, (outputs, n_slots, _, plan, _) in enumerate(progs):
            idx = np.flatnonzero(por == i)
            full_rec, full_out = hb.one(outputs, n_slots, [docs[j] for j in idx], values[idx], text[idx],
                                        np.full((len(idx), ample), GT.GUARD, dtype=np.uint8))
            for m, j in enumerate(idx):
                sts = GT.statuses_of(por, tri, j, tor)
                pos = 0
                for k, s in enumerate(sts):
                    st, got = T.rendered(rec, out, j, k)
                    fst, fgot = T.rendered(full_rec, full_out, m, k)
                    want_st = s if s != OK else fst
                    assert st == want_st, (shape, j, k, st, want_st)
                    assert got == (fgot if s == OK else b""), (shape, j, k)
                    assert int(rec[j, k, 0]) == pos, (shape, j, k)
                    pos += len(got)
                    counts[st] += 1
                assert (rec[j, len(outputs):] == GT.GUARD32).all()
        idle = por == GT.NONE
        assert idle.any() and (out[:n][idle] == GT.GUARD).all() and (rec[:n][idle] == GT.GUARD32).all()
        assert (ver[:n][idle].view(np.uint32) == GT.GUARD32).all()
        for stride in (16, ample):
            want_rec, want_out = GT.expected(por, docs, values, text, stride, tri, hb.one, tri_of_req=tor)
            rc, rec, out, _ = hb.gated(por, docs, values, text, stride, tri, tri_of_req=tor)
            assert rc == 0 and np.array_equal(rec[:n], want_rec), (shape, stride)
            assert np.array_equal(out[:n], want_out) and (out[n] == GT.GUARD).all(), (shape, stride)
    return counts


def check_one_byte_short(L=None, n=65):
    """Each request alone at a stride one byte short of its applicable outputs' total: a
    first ALWAYS output of '#' pads the total to 1 (mod 16). Records and the whole slot equal
    the ungated render of the applicable sub-program at that stride; at least one output
    that applies no longer fits. Returns the requests run."""
    L = GT.lib() if L is None else L
    hb = GT.HostBatch(L)
    por, docs, values, text = GT.batch(n)
    tri = GT.tri_rows(por, "random", seed=43)
    ran = 0
    for r in range(n):
        if por[r] == GT.NONE:
            continue
        outputs, n_slots, _, plan, _ = GT.programs()[por[r]]
        sts = GT.statuses_of(por, tri, r)
        sub = [o for o, s in zip(outputs, sts) if s == OK]
        rec0, _ = hb.one(sub, n_slots, [docs[r]], values[r:r + 1], text[r:r + 1], np.full((1, 8192), GT.GUARD, np.uint8))
        total = int(rec0[0, :, 1].sum()) if sub else 0
        if total == 0:
            continue
        pad = (1 - total) % 16 or 16
        stride = total + pad - 1
        assert stride % 16 == 0 and stride >= 16
        padded = [[(R.R_LIT, b"#" * pad)]] + outputs
        prog = T.HostProgram(padded, n_slots, L)
        gplan = None if plan is None else P.GatePlan(plan.top, plan.evaluators, [(P.GATE_ALWAYS, -1)] + plan.outputs,
                                                     plan.n_trees)
        gates = GT.HostGates(gplan, L) if gplan is not None else None
        want_rec, want_out = hb.one([padded[0]] + sub, n_slots, [docs[r]], values[r:r + 1], text[r:r + 1],
                                    np.full((1, stride), GT.GUARD, np.uint8))
        assert (want_rec[0, :, 2] == UNRENDERED).any()
        rc, rec, out, _ = hb.gated(None, [docs[r]], values[r:r + 1], text[r:r + 1], stride, tri[r:r + 1],
                                   records_stride=len(padded), progs=[prog], gates=[gates])
        assert rc == 0 and np.array_equal(out[0], want_out[0]) and (out[1] == GT.GUARD).all(), r
        q = 0
        pos = 0
        for k, s in enumerate((OK,) + sts):
            if s == OK:
                assert tuple(rec[0, k]) == tuple(want_rec[0, q]), (r, k)
                pos = int(rec[0, k, 0]) + int(rec[0, k, 1])
                q += 1
            else:
                assert tuple(rec[0, k]) == (pos, 0, s), (r, k)
        ran += 1
    return ran


def test_gated_body_equals_the_ungated_one():
    counts = check_gated_body()
    print("gated body: %s" % counts)
    assert all(c > 100 for c in counts.values())
    assert check_one_byte_short() > 30


def test_gated_einval_table():
    """gtm_render's argument checks are those of authjx_render_batch_gated_device; a refused
    call writes nothing."""
    hb = GT.HostBatch()
    n = 20
    por, docs, values, text = GT.batch(n)
    tri = GT.tri_rows(por, "granted")
    plans = GT.plans()

    def refused(**kw):
        a = dict(por=por, docs=docs, values=values, text=text, out_stride=256, tri=tri)
        a.update(kw)
        rc, rec, out, ver = hb.gated(**a)
        assert rc == EINVAL, kw
        assert (rec == GT.GUARD32).all() and (out == GT.GUARD).all() and (ver.view(np.uint32) == GT.GUARD32).all()

    assert hb.gated(por, docs, values, text, 256, tri)[0] == 0
    refused(por=None)                                  # four programs, no indices
    refused(progs=[], gates=[])                        # no programs
    refused(out_stride=24)
    refused(records_stride=len(GT.programs()[2][0]) - 1)
    refused(values=values[:, :7].copy())               # below the 8 slots of program 0
    refused(progs=[hb.progs[0], None] + hb.progs[2:])  # a NULL program
    refused(gates=[hb.gates[1]] + hb.gates[1:])        # gates of another program's n_outputs
    refused(tri=tri[:, :7].copy())                     # n_trees 8 above tri_stride 7
    refused(tri=None)                                  # gates without tri-states
    assert plans[3] is None
    rc, rec, out, ver = hb.gated(None, docs, values, text, 256, None, progs=[hb.progs[3]], gates=[None])
    assert rc == 0 and (rec[:n, :4, 2] <= UNRENDERED).all()  # NULL gates need no tri-states: everything renders
    assert (ver.view(np.uint32) == GT.GUARD32).all()          # ... and write no verdict


# ---- the checks bite ----
CHECKS = {
    "fold": check_fold,
    "known": lambda L: check_known_answers(V.host_render(L)),
    "corpus": lambda L: check_deny_corpus(V.host_render(L), V.SEEDS[:1]),
    "body": lambda L: check_gated_body(L, n=65, shapes=("alternating", "random")),
    "short": lambda L: check_one_byte_short(L, n=30),
}
_VH = "authorino_amd/csrc/ajx_verdict.h"
_RH = "authorino_amd/csrc/ajx_render.h"
# (name, file, exact old text, new text, the checks that must fail)
MUTANTS = [
    ("a skipped output renders", _RH, "const uint32_t q0 = gated == kRenderOk ? begin[k] : 0u, q1 = gated == kRenderOk ? begin[k + 1] : 0u;",
     "const uint32_t q0 = begin[k], q1 = begin[k + 1];", ("body", "short")),
    ("GRANTED and DENIED swapped", _VH, ["return AUTHJX_V_GRANTED;\n}", "            return AUTHJX_V_DENIED;"],
     ["return AUTHJX_V_DENIED;\n}", "            return AUTHJX_V_GRANTED;"], ("fold", "body", "short")),
    ("a level after the denial is read", _VH, "        if (undecided) return AUTHJX_V_UNDECIDED;\n        if (deny >= 0) {",
     "        if (deny >= 0 && !undecided) {", ("fold",)),
    ("rules of an unmet `when` not named", _VH, "undecided = undecided || w == AUTHJX_UNDECIDED || r == AUTHJX_UNDECIDED;",
     "undecided = undecided || w == AUTHJX_UNDECIDED || (w == AUTHJX_T && r == AUTHJX_UNDECIDED);", ("fold",)),
    ("integers keep their spelling", _RH, "if (op == R_STRINGIFY && v.type == T_NUMBER && v.esc != kValCount) {",
     "if (op == R_STRINGIFY && v.type == T_NUMBER && v.esc != kValCount && false) {", ("known", "corpus")),
    ("null written", _RH, "if (op != R_STRINGIFY) w.put_str(js", "w.put_str(js", ("known", "corpus")),
    ("UTF-8 not checked", _RH, "        if (!need) return false;\n        for (int k = 1; k < need; k++) {\n            const int x = s->next();\n            if (x < (int)lo || x > (int)hi) return false;\n            w.put",
     "        if (!need) continue;\n        for (int k = 1; k < need; k++) {\n            const int x = s->next();\n            if (x < 0) return true;\n            w.put", ("known",)),
]


def _mk(var: str) -> str:
    text = open(os.path.join(T.NATIVE, "gated.mk")).read()
    return re.search(r"^%s \??= *(.*)$" % var, text, re.M).group(1)


def _build_copy(root, edit=None):
    """The headers and sources gated.mk lists under `root` in the tree's layout, `edit` =
    (file, old, new) applied, compiled with gated.mk's CXXFLAGS: the library's path."""
    repo = os.path.dirname(T._HERE)
    native = os.path.join(root, "tests", "native")
    files = [os.path.normpath(os.path.join("tests/native", h.replace("$(CSRC)", _mk("CSRC")))) for h in _mk("HDRS").split()]
    for rel in files + ["tests/native/" + s for s in _mk("SRCS").split()]:
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        shutil.copyfile(os.path.join(repo, rel), os.path.join(root, rel))
    if edit:
        rel, olds, news = edit
        text = open(os.path.join(root, rel)).read()
        for old, new in zip([olds] if isinstance(olds, str) else olds, [news] if isinstance(news, str) else news):
            assert text.count(old) == 1, (rel, old, text.count(old))
            text = text.replace(old, new)
        with open(os.path.join(root, rel), "w") as f:
            f.write(text)
    so = os.path.join(native, "libajx_gatedtest.so")
    cmd = [os.environ.get("CXX", "g++")] + _mk("CXXFLAGS").split() + ["-std=c++17", "-shared", "-o", so, "gated_host.cpp"]
    p = subprocess.run(cmd, cwd=native, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return so


def test_mutants_are_caught(tmp_path):
    """Each mutant of ajx_verdict.h / ajx_render.h (a skipped output that renders, GRANTED and
    DENIED swapped, and the rest of MUTANTS), built as gated.mk builds the library, fails every
    check named for it; the unmutated copy passes every check. The mutants are text edits of a
    copy of the sources (as tests/test_render_values_host.py makes them), not compile-time
    switches in the product headers, and each is held to the checks that run the code it
    changes: a fold mutant cannot break the number formatter, nor a formatter mutant the fold."""
    with ThreadPoolExecutor(4) as pool:
        jobs = [pool.submit(_build_copy, str(tmp_path / "plain"))]
        jobs += [pool.submit(_build_copy, str(tmp_path / ("m%d" % i)), (rel, old, new))
                 for i, (_, rel, old, new, _) in enumerate(MUTANTS)]
        libs = [j.result() for j in jobs]
    plain = GT.load(libs[0])
    for check in CHECKS.values():
        check(plain)
    for (name, _, _, _, checks), so in zip(MUTANTS, libs[1:]):
        L = GT.load(so)
        for check in checks:
            try:
                CHECKS[check](L)
            except AssertionError:
                continue
            pytest.fail("mutant survived its check (%s): %s" % (check, name))


def test_sanitizer_program(tmp_path):
    """tests/native/san_gated (ASan + UBSan, its own main) over the gated batches of
    check_gated_body at stride 16 and an ample one: exit 0."""
    hb = GT.HostBatch()
    n = 130
    por, docs, values, text = GT.batch(n)
    cases = []
    for shape in SHAPES:
        tri = GT.tri_rows(por, shape)
        for stride in (16, 4096):
            want_rec, want_out = GT.expected(por, docs, values, text, stride, tri, hb.one)
            cases.append((por, docs, values, text, stride, tri, want_rec, want_out, GT.verdicts_of(por, tri)))
    path = tmp_path / "cases.bin"
    GT.write_cases(str(path), cases)
    p = subprocess.run([GT.make("san_gated"), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "%d cases" % len(cases) in p.stdout
