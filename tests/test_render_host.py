"""Render programs (response header values rendered on the device, include/authjx.h
authjx_render_*) on the CPU: the host build of authorino_amd/csrc/ajx_render.h
(tests/native/render_host.cpp) against the Python mirror.

"Expected" is always the bytes authorino_amd/response.py's host functions give over the
oracle's gjson (tests/_rendertest.py mirror / oracle_values); those functions are pinned to
the reference's own vectors by tests/test_response_host.py. The kernel runs the same header
on the GPU in tests/test_gpu_render.py."""
import json
import subprocess

import numpy as np
import pytest

import _rendertest as T
from authorino_amd import response as R
from test_pipeline_host import OracleCtx
from test_response_host import DOC


def _render(outputs, n_slots, docs, vals, text, out_stride=4096):
    prog = T.HostProgram(outputs, n_slots)
    assert prog.rc == 0, prog.error
    return T.host_render(prog, docs, vals, text, out_stride)


def _configs(cfgs, docs):
    """compile_render of the configs over oracle selectors, rendered for docs: [r][k] text."""
    sel = R.ResponseSelectors(cfgs, OracleCtx())
    ops, keys = R.compile_render(cfgs, sel)
    vals, text = T.oracle_values(docs, sel.paths)
    rec, out = _render(ops.outputs, ops.n_slots, docs, vals, text)
    rows = []
    for r in range(len(docs)):
        row = []
        for k in range(len(keys)):
            st, got = T.rendered(rec, out, r, k)
            assert st == R.RENDER_OK, (r, k)
            row.append(got.decode("utf-8"))
        rows.append(row)
    return rows


def test_fuzz_every_value_under_every_op():
    """_rand_doc's value mix (numbers with -0, 1e21, 20 digits, 1.0e-7; escapes, surrogate
    pairs, lone surrogates; nested containers; duplicate and escaped keys), every value under
    each of the five ops, 300 documents: no output declined, every byte as the mirror's."""
    docs = T.fuzz_docs(300)
    vals, text = T.oracle_values(docs, T.FUZZ_PATHS)
    rec, out = _render(T.FUZZ_OUTPUTS, len(T.FUZZ_PATHS), docs, vals, text, T.FUZZ_STRIDE)
    assert not (rec[:, :, 2] != R.RENDER_OK).any()
    ends = T.check_all(rec, out, T.FUZZ_OUTPUTS, docs, vals, text, T.FUZZ_STRIDE)
    for r, e in enumerate(ends):  # nothing written past the dword that holds the text's end
        assert (out[r, (e + 3) // 4 * 4:] == 0xA5).all(), r


def test_reference_template_vectors():
    """json_test.go:136-205 (test_replace_json_placeholders' cases, modifiers included) as
    LIT / STRING programs."""
    cases = [("Nothing to replace", "Nothing to replace"), ("Username: {auth.identity.username}", "Username: john"),
             ("Username: {auth.identity.username}, Email: {auth.identity.email}", "Username: john, Email: john@test"),
             ("{auth.identity.email_verified} (bool)", "true (bool)"),
             (r"Github.com: {auth.identity.github\.com}", "Github.com: https://github.com/john"),
             (r"This is NOT a \{variable placeholder\}, {auth.identity.username}!",
              "This is NOT a {variable placeholder}, john!"),
             ("{auth.identity.username}", "john"), (r"\\{auth.identity.username} \\o/", r"\john \o/"),
             ("username: {auth.identity.username", "username: "),
             (r"username: {auth.ide{ntit/y.u\sername}", "username: "),
             ("Username: {auth.identity.username.@case:upper}", "Username: JOHN"),
             ('Domain: {auth.identity.email.@extract:{"sep":"@","pos":1}}', "Domain: test"),
             (r'Github username: {auth.identity.github\.com|@extract:{"sep":"/","pos":3}|@case:upper}',
              "Github username: JOHN"),
             (r'\{"msg":"I can build a JSON with dynamic values","username":"{auth.identity.github\.com|'
              r'@extract:{"sep":"/","pos":3}|@case:upper}"\}',
              '{"msg":"I can build a JSON with dynamic values","username":"JOHN"}')]
    cfgs = [R.ResponseConfig("r%d" % i, plain=R.JSONValue(pattern=t), wrapper_key="h%d" % i)
            for i, (t, _) in enumerate(cases) if R.JSONValue(pattern=t).is_template()]
    want = [w for t, w in cases if R.JSONValue(pattern=t).is_template()]
    assert len(cfgs) >= 12
    assert _configs(cfgs, [DOC])[0] == want


def test_reference_stringify_and_wrap_vectors():
    """json_test.go:265-320 and response_test.go / dynamic_json_test.go / plain_test.go
    (test_stringify_json, test_wrap_and_call) as MARSHAL / SPRINT programs."""
    src = {"prop_str": "str", "prop_num": 123, "prop_bool": False, "prop_null": None,
           "prop_obj": {"a_prop": "a_value"}, "prop_arr": ["a", "b", "c"]}
    doc = json.dumps({"v": src, "auth": {"identity": {"username": "john"}}}).encode()
    props = [(k, R.JSONValue(pattern="v." + k)) for k in src]
    cfgs = [R.ResponseConfig("all", json_properties=props, wrapper_key="all"),
            R.ResponseConfig("whole", json_properties=[("v", R.JSONValue(pattern="v"))], wrapper_key="whole"),
            R.ResponseConfig("dj", json_properties=[("prop1", R.JSONValue(static="value1")),
                                                    ("prop2", R.JSONValue(pattern="auth.identity.username"))],
                             wrapper_key="dj"),
            R.ResponseConfig("plain", plain=R.JSONValue(pattern="auth.identity.username"), wrapper_key="p"),
            R.ResponseConfig("static", plain=R.JSONValue(static="my-value"), wrapper_key="s")]
    big = ('{"prop_arr":["a","b","c"],"prop_bool":false,"prop_null":null,"prop_num":123,'
           '"prop_obj":{"a_prop":"a_value"},"prop_str":"str"}')
    assert _configs(cfgs, [doc])[0] == [big, '{"v":%s}' % big, '{"prop1":"value1","prop2":"john"}', "john",
                                        "my-value"]
    # the scalar vectors, one MARSHAL each
    paths = ["v.prop_str", "v.prop_num", "v.prop_bool", "v.prop_null", "v.prop_obj", "v.prop_arr", "v.nope"]
    vals, text = T.oracle_values([doc], paths)
    outs = [[(R.R_MARSHAL, s)] for s in range(len(paths))] + [[(R.R_STRING, 0)]]
    rec, out = _render(outs, len(paths), [doc], vals, text)
    got = [T.rendered(rec, out, 0, k) for k in range(len(outs))]
    assert got == [(0, b'"str"'), (0, b"123"), (0, b"false"), (0, b"null"), (0, b'{"a_prop":"a_value"}'),
                   (0, b'["a","b","c"]'), (0, b"null"), (0, b"str")]


def test_reference_number_vectors():
    """test_go_number_formatting's vectors: fmt %v and encoding/json of float64."""
    g = {1685557675.0: "1.685557675e+09", 123456.0: "123456", 1e6: "1e+06", 0.0001: "0.0001",
         1e-05: "1e-05", 0.5: "0.5", -2.25: "-2.25", 0.0: "0", 1e21: "1e+21", 5e-324: "5e-324",
         1234567.0: "1.234567e+06"}
    j = {1e21: "1e+21", 1e20: "100000000000000000000", 1e-7: "1e-7", 1e-6: "0.000001", 123.0: "123",
         0.1: "0.1", -1.5e-10: "-1.5e-10", 1.7976931348623157e308: "1.7976931348623157e+308"}
    nums = list(g) + list(j)
    body = ",".join('"k%d":%s' % (i, repr(x)) for i, x in enumerate(nums))
    s = "<a&b>\u2028\x01\"\\"
    doc = ('{%s,"m":{"b":[1.0,"x",null],"a":true},"s":%s,"inf":1e999}' % (body, json.dumps(s, ensure_ascii=False))
           ).encode()
    paths = ["k%d" % i for i in range(len(nums))] + ["m", "s", "inf"]
    vals, text = T.oracle_values([doc], paths)
    outs = [[(R.R_SPRINT if i < len(g) else R.R_MARSHAL, i)] for i in range(len(nums))]
    outs += [[(R.R_SPRINT, len(nums))], [(R.R_MARSHAL, len(nums) + 1)], [(R.R_MARSHAL, len(nums) + 2)],
             [(R.R_SPRINT, len(nums) + 2)]]
    rec, out = _render(outs, len(paths), [doc], vals, text)
    got = [T.rendered(rec, out, 0, k) for k in range(len(outs))]
    want = list(g.values()) + list(j.values()) + [
        "map[a:true b:[1 x <nil>]]", '"\\u003ca\\u0026b\\u003e\\u2028\\u0001\\"\\\\"', "", "+Inf"]
    assert got == [(0, w.encode()) for w in want]
    assert [w for w in T.mirror(outs, doc, vals[0], text[0])] == want  # (the mirror agrees with the vectors)


def test_decline_reasons_exactly():
    """Each reason gives UNRENDERED for its output alone: depth kMaxRenderDepth renders and
    one more declines; a \\xff byte under MARSHAL / STRING_ESC (the same string under STRING /
    SPRINT renders); a slot of type 255; an output one byte longer than what is left."""
    depth = T.lib().rt_max_depth()
    assert depth == 8
    outputs, n_slots, docs, vals, text, expected = T.decline_case(depth)
    assert sum(st == T.UNRENDERED for st, _ in expected) == 7
    rec, out = _render(outputs, n_slots, docs, vals, text)
    T.check_expected(rec, out, expected)
    assert T.rendered(rec, out, 0, 7)[1] == b"a\xffb\n"
    outputs, n_slots, docs, vals, text, expected = T.overflow_case()
    rec, out = _render(outputs, n_slots, docs, vals, text, out_stride=16)
    T.check_expected(rec, out, expected)
    assert int(rec[0, 2, 0]) == 10 and out[0].tobytes() == b"0123456789zabcde"


def test_inf_under_marshal_and_object_members():
    """An Inf under MARSHAL, top-level or nested, empties the whole output with status OK;
    objects of 0, 1, 2 and 5 members with duplicate keys and "\\u0061" against "a"."""
    doc = (b'{"i":1e999,"ai":[1,[2,-1e999]],"one":7,'
           b'"o0":{},"o1":{"k":1},"o2":{"b":1,"a":2},'
           b'"o5":{"b":1,"\\u0061":2,"a":{"z":[],"y":{}},"c":"x","b":"last"}}')
    paths = ["i", "ai", "one", "o0", "o1", "o2", "o5"]
    vals, text = T.oracle_values([doc], paths)
    outs = [[(R.R_LIT, b'{"p":'), (R.R_MARSHAL, 0), (R.R_LIT, b"}")], [(R.R_MARSHAL, 2)],
            [(R.R_LIT, b'{"q":'), (R.R_MARSHAL, 2), (R.R_LIT, b',"p":'), (R.R_MARSHAL, 1), (R.R_LIT, b"}")],
            [(R.R_SPRINT, 1)]]
    outs += [[(op, s)] for s in (3, 4, 5, 6) for op in (R.R_MARSHAL, R.R_SPRINT, R.R_STRING)]
    rec, out = _render(outs, len(paths), [doc], vals, text)
    assert not rec[:, :, 2].any()
    T.check_all(rec, out, outs, [doc], vals, text, 4096)
    assert [int(x) for x in rec[0, :4, 1]] == [0, 1, 0, len("[1 [2 -Inf]]")]
    k = 4 + 3 * 3
    assert T.rendered(rec, out, 0, k)[1] == b'{"a":{"y":{},"z":[]},"b":"last","c":"x"}'
    assert T.rendered(rec, out, 0, k + 1)[1] == b"map[a:map[y:map[] z:[]] b:last c:x]"


def test_sanitizer_program(tmp_path):
    """tests/native/san_render (ASan + UBSan, its own main) over the fuzz and the decline
    inputs: exit 0."""
    docs = T.fuzz_docs(300)
    vals, text = T.oracle_values(docs, T.FUZZ_PATHS)
    exp = [[(R.RENDER_OK, w.encode("utf-8")) for w in T.mirror(T.FUZZ_OUTPUTS, d, vals[r], text[r])]
           for r, d in enumerate(docs)]
    cases = [(T.FUZZ_OUTPUTS, len(T.FUZZ_PATHS), docs, vals, text, T.FUZZ_STRIDE, exp)]
    o, ns, d, v, t, e = T.decline_case(T.lib().rt_max_depth())
    prog = T.HostProgram(o, ns)
    rec, out = T.host_render(prog, d, v, t, 4096)
    # (expected bytes: the mirror's, except where bytes that are not UTF-8 pass through)
    cases.append((o, ns, d, v, t, 4096, [[(st, T.rendered(rec, out, 0, k)[1] if k in (7, 8) else w.encode("utf-8"))
                                          for k, (st, w) in enumerate(e)]]))
    o, ns, d, v, t, e = T.overflow_case()
    cases.append((o, ns, d, v, t, 16, [[(st, w.encode()) for st, w in e]]))
    path = tmp_path / "cases.bin"
    T.write_cases(str(path), cases)
    p = subprocess.run([T.make("san_render"), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "3 cases" in p.stdout


def test_compile_render_c5_and_compile_errors():
    """compile_render of the c5 AuthConfig: four outputs with the expected op lists; the
    checks authjx_render_compile makes (build_render_program, the code it runs) return
    AUTHJX_EINVAL. The entry point itself needs a device: tests/test_gpu_render.py."""
    from authorino_amd import workloads as W

    w = W.make("c5", n=4, seed=51)
    sel = R.ResponseSelectors(w.auth_config.response, OracleCtx())
    ops, keys = R.compile_render(w.auth_config.response, sel)
    assert keys == ["x-auth-user", "x-auth-exp", "x-auth-claims", "x-auth-ctx"]
    assert ops.n_slots == len(sel.paths) and len(ops.outputs) == 4
    kinds = [[op for op, _ in o] for o in ops.outputs]
    assert kinds[1] == [R.R_SPRINT]
    assert kinds[2][0] == R.R_LIT and R.R_MARSHAL in kinds[2] and kinds[2][-1] == R.R_LIT
    assert ops.outputs[2][0][1].startswith(b'{"acr":')
    for o in ops.outputs:
        assert all(op == R.R_LIT or 0 <= arg < ops.n_slots for op, arg in o)
    docs = [w.doc(i) for i in range(w.n)]
    rows = _configs(w.auth_config.response, docs)
    for r, doc in enumerate(docs):
        spans = sel.resolve([doc], *T.pack([doc]))
        want = [c.wrap_object_as_header_value(sel.call(c, doc, spans[0])) for c in w.auth_config.response]
        assert rows[r] == want and "e+09" in rows[r][1]
    EINVAL = -1
    assert T.HostProgram([[(R.R_STRING, 2)]], 2).rc == EINVAL        # slot >= n_slots
    assert T.HostProgram([[(R.R_LIT, b"x"), (5, 0)]], 1).rc == EINVAL  # unknown op
    assert T.HostProgram([[(R.R_LIT, b"x"), (R.R_MARSHAL, 0)]], 1).rc == 0
    prog = T.HostProgram([[(R.R_STRING, 1)]], 2)
    arena, offs, lens = T.pack([b"{}"])
    one = np.zeros((1, 1, 3), np.uint32)
    out = np.zeros((1, 16), np.uint8)
    rec = np.zeros((1, 1, 3), np.uint32)
    L = T.lib()
    call = lambda vs, os_: L.rt_render(prog._h, arena.ctypes.data, offs.ctypes.data, lens.ctypes.data, 1,  # noqa: E731
                                       one.ctypes.data, vs, None, 0, out.ctypes.data, os_, rec.ctypes.data)
    assert call(1, 16) == EINVAL   # values_stride < n_slots
    assert call(2, 24) == EINVAL and call(2, 0) == EINVAL  # out_stride no multiple of 16
