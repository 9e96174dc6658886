"""CPU tests of what the kernels do to one request or one span, run as built: the host build
calls the bodies of authorino_amd/csrc/ajx_request.h (the exact scan, the select kernel's
request) and ajx_stream_body.h (the streaming kernel's span, its stage-B list) that the
kernels call, and the answers are compared with the oracle. Each case is the smallest shape
that reaches its path."""
import numpy as np
import pytest

import _hosttest as H
import fuzz_util as FU
import pyoracle as O

POISON = 0xDEADBEEFDEADBEEF


def _pack(docs):
    lens = np.array([len(d) for d in docs], dtype=np.uint32)
    offs = np.zeros(len(docs), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), offs, lens


def _bits(rs, n, d):
    return sum(1 << p for p in range(n) if rs.pattern(p, d) == 1)


# ---- the exact scan's body (eval_scan_one) ----

def _exact_docs(ns):
    full = "{" + ",".join('"k%d":"v%d"' % (i, i % 3) for i in range(ns)) + "}"
    return [full.encode(),                                           # all found
            full.replace('"k5":"v2",', "").encode(),                 # a key missing
            full[: len(full) // 2].encode(),                         # truncated JSON
            full.replace('"k1"', '"k\\u0031"').encode()]             # an escaped key


def _check_exact(hr, trees, docs, mods=-1):
    """eval_scan_one with a 3-word poisoned bitmap and without one: tri-state and error index
    per tree as the oracle's, T bits as the oracle's patterns, the third word zero."""
    rss = [O.Ruleset(*t) for t in trees]
    n_all = sum(len(t[0]) for t in trees)
    for d in docs:
        want = [rs.matches(d) for rs in rss]
        bits, base = 0, 0
        for rs, t in zip(rss, trees):
            bits |= _bits(rs, len(t[0]), d) << base
            base += len(t[0])
        for stride in (3, 0):
            tri, err, bm = H.eval_exact(hr, d, mods=mods, stride=stride, n_trees=len(trees))
            assert tri == [w[0] for w in want], (d, stride)
            # (a forest numbers its patterns across the trees)
            off = np.cumsum([0] + [len(t[0]) for t in trees])
            assert err == [w[1] + int(off[k]) if w[1] >= 0 else w[1] for k, w in enumerate(want)], (d, stride)
            if stride:
                assert n_all <= 128 and bm[2] == 0
                assert bm[0] | (bm[1] << 64) == bits, (d, hex(bits))


@pytest.mark.parametrize("ns,np_", [(33, 65), (32, 64)])
def test_exact_body_caches_and_their_off_paths(ns, np_):
    """One selector and one pattern over the per-request caches (kSelCache 32, kPatCache 64:
    every pattern re-resolved by gj_get, the fold re-evaluating them), and exactly at them."""
    pats = [("k%d" % (i % ns), 1 + (i % 2), "v%d" % (i % 3)) for i in range(np_)]
    nodes, root = FU.chain(np_)
    hr = H.HostRuleset(pats, nodes, root)
    assert hr.rc == 0, hr.error
    _check_exact(hr, [(pats, nodes, root)], _exact_docs(ns))
    for d in _exact_docs(ns):  # (and ht_eval's per-pattern values, read from what the body wrote)
        rs = O.Ruleset(pats, nodes, root)
        t, e, res = hr.eval(d)
        assert (t, e) == rs.matches(d) and res == [rs.pattern(p, d) for p in range(np_)]


def test_exact_body_forest():
    """A two-tree forest: one fold program and one result per tree."""
    t0 = ([("k0", 1, "v0"), ("k5", 2, "v2"), ("k7", 3, "1")], *FU.chain(3))
    t1 = ([("k1", 1, "v1"), ("k9", 4, "v")], *FU.chain(2))
    hr = H.HostRuleset.forest([t0, t1])
    assert hr.rc == 0, hr.error
    _check_exact(hr, [t0, t1], _exact_docs(12))


def test_exact_body_modifier_instance():
    """The MODS instance: a modifier chain on one selector (value_of read twice) and a "#."
    list on another, named and as the launcher picks it for this ruleset."""
    pats = [("user.name|@case:upper", 1, "JOHN DOE"), ("items.#.id", 3, "7"), ("user.name", 1, "John Doe")]
    nodes, root = FU.chain(3)
    hr = H.HostRuleset(pats, nodes, root)
    assert hr.rc == 0 and hr.status == [0, 0, 0], (hr.error, hr.status)
    full = '{"user":{"name":"John Doe"},"items":[{"id":3},{"id":7}]}'
    docs = [full.encode(), b'{"items":[{"id":3}]}', full[:30].encode(),
            full.replace('"name"', '"n\\u0061me"').encode()]
    _check_exact(hr, [(pats, nodes, root)], docs, mods=1)
    _check_exact(hr, [(pats, nodes, root)], docs, mods=-1)  # (the launcher's choice: the same instance)


# ---- the streaming kernel's bodies (stream_body, stream_fin_list, stream_finish_entry) ----

STREAM_PATS = [("a", 1, "1"), ("b", 2, "v"), ("c.d", 3, "x"), ("n", 1, "1.50")]
INVALID_DOC = b'{"a":1,"b"}'


def _oracle_all(pats, nodes, root, arena, offs, lens, tri, err, bm):
    rs = O.Ruleset(pats, nodes, root)
    otri, oerr, obm = O.eval_batch([rs], arena, offs, lens)
    np.testing.assert_array_equal(tri, otri)
    np.testing.assert_array_equal(err, oerr)
    np.testing.assert_array_equal(bm[:, :obm.shape[1]], obm)


@pytest.mark.parametrize("merge", [True, False])
def test_stream_one_request_per_wave_invalid_document(merge):
    """per = 1 with one document the stream cannot prove: with merge_slow its id goes to the
    stage-B list flagged kStageExact (the slow list only counts it), without to the slow
    list; the exact body's answer is the oracle's either way."""
    nodes, root = FU.chain(len(STREAM_PATS))
    docs = [b'{"a":1,"b":"w"}', b'{"c":{"d":["x"]},"a":1}', INVALID_DOC, b'{"n":1.5,"b":"v"}']
    a, o, ln = _pack(docs)
    hr = H.HostRuleset(STREAM_PATS, nodes, root)
    tri, err, bm, slow, lst = H.eval_stream(hr, a, o, ln, per=1, merge_slow=merge, lists=True)
    assert slow[2] == 1 and lst["slow_after_spans"] >= 1
    flagged = [e & ~H.STAGE_EXACT for e in lst["stage"] if e & H.STAGE_EXACT]
    plain = [e for e in lst["stage"] if not e & H.STAGE_EXACT]
    if merge:
        assert 2 in flagged and 2 not in plain and lst["slow_ids"] == []
    else:
        assert flagged == [] and 2 not in plain and 2 in lst["slow_ids"]
        assert sorted(lst["slow_ids"]) == [int(r) for r in np.nonzero(slow == 1)[0]]
    _oracle_all(STREAM_PATS, nodes, root, a, o, ln, tri, err, bm)


def test_stream_keep_rows_forest_and_select_from_rows():
    """keep_rows on a two-tree forest whose second tree is a root-less eq per selector: every
    request leaves a row, the invalid request's is kRowSlow, and the select kernel's body reads
    from those rows what it reads from the documents."""
    nodes, root = FU.chain(len(STREAM_PATS))
    sels = list(dict.fromkeys(p[0] for p in STREAM_PATS))
    hr = H.HostRuleset.forest([(STREAM_PATS, nodes, root), ([(s, 1, "") for s in sels], [], -1)])
    assert hr.rc == 0, hr.error
    docs = [b'{"a":1,"b":"w"}', b'{"c":{"d":["x","y"]},"a":1}', INVALID_DOC, b'{"n":1.50,"b":"v\\n"}',
            b'{"b":"' + b"q" * 2500 + b'","a":1}']  # (a value across steps: an open record, through stage B)
    a, o, ln = _pack(docs)
    row_stride = 5 + 16
    rows = np.full(64 * row_stride, POISON, np.uint64)
    tri, err, bm, slow = H.eval_stream(hr, a, o, ln, keep_rows=True, rows=rows, row_stride=row_stride, n_out=2)
    for r in range(len(docs)):
        assert rows[r] != POISON, r  # (word 0 of work-item r in the wave layout)
        t2, e2, b2 = H.eval_exact(hr, docs[r], stride=2, n_trees=2)
        assert (list(tri[r]), list(err[r]), list(bm[r])) == (t2, e2, b2), r
    assert rows[2] == H.ROW_SLOW and slow[2] == 1
    rs = O.Ruleset(STREAM_PATS, nodes, root)
    assert [int(t) for t in tri[:, 0]] == [rs.matches(d)[0] for d in docs]
    p0 = len(STREAM_PATS)
    from_rows = H.select_rows(hr, a, o, ln, len(sels), rows=rows, row_stride=row_stride, p0=p0, wave_rows=True)
    exact = H.select_rows(hr, a, o, ln, len(sels), p0=p0)
    np.testing.assert_array_equal(from_rows, exact)


@pytest.mark.parametrize("wave_off", [64 * 1024, 0])
def test_stream_multi_tenant_two_rulesets(wave_off):
    """The MT instance, three requests under two rulesets: with room for the wave's own copy
    of its blob, and with none (the blob read in place)."""
    p1, p2 = STREAM_PATS, [("b", 1, "v"), ("a", 2, "2"), ("n", 4, "5")]
    n1, r1 = FU.chain(len(p1))
    n2, r2 = FU.chain(len(p2))
    h1, h2 = H.HostRuleset(p1, n1, r1), H.HostRuleset(p2, n2, r2)
    docs = [b'{"a":1,"b":"w","n":1.50}', b'{"b":"v","a":2,"n":[5,6]}', INVALID_DOC]
    a, o, ln = _pack(docs)
    sor = np.array([0, 1, 0], np.uint32)
    tri, err, bm, slow = H.eval_stream(h1, a, o, ln, hr2=h2, set_of_req=sor, wave_off=wave_off)
    otri, oerr, obm = O.eval_batch([O.Ruleset(p1, n1, r1), O.Ruleset(p2, n2, r2)], a, o, ln, set_of_req=sor)
    np.testing.assert_array_equal(tri, otri)
    np.testing.assert_array_equal(err, oerr)
    np.testing.assert_array_equal(bm[:, :obm.shape[1]], obm)
    assert slow[2] == 1


def test_stream_stage_b_list_by_either_function():
    """One stage-B list, with entries of both kinds (a request the stream flagged for the
    exact scan, and one whose stage B runs on its row because its span did not fit a step),
    run by stream_fin_list and by stream_finish_entry: identical outputs, the oracle's."""
    pats = STREAM_PATS + [("s", 5, "^q+$")]
    nodes, root = FU.chain(len(pats))
    docs = [b'{"a":1,"s":"' + b"q" * 2300 + b'"}', INVALID_DOC, b'{"n":1.5,"s":"qq"}', b'{"s":"' + b"q" * 2300 + b'x"}']
    a, o, ln = _pack(docs)
    hr = H.HostRuleset(pats, nodes, root)
    outs = [H.eval_stream(hr, a, o, ln, per=1, fin=fin, lists=True) for fin in (True, False)]
    stage = outs[0][4]["stage"]
    assert any(e & H.STAGE_EXACT for e in stage) and any(not e & H.STAGE_EXACT for e in stage), stage
    for x, y in zip(outs[0][:4], outs[1][:4]):
        np.testing.assert_array_equal(x, y)
    _oracle_all(pats, nodes, root, a, o, ln, *outs[0][:3])


# ---- the select kernel's body (select_request) ----

SEL_PATS = [("user.name", 1, ""), ("missing.key", 1, ""), ("tags.1", 1, ""), ("esc", 1, ""), ("num", 1, ""),
            ("tags.#(x==1)", 1, "")]
SEL_MOD = ("user.name|@case:upper", 1, "")  # (a ruleset with a modifier chain takes no single-pass scan: no rows)
SEL_DOCS = [b'{"user":{"name":"John"},"tags":["a","b"],"esc":"x\\ny","num":-1.5e3}',
            b'{"num":7,"user":{"name":"A\\u00e9"},"tags":[]}',
            b'{"user" : {"name":"ws"}, "tags":[1,2]}',   # (whitespace: the lean scan hands it over)
            b'{"user":{"name":"John"}']                   # (truncated: both scans hand it over)


@pytest.mark.parametrize("scan", ["tok", "lean"])
def test_select_body_from_capture_rows(scan):
    """select_request on the rows of the token scanner and of the lean scan: every pattern's
    {start, len, type | esc} is the exact Get's (the same body without rows), which is the
    oracle's span; a selector that is not found, a slow row, a window of the patterns (p0 > 0,
    stride short of the rest) and an unsupported pattern."""
    # (the response selectors' shape: a forest whose last, root-less tree holds them, so that
    # the lean scan keeps their records too)
    hr = H.HostRuleset.forest([([("num", 1, "7")], *FU.chain(1)), (SEL_PATS, [], -1)])
    assert hr.rc == 0, hr.error
    H.lean_keep(True)
    n_sel, p0 = len(SEL_PATS), 1
    rows = np.zeros((len(SEL_DOCS), 1 + n_sel), np.uint64)
    for k, d in enumerate(SEL_DOCS):
        row = (H.eval_tok if scan == "tok" else H.eval_lean)(hr, d, mis=3 * k, n_sel=n_sel)[3]
        rows[k] = row if row is not None else [H.ROW_SLOW] + [POISON] * n_sel
    assert rows[0, 0] != H.ROW_SLOW and rows[3, 0] == H.ROW_SLOW
    a, o, ln = _pack(SEL_DOCS)
    np_ = len(SEL_PATS)
    exact = H.select_rows(hr, a, o, ln, np_, p0=p0)
    got = H.select_rows(hr, a, o, ln, np_, rows=rows.reshape(-1), row_stride=1 + n_sel, p0=p0)
    np.testing.assert_array_equal(got, exact)
    for k, d in enumerate(SEL_DOCS):
        for p in range(5):
            t, st, n = O.gjson_span(d, SEL_PATS[p][0])
            assert (int(exact[k, p, 2]) & 0xFF, int(exact[k, p, 1])) == (t, n), (k, p)
            assert n == 0 or int(exact[k, p, 0]) == st, (k, p)
        assert int(exact[k, 1, 2]) & 0xFF == 0 and int(exact[k, 1, 1]) == 0  # (not found: T_NULL)
        assert int(exact[k, 5, 2]) == 0xFF  # (unsupported)
    # patterns [2, 4) of 7: stride smaller than the rest
    win = H.select_rows(hr, a, o, ln, 2, rows=rows.reshape(-1), row_stride=1 + n_sel, p0=p0 + 1)
    np.testing.assert_array_equal(win, exact[:, 1:3])


def test_select_body_modifier_selector_needs_text():
    """A selector with a modifier chain reports 0xFF from the instance without TEXT; the TEXT
    instance resolves it to built text in the request's slot."""
    pats = SEL_PATS[:1] + [SEL_MOD]
    nodes, root = FU.chain(2)
    hr = H.HostRuleset(pats, nodes, root)
    assert hr.rc == 0 and hr.status == [0, 0], hr.status
    a, o, ln = _pack(SEL_DOCS[:2])
    plain = H.select_rows(hr, a, o, ln, 2)
    assert [int(x) for x in plain[:, 1, 2]] == [0xFF, 0xFF] and int(plain[0, 0, 2]) & 0xFF != 0xFF
    vals, text = H.select_rows(hr, a, o, ln, 2, text_stride=64)
    np.testing.assert_array_equal(vals[:, 0], plain[:, 0])
    st, n = int(vals[0, 1, 0]), int(vals[0, 1, 1])
    assert int(vals[0, 1, 2]) & 0xFF != 0xFF and bytes(text[st:st + n]).strip(b'"') == b"JOHN"
