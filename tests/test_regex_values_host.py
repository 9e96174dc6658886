"""`matches` on every kind of value through the per-request code on its host build: the
table's patterns (tests/regex_gen.py) on raw strings, strings with \\u escapes (surrogate
pairs, a lone or reversed surrogate), numbers whose String() is not their text, true /
false / null, raw object and array text and a missing value, through the lean scan, the
streaming kernels' bodies and the exact scan; verdicts, tri-state and error index equal to
the oracle's. The GPU tests (tests/test_gpu_regex.py) run the same rulesets and documents."""
import numpy as np
import pytest

import _hosttest as H
import pyoracle as O
import regex_gen as G

RULESETS = range(G.TABLE_PATTERNS // G.RULESET_PATTERNS)


@pytest.fixture(scope="module")
def oracle():
    """Per ruleset: (HostRuleset, docs, tri, err, bitmap, per-pattern verdicts by the oracle)."""
    out = []
    for pats, nodes, root, docs in G.table_rulesets():
        hr = H.HostRuleset(pats, nodes, root)
        assert hr.rc == 0 and not any(hr.status), (hr.error, hr.status)
        rs = O.Ruleset(pats, nodes, root)
        arena, offs, lens = G.pack(docs)
        tri, err, bm = O.eval_batch([rs], arena, offs, lens)
        res = [[rs.pattern(p, d) for p in range(len(pats))] for d in docs]
        assert not any(O.UNSUPPORTED in r for r in res)
        out.append((hr, docs, tri, err, bm, res))
    return out


def test_documents_cover_every_value_kind():
    sets = G.table_rulesets()
    assert len(sets) == len(RULESETS)
    docs = [d for _, _, _, ds in sets for d in ds]
    assert len(docs) == len(sets) * (2 * G.RULESET_PATTERNS * G.TABLE_TEXTS + len(G.OTHER_VALUES))
    for piece in (b"\\ud83d", b"\\udc00\\ud800", b"\\udbff\\uDFFF", b"\\n", b"\\t", b'\\"', b"\\\\", b"\\/", b"\\u00e9",
                  b"\xff", b"\xed\xa0\x80", b"\xf4\x8f\xbf\xbf", b'"v":1e21', b'"v":null', b'"v":[1,2]', b'"v":{"a"'):
        assert any(piece in d for d in docs), piece
    assert {d.index(b'",') - len(b'{"pad":"') for d in docs} == set(range(16))


@pytest.fixture(params=[False, True], ids=["", "arr"])
def arr(request):
    """Both instances of lean_request: the launcher's choice and the array-walking one (the
    kernel without a staged blob and the tenant kernel run it for every ruleset)."""
    H.lean_arr(request.param)
    yield request.param
    H.lean_arr(False)


@pytest.mark.parametrize("k", RULESETS)
def test_values_lean_scan(oracle, k, arr):
    hr, docs, tri, err, bm, res = oracle[k]
    decided = 0
    for j, d in enumerate(docs):
        tl, el, lres, _ = H.eval_lean(hr, d, mis=j & 15)
        assert tl != -2, "the ruleset is not eligible for the lean scan"
        if tl < 0:
            continue  # (handed to the exact scan: test_values_exact_scan)
        decided += 1
        assert (tl, el) == (tri[j], err[j]), (j, d)
        if 3 not in lres:
            assert lres == res[j], (j, d)
    print(f"ruleset {k}: lean scan decided {decided} of {len(docs)}")
    assert decided >= len(docs) // 2  # (the lean scan's own walkers saw most of them)


@pytest.mark.parametrize("k", RULESETS)
def test_values_stream(oracle, k):
    hr, docs, tri, err, bm, res = oracle[k]
    arena, offs, lens = G.pack(docs)
    out = H.eval_stream(hr, arena[:-64], offs, lens)
    assert out is not None, "the ruleset has no stream tables"
    stri, serr, sbm, slow = out
    np.testing.assert_array_equal(stri, tri)
    np.testing.assert_array_equal(serr, err)
    np.testing.assert_array_equal(sbm[:, :bm.shape[1]], bm)
    print(f"ruleset {k}: stream {int((slow == 0).sum())}, stage B {int((slow == 2).sum())}, "
          f"exact scan {int((slow == 1).sum())} of {len(docs)}")
    assert (slow == 1).sum() <= len(docs) // 2  # (the stream and its stage B decided most)


@pytest.mark.parametrize("k", RULESETS)
def test_values_exact_scan(oracle, k):
    hr, docs, tri, err, bm, res = oracle[k]
    for j, d in enumerate(docs):
        t, e, r = hr.eval(d)
        assert (t, e) == (tri[j], err[j]), (j, d)
        assert r == res[j], (j, d)
        xt, xe, xbm = H.eval_exact(hr, d, stride=1)
        assert (xt[0], xe[0], xbm[0]) == (tri[j], err[j], bm[j, 0]), (j, d)
