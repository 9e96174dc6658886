"""The regex compiler (csrc/ajx_regex.cpp, host build) against the oracle's Pike VM
(oracle/regex_ref.c) and, where Python can say the same thing, against Python's `re`, on
generated patterns and texts (tests/regex_gen.py); the answers generated texts cannot reach,
each pinned with its place in Go's documentation or source; and the product's DFA limits."""
import re

import numpy as np
import pytest

import _hosttest as H
import pyoracle as O
import regex_gen as G


def _host_status(go):
    return H.HostRegex(go).status


def _oracle_status(r: "O.Regex") -> int:
    return 2 if r.unsupported else 0 if r._h else 1


def test_table_has_both_verdicts():
    """The shared table: at least 192 patterns of 12 texts, and by the oracle alone at least
    60 % of the patterns have both a matching and a non-matching text (a table of patterns
    that match everything, as nullable unanchored ones do, would check no walker)."""
    tab = G.table()
    assert len(tab) >= 192 and all(len(t) >= 12 for _, t in tab)
    both = all_true = all_false = 0
    for p, texts in tab:
        r = O.Regex(p.go)
        assert r._h, p.go
        v = {r.match(t) for t in texts}
        both += v == {True, False}
        all_true += v == {True}
        all_false += v == {False}
    print(f"table: {len(tab)} patterns, both verdicts {both}, all true {all_true}, all false {all_false}")
    assert both >= 0.6 * len(tab)


def test_compile_status_and_error_text_agree():
    """Generated patterns and one-byte mutations of them: the device compiler's status (ok,
    error, unsupported) is the oracle's, and an error's text is equal."""
    rng = np.random.default_rng(77)
    counts = {0: 0, 1: 0, 2: 0}
    for k in range(3000):
        p = G.pattern(rng)
        cands = [p.go] + [G.mutate(rng, p.go) for _ in range(2)]
        for go in cands:
            h, o = H.HostRegex(go), O.Regex(go)
            assert h.status == _oracle_status(o), (go, h.status, h.error, o.error)
            if h.status == 1:
                assert h.error == o.error, go
            counts[h.status] += 1
    print(f"compile agreement: ok {counts[0]}, error {counts[1]}, unsupported {counts[2]}")
    assert counts[0] > 3000 and counts[1] > 300 and counts[2] > 100


N_VERDICT_PATTERNS = 12000  # (about 10 s)
N_VERDICT_TEXTS = 24


def test_verdicts_agree_three_ways():
    """Host DFA == oracle Pike VM on every (pattern, text), texts that are not UTF-8 among
    them; == Python's re.search where the pattern has a Python text and the text is UTF-8
    (but for the empty text under a \\B, which Python before 3.14 says does not match)."""
    rng = np.random.default_rng(4242)
    pairs = py_pairs = n_py = n_pat = 0
    for _ in range(N_VERDICT_PATTERNS):
        p = G.pattern(rng, host=_host_status)
        h = H.HostRegex(p.go)
        if h.status != 0:
            continue
        o = O.Regex(p.go)
        assert o._h, p.go
        n_pat += 1
        pr = re.compile(p.py, re.ASCII) if p.py is not None else None
        n_py += pr is not None
        skip_empty = pr is not None and G.holds_not_boundary(p)
        for t in G.texts(rng, p, N_VERDICT_TEXTS):
            hv = h.match(t)
            assert hv == o.match(t), (p.go, t)
            pairs += 1
            if pr is not None and G.is_utf8(t) and not (skip_empty and not t):
                assert hv == (pr.search(t.decode()) is not None), (p.go, p.py, t)
                py_pairs += 1
    print(f"verdict agreement: {n_pat} patterns ({n_py} with a Python text), {pairs} pairs host == oracle, "
          f"{py_pairs} pairs == Python re")
    assert pairs > 100000 and py_pairs > 20000


# Known answers the three-way leg cannot reach (Python does not say these, or says otherwise).
KNOWN = [
    # regexp/syntax doc: (?i) folds by unicode.SimpleFold; its orbits k K U+212A and s S U+017F
    # (unicode/letter.go SimpleFold's own examples)
    ("(?i)k", "K".encode(), True),
    ("(?i)s", "ſ".encode(), True),
    # regexp/syntax: \B "not at ASCII word boundary": both sides of the empty text are not
    # word characters, so it holds, and \b does not
    ("\\B", b"", True),
    ("\\b", b"", False),
    # regexp/syntax: $ "at end of text (like \z not \Z) or line (flag m=true)"
    ("a$", b"a\n", False),
    ("(?m)a$", b"a\n", True),
    # regexp/syntax: . "any character, possibly including newline (flag s=true)"
    ("^.$", b"\n", False),
    ("(?s)^.$", b"\n", True),
    # regexp/syntax: \s "whitespace (== [\t\n\f\r ])": no \v
    ("\\s", b"\v", False),
    # a negated class holds \n (syntax.ClassNL is among the parser's flags only without Perl's)
    ("^[^a]$", b"\n", True),
    # utf8.DecodeRune: "If the encoding is invalid, it returns (RuneError, 1)": every invalid
    # byte is one U+FFFD (regexp's input reads by DecodeRune, regexp/regexp.go inputBytes.step)
    ("^.$", b"\xff", True),
    ("^.$", b"\xff\xfe", False),
    ("^..$", b"\xff\xfe", True),
    # a surrogate's three bytes are invalid each (unicode/utf8 accept ranges: ED takes 80..9F)
    ("^...$", b"\xed\xa0\x80", True),
    ("^.$", b"\xed\xa0\x80", False),
    ("^\\x{FFFD}{3}$", b"\xed\xa0\x80", True),
]


@pytest.mark.parametrize("pat,text,want", KNOWN)
def test_known_answers(pat, text, want):
    h, o = H.HostRegex(pat), O.Regex(pat)
    assert h.status == 0 and o._h
    assert o.match(text) is want
    assert h.match(text) is want


AB10 = "[ab]*a[ab]{10}$"
AB11 = "[ab]*a[ab]{11}$"


def many_classes(n=260) -> str:
    """n single-rune sets, no two adjacent: n + 1 rune classes and more with the compiler's own cuts."""
    return "".join(chr(0x100 + 2 * k) for k in range(n))


def test_dfa_limits_are_unsupported_not_guessed():
    """kMaxDfaStates = 4096, kMaxDfaClasses = 255 (csrc/ajx_blob.h): a pattern under the
    limit compiles, one over it is RX_UNSUPPORTED (never a DFA cut short); the oracle, which
    builds no DFA, compiles all three."""
    h = H.HostRegex(AB10)
    assert h.status == 0 and 2048 <= h.states <= 4096, h.states
    print(f"{AB10}: {h.states} states")
    for t in (b"a" + b"b" * 10, b"bb" + b"a" + b"ab" * 5, b"b" * 11, b"a" * 10):
        assert h.match(t) == O.Regex(AB10).match(t)
    assert H.HostRegex(AB11).status == 2
    mc = many_classes()
    assert H.HostRegex(mc).status == 2
    assert H.HostRegex(many_classes(200)).status == 0
    for pat in (AB10, AB11, mc):
        assert O.Regex(pat)._h, pat
    assert O.Regex(mc).match(("x" + mc).encode()) and not O.Regex(mc).match(mc[1:].encode())


def _fold_case(kind, pats):
    """pats under one And (1) / Or (2) chain on the host build: per document (tri, err) of the
    exact scan, the lean scan and the stream, and the oracle's (which compiles every regexp)."""
    nodes = [(0, -1, -1, i) for i in range(len(pats))]
    root = -1
    for i in reversed(range(len(pats))):
        nodes.append((kind, i, root, -1))
        root = len(nodes) - 1
    hr, rs = H.HostRuleset(pats, nodes, root), O.Ruleset(pats, nodes, root)
    assert hr.rc == 0, hr.error
    mc = many_classes()
    hit = "x" + mc if any(p[2] == mc for p in pats) else "bbbbba" + "b" * 11
    docs = [('{"v":"%s","w":"%s"}' % (v, w)).encode() for v in (hit, "bbbb") for w in ("z", "q")]
    out = []
    for d in docs:
        t, e, _ = hr.eval(d)
        tl, el, _, _ = H.eval_lean(hr, d)
        assert tl < 0 or (tl, el) == (t, e), d
        out.append((t, e))
    arena = np.frombuffer(b"".join(docs), dtype=np.uint8)
    lens = np.array([len(d) for d in docs], dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    st = H.eval_stream(hr, arena, offs, lens)
    if st is not None:
        assert [(int(a), int(b)) for a, b in zip(st[0], st[1])] == out
    return hr, out, [rs.matches(d) for d in docs]


@pytest.mark.parametrize("big", [AB11, many_classes()], ids=["states", "classes"])
def test_too_large_regexp_is_no_error_and_yields_to_decided_operands(big):
    """Go's And / Or return the first operand that is an error or decides them. A regexp over
    the DFA limits is unsupported but compiles in Go, so it is T or F, never an error: the
    decided operands after it are looked at first (the compiler moves it behind them), and
    Any(<too large>, w eq "z") is T where w is "z", All(<too large>, w eq "z") is F where it is
    not; whatever the device decides is the oracle's answer. Behind an operand that is an
    error, or in front of one, nothing changes: the error, or UNDECIDED."""
    # documents: (v matches, w == z), (v matches, w != z), (v does not, z), (v does not, not z)
    hr, got, want = _fold_case(2, [("v", 5, big), ("w", 1, "z")])
    assert hr.status == [2, 0]
    assert got == [(1, -1), (3, 0), (1, -1), (3, 0)]
    assert [want[0], want[2]] == [(1, -1), (1, -1)]
    hr, got, want = _fold_case(1, [("v", 5, big), ("w", 1, "z")])
    assert got == [(3, 0), (0, -1), (3, 0), (0, -1)]
    assert [want[1], want[3]] == [(0, -1), (0, -1)]
    # an operand that is an error behind it: Go gives T or the error, by the regexp
    hr, got, want = _fold_case(2, [("v", 5, big), ("v", 5, "a**"), ("w", 1, "z")])
    assert hr.status == [2, 1, 0]
    assert [t for t, _ in got] == [3, 3, 3, 3]
    assert [t for t, _ in want] == [1, 1, 2, 2]
    # an error in front of it decides: nothing behind it is looked at
    hr, got, want = _fold_case(2, [("v", 5, "a**"), ("v", 5, big), ("w", 1, "z")])
    assert got == want == [(2, 0)] * 4
    # a regexp that is unsupported for its syntax may be an error in Go: it stays in front
    hr, got, want = _fold_case(2, [("v", 5, "\\p{Greek}"), ("w", 1, "z")])
    assert hr.status == [2, 0] and [t for t, _ in got] == [3, 3, 3, 3]
    # nested: the group that holds it is not moved, the operand inside it is
    pats = [("v", 5, big), ("w", 1, "z"), ("w", 1, "q")]
    nodes = [(0, -1, -1, 0), (0, -1, -1, 1), (0, -1, -1, 2), (2, 0, 1, -1), (1, 3, 2, -1)]  # All(Any(big, w=z), w=q)
    hn, rn = H.HostRuleset(pats, nodes, 4), O.Ruleset(pats, nodes, 4)
    for v in ("bbbbba" + "b" * 11, "bbbb"):
        d = ('{"v":"%s","w":"z"}' % v).encode()
        assert hn.eval(d)[:2] == rn.matches(d) == (0, -1)  # (Any is T, w eq q is F)
