"""A seeded generator of Go regular expressions, of an equivalent for Python's `re` where one
exists, and of texts for them (tests/test_regex_diff.py, test_regex_values_host.py,
test_gpu_regex.py). A plain helper module.

A pattern is a syntax tree over the atoms below, joined by concatenation, `|`, the groups
`( ) (?: ) (?i: ) (?s: ) (?m: )` and the quantifiers `* + ? {2} {0,2} {1,} {2,3} *? +? ??`,
nested at most four deep. Each pattern is rendered twice: as Go writes it, and for Python's
`re` under re.ASCII (None where Python cannot say the same thing).

What differs between the two, and how the Python text accounts for it:
  `$` without (?m)   Go: only at the end of the text; Python: also before a final \\n -> \\Z
  `\\z`               Python writes \\Z
  `\\s`               Go: [\\t\\n\\f\\r ] (no \\v, regexp/syntax/perl_groups.go); written out
  `\\x{..}`           Python: \\UXXXXXXXX
  `[[:alpha:]]` ...  expanded
  a quantified `^ $ \\b ...`   Go accepts it, Python says "nothing to repeat": None
  `(x*)*` and the like    an unbounded repeat of an unbounded repeat: Python backtracks for
                      minutes on a text of twenty runes: None
  (?i:                Go folds by unicode.SimpleFold, so k s reach U+212A and U+017F, a class
                      that holds U+212A folds to k, and non-ASCII letters fold; Python under
                      re.ASCII folds A-Z only. None unless everything under the flag folds
                      within ASCII both ways (Atom.ci).
"""
from __future__ import annotations

import re
from collections import namedtuple

import numpy as np

# go text, python text, members (texts of one rune the atom accepts: the directed walk's
# choices), ci: the same language under (?i: in Go and in Python's re.ASCII,
# width: False for the empty-width atoms (Python refuses to repeat them)
Atom = namedtuple("Atom", "go py members ci width")

_PY_S = " \\t\\n\\r\\f"


def _lit(c, ci=True):
    go = "\\" + c if c in ".-" else c
    return Atom(go, re.escape(c), [c], ci and c not in "ksKS", True)


ATOMS = (
    [_lit(c) for c in "abcksKSAZz019_- ."]
    + [
        Atom(".", ".", ["a", "é", " ", "\U0010ffff"], True, True),
        Atom("\\d", "\\d", ["0", "9"], True, True),
        Atom("\\D", "\\D", ["a", "_", "é"], True, True),
        Atom("\\w", "\\w", ["a", "K", "_", "1"], False, True),
        Atom("\\W", "\\W", ["-", " ", "é", "\n"], False, True),
        Atom("\\s", "[" + _PY_S + "]", [" ", "\n", "\t"], True, True),
        Atom("\\S", "[^" + _PY_S + "]", ["a", "é", "-"], True, True),
        Atom("[a-c]", "[a-c]", ["a", "b", "c"], True, True),
        Atom("[^a-c]", "[^a-c]", ["k", "\n", "é", "0"], True, True),
        Atom("[0-9_]", "[0-9_]", ["0", "_", "9"], True, True),
        Atom("[^\\n]", "[^\\n]", ["a", " ", "ÿ"], True, True),
        Atom("[\\d\\s]", "[\\d" + _PY_S + "]", ["1", " ", "\n"], True, True),
        Atom("[^\\W]", "[^\\W]", ["s", "_", "0"], False, True),
        Atom("[[:alpha:]]", "[A-Za-z]", ["k", "S", "a"], False, True),
        Atom("[[:^digit:]]", "[^0-9]", ["a", "-", "é"], True, True),
        Atom("é", "é", ["é"], False, True),
        Atom("[à-ÿ]", "[à-ÿ]", ["à", "é", "ÿ"], False, True),
        Atom("[^é]", "[^é]", ["a", "É", "\n", "Ā"], False, True),
        Atom("\\x41", "\\x41", ["A"], True, True),
        Atom("\\x{10FFFF}", "\\U0010ffff", ["\U0010ffff"], False, True),
        Atom("[\\x{100}-\\x{10FFFF}]", "[\\u0100-\\U0010ffff]", ["Ā", "ſ", "K", "\U0010ffff"], False, True),
        Atom("\\n", "\\n", ["\n"], True, True),
        Atom("\\b", "\\b", [""], True, False),
        Atom("\\B", "\\B", [""], True, False),
        Atom("^", "^", [""], True, False),
        Atom("$", None, [""], True, False),  # (rendered by the (?m) context)
        Atom("\\A", "\\A", [""], True, False),
        Atom("\\z", "\\Z", [""], True, False),
        Atom("(?:)", "(?:)", [""], True, True),
    ]
)
# (a third of the draws are literals, an eighth the empty-width atoms at the end: patterns
# made mostly of either kind match everything or nothing)
_N_LIT = 17
_N_EMPTY = 7

QUANTS = ["*", "+", "?", "{2}", "{0,2}", "{1,}", "{2,3}", "*?", "+?", "??"]
_QRANGE = {"*": (0, 3), "+": (1, 3), "?": (0, 1), "{2}": (2, 2), "{0,2}": (0, 2), "{1,}": (1, 3), "{2,3}": (2, 3),
           "*?": (0, 3), "+?": (1, 3), "??": (0, 1)}
GROUPS = ["(", "(?:", "(?i:", "(?s:", "(?m:"]
MAX_DEPTH = 4

# the texts' alphabet: the atoms' ASCII, what JSON escapes shortly, runes of 2, 3 and 4 bytes
VALID_UNITS = [c.encode() for c in "abcksKSAZz019_- .\n\t\"\\/"] + [
    c.encode() for c in ["é", "É", "ÿ", "à", "Ā", "ſ", "K", "\U0010ffff"]]
# not UTF-8: a byte that starts nothing, a lead byte alone, an overlong form, a 3-byte rune
# cut short, a surrogate, a rune past U+10FFFF (each byte of these is one U+FFFD to Go)
INVALID_UNITS = [b"\xff", b"\xc3", b"\xc0\xaf", b"\xe0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"]

Pattern = namedtuple("Pattern", "go py tree")


# --- trees: ("atom", Atom) ("cat", [t]) ("alt", [t]) ("grp", opener, t) ("rep", t, quant)
def _gen(rng, depth):
    r = rng.random()
    if depth >= MAX_DEPTH or r < 0.3:
        r = rng.random()
        if r < 0.35:
            return ("atom", ATOMS[int(rng.integers(0, _N_LIT))])
        if r < 0.47:
            return ("atom", ATOMS[int(rng.integers(len(ATOMS) - _N_EMPTY, len(ATOMS)))])
        return ("atom", ATOMS[int(rng.integers(_N_LIT, len(ATOMS) - _N_EMPTY))])
    if r < 0.55 or (depth == 0 and r < 0.75):  # (a root that is a sequence is rarely nullable)
        return ("cat", [_gen(rng, depth + 1) for _ in range(int(rng.integers(2, 5)))])
    if r < 0.68:
        return ("alt", [_gen(rng, depth + 1) for _ in range(int(rng.integers(2, 4)))])
    if r < 0.82:
        return ("grp", GROUPS[int(rng.integers(0, len(GROUPS)))], _gen(rng, depth + 1))
    t = _gen(rng, depth + 1)
    if t[0] in ("cat", "alt", "rep"):  # (a** is an error in Go: a repeat of a repeat takes a group)
        t = ("grp", GROUPS[int(rng.integers(0, 2))], t)
    return ("rep", t, QUANTS[int(rng.integers(0, len(QUANTS)))])


def render_go(t) -> str:
    k = t[0]
    if k == "atom":
        return t[1].go
    if k == "cat":
        return "".join("(?:" + render_go(x) + ")" if x[0] == "alt" else render_go(x) for x in t[1])
    if k == "alt":
        return "|".join(render_go(x) for x in t[1])
    if k == "grp":
        return t[1] + render_go(t[2]) + ")"
    return render_go(t[1]) + t[2]


_UNBOUNDED = ("*", "+", "{1,}", "*?", "+?")


def _has_unbounded(t) -> bool:
    if t[0] == "atom":
        return False
    if t[0] in ("cat", "alt"):
        return any(_has_unbounded(x) for x in t[1])
    if t[0] == "grp":
        return _has_unbounded(t[2])
    return t[2] in _UNBOUNDED or _has_unbounded(t[1])


def render_py(t, ci=False, multi=False):
    """The Python text of t under the flags in force, or None."""
    k = t[0]
    if k == "atom":
        a = t[1]
        if ci and not a.ci:
            return None
        if a.go == "$":
            return "$" if multi else "\\Z"
        return a.py
    if k == "cat":
        parts = []
        for x in t[1]:
            s = render_py(x, ci, multi)
            if s is None:
                return None
            parts.append("(?:" + s + ")" if x[0] == "alt" else s)
        return "".join(parts)
    if k == "alt":
        parts = [render_py(x, ci, multi) for x in t[1]]
        return None if None in parts else "|".join(parts)
    if k == "grp":
        s = render_py(t[2], ci or t[1] == "(?i:", multi or t[1] == "(?m:")
        return None if s is None else t[1] + s + ")"
    if t[1][0] == "atom" and not t[1][1].width:
        return None
    if t[2] in _UNBOUNDED and _has_unbounded(t[1]):
        return None
    s = render_py(t[1], ci, multi)
    return None if s is None else s + t[2]


def holds_not_boundary(p: Pattern) -> bool:
    """p has a \\B (Python before 3.14 says it does not match the empty text)."""
    def walk(t):
        if t[0] == "atom":
            return t[1].go == "\\B"
        if t[0] in ("cat", "alt"):
            return any(walk(x) for x in t[1])
        return walk(t[2] if t[0] == "grp" else t[1])
    return walk(p.tree)


def pattern(rng, host=None) -> Pattern:
    """One generated pattern. host: a function of the Go text that gives the device
    compiler's status (0 ok); where it is not 0 there is no Python text either."""
    t = _gen(rng, 0)
    go = render_go(t)
    py = render_py(t)
    if py is not None and host is not None and host(go) != 0:
        py = None
    return Pattern(go, py, t)


def mutate(rng, go: str) -> str:
    """go with one byte deleted, or one of ()[]{}*+?|\\^- inserted."""
    b = go.encode()
    i = int(rng.integers(0, len(b) + 1))
    if rng.random() < 0.4 and len(b):
        i = min(i, len(b) - 1)
        b = b[:i] + b[i + 1:]
    else:
        c = b"()[]{}*+?|\\^-"
        b = b[:i] + c[int(rng.integers(0, len(c))):][:1] + b[i:]
    return b.decode("utf-8", "replace")


# --- texts (bytes)
def random_text(rng, invalid=True) -> bytes:
    units = VALID_UNITS + INVALID_UNITS if invalid else VALID_UNITS
    return b"".join(units[int(rng.integers(0, len(units)))] for _ in range(int(rng.integers(0, 9))))


def _walk(rng, t, out):
    k = t[0]
    if k == "atom":
        m = t[1].members
        out.append(m[int(rng.integers(0, len(m)))])
    elif k == "cat":
        for x in t[1]:
            _walk(rng, x, out)
    elif k == "alt":
        _walk(rng, t[1][int(rng.integers(0, len(t[1])))], out)
    elif k == "grp":
        _walk(rng, t[2], out)
    else:
        lo, hi = _QRANGE[t[2]]
        for _ in range(int(rng.integers(lo, hi + 1))):
            _walk(rng, t[1], out)


def directed_text(rng, p: Pattern, invalid=True) -> bytes:
    """A walk of p's tree that emits a member of each atom it passes (a likely match),
    half the time with one rune deleted, inserted or replaced (a likely near miss)."""
    runes = []
    _walk(rng, p.tree, runes)
    units = [r.encode() for r in "".join(runes)][:24]
    if rng.random() < 0.5:
        pool = VALID_UNITS + INVALID_UNITS if invalid else VALID_UNITS
        u = pool[int(rng.integers(0, len(pool)))]
        i = int(rng.integers(0, len(units) + 1))
        e = int(rng.integers(0, 3))
        if e == 0 and units:
            del units[min(i, len(units) - 1)]
        elif e == 1 and units:
            units[min(i, len(units) - 1)] = u
        else:
            units.insert(i, u)
    return b"".join(units)


def texts(rng, p: Pattern, n: int, invalid=True):
    """n texts for p: random and directed ones alternate."""
    return [directed_text(rng, p, invalid) if j & 1 else random_text(rng, invalid) for j in range(n)]


def is_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


# --- JSON documents around a text: {"pad":"…","v":VALUE,"w":W}
_SHORT = {0x0A: b"\\n", 0x09: b"\\t", 0x22: b'\\"', 0x5C: b"\\\\", 0x2F: b"\\/"}


def _units(text: bytes):
    """text cut into its runes' bytes; a byte that starts no rune is a unit of its own."""
    out, i = [], 0
    while i < len(text):
        b = text[i]
        k = 1 if b < 0xC2 else 2 if b < 0xE0 else 3 if b < 0xF0 else 4 if b < 0xF5 else 1
        if not is_utf8(text[i:i + k]):
            k = 1
        out.append(text[i:i + k])
        i += k
    return out


def json_raw(text: bytes) -> bytes:
    """text as a JSON string with only what JSON must escape escaped."""
    return b'"' + b"".join(_SHORT[u[0]] if len(u) == 1 and u[0] in (0x0A, 0x09, 0x22, 0x5C) else u
                           for u in _units(text)) + b'"'


def json_escaped(rng, text: bytes) -> bytes:
    """text as a JSON string with a random subset of its runes written as \\uXXXX (a
    surrogate pair for an astral rune), \\n \\t \\" \\\\ \\/ as their short escapes, and now
    and then a lone high surrogate or a reversed pair put in (gjson: U+FFFD)."""
    out = []
    for u in _units(text):
        if len(u) == 1 and u[0] in _SHORT:
            out.append(_SHORT[u[0]])
        elif is_utf8(u) and rng.random() < 0.5:
            c = ord(u.decode())
            if c >= 0x10000:
                c -= 0x10000
                out.append(b"\\u%04x\\u%04X" % (0xD800 + (c >> 10), 0xDC00 + (c & 0x3FF)))
            else:
                out.append(b"\\u%04x" % c)
        else:
            out.append(u)
        r = rng.random()
        if r < 0.04:
            out.append(b"\\ud83d")
        elif r < 0.08:
            out.append(b"\\udc00\\ud800")
    return b'"' + b"".join(out) + b'"'


# numbers whose String() is not their text, the literals, containers (String() is the raw
# text), and None: no "v" at all
OTHER_VALUES = [b"1e3", b"1.50", b"-0", b"1E+2", b"0.000001", b"1e21", b"true", b"false", b"null",
                b'{"a":[1,"x"]}', b"[1,2]", None]


def document(value, pad: int, w: bytes = b"z") -> bytes:
    v = b"" if value is None else b'"v":' + value + b","
    return b'{"pad":"' + b"p" * pad + b'",' + v + b'"w":"' + w + b'"}'


RULESET_PATTERNS = 16


def chain_any(n):
    """Any(p0, Any(p1, ...)) over n patterns: (nodes, root)."""
    nodes = [(0, -1, -1, i) for i in range(n)]
    root = -1
    for i in reversed(range(n)):
        nodes.append((2, i, root, -1))
        root = len(nodes) - 1
    return nodes, root


_RULESETS = {}


def table_rulesets(seed: int = 2024):
    """The table packed for the per-request code: [(patterns, nodes, root, docs)], 16 table
    patterns as `matches` on v and one eq on w under an Any chain; docs: every text of the 16
    as a raw and as an escaped string, and OTHER_VALUES, behind 0..15 bytes of padding, a
    third of them with the w that makes the request true whatever v is."""
    if seed not in _RULESETS:
        tab = table(seed)
        rng = np.random.default_rng(seed + 1)
        out = []
        for k in range(0, len(tab), RULESET_PATTERNS):
            part = tab[k:k + RULESET_PATTERNS]
            pats = [("v", 5, p.go) for p, _ in part] + [("w", 1, "z")]
            values = []
            for _, tx in part:
                for t in tx:
                    values += [json_raw(t), json_escaped(rng, t)]
            values += OTHER_VALUES
            docs = [document(v, int(rng.integers(0, 16)), b"z" if j % 3 == 0 else b"y") for j, v in enumerate(values)]
            nodes, root = chain_any(len(pats))
            out.append((pats, nodes, root, docs))
        _RULESETS[seed] = out
    return _RULESETS[seed]


def pack(docs):
    """(arena with 64 bytes of slack, offs, lens) of docs laid end to end."""
    lens = np.array([len(d) for d in docs], dtype=np.uint32)
    offs = np.zeros(len(docs), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(docs) + b"\0" * 64, dtype=np.uint8).copy(), offs, lens


TABLE_PATTERNS = 192
TABLE_TEXTS = 12
_TABLES = {}


def table(seed: int = 2024):
    """[(Pattern, [text])]: TABLE_PATTERNS patterns the device compiler takes (status 0,
    no duplicates), TABLE_TEXTS texts each: the one table the CPU and GPU tests share."""
    if seed not in _TABLES:
        import _hosttest as H

        rng = np.random.default_rng(seed)
        out, seen = [], set()
        while len(out) < TABLE_PATTERNS:
            p = pattern(rng, host=lambda g: H.HostRegex(g).status)
            if p.go in seen or H.HostRegex(p.go).status != 0:
                continue
            seen.add(p.go)
            out.append((p, texts(rng, p, TABLE_TEXTS)))
        _TABLES[seed] = out
    return _TABLES[seed]
