"""A seeded generator of JSON values for the render tests (tests/test_render_values_host.py,
tests/test_gpu_render_values.py): number tokens, string bodies, object keys, containers and
the documents around them. A plain helper module; every draw comes from the
`random.Random(seed)` it is given, so a seed names a corpus.

Numbers   random float64 bit patterns as repr / %.17g / %.16g / %.15g; integers of 1-25
          digits, with trailing zeros; d.f of up to 19 + 21 digits; 0.000...d; <int>e<+-30>;
          THRESHOLDS, the texts around every layout switch of 'g', 'f' and encoding/json's
          'e'; EDGES (subnormals, the smallest normal's neighbours, the largest double,
          overflow to Inf, underflow to 0, the zeros).
Strings   sequences of ATOMS: ASCII with JSON's and HTML's special characters, every JSON
          escape, \\u escapes (NUL, U+2028 / U+2029, a pair, lone and mismatched surrogates),
          raw runes at the 1/2/3/4-byte edges; short (0-12 atoms) or long (to ~3,000 bytes).
          Always valid UTF-8 without raw control bytes.
Keys      KEYS: a pool that collides (a / \\u0061, raw and escaped runes), nests (a, ab,
          a\\u0000) and orders bytes above 0x7F against ASCII, plus random short strings.
Containers random objects (0-12 members) and arrays to a chosen depth, random whitespace
          around every token and colon, the three literals.
Documents {"x":{"k0":V0,...,"k7":V7}} (PATHS), every slot under every op (OUTPUTS).
Depth profile  depth_doc(i): a value of exactly 1 + (5 i mod 8) levels whose members are
          derived from i.
"""
from __future__ import annotations

import math
import struct

from authorino_amd import response as R

MAX_DEPTH = 8  # kMaxRenderDepth (tests/_rendertest.py lib().rt_max_depth() is asserted equal)
OPS = (R.R_STRING, R.R_STRING_ESC, R.R_SPRINT, R.R_MARSHAL)
N_SLOTS = 8
PATHS = ["x.k%d" % k for k in range(N_SLOTS)]
# every slot under every op (a LIT in front of STRING, so that the fifth op is there too)
OUTPUTS = [([(R.R_LIT, b"v=")] if op == R.R_STRING else []) + [(op, s)] for s in range(N_SLOTS) for op in OPS]

# ---- numbers ----
_MANTISSAS = ["1", "9.999999999999999", "9.9999999999999995", "1.0000000000000002", "2.5", "1.00"]
_EXPONENTS = list(range(-8, -2)) + list(range(4, 8)) + list(range(19, 24))
THRESHOLDS = [m + e + s + str(abs(x)) for m in _MANTISSAS for x in _EXPONENTS for e in "eE"
              for s in (("-",) if x < 0 else ("", "+"))]
EDGES = ["5e-324", "4.9e-324", "2.4e-324", "2.5e-324", "2.225073858507201e-308", "2.2250738585072014e-308",
         "2.225073858507202e-308", "1.7976931348623157e308", "1e400", "-1e400", "1e999", "1e-400", "-1e-400",
         "-0", "-0.0", "0e5", "-0e-3"]


def _digits(rng, n, first_nonzero=True):
    s = "".join(rng.choice("0123456789") for _ in range(n))
    if first_nonzero and s[0] == "0":
        s = rng.choice("123456789") + s[1:]
    return s


def float_bits(rng) -> float:
    """A finite float64 of a random bit pattern."""
    while True:
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if math.isfinite(x):
            return x


def number(rng) -> str:
    """One JSON number token."""
    k = rng.randrange(10)
    if k < 3:
        x = float_bits(rng)
        f = rng.randrange(4)
        return repr(x) if f == 0 else ("%.17g", "%.16g", "%.15g")[f - 1] % x
    sign = "-" if rng.random() < 0.25 else ""
    if k == 3:
        return sign + _digits(rng, rng.randrange(1, 26))
    if k == 4:
        return sign + _digits(rng, rng.randrange(1, 8)) + "0" * rng.randrange(1, 19)
    if k == 5:
        return sign + _digits(rng, rng.randrange(1, 20)) + "." + _digits(rng, rng.randrange(1, 22), False)
    if k == 6:
        return sign + "0." + "0" * rng.randrange(1, 12) + _digits(rng, rng.randrange(1, 18))
    if k == 7:
        return sign + _digits(rng, rng.randrange(1, 18)) + rng.choice("eE") + rng.choice(["", "+", "-"]) + str(
            rng.randrange(0, 31))
    if k == 8:
        return sign + rng.choice(THRESHOLDS)
    return rng.choice(EDGES)


# ---- strings: atoms are bytes as they stand between the quotes of the document ----
_ASCII = [c.encode() for c in "abcxyzABZ019_-.{}[],:<>&' "] + [b"\x7f"]
_ESCAPES = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t"]
_UESC = [b"\\u0000", b"\\u001f", b"\\u0041", b"\\u00e9", b"\\u2028", b"\\u2029", b"\\ud83d\\ude00", b"\\ud800",
         b"\\udc00", b"\\ud800\\u0041"]
_RAW = [chr(c).encode("utf-8") for c in (0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x1F600, 0x10FFFF, 0x2028, 0x2029)]
ATOMS = _ASCII + _ESCAPES + _UESC + _RAW


def _atom(rng) -> bytes:
    r = rng.random()  # (half ASCII: a string of escapes alone has no plain runs to copy)
    return rng.choice(_ASCII) if r < 0.5 else rng.choice(_ESCAPES) if r < 0.65 else rng.choice(_UESC) if r < 0.82 \
        else rng.choice(_RAW)


def short_string(rng) -> bytes:
    """The body (between the quotes) of a string of 0-12 atoms."""
    return b"".join(_atom(rng) for _ in range(rng.randrange(0, 13)))


def long_string(rng) -> bytes:
    """A body of 200 to about 3,000 bytes."""
    want = rng.randrange(200, 3000)
    parts, n = [], 0
    while n < want:
        parts.append(_atom(rng))
        n += len(parts[-1])
    return b"".join(parts)


# ---- keys ----
KEYS = [b"", b"a", b"\\u0061", b"ab", b"a\\u0000", b"b", b"B", chr(0xE9).encode(), b"\\u00e9", b"a\\/b", b"a/b", b'\\"',
        b"k<", chr(0x1F600).encode(), b"\\ud83d\\ude00", b"\\ud800", chr(0xFFFF).encode(), b"~", b"\x7f"]


def key(rng) -> bytes:
    if rng.random() < 0.8:
        return rng.choice(KEYS)
    return b"".join(_atom(rng) for _ in range(rng.randrange(0, 4)))


# ---- containers ----
_WS = [b" ", b"\n", b"\t", b"\r\n"]


def ws(rng) -> bytes:
    r = rng.random()
    return b"" if r < 0.6 else rng.choice(_WS) if r < 0.9 else rng.choice(_WS) + rng.choice(_WS)


def scalar(rng) -> bytes:
    r = rng.random()
    if r < 0.4:
        return number(rng).encode()
    if r < 0.85:
        return b'"' + short_string(rng) + b'"'
    return rng.choice([b"true", b"false", b"null"])


def value(rng, depth: int) -> bytes:
    """A value of at most `depth` container levels (0: a scalar)."""
    if depth <= 0:
        return scalar(rng)
    obj = rng.random() < 0.5
    m = rng.randrange(0, 13) if obj else rng.randrange(0, 7)
    deep = rng.randrange(m) if m and rng.random() < 0.7 else -1  # (one member goes all the way down)
    parts = []
    for j in range(m):
        d = depth - 1 if j == deep else rng.randrange(depth) if rng.random() < 0.15 else 0
        v = ws(rng) + value(rng, d) + ws(rng)
        parts.append(ws(rng) + b'"' + key(rng) + b'"' + ws(rng) + b":" + v if obj else v)
    body = b",".join(parts) if parts else ws(rng)
    return (b"{" + body + b"}") if obj else (b"[" + body + b"]")


# ---- documents ----
def wrap(values) -> bytes:
    """{"x":{"k0":V0,...}}; a None leaves its key out (the selector finds nothing)."""
    return b'{"x":{' + b",".join(b'"k%d":' % k + v for k, v in enumerate(values) if v is not None) + b"}}"


def document(rng, long_p: float = 0.04) -> bytes:
    vals = []
    for _ in range(N_SLOTS):
        r = rng.random()
        if r < 0.3:
            v = number(rng).encode()
        elif r < 0.55:
            v = b'"' + short_string(rng) + b'"'
        elif r < 0.55 + long_p:
            v = b'"' + long_string(rng) + b'"'
        elif r < 0.9:
            v = value(rng, rng.randrange(1, MAX_DEPTH + 1))
        elif r < 0.96:
            v = rng.choice([b"true", b"false", b"null"])
        else:
            v = None
        vals.append(None if v is None else ws(rng) + v + ws(rng))
    return wrap(vals)


def corpus(rng, n: int):
    return [document(rng) for _ in range(n)]


def long_docs(rng, n: int):
    """Documents whose slot 0 is a long string."""
    return [wrap([b'"' + long_string(rng) + b'"']) for _ in range(n)]


# ---- the depth profile ----
DEPTH_PATHS = ["x.k0"]
DEPTH_OUTPUTS = [[(R.R_SPRINT, 0)], [(R.R_MARSHAL, 0)]]


def depth_levels(i: int) -> int:
    return 1 + (5 * i) % MAX_DEPTH


def depth_doc(i: int) -> bytes:
    """Document i of the profile: exactly depth_levels(i) levels, objects and arrays in turn
    (odd i starts with an array), every key and scalar derived from i. Consecutive documents
    have depths 1, 6, 3, 8, 5, 2, 7, 4: the lanes of a wave hold every depth, and what a
    lane's level l holds differs from every other lane's."""
    n = depth_levels(i)
    v = b'"leaf%d"' % i
    for lv in reversed(range(n)):
        if (lv + i) % 2 == 0:  # (keys out of order, one of them escaped, the nested member in the middle)
            v = b'{"z%d":%d,"m%d_%d":%s,"\\u0061%d":"%d.%d"}' % (i, lv, i, lv, v, i, i, lv)
        else:
            v = b'[%d.5,%s,"e%d_%d"]' % (i, v, i, lv)
    return wrap([v])


def nesting(raw: bytes) -> int:
    """Container levels of a JSON text (strings skipped)."""
    deep = cur = 0
    i, n = 0, len(raw)
    while i < n:
        c = raw[i]
        if c == 0x22:
            i += 1
            while raw[i] != 0x22:
                i += 2 if raw[i] == 0x5C else 1
        elif c in b"{[":
            cur += 1
            deep = max(deep, cur)
        elif c in b"}]":
            cur -= 1
        i += 1
    return deep
