"""Documents that put the lean walker's grouped ring reads (ajx_lean.h, Walk::walk) at their
edges, for tests/test_lean_reads.py (host build) and tests/test_gpu_lean_reads.py (kernel).

A document is `{"pad":"ppp…",MEMBER,TAIL}` (or with MEMBER last). The pad string's length
moves MEMBER over every byte offset 0..127 of the ring: a key's closing quote at each offset
of a 32-byte sub-window, the key's last 8 bytes and the value's first bytes across the
16-byte chunks, the 32- and 64-byte boundaries and the ring's wrap at 128, a value that
starts in the last bytes of the sub-window pair, a literal that ends exactly at a
sub-window's end. The document's misalignment (0..15) shifts all of that once more."""
import fuzz_util as FU

EQ, NEQ, INCL, EXCL = 1, 2, 3, 4
LIT_LENS = (0, 1, 7, 8, 9, 15, 16, 17)  # eager literals hold up to 16 bytes: 17 goes to stage B


def lit(n):
    return "0123456789abcdefg"[:n]


LONG = "The quick brown fox jumps over the lazy dog, twice over."  # 56 bytes: pending over sub-windows


def patterns(arr):
    """[(selector, op, value)]; arr: with an array-index selector (the walker's ARR instance)."""
    ps = []
    for n in LIT_LENS:
        ps += [("s%d" % n, EQ, lit(n)), ("s%d" % n, NEQ, lit(n))]
    ps += [("t", EQ, "true"), ("f", EQ, "false"), ("n", EQ, ""), ("n", NEQ, "null"),
           ("pv", EQ, LONG), ("pv", NEQ, "x"), ("es", EQ, 'a"' + LONG), ("k\\\\q", EQ, "v"),
           ("a-long-key-name", EQ, "A"), ("b-long-key-name", EQ, "B"), ("b-long-key-name", NEQ, "A"),
           ("o.in", EQ, "abc"), ("o", NEQ, ""), ("num", EQ, "12"), ("q.s8", EQ, lit(8))]
    if arr:
        ps += [("arr.1", EQ, "x"), ("arr.2", EQ, "true"), ("arr.3.in", EQ, "abc")]
    return ps


def _members():
    """MEMBER texts: every eager literal length equal and differing in its last byte only, the
    literals and a broken one, a string pending over two sub-windows (with and without a
    backslash near its start, which the walk then knows only as `lbs1`), a backslash in the
    key and in the value, long keys sharing their last 8 bytes, a container, an array."""
    ms = []
    for n in LIT_LENS:
        ms.append('"s%d":"%s"' % (n, lit(n)))
        if n:
            ms.append('"s%d":"%sX"' % (n, lit(n)[:-1]))
            ms.append('"s%d":"%s"' % (n, lit(n) + "Y"))  # (one byte longer)
    ms += ['"t":true', '"t":false', '"f":false', '"n":null', '"n":nul0', '"t":truE', '"num":12', '"num":123',
           '"pv":"%s"' % LONG, '"pv":"%sZ"' % LONG[:-1], '"es":"a\\"%s"' % LONG, '"es":"a\\"%s"' % LONG[:-1],
           '"s8":"0123\\u0034567"', '"s8":"01234\\\\7"', '"k\\\\q":"v"', '"k\\\\q":"w"', '"s\\u0038":"01234567"',
           '"a-long-key-name":"A"', '"b-long-key-name":"B"', '"c-long-key-name":"B"', '"b-long-key-name":"A"',
           '"o":{"in":"abc"}', '"o":{"x":{"in":"no"},"in":"abc"}', '"o":{}', '"q":{"s8":"%s"}' % lit(8),
           '"q":{"s8":"%s","t":true}' % lit(8), '"arr":["w","x",true,{"in":"abc"}]', '"arr":["x","w",false,{"in":"abd"}]',
           '"arr":[[1,2],"x",true]', '"arr":[]']
    return ms


MEMBERS = _members()
TAILS = ('"z":1}', None, '"zz":"\\\\"}')  # (None: MEMBER is the object's last member)
PADS = 128


def doc(kind, pad, tail=0, bs_pad=False):
    """bs_pad: the pad string ends in an escaped backslash (a backslash just before MEMBER,
    in MEMBER's own sub-window or only in the one before it)."""
    p = "p" * pad + ("\\\\" if bs_pad else "")
    t = TAILS[tail % len(TAILS)]
    body = '{"pad":"%s",%s' % (p, MEMBERS[kind % len(MEMBERS)])
    return (body + ("," + t if t else "}")).encode()


def sweep():
    """Every member at every pad length 0..127 (tails and the pad's backslash in rotation)."""
    k = 0
    for kind in range(len(MEMBERS)):
        for pad in range(PADS):
            yield doc(kind, pad, tail=k, bs_pad=(k % 5 == 0))
            k += 1


def sample(count, stride=37):
    """`count` documents of the sweep, `stride` apart (coprime to its length: kinds, pads and
    tails all rotate)."""
    docs = list(sweep())
    assert len(docs) % stride != 0
    return [docs[(i * stride) % len(docs)] for i in range(count)]


def chain(n):
    return FU.chain(n)
