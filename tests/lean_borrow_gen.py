"""Documents for the tests of the lean walk taking the next sub-window's tokens early
(tests/test_lean_borrow.py on the host build, tests/test_gpu_lean_borrow.py on the kernel):
the edge family, which moves each kind of member over every offset of a sub-window pair and
breaks or cuts the document in and after the member, and documents of equal length with
many and with few tokens, so that lanes of one wave finish a sub-window at different times."""
import lean_reads_gen as G

EDGE_PATS = [("k", 1, "v"), ("k", 2, "0123456789abcdef"), ("num", 1, "12"), ("num", 2, "123456"), ("t", 1, "true"),
             ("n", 1, ""), ("o.in", 1, "abc"), ("o", 2, ""), ("sq", 2, ""), ("e", 2, "x"), ("z", 1, "1"),
             ("long", 1, G.LONG), ("o.deep.in", 1, "abc"), ("o.deep", 2, "")]
EDGE_ARR_PATS = EDGE_PATS + [("arr.0", 1, "w"), ("arr.2", 1, "true"), ("arr.3.in", 1, "abc"), ("arr.4", 1, "12"),
                             ("arr.5", 1, "")]
EDGE_MEMBERS = [
    '"k":"v"', '"k":""', '"k":"0123456789abcdef"', '"k":"%s"' % ("s" * 29), '"long":"%s"' % G.LONG,
    '"num":12', '"num":1', '"num":123456', '"num":-1.5e10', '"t":true', '"t":false', '"n":null', '"u":12',
    '"o":{"in":"abc"}', '"o":{}', '"o":{"x":1,"in":"abc","y":[1]}', '"o":{"deep":{"in":"abc"}}',
    '"sq":{"x":{"y":[1,{"q":2}]},"w":"}"}', '"sq":[]', '"sq":[[],[[]],{"a":"]"}]', '"e":{}', '"u":{"v":{"w":{}}}',
    '"arr":["w","x",true,{"in":"abc"},12,null]', '"arr":[12,[1,2],true,{"in":"abc","z":{}},12]', '"arr":[]',
    '"arr":[null,null,true]', '"arr":[{"in":"no"},"a long element string here",true,{"x":1,"in":"abc"}]',
]
EDGE_TAILS = ['"z":1}', None, '"z":{"a":{}}}']
# (a mismatched close, a value where a key belongs, a key without a value, a second
# colon, a broken literal, a paren: failures in the token's own or the next bytes)
EDGE_BREAKS = [(b"}", b"]"), (b',"z"', b',{"z"'), (b":", b""), (b":", b"::"), (b"true", b"trux"), (b",", b"(,")]


def edge_doc(kind, pad, tail):
    t = EDGE_TAILS[tail % len(EDGE_TAILS)]
    body = '{"pad":"%s",%s' % ("p" * pad, EDGE_MEMBERS[kind])
    return (body + ("," + t if t else "}")).encode()


def edge_docs():
    """Every member at pads 0..70 (each of its bytes at every offset of a sub-window pair),
    then the same documents broken after the pad (the first failure in the member or just
    after it) and cut short inside and after the member (containers that never close)."""
    k = 0
    for kind in range(len(EDGE_MEMBERS)):
        for pad in range(71):
            d = edge_doc(kind, pad, k)
            yield d, True
            at = d.find(b'",') + 2  # the member's first byte
            a, b = EDGE_BREAKS[k % len(EDGE_BREAKS)]
            j = d.find(a, at + (k % 3))
            if j >= 0:
                yield d[:j] + b + d[j + len(a):], False
            yield d[:at + 1 + (k * 5) % (len(d) - at)], False
            k += 1


def dense_doc(n):
    """n bytes of short members: a token every few bytes."""
    body, end, i = '{"k":"v","num":12', ',"z":"%s"}', 0
    while True:
        m = ',"a%d":%d' % (i % 10, i % 7)
        if len(body) + len(m) + len(end % "") > n:
            break
        body += m
        i += 1
    return (body + end % ("f" * (n - len(body) - len(end % "")))).encode()


def sparse_doc(n):
    """n bytes of three long strings: a handful of tokens."""
    fill = n - len('{"pad":"","k":"v","long":"","num":12}')
    a = fill // 2
    return ('{"pad":"%s","k":"v","long":"%s","num":12}' % ("p" * a, "q" * (fill - a))).encode()
