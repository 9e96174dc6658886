"""CPU test of the lean walker's grouped ring reads (ajx_lean.h, Walk::walk: the key's last 8
bytes and the value's first 8 read together before the key table; the content's other bytes
with the eager entry) on the host build, against the oracle. The documents
(tests/lean_reads_gen.py) move each kind of member over every ring offset 0..127, and every
document is scanned at every misalignment 0..15, so each read falls on every chunk,
sub-window and window boundary and on the ring's wrap."""
import pytest

import _hosttest as H
import lean_reads_gen as G
import pyoracle as O


@pytest.fixture(scope="module", params=[False, True], ids=["no_array_selector", "array_selector"])
def rulesets(request):
    pats = G.patterns(request.param)
    nodes, root = G.chain(len(pats))
    return pats, O.Ruleset(pats, nodes, root), H.HostRuleset(pats, nodes, root)


@pytest.fixture(scope="module")
def docs():
    return list(G.sweep())


def test_generator_reaches_the_edges(docs):
    """The cases the sweep must hold (found in its documents, not assumed): a key's closing
    quote at every offset of a sub-window; a key's last 8 bytes across the 16-, 32- and
    64-byte boundaries and the ring's wrap; a value that starts 33 bytes past a sub-window's
    base; a literal that ends at a sub-window's end; eager literals of every length."""
    quote_off, straddle, v33, lit_end = set(), set(), False, set()
    for d in docs:
        for key in (b'"s8":', b'"a-long-key-name":', b'"t":', b'"n":', b'"f":'):
            at = d.find(key)
            if at < 0:
                continue
            cq = at + len(key) - 2  # the key's closing quote
            for mis in range(16):
                quote_off.add((cq + mis) % 32)
                first, last = (cq - 8 + mis) % 128, (cq - 1 + mis) % 128
                for b in (16, 32, 64, 128):
                    if first // b != last // b or last < first:
                        straddle.add(b if last >= first else 128)
                v33 |= (cq + mis) % 32 == 31  # (the value starts at the quote + 2)
                if key in (b'"t":', b'"n":', b'"f":'):
                    end = min(x for x in (d.find(b",", cq), d.find(b"}", cq)) if x >= 0)  # first byte after it
                    lit_end.add((end + mis) % 32)
    assert quote_off == set(range(32))
    assert straddle == {16, 32, 64, 128}
    assert v33
    assert 0 in lit_end
    assert {len(G.lit(n)) for n in G.LIT_LENS} == {0, 1, 7, 8, 9, 15, 16, 17}


def test_grouped_reads_match_the_oracle(rulesets, docs):
    pats, rs, hr = rulesets
    assert hr.rc == 0, hr.error
    n_lean = n_slow = 0
    for d in docs:
        ot = [rs.pattern(p, d) for p in range(len(pats))]
        t_or, _ = rs.matches(d)
        for mis in range(16):
            tl, _, lres, _ = H.eval_lean(hr, d, mis=mis)
            assert tl != -2
            if tl < 0 or 3 in lres:  # (handed to the exact scan: escaped keys, broken literals)
                n_slow += 1
                continue
            n_lean += 1
            assert lres == ot, (d, mis)
            assert tl == t_or, (d, mis)
    # the lean scan decides all but the members written for the exact scan
    assert n_lean > 0.8 * 16 * len(docs), (n_lean, n_slow)


def test_lean_takes_the_plain_members(rulesets):
    """Members without escapes in the key or broken literals are decided by the lean scan
    itself at every pad and misalignment (so the comparison above is of its reads, not of
    the exact scan's)."""
    _, _, hr = rulesets
    for kind, m in enumerate(G.MEMBERS):
        if m.startswith(('"k\\', '"s\\', '"n":nul0', '"t":truE')):
            continue
        for pad in (0, 13, 29, 30, 31, 61, 62, 63, 100, 127):
            for mis in (0, 1, 15):
                d = G.doc(kind, pad, tail=pad)
                tl, _, lres, _ = H.eval_lean(hr, d, mis=mis)
                assert tl >= 0, (d, mis)
