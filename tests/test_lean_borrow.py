"""CPU tests of the lean walk taking the next sub-window's tokens early (ajx_lean.h,
Walk::walk: on the device a lane whose own tokens are gone takes them while its wave's
busiest lane goes on). The host build has no wave, so the library of
tests/native/lean_borrow.mk gives each walk() call a spare budget from a policy: none (the
walk of a lane alone), 1, 2 or 3 iterations, unlimited, or a random 0..4 per call. Whatever
the policy, a document must give the same tri-state, error index, per-pattern results,
capture row and eager `dec` words, and must go to the exact scan under every policy or
under none; policy 0's results are compared with the oracle."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import _hosttest as H
import fuzz_util as FU
import lean_borrow_gen as B
import lean_reads_gen as G
import pyoracle as O

_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
POLICIES = [(1, 1, 0), (1, 2, 0), (1, 3, 0), (2, 0, 0)] + [(3, 0, s) for s in (1, 2, 3, 4, 5)]


@pytest.fixture(scope="module", autouse=True)
def borrow_lib():
    """The harness with the spare-budget setters, in place of _hosttest's library for this
    module (the same sources plus lean_borrow_host.cpp)."""
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "lean_borrow.mk", "libajx_leanborrow.so"], check=True)
    old = H._L
    H._L = None
    os.environ["AJX_HOSTTEST_LIB"] = os.path.join(_NATIVE, "libajx_leanborrow.so")
    try:
        lib = H.lib()
    finally:
        del os.environ["AJX_HOSTTEST_LIB"]
    lib.ht_lean_spare.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    lib.ht_lean_spare.restype = None
    lib.ht_lean_early.restype = C.c_uint64
    lib.ht_lean_counts.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ht_lean_counts.restype = None
    yield lib
    lib.ht_lean_spare(0, 0, 0)
    H.lean_keep(True)
    gc.collect()  # (this module's rulesets are freed by the library that made them)
    H._L = old


def _scan(hr, d, mis, n_sel):
    t, e, res, row = H.eval_lean(hr, d, mis=mis, n_sel=n_sel)
    return (t, e, res, row, H.lean_last_dec()) if t >= 0 else (t,)


class Tally:
    def __init__(self):
        self.n = self.lean = self.early = 0


def check(lib, hr, rs, d, mis, n_sel, tally, n_pat=None, full=True):
    """d at misalignment mis under every policy; policy 0 against the oracle. full False:
    a document the oracle may call unsupported / the exact scan may own (fuzz)."""
    lib.ht_lean_spare(0, 0, 0)
    e0 = lib.ht_lean_early()
    base = _scan(hr, d, mis, n_sel)
    assert lib.ht_lean_early() == e0  # (policy 0 takes nothing early)
    tally.n += 1
    if base[0] >= 0:
        tally.lean += 1
        n_pat = n_pat if n_pat is not None else len(base[2])
        ot = [rs.pattern(p, d) for p in range(n_pat)]
        if full or (O.UNSUPPORTED not in ot and 3 not in base[2]):
            assert base[2][:n_pat] == ot, (d, mis)
    for pol in POLICIES:
        lib.ht_lean_spare(*pol)
        got = _scan(hr, d, mis, n_sel)
        assert got == base, (pol, mis, d, got, base)
    tally.early += lib.ht_lean_early() - e0
    lib.ht_lean_spare(0, 0, 0)
    return base


@pytest.fixture(params=[True, False], ids=["keep_rows", "needed_rows"])
def keep(request, borrow_lib):
    H.lean_keep(request.param)
    yield request.param
    H.lean_keep(True)


@pytest.mark.parametrize("workload", ["c2", "c3", "c4", "c5"])
def test_workload_documents_every_policy(borrow_lib, workload, keep):
    """200 documents of each bench workload at every misalignment 0..15 (c4: its
    first tenant's ruleset on the shared documents, c5: the forest of its AuthConfig)."""
    from authorino_amd import workloads as W

    w = W.make(workload, n=200, seed=17)
    if workload == "c5":
        ac = w.auth_config
        ex = [ac.conditions] + [e for c in ac.authorization for e in (c.conditions, c.rules)]
        trees = [([(p.selector, int(p.operator), p.value) for p in pats], nodes, root)
                 for pats, nodes, root in (e.flatten() for e in ex)]
        pats = [p for t in trees for p in t[0]]
        sels = list(dict.fromkeys(p[0] for p in pats))
        if keep:
            trees.append(([(s, 1, "") for s in sels], [], -1))
        hr = H.HostRuleset.forest(trees)
        rs = O.Ruleset(pats, *FU.chain(len(pats)))
        n_pat, n_sel = len(pats), len(sels)
    else:
        hr = H.HostRuleset.with_selector_tree(w.expr) if keep else H.HostRuleset.from_expression(w.expr)
        rs = O.Ruleset.from_expression(w.expr)
        n_pat = len(w.expr.flatten()[0])
        n_sel = len({p.selector for p in w.expr.flatten()[0]})
    assert hr.rc == 0, hr.error
    tally = Tally()
    for i in range(w.n):
        d = w.doc(i)
        for mis in range(16):
            base = check(borrow_lib, hr, rs, d, mis, n_sel, tally, n_pat=n_pat, full=workload != "c5")
            assert base[0] >= 0, (i, mis)
    assert tally.early > 20 * tally.n  # (tokens taken early, summed over the policies)
    assert tally.n == 200 * 16


@pytest.mark.parametrize("arr", [False, True], ids=["no_array_selector", "array_selector"])
def test_member_kinds_at_every_ring_offset(borrow_lib, arr):
    """tests/lean_reads_gen.py's members at every pad 0..127 (every ring offset), the
    misalignment in rotation."""
    pats = G.patterns(arr)
    nodes, root = G.chain(len(pats))
    rs, hr = O.Ruleset(pats, nodes, root), H.HostRuleset(pats, nodes, root)
    tally = Tally()
    for k, d in enumerate(G.sweep()):
        base = check(borrow_lib, hr, rs, d, (k * 7) % 16, 0, tally, full=False)
        if base[0] >= 0 and 3 not in base[2]:
            assert base[0] == rs.matches(d)[0], d
    assert tally.lean > 0.8 * tally.n and tally.early > 5 * tally.n


def edge_mis(k):
    """The two misalignments document k of the edge family is scanned at."""
    return ((k * 3) % 16, (k * 3 + 8) % 16)


def test_edge_family_reaches_the_positions():
    """Found in the documents, not assumed: a key's closing quote, a value's first byte, the
    structural byte that ends a scalar, a string's closing quote, an open and a close, each
    at every offset of a sub-window pair (so at 28..35, around the boundary between c and l,
    and at 60..63, l's last bytes), at the misalignments test_edge_family_every_policy scans
    each document at (edge_mis)."""
    seen = {k: set() for k in ("key", "vstart", "send", "sclose", "open", "close")}
    for k, (d, ok) in enumerate(B.edge_docs()):
        if not ok:
            continue
        at = d.find(b'",') + 2
        colon = d.find(b":", at)
        for mis in edge_mis(k):
            seen["key"].add((colon - 1 + mis) % 64)
            seen["vstart"].add((colon + 1 + mis) % 64)
            v = d[colon + 1:colon + 2]
            if v in b"-0123456789tfn":
                end = min(x for x in (d.find(b",", colon), d.find(b"}", colon)) if x >= 0)
                seen["send"].add((end + mis) % 64)
            elif v == b'"':
                seen["sclose"].add((d.find(b'"', colon + 2) + mis) % 64)
            else:
                seen["open"].add((colon + 1 + mis) % 64)
                for j in range(colon + 1, len(d)):
                    if d[j:j + 1] in b"}]":
                        seen["close"].add((j + mis) % 64)
    for k, s in seen.items():
        assert s == set(range(64)), (k, sorted(set(range(64)) - s))


@pytest.mark.parametrize("arr", [False, True], ids=["no_array_selector", "array_selector"])
def test_edge_family_every_policy(borrow_lib, arr, keep):
    pats = B.EDGE_ARR_PATS if arr else B.EDGE_PATS
    nodes, root = FU.chain(len(pats))
    rs = O.Ruleset(pats, nodes, root)
    sels = list(dict.fromkeys(p[0] for p in pats))
    hr = H.HostRuleset.forest([(pats, nodes, root), ([(s, 1, "") for s in sels], [], -1)]) if keep else \
        H.HostRuleset(pats, nodes, root)
    assert hr.rc == 0, hr.error
    tally = Tally()
    n_valid = n_valid_lean = 0
    for k, (d, ok) in enumerate(B.edge_docs()):
        for mis in edge_mis(k):
            base = check(borrow_lib, hr, rs, d, mis, len(sels) if keep else 0, tally, n_pat=len(pats), full=ok)
            if not keep and base[0] >= 0 and 3 not in base[2]:  # (keep: a forest's fold, not the chain's)
                assert base[0] == rs.matches(d)[0], (d, mis)
            n_valid += ok
            n_valid_lean += ok and base[0] >= 0
    assert n_valid_lean == n_valid  # (every unbroken document is the lean scan's own)
    assert tally.early > 5 * tally.n


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_and_mutated_documents_every_policy(borrow_lib, seed, keep):
    rng = np.random.default_rng(7100 + seed)
    tally = Tally()
    for _ in range(70):
        pats = FU.rand_patterns(rng, int(rng.integers(1, 8)))
        nodes, root = FU.chain(len(pats))
        rs = O.Ruleset(pats, nodes, root)
        hr = H.HostRuleset(pats, nodes, root)
        for _ in range(12):
            r = rng.random()
            d = FU.long_doc(rng, pats) if r < 0.25 else FU.rand_doc(rng, ws=False) if r < 0.85 else FU.rand_doc(rng)
            if rng.random() < 0.4:
                d = FU.mutate(rng, d)
            base = check(borrow_lib, hr, rs, d, int(rng.integers(0, 16)), 0, tally, full=False)
            if base[0] >= 0 and 3 not in base[2] and O.UNSUPPORTED not in [rs.pattern(p, d) for p in range(len(pats))]:
                assert base[0] == rs.matches(d)[0], (pats, d)
    assert tally.lean > 200 and tally.early > tally.n


def test_policy_zero_takes_none_early_unlimited_many(borrow_lib):
    """Policy 0 takes no token early; with an unlimited budget a good part of the tokens is
    taken early, for about the same number of iterations (a host lane never idles)."""
    from authorino_amd import workloads as W

    w = W.make("c2", n=64, seed=5)
    hr = H.HostRuleset.from_expression(w.expr)
    it, sb = C.c_uint64(), C.c_uint64()
    counts = []
    for pol in ((0, 0, 0), (2, 0, 0)):
        borrow_lib.ht_lean_spare(*pol)
        borrow_lib.ht_lean_counts(C.byref(it), C.byref(sb))
        i0, e0 = it.value, borrow_lib.ht_lean_early()
        for i in range(w.n):
            assert H.eval_lean(hr, w.doc(i), mis=i % 16)[0] >= 0
        borrow_lib.ht_lean_counts(C.byref(it), C.byref(sb))
        counts.append((it.value - i0, borrow_lib.ht_lean_early() - e0))
    borrow_lib.ht_lean_spare(0, 0, 0)
    assert counts[0][1] == 0
    # (a key taken early whose string value closes past the next sub-window goes pending: its
    # closing quote is a token of its own then, which the key's own walk would have taken
    # with the key. At most one more iteration per token taken early)
    assert counts[0][0] <= counts[1][0] <= counts[0][0] + counts[1][1]
    assert counts[1][1] > 0.3 * counts[1][0]


def test_every_policy_under_asan_ubsan():
    """tests/native/san_borrow.cpp: the same walk with its own main under AddressSanitizer
    and UBSan (no Python in the process), every policy on members at every offset, whole,
    broken and cut short; it fails on a report, on a difference from policy 0, and when no
    token was taken early."""
    subprocess.run(["make", "-s", "-C", _NATIVE, "-f", "lean_borrow.mk", "san_borrow"], check=True)
    r = subprocess.run([os.path.join(_NATIVE, "san_borrow")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "mismatches 0" in r.stdout


def _iters(lib, hr, d, mis=0):
    it, sb = C.c_uint64(), C.c_uint64()
    lib.ht_lean_counts(C.byref(it), C.byref(sb))
    i0 = it.value
    t = H.eval_lean(hr, d, mis=mis)[0]
    lib.ht_lean_counts(C.byref(it), C.byref(sb))
    return t, it.value - i0


def test_value_closing_at_the_pairs_last_byte_goes_pending(borrow_lib):
    """The two rules that keep a document's path independent of the schedule. A key's string
    value whose closing quote is the last byte of the sub-window pair goes pending (the
    bit of the colon after it belongs to the next sub-window): its closing quote is a token
    of its own, one more iteration than a value that closes a byte earlier. And a key's string
    value followed by a colon goes to the exact scan wherever its sub-windows fall, under
    every policy."""
    pats = [("k", 1, "v"), ("z", 1, "1")]
    nodes, root = FU.chain(len(pats))
    hr = H.HostRuleset(pats, nodes, root)
    borrow_lib.ht_lean_spare(0, 0, 0)
    # {"k":"<L bytes>","z":1}: the key's closing quote at byte 3, the value's at byte 6 + L
    # (root, k with its value, z with its value and the root's close: 3 iterations)
    doc = lambda n: ('{"k":"%s","z":1}' % ("s" * n)).encode()  # noqa: E731
    assert _iters(borrow_lib, hr, doc(40)) == (0, 3)
    assert _iters(borrow_lib, hr, doc(56)) == (0, 3)  # closes at byte 62
    assert _iters(borrow_lib, hr, doc(57)) == (0, 4)  # closes at byte 63: pending
    assert _iters(borrow_lib, hr, doc(58)) == (0, 4)  # closes past the pair: pending, as ever
    for pol in [(0, 0, 0)] + POLICIES:
        borrow_lib.ht_lean_spare(*pol)
        for pad in range(0, 70):
            for mis in (0, 5, 15):
                bad = ('{"pad":"%s","k":"v":"z":1}' % ("p" * pad)).encode()
                good = ('{"pad":"%s","k":"v","z":1}' % ("p" * pad)).encode()
                assert H.eval_lean(hr, bad, mis=mis)[0] == -1, (pol, pad, mis)
                assert H.eval_lean(hr, good, mis=mis)[0] >= 0, (pol, pad, mis)
    borrow_lib.ht_lean_spare(0, 0, 0)
