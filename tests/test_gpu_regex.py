"""GPU: `matches` through every DFA walker and on both sides of the staging limits, against
the oracle (tri-state, error index, T bitmap; no UNDECIDED where the product compiles the
pattern).

The table of generated patterns (tests/regex_gen.py; tests/test_regex_values_host.py runs
the same rulesets and documents on the host build) through each kernel at small shapes; the
16-byte step of dfa_match_span with a multi-byte, invalid or truncated sequence at every
offset of it; rulesets whose blob is under and over kMaxSharedBlobBytes and whose hot prefix
fits, shares or overflows the tenant kernel's staging region (each case's side of the limit
asserted on the host build of the compiler); and patterns over kMaxDfaStates and
kMaxDfaClasses, which are UNDECIDED and never a guess."""
import numpy as np
import pytest

import _hosttest as H
import pyoracle as O
import regex_gen as G
from test_regex_diff import AB11, many_classes

pytestmark = pytest.mark.gpu

SHARED_BLOB = 48 * 1024   # ajx::kMaxSharedBlobBytes
TENANT_STAGE = 16 * 1024  # ajx::kMaxTenantStageBytes; launch_tenant stages into 256 bytes less
TENANT_REGION = TENANT_STAGE - 256
TENANT_BLOCK = 512        # requests of a tenant workgroup


@pytest.fixture(scope="module")
def ctx():
    from authorino_amd import runtime

    c = runtime.Context(0)
    yield c
    c.set_kernel_mode(0)


class _Set:
    """One ruleset on the device, with the oracle's answers for its documents."""

    def __init__(self, ctx, pats, nodes, root, docs, may_be_unsupported=False):
        self.spec = (pats, nodes, root)
        self.docs = docs
        self.dev = ctx.compile(pats, nodes, root)
        assert may_be_unsupported or not any(self.dev.status), self.dev.status
        self.orc = O.Ruleset(pats, nodes, root)
        arena, offs, lens = G.pack(docs)
        self.tri, self.err, self.bm = O.eval_batch([self.orc], arena, offs, lens)

    def host(self):
        hr = H.HostRuleset(*self.spec)
        assert hr.rc == 0, hr.error
        return hr


@pytest.fixture(scope="module")
def table(ctx):
    return [_Set(ctx, *spec) for spec in G.table_rulesets()]


def _eval(ctx, sets, picks, mode, words=1):
    """picks: [(set index, document index)], one request each, evaluated under `mode` in one
    batch; returns (device outputs, oracle outputs) — the oracle's taken from each set's table."""
    docs = [sets[s].docs[d] for s, d in picks]
    arena, offs, lens = G.pack(docs)
    sor = None if len(sets) == 1 else np.array([s for s, _ in picks], dtype=np.uint32)
    ctx.set_kernel_mode(mode)
    try:
        got = ctx.eval_host_arena([s.dev for s in sets], arena, offs, lens, set_of_req=sor)
    finally:
        ctx.set_kernel_mode(0)
    want = (np.array([sets[s].tri[d] for s, d in picks], dtype=np.uint8),
            np.array([sets[s].err[d] for s, d in picks], dtype=np.int32),
            np.array([sets[s].bm[d] for s, d in picks], dtype=np.uint64).reshape(len(picks), -1))
    return got, want


def _same(got, want, undecided_ok=False):
    (tri, err, bm), (otri, oerr, obm) = got, want
    bad = np.nonzero(tri != otri)[0]
    assert bad.size == 0, (bad[:8], tri[bad[:8]], otri[bad[:8]])
    assert np.array_equal(err, oerr), np.nonzero(err != oerr)[0][:8]
    assert np.array_equal(bm[:, :obm.shape[1]], obm), np.nonzero((bm[:, :obm.shape[1]] != obm).any(axis=1))[0][:8]
    assert not bm[:, obm.shape[1]:].any()
    assert undecided_ok or not (tri == 3).any()


@pytest.mark.parametrize("mode,n", [(0, 1), (0, 64), (0, 65), (0, 2049), (41, 65), (41, 396), (52, 396)],
                         ids=["stream-1", "stream-64", "stream-65", "stream-2049-two-per-wave", "lean-65", "lean-396",
                              "stream-32-per-wave-396"])
def test_table_each_ruleset_alone(ctx, table, mode, n):
    """Mode 0: the streaming kernel and its in-kernel stage B on the LDS copy (n <= 2048: one
    request per wave; 2049: two, and the finish kernel); 41: the lean kernel; 52: the streaming
    kernel at 32 requests per wave."""
    for k, s in enumerate(table):
        assert len(s.docs) >= 396
        # (n = 1: a string with \u escapes, not always document 0's raw one)
        picks = [(0, (j + (2 * k + 1 if n == 1 else 0)) % len(s.docs)) for j in range(n)]
        _same(*_eval(ctx, [s], picks, mode))


def test_table_all_rulesets_multi_tenant_stream(ctx, table):
    """Mode 0, 396 requests over all rulesets: the multi-tenant stream, one request per wave."""
    picks = [(j % len(table), (7 * j) % len(table[j % len(table)].docs)) for j in range(396)]
    picks.sort(key=lambda p: p[0])
    _same(*_eval(ctx, table, picks, 0))


def test_table_all_rulesets_tenant_kernel(ctx, table):
    """Mode 40, about 1,500 requests in runs of 1 to 200 of one ruleset each: the tenant kernel,
    with waves of one staged ruleset (the lean scan on its LDS copy) and waves of several (the
    token scanner)."""
    rng = np.random.default_rng(9)
    picks = []
    while len(picks) < 1500:
        s = int(rng.integers(0, len(table)))
        run = int(rng.choice([1, 2, 5, 30, 64, 100, 200]))
        d0 = int(rng.integers(0, len(table[s].docs)))
        picks += [(s, (d0 + j) % len(table[s].docs)) for j in range(run)]
    sor = np.array([s for s, _ in picks])
    starts = np.nonzero(np.diff(sor))[0] + 1
    waves = sor[: len(sor) // 64 * 64].reshape(-1, 64)
    uniform = (waves == waves[:, :1]).all(axis=1)
    assert uniform.sum() >= 4 and (~uniform).sum() >= 4, "both kinds of wave"
    assert len(starts) >= 12
    _same(*_eval(ctx, table, picks, 40))


# --- the 16-byte step of dfa_match_span
SPAN_PATS = [("v", 5, "^[a-zé€\\x{10000}-\\x{10FFFF}]+$"), ("v", 5, "€$"), ("w", 1, "z")]
SPAN_SEQS = ["é".encode(), "€".encode(), "\U00010000".encode(),  # 2, 3 and 4 bytes
             b"\xff", b"\xc3", b"\xe2\x82", b"\xf0\x90\x80"]     # invalid, and three cut short
SPAN_LENS = [16, 17, 19, 32, 33, 48, 50]


def _span_docs():
    docs, at_end = [], 0
    for n in SPAN_LENS:
        for off in range(19):
            for q in SPAN_SEQS:
                if off + len(q) > n:
                    continue
                body = bytes(97 + (off + j) % 26 for j in range(n - len(q)))
                text = body[:off] + q + body[off:]
                assert len(text) == n
                at_end += off + len(q) == n and q == b"\xe2\x82"
                for pad in range(4):  # (four consecutive paddings: every alignment of the string mod 4)
                    docs.append(G.document(b'"' + text + b'"', pad, b"y"))
    assert at_end >= 3, "a 3-byte rune cut short at the string's end"
    return docs


@pytest.mark.parametrize("mode", [41, 0], ids=["lean", "stream"])
def test_span_step_every_offset(ctx, mode):
    """Strings of 16 to 50 bytes (a whole number of 16-byte steps among them) with one rune of
    2, 3 or 4 bytes, an invalid byte or a sequence cut short at every byte offset 0..18 (inside
    the first step, across its end, in the second), at every alignment mod 4 (dfa_match_span's
    shift, with and without its fifth dword)."""
    nodes, root = G.chain_any(len(SPAN_PATS))
    docs = _span_docs()
    assert 3000 < len(docs) <= 4096  # (mode 0: the streaming kernel takes up to 4096)
    s = _Set(ctx, SPAN_PATS, nodes, root, docs)
    arena, offs, lens = G.pack(docs)
    align = {int(offs[j] + docs[j].index(b'"v":"') + 5) & 3 for j in range(len(docs))}
    assert align == {0, 1, 2, 3}
    assert 0 < int((s.bm[:, 0] & 1).sum()) < len(docs) and 0 < int((s.bm[:, 0] & 2).sum()) < len(docs)
    _same(*_eval(ctx, [s], [(0, j) for j in range(len(docs))], mode))


# --- staging limits
def _big(letters, k):
    a, b = letters
    return "[%s]*%s[%s]{%d}$" % (letters, a, letters, k)


def _big_docs(rng, letters, n):
    """v and w: strings over `letters` of 9 to 14 bytes (deep states of the big DFAs)."""
    out = []
    for j in range(n):
        v, w = ("".join(rng.choice(list(letters), size=int(rng.integers(9, 15)))) for _ in range(2))
        out.append(b'{"pad":"%s","v":"%s","w":"%s"}' % (b"p" * (j % 16), v.encode(), w.encode()))
    return out


def _big_set(ctx, rng, pats, letters="ab", n=130):
    nodes, root = G.chain_any(len(pats))
    s = _Set(ctx, pats, nodes, root, _big_docs(rng, letters, n))
    for p in range(len(pats)):
        if pats[p][1] == 5:
            hits = int(((s.bm[:, 0] >> np.uint64(p)) & np.uint64(1)).sum())
            assert 0 < hits < n, (pats[p], hits)
    return s


@pytest.mark.parametrize("n_dfa", [2, 3])
def test_blob_under_and_over_the_lds_limit(ctx, n_dfa):
    """Two 2053-state DFAs: a blob just under kMaxSharedBlobBytes, staged in LDS, taken by the
    streaming kernel. Three: over it, so the lean kernel reads its tables from global memory
    (its SHARED = false instance) and the ruleset does not stream: a batch of one request takes
    the lean kernel too. Neither may simply hand its requests to the exact scan."""
    rng = np.random.default_rng(17)
    pats = [("v", 5, _big("ab", 10)), ("w", 5, _big("ba", 10)), ("v", 5, "[ab]*a[ab]{9}a$")][:n_dfa]
    s = _big_set(ctx, rng, pats)
    hr = s.host()
    print(f"{n_dfa} DFAs: blob {hr.blob_size} B, hot {hr.blob_hot_bytes} B")
    assert (hr.blob_size <= SHARED_BLOB) == (n_dfa == 2)
    # the plan for a batch of one request (a ruleset streams only while its blob fits LDS,
    # stream_eligible in csrc/ajx_kernels.hip): Path 1 the stream, 2 the lean kernel
    plan = H.plan_eval(n=1, n_sets=1, all_stream=int(hr.blob_size <= SHARED_BLOB), max_blob=hr.blob_size,
                       stream_max_n=4096, bitmap=1)
    assert (plan["path"], plan["stage_bytes"] != 0) == ((1, False) if n_dfa == 2 else (2, False))
    for mode, n in [(0, 1), (0, 65), (41, 65)]:
        picks = [(0, j) for j in range(n)]
        if n == 1:
            picks = [(0, 3)]
        _same(*_eval(ctx, [s], picks, mode))
        assert ctx.last_exact_count() == 0, (mode, n, ctx.last_exact_count())


def test_tenant_staging_region_fits_shares_overflows(ctx, table):
    """Mode 40, 1,500 requests in runs of 100 to 300 over four kinds of ruleset: A, two table
    patterns (under 2 KiB); B, one 1029-state DFA, whose hot prefix fits the staging region
    alone; C, another of B's kind, which does not fit next to B; D, two such DFAs, which never
    fit. Workgroups of 512 requests see A + B + C (C's waves read global memory), B + D, and
    two rulesets of D's kind alone (nothing staged)."""
    rng = np.random.default_rng(23)
    pats, _, _, docs = G.table_rulesets()[0]
    pats = pats[:2] + pats[-1:]
    a = _Set(ctx, pats, *G.chain_any(len(pats)), docs)
    b =_big_set(ctx, rng, [("v", 5, _big("ab", 9)), ("w", 1, "z")], n=300)
    c = _big_set(ctx, rng, [("v", 5, _big("cd", 9)), ("w", 1, "z")], "cd", n=300)
    d = _big_set(ctx, rng, [("v", 5, _big("ab", 9)), ("w", 5, _big("ba", 9))], n=300)
    d2 = _big_set(ctx, rng, [("v", 5, _big("ba", 9)), ("w", 5, _big("ab", 9))], n=300)
    ha, hb, hc, hd, hd2 = (x.host().blob_hot_bytes for x in (a, b, c, d, d2))
    print(f"hot bytes: A {ha}, B {hb}, C {hc}, D {hd}, D' {hd2}; region {TENANT_REGION}")
    assert ha + hb <= TENANT_REGION, "A and B are staged together"
    assert hb + hc > TENANT_STAGE, "C does not fit next to B"
    assert hd > TENANT_STAGE and hd2 > TENANT_STAGE, "D never fits"
    sets = [a, b, c, d, d2]
    runs = [(0, 100), (1, 200), (2, 212),  # workgroup 0: A + B + C
            (1, 212), (3, 300),            # workgroup 1: B + D
            (4, 250), (3, 226)]            # workgroup 2: D' + D
    assert [sum(n for _, n in runs[:k]) for k in (3, 5)] == [TENANT_BLOCK, 2 * TENANT_BLOCK]
    picks = [(s, j % len(sets[s].docs)) for s, n in runs for j in range(n)]
    assert len(picks) == 1500
    _same(*_eval(ctx, sets, picks, 40))


# --- over the limits
def _over_limit(ctx, pat, mode, eq_first):
    """68 requests, (v matches, v does not) x (w == "z", another w), under Any of `v matches
    pat` and `w eq "z"` in either order: (tri, bit of the eq pattern, index of the regex)."""
    pats = [("v", 5, pat), ("w", 1, "z")]
    if eq_first:
        pats.reverse()
    nodes, root = G.chain_any(2)
    hit = "b" * 5 + "a" + "b" * 11 if pat == AB11 else "x" + pat
    docs = [('{"v":"%s","w":"%s"}' % (v, w)).encode() for v in (hit, "bbbb") for w in ("z", "q")] * 17
    s = _Set(ctx, pats, nodes, root, docs, may_be_unsupported=True)
    rx = 1 if eq_first else 0
    assert s.dev.status[rx] == 2 and s.dev.status[1 - rx] == 0
    assert s.tri[:4].tolist() == [1, 1, 1, 0], "the oracle decides every one"
    (tri, err, bm), _ = _eval(ctx, [s], [(0, j) for j in range(len(docs))], mode)
    assert not ((bm[:, 0] >> np.uint64(rx)) & np.uint64(1)).any(), "an unsupported pattern is never T"
    assert ((bm[:, 0] >> np.uint64(1 - rx)) & np.uint64(1)).tolist() == [1, 0, 1, 0] * 17
    return tri.reshape(17, 4), err.reshape(17, 4), rx


OVER = pytest.mark.parametrize("pat", [AB11, many_classes()], ids=["states", "classes"])


@OVER
@pytest.mark.parametrize("mode", [0, 41])
def test_over_the_dfa_limits_is_undecided(ctx, pat, mode):
    """A pattern over kMaxDfaStates or kMaxDfaClasses is status 2. Under Any with `w eq "z"`, in
    either order, a request with that w is T (such a regexp compiles in Go, so it is no error
    and the compiler lets the decided operand speak first), and a request with another w is
    UNDECIDED with the pattern's index: never F, though the oracle (which builds no DFA)
    decides it, and both ways."""
    for eq_first in (False, True):
        tri, err, rx = _over_limit(ctx, pat, mode, eq_first)
        assert (tri[:, [0, 2]] == 1).all() and (err[:, [0, 2]] == -1).all(), (eq_first, tri[0], err[0])
        assert (tri[:, [1, 3]] == 3).all() and (err[:, [1, 3]] == rx).all(), (eq_first, tri[0], err[0])
