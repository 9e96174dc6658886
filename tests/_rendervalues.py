"""TEST-ONLY: the cases and checks tests/test_render_values_host.py (host build) and
tests/test_gpu_render_values.py (the kernel) share. Inputs come from tests/render_gen.py,
render inputs from the oracle (_rendertest.oracle_values), and every expected byte from the
Python mirror (_rendertest.mirror) or, where the mirror cannot say it (bytes that are not
UTF-8 pass through STRING / SPRINT), from the case's own construction. Nothing is compared
with another run of the code under test.

A check takes `render(outputs, n_slots, docs, values, text, out_stride) -> (records
u32[n][n_outputs][3] with the status masked to its byte, out_text u8[n + 1][out_stride])`:
the slots pre-filled with 0xA5, one guard row after the batch. Not product code."""
from __future__ import annotations

import functools
import json
import random
from collections import namedtuple

import numpy as np

import _rendertest as T
import render_gen as G
from authorino_amd import response as R

GUARD = 0xA5
OK, UNRENDERED = R.RENDER_OK, R.RENDER_UNRENDERED
SEEDS = (3101, 3102, 3103)
DOCS_PER_SEED = 400

Case = namedtuple("Case", "outputs n_slots docs vals text want stride")


def _up16(n: int) -> int:
    return max(16, (n + 15) // 16 * 16)


def host_render(L=None):
    """render() over the host build: the tree's library, or one loaded by _rendertest.load."""
    def render(outputs, n_slots, docs, vals, text, out_stride):
        prog = T.HostProgram(outputs, n_slots, L)
        assert prog.rc == 0, prog.error
        slots = np.full((len(docs) + 1, out_stride), GUARD, dtype=np.uint8)
        return T.host_render(prog, docs, vals, text, out_stride, out_text=slots)
    return render


def device_render(ctx):
    """render() through authjx_render_batch (the one-program kernel)."""
    def render(outputs, n_slots, docs, vals, text, out_stride):
        prog = ctx.compile_render(outputs, n_slots)
        arena, offs, lens = T.pack(docs)
        slots = np.full((len(docs) + 1, out_stride), GUARD, dtype=np.uint8)
        return ctx.render_host_arena(prog, arena, offs, lens, vals, text, out_text=slots)
    return render


def _case(outputs, n_slots, docs, paths, text_stride=16):
    vals, text = T.oracle_values(docs, paths, text_stride=text_stride)
    want = [[w.encode("utf-8") for w in T.mirror(outputs, d, vals[r], text[r])] for r, d in enumerate(docs)]
    return Case(outputs, n_slots, docs, vals, text, want, _up16(max(sum(len(w) for w in row) for row in want)))


@functools.lru_cache(maxsize=None)
def corpus(seed: int, n: int = DOCS_PER_SEED) -> Case:
    """n generated documents, their values from the oracle and the mirror's bytes of every
    slot under every op; stride: the least multiple of 16 that holds every request's text."""
    return _case(G.OUTPUTS, G.N_SLOTS, G.corpus(random.Random(seed), n), G.PATHS)


def prefix(c: Case, n: int) -> Case:
    return Case(c.outputs, c.n_slots, c.docs[:n], c.vals[:n], None if c.text is None else c.text[:n], c.want[:n],
                c.stride)


def _is_marshal(ops) -> bool:
    return any(op == R.R_MARSHAL for op, _ in ops)


# ---- the two rules an output is judged by ----
def check_exact(c: Case, rec, out, stride=None):
    """Ample stride: every output OK, byte-equal, packed back to back; nothing written past
    the dword that holds the request's last byte; the row after the batch untouched."""
    stride = c.stride if stride is None else stride
    n = len(c.docs)
    assert rec.shape[:2] == (n, len(c.outputs)) and out.shape == (n + 1, stride)
    for r in range(n):
        pos = 0
        for k, w in enumerate(c.want[r]):
            st, got = T.rendered(rec, out, r, k)
            assert st == OK, ("declined", r, k, c.outputs[k], c.docs[r])
            assert got == w, (r, k, c.outputs[k], got, w, c.docs[r])
            assert int(rec[r, k, 0]) == pos, (r, k)
            pos += len(w)
        assert pos <= stride
        # (a MARSHAL that met an Inf took its text back: the blocks it had stored stay, inside the slot)
        if not any(w == b"" and _is_marshal(ops) for w, ops in zip(c.want[r], c.outputs)):
            assert (out[r, (pos + 3) // 4 * 4:] == GUARD).all(), ("written past the end", r)
    assert (out[n] == GUARD).all(), "the slot after the batch"
    return n * len(c.outputs)


def check_fill(c: Case, rec, out, stride: int):
    """Any stride: an output is OK at the expected start exactly when the mirror's bytes fit
    the room left, else UNRENDERED with length 0, and the outputs after it are still right.
    The one allowed deviation: a MARSHAL output the mirror gives as "" (an Inf below it) may
    be UNRENDERED. Returns (outputs that did not fit, such deviations)."""
    n = len(c.docs)
    assert out.shape == (n + 1, stride)
    unfit = inf_unrendered = 0
    for r in range(n):
        pos, clean = 0, True
        for k, w in enumerate(c.want[r]):
            st, got = T.rendered(rec, out, r, k)
            if pos + len(w) > stride:
                assert (st, got) == (UNRENDERED, b""), (stride, r, k, st, got, w)
                unfit += 1
                clean = False
            elif w == b"" and _is_marshal(c.outputs[k]) and st == UNRENDERED:
                assert int(rec[r, k, 1]) == 0
                inf_unrendered += 1
                clean = False
            else:
                assert (st, got) == (OK, w), (stride, r, k, st, got, w, c.docs[r])
                assert int(rec[r, k, 0]) == pos, (stride, r, k)
                pos += len(w)
                clean = clean and not (w == b"" and _is_marshal(c.outputs[k]))
        if clean:  # (after an output that took its text back the bytes above the position are unspecified)
            assert (out[r, (pos + 3) // 4 * 4:] == GUARD).all(), (stride, r)
    assert (out[n] == GUARD).all(), "the slot after the batch"
    return unfit, inf_unrendered


def fill_expected(c: Case, rec, stride: int):
    """The (status, bytes) rows check_fill accepted (the case file of san_render)."""
    rows = []
    for r in range(len(c.docs)):
        pos, row = 0, []
        for k, w in enumerate(c.want[r]):
            if pos + len(w) > stride or int(rec[r, k, 2]) == UNRENDERED:
                row.append((UNRENDERED, b""))
            else:
                row.append((OK, w))
                pos += len(w)
        rows.append(row)
    return rows


# ---- the checks ----
def check_corpus(render, seeds=SEEDS, n=DOCS_PER_SEED):
    total = 0
    for seed in seeds:
        c = corpus(seed, n)
        rec, out = render(c.outputs, c.n_slots, c.docs, c.vals, c.text, c.stride)
        total += check_exact(c, rec, out)
    return total


def check_fill_levels(render, seeds=SEEDS, n=DOCS_PER_SEED, strides=(16, 64, 256)):
    """{stride: (outputs, did not fit, Inf given as UNRENDERED)}; at the ample stride every
    Inf is OK-empty (check_exact)."""
    counts = {}
    for stride in strides:
        tot = unfit = inf = 0
        for seed in seeds:
            c = corpus(seed, n)
            rec, out = render(c.outputs, c.n_slots, c.docs, c.vals, c.text, stride)
            u, i = check_fill(c, rec, out, stride)
            tot, unfit, inf = tot + len(c.docs) * len(c.outputs), unfit + u, inf + i
        counts[stride] = (tot, unfit, inf)
    return counts


@functools.lru_cache(maxsize=None)
def depth_case(n: int = 257) -> Case:
    """The depth profile: request i holds exactly 1 + (5 i mod 8) levels under SPRINT and
    MARSHAL, so the lanes of a wave sit at every level of their stacks at once."""
    return _case(G.DEPTH_OUTPUTS, 1, [G.depth_doc(i) for i in range(n)], G.DEPTH_PATHS)


def check_depth_profile(render):
    c = depth_case()
    assert {G.nesting(d) - 2 for d in c.docs[:64]} == set(range(1, G.MAX_DEPTH + 1))
    rec, out = render(c.outputs, c.n_slots, c.docs, c.vals, c.text, c.stride)
    return check_exact(c, rec, out)


LONG_OUTPUTS = [[(R.R_LIT, b"v="), (op, 0)] for op in G.OPS]


@functools.lru_cache(maxsize=None)
def long_case(seed: int = 3301, n: int = 130) -> Case:
    """Strings of 200 to about 3,000 bytes, LIT + each op in one program; the stride is the
    mirror's longest request rounded up to a multiple of 16."""
    return _case(LONG_OUTPUTS, 1, G.long_docs(random.Random(seed), n), ["x.k0"])


def check_long_strings(render):
    c = long_case()
    assert max(len(d) for d in c.docs) > 2500 and c.stride > 4096
    rec, out = render(c.outputs, c.n_slots, c.docs, c.vals, c.text, c.stride)
    return check_exact(c, rec, out)


COUNTS = (0, 7, 10, 100, 999999, 1000000, 1234500, 20000000, 4294967295)


@functools.lru_cache(maxsize=None)
def counts_case() -> Case:
    """Element counts (a `#` path part) fed directly: (count, 0, NUMBER | VAL_COUNT << 8)."""
    outputs = [[(op, s)] for s in range(len(COUNTS)) for op in G.OPS]
    vals = np.array([[(x, 0, R.NUMBER | R.VAL_COUNT << 8) for x in COUNTS]], dtype=np.uint32)
    want = [[w.encode() for w in T.mirror(outputs, b"{}", vals[0], None)]]
    return Case(outputs, len(COUNTS), [b"{}"], vals, None, want, 512)


def check_counts(render):
    c = counts_case()
    # (what the mirror must say of two of them, so that the table is not judged by itself alone)
    assert c.want[0][4 * 5:4 * 5 + 4] == [b"1000000", b"1000000", b"1e+06", b"1000000"]
    assert c.want[0][4 * 6 + 2] == b"1.2345e+06" and c.want[0][4 * 8 + 2] == b"4.294967295e+09"
    rec, out = render(c.outputs, c.n_slots, c.docs, c.vals, c.text, c.stride)
    return check_exact(c, rec, out)


# utf8.DecodeRune's rejections and their valid neighbours
UTF8_INVALID = [b"\x80", b"\xbf", b"\xc0\x80", b"\xc1\xbf", b"\xc2", b"\xc2\x41", b"\xe0\x80\x80", b"\xe0\x9f\xbf",
                b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xe2\x82", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf",
                b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf0\x9f\x98", b"\xff", b"\xfe"]
UTF8_VALID = [b"\xc2\x80", b"\xdf\xbf", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xef\xbf\xbf",
              b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf"]
UTF8_OUTPUTS = [[(op, 0)] for op in G.OPS]
# placement: (the document's value around the string body, SPRINT's text around it)
_PLACES = [(b'"%s"', b"%s"), (b'["%s"]', b"[%s]"), (b'{"k":"%s"}', b"map[k:%s]"), (b'{"%s":1}', b"map[%s:1]")]


@functools.lru_cache(maxsize=None)
def utf8_table():
    """(Case, valid[r]): each sequence behind "" / "a" and before "" / "z", as a scalar, an
    array element, an object value and an object's only key. STRING / SPRINT: the bytes
    pass through (expected from the case itself; the mirror's too where they are UTF-8).
    STRING_ESC / MARSHAL: the mirror's where they are UTF-8, else UNRENDERED (None)."""
    docs, direct, valid = [], [], []
    for seq in UTF8_INVALID + UTF8_VALID:
        for pre in (b"", b"a"):
            for suf in (b"", b"z"):
                body = pre + seq + suf
                for k, (place, sprint) in enumerate(_PLACES):
                    v = place % body
                    docs.append(b'{"v":' + v + b"}")
                    direct.append((body if k == 0 else v, sprint % body))
                    valid.append(seq in UTF8_VALID)
    vals, text = T.oracle_values(docs, ["v"], text_stride=16)
    want = []
    for r, d in enumerate(docs):
        if valid[r]:
            m = [w.encode("utf-8") for w in T.mirror(UTF8_OUTPUTS, d, vals[r], None)]
            assert (m[0], m[2]) == direct[r], (d, m)
            want.append(m)
        else:
            want.append([direct[r][0], None, direct[r][1], None])
    return Case(UTF8_OUTPUTS, 1, docs, vals, None, want, 64), valid


def check_utf8_table(render):
    c, valid = utf8_table()
    assert len(c.docs) == (len(UTF8_INVALID) + len(UTF8_VALID)) * 16
    rec, out = render(c.outputs, c.n_slots, c.docs, c.vals, c.text, c.stride)
    declined = 0
    for r in range(len(c.docs)):
        pos = 0
        for k, w in enumerate(c.want[r]):
            st, got = T.rendered(rec, out, r, k)
            if w is None:
                assert (st, got) == (UNRENDERED, b""), ("not declined", c.docs[r], k, got)
                declined += 1
            else:
                assert (st, got) == (OK, w), (c.docs[r], k, st, got, w)
                assert int(rec[r, k, 0]) == pos
                pos += len(w)
    assert (out[len(c.docs)] == GUARD).all()
    assert declined == 2 * 16 * len(UTF8_INVALID)
    return declined


# ---- built text: modifier chains and "#." lists in the request's text slot ----
BUILT_SEEDS = (3203, 3202, 3201)  # (the first: the one seed the kernel and the mutants run)
BUILT_DOCS = 300
BUILT_TEXT_STRIDE = 4096


def _is_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@functools.lru_cache(maxsize=None)
def built_case(seed: int, n: int = BUILT_DOCS) -> Case:
    """n documents of tests/test_modifiers.py's _doc with a list "l" of {"k": V} / {"j": V}
    members over generated numbers, strings and small containers; six of its _chain
    selectors and the lists l.#.k, l.#.j as the eight slots, each under the four ops."""
    import pyoracle as O
    from test_modifiers import _chain, _doc

    rng = random.Random(seed)
    docs = []
    for _ in range(n):
        items = []
        for _ in range(rng.randrange(0, 6)):
            ks = rng.choice([("k",), ("j",), ("k", "j"), ("j", "k")])
            items.append(b"{" + b",".join(b'"%s":%s' % (k.encode(), G.value(rng, rng.randrange(2))) for k in ks) + b"}")
        docs.append(_doc(rng)[:-1] + b',"l":[' + b",".join(items) + b"]}")
    paths = []
    while len(paths) < 6:
        sel = _chain(rng)
        try:
            O.gjson_get_mods(docs[0], sel)
        except ValueError:  # (a form neither side compiles)
            continue
        paths.append(sel)
    paths += ["l.#.k", "l.#.j"]
    return _case(G.OUTPUTS, G.N_SLOTS, docs, paths, text_stride=BUILT_TEXT_STRIDE)


def check_built(render, seeds=BUILT_SEEDS):
    """Every decided output equals the mirror. A slot of type 255 declines; a supported
    value declines only under STRING_ESC / MARSHAL and only when its bytes are not UTF-8
    (then it must). Returns (outputs, from the text slot, declined as not UTF-8, of type 255)."""
    tot = from_text = not_utf8 = unsupported = 0
    for seed in seeds:
        c = built_case(seed)
        rec, out = render(c.outputs, c.n_slots, c.docs, c.vals, c.text, c.stride)
        for r, doc in enumerate(c.docs):
            pos = 0
            for k, ops in enumerate(c.outputs):
                op, slot = ops[-1]
                s0, ln, t = (int(x) for x in c.vals[r, slot])
                st, got = T.rendered(rec, out, r, k)
                tot += 1
                from_text += bool((t >> 8) & R.VAL_TEXT)
                if (t & 0xFF) == 255:
                    assert (st, got) == (UNRENDERED, b""), (seed, r, k)
                    unsupported += 1
                    continue
                src = c.text[r].tobytes() if (t >> 8) & R.VAL_TEXT else doc
                utf8 = _is_utf8(src[s0:s0 + ln])  # (an escape never unescapes to bytes that are not UTF-8)
                if not utf8 and op in (R.R_STRING_ESC, R.R_MARSHAL):
                    assert (st, got) == (UNRENDERED, b""), (seed, r, k, src[s0:s0 + ln])
                    not_utf8 += 1
                    continue
                assert st == OK, ("declined", seed, r, k, ops, src[s0:s0 + ln])
                if utf8:
                    assert got == c.want[r][k], (seed, r, k, got, c.want[r][k])
                else:  # bytes pass through; the mirror's str has U+FFFD for them
                    assert got.decode("utf-8", "replace") == c.want[r][k].decode("utf-8"), (seed, r, k, got)
                    if op == R.R_STRING and (t & 0xFF) == R.STRING:
                        raw = src[s0 + 1:s0 + ln - 1]
                        assert got == b"v=" + (R.gjson_unescape(raw) if b"\\" in raw else raw), (seed, r, k)
                assert int(rec[r, k, 0]) == pos, (seed, r, k)
                pos += len(got)
        assert (out[len(c.docs)] == GUARD).all()
    return tot, from_text, not_utf8, unsupported


# ---- the expected side judged from outside, for what Python can judge ----
def _sig_digits(s: str) -> int:
    m = s.lower().lstrip("+-").partition("e")[0].replace(".", "").lstrip("0").rstrip("0")
    return max(len(m), 1)


def _no_surrogates(v) -> bool:
    if isinstance(v, str):
        return not any(0xD800 <= ord(ch) <= 0xDFFF for ch in v)
    if isinstance(v, dict):
        return all(_no_surrogates(k) and _no_surrogates(x) for k, x in v.items())
    if isinstance(v, list):
        return all(_no_surrogates(x) for x in v)
    return True


def _ordered(pairs):
    keys = [k.encode("utf-8") for k, _ in pairs]
    assert all(a < b for a, b in zip(keys, keys[1:])), ("object keys out of bytewise order", keys)
    return dict(pairs)


def check_outside(seeds=SEEDS, n=DOCS_PER_SEED):
    """The mirror's bytes against Python's own json and float: (containers judged, numbers
    judged)."""
    containers = numbers = 0
    for seed in seeds:
        c = corpus(seed, n)
        for r, doc in enumerate(c.docs):
            for k, ops in enumerate(c.outputs):
                op, slot = ops[-1]
                if op not in (R.R_SPRINT, R.R_MARSHAL):
                    continue
                s0, ln, t = (int(x) for x in c.vals[r, slot])
                raw, w = doc[s0:s0 + ln].decode("utf-8"), c.want[r][k].decode("utf-8")
                if (t & 0xFF) == R.JSON and op == R.R_MARSHAL and w:
                    ref = json.loads(raw, parse_int=float)  # (a dict: the last duplicate wins)
                    if not _no_surrogates(ref):  # (Python keeps a lone surrogate, Go writes U+FFFD)
                        continue
                    assert json.loads(w, parse_int=float, object_pairs_hook=_ordered) == ref, (raw, w)
                    containers += 1
                elif (t & 0xFF) == R.NUMBER and float(raw) - float(raw) == 0:
                    assert float(w) == float(raw), (raw, w)
                    assert _sig_digits(w) == _sig_digits(repr(float(raw))), (raw, w)
                    numbers += 1
    return containers, numbers
