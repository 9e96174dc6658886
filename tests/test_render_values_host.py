"""Generated values through every render op on the CPU: the host build of
authorino_amd/csrc/ajx_render.h (tests/native/render_host.cpp) over tests/render_gen.py's
numbers, strings, keys and containers, against the Python mirror over the oracle's gjson
(tests/_rendervalues.py has the cases and checks; tests/test_gpu_render_values.py runs them
through the kernel). Every comparison is byte equality with the mirror, never with another
run of the code under test; test_mutants_are_caught shows that the checks bite."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import _rendertest as T
import _rendervalues as V
import render_gen as G
from authorino_amd import response as R


def test_generator_covers_its_classes():
    """The committed seeds reach what the file is for: every nesting depth to
    kMaxRenderDepth, whitespace inside containers, numbers of 20+ digits, every atom, long
    strings, colliding keys; the depth profile has exactly the depths it names."""
    assert T.lib().rt_max_depth() == G.MAX_DEPTH
    depths, atoms, long_, big, dup = set(), set(), 0, 0, 0
    for seed in V.SEEDS:
        c = V.corpus(seed)
        for r, doc in enumerate(c.docs):
            for s in range(G.N_SLOTS):
                s0, ln, t = (int(x) for x in c.vals[r, s])
                raw = doc[s0:s0 + ln]
                if (t & 0xFF) == R.JSON:
                    depths.add(G.nesting(raw))
                    dup += b'"a"' in raw and b'"\\u0061"' in raw
                elif (t & 0xFF) == R.STRING:
                    long_ += ln > 200
                elif (t & 0xFF) == R.NUMBER:
                    big += sum(ch in b"0123456789" for ch in raw) >= 20
            atoms.update(a for a in G.ATOMS if a in doc)
    assert depths == set(range(1, G.MAX_DEPTH + 1))
    assert len(atoms) == len(G.ATOMS) and long_ >= 30 and big >= 100 and dup >= 30
    assert [G.depth_levels(i) for i in range(8)] == [1, 6, 3, 8, 5, 2, 7, 4]
    for i in range(16):
        assert G.nesting(G.depth_doc(i)) - 2 == G.depth_levels(i)
    assert G.depth_doc(2) != G.depth_doc(10)  # (same depth, other members)


def test_corpus_equals_the_mirror():
    """1,200 documents of 8 values under the four ops at the ample stride: 0 declined,
    every output byte-equal and packed back to back, nothing written past the dword holding
    the text's end, the row after the batch untouched."""
    assert len(V.SEEDS) >= 3 and len(V.SEEDS) * V.DOCS_PER_SEED >= 1000
    total = V.check_corpus(V.host_render())
    print("corpus: %d documents, %d outputs, 0 declined" % (len(V.SEEDS) * V.DOCS_PER_SEED, total))
    assert total == len(V.SEEDS) * V.DOCS_PER_SEED * len(G.OUTPUTS)


def test_mirror_judged_by_python_json_and_float():
    """The expected side from outside: MARSHAL of a container parses (json.loads) to what the
    raw text parses to, keys in bytewise order; MARSHAL / SPRINT of a finite number is the
    same float64 in repr's number of digits."""
    containers, numbers = V.check_outside()
    print("judged from outside: %d containers, %d numbers" % (containers, numbers))
    assert containers > 1000 and numbers > 3000


def test_counts():
    """Element counts as values under the four ops."""
    assert V.check_counts(V.host_render()) == 4 * len(V.COUNTS)


def test_utf8_acceptance_table():
    """STRING_ESC / MARSHAL decline each of utf8.DecodeRune's rejections and render their
    valid neighbours; STRING / SPRINT pass the bytes through."""
    V.check_utf8_table(V.host_render())


def test_depth_profile_and_long_strings():
    """A value of exactly 1 + (5 i mod 8) levels per request under SPRINT / MARSHAL; strings
    of up to about 3,000 bytes behind a LIT under each op (outputs of many 16-byte blocks)."""
    assert V.check_depth_profile(V.host_render()) == 2 * 257
    assert V.check_long_strings(V.host_render()) == 4 * 130


def test_every_fill_level():
    """The corpus at out_stride 16, 64 and 256: OK exactly when the mirror's bytes fit."""
    counts = V.check_fill_levels(V.host_render())
    for stride, (tot, unfit, inf) in counts.items():
        print("out_stride %d: %d outputs, %d did not fit, %d Inf under MARSHAL given as UNRENDERED"
              % (stride, tot, unfit, inf))
        assert 0 < unfit < tot
    assert sum(inf for _, _, inf in counts.values()) > 0  # (the allowance is not an empty case)


def test_built_text():
    """Modifier chains and "#." lists rendered from the text slot."""
    tot, from_text, not_utf8, unsupported = V.check_built(V.host_render())
    print("built text: %d outputs, %d from the text slot, %d declined as not UTF-8, %d of type 255"
          % (tot, from_text, not_utf8, unsupported))
    assert from_text > tot // 2 and not_utf8 > 0 and unsupported > 0
    assert not_utf8 <= tot // 100 and unsupported <= 3 * tot // 100


# ---- the checks bite ----
CHECKS = {
    "corpus": V.check_corpus,
    "counts": V.check_counts,
    "utf8": V.check_utf8_table,
    "fill": V.check_fill_levels,
    "depth": V.check_depth_profile,
    "long": V.check_long_strings,
    "built": lambda render: V.check_built(render, V.BUILT_SEEDS[:1]),
}
_RH = "authorino_amd/csrc/ajx_render.h"
# (name, file, exact old text, new text, the check that must fail)
MUTANTS = [
    ("signed key bytes", _RH, "if (x != y) return x < y ? -1 : 1;",
     "if (x != y) return (int8_t)x < (int8_t)y ? -1 : 1;", "corpus"),
    ("end sorts last", _RH, "if (x != y) return x < y ? -1 : 1;",
     "if (x != y) return (x < 0 ? 256 : x) < (y < 0 ? 256 : y) ? -1 : 1;", "corpus"),
    ("U+2029 raw", _RH, "if (word == 0xA880E2u || word == 0xA980E2u) {", "if (word == 0xA880E2u) {", "corpus"),
    ("no \\r case", _RH, "                case '\\r': w.put('\\\\'); w.put('r'); break;\n", "", "corpus"),
    ("keep trailing zeros", _RH, "    while (nd > 1 && c.dig_at(nd - 1) == '0') nd--;\n", "", "counts"),
    ("first duplicate wins", _RH, "if (have && render_key_cmp(d, ks, ke, kesc, bks, bke, besc) > 0) continue;",
     "if (have && render_key_cmp(d, ks, ke, kesc, bks, bke, besc) >= 0) continue;", "corpus"),
    ("whitespace after ':' kept", _RH, "                while (i < e && d[i] <= ' ') i++;\n", "", "corpus"),
    ("'g' takes %e from 1e21", _RH, "(exp < -4 || exp >= 6)", "(exp < -4 || exp >= 21)", "corpus"),
]


def _mk(var: str) -> str:
    text = open(os.path.join(T.NATIVE, "render.mk")).read()
    return re.search(r"^%s \??= *(.*)$" % var, text, re.M).group(1)


def _build_copy(root, edit=None):
    """The headers render.mk lists and render_host.cpp under `root` in the tree's layout,
    `edit` = (file, old, new) applied, compiled with render.mk's CXXFLAGS: the library's path."""
    repo = os.path.dirname(T._HERE)
    native = os.path.join(root, "tests", "native")
    files = [os.path.normpath(os.path.join("tests/native", h.replace("$(CSRC)", _mk("CSRC")))) for h in _mk("HDRS").split()]
    for rel in files + ["tests/native/render_host.cpp"]:
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        shutil.copyfile(os.path.join(repo, rel), os.path.join(root, rel))
    if edit:
        rel, old, new = edit
        text = open(os.path.join(root, rel)).read()
        assert text.count(old) == 1, (rel, old, text.count(old))
        with open(os.path.join(root, rel), "w") as f:
            f.write(text.replace(old, new))
    so = os.path.join(native, "libajx_rendertest.so")
    cmd = [os.environ.get("CXX", "g++")] + _mk("CXXFLAGS").split() + ["-std=c++17", "-shared", "-o", so, "render_host.cpp"]
    p = subprocess.run(cmd, cwd=native, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return so


def test_mutants_are_caught(tmp_path):
    """Each one-line mutant of ajx_render.h, built as render.mk builds the library, fails the
    check named for it; the unmutated copy passes every check."""
    assert len(MUTANTS) >= 8
    with ThreadPoolExecutor(4) as pool:
        jobs = [pool.submit(_build_copy, str(tmp_path / "plain"))]
        jobs += [pool.submit(_build_copy, str(tmp_path / ("m%d" % i)), (rel, old, new))
                 for i, (_, rel, old, new, _) in enumerate(MUTANTS)]
        libs = [j.result() for j in jobs]
    plain = V.host_render(T.load(libs[0]))
    for check in CHECKS.values():
        check(plain)
    for (name, _, _, _, check), so in zip(MUTANTS, libs[1:]):
        try:
            CHECKS[check](V.host_render(T.load(so)))
        except AssertionError:
            continue
        pytest.fail("mutant survived its check (%s): %s" % (check, name))


def test_sanitizer_program(tmp_path):
    """tests/native/san_render (ASan + UBSan, its own main) over one seed of the corpus at
    the ample stride and at 16, the UTF-8 table and the counts: exit 0."""
    c = V.corpus(V.SEEDS[0])
    ok = lambda case: [[(R.RENDER_OK, w) for w in row] for row in case.want]  # noqa: E731
    cases = [(c.outputs, c.n_slots, c.docs, c.vals, c.text, c.stride, ok(c))]
    rec, out = V.host_render()(c.outputs, c.n_slots, c.docs, c.vals, c.text, 16)
    V.check_fill(c, rec, out, 16)
    cases.append((c.outputs, c.n_slots, c.docs, c.vals, c.text, 16, V.fill_expected(c, rec, 16)))
    u, _ = V.utf8_table()
    cases.append((u.outputs, u.n_slots, u.docs, u.vals, u.text, u.stride,
                  [[(R.RENDER_UNRENDERED, b"") if w is None else (R.RENDER_OK, w) for w in row] for row in u.want]))
    k = V.counts_case()
    cases.append((k.outputs, k.n_slots, k.docs, k.vals, k.text, k.stride, ok(k)))
    path = tmp_path / "cases.bin"
    T.write_cases(str(path), cases)
    p = subprocess.run([T.make("san_render"), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "4 cases" in p.stdout
