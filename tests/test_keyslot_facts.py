"""CPU test of the child facts a key slot carries (KeySlot::facts, ajx_blob.h: the child
node's selector + 1, has children, has array-index children), which the lean walk takes from
the slot where it used to read the child's TrieNode. The reconcile-time compiler runs on the
host (tests/native/blob_host.cpp) and the test reads the blob's tables as the kernels do:
every occupied slot's facts equal its child's TrieNode fields, every trie edge is found in
the table where the walker looks for it, and on hand-written selector sets the facts are
what the selectors say."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _hosttest as H
import fuzz_util as FU

_NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
SEL_MASK, KIDS, ARR_KIDS = 0x7F, 0x80, 0x100  # kSlotSelMask, kSlotKids, kSlotArrKids
INDEX_KEY_LEN = 0xFFFF                        # kIndexKeyLen
EMPTY = 0xFFFFFFFF                            # kEmptySlot

TRIE_NODE = np.dtype([("child_begin", "<u2"), ("n_children", "u1"), ("flags", "u1"), ("selector", "<i2"),
                      ("pad", "<u2")])
TRIE_CHILD = np.dtype([("sig", "<u8"), ("key_len", "<u4"), ("key_off", "<u4"), ("array_index", "<i4"),
                       ("node", "<u4")])
KEY_SLOT = np.dtype([("sig", "<u8"), ("meta", "<u4"), ("key_off8", "<u2"), ("facts", "<u2")])


@pytest.fixture(scope="module")
def bt(tmp_path_factory):
    # (the compiler alone, built for this module: the flags of tests/native/Makefile)
    csrc = os.path.join(_NATIVE, "..", "..", "authorino_amd", "csrc")
    so = str(tmp_path_factory.mktemp("blobtest") / "libajx_blobtest.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
                    "-Wno-unknown-pragmas", "-shared", "-o", so, os.path.join(_NATIVE, "blob_host.cpp"),
                    os.path.join(csrc, "ajx_compiler.cpp"), os.path.join(csrc, "ajx_regex.cpp")], check=True)
    L = C.CDLL(so)
    L.bt_compile.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]
    L.bt_compile.restype = C.c_uint32
    L.bt_blob.argtypes = [C.c_void_p]
    L.bt_layout.argtypes = [C.POINTER(C.c_uint32)]
    L.bt_home.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    L.bt_home.restype = C.c_uint32
    return L


class Tables:
    def __init__(self, L, patterns, nodes=None, root=None):
        if nodes is None:
            nodes, root = FU.chain(len(patterns))
        t, keep = H.make_tree(patterns, nodes, root)
        err = C.create_string_buffer(512)
        rc = C.c_int(0)
        size = L.bt_compile(C.byref(t), err, 512, C.byref(rc))
        assert rc.value == 0 and size, err.value
        self.L = L
        self.blob = np.zeros(size, np.uint8)
        L.bt_blob(self.blob.ctypes.data)
        lay = (C.c_uint32 * 13)()
        L.bt_layout(lay)
        (self.fast_ok, n_nodes, off_tn, off_tc, off_ks, self.log2, self.probes, _, _, s_tn, s_tc, s_ks,
         self.lean_feat) = list(lay)
        assert (s_tn, s_tc, s_ks) == (TRIE_NODE.itemsize, TRIE_CHILD.itemsize, KEY_SLOT.itemsize)
        self.tn = np.frombuffer(self.blob, TRIE_NODE, n_nodes, off_tn)
        n_tc = int(self.tn["n_children"].sum())
        self.tc = np.frombuffer(self.blob, TRIE_CHILD, n_tc, off_tc)
        self.ks = np.frombuffer(self.blob, KEY_SLOT, 1 << self.log2, off_ks)

    def facts_of(self, node):
        t = self.tn[node]
        return ((int(t["selector"]) + 1) & SEL_MASK) | (KIDS if t["n_children"] else 0) | (ARR_KIDS if t["flags"] & 1 else 0)

    def find(self, sig, klen, parent, key_off=None):
        """The walker's lookup: the slots of (sig, len, parent) within key_probes of home."""
        home = self.L.bt_home(sig, klen, parent)
        hits = []
        for t in range(self.probes):
            s = self.ks[(home + t) & ((1 << self.log2) - 1)]
            if s["meta"] != EMPTY and s["sig"] == sig and (int(s["meta"]) & 0xFFFFFF) == (klen | parent << 16):
                if key_off is None or int(s["key_off8"]) * 8 == key_off:
                    hits.append(s)
        return hits

    def check(self):
        """-> number of occupied slots (every one checked against its child's node)."""
        occupied = self.ks[self.ks["meta"] != EMPTY]
        for s in occupied:
            node = int(s["meta"]) >> 24
            assert node < len(self.tn)
            assert int(s["facts"]) == self.facts_of(node), (s, self.tn[node])
        edges = 0
        for parent, t in enumerate(self.tn):
            for ch in self.tc[int(t["child_begin"]):int(t["child_begin"]) + int(t["n_children"])]:
                if ch["key_len"] < INDEX_KEY_LEN:
                    hits = self.find(int(ch["sig"]), int(ch["key_len"]), parent,
                                     int(ch["key_off"]) if ch["key_len"] > 8 else None)
                    assert [int(h["meta"]) >> 24 for h in hits] == [int(ch["node"])], (parent, ch)
                    assert int(hits[0]["facts"]) == self.facts_of(int(ch["node"]))
                    edges += 1
                if ch["array_index"] >= 0:
                    hits = self.find(int(ch["array_index"]), INDEX_KEY_LEN, parent)
                    assert [int(h["meta"]) >> 24 for h in hits] == [int(ch["node"])], (parent, ch)
                    assert int(hits[0]["facts"]) == self.facts_of(int(ch["node"]))
                    edges += 1
        assert edges == len(occupied)
        return len(occupied)

    def walk(self, path):
        """The facts at the end of `path` (plain keys; a number is an array index where the
        parent has array-index children, as the walker looks elements up), from the root."""
        node, facts = 0, self.facts_of(0)
        for comp in path:
            if isinstance(comp, int):
                hits = self.find(comp, INDEX_KEY_LEN, node)
            else:
                kb = comp.encode()
                sig = int.from_bytes(kb[-8:], "little")
                hits = [h for h in self.find(sig, len(kb), node)
                        if len(kb) <= 8 or bytes(self.blob[self.off_lit(h):self.off_lit(h) + len(kb) - 8]) == kb[:-8]]
            if not hits:
                return None
            assert len(hits) == 1
            node, facts = int(hits[0]["meta"]) >> 24, int(hits[0]["facts"])
        return facts

    def off_lit(self, slot):
        lay = (C.c_uint32 * 13)()
        self.L.bt_layout(lay)
        return lay[8] + int(slot["key_off8"]) * 8


def test_hand_written_selector_sets(bt):
    EQ = 1
    sels = ["a.k", "b.k.x",                                  # one key under two parents: a leaf, a container
            "r.a-long-key-name", "r.b-long-key-name.z",      # long keys sharing their last 8 bytes
            "arr.0", "arr.1.id", "arr.2.3", "m.7.deep.0",    # array-index entries
            "p", "p.q", "p.q.r"]                             # a selector that is a prefix of another
    T = Tables(bt, [(s, EQ, "v") for s in sels])
    assert T.fast_ok
    assert T.check() >= 20
    leaf = lambda f: f is not None and (f & SEL_MASK) and not (f & (KIDS | ARR_KIDS))  # noqa: E731
    inner = lambda f: f is not None and not (f & SEL_MASK) and (f & KIDS)              # noqa: E731
    assert leaf(T.walk(["a", "k"])) and inner(T.walk(["b", "k"])) and not (T.walk(["b", "k"]) & ARR_KIDS)
    assert (T.walk(["a", "k"]) & SEL_MASK) == 1 and (T.walk(["b", "k", "x"]) & SEL_MASK) == 2
    assert leaf(T.walk(["r", "a-long-key-name"])) and inner(T.walk(["r", "b-long-key-name"]))
    assert T.walk(["r", "c-long-key-name"]) is None
    f = T.walk(["arr"])
    assert not (f & SEL_MASK) and (f & KIDS) and (f & ARR_KIDS)
    assert leaf(T.walk(["arr", 0])) and leaf(T.walk(["arr", "0"])) and T.walk(["arr", 0]) == T.walk(["arr", "0"])
    assert inner(T.walk(["arr", 1])) and not (T.walk(["arr", 1]) & ARR_KIDS)
    assert T.walk(["arr", 2]) & ARR_KIDS and leaf(T.walk(["arr", 2, 3]))
    assert T.walk(["arr", 3]) is None
    assert T.walk(["m", 7, "deep"]) & ARR_KIDS and leaf(T.walk(["m", 7, "deep", 0]))
    # prefixes: a selector ends at a node with children
    for path, has_kids in ((["p"], True), (["p", "q"], True), (["p", "q", "r"], False)):
        f = T.walk(path)
        assert (f & SEL_MASK) == 9 + len(path) - 1 and bool(f & KIDS) == has_kids
    assert T.lean_feat == 3  # (kLeanArr | kLeanCaps)


@pytest.mark.parametrize("workload", ["c1", "c2", "c3", "c4", "c5"])
def test_workload_rulesets(bt, workload):
    from authorino_amd import workloads as W

    w = W.make(workload, n=64, seed=3)
    n = 0
    for e in w.sets[:150]:
        pats, nodes, root = e.flatten()
        T = Tables(bt, [(p.selector, int(p.operator), p.value) for p in pats], nodes, root)
        if T.fast_ok:
            n += T.check()
    assert n > 0


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_rulesets(bt, seed):
    rng = np.random.default_rng(700 + seed)
    n = with_arr = with_caps = 0
    for _ in range(100):
        T = Tables(bt, FU.rand_patterns(rng, int(rng.integers(1, 12))))
        if not T.fast_ok:
            continue
        n += T.check()
        with_arr += T.lean_feat & 1
        with_caps += (T.lean_feat >> 1) & 1
    assert n > 300 and with_arr > 5 and with_caps > 5
