"""Model of the lean walk's wave cost (profiling aid, not product code).

The host build of ajx_lean.h traces every walker iteration of a document (sub-window,
token kind; AJX_LEAN_TRACE). Requests go to waves of 64 in the kernel's length order; a
wave runs each sub-window's token loop as long as its busiest lane, and an iteration costs
the union of the branches its lanes take. The model compares that with other schedules:

  lockstep   now: iteration j of sub-window s runs every kind that some lane's j-th token has
  typed      each step runs ONE kind (the most common among the lanes' next tokens); lanes
             whose next token is another kind wait
  window64   lockstep over 64-byte windows (two sub-windows per loop)
  borrow     lockstep, and a lane done with its sub-window takes the next one's tokens while
             the wave's busiest lane goes on, by the walk's own eligibility
             (the trace's second word: tests/native/lean_borrow.mk's library); `borrow_all`
             with every token eligible, `decoupled` the busiest lane's tokens per wave

  python scripts/sim_walk_sched.py [--workload c2] [--n 8192]
"""
import argparse
import collections
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KINDS = ["squash", "str_elem", "pend_val", "key_str", "key_cont", "key_scalar", "root", "elem_cont", "close",
         "scalar_elem"]
# rough per-kind cost in wave instructions (VALU + SALU) of the branch body
COST = [20, 90, 60, 140, 120, 110, 40, 100, 50, 90]
OVERHEAD = 30  # loop head: ctz, bit clear, dispatch tests
KIND_ITERS = collections.Counter()  # iterations in which some lane runs each kind
NKINDS = []


ELIG, STOP, SPLIT = 1 << 24, 1 << 25, 1 << 27  # (ajx_lean.h, kTrace*)


def traces(exprs, docs):
    """[(sub-window, kind, flags)] per document; exprs: one expression, or one per document."""
    import subprocess

    native = os.path.join(ROOT, "tests", "native")
    subprocess.run(["make", "-s", "-C", native, "-f", "lean_borrow.mk", "libajx_leanborrow.so"], check=True)
    os.environ["AJX_HOSTTEST_LIB"] = os.path.join(native, "libajx_leanborrow.so")
    import _hosttest as H

    L = H.lib()
    L.ht_lean_trace.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    L.ht_lean_trace.restype = C.c_uint32
    L.ht_lean_trace_pos.argtypes = [C.POINTER(C.c_uint32)]
    L.ht_lean_trace_pos.restype = None
    one = not isinstance(exprs, list)
    hrs = {}
    buf = (C.c_uint32 * (1 << 16))()
    pos = (C.c_uint32 * (1 << 16))()
    L.ht_lean_trace_pos(pos)
    out = []
    for k, d in enumerate(docs):
        e = exprs if one else exprs[k]
        if id(e) not in hrs:
            hrs[id(e)] = H.HostRuleset.from_expression(e)
        L.ht_lean_trace(buf, 1 << 16)
        H.eval_lean(hrs[id(e)], d, mis=0)
        n = L.ht_lean_trace(None, 0)
        t = np.frombuffer(buf, dtype=np.uint32, count=n).copy()
        out.append((t >> 8, t & 0xFF, np.frombuffer(pos, dtype=np.uint32, count=n).copy()))
    L.ht_lean_trace_pos(None)
    return out


def borrow_iters(wave, real=True):
    """Iterations of a wave when a lane whose own tokens of sub-window s are gone takes its
    tokens of s + 1: one at a time and in order, only eligible ones (real), none after a
    token that stops it (a squash going on, the walk's end), none while it squashes through
    s. A key taken early whose string value closes one sub-window on leaves that closing
    quote as a token of its own (SPLIT)."""
    lanes = []
    for sub, kind, fl in wave:
        lanes.append([[int(s), int(f)] for s, f in zip(sub.tolist(), fl.tolist())])
    heads = [0] * len(lanes)
    last_stop = [False] * len(lanes)
    nsub = max((q[-1][0] for q in lanes if q), default=0) + 2
    iters = 0
    for s in range(1, nsub):
        # (the kernel's go is !skipw after the walk's preamble; the trace knows only that the
        # lane's last token left it squashing. A squash that ends in s with no own token of
        # the lane after it leaves the lane free in the kernel and stopped here: the model
        # errs a little to the pessimistic side)
        go = []
        for i, q in enumerate(lanes):
            h = heads[i]
            own = h < len(q) and q[h][0] <= s
            go.append(own or not last_stop[i])
        while True:
            if not any(heads[i] < len(q) and q[heads[i]][0] <= s for i, q in enumerate(lanes)):
                break
            iters += 1
            for i, q in enumerate(lanes):
                h = heads[i]
                if h >= len(q):
                    continue
                ts, f = q[h]
                if ts <= s:
                    heads[i] += 1
                    last_stop[i] = bool(f & STOP)
                    go[i] = not last_stop[i]
                elif go[i] and ts == s + 1 and (not real or f & ELIG):
                    heads[i] += 1
                    last_stop[i] = bool(f & STOP)
                    go[i] = not last_stop[i]
                    if f & SPLIT:  # (the closing quote: a token of s + 2, never at its last byte)
                        q.insert(heads[i], [s + 2, ELIG])
                else:
                    go[i] = False
    return iters


def per_sub(tr, window=1):
    sub, kind = tr
    g = collections.defaultdict(list)
    for s, k in zip(sub.tolist(), kind.tolist()):
        g[s // window].append(k)
    return g


def wave_costs(wave, window=1):
    subs = [per_sub(t, window) for t in wave]
    keys = set()
    for g in subs:
        keys |= set(g)
    lock = typed = iters = tsteps = 0
    for s in sorted(keys):
        seqs = [g.get(s, []) for g in subs]
        m = max(len(q) for q in seqs)
        iters += m
        for j in range(m):
            present = {q[j] for q in seqs if j < len(q)}
            lock += OVERHEAD + sum(COST[k] for k in present)
            KIND_ITERS.update(present)
            NKINDS.append(len(present))
        heads = [0] * len(seqs)
        while True:
            c = collections.Counter(q[h] for q, h in zip(seqs, heads) if h < len(q))
            if not c:
                break
            k = c.most_common(1)[0][0]
            tsteps += 1
            typed += OVERHEAD + 12 + COST[k]
            for i, q in enumerate(seqs):
                if heads[i] < len(q) and q[heads[i]] == k:
                    heads[i] += 1
    return lock, typed, iters, tsteps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--n", type=int, default=4096)
    a = ap.parse_args()
    from authorino_amd import workloads

    w = workloads.make(a.workload, n=a.n, unique=a.n, uniquify=True)
    docs = [w.doc(i) for i in range(w.n)]
    order = np.argsort(-(w.lens.astype(np.int64) >> 3), kind="stable")  # the kernel's length classes
    if w.set_of_req is not None:  # (c4: each document with its tenant's ruleset, in the batch's order)
        order = np.arange(w.n)
        trs = traces([w.sets[int(w.set_of_req[i])] for i in order], docs)
    else:
        trs = traces(w.expr, [docs[i] for i in order])
    kinds = collections.Counter()
    for _, k, _ in trs:
        kinds.update(k.tolist())
    print("tokens per doc:", round(sum(kinds.values()) / len(trs), 1),
          {KINDS[k]: round(v / len(trs), 1) for k, v in sorted(kinds.items())})
    tot = collections.Counter()
    for b in range(0, len(trs) - 63, 64):
        wave = trs[b:b + 64]
        l1, t1, i1, s1 = wave_costs([t[:2] for t in wave], 1)
        l2, _, i2, _ = wave_costs([t[:2] for t in wave], 2)
        tot.update({"lock": l1, "typed": t1, "iters": i1, "typed_steps": s1, "win64": l2, "win64_iters": i2,
                    "borrow_iters": borrow_iters(wave), "borrow_all_iters": borrow_iters(wave, real=False),
                    "decoupled_iters": max(len(t[0]) for t in wave), "waves": 1})
    nw = tot["waves"]
    print({k: round(v / nw, 1) for k, v in tot.items()})
    print("kinds per lockstep iteration:", round(float(np.mean(NKINDS)), 2),
          "iterations per wave running each kind:", {KINDS[k]: round(v / nw / 2, 1) for k, v in KIND_ITERS.items()})


if __name__ == "__main__":
    main()
