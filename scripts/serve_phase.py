#!/usr/bin/env python
"""The serving path of c5 (the full phase plus its four response headers) under load.

  python scripts/serve_phase.py --mode phase    [--requests N] [--out FILE]
  AUTHJX_LIB=<a library of the parent commit> python scripts/serve_phase.py --mode baseline ...

--mode phase: authjx_batcher_phase, the decision and the rendered headers from one blocking
call. Closed loop at 64 and 256 native producer threads (authjx_debug_phase_loadgen): p50 /
p99 latency, requests/s, the batcher profile's pack / launch / wait split per batch; the
same call from 64 Python producer threads (what the baseline below is driven by, so the two
can be compared like for like); and the device time of each stage of one 64-request batch
(eval, multi-set select, multi-program render) between HIP events on one stream. Every
request's header bytes are checked by their FNV-1a against the one-program
authjx_select_text_batch + authjx_render_batch calls over the whole sample.

--mode baseline: what a shim can do without that call, with the library AUTHJX_LIB names (a
build of the parent commit has no more): per request one authjx_batcher_eval, then one
authjx_select_text_batch (n = 1) and one authjx_render_batch (n = 1), from 64 and 256
Python producer threads (ctypes releases the GIL around each call).

Prints one JSON line; --out also writes it to a file. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _pct(lat_ns):
    us = np.sort(np.asarray(lat_ns, dtype=np.float64) / 1e3)
    n = len(us)
    return {"p50": round(float(us[n // 2]), 1), "p99": round(float(us[int(n * 0.99)]), 1), "max": round(float(us[-1]), 1)}


def _fnv(vals):
    h = 0xcbf29ce484222325
    for v in vals:
        h = ((h ^ (0 if v is not None else 1)) * 0x100000001b3) & (2 ** 64 - 1)
        for x in v or b"":
            h = ((h ^ x) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def _python_producers(threads, n, call):
    """n requests from `threads` Python threads, request i by thread i % threads:
    (latencies ns, results, wall ns)."""
    lat = np.zeros(n, dtype=np.uint64)
    res = [None] * n

    def run(t):
        for i in range(t, n, threads):
            a = time.perf_counter_ns()
            res[i] = call(i)
            lat[i] = time.perf_counter_ns() - a

    ts = [threading.Thread(target=run, args=(t,)) for t in range(threads)]
    t0 = time.perf_counter_ns()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return lat, res, time.perf_counter_ns() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("phase", "baseline"), default="phase")
    ap.add_argument("--requests", type=int, default=1 << 15, help="requests of the native closed loops")
    ap.add_argument("--py-requests", type=int, default=1 << 13, help="requests of the Python producers' loops")
    ap.add_argument("--window-us", type=int, default=50)
    ap.add_argument("--out-stride", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from authorino_amd import response as R, runtime, workloads

    n = max(args.requests, args.py_requests)
    w = workloads.make("c5", n=n, seed=workloads.DEFAULT_SEEDS.get("c5", 0), unique=4096, uniquify=True)
    ctx = runtime.Context(0)
    cfg = w.auth_config
    exprs = [cfg.conditions] + [e for c in cfg.authorization for e in (c.conditions, c.rules)]
    forest = ctx.compile_forest(exprs)
    sel = R.ResponseSelectors(cfg.response, ctx)
    prog, _ = sel._render_program()
    docs = [w.doc(i) for i in range(args.py_requests)]
    result = {"workload": "c5", "mode": args.mode, "window_us": args.window_us, "max_batch": 8192, "workers": 2,
              "out_stride": args.out_stride, "library": os.environ.get("AUTHJX_LIB", "in-tree"),
              "device": torch.cuda.get_device_name(0), "loops": []}

    # what every request's headers must be: the one-program calls over the whole sample
    m = args.py_requests
    spans = sel.resolve(docs, w.arena, w.offs[:m], w.lens[:m])
    want, status = sel.render(w.arena, w.offs[:m], w.lens[:m], spans, out_stride=args.out_stride)
    want_hash = np.array([_fnv(row) for row in want], dtype=np.uint64)
    result["unrendered_share"] = float((status != R.RENDER_OK).mean())

    if args.mode == "baseline":
        def call(i):
            tri, _ = b.eval(forest, docs[i])
            o, ln = w.offs[i:i + 1] * 0, w.lens[i:i + 1]
            arena = np.frombuffer(docs[i] + b"\0", dtype=np.uint8)
            sp = sel.resolve([docs[i]], arena, o, ln)
            vals, _ = sel.render(arena, o, ln, sp, out_stride=args.out_stride)
            return tri[0], _fnv(vals[0])

        for threads in (64, 256):
            b = runtime.Batcher(ctx, max_batch=8192, window_us=args.window_us)
            try:
                _python_producers(threads, min(1024, m), call)  # (warm up)
                lat, res, wall = _python_producers(threads, m, call)
                prof = b.profile()
            finally:
                b.close()
            ok = all(int(h) == int(want_hash[i]) for i, (_, h) in enumerate(res))
            result["loops"].append({"producers": "python threads", "producer_threads": threads, "requests": m,
                                    "requests_per_s": round(m / (wall * 1e-9), 1), "latency_us": _pct(lat),
                                    "headers_equal_one_program_calls": ok, "batcher_profile_us": prof,
                                    "calls_per_request": "authjx_batcher_eval + authjx_select_text_batch(n=1) + "
                                                         "authjx_render_batch(n=1)"})
    else:
        phase, keys = sel.phase(forest, out_stride=args.out_stride)
        result["outputs"] = keys
        ns = args.requests
        por = np.zeros(ns, dtype=np.uint32)
        for threads in (64, 256):
            b = runtime.Batcher(ctx, max_batch=8192, window_us=args.window_us)
            try:
                b.phase_loadgen([phase], por[:4096], w.arena, w.offs[:4096], w.lens[:4096], threads=threads)  # (warm up)
                p0 = b.profile()
                lat, tri, hsh, wall = b.phase_loadgen([phase], por, w.arena, w.offs[:ns], w.lens[:ns], threads=threads)
                p1 = b.profile()
            finally:
                b.close()
            nb = max(p1["batches"] - p0["batches"], 1)
            split = {k: round((p1[k] * p1["batches"] - p0[k] * p0["batches"]) / nb, 2)
                     for k in ("pack_us", "launch_us", "sync_us", "wake_us", "eval_us")}
            k = min(ns, m)
            result["loops"].append({"producers": "native threads (authjx_debug_phase_loadgen)",
                                    "producer_threads": threads, "requests": ns,
                                    "requests_per_s": round(ns / (wall * 1e-9), 1), "latency_us": _pct(lat),
                                    "batches": nb, "mean_batch": round(ns / nb, 1), "per_batch_us": split,
                                    "headers_equal_one_program_calls": bool(np.array_equal(hsh[:k], want_hash[:k]))})
        b = runtime.Batcher(ctx, max_batch=8192, window_us=args.window_us)
        try:
            call = lambda i: b.phase(phase, docs[i])  # noqa: E731
            _python_producers(64, min(1024, m), call)
            lat, res, wall = _python_producers(64, m, call)
        finally:
            b.close()
        ok = all(_fnv(r[2]) == int(want_hash[i]) for i, r in enumerate(res))
        result["loops"].append({"producers": "python threads", "producer_threads": 64, "requests": m,
                                "requests_per_s": round(m / (wall * 1e-9), 1), "latency_us": _pct(lat),
                                "headers_equal_one_program_calls": ok})

        # one 64-request batch, stage by stage, as the batcher queues it (device buffers)
        dev = torch.device("cuda", 0)
        nb = 64
        end = int(w.offs[nb - 1] + w.lens[nb - 1])
        A = torch.from_numpy(w.arena[:end + 1].copy()).to(dev)
        Of = torch.from_numpy(w.offs[:nb].view(np.int64).copy()).to(dev)
        Ln = torch.from_numpy(w.lens[:nb].view(np.int32).copy()).to(dev)
        tri = torch.empty(nb * forest.n_trees, dtype=torch.uint8, device=dev)
        err = torch.empty(nb * forest.n_trees, dtype=torch.int32, device=dev)
        vals = torch.empty((nb, len(sel.paths), 3), dtype=torch.int32, device=dev)
        text = torch.empty((nb, sel.TEXT_STRIDE), dtype=torch.uint8, device=dev)
        out = torch.empty((nb, args.out_stride), dtype=torch.uint8, device=dev)
        rec = torch.empty((nb, prog.n_outputs, 3), dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(dev)
        sp = stream.cuda_stream
        times = {"eval": [], "select": [], "render": []}
        for it in range(30):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(stream)
            ctx.eval_device([forest], A, Of, Ln, tri, err, None, stream=sp)
            ev[1].record(stream)
            ctx.select_text_device([sel.ruleset], A, Of, Ln, vals, text, stream=sp)
            ev[2].record(stream)
            ctx.render_multi_device([prog], None, A, Of, Ln, vals, out, rec, text=text, stream=sp)
            ev[3].record(stream)
            stream.synchronize()
            if it >= 10:
                for j, name in enumerate(("eval", "select", "render")):
                    times[name].append(ev[j].elapsed_time(ev[j + 1]) * 1e3)
        ctx.release_stream(sp)
        result["one_batch_of_64_device_us"] = {
            name: {"median": round(float(np.median(t)), 1), "min": round(float(np.min(t)), 1),
                   "max": round(float(np.max(t)), 1)} for name, t in times.items()}
        result["one_batch_of_64_device_us"]["note"] = ("20 timed after 10 warm-up iterations; HIP events on one "
                                                       "stream, each interval holds the stage's launches")

    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(lp["headers_equal_one_program_calls"] for lp in result["loops"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
