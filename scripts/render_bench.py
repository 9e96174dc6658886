#!/usr/bin/env python
"""Time the device-resident response phase of c5 stage by stage: authjx_eval_batch_device
(the forest with the response selectors as its last tree), authjx_select_from_eval_device,
authjx_render_batch_device, all on one stream, each between HIP events.

  python scripts/render_bench.py [--requests N] [--warmup 5] [--steps 20] [--out FILE]

5 warm-up iterations, 20 timed, the median of each stage. For the render kernel also the
bytes it must move — values read + source bytes read + output bytes and records written,
counted from the batch, not measured — the GB/s that implies, and the share of outputs
the device declined (UNRENDERED; expected 0 on c5). A 4096-request sample of the rendered
headers is compared with response.py's host functions (0 mismatches expected). Prints one
JSON line; --out also writes it to a file. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=None, help="requests (default: the benchmark's c5 size)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out-stride", type=int, default=1024, help="bytes of rendered text per request")
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from authorino_amd import response as R, runtime, workloads

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    w = workloads.make("c5", n=args.requests, seed=workloads.DEFAULT_SEEDS.get("c5", 0), unique=4096, uniquify=True)
    ctx = runtime.Context(0)
    cfg = w.auth_config
    exprs = [cfg.conditions] + [e for c in cfg.authorization for e in (c.conditions, c.rules)]
    sel = R.ResponseSelectors(cfg.response, ctx)
    ops, keys = R.compile_render(cfg.response, sel)
    prog = ctx.compile_render(ops.outputs, ops.n_slots)
    forest = ctx.compile_forest(exprs, extra_selectors=sel.paths)
    k = len(sel.paths)
    first = forest.n_patterns - k
    n, no = w.n, prog.n_outputs
    arena = torch.from_numpy(w.arena).to(dev)
    offs = torch.from_numpy(w.offs.view(np.int64)).to(dev)
    lens = torch.from_numpy(w.lens.view(np.int32)).to(dev)
    tri = torch.empty(n * forest.n_trees, dtype=torch.uint8, device=dev)
    err = torch.empty(n * forest.n_trees, dtype=torch.int32, device=dev)
    bm = torch.empty((n, (forest.n_patterns + 63) // 64), dtype=torch.int64, device=dev)
    vals = torch.empty((n, k, 3), dtype=torch.int32, device=dev)
    out_text = torch.empty((n, args.out_stride), dtype=torch.uint8, device=dev)
    rec = torch.empty((n, no, 3), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream

    times = {"eval": [], "select": [], "render": []}
    for it in range(args.warmup + args.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(stream)
        ctx.eval_device([forest], arena, offs, lens, tri, err, bm, stream=sp)
        ev[1].record(stream)
        ctx.select_from_eval_device(forest, first, arena, offs, lens, vals, stream=sp)
        ev[2].record(stream)
        ctx.render_device(prog, arena, offs, lens, vals, out_text, rec, stream=sp)
        ev[3].record(stream)
        stream.synchronize()
        if it >= args.warmup:
            for j, name in enumerate(("eval", "select", "render")):
                times[name].append(ev[j].elapsed_time(ev[j + 1]))
    med = {name: float(np.median(t)) for name, t in times.items()}

    # the bytes the render kernel must move, counted from the batch
    v = vals.cpu().numpy().view(np.uint32)
    r = rec.cpu().numpy().view(np.uint32).copy()
    r[:, :, 2] &= 0xFF
    refs = np.zeros(k, dtype=np.int64)  # ops that read each slot
    lit_bytes = 0
    for o in ops.outputs:
        for op, arg in o:
            if op == R.R_LIT:
                lit_bytes += len(arg)
            else:
                refs[arg] += 1
    spans = ((v[:, :, 2] >> 8) & 0xFF) != R.VAL_COUNT  # (a count has no source bytes)
    src_bytes = int((v[:, :, 1].astype(np.int64) * spans * refs[None, :]).sum())
    val_bytes = n * k * 12
    out_bytes = int(r[:, :, 1].astype(np.int64).sum()) + n * no * 12
    moved = val_bytes + src_bytes + out_bytes
    unrendered = float((r[:, :, 2] != R.RENDER_OK).mean())

    # a sample against the host mirror (response.py over the same selected values)
    m = min(args.sample, n)
    idx = np.linspace(0, n - 1, m).astype(np.int64)
    text = out_text[torch.from_numpy(idx).to(dev)].cpu().numpy()
    http = [c for c in cfg.response if c.wrapper == R.HTTP_HEADER_WRAPPER]
    mismatches = 0
    for j, i in enumerate(idx.tolist()):
        doc = w.doc(i)
        row = R.SelectedRow(v[i])
        for kk, c in enumerate(http):
            want = c.wrap_object_as_header_value(sel.call(c, doc, row))
            s, ln, st = (int(x) for x in r[i, kk])
            got = text[j, s:s + ln].tobytes().decode("utf-8", "replace")
            mismatches += not (st == R.RENDER_OK and got == want)

    result = {
        "workload": "c5", "requests": n, "warmup": args.warmup, "steps": args.steps, "outputs": keys,
        "eval_ms": round(med["eval"], 4), "select_ms": round(med["select"], 4), "render_ms": round(med["render"], 4),
        "render_ms_min": round(float(np.min(times["render"])), 4),
        "render_bytes_counted": {"values": val_bytes, "source": src_bytes, "output": out_bytes, "total": moved},
        "literal_bytes_per_request": lit_bytes,
        "render_gbps_counted": round(moved / (med["render"] * 1e-3) / 1e9, 2),
        "unrendered_share": unrendered, "out_stride": args.out_stride,
        "sample": m, "sample_mismatches": int(mismatches),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if mismatches == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
