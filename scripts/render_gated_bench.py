#!/usr/bin/env python
"""Time the gated render beside the ungated one on c5: its response program plus a
three-output denyWith (a static message, a template body, a pattern header), the values
selected once (authjx_eval_batch_device + authjx_select_from_eval_device over the union of
the response and denyWith paths), the tri-states given directly as a device array of one
tree (the rules), then, alternating in one session and each between HIP events:

  ungated       authjx_render_batch_device, the response program alone
  granted       authjx_render_batch_gated_device, every request granted
  quarter       ... every fourth request denied (a denied lane in each group of four:
                every wave holds both kinds and walks both sets of outputs)
  quarter_runs  ... the first quarter of the batch denied (whole waves of one kind)
  denied        ... every request denied

  python scripts/render_gated_bench.py [--requests N] [--warmup 5] [--steps 20] [--repeats 3] [--out FILE]

A repeat is 5 warm-up and 20 timed rounds of the five; per repeat the median of each, so
that the ungated kernel's own spread between repeated medians is on record beside the others.
A 2048-request sample of each gated variant is compared with response.py's host functions
(0 mismatches expected). Prints one JSON line; --out also writes it to a file. Needs a GPU:
there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("ungated", "granted", "quarter", "quarter_runs", "denied")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=None, help="requests (default: the benchmark's c5 size)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out-stride", type=int, default=1024, help="bytes of rendered text per request")
    ap.add_argument("--sample", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from authorino_amd import pipeline as P, response as R, runtime, workloads

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    w = workloads.make("c5", n=args.requests, seed=workloads.DEFAULT_SEEDS.get("c5", 0), unique=4096, uniquify=True)
    ctx = runtime.Context(0)
    cfg = w.auth_config
    JV = R.JSONValue
    deny = P.DenyWithValues(
        code=403, message=JV(static="Access denied"),
        body=JV(pattern="user {auth.identity.sub} may not {context.request.http.method} on {context.request.http.host}"),
        headers=[("x-roles", JV(pattern="auth.identity.realm_access.roles"))])
    exprs = [cfg.conditions] + [e for c in cfg.authorization for e in (c.conditions, c.rules)]
    sel = P.GatedSelectors(cfg.response, deny.values(), ctx)
    rops, keys = R.compile_render(cfg.response, sel)
    dops, kinds = R.compile_deny_render(deny, sel)
    ungated = ctx.compile_render(rops.outputs, rops.n_slots)
    prog = ctx.compile_render(rops.outputs + dops.outputs, rops.n_slots)
    n_resp, no = len(rops.outputs), len(rops.outputs) + len(dops.outputs)
    gates = ctx.compile_gates(-1, [(-1, 0, 0)], [(P.GATE_GRANTED, -1)] * n_resp + [(P.GATE_DENIED, -1)] * len(dops.outputs), 1)
    forest = ctx.compile_forest(exprs, extra_selectors=sel.paths)
    k = len(sel.paths)
    first = forest.n_patterns - k
    n = w.n
    arena = torch.from_numpy(w.arena).to(dev)
    offs = torch.from_numpy(w.offs.view(np.int64)).to(dev)
    lens = torch.from_numpy(w.lens.view(np.int32)).to(dev)
    tri_all = torch.empty(n * forest.n_trees, dtype=torch.uint8, device=dev)
    err = torch.empty(n * forest.n_trees, dtype=torch.int32, device=dev)
    bm = torch.empty((n, (forest.n_patterns + 63) // 64), dtype=torch.int64, device=dev)
    vals = torch.empty((n, k, 3), dtype=torch.int32, device=dev)
    out_text = torch.empty((n, args.out_stride), dtype=torch.uint8, device=dev)
    rec = torch.empty((n, no, 3), dtype=torch.int32, device=dev)
    ver = torch.empty((n, 2), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    ctx.eval_device([forest], arena, offs, lens, tri_all, err, bm, stream=sp)
    ctx.select_from_eval_device(forest, first, arena, offs, lens, vals, stream=sp)
    lane = torch.arange(n, device=dev)
    tri = {"granted": torch.ones((n, 1), dtype=torch.uint8, device=dev),
           "quarter": (lane % 4 != 3).to(torch.uint8).reshape(n, 1).contiguous(),
           "quarter_runs": (lane >= n // 4).to(torch.uint8).reshape(n, 1).contiguous(),
           "denied": torch.zeros((n, 1), dtype=torch.uint8, device=dev)}
    stream.synchronize()

    rec_ungated = torch.empty((n, n_resp, 3), dtype=torch.int32, device=dev)

    def launch(name):
        if name == "ungated":
            ctx.render_device(ungated, arena, offs, lens, vals, out_text, rec_ungated, stream=sp)
        else:
            ctx.render_gated_device([prog], [gates], None, arena, offs, lens, vals, out_text, rec, tri[name],
                                    verdicts=ver, stream=sp)

    repeats = []
    for _ in range(args.repeats):
        times = {name: [] for name in VARIANTS}
        for it in range(args.warmup + args.steps):
            for name in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch(name)
                e1.record(stream)
                stream.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        repeats.append({name: round(float(np.median(t)), 4) for name, t in times.items()})

    # a sample of each gated variant against the host mirror
    v = vals.cpu().numpy().view(np.uint32)
    m = min(args.sample, n)
    idx = np.linspace(0, n - 1, m).astype(np.int64)
    http = [c for c in cfg.response if c.wrapper == R.HTTP_HEADER_WRAPPER]
    dvals = [x for x in (deny.message, deny.body) if x is not None] + [x for _, x in deny.headers]
    mismatches, statuses = 0, {}
    for name in VARIANTS[1:]:
        launch(name)
        stream.synchronize()
        r = rec.cpu().numpy().view(np.uint32).copy()
        r[:, :, 2] &= 0xFF
        statuses[name] = [int((r[:, :, 2] == s).sum()) for s in (R.RENDER_OK, R.RENDER_UNRENDERED, R.RENDER_SKIPPED)]
        text = out_text[torch.from_numpy(idx).to(dev)].cpu().numpy()
        vd = ver.cpu().numpy()
        t = tri[name].cpu().numpy()
        for j, i in enumerate(idx.tolist()):
            doc, row = w.doc(i), R.SelectedRow(v[i])
            granted = t[i, 0] == runtime.T
            mismatches += int(vd[i, 0] & 0xFF) != (P.V_GRANTED if granted else P.V_DENIED)
            want = [c.wrap_object_as_header_value(sel.call(c, doc, row)) if granted else None for c in http]
            want += [None if granted else R.stringify_json(sel.value(x, doc, row)) for x in dvals]
            for kk, wnt in enumerate(want):
                s, ln, st = (int(x) for x in r[i, kk])
                got = text[j, s:s + ln].tobytes().decode("utf-8", "replace")
                mismatches += not ((st, got) == (R.RENDER_OK, wnt) if wnt is not None else (st, ln) == (R.RENDER_SKIPPED, 0))

    med = {name: float(np.median([rp[name] for rp in repeats])) for name in VARIANTS}
    spread = max(rp["ungated"] for rp in repeats) - min(rp["ungated"] for rp in repeats)
    result = {
        "workload": "c5", "requests": n, "warmup": args.warmup, "steps": args.steps, "repeats": repeats,
        "outputs": keys + ["%s:%s" % kn if kn[1] else kn[0] for kn in kinds], "out_stride": args.out_stride,
        "render_ms_median": {name: round(x, 4) for name, x in med.items()},
        "ungated_spread_between_repeats_ms": round(spread, 4),
        "granted_minus_ungated_ms": round(med["granted"] - med["ungated"], 4),
        "statuses_ok_unrendered_skipped": statuses, "sample": m, "sample_mismatches": int(mismatches),
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
