#!/usr/bin/env python3
"""Time one evaluation pass over a synthetic resident split (uint8 noise, ViT-B/16 + CaRA rank 16) through

  (a) recipe.evaluate(model, split.eval_batches(B)())   -- the reference loop: normalise on the device, model(x), argmax,
      one .item() per batch, the training-sized workspace of the engine;
  (b) engine.evaluate(split, B)                         -- the uint8 forward on an inference-sized workspace, the counting
      kernel after every batch, one host read per pass;

and print seconds per pass (median, min, max over --passes after one warm-up each), images/s and the workspace bytes of
both.  Standalone: not part of bench.py.  --only a|b runs one leg (the leg (a) of an older build: CARA_LIB_PATH).
--report (with --only none to skip the legs above) times (b) against engine.evaluate(split, B, report=True): the same pass with
cara_eval_accumulate_report instead of cara_eval_accumulate after every batch (docs/findings/eval_report.md).
--views center|flip|five|ten times (b) against engine.evaluate(split, B, views=...) on the same split, alternating: 1, 2, 5 or 10
forwards per image in batches of B // V whole samples, and the device time of one cara_eval_combine_views launch on such a batch
as a share of the pass (docs/findings/eval_views.md).  --combine prob|logit.
--predict times (b) against engine.predict(split, k, B) on the same split, alternating: the same forwards with one
cara_eval_predict launch per batch instead of the counting launch, and the device time of that launch beside the counting launches'
(docs/findings/eval_predict.md).  --k."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10_000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--only", default="ab", choices=["a", "b", "ab", "none"])
    ap.add_argument("--report", action="store_true", help="time engine.evaluate with and without report=True, alternating")
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2, help="--report / --views: alternations of (plain passes, other passes)")
    ap.add_argument("--views", default=None, choices=["center", "flip", "five", "ten"],
                    help="time engine.evaluate with and without these views (centre crop, centre crop + flip, five crops, ten crops)")
    ap.add_argument("--combine", default="prob", choices=["prob", "logit"])
    ap.add_argument("--predict", action="store_true", help="time engine.evaluate against engine.predict, alternating")
    ap.add_argument("--k", type=int, default=5, help="--predict: top-k slots per sample")
    args = ap.parse_args()
    from cara_amd import cara, create_model, recipe
    from cara_amd.data import ResidentSplit
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = create_model("vit_base_patch16_224_in21k", depth=args.depth, num_classes=args.classes, drop_path_rate=0.1)
    m = cara({"model": m, "rank": args.rank, "scale": 0.1, "l_mu": 1.5, "l_std": 0.1, "precision": args.precision}).to(dev).eval()
    eng = m._cara_engine
    g = torch.Generator(device=dev).manual_seed(1)
    px = torch.randint(0, 256, (args.images, 3, 224, 224), generator=g, dtype=torch.uint8, device=dev)
    y = torch.randint(0, args.classes, (args.images,), generator=g, device=dev)
    split = ResidentSplit.from_tensors(px, y)

    def timed(fn):
        fn()   # warm-up: workspaces allocated, weights ingested
        torch.cuda.synchronize(dev)
        out = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            out.append(time.perf_counter() - t0)
        return out

    res = {"images": args.images, "batch": args.batch, "passes": args.passes, "precision": args.precision, "depth": args.depth}

    def report(name, ts, ws_bytes, acc):
        med = statistics.median(ts)
        res[name] = {"seconds": [round(t, 4) for t in ts], "median_s": round(med, 4), "min_s": round(min(ts), 4),
                     "max_s": round(max(ts), 4), "spread_pct": round(100 * (max(ts) - min(ts)) / med, 2),
                     "images_per_s": round(args.images / med, 1), "workspace_bytes": int(ws_bytes), "top1": acc}

    if "a" in args.only:
        acc = [0.0]
        ts = timed(lambda: acc.__setitem__(0, recipe.evaluate(m, split.eval_batches(args.batch)())))
        # (the reference loop leaves the workspace of its LAST batch shape alive; the full-batch one is the larger)
        peak = max(st["ws"].numel() for st in eng._ws.values())
        full = int(eng._lib().cara_vit_workspace_bytes(*[C.byref(v) for v in _shape(eng, m, args.batch)]))
        report("reference_loop", ts, max(peak, full), acc[0])
        eng._ws.clear()
        torch.cuda.empty_cache()
    if "b" in args.only:
        out = [None]
        ts = timed(lambda: out.__setitem__(0, eng.evaluate(split, args.batch)))
        report("engine_evaluate", ts, eng.eval_workspace_bytes(), out[0]["top1"])
        res["engine_evaluate"].update(top5=out[0]["top5"], loss=out[0]["loss"], n=out[0]["n"])
    if args.report:
        # the plain pass and the report pass in turn, --rounds times, on the same box in one run: their ratio is the report's cost
        plain, rep, out = [], [], [None]
        for _ in range(args.rounds):
            plain += timed(lambda: out.__setitem__(0, eng.evaluate(split, args.batch)))
            rep += timed(lambda: out.__setitem__(0, eng.evaluate(split, args.batch, report=True, bins=args.bins)))
        report("plain_pass", plain, eng.eval_workspace_bytes(), out[0]["top1"])
        report("report_pass", rep, eng.eval_workspace_bytes(), out[0]["top1"])
        res["report_pass"].update(bins=args.bins, mean_per_class=out[0]["mean_per_class"], ece=out[0]["ece"],
                                  report_bytes=8 * (args.classes ** 2 + 3 * args.bins))
        res["report_over_plain"] = round(res["report_pass"]["median_s"] / res["plain_pass"]["median_s"], 4)
        res["counting_launch_us"] = _launch_us(eng, args, dev)
    if args.views:
        from cara_amd.data import EvalViews
        views = {"center": EvalViews.center(224), "flip": EvalViews.center(224, flip=True), "five": EvalViews.five_crop(224),
                 "ten": EvalViews.ten_crop(224)}[args.views]
        plain, multi, out = [], [], [None]
        for _ in range(args.rounds):
            plain += timed(lambda: out.__setitem__(0, eng.evaluate(split, args.batch)))
            multi += timed(lambda: out.__setitem__(0, eng.evaluate(split, args.batch, views=views, combine=args.combine)))
        report("plain_pass", plain, eng.eval_workspace_bytes(), None)
        report("views_pass", multi, eng.eval_workspace_bytes(), out[0]["top1"])
        S = args.batch // views.V
        batches = -(-args.images // S)
        us = _combine_us(eng, args, dev, S, views.V) if views.V > 1 else 0.0     # (one view: no combine launch)
        res["views_pass"].update(views=args.views, V=views.V, combine=args.combine, samples_per_batch=S, batches=batches, n=out[0]["n"],
                                 loss=out[0]["loss"], combine_launch_us=us,
                                 combine_share_pct=round(100 * us * 1e-6 * batches / res["views_pass"]["median_s"], 4))
        res["views_over_plain"] = round(res["views_pass"]["median_s"] / res["plain_pass"]["median_s"], 4)
    if args.predict:
        # the plain pass and the predict pass in turn, --rounds times, on the same box in one run: their ratio is the table's cost
        plain, pred, out, tab = [], [], [None], [None]
        for _ in range(args.rounds):
            plain += timed(lambda: out.__setitem__(0, eng.evaluate(split, args.batch)))
            pred += timed(lambda: tab.__setitem__(0, eng.predict(split, args.k, args.batch)))
        counts = tab[0].counts()
        report("plain_pass", plain, eng.eval_workspace_bytes(), out[0]["top1"])
        report("predict_pass", pred, eng.eval_workspace_bytes(), counts["top1"])
        res["predict_pass"].update(k=args.k, n=counts["n"], loss=counts["loss"], table_bytes=4 * args.images * (2 * args.k + 2),
                                   same_counts=[counts[key] == out[0][key] for key in ("n", "top1", "top5")])
        res["predict_over_plain"] = round(res["predict_pass"]["median_s"] / res["plain_pass"]["median_s"], 4)
        res["counting_launch_us"] = _launch_us(eng, args, dev)
    print(json.dumps(res))


def _combine_us(eng, args, dev, S, V, launches=200):
    """device time of one cara_eval_combine_views launch on a [S*V, classes] logit table (events around `launches` back-to-back
    launches, best of six after a warm-up)"""
    from cara_amd import _lib as L
    lib = eng._lib()
    lg = torch.randn(S * V, args.classes, device=dev) * 3.0
    out = torch.empty(S, args.classes, device=dev)
    best = float("inf")
    for _ in range(7):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            L.check(lib.cara_eval_combine_views(L.ptr(lg), args.classes, S, V, args.classes, L.EVAL_COMBINE[args.combine], L.ptr(out),
                                                args.classes, L.stream(dev)), "cara_eval_combine_views")
        t1.record()
        torch.cuda.synchronize(dev)
        best = min(best, t0.elapsed_time(t1) * 1e3 / launches)
    return round(best, 3)


def _launch_us(eng, args, dev, launches=200):
    """device time of one counting launch on a [batch, classes] logit table, plain, with the report and as cara_eval_predict (events around `launches`
    back-to-back launches, best of five after a warm-up)"""
    from cara_amd._lib import check, ptr, stream
    lib = eng._lib()
    lg = torch.randn(args.batch, args.classes, device=dev) * 3.0
    y = torch.randint(0, args.classes, (args.batch,), device=dev)
    st = torch.zeros(5, dtype=torch.int64, device=dev)
    rep = torch.zeros(args.classes ** 2 + 3 * args.bins, dtype=torch.int64, device=dev)
    k = getattr(args, "k", 5)
    tab = (torch.zeros(args.batch, k, dtype=torch.int32, device=dev), torch.zeros(args.batch, k, device=dev),
           torch.zeros(args.batch, device=dev), torch.zeros(args.batch, dtype=torch.int32, device=dev))
    calls = {"plain": lambda: lib.cara_eval_accumulate(ptr(lg), args.classes, ptr(y), args.batch, args.batch, args.classes, ptr(st),
                                                       stream(dev)),
             "report": lambda: lib.cara_eval_accumulate_report(ptr(lg), args.classes, ptr(y), args.batch, args.batch, args.classes,
                                                               ptr(st), ptr(rep), args.bins, stream(dev)),
             "predict": lambda: lib.cara_eval_predict(ptr(lg), args.classes, ptr(y), args.batch, args.batch, args.classes, k, 0, args.batch,
                                                      ptr(tab[0]), ptr(tab[1]), ptr(tab[2]), ptr(tab[3]), stream(dev))}
    out = {}
    for name, call in calls.items():
        best = float("inf")
        for _ in range(6):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                check(call(), name)
            t1.record()
            torch.cuda.synchronize(dev)
            best = min(best, t0.elapsed_time(t1) * 1e3 / launches)
        out[name] = round(best, 3)
    return out


def _shape(eng, m, B):
    """(geom, shape) of the engine's training-sized workspace at batch B: what model(x) allocates for a full batch"""
    from cara_amd import _lib as L
    pe = m.patch_embed
    patch = pe.proj.kernel_size[0]
    geom = L.Geom(len(m.blocks), m.embed_dim, m.blocks[0].attn.num_heads, eng.rank, eng.Rp, eng.scale, eng.cp_length)
    shape = L.VitShape(B, 224, patch, 3, (224 // patch) ** 2 + 1, m.head.out_features, float(m.norm.eps), 0, 0.1, 0, 0)
    return geom, shape


if __name__ == "__main__":
    main()
