#!/usr/bin/env python3
"""What sharpness-aware minimisation costs in the training step of the headline configuration (ViT-B/16 + CaRA rank 16, batch 64,
224 px, DropPath 0.1, factored adapters, AdamW), on one GPU:

  step            CaraEngine.train_step as it is (the yardstick: the plain step on the same box, in the same run);
  step+sam        the same step with sam_rho= (two forward/backward passes, one tail, three small launches between them);
  graph           the plain step replayed from a hipGraph (recipe.GraphedTrainStep);
  graph+sam       the SAM step replayed from ONE graph;
  kernel/measure  cara_grad_clip with max_norm = inf over the flat gradient buffer (two launches: it only measures),
  kernel/perturb  cara_sam_perturb over the 14 trainable tensors,
  kernel/restore  cara_sam_restore over them: device events around --kernel-launches back-to-back calls (rho = 0 there, so that
                  the weights stand still: the launches' work is the same).

The legs run interleaved in one process, round by round, after --warmup steps of each; the line printed says the median / min / max
over the rounds.  Every timed window runs under its own time limit (--window-timeout seconds: the process dumps its stacks and
exits when a window does not come back), and nothing is tried twice.  Standalone: not part of bench.py."""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--rho", type=float, default=0.05)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--kernel-launches", type=int, default=500)
    ap.add_argument("--window-timeout", type=float, default=120.0)
    args = ap.parse_args()
    from cara_amd import _lib as L
    from cara_amd import cara, create_model
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    dev = torch.device("cuda", 0)
    torch.manual_seed(14)
    m = create_model("vit_base_patch16_224_in21k", depth=args.depth, num_classes=100, drop_path_rate=0.1)
    m = cara({"model": m, "rank": args.rank, "scale": 0.1, "l_mu": 1.5, "l_std": 0.1, "precision": args.precision})
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():   # non-zero adapters, as bench.py's model
        m.CP_A2.copy_(0.05 * torch.randn(m.CP_A2.shape, generator=g))
        m.CP_P2.copy_(0.05 * torch.randn(m.CP_P2.shape, generator=g))
    m = m.to(dev).train()
    eng = m._cara_engine
    eng.seed_rank_streams(2024, 0)
    for n, p in m.named_parameters():
        p.requires_grad = "CP" in n or "head" in n
    # (one capturable AdamW for all four legs: the eager ones advance it by hand, as GraphedTrainStep does)
    opt = AdamW(eng.trainable_parameters(), lr=1e-4, weight_decay=1e-4, capturable=True)
    gd = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(args.batch, 3, 224, 224, generator=gd, device=dev)
    y = torch.randint(0, 100, (args.batch,), generator=gd, device=dev)
    gplain, gsam = GraphedTrainStep(eng, opt), GraphedTrainStep(eng, opt, sam_rho=args.rho)

    def eager(**kw):
        opt.advance()
        return eng.train_step(x, y, opt, **kw)
    steps = {"step": eager, "step+sam": lambda: eager(sam_rho=args.rho), "graph": lambda: gplain(x, y), "graph+sam": lambda: gsam(x, y)}

    def limited(fn, *a):
        faulthandler.dump_traceback_later(args.window_timeout, exit=True)
        try:
            return fn(*a)
        finally:
            faulthandler.cancel_dump_traceback_later()

    def step_window(name, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            loss = steps[name]()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / n, float(loss)

    for name in steps:
        limited(step_window, name, args.warmup)
    # the three launches alone, on the engine's own SAM buffers (left by the steps above)
    lib, st = eng._lib(), L.stream(dev)
    sam = eng._sam_perturb(m, dev, args.batch, 0.0)
    eng._sam_restore(sam, dev)
    _, k, parr, garr, barr, narr = sam["plan"]
    flat, nflat = eng._flat_grad, eng._flat_grad.numel() - 1
    ptr = L.ptr
    kernels = {"kernel/measure": lambda: lib.cara_grad_clip(ptr(flat), nflat, float("inf"), ptr(sam["scratch"]), None, ptr(sam["norm"]), st),
               "kernel/perturb": lambda: lib.cara_sam_perturb(k, parr, garr, barr, narr, 0.0, ptr(sam["norm"]), None, ptr(sam["state"]), st),
               "kernel/restore": lambda: lib.cara_sam_restore(k, parr, barr, narr, ptr(sam["state"]), None, st)}

    def kernel_window(name, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        bad = 0
        e0.record()
        for _ in range(n):
            bad |= kernels[name]()
        e1.record()
        torch.cuda.synchronize(dev)
        if bad:
            raise SystemExit(f"{name}: a call returned status {bad}")
        return e0.elapsed_time(e1) * 1e3 / n      # us per call
    for name in kernels:
        limited(kernel_window, name, 20)
    ms, us, last = {n: [] for n in steps}, {n: [] for n in kernels}, {}
    for _ in range(args.rounds):
        for name in steps:
            t, last[name] = limited(step_window, name, args.steps)
            ms[name].append(t)
        for name in kernels:
            us[name].append(limited(kernel_window, name, args.kernel_launches))
    params = eng.trainable_parameters()
    res = {"config": {"model": "vit_base_patch16_224_in21k", "depth": args.depth, "batch": args.batch, "rank": args.rank, "rho": args.rho,
                      "precision": args.precision, "steps_per_window": args.steps, "rounds": args.rounds,
                      "kernel_launches": args.kernel_launches, "tensors": len(params), "elements": sum(p.numel() for p in params),
                      "device": torch.cuda.get_device_name(dev)}}
    for unit, table in (("ms_per_step", ms), ("us_per_call", us)):
        for name, ts in table.items():
            res[name] = {unit: [round(t, 4) for t in ts], "median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                         "max": round(max(ts), 4), "spread": round(max(ts) - min(ts), 4)}
            print(f"{name:15s} {statistics.median(ts):9.4f} {unit.split('_')[0]} (min {min(ts):.4f}, max {max(ts):.4f})")
    res["sam_over_plain_eager"] = round(res["step+sam"]["median"] / res["step"]["median"], 4)
    res["sam_over_plain_graph"] = round(res["graph+sam"]["median"] / res["graph"]["median"], 4)
    res["last_loss"] = last
    res["skipped_steps"] = eng.skipped_steps
    print(json.dumps(res))


if __name__ == "__main__":
    main()
