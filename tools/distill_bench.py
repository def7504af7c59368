#!/usr/bin/env python3
"""What knowledge distillation costs in the training step of the headline configuration (ViT-B/16 + CaRA rank 16, batch 64, 224 px,
DropPath 0.1, factored adapters, AdamW), on one GPU:

  step            CaraEngine.train_step as it is (the yardstick: the plain step on the same box, in the same run);
  step+tensor     the same step with distill=Distill(<recorded logits>): no teacher pass, cara_distill_loss in the loss's place;
  step+ema        distill=Distill(<the step's own ParamEma>) with ema=: the mean teacher, one inference forward more;
  step+model      distill=Distill(<a rank --teacher-rank cara() model>): one inference forward through the teacher's engine;
  graph, graph+tensor, graph+ema, graph+model: the same four replayed from a hipGraph each (recipe.GraphedTrainStep);
  forward         the inference forward alone (what a teacher pass runs: need_backward = False, no DropPath), for the expectation
                  "a distilled step costs a step plus one forward";
  kernel/mix C, kernel/distill C: cara_cross_entropy_mix and cara_distill_loss (soft, alpha 0.5, T 2) alone on [batch, C] logits,
                  C = 100 and 1000, --kernel-launches back-to-back calls replayed from a captured graph between device events.

The legs run interleaved in one process, round by round, after --warmup steps of each; the line printed says the median / min / max
over the rounds.  Every timed window runs under its own time limit (--window-timeout seconds: the process dumps its stacks and
exits when a window does not come back), and nothing is tried twice.  Standalone: not part of bench.py."""
import argparse
import ctypes as C
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
    ap.add_argument("--teacher-rank", type=int, default=64)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--kernel-launches", type=int, default=200)
    ap.add_argument("--window-timeout", type=float, default=120.0)
    args = ap.parse_args()
    from cara_amd import _lib as L
    from cara_amd import cara, create_model
    from cara_amd.feed import Feed
    from cara_amd.loss import Distill
    from cara_amd.optim import AdamW
    from cara_amd.recipe import GraphedTrainStep
    dev = torch.device("cuda", 0)
    torch.manual_seed(14)

    def build(rank):
        m = create_model("vit_base_patch16_224_in21k", depth=args.depth, num_classes=100, drop_path_rate=0.1)
        m = cara({"model": m, "rank": rank, "scale": 0.1, "l_mu": 1.5, "l_std": 0.1, "precision": args.precision})
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():   # non-zero adapters, as bench.py's model
            m.CP_A2.copy_(0.05 * torch.randn(m.CP_A2.shape, generator=g))
            m.CP_P2.copy_(0.05 * torch.randn(m.CP_P2.shape, generator=g))
        return m.to(dev)
    m = build(args.rank).train()
    teacher = build(args.teacher_rank).eval()
    eng = m._cara_engine
    eng.seed_rank_streams(2024, 0)
    for n, p in m.named_parameters():
        p.requires_grad = "CP" in n or "head" in n
    # (one capturable AdamW and one capturable average for all legs: the eager ones advance them by hand, as GraphedTrainStep does)
    opt = AdamW(eng.trainable_parameters(), lr=1e-4, weight_decay=1e-4, capturable=True)
    ema = eng.make_ema(0.999, capturable=True)
    gd = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(args.batch, 3, 224, 224, generator=gd, device=dev)
    y = torch.randint(0, 100, (args.batch,), generator=gd, device=dev)
    recorded = torch.randn(args.batch, 100, generator=gd, device=dev)
    kd = dict(alpha=args.alpha, temperature=args.temperature)
    legs = {"": {}, "+tensor": {"distill": Distill(recorded, **kd)}, "+ema": {"distill": Distill(ema, **kd), "ema": ema},
            "+model": {"distill": Distill(teacher, **kd)}}
    graphed = {name: GraphedTrainStep(eng, opt, **kw) for name, kw in legs.items()}

    def eager(kw):
        opt.advance()
        if "ema" in kw:
            ema.advance()
        return eng.train_step(x, y, opt, **kw)

    def forward_only():
        cp, hw, hb = eng._forward_weights(m, dev, None)
        with torch.no_grad():
            return eng._run_forward_on(m, x, Feed(None), None, hw, hb, cp, False, dev, teacher=True)[0, 0]
    steps = {"step" + name: (lambda kw=kw: eager(kw)) for name, kw in legs.items()}
    steps.update({"graph" + name: (lambda gs=gs: gs(x, y)) for name, gs in graphed.items()})
    steps["forward"] = forward_only

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
    # the two loss entries alone: --kernel-launches calls captured into one graph each, replayed between events
    lib, ptr, f = eng._lib(), L.ptr, C.c_float
    kernels = {}
    for ncls in (100, 1000):
        z = torch.randn(args.batch, ncls, generator=gd, device=dev)
        t = torch.randn(args.batch, ncls, generator=gd, device=dev)
        yk = torch.randint(0, ncls, (args.batch,), generator=gd, device=dev)
        loss, dl = torch.empty(1 + args.batch, device=dev), torch.empty(args.batch, ncls, device=dev)

        def mix_call(z=z, yk=yk, loss=loss, dl=dl, ncls=ncls):
            return lib.cara_cross_entropy_mix(ptr(z), ptr(yk), None, f(0.1), ptr(loss), ptr(dl), args.batch, ncls, f(1.0), None, None, L.stream(dev))

        def kd_call(z=z, t=t, yk=yk, loss=loss, dl=dl, ncls=ncls):
            return lib.cara_distill_loss(ptr(z), ptr(t), ptr(yk), None, f(0.1), f(args.alpha), f(args.temperature), 0, ptr(loss), ptr(dl),
                                         args.batch, ncls, f(1.0), None, None, L.stream(dev))
        for kname, call in ((f"kernel/mix {ncls}", mix_call), (f"kernel/distill {ncls}", kd_call)):
            call()
            torch.cuda.synchronize(dev)
            gr, side, bad = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev), 0
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                with torch.cuda.graph(gr, stream=side):
                    for _ in range(args.kernel_launches):
                        bad |= call()
            torch.cuda.current_stream(dev).wait_stream(side)
            if bad:
                raise SystemExit(f"{kname}: a call returned status {bad}")
            kernels[kname] = (gr, (z, t, yk, loss, dl))

    def kernel_window(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kernels[name][0].replay()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / args.kernel_launches      # us per call (two launches each)
    for name in kernels:
        limited(kernel_window, name)
    ms, us, last = {n: [] for n in steps}, {n: [] for n in kernels}, {}
    for _ in range(args.rounds):
        for name in steps:
            t_, last[name] = limited(step_window, name, args.steps)
            ms[name].append(t_)
        for name in kernels:
            us[name].append(limited(kernel_window, name))
    res = {"config": {"model": "vit_base_patch16_224_in21k", "depth": args.depth, "batch": args.batch, "rank": args.rank,
                      "teacher_rank": args.teacher_rank, "alpha": args.alpha, "temperature": args.temperature, "precision": args.precision,
                      "steps_per_window": args.steps, "rounds": args.rounds, "kernel_launches": args.kernel_launches,
                      "device": torch.cuda.get_device_name(dev)}}
    for unit, table in (("ms_per_step", ms), ("us_per_call", us)):
        for name, ts in table.items():
            res[name] = {unit: [round(v, 4) for v in ts], "median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                         "max": round(max(ts), 4), "spread": round(max(ts) - min(ts), 4)}
            print(f"{name:20s} {statistics.median(ts):9.4f} {unit.split('_')[0]} (min {min(ts):.4f}, max {max(ts):.4f})")
    fwd = res["forward"]["median"]
    for how in ("step", "graph"):
        for name in ("+tensor", "+ema", "+model"):
            res[f"{how}{name}_minus_plain_over_forward"] = round((res[how + name]["median"] - res[how]["median"]) / fwd, 4)
    del last["forward"]
    res["last_loss"] = last
    res["skipped_steps"] = eng.skipped_steps
    print(json.dumps(res))


if __name__ == "__main__":
    main()
