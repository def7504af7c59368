#!/usr/bin/env python3
"""What the weight EMA costs in the training step of the headline configuration (ViT-B/16 + CaRA rank 16, batch 64, 224 px,
DropPath 0.1, factored adapters, AdamW), on one GPU:

  step            CaraEngine.train_step as it is;
  step+ema        the same step with ema= (cara_ema_update: one more launch in the tail);
  kernel/ema      cara_ema_update alone over the 14 trainable tensors, device events around --kernel-launches back-to-back launches;
  torch/lerp      torch._foreach_lerp_ over the same 14 tensors, the same way: the yardstick.

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
    ap.add_argument("--steps", type=int, default=60, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--kernel-launches", type=int, default=500)
    ap.add_argument("--window-timeout", type=float, default=120.0)
    args = ap.parse_args()
    from cara_amd import cara, create_model
    from cara_amd.optim import AdamW
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
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    ema = eng.make_ema(0.9998)
    gd = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(args.batch, 3, 224, 224, generator=gd, device=dev)
    y = torch.randint(0, 100, (args.batch,), generator=gd, device=dev)
    params = [p.detach() for p in eng.trainable_parameters()]
    lerp_shadow = [p.clone() for p in params]
    steps = {"step": lambda: eng.train_step(x, y, opt), "step+ema": lambda: eng.train_step(x, y, opt, ema=ema)}
    kernels = {"kernel/ema": ema.update, "torch/lerp": lambda: torch._foreach_lerp_(lerp_shadow, params, 2e-4)}

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

    def kernel_window(name, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            kernels[name]()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / n      # us per launch
    for name in steps:
        limited(step_window, name, args.warmup)
    for name in kernels:
        limited(kernel_window, name, 20)
    ms, us, last = {n: [] for n in steps}, {n: [] for n in kernels}, {}
    for _ in range(args.rounds):
        for name in steps:
            t, last[name] = limited(step_window, name, args.steps)
            ms[name].append(t)
        for name in kernels:
            us[name].append(limited(kernel_window, name, args.kernel_launches))
    res = {"config": {"model": "vit_base_patch16_224_in21k", "depth": args.depth, "batch": args.batch, "rank": args.rank,
                      "precision": args.precision, "steps_per_window": args.steps, "rounds": args.rounds,
                      "kernel_launches": args.kernel_launches, "tensors": len(params), "elements": sum(p.numel() for p in params),
                      "device": torch.cuda.get_device_name(dev)}}
    for unit, table in (("ms_per_step", ms), ("us_per_launch", us)):
        for name, ts in table.items():
            res[name] = {unit: [round(t, 4) for t in ts], "median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                         "max": round(max(ts), 4), "spread": round(max(ts) - min(ts), 4)}
            print(f"{name:12s} {statistics.median(ts):9.4f} {unit.split('_')[0]} (min {min(ts):.4f}, max {max(ts):.4f})")
    res["ema_minus_plain_us"] = round((res["step+ema"]["median"] - res["step"]["median"]) * 1e3, 2)
    res["last_loss"] = last
    res["ema_updates"] = ema.num_updates
    print(json.dumps(res))


if __name__ == "__main__":
    main()
