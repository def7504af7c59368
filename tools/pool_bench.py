#!/usr/bin/env python3
"""What the mean-pooled readout (global_pool = "avg" + fc_norm) costs in the training step of the headline configuration (ViT-B/16 +
CaRA rank 16, batch 64, 224 px, DropPath 0.1, factored adapters, AdamW), on one GPU.  One leg per process -- the library reads its
switches once, and the yardstick is the token step under CARA_CLS_SHORTCUT=0 (the same full last block) -- so a caller alternates
processes:

  --leg token     CaraEngine.train_step of the token-readout model (run it with CARA_CLS_SHORTCUT=0 for the yardstick);
  --leg pooled    the same step of the pooled model;
  --leg kernels   cara_token_mean and cara_token_mean_bwd alone at [batch, 197, 768]: --kernel-launches back-to-back launches between
                  device events, and the bytes each must move over that time against the HBM roof (MI355X: 8 TB/s).

Every leg prints one JSON line: median / min / max over --rounds windows of --steps steps behind --warmup steps.  Standalone: not part
of bench.py."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_ROOF = 8.0e12   # bytes/s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["token", "pooled", "kernels"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--kernel-launches", type=int, default=200)
    args = ap.parse_args()
    from cara_amd import _lib as L
    from cara_amd import cara, create_model
    from cara_amd.optim import AdamW
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(14)
    out = {"leg": args.leg, "batch": args.batch, "precision": args.precision, "cls_shortcut": os.environ.get("CARA_CLS_SHORTCUT", "1")}

    def window(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    def stats(ms):
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    if args.leg == "kernels":
        lib = L.lib(args.precision)
        B, N, D = args.batch, 197, 768
        x = torch.randn(B, N, D, device=dev)
        pooled, dpool = torch.empty(B, D, device=dev), torch.randn(B, D, device=dev)
        dx, dyb = torch.empty(B, N, D, device=dev), torch.empty(B, N, D, dtype=L.act_dtype(args.precision), device=dev)
        scale = torch.full((B,), 1 / 0.9, device=dev)
        st = L.stream(dev)
        calls = {
            "cara_token_mean": (lambda: L.check(lib.cara_token_mean(L.ptr(x), B, N, 1, D, L.ptr(pooled), st), "cara_token_mean"),
                                B * (N - 1) * D * 4 + B * D * 4),
            "cara_token_mean_bwd": (lambda: L.check(lib.cara_token_mean_bwd(L.ptr(dpool), L.ptr(scale), B, N, 1, D, L.ptr(dx), L.ptr(dyb), 0, st),
                                                    "cara_token_mean_bwd"), B * D * 4 + B * N * D * (4 + 2)),
            # what the pooled backward replaces on the CARA_CLS_SHORTCUT=0 path: the two memsets (the cls-row LayerNorm backward stays, on pooled rows)
            "memsets": (lambda: (dx.zero_(), dyb.zero_()), B * N * D * (4 + 2)),
        }
        for name, (fn, nbytes) in calls.items():
            window(fn, 20)
            s = stats([window(fn, args.kernel_launches) for _ in range(args.rounds)])
            out[name] = dict(s, bytes=nbytes, bytes_per_s=nbytes / (s["median_ms"] * 1e-3), share_of_hbm_roof=nbytes / (s["median_ms"] * 1e-3) / HBM_ROOF)
        print(json.dumps(out))
        return

    pool = {"global_pool": "avg"} if args.leg == "pooled" else {}   # (the token leg also runs against a library and package without the feature)
    m = create_model("vit_base_patch16_224_in21k", depth=args.depth, num_classes=100, drop_path_rate=0.1, **pool)
    m = cara({"model": m, "rank": args.rank, "scale": 0.1, "l_mu": 1.5, "l_std": 0.1, "precision": args.precision})
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():   # non-zero adapters, as bench.py's model
        m.CP_A2.copy_(0.05 * torch.randn(m.CP_A2.shape, generator=g))
        m.CP_P2.copy_(0.05 * torch.randn(m.CP_P2.shape, generator=g))
    m = m.to(dev).train()
    eng = m._cara_engine
    eng.seed_rank_streams(2024, 0)
    opt = AdamW(eng.trainable_parameters(), lr=1e-4, weight_decay=1e-4)
    gd = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(args.batch, 3, 224, 224, generator=gd, device=dev)
    y = torch.randint(0, 100, (args.batch,), generator=gd, device=dev)
    step = lambda: eng.train_step(x, y, opt)   # noqa: E731
    window(step, args.warmup)
    out.update(stats([window(step, args.steps) for _ in range(args.rounds)]))
    out["loss"] = float(step())
    out["workspace_bytes"] = int(sum(st["ws"].numel() for st in eng._ws.values()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
