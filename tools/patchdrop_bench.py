#!/usr/bin/env python3
"""What a patch dropout buys in the training step of the headline configuration (ViT-B/16 + CaRA rank 16, batch 64, 224 px,
DropPath 0.1, factored adapters, AdamW; eager launches), on one GPU:

  K=196            CaraEngine.train_step as it is (no table);
  K=196/identity   the same step with keep = identity_keep: the keep kernels on every patch (the cost of the table itself);
  K=147, 98, 49    train_step(..., keep=) on a table of data.PatchDropout (a fresh step's view per call).

Each leg runs eager (CaraEngine.train_step) and graphed (recipe.GraphedTrainStep: the table is a static input; "graph:" legs).
The legs run interleaved in one process, round by round, after --warmup steps of each, every leg on a workspace of its own
(the token count is part of the engine's workspace key); the line printed says the median / min / max over the rounds.  Behind the
timed rounds every eager leg runs --site-steps steps with the event brackets of cara_profile_sites around every call site of
the forward and backward: ms per step and site, which says where the step stops shrinking with the token count (bracketed steps
are slower: every bracket idles the chip).  Every timed window runs under its own time limit (--window-timeout seconds: the
process dumps its stacks and exits when a window does not come back), and nothing is tried twice.  Standalone: not part of
bench.py.  --root DIR imports cara_amd from another checkout (with --keeps none --no-identity: the full step of a tree that has
no keep tables, for a comparison on the same box)."""
import argparse
import ctypes as C
import faulthandler
import json
import os
import statistics
import sys
import time

import torch  # noqa: E402

SITES = ["qkv_fwd", "proj_fwd", "fc1_fwd", "fc2_fwd", "qkv_bwd", "proj_bwd", "fc1_bwd", "fc2_bwd", "attn_fwd", "attn_bwd",
         "ln1_fwd", "ln2_fwd", "ln1_bwd", "ln2_bwd", "skinny_fwd", "skinny_bwd"]   # include/cara_hip.h CARA_SITE_*


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--keeps", default="147,98,49")
    ap.add_argument("--window-timeout", type=float, default=120.0)
    ap.add_argument("--no-identity", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--site-steps", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from cara_amd import _lib, cara, create_model
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
    eng._keep_ws = True   # every leg keeps its workspace: the legs alternate
    for n, p in m.named_parameters():
        p.requires_grad = "CP" in n or "head" in n
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    gstep = GraphedTrainStep(eng, opt)
    gd = torch.Generator(device=dev).manual_seed(1)
    B, P = args.batch, 196
    x = torch.randn(B, 3, 224, 224, generator=gd, device=dev)
    y = torch.randint(0, 100, (B,), generator=gd, device=dev)
    eager = {"K=196": None}
    if not args.no_identity:
        from cara_amd.data import identity_keep
        eager["K=196/identity"] = identity_keep(B, P, steps=1).to(dev)
    for K in (int(v) for v in args.keeps.split(",") if v.strip().isdigit()):
        from cara_amd.data import PatchDropout, check_keep
        t = PatchDropout(1.0 - (K + 0.5) / P).draw(P, B, 8, torch.Generator().manual_seed(K))
        assert t.shape[-1] == K, (K, t.shape)
        check_keep(t, B, P)
        eager[f"K={K}"] = t.to(dev)
    tables = dict(eager)
    if not args.no_graph:
        tables.update({"graph:" + n: t for n, t in eager.items()})
    count = {n: 0 for n in tables}

    def step(name):
        t = tables[name]
        count[name] += 1
        kw = {} if t is None else {"keep": t[count[name] % t.shape[0]]}
        if name.startswith("graph:"):
            return gstep(x, y, **kw)
        opt.advance()
        return eng.train_step(x, y, opt, **kw)

    def limited(fn, *a):
        faulthandler.dump_traceback_later(args.window_timeout, exit=True)
        try:
            return fn(*a)
        finally:
            faulthandler.cancel_dump_traceback_later()

    def window(name, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            loss = step(name)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / n, float(loss)
    for name in tables:
        limited(window, name, args.warmup)
    ms, last = {n: [] for n in tables}, {}
    for _ in range(args.rounds):
        for name in tables:
            t, last[name] = limited(window, name, args.steps)
            ms[name].append(t)
    res = {"config": {"model": "vit_base_patch16_224_in21k", "depth": args.depth, "batch": B, "rank": args.rank, "precision": args.precision,
                      "launch": "eager and graph:", "steps_per_window": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}}
    for name, ts in ms.items():
        base = statistics.median(ms["graph:K=196" if name.startswith("graph:") else "K=196"])
        med = statistics.median(ts)
        res[name] = {"ms_per_step": [round(t, 4) for t in ts], "median": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
                     "vs_full": round(med / base, 4)}
        print(f"{name:15s} {med:8.4f} ms (min {min(ts):.4f}, max {max(ts):.4f}) = {med / base:.3f} x the full step")
    # per-site time of the eager legs: event brackets around every call site, --site-steps steps each
    lib = _lib.lib(args.precision)
    sites = {}
    for name in eager:
        if args.site_steps <= 0:
            break
        _lib.check(lib.cara_profile_sites(C.c_ulonglong((1 << len(SITES)) - 1), 1), "cara_profile_sites")
        limited(window, name, args.site_steps)
        row = {}
        for i, sname in enumerate(SITES):
            avg, mark, cnt = C.c_float(0), C.c_float(0), C.c_int(0)
            _lib.check(lib.cara_profile_site_read(i, C.byref(avg), C.byref(mark), C.byref(cnt)), "cara_profile_site_read")
            if cnt.value > 0:
                row[sname] = round(avg.value * cnt.value / args.site_steps, 4)
        lib.cara_profile_sites(C.c_ulonglong(0), 1)
        row["sum"] = round(sum(row.values()), 4)
        sites[name] = row
        print(f"sites {name:15s} " + " ".join(f"{k}={v:.3f}" for k, v in row.items()))
    res["site_ms_per_step"] = sites
    res["last_loss"] = last
    res["bad_entries"] = eng.resident_bad_rows()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
