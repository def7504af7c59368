#!/usr/bin/env python3
"""Time the training step of the headline configuration (ViT-B/16 + CaRA rank 16, batch 64, 224 px, DropPath 0.1, factored
adapters, AdamW) over a synthetic resident split of 1 000 uint8 images under its two feeds:

  batches   ResidentSplit.train_batches + CaraEngine.train_step: index upload, index_select, four normalisation passes, then
            the patch rows from the fp32 batch (under --graph also the copy of the batch into the graph's static input);
  resident  ResidentSplit.train_rows + CaraEngine.train_step_resident: one index upload per epoch, the patch rows straight
            from the uint8 pixels by index.

Eager and from a hipGraph (recipe.GraphedTrainStep).  The legs run interleaved in one process -- per round a window of
--steps steps of each, barrier + synchronize on both sides of a window, after --warmup steps of every leg -- and the line
printed says ms per step of each leg (median / min / max over the rounds) and the run-to-run spread of each.  Standalone:
not part of bench.py.

--augment runs other legs instead (the lines above are then not printed): the eager resident step as it is, the same step through
crop boxes (data.RandomResizedCropFlip on a 256-px split of the same images count: "resize 256, random-resized-crop 224"), and the
two patch-row kernels alone (cara_im2col_patches_u8_rows / cara_im2col_patches_u8_rows_crop at the step's output shape, device
events around --kernel-launches back-to-back launches), all interleaved round by round.

--mix adds to the --augment legs, interleaved with them in the same process: the augmented step with Mixup / CutMix tables
(data.MixupCutmix) and label smoothing 0.1, and cara_im2col_patches_u8_rows_mix alone on an identity table, a Mixup table and a
CutMix table.

--aug adds to the --mix legs: the mixed step with an all-zero colour table, with colour jitter alone and with jitter and Random
Erasing (data.ColorJitterErase), and cara_im2col_patches_u8_rows_aug alone (its two pre-pass launches included) on an all-zero
table, a jitter table and a jitter + erase table, each over the identity mix table.

--ra adds to the --aug legs: the cropped step with RandAugment tables (data.RandAugment) -- an identity table, geometric ops only,
lookup ops only, equalize on every sample, and everything (all ops, Mixup / CutMix, Random Erasing) -- and
cara_im2col_patches_u8_rows_ra alone on one drawn table of each kind (its pre-pass launches included, as the step runs them)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=60, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--legs", default="eager,graph")
    ap.add_argument("--augment", action="store_true", help="time the augmented resident step and the two patch-row kernels instead")
    ap.add_argument("--mix", action="store_true", help="the --augment legs plus the mixed step and the mix kernel alone")
    ap.add_argument("--aug", action="store_true", help="the --mix legs plus the jittered / erased steps and the aug kernels alone")
    ap.add_argument("--ra", action="store_true", help="the --aug legs plus the RandAugmented steps and the ra kernels alone")
    ap.add_argument("--source", type=int, default=256, help="--augment: side of the split the boxes are drawn on")
    ap.add_argument("--kernel-launches", type=int, default=200, help="--augment: launches per timed kernel window")
    args = ap.parse_args()
    import torch.distributed as dist
    from cara_amd import cara, create_model
    from cara_amd.data import ResidentSplit
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
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    gd = torch.Generator(device=dev).manual_seed(1)
    px = torch.randint(0, 256, (args.images, 3, 224, 224), generator=gd, dtype=torch.uint8, device=dev)
    y = torch.randint(0, 100, (args.images,), generator=gd, device=dev)
    split = ResidentSplit.from_tensors(px, y)

    def feeder(of_epoch):
        """the feed's items across epochs, as a training loop draws them"""
        epoch = 0
        while True:
            yield from of_epoch(epoch)
            epoch += 1

    if args.ra:
        args.aug = True
    if args.aug:
        args.mix = True
    if args.augment or args.mix:
        return augment_legs(args, eng, opt, split, feeder, dev, gd)
    gstep = GraphedTrainStep(eng, opt)

    def eager_batches(item):
        opt.advance()
        return eng.train_step(item[0], item[1], opt)

    def eager_resident(rows):
        opt.advance()
        return eng.train_step_resident(split, rows, opt)
    legs = {}
    for mode in args.legs.split(","):
        if mode == "eager":
            legs["eager/batches"] = (feeder(split.train_batches(args.batch)), eager_batches)
            legs["eager/resident"] = (feeder(split.train_rows(args.batch)), eager_resident)
        elif mode == "graph":
            legs["graph/batches"] = (feeder(split.train_batches(args.batch)), lambda item: gstep(item[0], item[1]))
            legs["graph/resident"] = (feeder(split.train_rows(args.batch)), lambda rows: gstep(split, rows))
        else:
            raise SystemExit(f"unknown leg {mode!r}")

    def fence():
        if dist.is_available() and dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize(dev)

    def window(name, steps):
        feed, step = legs[name]
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step(next(feed))
        fence()
        return (time.perf_counter() - t0) * 1e3 / steps, loss

    for name in legs:
        window(name, args.warmup)
    ms = {name: [] for name in legs}
    last = {}
    for _ in range(args.rounds):
        for name in legs:
            t, loss = window(name, args.steps)
            ms[name].append(t)
            last[name] = float(loss)
    res = {"config": {"model": "vit_base_patch16_224_in21k", "depth": args.depth, "batch": args.batch, "rank": args.rank,
                      "images": args.images, "precision": args.precision, "steps_per_window": args.steps, "rounds": args.rounds,
                      "warmup": args.warmup, "device": torch.cuda.get_device_name(dev)}}
    for name, ts in ms.items():
        med = statistics.median(ts)
        res[name] = {"ms_per_step": [round(t, 4) for t in ts], "median": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
                     "spread_ms": round(max(ts) - min(ts), 4), "last_loss": last[name]}
    for mode in args.legs.split(","):
        b, r = res[f"{mode}/batches"], res[f"{mode}/resident"]
        res[f"{mode}/resident_minus_batches_ms"] = round(r["median"] - b["median"], 4)
        res[f"{mode}/not_slower_within_batches_spread"] = bool(r["median"] - b["median"] <= b["spread_ms"])
    res["bad_rows"] = eng.resident_bad_rows()
    for name, v in ms.items():
        print(f"{name:15s} {statistics.median(v):8.4f} ms/step (min {min(v):.4f}, max {max(v):.4f})")
    print(json.dumps(res))


def augment_legs(args, eng, opt, split, feeder, dev, gd):
    from cara_amd import _lib as L
    from cara_amd.data import IMAGENET_MEAN, IMAGENET_STD, MixupCutmix, RandomResizedCropFlip, ResidentSplit, identity_mix
    from cara_amd.feed import Feed
    S, B = args.source, args.batch
    big = ResidentSplit.from_tensors(torch.randint(0, 256, (args.images, 3, S, S), generator=gd, dtype=torch.uint8, device=dev), split.labels)
    aug = RandomResizedCropFlip(224)

    def plain(rows):
        opt.advance()
        return eng.train_step_resident(split, rows, opt)

    def tabled(item, **kw):
        """the step on whatever tables the feed's item carries"""
        opt.advance()
        f = Feed.of(item)
        return eng.train_step_resident(big, f.rows, opt, **f.tables(), **kw)

    def smoothed(item):
        return tabled(item, label_smoothing=0.1)
    steps = {"eager/resident": (feeder(split.train_rows(B)), plain),
             f"eager/resident+crop{S}": (feeder(big.train_rows(B, augment=aug)), tabled)}
    # the kernels alone, on the rows and boxes of one drawn batch, into one patches buffer of the step's shape
    lib, dt = L.lib(args.precision), L.act_dtype(args.precision)
    rows, boxes = next(big.train_rows(B, augment=aug)(0))
    mean, std = torch.tensor(IMAGENET_MEAN, device=dev), torch.tensor(IMAGENET_STD, device=dev)
    patches = torch.empty(B * 196, 768, dtype=dt, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    st = L.stream(dev)

    def k_rows():
        L.check(lib.cara_im2col_patches_u8_rows(L.ptr(split.pixels), len(split), L.ptr(rows), L.ptr(mean), L.ptr(std), L.ptr(patches),
                                                L.ptr(bad), B, 3, 224, 224, 16, st), "cara_im2col_patches_u8_rows")

    def k_crop():
        L.check(lib.cara_im2col_patches_u8_rows_crop(L.ptr(big.pixels), len(big), S, S, L.ptr(rows), L.ptr(boxes), L.ptr(mean), L.ptr(std),
                                                     L.ptr(patches), L.ptr(bad), B, 3, 224, 224, 16, st), "cara_im2col_patches_u8_rows_crop")
    kernels = {"kernel/u8_rows": k_rows, f"kernel/u8_rows_crop{S}": k_crop}
    if args.mix:
        steps[f"eager/resident+crop{S}+mix"] = (feeder(big.train_rows(B, augment=aug, mix=MixupCutmix(224))), smoothed)
        rev = B - 1 - torch.arange(B, dtype=torch.int32)
        half = torch.tensor(0.5).view(torch.int32).item()
        mixup, cutmix = identity_mix(B), identity_mix(B)
        mixup[:, 0], mixup[:, 5], mixup[:, 6] = rev, half, half
        cutmix[:, 0], cutmix[:, 6] = rev, half
        cutmix[:, 1:5] = torch.tensor([33, 33, 158, 158], dtype=torch.int32)       # half of the 224 x 224 output, on no tile edge
        for name, t in (("identity", identity_mix(B)), ("mixup", mixup), ("cutmix", cutmix)):
            t = t.to(dev)

            def k_mix(t=t):
                L.check(lib.cara_im2col_patches_u8_rows_mix(L.ptr(big.pixels), len(big), S, S, L.ptr(rows), L.ptr(boxes), L.ptr(t), L.ptr(mean),
                                                            L.ptr(std), L.ptr(patches), L.ptr(bad), B, 3, 224, 224, 16, st),
                        "cara_im2col_patches_u8_rows_mix")
            kernels[f"kernel/u8_rows_mix{S}/{name}"] = k_mix
    if args.aug:
        from cara_amd.data import ColorJitterErase, identity_aug
        zero_color = type("ZeroColor", (), {"Hi": 224, "Wi": 224, "draw": staticmethod(lambda B_, steps, generator: identity_aug(B_, steps))})()
        jitter, full = ColorJitterErase(224, erase_prob=0.0), ColorJitterErase(224)

        for name, c in (("aug0", zero_color), ("jitter", jitter), ("jitter+erase", full)):
            steps[f"eager/resident+crop{S}+mix+{name}"] = (feeder(big.train_rows(B, augment=aug, mix=MixupCutmix(224), color=c)), smoothed)
        ident = identity_mix(B).to(dev)
        stat = torch.empty(int(lib.cara_aug_stat_bytes(B)) // 4, device=dev)
        gk = torch.Generator().manual_seed(9)
        for name, t in (("zero", identity_aug(B)), ("jitter", jitter.draw(B, 1, gk)[0]), ("jitter+erase", ColorJitterErase(224, erase_prob=1.0).draw(B, 1, gk)[0])):
            t = t.contiguous().to(dev)

            def k_aug(t=t):
                L.check(lib.cara_im2col_patches_u8_rows_aug(L.ptr(big.pixels), len(big), S, S, L.ptr(rows), L.ptr(boxes), L.ptr(ident), L.ptr(t),
                                                            L.ptr(stat), L.ptr(mean), L.ptr(std), L.ptr(patches), L.ptr(bad), B, 3, 224, 224, 16, st),
                        "cara_im2col_patches_u8_rows_aug")
            kernels[f"kernel/u8_rows_aug{S}/{name}"] = k_aug
    if args.ra:
        from cara_amd.data import ColorJitterErase, RandAugment, identity_ra
        GEO, LOOK = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"), ("Posterize", "Solarize", "SolarizeAdd", "Invert")
        ident_ra = type("IdentityRa", (), {"Hi": 224, "Wi": 224, "draw": staticmethod(
            lambda B_, steps, generator: (identity_ra(B_, steps), torch.zeros(steps, B_, 6, dtype=torch.int32)))})()
        kinds = (("ra0", ident_ra), ("geometry", RandAugment(224, prob=1.0, ops=GEO)), ("lookup", RandAugment(224, prob=1.0, ops=LOOK)),
                 ("equalize", RandAugment(224, n=1, prob=1.0, ops=("Equalize",))))

        for name, r in kinds:
            steps[f"eager/resident+crop{S}+{name}"] = (feeder(big.train_rows(B, augment=aug, rand=r)), smoothed)
        steps[f"eager/resident+crop{S}+mix+erase+ra"] = (feeder(big.train_rows(B, augment=aug, mix=MixupCutmix(224),
                                                                               color=ColorJitterErase(224, 0.0, 0.0, 0.0), rand=RandAugment(224))),
                                                         smoothed)
        ra_scratch = torch.empty(int(lib.cara_ra_stat_bytes(B)) // 4, dtype=torch.int32, device=dev)
        stat_ra = torch.empty(int(lib.cara_aug_stat_bytes(B)) // 4, device=dev)
        gr = torch.Generator().manual_seed(10)
        for name, r in kinds + (("all", RandAugment(224)),):
            t, slots = r.draw(B, 1, gr)
            t = t[0].contiguous().to(dev)
            a = identity_aug(B)
            a[:, :6] = slots[0]
            a = a.contiguous().to(dev) if name == "all" else None

            def k_ra(t=t, a=a):
                L.check(lib.cara_im2col_patches_u8_rows_ra(L.ptr(big.pixels), len(big), S, S, L.ptr(rows), L.ptr(boxes), None, L.ptr(a),
                                                           L.ptr(stat_ra) if a is not None else None, L.ptr(t), L.ptr(ra_scratch), None, 0,
                                                           L.ptr(mean), L.ptr(std), L.ptr(patches), L.ptr(bad), B, 3, 224, 224, 16, st),
                        "cara_im2col_patches_u8_rows_ra")
            kernels[f"kernel/u8_rows_ra{S}/{name}"] = k_ra

    def step_window(name, n):
        feed, step = steps[name]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            loss = step(next(feed))
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
        step_window(name, args.warmup)
    for name in kernels:
        kernel_window(name, 20)
    ms, us, last = {n: [] for n in steps}, {n: [] for n in kernels}, {}
    for _ in range(args.rounds):
        for name in steps:
            t, last[name] = step_window(name, args.steps)
            ms[name].append(t)
        for name in kernels:
            us[name].append(kernel_window(name, args.kernel_launches))
    res = {"config": {"model": "vit_base_patch16_224_in21k", "depth": args.depth, "batch": B, "rank": args.rank, "images": args.images,
                      "source": S, "precision": args.precision, "steps_per_window": args.steps, "rounds": args.rounds,
                      "kernel_launches": args.kernel_launches, "device": torch.cuda.get_device_name(dev)}}
    for unit, table in (("ms_per_step", ms), ("us_per_launch", us)):
        for name, ts in table.items():
            res[name] = {unit: [round(t, 4) for t in ts], "median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                         "max": round(max(ts), 4), "spread": round(max(ts) - min(ts), 4)}
            print(f"{name:32s} {statistics.median(ts):9.4f} {unit.split('_')[0]} (min {min(ts):.4f}, max {max(ts):.4f})")
    a, b = res["eager/resident"], res[f"eager/resident+crop{S}"]
    res["crop_minus_plain_ms"] = round(b["median"] - a["median"], 4)
    res["crop_not_slower_within_plain_spread"] = bool(b["median"] - a["median"] <= a["spread"])
    if args.mix:
        res["mix_minus_crop_ms"] = round(res[f"eager/resident+crop{S}+mix"]["median"] - b["median"], 4)
    res["last_loss"] = last
    res["bad_rows"] = eng.resident_bad_rows()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
