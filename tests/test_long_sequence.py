"""Image sizes above 384 px: ViT-B/16 at 448 px (785 tokens), 512 px (1 025) and 768 px (2 305) -- more tokens than a head's K / V
image fits in LDS (608), served by the streamed attention kernels.  The workspace layout is host code and is checked without a
GPU; the whole-model, train-step and module-level cases follow their 224-px counterparts in tests/test_model_gpu.py with the
same bounds (tests/tolerances.py), the oracle computed live on the CPU."""
import ctypes as C

import pytest
import torch

DEV = "cuda"


def _workspace_bytes(img, batch=2, depth=2, dim=768, heads=12, rank=16, Rp=32):
    from cara_amd import _lib
    geom = _lib.Geom(depth, dim, heads, rank, Rp, 0.1, 4)
    shape = _lib.VitShape(batch, img, 16, 3, (img // 16) ** 2 + 1, 100, 1e-6, 0, 0.1, 0)
    return int(_lib.lib().cara_vit_workspace_bytes(C.byref(geom), C.byref(shape)))


def test_workspace_layout_accepts_more_than_608_tokens():
    """cara_vit_workspace_bytes (0 = refused geometry) for ViT-B geometry, depth 2, Rp 32, batch 2."""
    sizes = [_workspace_bytes(img) for img in (448, 512, 768)]          # 785, 1 025, 2 305 tokens
    assert all(s > 0 for s in sizes), sizes
    assert sizes[0] < sizes[1] < sizes[2], sizes
    # existing shapes keep their workspace: 577 tokens (384 px) as before the token limit was lifted
    assert _workspace_bytes(384) == 154016256
    assert _workspace_bytes(384) < sizes[0]
    # what the layout still refuses: a token count that does not match the image, a head dim other than 64
    from cara_amd import _lib
    geom = _lib.Geom(2, 768, 12, 16, 32, 0.1, 4)
    bad = _lib.VitShape(2, 448, 16, 3, 786, 100, 1e-6, 0, 0.1, 0)
    assert _lib.lib().cara_vit_workspace_bytes(C.byref(geom), C.byref(bad)) == 0
    assert _workspace_bytes(448, heads=8) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("img,batch,precision", [(448, 2, "bf16"), (448, 2, "fp16"), (512, 3, "bf16")])
def test_whole_model_above_608_tokens(img, batch, precision):
    """Depth 2, rank 16 against the oracle: logits through check_logits, every CP gradient below grad_bar.  (512 px runs in bf16
    only: the fp32 top-2 margins of these inputs are 0.008 / 0.02 / 0.22 there, too thin for the fp16 branch's unfiltered
    "every class index equal"; the bf16 branch filters by margin.)"""
    from oracle import cara_oracle as O
    from tests.test_model_gpu import build, check_logits, grad_bar, rel
    depth, rank = 2, 16
    w = O.synthetic_backbone(depth=depth, img=img)
    cp = O.synthetic_cp(rank=rank, depth=depth)
    x, y = O.synthetic_batch(batch=batch, img=img)
    m = build(w, cp, rank, 0.1, depth, img, precision=precision).eval()
    logits = m(x.to(DEV))
    with torch.no_grad():
        ref = O.vit_cara_forward(x, w, cp, s=0.1, depth=depth)
        sim = O.vit_cara_forward(x, w, cp, s=0.1, depth=depth, factored=True, bf16_sim=True)
    check_logits(logits, ref, sim, precision, f"rank {rank}, {img} px ({(img // 16) ** 2 + 1} tokens), batch {batch}")
    torch.nn.functional.cross_entropy(logits, y.to(DEV)).backward()
    head = {"weight": w["head.weight"], "bias": w["head.bias"]}
    _, _, gref = O.train_step_as_written(x, y, w, cp, head, s=0.1, depth=depth)
    worst = max(rel(getattr(m, n).grad, gref[n]) for n in O.CP_NAMES)
    print(f"rank {rank}, {img} px [{precision}]: worst CP gradient {worst:.2e}")
    assert worst < grad_bar(precision), worst


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_train_step_at_448_px_against_oracle(precision):
    """engine.train_step at 785 tokens, batch 2, depth 2, train mode with given DropPath masks: loss and p.grad of every trainable
    tensor against fp32 autograd of the as-written algorithm with the same masks (the body and bounds of
    test_train_step_against_oracle)."""
    from oracle import cara_oracle as O
    from tests.test_model_gpu import _keep, build, check_logits, grad_bar, rel
    depth, B, img = 2, 2, 448
    w = O.synthetic_backbone(depth=depth, img=img)
    cp = O.synthetic_cp(rank=16, depth=depth)
    x, y = O.synthetic_batch(batch=B, img=img)
    m = build(w, cp, 16, 0.1, depth, img, precision=precision).train()
    eng = m._cara_engine
    keep = _keep(depth, B)
    loss = eng.train_step(x.to(DEV), y.to(DEV), None, droppath=keep.to(DEV))
    cps = dict(cp)
    cps["CP_A1"], cps["CP_P1"] = cp["CP_A1"][:3 * depth], cp["CP_P1"][:9 * depth]
    head = {"weight": w["head.weight"], "bias": w["head.bias"]}
    rloss, rlogits, gref = O.train_step_as_written(x, y, w, cps, head, s=0.1, depth=depth, drop_path_keep=keep)
    assert abs(loss.item() - rloss.item()) < (5e-4 if precision == "fp16" else 5e-3) * max(1.0, abs(rloss.item())), (loss.item(), rloss.item())
    if precision == "fp16":
        with torch.no_grad():
            check_logits(eng.forward(x.to(DEV), droppath=keep.to(DEV)), rlogits, None, precision, "train-mode forward, 448 px")
    worst = 0.0
    for n in O.CP_NAMES:
        p_ = getattr(m, n)
        assert p_.grad is not None
        worst = max(worst, rel(p_.grad, gref[n]))
    print(f"train_step 448 px [{precision}]: loss {loss.item():.5f} vs oracle {rloss.item():.5f}; worst CP-gradient rel-L2 {worst:.2e}")
    assert worst < grad_bar(precision)
    assert rel(m.head.weight.grad, gref["head.weight"]) < grad_bar(precision) and rel(m.head.bias.grad, gref["head.bias"]) < grad_bar(precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_module_level_attention_at_785_tokens(precision):
    """blocks[0].attn called on its own with x [2, 785, 768]: no refusal, output against the oracle's attn_as_written (fp64)
    within the block-level bound of test_module_level_forwards_against_reference_vectors for the precision, dX likewise."""
    from oracle import cara_oracle as O
    from tests.test_model_gpu import build, rel
    depth, img, S = 2, 448, 0.1
    w = O.synthetic_backbone(depth=depth, img=img)
    cp = O.synthetic_cp(rank=16, depth=depth)
    m = build(w, cp, 16, S, depth, img, precision=precision).eval()
    bar_y, bar_gx = (1.5e-3, 3e-3) if precision == "fp16" else (1e-2, 2e-2)
    x = torch.randn(2, 785, 768, generator=torch.Generator().manual_seed(5))
    a_idx, a_aidx, _ = O.block_indices(depth)[0]
    xd = x.to(DEV).requires_grad_(True)
    y = m.blocks[0].attn.forward(xd)
    d = lambda t: t.double()  # noqa: E731
    p = "blocks.0."
    cpv = {k: d(v) for k, v in cp.items()}
    xr = d(x).clone().requires_grad_(True)
    yr = O.attn_as_written(xr, cpv, d(w[p + "attn.qkv.weight"]), d(w[p + "attn.qkv.bias"]), d(w[p + "attn.proj.weight"]),
                           d(w[p + "attn.proj.bias"]), attn_idx=a_aidx, idx=a_idx, s=S, num_heads=12, scale=64 ** -0.5)
    r = rel(y, yr.detach())
    print(f"module attn, 785 tokens [{precision}]: rel-L2 vs the as-written oracle {r:.2e}")
    assert tuple(y.shape) == (2, 785, 768) and r < bar_y, r
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
    y.backward(gy.to(DEV))
    yr.backward(d(gy))
    rg = rel(xd.grad, xr.grad)
    print(f"module attn, 785 tokens [{precision}]: dX rel-L2 {rg:.2e}")
    assert rg < bar_gx, rg
