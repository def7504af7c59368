"""Host proof of oracle.cara_oracle.backward_rounding_model / block_rounding_model, the float64 restatement of the factored train
step with the device's rounding points that tests/test_backward_contract_gpu.py measures the device against.

* identity: with no rounding the hand-written backward IS float64 autograd of the as-written algorithm (1e-9 rel-L2): ranks 16 and
  64, cp_length 3 / 4 / 5, DropPath masks with dropped samples; and its forward is vit_cara_forward(factored, sim_dtype);
* premise: with bf16 and with fp16 rounding the model ALONE sits inside the existing gradient bars divided by LOGITS_VS_MODEL, for
  every part at every shape of the device module -- otherwise "device error <= 1.15 x model error" could ask less than CP_GRAD does;
* sensitivity: the model with one rounding point left out against the committed model, per tensor (printed; docs/findings/
  backward_contract.md holds the tables).  No GPU."""
import functools

import pytest
import torch

from oracle import cara_oracle as O
from tests import tolerances as T

S = 0.1
FP16_CP_GRAD = 0.2 * T.CP_GRAD           # tests/test_model_gpu.py
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
from cara_amd.engine import CaraEngine   # noqa: E402  (the class alone: nothing here loads the HIP library)
LOSS_SCALE = {"bf16": 1.0, "fp16": CaraEngine.FP16_LOSS_SCALE}
# whole-model cases of the device module: (name, depth, batch, rank, cp_length)
MODEL_CASES = [("d2-b2", 2, 2, 16, 4), ("d3-b8", 3, 8, 16, 4), ("d3-b21", 3, 21, 16, 4), ("d3-b4-r64", 3, 4, 64, 4), ("d2-b2-cp3", 2, 2, 16, 3)]
# one-block cases: (batch, rank) -- 394, 1 576 and 4 137 rows, Rp 32 and 64
BLOCK_CASES = [(B, R) for R in (16, 64) for B in (2, 8, 21)]


def rel(a, b):
    a, b = a.double(), b.double().to(a.device)
    return ((a - b).norm() / b.norm()).item()


def grad_bar(build):
    return FP16_CP_GRAD if build == "fp16" else T.CP_GRAD


def keep_masks(depth, B, seed=11):
    """tests/test_model_gpu.py::_keep with a rate that drops samples at these batch sizes: multipliers 0 or 1 / 0.7 in every block
    but the first (timm's rates start at 0), fixed seed; sample 0 is dropped from the LAST block's MLP branch whatever the draw."""
    g = torch.Generator().manual_seed(seed)
    rates = torch.linspace(0, 0.3, depth)
    keep = (1 - rates).reshape(-1, 1, 1)
    k = ((keep + torch.rand(depth, 2, B, generator=g)).floor() / keep).float()
    k[depth - 1, 1, 0] = 0.0
    return k


@functools.lru_cache(maxsize=None)
def model_inputs(depth, B, rank, cp_length):
    w = O.synthetic_backbone(depth=depth)
    cp = O.synthetic_cp(rank=rank, cp_length=cp_length)
    cp["CP_A1"], cp["CP_P1"] = cp["CP_A1"][:(1 if cp_length == 5 else 3) * depth], cp["CP_P1"][:9 * depth]
    x, y = O.synthetic_batch(batch=B)
    head = {"weight": w["head.weight"], "bias": w["head.bias"]}
    return w, cp, x, y, head, keep_masks(depth, B)


def model_fp64(depth, B, rank, cp_length, device="cpu"):
    """float64 autograd of the as-written algorithm: (loss, logits, grads)"""
    w, cp, x, y, head, keep = model_inputs(depth, B, rank, cp_length)
    d = lambda t: {k: v.double().to(device) for k, v in t.items()}   # noqa: E731
    return O.train_step_as_written(x.double().to(device), y.to(device), d(w), d(cp), d(head), s=S, depth=depth,
                                   drop_path_keep=keep.double().to(device))


def model_sim(depth, B, rank, cp_length, build=None, device="cpu", **kw):
    w, cp, x, y, head, keep = model_inputs(depth, B, rank, cp_length)
    return O.backward_rounding_model(x.to(device), y.to(device), w, cp, head, s=S, depth=depth, drop_path_keep=keep,
                                     dtype=DTYPES.get(build), loss_scale=LOSS_SCALE.get(build, 1.0), **kw)


@functools.lru_cache(maxsize=None)
def block_inputs(B, rank, build):
    """depth-2 backbone, block 1; x and dy representable in the operand type"""
    w = O.synthetic_backbone(depth=2)
    cp = O.synthetic_cp(rank=rank)
    cp["CP_A1"], cp["CP_P1"] = cp["CP_A1"][:6], cp["CP_P1"][:18]
    r = O.make_rounder(DTYPES[build])
    x = r(torch.randn(B, 197, 768, generator=torch.Generator().manual_seed(3)))
    # (unit scale: the module-level path has no loss scaling, and gradients of 1e-3 would sit in fp16's subnormal range two GEMMs on)
    dy = r(torch.randn(B, 197, 768, generator=torch.Generator().manual_seed(4)))
    return w, cp, x, dy


def block_parts(y, dx, pieces):
    return dict(pieces, y=y, dx=dx)


def block_sim(kind, B, rank, build, rounded=True, device="cpu", **kw):
    w, cp, x, dy = block_inputs(B, rank, build)
    w = {k: v.to(device) for k, v in w.items() if k.startswith("blocks.1.")}
    cp = {k: v.to(device) for k, v in cp.items()}
    return block_parts(*O.block_rounding_model(kind, x.to(device), dy.to(device), w, cp, layer=1, s=S, depth=2,
                                               dtype=DTYPES[build] if rounded else None, **kw))


# ------------------------------------------------------------------------------------------
# identity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank,cp_length", [(16, 4), (64, 4), (16, 3), (16, 5)])
def test_without_rounding_the_model_is_float64_autograd(rank, cp_length):
    depth, B = 2, 3
    keep = model_inputs(depth, B, rank, cp_length)[5]
    assert (keep == 0).any() and (keep > 1).any()
    rloss, rlogits, gref = model_fp64(depth, B, rank, cp_length)
    loss, logits, g, pieces = model_sim(depth, B, rank, cp_length, want_pieces=True)
    worst = max(rel(g[k], gref[k]) for k in gref)
    print(f"\nidentity rank {rank} cp_length {cp_length}: worst rel-L2 {worst:.2e}, loss {abs(loss - rloss).item():.1e}")
    assert set(g) == set(gref)
    assert abs(loss - rloss).item() <= 1e-9 * abs(rloss).item() and rel(logits, rlogits) <= 1e-9
    for k in gref:
        assert gref[k].norm() > 0 and rel(g[k], gref[k]) <= 1e-9, (k, rel(g[k], gref[k]))
    # a dropped sample's branch carries no gradient: its rows of that branch's dx are exactly zero
    d, j, b = (keep == 0).nonzero()[0].tolist()
    rows = slice(b * 197, (b + 1) * 197)
    assert torch.count_nonzero(pieces[d]["dx_mlp" if j else "dx_attn"][rows]) == 0


@pytest.mark.parametrize("kind", ["attn", "mlp"])
def test_one_block_without_rounding_is_float64_autograd(kind):
    w, cp, x, dy = block_inputs(2, 16, "bf16")
    got = block_sim(kind, 2, 16, "bf16", rounded=False)
    xv = x.double().requires_grad_(True)
    wd = {k: v.double() for k, v in w.items()}
    fac = O.build_factored({k: v.double() for k, v in cp.items()}, S, depth=2)[1]
    fac = {n: tuple(None if t is None else t.clone().requires_grad_(True) for t in f) for n, f in fac.items()}   # U, Vs, c as leaves
    ident = O.make_rounder(None)
    y = O._attn_factored(xv, wd, "blocks.1.", fac, 12, 64 ** -0.5, ident) if kind == "attn" else O._mlp_factored(xv, wd, "blocks.1.", fac, ident)
    y.backward(dy.double())
    assert rel(got["y"], y.detach()) <= 1e-9 and rel(got["dx"], xv.grad) <= 1e-9
    for n in (("qkv", "proj") if kind == "attn" else ("fc1", "fc2")):
        U, Vs, c = fac[n]
        assert rel(got["dU_" + n], U.grad) <= 1e-9 and rel(got["dVs_" + n], Vs.grad) <= 1e-9
        if c is not None:
            assert rel(got["dc_" + n], c.grad) <= 1e-9


@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_the_models_forward_is_the_forward_rounding_model(build):
    depth, B, rank = 2, 2, 16
    w, cp, x, y, head, keep = model_inputs(depth, B, rank, 4)
    d = lambda t: {k: v.double() for k, v in t.items()}   # noqa: E731
    sim = O.vit_cara_forward(x.double(), d(w), d(cp), s=S, depth=depth, factored=True, sim_dtype=DTYPES[build], drop_path_keep=keep.double())
    loss, logits, _ = model_sim(depth, B, rank, 4, build)
    assert rel(logits, sim) <= 1e-9
    assert abs(loss - torch.nn.functional.cross_entropy(sim, y)).item() <= 1e-9


# ------------------------------------------------------------------------------------------
# premise
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth,B,rank,cp_length", MODEL_CASES)
def test_whole_model_alone_is_inside_the_gradient_bars(name, depth, B, rank, cp_length):
    _, _, gref = model_fp64(depth, B, rank, cp_length)
    for build in DTYPES:
        _, _, g = model_sim(depth, B, rank, cp_length, build)
        errs = {k: rel(g[k], gref[k]) for k in gref}
        print(f"\nPREMISE {build} {name}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        bad = {k: v for k, v in errs.items() if not v <= grad_bar(build) / T.LOGITS_VS_MODEL}
        assert not bad, (build, name, bad)


@pytest.mark.parametrize("B,rank", BLOCK_CASES)
def test_one_block_alone_is_inside_the_gradient_bars(B, rank):
    for build in DTYPES:
        for kind in ("attn", "mlp"):
            ref, sim = block_sim(kind, B, rank, build, rounded=False), block_sim(kind, B, rank, build)
            errs = {k: rel(sim[k], ref[k]) for k in ref if k != "y"}
            print(f"\nPREMISE {build} block {kind} B={B} rank {rank}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            bad = {k: v for k, v in errs.items() if not v <= grad_bar(build) / T.LOGITS_VS_MODEL}
            assert not bad, (build, kind, B, rank, bad)


# ------------------------------------------------------------------------------------------
# sensitivity, and what the two slips of the findings note would do to the model
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_sensitivity_of_every_tensor_to_every_rounding_point(build):
    """e(model without the point) / e(model), both against fp64, per tensor: depth 3, batch 4 (a table for the findings note: printed, not
    bounded)."""
    depth, B, rank = 3, 4, 16
    _, _, gref = model_fp64(depth, B, rank, 4)
    _, _, g = model_sim(depth, B, rank, 4, build)
    base = {k: rel(g[k], gref[k]) for k in gref}
    print(f"\nSENS {build} committed: " + "  ".join(f"{k} {v:.2e}" for k, v in base.items()))
    for point in O.BACKWARD_POINTS + ("T", "xn", "h", "qkv"):
        _, _, gp = model_sim(depth, B, rank, 4, build, skip=(point,))
        ratio = {k: rel(gp[k], gref[k]) / base[k] for k in gref}
        print(f"SENS {build} without {point}: " + "  ".join(f"{k} {v:.3f}" for k, v in ratio.items()))
        assert all(v == v and v < float("inf") for v in ratio.values())


SLIPS = [("dU of block 1's fc2 without its last 64 token rows", {"rider_rows": ("blocks.1.fc2", 64)}, True),
         ("dU of block 0's qkv without its last token row", {"rider_rows": ("blocks.0.qkv", 1)}, True),
         ("(a) rowscale missing from the 16-bit branch gradients of block 1", {"no_rowscale": ("blocks.1.",)}, False),
         ("(b) dGELU of block 1 from the rounded h", {"dgelu_from_h": ("blocks.1.",)}, False)]


@pytest.mark.parametrize("what,slip,under_the_old_bar", SLIPS, ids=[str(i) for i in range(len(SLIPS))])
def test_what_a_slip_does_to_the_model(what, slip, under_the_old_bar):
    """One deliberate defect in the model (``slip``), bf16, depth 3 / batch 8: a device that carried it would sit where the slipped
    model sits.  The two small ones -- a ragged row tile skipped by one rider product of one block -- stay under CP_GRAD in every
    tensor, so the fixed bar passes them, and are beyond 1.15 x the committed model's error in at least one tensor with >= 1e4
    numbers, so the ratio assertion of the device module does not.  The two gross ones of the findings note are beyond both."""
    depth, B, rank = 3, 8, 16
    _, _, gref = model_fp64(depth, B, rank, 4)
    _, _, g = model_sim(depth, B, rank, 4, "bf16")
    _, _, gs = model_sim(depth, B, rank, 4, "bf16", slip=slip)
    e, es = {k: rel(g[k], gref[k]) for k in gref}, {k: rel(gs[k], gref[k]) for k in gref}
    print(f"\nSLIP {what}: " + "  ".join(f"{k} {es[k]:.2e}/{e[k]:.2e}={es[k] / e[k]:.2f}" for k in gref))
    big = [k for k in gref if gref[k].numel() >= 10_000]
    assert max(es[k] / e[k] for k in big) > T.LOGITS_VS_MODEL
    assert (max(es.values()) < T.CP_GRAD) == under_the_old_bar
