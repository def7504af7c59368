"""Every gradient of the device's backward held to what rounding explains, in both operand builds: for every part,
rel-L2(device, fp64) <= F x rel-L2(model, fp64), where the model is oracle.cara_oracle.backward_rounding_model /
block_rounding_model (float64, rounded where the kernels round: proven on the host by tests/test_backward_model.py) and F =
tolerances.LOGITS_VS_MODEL, with the small-part allowance of docs/findings/attention_contract.md section 2.  The CP_GRAD bars
stay as a ceiling; a part that is exactly zero in fp64 is exactly zero on the device.

An excess is resolved by finding the rounding point the model misses (cite its kernel line in the model's docstring) or the kernel
defect -- never by a larger factor.  The fp64 reference and the model run in torch on the device (float64); nothing here reads a
fixture.  Figures are printed (-s) before they are asserted; docs/findings/backward_contract.md holds the tables."""
import functools
import math
import os

import pytest
import torch

from tests import tolerances as T
from tests.test_backward_model import (BLOCK_CASES, MODEL_CASES, S, block_inputs, block_sim, grad_bar, model_fp64, model_inputs,
                                       model_sim, rel)
from tests.test_model_gpu import DEV, build

pytestmark = pytest.mark.gpu
BUILDS = ["bf16", "fp16"]


def _factor(n):
    """tests/test_attention_contract_gpu.py::_factor: parts with fewer than 1e4 numbers get three standard deviations of the ratio
    of two root-mean-squares of n noise terms on top"""
    return T.LOGITS_VS_MODEL * (1 + 3 / math.sqrt(n)) if n < 10_000 else T.LOGITS_VS_MODEL


def _saved_gelu_grad():
    """what save_gelu_grad() / epi_riders_env() of cara_amd/csrc/vit.hip decide from the environment of this process (dim 768,
    factored mode): a MIRROR of that logic -- if those two functions change, this one changes with them"""
    v = int(os.environ.get("CARA_SAVE_GELU_GRAD", "-1"))
    on = int(os.environ.get("CARA_EPI_RIDERS", "0")) != 0 if v < 0 else v != 0
    return on and int(os.environ.get("CARA_FUSE_XU", "1")) != 0


def _hold(tag, build, parts, sum_bounds=None, not_held=()):
    """parts: name -> (device, model, model evaluated a second time with fp32 accumulators in another order, fp64).  sum_bounds:
    name -> elementwise bound for a part that has NO rounding point (dc of the linear that receives the test's own dy: the model is
    fp64 to the last bit, its error exactly zero, and the device's is that of an fp32 sum).  not_held: the parts whose direct
    device-to-model distance is NOT asserted because the yardstick is not well below the model's error; every other part must be
    held -- a part that drops out of the direct check fails the test instead of leaving it silently."""
    bad, dropped = [], set()
    for name, (dev_t, sim_t, sim32_t, ref_t) in parts.items():
        ref_t = ref_t.to(DEV)
        if sum_bounds and name in sum_bounds:
            assert rel(sim_t, ref_t) == 0
            worst = ((dev_t.double() - ref_t).abs() / sum_bounds[name]).max().item()
            print(f"RATIO {build} {tag} {name}: no rounding point (model error 0); device rel-L2 {rel(dev_t, ref_t):.3e}, worst error / fp32-sum bound {worst:.3e}")
            if not worst <= 1:
                bad.append(f"{name}: beyond the bound of an fp32 sum ({worst:.3e})")
            continue
        if ref_t.norm() == 0:
            print(f"RATIO {build} {tag} {name}: fp64 is exactly zero; device nonzeros {int(torch.count_nonzero(dev_t))}")
            if torch.count_nonzero(dev_t) != 0:
                bad.append(f"{name}: nonzero where fp64 is exactly zero")
            continue
        e_dev, e_sim, f = rel(dev_t, ref_t), rel(sim_t, ref_t), _factor(ref_t.numel())
        direct, yard = rel(dev_t, sim_t), rel(sim32_t, sim_t)
        # the direct distance is held to BWD_VS_MODEL_ORDER x the yardstick where that says more than the ratio does
        use_direct = T.BWD_VS_MODEL_ORDER * yard <= e_sim
        if not use_direct:
            dropped.add(name)
        print(f"RATIO {build} {tag} {name}: dev/sim={e_dev / e_sim:.3f} (device {e_dev:.3e}, model {e_sim:.3e}, F {f:.3f}, n {ref_t.numel()}); "
              f"device-to-model {direct:.3e}, yardstick {yard:.3e}" + ("" if use_direct else " (not well below the model's error: not held)"))
        if not e_dev <= f * e_sim:
            bad.append(f"{name}: device {e_dev:.3e} > {f:.3f} x model {e_sim:.3e}")
        if not e_dev < grad_bar(build):
            bad.append(f"{name}: device {e_dev:.3e} above the bar {grad_bar(build):.1e}")
        if use_direct and not direct <= T.BWD_VS_MODEL_ORDER * yard:
            bad.append(f"{name}: device-to-model {direct:.3e} > {T.BWD_VS_MODEL_ORDER} x yardstick {yard:.3e}")
    if not dropped <= set(not_held):
        bad.append(f"the direct device-to-model check no longer covers {sorted(dropped - set(not_held))}")
    assert not bad, f"{build} {tag}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------
# one block, module level
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block_module(rank, build):
    w, cp, _, _ = block_inputs(2, rank, build)
    return build_model(w, cp, rank, 2, build).eval()


def build_model(w, cp, rank, depth, precision, cp_length=4):
    return build(w, cp, rank, S, depth, 224, cp_length=cp_length, precision=precision)


@pytest.mark.parametrize("kind", ["attn", "mlp"])
@pytest.mark.parametrize("B,rank", BLOCK_CASES)
@pytest.mark.parametrize("operands", BUILDS)
def test_one_block_gradients(operands, B, rank, kind, monkeypatch):
    """blk.attn / blk.mlp under autograd on operand-representable x and dy: dx and the per-linear dU, dVs, dc that
    cara_amd.modules hands to cara_factor_grad_reduce (caught on their way into modules._scatter)."""
    from cara_amd import modules
    m = _block_module(rank, operands)
    _, _, x, dy = block_inputs(B, rank, operands)
    caught, padding, scatter = {}, [], modules._scatter

    def catching(eng, model, dev, layer, pieces):
        # (what cara_factor_grad_reduce is handed: the columns rank .. Rp of dU / dVs are padding and must be zero)
        padding.extend(int(torch.count_nonzero(v[:, rank:])) for v in pieces.values() if v.ndim == 2)
        caught.update({k: v[:, :rank].clone() if v.ndim == 2 else v.clone() for k, v in pieces.items()})
        return scatter(eng, model, dev, layer, pieces)
    monkeypatch.setattr(modules, "_scatter", catching)
    xd = x.to(DEV).requires_grad_(True)
    y = getattr(m.blocks[1], kind)(xd)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert not torch.isnan(xd.grad).any() and caught
    assert not any(padding), f"nonzero padding columns in the per-linear pieces: {padding}"
    ref = block_sim(kind, B, rank, operands, rounded=False, device=DEV)
    sim = block_sim(kind, B, rank, operands, device=DEV)
    sim32 = block_sim(kind, B, rank, operands, device=DEV, acc32=True)
    dev_parts = dict(caught, dx=xd.grad, y=y.detach())
    assert set(dev_parts) == set(ref)
    # dc = colsum dy: an fp32 sum of n = B 197 exactly representable terms, in whatever order: |error| <= n 2^-24 sum |dy| per column
    own_dc = "dc_proj" if kind == "attn" else "dc_fc2"
    bound = {own_dc: B * 197 * 2.0 ** -24 * dy.double().abs().reshape(-1, 768).sum(0).to(DEV)}
    _hold(f"block-{kind} B={B} rank={rank}", operands, {k: (dev_parts[k], sim[k], sim32[k], ref[k]) for k in ref}, bound,
          not_held=("dU_qkv", "dVs_proj") if (operands, kind) == ("fp16", "attn") else ())


# ------------------------------------------------------------------------------------------
# whole model through train_step
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_ref(depth, B, rank, cp_length):
    return model_fp64(depth, B, rank, cp_length, device=DEV)


@pytest.mark.parametrize("name,depth,B,rank,cp_length", MODEL_CASES)
@pytest.mark.parametrize("operands", BUILDS)
def test_whole_model_gradients(operands, name, depth, B, rank, cp_length):
    """train_step(x, y, None, droppath=keep) with dropped samples, the last block on its cls rows: every CP gradient, the head's,
    the loss."""
    w, cp, x, y, head, keep = model_inputs(depth, B, rank, cp_length)
    assert (keep == 0).any()
    m = build_model(w, cp, rank, depth, operands, cp_length).train()
    eng = m._cara_engine
    loss = eng.train_step(x.to(DEV), y.to(DEV), None, droppath=keep.to(DEV))
    torch.cuda.synchronize()
    rloss, _, gref = _model_ref(depth, B, rank, cp_length)
    kw = dict(device=DEV, saved_gelu_grad=_saved_gelu_grad())
    sloss, _, gsim = model_sim(depth, B, rank, cp_length, operands, **kw)
    _, _, gsim32 = model_sim(depth, B, rank, cp_length, operands, acc32=True, **kw)
    dev_g = {k: getattr(m, k).grad for k in cp}
    dev_g.update({"head.weight": m.head.weight.grad, "head.bias": m.head.bias.grad})
    assert set(dev_g) == set(gref)
    # the loss is a part of ONE number: the small-part rule gives it F (1 + 3 / sqrt(1)) = 4.6; the existing bound stays as its ceiling
    e_dev, e_sim = abs(loss.item() - rloss.item()), abs(sloss.item() - rloss.item())
    print(f"\nRATIO {operands} {name} loss: device {loss.item():.6f} model {sloss.item():.6f} fp64 {rloss.item():.6f}: |dev - fp64| {e_dev:.2e}, |model - fp64| {e_sim:.2e}")
    assert e_dev <= _factor(1) * e_sim, f"loss: device {e_dev:.3e} > {_factor(1):.2f} x model {e_sim:.3e}"
    assert e_dev < (5e-4 if operands == "fp16" else 5e-3) * max(1.0, abs(rloss.item()))
    # (no whole-model part has a yardstick well below the model's error: docs/findings/backward_contract.md section 5)
    _hold(name, operands, {k: (dev_g[k], gsim[k], gsim32[k], gref[k]) for k in gref}, not_held=tuple(gref))
