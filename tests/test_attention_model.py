"""Host proof of oracle.cara_oracle.attn_rounding_model, the float64 restatement of attention.hip with the kernels' rounding points
that tests/test_attention_contract_gpu.py measures the device against: the model ALONE -- rounding noise and nothing else -- must
sit inside the bounds the device attention tests assert (tests/test_kernels_gpu.py::test_attention_fwd_bwd), at flat and at peaked
softmaxes and for both operand types.  If it did not, those bounds would reject a correct kernel, and "device error <= 1.15 x
model error" would mean nothing.  No GPU."""
import math

import pytest
import torch

from oracle.cara_oracle import attn_rounding_model

SPREADS = [1, 4, 9, 16, 36]   # score spread sigma^2: the q and k thirds of the seeded input are multiplied by sigma


def attn_inputs(B, N, H, sigma2=1, dtype=torch.bfloat16, device="cpu", cls_only=False):
    """The attention tests' inputs -- qkv = randn(seed 1), dout = randn(seed 2), drawn on the host and rounded to ``dtype`` -- with
    the q and k columns multiplied by sqrt(sigma2): the scores' standard deviation is sigma2 at scale 1/8 (1: mean max-probability
    0.05 at 197 tokens; 36: 0.95, the peaked rows of a trained ViT).  cls_only: the gradient arrives on the cls rows alone."""
    def rnd(*shape, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return torch.randn(*shape, generator=g).to(dtype)
    x = rnd(B * N, 3 * H * 64, seed=1).float().reshape(B * N, 3, H * 64)
    x[:, :2] *= math.sqrt(sigma2)
    qkv = x.reshape(B * N, 3 * H * 64).to(dtype)
    if cls_only:
        dout = torch.zeros(B * N, H * 64, dtype=dtype)
        dout[torch.arange(B) * N] = rnd(B, H * 64, seed=2)
    else:
        dout = rnd(B * N, H * 64, seed=2)
    return qkv.to(device), dout.to(device)


def attn_fp64(qkv, dout, B, N, H, scale):
    """plain float64 attention and its autograd gradient: (out, lse, dqkv)"""
    qd = qkv.double().requires_grad_(True)
    q, k, v = qd.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * scale
    out = (s.softmax(-1) @ v).transpose(1, 2).reshape(B * N, H * 64)
    out.backward(dout.double())
    return out.detach(), torch.logsumexp(s, -1).detach(), qd.grad


def rel(a, b):
    return ((a.double() - b).norm() / b.norm()).item()


@pytest.mark.parametrize("sigma2", SPREADS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_rounding_model_alone_is_inside_the_device_bounds(dtype, sigma2):
    B, N, H, scale = 2, 197, 3, 0.125
    qkv, dout = attn_inputs(B, N, H, sigma2, dtype)
    ref, ref_lse, g = attn_fp64(qkv, dout, B, N, H, scale)
    out, lse, dqkv = attn_rounding_model(qkv, dout, B, N, H, scale, dtype)
    e_out = (out - ref).abs() / (4e-3 + 2 ** -7 * ref.abs())
    e_lse = (lse - ref_lse).abs() / (1e-4 + 1e-4 * ref_lse.abs())
    e_g = (dqkv - g).abs() / (2 ** -6 * g.abs() + 0.02 * g.abs().max())
    parts = [rel(dqkv.reshape(B * N, 3, -1)[:, i], g.reshape(B * N, 3, -1)[:, i]) for i in range(3)]
    norms = [g.reshape(B * N, 3, -1)[:, i].norm().item() for i in range(3)]
    print(f"{dtype} sigma^2 {sigma2}: out rel-L2 {rel(out, ref):.2e} worst/bound {e_out.max():.3f}; lse worst/bound {e_lse.max():.3f}; "
          f"bwd rel-L2 {rel(dqkv, g):.2e} worst/bound {e_g.max():.3f}; dQ dK dV rel-L2 {parts[0]:.2e} {parts[1]:.2e} {parts[2]:.2e}; "
          f"|g| {g.norm():.1f} = {norms[0]:.1f} {norms[1]:.1f} {norms[2]:.1f}")
    assert e_out.max() <= 1 and e_lse.max() <= 1
    assert e_g.max() <= 1
    assert rel(dqkv, g) < 8e-3
    # The gradient must not collapse as the rows saturate, or the backward bounds would be met by noise on nothing.  dV = P^T dO
    # is smallest for the uniform softmax, where every row of dV is the mean row of dO: |dV| >= |dO| / sqrt(N).  dQ and dK vanish
    # only for one-hot rows; they must still carry a visible share of the whole (1 %: 100 x the bf16 rounding step of the rest).
    assert norms[2] >= 0.99 * dout.double().norm().item() / math.sqrt(N)
    assert min(norms[0], norms[1]) >= 1e-2 * g.norm().item()
