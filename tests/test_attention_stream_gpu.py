"""The streamed-K/V attention kernels (N > 608 tokens; 224 < N <= 608 behind CARA_ATTN_STREAM=1) against fp64 restatements on the
same seeded inputs.  Bodies and tolerances are those of tests/test_kernels_gpu.py (test_attention_fwd_bwd,
test_attention_softmax_extremes, test_attention_for_the_cls_query_alone): the bounds describe the rounding points -- P rounded to
the operand type before P.V, one output rounding, P recomputed from the LSE in the backward -- which do not change with N.
Measured figures are printed (-s) before they are asserted."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from tests.test_kernels_gpu import DEV, L, attn_ref, close, rnd

pytestmark = pytest.mark.gpu

# one past the resident kernels' limit; whole tiles; ViT-B/16 @448 (785 = 24 * 32 + 17) at its head count; @512 (1025: a one-row
# tail); a longer tail in the second block of a tile (1050 = 16 * 64 + 26); @768 (2305)
SHAPES = [(1, 609, 1), (2, 640, 2), (2, 785, 12), (1, 1025, 3), (1, 1050, 2), (1, 2305, 1)]


def _fwd(qkv, B, N, H, scale, fill=float("nan")):
    lib, p, st = L().lib(), L().ptr, L().stream
    out = torch.full((B * N, H * 64), fill, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, N), fill, device=DEV)
    L().check(lib.cara_attention_fwd(p(qkv), p(out), p(lse), B, N, H, C.c_float(scale), st()), "attn fwd")
    return out, lse


def _bwd(qkv, out, dout, lse, B, N, H, scale):
    lib, p, st = L().lib(), L().ptr, L().stream
    dqkv = torch.full_like(qkv, float("nan"))
    L().check(lib.cara_attention_bwd(p(qkv), p(out), p(dout), p(lse), p(dqkv), B, N, H, C.c_float(scale), st()), "attn bwd")
    return dqkv


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_streamed_attention_fwd_bwd(B, N, H):
    scale = 64 ** -0.5
    qkv = rnd(B * N, 3 * H * 64, seed=1, scale=1.0)
    out, lse = _fwd(qkv, B, N, H, scale)
    qd = qkv.double().requires_grad_(True)
    ref, ref_lse = attn_ref(qd, B, N, H, scale)
    e_out = (out.double() - ref).abs()
    print(f"N={N}: out max err {e_out.max():.3e} (worst err / bound {(e_out / (4e-3 + 2 ** -7 * ref.abs())).max():.3f}), "
          f"lse max err {(lse.double() - ref_lse).abs().max():.3e}")
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()          # pre-filled with NaN: fully overwritten
    # P is rounded to bf16 before P.V (2^-9 relative on each weight), output rounded to bf16
    close(out, ref, 2 ** -7, 4e-3, "attn out")
    close(lse, ref_lse, 1e-4, 1e-4, "attn lse")
    dout = rnd(B * N, H * 64, seed=2)
    ref.backward(dout.double())
    dqkv = _bwd(qkv, out, dout, lse, B, N, H, scale)
    g = qd.grad
    err = (dqkv.double() - g).abs()
    tol = 2 ** -6 * g.abs() + 0.02 * g.abs().max()
    rel = (dqkv.double() - g).norm() / g.norm()
    print(f"N={N}: bwd max err {err.max():.3e} vs grad max {g.abs().max():.3e} (worst err / bound {(err / tol).max():.3f}), rel-L2 {rel:.3e}")
    assert not torch.isnan(dqkv).any()
    assert (err <= tol).all(), f"attn bwd max err {err.max():.3e} vs grad max {g.abs().max():.3e}"
    assert rel < 8e-3, f"attn bwd rel-L2 {rel:.3e}"


@pytest.mark.parametrize("N", [785, 1025])
def test_streamed_attention_softmax_extremes(N):
    """Large-magnitude scores: the exact two-sweep softmax must not overflow."""
    B, H = 1, 1
    qkv = rnd(B * N, 3 * 64, seed=3, scale=6.0)
    out, _ = _fwd(qkv, B, N, H, 0.125, fill=0.0)
    ref, _ = attn_ref(qkv, B, N, H, 0.125)
    assert torch.isfinite(out).all()
    close(out, ref, 2 ** -6, 0.05, "attn extreme")


@pytest.mark.parametrize("B,N,H", [(2, 785, 12), (1, 1025, 3)])
def test_streamed_attention_for_the_cls_query_alone(B, N, H):
    """cara_attention_cls_fwd / _bwd above 608 tokens against the full streamed kernels' cls rows and against fp64; the backward
    with a gradient on the cls rows only, all of dqkv."""
    lib = L().lib()
    p, st = L().ptr, L().stream
    scale = 64 ** -0.5
    qkv = rnd(B * N, 3 * H * 64, seed=1, scale=1.0)
    out_full, lse_full = _fwd(qkv, B, N, H, scale)
    out = torch.full((B * N, H * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, N), float("nan"), device=DEV)
    L().check(lib.cara_attention_cls_fwd(p(qkv), p(out), p(lse), B, N, H, C.c_float(scale), st()), "attn cls fwd")
    cls = torch.arange(B, device=DEV) * N
    qd = qkv.double().requires_grad_(True)
    ref, ref_lse = attn_ref(qd, B, N, H, scale)
    close(out[cls], ref[cls], 2 ** -7, 4e-3, "cls out")
    close(out[cls], out_full[cls].double(), 2 ** -7, 2e-3, "cls out vs the full kernel")
    close(lse[:, :, 0], ref_lse[:, :, 0], 1e-4, 1e-4, "cls lse")
    mask = torch.ones(B * N, dtype=torch.bool, device=DEV)
    mask[cls] = False
    assert torch.isnan(out[mask]).all() and torch.isnan(lse[:, :, 1:]).all()          # nothing else is written
    dout = torch.zeros(B * N, H * 64, dtype=torch.bfloat16, device=DEV)
    dout[cls] = rnd(B, H * 64, seed=2)
    ref.backward(dout.double())
    dqkv = torch.full_like(qkv, float("nan"))
    L().check(lib.cara_attention_cls_bwd(p(qkv), p(out), p(dout), p(lse), p(dqkv), B, N, H, C.c_float(scale), st()), "attn cls bwd")
    g = qd.grad
    assert not torch.isnan(dqkv).any()
    err = (dqkv.double() - g).abs()
    assert (err <= 2 ** -6 * g.abs() + 0.02 * g.abs().max()).all(), f"max err {err.max():.3e} vs grad max {g.abs().max():.3e}"
    assert (dqkv.double() - g).norm() / g.norm() < 8e-3
    qblock = dqkv.reshape(B, N, 3, H * 64)[:, 1:, 0]
    assert torch.count_nonzero(qblock) == 0                                          # no query but the cls one was in play
    dfull = _bwd(qkv, out_full, dout, lse_full, B, N, H, scale)
    assert (dqkv.double() - dfull.double()).norm() / dfull.double().norm() < 8e-3


def test_streamed_attention_is_bitwise_reproducible():
    """No atomics, no cross-workgroup sums: two launches on the same inputs give the same bits."""
    B, N, H = 2, 785, 12
    scale = 64 ** -0.5
    qkv = rnd(B * N, 3 * H * 64, seed=1)
    dout = rnd(B * N, H * 64, seed=2)
    out1, lse1 = _fwd(qkv, B, N, H, scale)
    out2, lse2 = _fwd(qkv, B, N, H, scale)
    assert torch.equal(out1, out2) and torch.equal(lse1, lse2)
    d1 = _bwd(qkv, out1, dout, lse1, B, N, H, scale)
    d2 = _bwd(qkv, out1, dout, lse1, B, N, H, scale)
    assert not torch.isnan(d1).any() and torch.equal(d1, d2)


def test_stream_switch_passes_the_resident_kernels_tests():
    """CARA_ATTN_STREAM=1 (read once per process) hands 224 < N <= 608 to the streamed kernels: the existing attention tests and
    the ViT-L/16 @384 whole-model test (577 tokens) run again, unmodified, in a process with the switch set."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CARA_ATTN_STREAM="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_kernels_gpu.py"),
                          os.path.join(root, "tests", "test_model_gpu.py"), "-x", "-q", "-s", "-k",
                          "test_attention_fwd_bwd or test_attention_softmax_extremes or test_attention_for_the_cls_query_alone "
                          "or test_vit_large_384_against_oracle"],
                         cwd=root, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(out.stdout.strip().split("\n")[-12:])
    print(tail)
    assert out.returncode == 0, tail + out.stderr[-2000:]
    assert "passed" in tail and "failed" not in tail
