"""What cara_amd/csrc/attention.hip promises, held to it on the device, in both operand builds (bf16 and fp16):

* B  the device's error against fp64 is no larger than the error of the kernels' own rounding model
     (oracle.cara_oracle.attn_rounding_model, proven on the host by tests/test_attention_model.py), part by part (out, dQ, dK, dV),
     at flat and at peaked softmaxes, one shape per dispatch path and the cls pair;
* C  every edge of the dispatch (attn_path), of the tile counts, of the streamed workgroup width, the ViT token counts g^2 + 1 and
     the grid edges of the persistent kernels, against fp64 with the bounds of tests/test_kernels_gpu.py::test_attention_fwd_bwd;
     bitwise equal results of two launches on every path;
* D  isolation, bit for bit: what a (sample, head) pair gets does not depend on any other sample or head nor on what lies before
     or behind the buffers, and nothing is written outside them.

Measured figures are printed (-s) before they are asserted; docs/findings/attention_contract.md holds the tables."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from oracle.cara_oracle import attn_rounding_model
from tests import tolerances as T
from tests.test_attention_model import SPREADS, attn_inputs, rel
from tests.test_kernels_gpu import DEV, L, attn_ref, close, rnd

pytestmark = pytest.mark.gpu

OPERANDS = ["bf16", "fp16"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st_width():
    """queries (keys) per workgroup of the streamed kernels: ST_WAVES * 32, read from the source"""
    src = open(os.path.join(ROOT, "cara_amd", "csrc", "attention.hip")).read()
    return int(re.search(r"constexpr int ST_WAVES = (\d+);", src).group(1)) * 32


def _fwd(lib, qkv, B, N, H, scale, out=None, lse=None, cls=False):
    p, st = L().ptr, L().stream
    if out is None:
        out = torch.full((B * N, H * 64), float("nan"), dtype=qkv.dtype, device=DEV)
    if lse is None:
        lse = torch.full((B, H, N), float("nan"), device=DEV)
    fn = lib.cara_attention_cls_fwd if cls else lib.cara_attention_fwd
    L().check(fn(p(qkv), p(out), p(lse), B, N, H, C.c_float(scale), st()), "attn fwd")
    return out, lse


def _bwd(lib, qkv, out, dout, lse, B, N, H, scale, dqkv=None, cls=False):
    p, st = L().ptr, L().stream
    if dqkv is None:
        dqkv = torch.full_like(qkv, float("nan"))
    fn = lib.cara_attention_cls_bwd if cls else lib.cara_attention_bwd
    L().check(fn(p(qkv), p(out), p(dout), p(lse), p(dqkv), B, N, H, C.c_float(scale), st()), "attn bwd")
    return dqkv


def _parts(t, B, N):
    return [t.reshape(B * N, 3, -1)[:, i] for i in range(3)]


# ------------------------------------------------------------------------------------------
# B. device error <= LOGITS_VS_MODEL x the rounding model's error
# ------------------------------------------------------------------------------------------
CASES = [("short", 2, 97, 3, False), ("headline", 2, 197, 3, False), ("long", 2, 300, 3, False), ("streamed", 1, 785, 2, False),
         ("cls", 2, 197, 3, True), ("cls-streamed", 1, 785, 2, True)]


def _factor(n):
    """Device and model are two draws of the same rounding noise, so their rel-L2 errors against fp64 agree to a few percent over
    the 1e5 .. 1e6 elements of a tensor: tolerances.LOGITS_VS_MODEL (1.15), by the argument made there.  Two parts of the cls
    pair are SMALL -- its `out` and dQ are the cls rows alone, B H 64 = 128 or 384 numbers -- and a root-mean-square of n noise
    terms scatters by about 1 / sqrt(2 n) of itself, the ratio of two such by 1 / sqrt(n): 9 % at n = 128.  Those parts (n < 1e4)
    get three of these standard deviations on top; every other part is held to 1.15 as it stands."""
    return T.LOGITS_VS_MODEL * (1 + 3 / math.sqrt(n)) if n < 10_000 else T.LOGITS_VS_MODEL


@pytest.mark.parametrize("sigma2", SPREADS)
@pytest.mark.parametrize("path,B,N,H,cls", CASES)
@pytest.mark.parametrize("operands", OPERANDS)
def test_device_error_is_the_rounding_models(operands, path, B, N, H, cls, sigma2):
    lib, dt, scale = L().lib(operands), L().act_dtype(operands), 0.125
    qkv, dout = attn_inputs(B, N, H, sigma2, dt, DEV, cls_only=cls)
    out, lse = _fwd(lib, qkv, B, N, H, scale, cls=cls)
    dqkv = _bwd(lib, qkv, out, dout, lse, B, N, H, scale, cls=cls)
    qd = qkv.double().requires_grad_(True)
    ref, ref_lse = attn_ref(qd, B, N, H, scale)
    ref.backward(dout.double())
    ref, g = ref.detach(), qd.grad
    m_out, m_lse, m_g = attn_rounding_model(qkv, dout, B, N, H, scale, dt)
    rows = torch.arange(B, device=DEV) * N if cls else slice(None)   # the cls pair writes the cls rows of out / lse only
    lcol = 0 if cls else slice(None)
    triples = [("out", out[rows], m_out[rows], ref[rows])]
    gp, mp, rp = _parts(dqkv, B, N), _parts(m_g, B, N), _parts(g, B, N)
    for i, name in enumerate(("dQ", "dK", "dV")):
        sel = rows if (cls and i == 0) else slice(None)                # dQ of the cls pair: the cls rows (the others are zero)
        triples.append((name, gp[i][sel], mp[i][sel], rp[i][sel]))
    line, bad = [], []
    for name, dev_t, sim_t, ref_t in triples:
        e_dev, e_sim, f = rel(dev_t, ref_t), rel(sim_t, ref_t), _factor(ref_t.numel())
        line.append(f"{name} {e_dev:.3e}/{e_sim:.3e}={e_dev / e_sim:.3f}")
        if not e_dev <= f * e_sim:
            bad.append(f"{name}: device {e_dev:.3e} > {f:.3f} x model {e_sim:.3e}")
    e_lse = (lse[:, :, lcol].double() - ref_lse[:, :, lcol]).abs()
    err = (dqkv.double() - g).abs()
    tol = 2 ** -6 * g.abs() + 0.02 * g.abs().max()
    print(f"\nRATIO {operands} {path} ({B},{N},{H}) sigma2={sigma2}: " + "  ".join(line) +
          f"  | lse max err {e_lse.max():.2e}  bwd worst/bound {(err / tol).max():.3f} rel-L2 {rel(dqkv, g):.3e}")
    assert not torch.isnan(dqkv).any() and not torch.isnan(out[rows]).any()
    assert not bad, "; ".join(bad)
    close(lse[:, :, lcol], ref_lse[:, :, lcol], 1e-4, 1e-4, "attn lse")
    close(out[rows], ref[rows], 2 ** -7, 4e-3, "attn out")              # the existing elementwise bounds stay as a floor
    assert (err <= tol).all(), f"attn bwd max err {err.max():.3e} vs grad max {g.abs().max():.3e}"
    assert rel(dqkv, g) < 8e-3


# ------------------------------------------------------------------------------------------
# C. path edges, tile counts, grid edges: the bodies and bounds of test_attention_fwd_bwd / test_attention_for_the_cls_query_alone
# ------------------------------------------------------------------------------------------
def _fwd_bwd_against_fp64(operands, B, N, H, backward=True):
    lib, dt, scale = L().lib(operands), L().act_dtype(operands), 64 ** -0.5
    qkv = rnd(B * N, 3 * H * 64, seed=1, scale=1.0, dtype=dt)
    out, lse = _fwd(lib, qkv, B, N, H, scale)
    qd = qkv.double().requires_grad_(True)
    ref, ref_lse = attn_ref(qd, B, N, H, scale)
    e_out = (out.double() - ref).abs()
    print(f"\n{operands} ({B},{N},{H}): out worst err / bound {(e_out / (4e-3 + 2 ** -7 * ref.abs())).max():.3f}, "
          f"lse max err {(lse.double() - ref_lse).abs().max():.3e}", end="")
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()          # pre-filled with NaN: fully overwritten
    close(out, ref, 2 ** -7, 4e-3, "attn out")
    close(lse, ref_lse, 1e-4, 1e-4, "attn lse")
    if not backward:
        return
    dout = rnd(B * N, H * 64, seed=2, dtype=dt)
    ref.backward(dout.double())
    dqkv = _bwd(lib, qkv, out, dout, lse, B, N, H, scale)
    g = qd.grad
    err = (dqkv.double() - g).abs()
    tol = 2 ** -6 * g.abs() + 0.02 * g.abs().max()
    r = rel(dqkv, g)
    print(f"; bwd worst err / bound {(err / tol).max():.3f}, rel-L2 {r:.3e}", end="")
    assert not torch.isnan(dqkv).any()
    assert (err <= tol).all(), f"attn bwd max err {err.max():.3e} vs grad max {g.abs().max():.3e}"
    assert r < 8e-3, f"attn bwd rel-L2 {r:.3e}"


# SHORT <= 128 < HEADLINE <= 224 < LONG <= 608 < STREAMED; tiles of 32 keys; the persistent forward is specialised on 5 / 6 / 7 tiles
PATH_EDGES = [1, 2, 31, 32, 65, 96, 97, 127, 128, 159, 191, 192, 223, 256, 257, 607]
# the streamed kernels' workgroup owns W = ST_WAVES * 32 rows: every multiple of W in 609 .. 1100, and one to either side
STREAM_EDGES = [_st_width() * k + d for k in range(1, 1100 // _st_width() + 1) for d in (-1, 0, 1)
                if 609 <= _st_width() * k - 1 and _st_width() * k + 1 <= 1100]
# token counts the attention tests already run (tests/test_kernels_gpu.py, tests/test_attention_stream_gpu.py)
ELSEWHERE = {5, 33, 64, 129, 160, 161, 193, 197, 224, 225, 300, 577, 608, 609, 640, 785, 1025, 1050, 2305}
# "any square size that the patch size divides": a g x g grid of patches and the cls token
VIT_GRIDS = [g for g in range(1, 33) if g * g + 1 not in ELSEWHERE | set(PATH_EDGES) | set(STREAM_EDGES)]


@pytest.mark.parametrize("N", PATH_EDGES + STREAM_EDGES)
@pytest.mark.parametrize("operands", OPERANDS)
def test_path_and_tile_edges(operands, N):
    _fwd_bwd_against_fp64(operands, 2, N, 2)


@pytest.mark.parametrize("g", VIT_GRIDS)
@pytest.mark.parametrize("operands", OPERANDS)
def test_every_vit_grid(operands, g):
    """N = g^2 + 1 for every grid up to 32 x 32 (512 pixels at patch 16): forward and LSE for all, the backward for every third."""
    _fwd_bwd_against_fp64(operands, 2, g * g + 1, 2, backward=VIT_GRIDS.index(g) % 3 == 0)


@pytest.mark.parametrize("B,H", [(85, 3), (256, 1), (257, 1), (512, 1), (171, 3), (769, 1)])
@pytest.mark.parametrize("operands", OPERANDS)
def test_persistent_grid_edges(operands, B, H):
    """The headline kernels walk the (batch, head) pairs on a grid of min(B H, 256) workgroups and prefetch the next pair:
    B H = 255, 256 (no workgroup has a next pair), 257 (one has), 512, 513 (ragged third round), 769."""
    _fwd_bwd_against_fp64(operands, B, 197, H)


@pytest.mark.parametrize("N", [1, 2, 128, 129, 224, 225, 608, 609])
@pytest.mark.parametrize("operands", OPERANDS)
def test_cls_pair_at_path_edges(operands, N):
    """cara_attention_cls_fwd / _bwd at the edges of the full kernels' paths and at its own forward switch (608 | 609): against
    fp64, against the full kernels' cls rows, and nothing but the cls rows written."""
    B, H = 2, 2
    lib, dt, scale = L().lib(operands), L().act_dtype(operands), 64 ** -0.5
    qkv = rnd(B * N, 3 * H * 64, seed=1, scale=1.0, dtype=dt)
    out_full, lse_full = _fwd(lib, qkv, B, N, H, scale)
    out, lse = _fwd(lib, qkv, B, N, H, scale, cls=True)
    cls = torch.arange(B, device=DEV) * N
    qd = qkv.double().requires_grad_(True)
    ref, ref_lse = attn_ref(qd, B, N, H, scale)
    print(f"\n{operands} cls N={N}: out max err {(out[cls].double() - ref[cls]).abs().max():.3e}, "
          f"lse max err {(lse[:, :, 0].double() - ref_lse[:, :, 0]).abs().max():.3e}", end="")
    close(out[cls], ref[cls], 2 ** -7, 4e-3, "cls out")
    close(out[cls], out_full[cls].double(), 2 ** -7, 2e-3, "cls out vs the full kernel")
    close(lse[:, :, 0], ref_lse[:, :, 0], 1e-4, 1e-4, "cls lse")
    mask = torch.ones(B * N, dtype=torch.bool, device=DEV)
    mask[cls] = False
    assert torch.isnan(out[mask]).all() and torch.isnan(lse[:, :, 1:]).all()          # nothing else is written
    dout = torch.zeros(B * N, H * 64, dtype=dt, device=DEV)
    dout[cls] = rnd(B, H * 64, seed=2, dtype=dt)
    ref.backward(dout.double())
    dqkv = _bwd(lib, qkv, out, dout, lse, B, N, H, scale, cls=True)
    g = qd.grad
    assert not torch.isnan(dqkv).any()
    err = (dqkv.double() - g).abs()
    tol = 2 ** -6 * g.abs() + 0.02 * g.abs().max()
    print(f"; bwd worst err / bound {(err / tol).max():.3f}, rel-L2 {rel(dqkv, g):.3e}", end="")
    assert (err <= tol).all(), f"max err {err.max():.3e} vs grad max {g.abs().max():.3e}"
    assert rel(dqkv, g) < 8e-3
    if N > 1:
        assert torch.count_nonzero(dqkv.reshape(B, N, 3, H * 64)[:, 1:, 0]) == 0     # no query but the cls one was in play
    dfull = _bwd(lib, qkv, out_full, dout, lse_full, B, N, H, scale).double()
    assert (dqkv.double() - dfull).norm() / dfull.norm() < 8e-3


@pytest.mark.parametrize("B,N,H", [(3, 64, 2), (2, 197, 12), (2, 577, 4)])
@pytest.mark.parametrize("operands", OPERANDS)
def test_two_launches_give_the_same_bits(operands, B, N, H):
    """No atomics, no cross-workgroup sums on any path (tests/test_attention_stream_gpu.py has the streamed one), the cls pair
    included."""
    lib, dt, scale = L().lib(operands), L().act_dtype(operands), 64 ** -0.5
    qkv = rnd(B * N, 3 * H * 64, seed=1, dtype=dt)
    dout = rnd(B * N, H * 64, seed=2, dtype=dt)
    for cls in (False, True):
        rows = torch.arange(B, device=DEV) * N if cls else slice(None)
        lcol = 0 if cls else slice(None)
        out1, lse1 = _fwd(lib, qkv, B, N, H, scale, cls=cls)
        out2, lse2 = _fwd(lib, qkv, B, N, H, scale, cls=cls)
        assert not torch.isnan(out1[rows]).any() and not torch.isnan(lse1[:, :, lcol]).any()
        assert torch.equal(out1[rows], out2[rows]) and torch.equal(lse1[:, :, lcol], lse2[:, :, lcol])
        d1 = _bwd(lib, qkv, out1, dout, lse1, B, N, H, scale, cls=cls)
        d2 = _bwd(lib, qkv, out1, dout, lse1, B, N, H, scale, cls=cls)
        assert not torch.isnan(d1).any() and torch.equal(d1, d2)


# ------------------------------------------------------------------------------------------
# D. isolation, bit for bit
# ------------------------------------------------------------------------------------------
GUARD_ROWS = 64
SENTINEL = {2: (torch.int16, 0x5A5A), 4: (torch.int32, 0x5A5A5A5A)}   # finite in bf16, fp16 and fp32


class _Guarded:
    """A [rows, cols] tensor inside a larger allocation, GUARD_ROWS rows of guard in front of it and behind it."""

    def __init__(self, rows, cols, dtype):
        g = GUARD_ROWS * cols
        self.big = torch.empty((rows + 2 * GUARD_ROWS) * cols, dtype=dtype, device=DEV)
        self.t = self.big[g:g + rows * cols].view(rows, cols)
        self.guards = (self.big[:g], self.big[g + rows * cols:])
        self.idt, self.word = SENTINEL[self.big.element_size()]

    def set_sentinels(self, inner=True):
        for t in self.guards + ((self.t,) if inner else ()):
            t.view(self.idt).fill_(self.word)

    def sentinels_intact(self):
        return all(bool((t.view(self.idt) == self.word).all()) for t in self.guards)

    def fill_guards(self, seed):
        """finite seeded data (seed given) or NaN (None)"""
        for i, t in enumerate(self.guards):
            t.copy_(rnd(t.numel(), seed=seed + i, dtype=t.dtype) if seed is not None else torch.full_like(t, float("nan")))


def _isolation_run(lib, dt, B, N, H, kb, kh, hostile, cls):
    """One forward + backward with every buffer guarded.  Both runs hold the same bits for sample kb, head kh; `hostile` replaces
    everything else in qkv / dout by other data at 100 x the magnitude and fills every guard a kernel could read with NaN."""
    scale = 64 ** -0.5
    qkv, dout = _Guarded(B * N, 3 * H * 64, dt), _Guarded(B * N, H * 64, dt)
    out, dqkv = _Guarded(B * N, H * 64, dt), _Guarded(B * N, 3 * H * 64, dt)
    lse = _Guarded(B * H, N, torch.float32)
    rows = slice(kb * N, (kb + 1) * N)
    base_qkv, base_dout = rnd(B * N, 3 * H * 64, seed=1, dtype=dt), rnd(B * N, H * 64, seed=2, dtype=dt)
    if hostile:
        qkv.t.copy_(rnd(B * N, 3 * H * 64, seed=11, scale=100.0, dtype=dt))
        dout.t.copy_(rnd(B * N, H * 64, seed=12, scale=100.0, dtype=dt))
        for part in range(3):
            cols = slice(part * H * 64 + kh * 64, part * H * 64 + kh * 64 + 64)
            qkv.t[rows, cols] = base_qkv[rows, cols]
        dout.t[rows, kh * 64:kh * 64 + 64] = base_dout[rows, kh * 64:kh * 64 + 64]
    else:
        qkv.t.copy_(base_qkv)
        dout.t.copy_(base_dout)
    qkv.fill_guards(None if hostile else 21)
    dout.fill_guards(None if hostile else 23)
    for t in (out, lse, dqkv):
        t.set_sentinels()
    lse3 = lse.t.view(B, H, N)
    _fwd(lib, qkv.t, B, N, H, scale, out=out.t, lse=lse3, cls=cls)
    torch.cuda.synchronize()
    assert out.sentinels_intact() and lse.sentinels_intact(), "the forward wrote outside out / lse"
    if cls:   # only the cls rows are written
        other = torch.ones(B * N, dtype=torch.bool, device=DEV)
        other[torch.arange(B, device=DEV) * N] = False
        assert bool((out.t[other].view(out.idt) == out.word).all()) and bool((lse3[:, :, 1:].contiguous().view(lse.idt) == lse.word).all())
        assert not torch.isnan(out.t[~other]).any() and not torch.isnan(lse3[:, :, 0]).any()
    else:
        assert not torch.isnan(out.t).any() and not torch.isnan(lse.t).any()
    # out and lse are inputs of the backward: their guards turn into input guards
    out.fill_guards(None if hostile else 25)
    lse.fill_guards(None if hostile else 27)
    _bwd(lib, qkv.t, out.t, dout.t, lse3, B, N, H, scale, dqkv=dqkv.t, cls=cls)
    torch.cuda.synchronize()
    assert dqkv.sentinels_intact(), "the backward wrote outside dqkv"
    assert not torch.isnan(dqkv.t).any()
    kept = [out.t[rows, kh * 64:kh * 64 + 64], lse3[kb, kh]]
    kept += [dqkv.t[rows, part * H * 64 + kh * 64:part * H * 64 + kh * 64 + 64] for part in range(3)]
    return [k.clone() for k in kept]


@pytest.mark.parametrize("cls", [False, True], ids=["full", "cls"])
@pytest.mark.parametrize("keep", ["middle", "last"])
@pytest.mark.parametrize("N", [33, 97, 197, 300, 785])
@pytest.mark.parametrize("operands", OPERANDS)
def test_a_head_depends_on_nothing_but_its_own_rows(operands, N, keep, cls):
    """Ragged tails on every path: for n >= N the rows a tile touches belong to the next sample, past the last sample (keep =
    "last": sample 2, head 2) they lie behind the buffer.  A tail leaking at weight 1 / N hides inside every tolerance; it cannot
    hide from torch.equal, nor from a NaN."""
    B, H = 3, 3
    lib, dt = L().lib(operands), L().act_dtype(operands)
    kb, kh = (1, 1) if keep == "middle" else (B - 1, H - 1)
    first = _isolation_run(lib, dt, B, N, H, kb, kh, False, cls)
    second = _isolation_run(lib, dt, B, N, H, kb, kh, True, cls)
    for name, a, b in zip(("out", "lse", "dQ", "dK", "dV"), first, second):
        assert torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                           b.view(torch.int16 if b.element_size() == 2 else torch.int32)), \
            f"{name} of sample {kb}, head {kh} changed with the other samples / heads / guards: {int((a != b).sum())} of {a.numel()} elements"
