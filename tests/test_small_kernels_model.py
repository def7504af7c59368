"""The contract of the kernels around the blocks, proven on the host before a GPU is involved (oracle/small_kernels.py):

* with rounding switched off every restatement IS the operation: float64 torch (layer_norm and its autograd, cross_entropy,
  torch.optim.AdamW) to 1e-12 relative;
* an fp32 restatement of each kernel in ANOTHER summation order (reduction trees of the kernels' depth, other leaves) stays inside
  every derived bound at every case the device tests run, using at most HALF of each cap on neighbour cases;
* each of ten plausible slips put into that fp32 restatement breaks a bound on at least one case -- the old fixed tolerance of
  tests/test_kernels_gpu.py is printed beside it (-s; docs/findings/small_kernels_contract.md has the table).

The case builders (tests/small_kernels_common.py) are the ones tests/test_small_kernels_gpu.py runs on the device."""
import math

import pytest
import torch

from oracle import small_kernels as K
from tests import tolerances as T

from tests.small_kernels_common import (  # noqa: F401
    ADAMW_HYPER, ADAMW_SIZES, ADAMW_STEPS, DTYPES, EPS, FAMILIES, HEAD_BWD_CASES, HEAD_FWD_CASES, LN_C, LN_M_FUSED,
    LN_M_PLAIN, Shares, XENT_B, XENT_C, XU_RANKS, _cap, _gen, adamw_f32, adamw_inputs, check_16, check_32, fails_16,
    fails_32, family_rows, head_bwd_f32, head_bwd_inputs, head_fwd_inputs, ln_bwd_f32, ln_bwd_inputs, ln_fwd_f32,
    ln_params, share, tree_sum, xent_f32, xent_inputs, xu_f32, xu_factor)


# --- 1. rounding off: the restatements are the operations --------------------------------------------------------------------
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_restatements_equal_float64_torch():
    x, _ = family_rows(9, 768)
    g, b = ln_params(768)
    xd = x.double().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xd, (768,), g.double(), b.double(), EPS)
    f = K.ln_fwd(x, g, b, EPS)
    assert _rel(f["y"][0], ref.detach()) < 1e-12
    dy, dx_in, rs = ln_bwd_inputs(9, 768, torch.float64, 7)
    ref.backward(dy)
    bw = K.ln_bwd(dy, x, g, f["mean"][0], f["rstd"][0], dx_in, rs, 7)
    # (the all-zero and constant rows have rstd = 1000 and a gradient that cancels to ~1e-13 of its terms: absolute there)
    assert _rel(bw["dx"][0], dx_in.double() + xd.grad) < 1e-12
    assert _rel(bw["dyb"][0], (dx_in.double() + xd.grad) * rs.double().repeat_interleave(7)[:9, None]) < 1e-12
    # head: LayerNorm + linear, and the linear's autograd
    x, gm, bt, W, hb = head_fwd_inputs(3, 10, 1024)
    h = K.head_fwd(x, gm, bt, W, hb, EPS)
    xn = torch.nn.functional.layer_norm(x.double(), (1024,), gm.double(), bt.double(), EPS)
    assert _rel(h["logits"][0], xn @ W.double().t() + hb.double()) < 1e-12
    dl, xn, W = head_bwd_inputs(5, 257, 768, torch.float64)
    xr, Wr, br = xn.clone().requires_grad_(True), W.double().requires_grad_(True), torch.zeros(257, dtype=torch.float64, requires_grad=True)
    (xr @ Wr.t() + br).backward(dl.double())
    hb_ = K.head_bwd(dl, xn, W)
    assert _rel(hb_["dW"][0], Wr.grad) < 1e-12 and _rel(hb_["db"][0], br.grad) < 1e-12 and _rel(hb_["dxn"][0], xr.grad) < 1e-12
    # cross-entropy with dscale x loss scale
    l, y = xent_inputs(5, 1000)
    ld = l.double().requires_grad_(True)
    rl = torch.nn.functional.cross_entropy(ld, y)
    (rl * 128.0).backward()
    xe = K.xent(l, y, 0.25, 512.0)
    assert abs(float(xe["loss"][0]) - float(rl.detach())) <= 1e-12 * abs(float(rl.detach())) and _rel(xe["dlogits"][0], ld.grad) < 1e-12
    # AdamW, both forms' common formulas, five steps
    p, gr, m, v = (t.double() for t in adamw_inputs(1025, 1))
    rp = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([rp], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for step in range(1, 6):
        rp.grad = gr * step
        opt.step()
        o = K.adamw(p, gr * step, m, v, step=step, rounding=False, **ADAMW_HYPER)
        p, m, v = o["p"][0], o["m"][0], o["v"][0]
        assert _rel(p, rp.detach()) < 1e-12 and _rel(m, opt.state[rp]["exp_avg"]) < 1e-12 and _rel(v, opt.state[rp]["exp_avg_sq"]) < 1e-12


# --- 2. the fp32 other-order restatement stays inside every bound, with at most half of each cap ----------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", LN_C)
def test_other_order_layernorm_inside_the_bounds(C, dt):
    for M in sorted(set(LN_M_FUSED + LN_M_PLAIN)):
        x, fam = family_rows(M, C)
        g, b = ln_params(C)
        print(f"LN C={C} M={M} {dt}")
        mu, rs, _, y16 = ln_fwd_f32(x, g, b, dt)
        f = K.ln_fwd(x, g, b, EPS)
        check_32("mean", mu, f["mean"])
        check_32("rstd", rs, f["rstd"])
        check_16("y", y16, f["y"], dt, T.SMALL_CAPS["ln_y"], 0.5, fam)
        for rps in (1, 7):
            dy, dx_in, sc = ln_bwd_inputs(M, C, dt, rps)
            dx, dyb = ln_bwd_f32(dy, x, g, mu, rs, dx_in, sc, rps, dt)
            bw = K.ln_bwd(dy, x, g, mu, rs, dx_in, sc, rps)
            check_32("dx", dx, bw["dx"])
            check_16("dyb", dyb, bw["dyb"], dt, T.SMALL_CAPS["ln_dyb"], 0.5, fam)


@pytest.mark.parametrize("rank,Rp", XU_RANKS)
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", LN_C)
def test_other_order_fused_contraction_inside_the_bound(C, dt, rank, Rp):
    """T = y U and G' = dyb U of the fused kernels from the 16-bit rows the fp32 LayerNorm restatement leaves; neighbour cases are
    counted over all M of one (C, rank, build), as the device test counts them"""
    Ut = xu_factor(Rp, C, rank, dt)
    for name in ("T", "G'"):
        sh, worst = Shares(), 0.0
        for M in LN_M_FUSED:
            x, _ = family_rows(M, C)
            g, b = ln_params(C)
            mu, rs, _, y16 = ln_fwd_f32(x, g, b, dt)
            if name == "G'":
                dy, dx_in, sc = ln_bwd_inputs(M, C, dt, 7)
                _, y16 = ln_bwd_f32(dy, x, g, mu, rs, dx_in, sc, 7, dt)
                y16 = torch.nan_to_num(y16, posinf=0.0, neginf=0.0)
            ok, ratio = sh.add(xu_f32(y16, Ut, dt), K.xu_contract(y16, Ut)["T"], dt)
            worst = max(worst, ratio)
            assert ok.all(), f"{name} C={C} M={M}: {int((~ok).sum())} outside the derived bound (worst ratio {ratio:.3f})"
        print(f"XU {name} C={C} {dt} rank={rank}: worst/bound {worst:.3f}  neighbours {sh.n}/{sh.total} = {sh.share:.4f} (cap {T.SMALL_CAPS['xu_T']})")
        assert sh.share <= 0.5 * T.SMALL_CAPS["xu_T"]


def test_slip_in_the_fused_contraction_breaks_the_bound():
    caught = []
    for C in LN_C:
        for M in LN_M_FUSED:
            x, _ = family_rows(M, C)
            g, b = ln_params(C)
            y16 = ln_fwd_f32(x, g, b, torch.bfloat16)[3]
            Ut = xu_factor(32, C, 32, torch.bfloat16)
            if not K.hold_16(xu_f32(y16, Ut, torch.bfloat16, slip="last_panel"), *K.xu_contract(y16, Ut)["T"], torch.bfloat16)[0].all():
                caught.append((C, M))
    print(f"SLIP last K panel of the contraction left out: new bound fails at {len(caught)} of {len(LN_C) * len(LN_M_FUSED)} cases")
    assert caught


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_other_order_head_inside_the_bounds(dt):
    for B, classes, D, _ in HEAD_FWD_CASES:
        x, gm, bt, W, hb = head_fwd_inputs(B, classes, D)
        fam = family_rows(B, D, seed=3)[1]
        print(f"head fwd {B} {classes} {D} {dt}")
        mu, rs, xn, xn16 = ln_fwd_f32(x, gm, bt, dt, lanes=256)
        logits = torch.stack([tree_sum(W.float() * xn[i], 256) for i in range(B)]) + hb.float()
        h = K.head_fwd(x, gm, bt, W, hb, EPS)
        check_32("mean", mu, h["mean"])
        check_32("rstd", rs, h["rstd"])
        check_32("logits", logits, h["logits"])
        check_16("xn16", xn16, h["xn16"], dt, T.SMALL_CAPS["head_xn16"], 0.5, fam)
    for B, classes, D in HEAD_BWD_CASES:
        dl, xn, W = head_bwd_inputs(B, classes, D, dt)
        print(f"head bwd {B} {classes} {D} {dt}")
        dW, db, dxn = head_bwd_f32(dl, xn, W, dt)
        hb_ = K.head_bwd(dl, xn, W)
        check_32("dW", dW, hb_["dW"])
        check_32("db", db, hb_["db"])
        check_16("dxn", dxn, hb_["dxn"], dt, T.SMALL_CAPS["head_dxn"], 0.5)


def test_other_order_cross_entropy_inside_the_bounds():
    for C in XENT_C:
        for B in XENT_B:
            l, y = xent_inputs(B, C)
            print(f"xent B={B} C={C}")
            for dscale, ls in ((1.0, 1.0), (0.25, 512.0)):
                term, loss, dl = xent_f32(l, y, dscale, ls)
                xe = K.xent(l, y, dscale, ls)
                check_32("terms", term, xe["terms"])
                check_32("loss", loss, xe["loss"])
                check_32("dlogits", dl, xe["dlogits"])


def test_other_order_adamw_inside_the_bounds():
    for n in ADAMW_SIZES:
        for step in ADAMW_STEPS:
            p, g, m, v = adamw_inputs(n, step)
            p2, m2, v2 = adamw_f32(p, g, m, v, step=step, **ADAMW_HYPER)
            for dyn in (False, True):
                print(f"adamw n={n} step={step} dyn={dyn}")
                o = K.adamw(p, g, m, v, step=step, dyn=dyn, **ADAMW_HYPER)
                check_32("p", p2, o["p"])
                check_32("m", m2, o["m"])
                check_32("v", v2, o["v"])


# --- 3. every slip breaks a bound on at least one listed case ---------------------------------------------------------------
def _old_close(got, ref, rtol, atol):
    """the fixed bar tests/test_kernels_gpu.py held before: |got - ref| <= atol + rtol |ref|"""
    return bool(((got.double() - ref).abs() <= atol + rtol * ref.abs()).all())


LN_SLIPS = ["var_c_minus_1", "no_eps", "one_pass", "rstd_1e-4"]


@pytest.mark.parametrize("slip", LN_SLIPS)
def test_slips_in_the_layernorm_forward_break_a_bound(slip):
    dt, caught, old_caught = torch.bfloat16, [], False
    for C in LN_C:
        for M in LN_M_FUSED:
            x, fam = family_rows(M, C)
            g, b = ln_params(C)
            mu, rs, _, y16 = ln_fwd_f32(x, g, b, dt, slip=slip)
            f = K.ln_fwd(x, g, b, EPS)
            if fails_32(mu, f["mean"]) or fails_32(rs, f["rstd"]) or fails_16(y16, f["y"], dt, T.SMALL_CAPS["ln_y"], fam):
                caught.append((C, M))
            # the old test: Gaussian 2 randn + 0.5 rows, y to 2^-8 |ref| + 1e-3, the mean to 1e-5 + 1e-5 |ref|, rstd not at all
            xo = 2 * torch.randn(max(M, 33), C, generator=_gen(1)) + 0.5
            muo, _, _, yo = ln_fwd_f32(xo, g, b, dt, slip=slip)
            fo = K.ln_fwd(xo, g, b, EPS)
            old_caught |= not (_old_close(yo, fo["y"][0], 2 ** -8, 1e-3) and _old_close(muo, fo["mean"][0], 1e-5, 1e-5))
    print(f"SLIP {slip}: new bound fails at {len(caught)} of {len(LN_C) * len(LN_M_FUSED)} cases; old fixed tolerance "
          f"(2^-8 rel + 1e-3 on Gaussian rows) {'caught' if old_caught else 'PASSED'} it")
    assert caught


@pytest.mark.parametrize("slip", ["no_c2", "rowscale_rps_plus_1"])
def test_slips_in_the_layernorm_backward_break_a_bound(slip):
    dt, caught, old_caught = torch.bfloat16, [], False
    for C in LN_C:
        for M in LN_M_FUSED:
            x, fam = family_rows(M, C)
            g, b = ln_params(C)
            mu, rs, _, _ = ln_fwd_f32(x, g, b, dt)
            dy, dx_in, sc = ln_bwd_inputs(M, C, dt, 7)
            dx, dyb = ln_bwd_f32(dy, x, g, mu, rs, dx_in, sc, 7, dt, slip=slip)
            bw = K.ln_bwd(dy, x, g, mu, rs, dx_in, sc, 7)
            if fails_32(dx, bw["dx"]) or fails_16(dyb, bw["dyb"], dt, T.SMALL_CAPS["ln_dyb"], fam):
                caught.append((C, M))
        # the old test: Gaussian 2 randn + 0.5 rows (M = 64 and 33 there), the row scale (i % 3) / 2 with 7 rows per sample,
        # dx to 1e-4 + 1e-4 |ref| and dyb to 2^-8 |ref| + 1e-3
        go = _gen(C)
        Mo = 64
        xo = 2 * torch.randn(Mo, C, generator=go) + 0.5
        dyo, dxo = torch.randn(Mo, C, generator=go).to(dt), torch.randn(Mo, C, generator=go)
        sco = (torch.arange((Mo + 6) // 7) % 3).float() * 0.5
        muo, rso, _, _ = ln_fwd_f32(xo, g, b, dt)
        dx, dyb = ln_bwd_f32(dyo, xo, g, muo, rso, dxo, sco, 7, dt, slip=slip)
        bo = K.ln_bwd(dyo, xo, g, muo, rso, dxo, sco, 7)
        old_caught |= not (_old_close(dx, bo["dx"][0], 1e-4, 1e-4) and _old_close(dyb, bo["dyb"][0], 2 ** -8, 1e-3))
    print(f"SLIP {slip}: new bound fails at {len(caught)} of {len(LN_C) * len(LN_M_FUSED)} cases; old fixed tolerance "
          f"(dx 1e-4 + 1e-4, dyb 2^-8 + 1e-3 on the old test's Gaussian rows) {'caught' if old_caught else 'PASSED'} it")
    assert caught


@pytest.mark.parametrize("slip", ["t_minus_1", "decay_after"])
def test_slips_in_adamw_break_a_bound(slip):
    caught, old_caught = [], False
    for n in ADAMW_SIZES:
        for step in ADAMW_STEPS:
            p, g, m, v = adamw_inputs(n, step)
            p2, m2, v2 = adamw_f32(p, g, m, v, step=step, slip=slip, **ADAMW_HYPER)
            o = K.adamw(p, g, m, v, step=step, **ADAMW_HYPER)
            if not torch.isfinite(p2).all() or fails_32(p2, o["p"]):
                caught.append((n, step))
            old_caught |= not _old_close(torch.nan_to_num(p2, nan=1e30), o["p"][0], 2e-6, 2e-7)
    print(f"SLIP {slip}: new bound fails at {len(caught)} of {len(ADAMW_SIZES) * 2} cases; old fixed tolerance (2e-6 rel + 2e-7) "
          f"{'caught' if old_caught else 'PASSED'} it")
    assert caught


def test_slip_in_the_cross_entropy_scale_breaks_a_bound():
    caught, old_caught = [], False
    for C in XENT_C:
        for B in XENT_B:
            l, y = xent_inputs(B, C)
            _, _, dl = xent_f32(l, y, slip="B_plus_1")
            xe = K.xent(l, y)
            if fails_32(dl, xe["dlogits"]):
                caught.append((B, C))
            old_caught |= not _old_close(dl, xe["dlogits"][0], 1e-4, 1e-7)
    print(f"SLIP softmax - onehot over B + 1: new bound fails at {len(caught)} of {len(XENT_C) * 2} cases; old fixed tolerance "
          f"(1e-4 rel + 1e-7) {'caught' if old_caught else 'PASSED'} it")
    assert caught


def test_slip_in_the_head_bias_gradient_breaks_a_bound():
    caught = []
    for B, classes, D in HEAD_BWD_CASES:
        dl, xn, W = head_bwd_inputs(B, classes, D, torch.bfloat16)
        _, db, _ = head_bwd_f32(dl, xn, W, torch.bfloat16, slip="db_B_minus_1")
        if fails_32(db, K.head_bwd(dl, xn, W)["db"]):
            caught.append((B, classes, D))
    print(f"SLIP db over B - 1 samples: new bound fails at {len(caught)} of {len(HEAD_BWD_CASES)} cases; no old test of "
          "cara_head_backward existed (whole-model runs only): PASSED")
    assert caught
