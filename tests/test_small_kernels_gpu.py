"""The kernels around the blocks on the device, in both operand builds, held to the derived bounds of oracle/small_kernels.py (proven
attainable on the host by tests/test_small_kernels_model.py, whose case builders run here): the LayerNorm family (plain, fused
contraction, K-panel images, strided rows), the fp32 head forward and backward, cross-entropy with its label guard, the transposes,
the fp32 -> 16-bit conversion and AdamW in its host and dyn forms.  Besides the values: nothing is written outside an output
(sentinel rows / columns / words of the 0x5A5A pattern around every one), a row's outputs do not depend on any other row, and the
fused and plain forms agree bit for bit.  Figures are printed (-s) before they are asserted; docs/findings/small_kernels_contract.md
holds the tables."""
import ctypes as C
import math

import pytest
import torch

from oracle import small_kernels as K
from tests import tolerances as T
from tests import small_kernels_common as S
from tests.test_kernels_gpu import DEV, L

pytestmark = pytest.mark.gpu

OPERANDS = ["bf16", "fp16"]
GUARD = 16
SENT = {2: (torch.int16, 0x5A5A), 4: (torch.int32, 0x5A5A5A5A)}   # finite in bf16, fp16 and fp32


def sentinel(shape, dtype):
    it, val = SENT[torch.empty(0, dtype=dtype).element_size()]
    return torch.full(shape, val, dtype=it, device=DEV).view(dtype)


def is_sentinel(t):
    it, val = SENT[t.element_size()]
    return bool((t.contiguous().view(it) == val).all())


def guarded(rows, cols, dtype):
    """-> (whole allocation of rows + GUARD sentinel rows, its first `rows` rows)"""
    full = sentinel((rows + GUARD, cols), dtype)
    return full, full[:rows]


def panels(X):
    M, Kc = X.shape
    return X.view(M, Kc // 32, 32).permute(1, 0, 2).contiguous()


def _check_T(name, Tdev, y16, Ut, dt, shares):
    """T = (16-bit)(y U) of the fused kernels from the 16-bit rows they staged, held to oracle.small_kernels.xu_contract; the
    neighbour cases are added to `shares`, which the test caps over all its M (tolerances.SMALL_CAPS["xu_T"])"""
    ok, ratio = shares.add(Tdev, K.xu_contract(y16, Ut)["T"], dt)
    print(f"  {name}: worst/bound {ratio:.3f}  neighbours so far {shares.n}/{shares.total}")
    assert ok.all(), f"{name}: {int((~ok).sum())}/{ok.numel()} outside the derived bound (worst ratio {ratio:.3f})"


class _Ln:
    """one fused forward + backward launch pair with guards on every output"""

    def __init__(self, lib, dt, x, g, b, Ut, rank, Rp, dy, dx_in, rs, rps, yp=0):
        p, st = L().ptr, L().stream
        M, Cc = x.shape
        self.ldt = (M + 31) // 32 * 32 + 32                      # 32 sentinel columns beyond roundup32(M)
        self.y_full, self.y = (sentinel((Cc // 32, yp, 32), dt),) * 2 if yp else guarded(M, Cc, dt)
        self.mean_full, self.mean = guarded(M, 1, torch.float32)
        self.rstd_full, self.rstd = guarded(M, 1, torch.float32)
        self.T_full, self.T = guarded(M, Rp, dt)
        self.Tt = sentinel((Rp, self.ldt), dt)
        L().check(lib.cara_layernorm_fwd_ex(p(x), C.c_long(Cc), p(g), p(b), p(self.y_full), p(self.mean_full), p(self.rstd_full), M, Cc,
                                            C.c_float(S.EPS), p(Ut), rank, Rp, p(self.T_full), p(self.Tt), self.ldt, yp, st()), "ln fwd ex")
        self.dx_full, self.dx = guarded(M, Cc, torch.float32)
        self.dyb_full, self.dyb = (sentinel((Cc // 32, yp, 32), dt),) * 2 if yp else guarded(M, Cc, dt)
        self.G_full, self.G = guarded(M, Rp, dt)
        self.Gt = sentinel((Rp, self.ldt), dt)
        L().check(lib.cara_layernorm_bwd_ex(p(dy), p(x), C.c_long(Cc), p(g), p(self.mean_full), p(self.rstd_full), p(dx_in), p(self.dx_full),
                                            p(self.dyb_full), p(rs), rps, M, Cc, p(Ut), rank, Rp, p(self.G_full), p(self.Gt), self.ldt, yp,
                                            st()), "ln bwd ex")
        torch.cuda.synchronize()


@pytest.mark.parametrize("rank,Rp", S.XU_RANKS)
@pytest.mark.parametrize("C_", S.LN_C)
@pytest.mark.parametrize("operands", OPERANDS)
def test_layernorm_fused_forms(operands, C_, rank, Rp):
    """cara_layernorm_fwd_xu / _bwd_xu / _fwd_ex / _bwd_ex at M = one partial block .. two blocks and a row, all row families in
    one launch, the row scale 0, 1 and 1 / (1 - p) in one launch, rows_per_sample 1 and 7.
    The OFFSET rows (mean 100, spread 1e-2) are not under the neighbour rule: their derived term is several 16-bit steps of y, so
    y is held to that multi-step interval alone, with no cap on the share (tests/tolerances.py); what checks those rows sharply is
    mean and rstd."""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    p, st = L().ptr, L().stream
    sh_T, sh_G = S.Shares(), S.Shares()
    for M in S.LN_M_FUSED:
        xh, fam = S.family_rows(M, C_)
        gh, bh = S.ln_params(C_)
        x, g, b = xh.to(DEV), gh.to(DEV), bh.to(DEV)
        Ut = S.xu_factor(Rp, C_, rank, dt).to(DEV)
        print(f"\nLN fused {operands} C={C_} M={M} rank={rank}")
        for rps in (1, 7):
            dyh, dxh, rsh = S.ln_bwd_inputs(M, C_, dt, rps)
            dy, dx_in, rs = dyh.to(DEV), dxh.to(DEV), rsh.to(DEV)
            r = _Ln(lib, dt, x, g, b, Ut, rank, Rp, dy, dx_in, rs, rps)
            f = K.ln_fwd(xh, gh, bh, S.EPS)
            S.check_32("mean", r.mean[:, 0], f["mean"])
            S.check_32("rstd", r.rstd[:, 0], f["rstd"])
            S.check_16("y", r.y, f["y"], dt, T.SMALL_CAPS["ln_y"], fam=fam)
            _check_T("T", r.T, r.y, Ut, dt, sh_T)
            bw = K.ln_bwd(dyh, xh, gh, r.mean[:, 0], r.rstd[:, 0], dxh, rsh, rps)
            S.check_32("dx", r.dx, bw["dx"])
            S.check_16("dyb", r.dyb, bw["dyb"], dt, T.SMALL_CAPS["ln_dyb"])
            _check_T("G'", r.G, r.dyb, Ut, dt, sh_G)
            # nothing beyond M: guard rows, and of Tt / Gt everything but the zeroed [M, roundup32(M)) columns
            m32 = (M + 31) // 32 * 32
            for full in (r.y_full, r.mean_full, r.rstd_full, r.T_full, r.dx_full, r.dyb_full, r.G_full):
                assert is_sentinel(full[M:])
            for tt, t in ((r.Tt, r.T), (r.Gt, r.G)):
                assert torch.equal(tt[:, :M], t.t()) and torch.count_nonzero(tt[:, M:m32].view(torch.int16)) == 0 and is_sentinel(tt[:, m32:])
            assert torch.count_nonzero(r.T[:, rank:].view(torch.int16)) == 0
            # the plain forms: bitwise the same y, mean, rstd, dx, dyb
            y2, dyb2 = sentinel((M, C_), dt), sentinel((M, C_), dt)
            mean2, rstd2, dx2 = sentinel((M,), torch.float32), sentinel((M,), torch.float32), sentinel((M, C_), torch.float32)
            L().check(lib.cara_layernorm_fwd(p(x), C.c_long(C_), p(g), p(b), p(y2), p(mean2), p(rstd2), M, C_, C.c_float(S.EPS), st()), "ln")
            L().check(lib.cara_layernorm_bwd(p(dy), p(x), C.c_long(C_), p(g), p(mean2), p(rstd2), p(dx_in), p(dx2), p(dyb2), p(rs), rps, M,
                                             C_, st()), "ln bwd")
            assert torch.equal(y2, r.y) and torch.equal(mean2, r.mean[:, 0]) and torch.equal(rstd2, r.rstd[:, 0])
            assert torch.equal(dx2, r.dx) and torch.equal(dyb2, r.dyb)
        # K-panel images with y_panels = M + 5: the same bits, nothing in the five rows beyond M of any panel
        q = _Ln(lib, dt, x, g, b, Ut, rank, Rp, dy, dx_in, rs, rps, yp=M + 5)
        assert torch.equal(q.y[:, :M], panels(r.y)) and is_sentinel(q.y[:, M:])
        assert torch.equal(q.dyb[:, :M], panels(r.dyb)) and is_sentinel(q.dyb[:, M:])
        assert torch.equal(q.T, r.T) and torch.equal(q.G, r.G) and torch.equal(q.dx, r.dx) and torch.equal(q.Tt, r.Tt)
        # row isolation: other finite values in one row of x change no other row of any output
        k = M // 2
        x2 = x.clone()
        x2[k] = torch.randn(C_, generator=torch.Generator().manual_seed(M)).to(DEV) * 5 - 2
        r2 = _Ln(lib, dt, x2, g, b, Ut, rank, Rp, dy, dx_in, rs, rps)
        keep = [i for i in range(M) if i != k]
        for a, c in ((r.y, r2.y), (r.mean, r2.mean), (r.rstd, r2.rstd), (r.T, r2.T), (r.dx, r2.dx), (r.dyb, r2.dyb), (r.G, r2.G)):
            assert torch.equal(a[keep], c[keep])
        assert M == 1 or not torch.equal(r.y[k], r2.y[k])
    cap = T.SMALL_CAPS["xu_T"]
    print(f"XU {operands} C={C_} rank={rank}: neighbour cases over all M: T {sh_T.share:.4f}  G' {sh_G.share:.4f}  (cap {cap:g})")
    assert sh_T.share <= cap and sh_G.share <= cap, (sh_T.share, sh_G.share, cap)


@pytest.mark.parametrize("C_", S.LN_C)
@pytest.mark.parametrize("operands", OPERANDS)
def test_layernorm_plain_forms_and_strided_backward(operands, C_):
    """cara_layernorm_fwd / _bwd (four rows per block) at M = 1, 3, 4, 5, 9 with guards; then the final norm's backward: rows
    3 C apart, no running gradient, rows_per_sample = 1, dyb given and NULL -- every element between the strided rows untouched.
    (Offset rows: held to their multi-step interval without a cap, see test_layernorm_fused_forms.)"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    p, st = L().ptr, L().stream
    for M in S.LN_M_PLAIN:
        xh, fam = S.family_rows(M, C_)
        gh, bh = S.ln_params(C_)
        x, g, b = xh.to(DEV), gh.to(DEV), bh.to(DEV)
        print(f"\nLN plain {operands} C={C_} M={M}")
        y_full, y = guarded(M, C_, dt)
        mean_full, mean = guarded(M, 1, torch.float32)
        rstd_full, rstd = guarded(M, 1, torch.float32)
        L().check(lib.cara_layernorm_fwd(p(x), C.c_long(C_), p(g), p(b), p(y_full), p(mean_full), p(rstd_full), M, C_, C.c_float(S.EPS),
                                         st()), "ln")
        f = K.ln_fwd(xh, gh, bh, S.EPS)
        S.check_32("mean", mean[:, 0], f["mean"])
        S.check_32("rstd", rstd[:, 0], f["rstd"])
        S.check_16("y", y, f["y"], dt, T.SMALL_CAPS["ln_y"], fam=fam)
        for rps in (1, 7):
            dyh, dxh, rsh = S.ln_bwd_inputs(M, C_, dt, rps)
            dy, dx_in, rs = dyh.to(DEV), dxh.to(DEV), rsh.to(DEV)   # (held in names: a temporary would be freed before the launch)
            dx_full, dx = guarded(M, C_, torch.float32)
            dyb_full, dyb = guarded(M, C_, dt)
            L().check(lib.cara_layernorm_bwd(p(dy), p(x), C.c_long(C_), p(g), p(mean_full), p(rstd_full), p(dx_in),
                                             p(dx_full), p(dyb_full), p(rs), rps, M, C_, st()), "ln bwd")
            bw = K.ln_bwd(dyh, xh, gh, mean[:, 0], rstd[:, 0], dxh, rsh, rps)
            S.check_32("dx", dx, bw["dx"])
            S.check_16("dyb", dyb, bw["dyb"], dt, T.SMALL_CAPS["ln_dyb"])
            for full in (y_full, mean_full, rstd_full, dx_full, dyb_full):
                assert is_sentinel(full[M:])
        # row isolation of the plain forms: other finite values in one row change no other row of y, mean, rstd, dx, dyb
        k = M // 2
        x2 = x.clone()
        x2[k] = torch.randn(C_, generator=torch.Generator().manual_seed(M)).to(DEV) * 5 - 2
        y2, dyb2 = sentinel((M, C_), dt), sentinel((M, C_), dt)
        mean2, rstd2, dx2 = sentinel((M, 1), torch.float32), sentinel((M, 1), torch.float32), sentinel((M, C_), torch.float32)
        L().check(lib.cara_layernorm_fwd(p(x2), C.c_long(C_), p(g), p(b), p(y2), p(mean2), p(rstd2), M, C_, C.c_float(S.EPS), st()), "ln")
        L().check(lib.cara_layernorm_bwd(p(dy), p(x2), C.c_long(C_), p(g), p(mean2), p(rstd2), p(dx_in), p(dx2), p(dyb2), p(rs), rps, M,
                                         C_, st()), "ln bwd")
        keep = [i for i in range(M) if i != k]
        for a, c in ((y, y2), (mean, mean2), (rstd, rstd2), (dx, dx2), (dyb, dyb2)):
            assert torch.equal(a[keep], c[keep])
        assert M == 1 or not torch.equal(y[k], y2[k])
        # strided: x, dx_out and dyb at row * 3 C, dy at row * C
        ldx = 3 * C_
        xs = torch.randn(M, ldx, generator=torch.Generator().manual_seed(5)).to(DEV)
        xs[:, :C_] = x
        dyh, _, rsh = S.ln_bwd_inputs(M, C_, dt, 1)
        dy, rs = dyh.to(DEV), rsh.to(DEV)
        L().check(lib.cara_layernorm_fwd(p(xs), C.c_long(ldx), p(g), p(b), p(y_full), p(mean_full), p(rstd_full), M, C_, C.c_float(S.EPS),
                                         st()), "ln strided")
        bw = K.ln_bwd(dyh, xh, gh, mean[:, 0], rstd[:, 0], None, rsh, 1)
        for with_dyb in (True, False):
            dxs, dybs = sentinel((M + 1, ldx), torch.float32), sentinel((M + 1, ldx), dt)
            L().check(lib.cara_layernorm_bwd(p(dy), p(xs), C.c_long(ldx), p(g), p(mean_full), p(rstd_full), None, p(dxs),
                                             p(dybs) if with_dyb else None, p(rs), 1, M, C_, st()), "ln bwd strided")
            S.check_32("dx strided", dxs[:M, :C_], bw["dx"])
            assert is_sentinel(dxs[:M, C_:]) and is_sentinel(dxs[M:])
            if with_dyb:
                S.check_16("dyb strided", dybs[:M, :C_], bw["dyb"], dt, T.SMALL_CAPS["ln_dyb"])
                assert is_sentinel(dybs[:M, C_:]) and is_sentinel(dybs[M:])
            else:
                assert is_sentinel(dybs)


# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,classes,D,tokens", S.HEAD_FWD_CASES)
@pytest.mark.parametrize("operands", OPERANDS)
def test_head_forward_on_the_row_families(operands, B, classes, D, tokens):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    p, st = L().ptr, L().stream
    xh, gh, bh, Wh, hbh = S.head_fwd_inputs(B, classes, D)
    fam = S.family_rows(B, D, seed=3)[1]
    x = torch.randn(B, tokens, D, generator=torch.Generator().manual_seed(2)).to(DEV)
    x[:, 0] = xh.to(DEV)
    xn_full, xn16 = guarded(B, D, dt)
    lg_full, logits = guarded(B, classes, torch.float32)
    mean, rstd = sentinel((B + 1,), torch.float32), sentinel((B + 1,), torch.float32)
    g, b, W, hb = gh.to(DEV), bh.to(DEV), Wh.to(DEV), hbh.to(DEV)
    L().check(lib.cara_head_forward(p(x), C.c_long(tokens * D), p(g), p(b), p(W), p(hb), p(xn_full),
                                    p(mean), p(rstd), p(lg_full), B, classes, D, C.c_float(S.EPS), st()), "head fwd")
    h = K.head_fwd(xh, gh, bh, Wh, hbh, S.EPS)
    print(f"\nhead fwd {operands} {B} {classes} {D}")
    S.check_32("mean", mean[:B], h["mean"])
    S.check_32("rstd", rstd[:B], h["rstd"])
    S.check_32("logits", logits, h["logits"])
    S.check_16("xn16", xn16, h["xn16"], dt, T.SMALL_CAPS["head_xn16"], fam=fam)
    assert is_sentinel(xn_full[B:]) and is_sentinel(lg_full[B:]) and is_sentinel(mean[B:]) and is_sentinel(rstd[B:])


@pytest.mark.parametrize("B,classes,D", S.HEAD_BWD_CASES)
@pytest.mark.parametrize("operands", OPERANDS)
def test_head_backward(operands, B, classes, D):
    """cara_head_backward alone: dW, db, dxn against the float64 restatement, guard words behind each"""
    lib, dt = L().lib(operands), L().act_dtype(operands)
    p, st = L().ptr, L().stream
    dl, xn, W = S.head_bwd_inputs(B, classes, D, dt)
    dW_full, dW = guarded(classes, D, torch.float32)
    db = sentinel((classes + GUARD,), torch.float32)
    dxn_full, dxn = guarded(B, D, dt)
    dl_d, xn_d, W_d = dl.to(DEV), xn.to(DEV), W.to(DEV)
    L().check(lib.cara_head_backward(p(dl_d), p(xn_d), p(W_d), p(dW_full), p(db), p(dxn_full), B, classes, D, st()),
              "head bwd")
    o = K.head_bwd(dl, xn, W)
    print(f"\nhead bwd {operands} {B} {classes} {D}")
    S.check_32("dW", dW, o["dW"])
    S.check_32("db", db[:classes], o["db"])
    S.check_16("dxn", dxn, o["dxn"], dt, T.SMALL_CAPS["head_dxn"])
    assert is_sentinel(dW_full[classes:]) and is_sentinel(db[classes:]) and is_sentinel(dxn_full[B:])


# ----------------------------------------------------------------------------------------------------------------------------
def _xent(lib, logits, labels, B, Cn, dl=True, scaled=False):
    p, st = L().ptr, L().stream
    loss = sentinel((1 + B + 1,), torch.float32)
    d = sentinel((B + 1, Cn), torch.float32) if dl else None
    if scaled:
        amp, found = torch.tensor([512.0, 0.0, 0.0, 0.0], device=DEV), torch.ones(1, device=DEV)
        L().check(lib.cara_cross_entropy_ex(p(logits), p(labels), p(loss), p(d), B, Cn, C.c_float(0.25), p(amp), p(found), st()), "xent ex")
        assert found.item() == 0.0
    else:
        L().check(lib.cara_cross_entropy(p(logits), p(labels), p(loss), p(d), B, Cn, st()), "xent")
    torch.cuda.synchronize()
    assert is_sentinel(loss[1 + B:]) and (d is None or is_sentinel(d[B:]))
    return loss[:1 + B], None if d is None else d[:B]


@pytest.mark.parametrize("operands", OPERANDS)
def test_cross_entropy_edges(operands):
    lib = L().lib(operands)
    for Cn in S.XENT_C:
        for B in S.XENT_B:
            lh, yh = S.xent_inputs(B, Cn)
            logits, labels = lh.to(DEV), yh.to(DEV)
            for scaled in (False, True):
                print(f"\nxent {operands} B={B} C={Cn} scaled={scaled}")
                loss, d = _xent(lib, logits, labels, B, Cn, scaled=scaled)
                xe = K.xent(lh, yh, *((0.25, 512.0) if scaled else (1.0, 1.0)))
                S.check_32("terms", loss[1:], xe["terms"])
                S.check_32("loss", loss[0], xe["loss"])
                S.check_32("dlogits", d, xe["dlogits"])
                loss2, _ = _xent(lib, logits, labels, B, Cn, dl=False, scaled=scaled)
                assert torch.equal(loss, loss2)


@pytest.mark.parametrize("Cn", [2, 65, 1000])
@pytest.mark.parametrize("operands", OPERANDS)
def test_cross_entropy_label_outside_the_classes(operands, Cn):
    """A label of -1 (sample 1) and of C (sample 3, B = 5): those samples' loss terms and dlogits rows are NaN and so is the loss;
    every other sample's term and gradient row is bitwise what valid labels give.  The logits are a view with a whole row of
    margin on either side, so that no version of the kernel can read outside the allocation here."""
    lib, B = L().lib(operands), 5
    lh, yh = S.xent_inputs(B, Cn)
    big = torch.zeros(B + 2, Cn, device=DEV)
    big[1:B + 1] = lh.to(DEV)
    logits = big[1:B + 1]
    loss, d = _xent(lib, logits, yh.to(DEV), B, Cn)
    bad = yh.clone()
    bad[1], bad[3] = -1, Cn
    loss_b, d_b = _xent(lib, logits, bad.to(DEV), B, Cn)
    good = [0, 2, 4]
    assert torch.isnan(loss_b[0]) and torch.isnan(loss_b[1 + 1]) and torch.isnan(loss_b[1 + 3])
    assert torch.isnan(d_b[1]).all() and torch.isnan(d_b[3]).all()
    assert torch.equal(loss_b[1:][good], loss[1:][good]) and torch.equal(d_b[good], d[good])
    loss_c, _ = _xent(lib, logits, bad.to(DEV), B, Cn, dl=False)
    assert torch.equal(loss_c[1:][good], loss[1:][good]) and torch.isnan(loss_c[[0, 2, 4]]).all()


# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 9), (63, 65), (64, 64), (65, 63), (130, 200)])
@pytest.mark.parametrize("operands", OPERANDS)
def test_transposes(operands, rows, cols):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    p, st = L().ptr, L().stream
    lds, ldd = (cols + 7) // 8 * 8 + 8, (rows + 7) // 8 * 8 + 16
    src = torch.randn(rows, lds, generator=torch.Generator().manual_seed(rows + cols)).to(dt).to(DEV)
    dst = sentinel((cols + 1, ldd), dt)
    L().check(lib.cara_transpose_bf16_ld(p(src), C.c_long(lds), p(dst), C.c_long(ldd), rows, cols, st()), "transpose ld")
    assert torch.equal(dst[:cols, :rows], src[:, :cols].t()) and is_sentinel(dst[:cols, rows:]) and is_sentinel(dst[cols:])
    for bad_lds, bad_ldd in ((lds + 4, ldd), (lds, ldd + 4), (cols - 1 if cols > 8 else 0, ldd), (lds, (rows - 1) // 8 * 8)):
        assert lib.cara_transpose_bf16_ld(p(src), C.c_long(bad_lds), p(dst), C.c_long(bad_ldd), rows, cols, st()) != 0
    s2 = src[:, :cols].contiguous()
    d2 = sentinel((cols + 1, rows), dt)
    L().check(lib.cara_transpose_bf16(p(s2), p(d2), rows, cols, st()), "transpose")
    assert torch.equal(d2[:cols], s2.t()) and is_sentinel(d2[cols:])


@pytest.mark.parametrize("operands", OPERANDS)
def test_f32_to_16_bit(operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    p, st = L().ptr, L().stream
    for n in (1, 3, 4, 5, 1023, 1025):
        f = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)
        o = sentinel((n + 1,), dt)
        L().check(lib.cara_f32_to_bf16(p(f), p(o), C.c_size_t(n), st()), "cvt")
        assert torch.equal(o[:n], f.to(dt)) and is_sentinel(o[n:])


# ----------------------------------------------------------------------------------------------------------------------------
def _adamw_launch(lib, tensors, step, dyn, skip=None, ntensors=None):
    a, h = L().AdamWArgs(), S.ADAMW_HYPER
    for j, (p_, g_, m_, v_, n) in enumerate(tensors[:L().ADAMW_MAX_TENSORS]):
        a.t[j] = L().AdamWTensor(p_.data_ptr(), g_.data_ptr(), m_.data_ptr(), v_.data_ptr(), n, 0)
    a.ntensors, a.step = len(tensors) if ntensors is None else ntensors, step
    a.lr[0], a.weight_decay[0] = h["lr"], h["wd"]
    a.one_minus_beta1, a.beta2, a.one_minus_beta2, a.eps = 1.0 - h["beta1"], h["beta2"], 1.0 - h["beta2"], h["eps"]
    a.bias_correction1, a.bias_correction2_sqrt = 1.0 - h["beta1"] ** step, math.sqrt(1.0 - h["beta2"] ** step)
    a.skip_flag = skip.data_ptr() if skip is not None else None
    keep = torch.tensor([float(step), h["lr"], 0.0, 0.0, 0.0], device=DEV) if dyn else None
    a.dyn = keep.data_ptr() if dyn else None
    rc = lib.cara_adamw_step(C.byref(a), L().stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dyn", [False, True], ids=["host", "dyn"])
@pytest.mark.parametrize("step", S.ADAMW_STEPS)
@pytest.mark.parametrize("operands", OPERANDS)
def test_adamw_to_its_restatement(operands, step, dyn):
    """32 tensors (CARA_ADAMW_MAX_TENSORS) of 1 .. 1025 elements in one launch, a guard word behind each array; 33 are refused; with
    the skip word set nothing moves"""
    lib = L().lib(operands)
    host, dev = [], []
    for j in range(L().ADAMW_MAX_TENSORS):
        n = S.ADAMW_SIZES[j % len(S.ADAMW_SIZES)]
        hs = S.adamw_inputs(n, step, seed=j)
        ds = []
        for t in hs:
            full = sentinel((n + 1,), torch.float32)
            full[:n] = t.to(DEV)
            ds.append(full)
        host.append(hs)
        dev.append((*ds, n))
    before = [[t.clone() for t in d[:4]] for d in dev]
    skip = torch.ones(1, device=DEV)
    assert _adamw_launch(lib, dev, step, dyn, skip=skip) == 0
    assert all(torch.equal(a, b) for d, bf in zip(dev, before) for a, b in zip(d[:4], bf))
    assert _adamw_launch(lib, dev, step, dyn, ntensors=L().ADAMW_MAX_TENSORS + 1) != 0
    assert _adamw_launch(lib, dev, step, dyn, skip=skip.zero_()) == 0
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for (p_, g_, m_, v_), (dp, dg, dm, dv, n) in zip(host, dev):
        o = K.adamw(p_, g_, m_, v_, step=step, dyn=dyn, **S.ADAMW_HYPER)
        for name, t in (("p", dp), ("m", dm), ("v", dv)):
            ok, ratio = K.hold_f32(t[:n], *o[name])
            worst[name] = max(worst[name], ratio)
            assert ok.all(), f"{name} of a tensor of {n}: worst ratio {ratio:.3f}"
            assert is_sentinel(t[n:])
        assert torch.equal(dg[:n].cpu(), g_) and is_sentinel(dg[n:])
    print(f"\nadamw {operands} step={step} dyn={dyn}: worst/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
