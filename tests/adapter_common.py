"""Cases, input families, the fp32 other-order restatement with its slips and the check helpers shared by
tests/test_adapter_model.py (host) and tests/test_adapter_contract_gpu.py (device).  The float64 restatement and its derived terms:
oracle/adapter_model.py; the cap on neighbour cases: tests/tolerances.py (ADAPTER_CAPS)."""
import numpy as np
import torch

from oracle import adapter_model as A
from tests import tolerances as T
from tests.gemm_common import check_16

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
S = 0.3
# (depth, dim, heads, rank, Rp, order): each chosen for the edge named
GEOMS = [
    (1, 8, 1, 1, 32, 4),        # one row per split piece; three of the four layer groups empty; n1 = 4 dim
    (3, 64, 16, 3, 32, 4),      # heads > hd (hd 4); rank < 4; depth % 4 != 0
    (5, 40, 5, 17, 32, 5),      # order 5; half-filled 32-lane group; five rows per piece; dim not a multiple of 64
    (2, 192, 3, 33, 64, 3),     # order 3; second rb pass with one live lane; Rr = 64 in stage 2
    (12, 256, 4, 16, 64, 4),    # rank 16 inside Rp 64 (48 padding columns); nine (layer, slot) pairs per lane group
    (2, 1024, 16, 64, 64, 5),   # ViT-L's dim and heads; rank = Rp; 20 nb_a blocks
    (24, 64, 1, 8, 32, 4),      # depth 24; one head (hd = dim)
    (7, 128, 2, 32, 32, 2),     # order 2
]
EX_GEOMS = [GEOMS[1], GEOMS[2], GEOMS[3], GEOMS[7]]   # one small geometry per order for the _ex entry
OLD_GEOM = (12, 768, 12, 16, 32, 4)                   # the one geometry of tests/test_kernels_gpu.py::test_factor_prep_and_grad_reduce
FAMILIES = ["gaussian", "pow2", "cancel"]
_SCALE = {"A1": 0.7, "A2": 1.3, "A3": 0.9, "A4": 1.7, "A5": 0.6, "P1": 1.1, "P2": 0.8, "P3": 1.5}


def gid(geom):
    return "L%d_d%d_h%d_r%d_Rp%d_o%d" % geom


def cp_shapes(geom):
    L, dim, H, R, Rp, order = geom
    hd = dim // H
    a = {5: {"A1": (L, R), "A2": (3, R), "A3": (dim, R), "A4": (H, R), "A5": (hd, R)},
         4: {"A1": (3 * L, R), "A2": (dim, R), "A3": (H, R), "A4": (hd, R)},
         3: {"A1": (3 * L, R), "A2": (dim, R), "A3": (dim, R)},
         2: {"A1": (3 * L, R), "A2": (dim * dim, R)}}[order]
    a.update({"P1": (9 * L, R), "P2": (dim, R), "P3": (dim, R), "R1": (R,), "R2": (R,), "bias1": (dim,), "bias2": (4 * dim,), "bias3": (dim,)})
    return a


def draw_cp(geom, early=False, seed=0):
    """Every factor non-zero (|x| >= a quarter of its scale), each tensor at a scale of its own (a swapped factor shows), R1 about
    1.5 and R2 about 0.6 (away from 1).  early: the zero-initialised factor (A2; A3 at order 5) and P2 at 1e-6 -- the first steps of
    training, where in the fp16 build the pack's products are half-precision subnormals."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * geom[0] + 7 * geom[1] + geom[3] + geom[5])
    cp = {}
    for name, shape in cp_shapes(geom).items():
        x = torch.randn(*shape, generator=g)
        if name in _SCALE:
            x = torch.sign(x + (x == 0)) * (0.25 + x.abs()) * _SCALE[name]
        elif name == "R1":
            x = 1.5 + 0.1 * x
        elif name == "R2":
            x = 0.6 + 0.05 * x
        else:
            x = 0.2 * x
        cp[name] = x.float()
    if early:
        for name in (A.zero_init_factor(geom[5]), "P2"):
            cp[name] = cp[name] * 1e-6
    return cp


def draw_bias(geom, seed=0):
    L, dim = geom[0], geom[1]
    g = torch.Generator().manual_seed(77 + seed + L + dim)
    return [torch.randn(L, n, generator=g) for n in (dim, 4 * dim, dim)]


def lg_shapes(geom):
    L, dim, H, R, Rp, order = geom
    rows = {"dU_qkv": dim, "dVs_qkv": 3 * dim, "dU_proj": dim, "dVs_proj": dim, "dU_fc1": dim, "dVs_fc1": 4 * dim, "dU_fc2": 4 * dim,
            "dVs_fc2": dim, "dc_proj": dim, "dc_fc1": 4 * dim, "dc_fc2": dim}
    return {k: (L, n) if k.startswith("dc") else (L, n, Rp) for k, n in rows.items()}


def draw_lg(geom, family, seed=0, nan_pad=True):
    """The per-layer gradients.  gaussian: O(1).  pow2: layer l times 2^k, k from -10 to 10 over the layers (every addition over
    layers rounds).  cancel: layers in pairs of opposite sign, (1 + 2^-10 n) apart (the sums over layers are small against the sums
    of absolute terms); an unpaired last layer is Gaussian at 2^-6.  The padding columns rank .. Rp of every dU / dVs are NaN."""
    L, R = geom[0], geom[3]
    g = torch.Generator().manual_seed(5000 + 100 * seed + FAMILIES.index(family) + 13 * L + geom[1])
    lg = {}
    for name, shape in lg_shapes(geom).items():
        x = torch.randn(*shape, generator=g)
        if family == "pow2" and L > 1:
            k = torch.round(-10 + 20 * torch.arange(L) / (L - 1))
            x = x * (2.0 ** k).reshape(L, *([1] * (x.dim() - 1)))
        elif family == "cancel":
            for l in range(1, L, 2):
                x[l] = -x[l - 1] * (1 + 2.0 ** -10 * torch.randn(*shape[1:], generator=g))
            if L % 2 and L > 1:
                x[L - 1] *= 2.0 ** -6
        if x.dim() == 3 and nan_pad:
            x[..., R:] = float("nan")
        lg[name] = x.float().contiguous()
    return lg


# --- fp32 in another order --------------------------------------------------------------------------------------------------
def osum(x, axis, pieces):
    """fp32 sum over `axis`: `pieces` contiguous runs (halved until they divide the length) added last to first, then adjacent runs
    pair up -- none of the kernels' partial sums"""
    x = np.moveaxis(x, axis, -1)
    n = x.shape[-1]
    p = pieces
    while n % p:
        p //= 2
    x = x.reshape(x.shape[:-1] + (p, n // p))
    acc = x[..., -1].copy()
    for j in range(n // p - 2, -1, -1):
        acc = acc + x[..., j]
    while acc.shape[-1] > 1:
        if acc.shape[-1] % 2:
            acc = np.concatenate((acc, np.zeros_like(acc[..., :1])), -1)
        acc = acc[..., 0::2] + acc[..., 1::2]
    assert acc.dtype == np.float32
    return acc[..., 0]


SLIPS = ["groups_drop_remainder", "split_piece_left_out", "rb_first_pass_only", "heads_hd_exchanged", "fc2_row_off_by_one", "r2_on_fc2_rows",
         "s_missing_from_zv", "o5_dA2_without_R1", "o5_dA1_wrong_k", "o3_dA3_without_A1", "loss_scale_not_on_R", "padding_column_read",
         "transpose_of_wrong_matrix"]


def slip_applies(geom, slip):
    L, dim, H, R, Rp, order = geom
    return {"groups_drop_remainder": L % 4 != 0, "rb_first_pass_only": R > 32, "heads_hd_exchanged": order in (4, 5) and 1 < H < dim,
            "o5_dA2_without_R1": order == 5, "o5_dA1_wrong_k": order == 5, "o3_dA3_without_A1": order == 3,
            "padding_column_read": R < Rp}.get(slip, True)


def _np(d):
    return {k: v.numpy().astype(np.float32) for k, v in d.items()}


def _out_index(geom, slip):
    """(head, head-dim index) of output column o: o = head hd + d"""
    dim, H = geom[1], geom[2]
    hd = dim // H
    o = np.arange(dim)
    return (o % H, o // H) if slip == "heads_hd_exchanged" else (o // hd, o % hd)


def _qkv_factors(geom, c, slip):
    """-> coef [L, 3, R], in factor [dim, R], out factor [dim, R], and for orders 4 / 5 (head factor, head-dim factor, names)"""
    L, dim, H, R, Rp, order = geom
    if order == 5:
        coef, fin, Fh, Fd, names = c["A1"][:, None, :] * c["A2"][None], c["A3"], c["A4"], c["A5"], ("A4", "A5")
    else:
        coef, fin = c["A1"].reshape(L, 3, R), c["A2"]
        Fh, Fd, names = (c["A3"], c["A4"], ("A3", "A4")) if order == 4 else (None, None, None)
    if order == 3:
        return coef, fin, c["A3"], None
    hh, d = _out_index(geom, slip)
    return coef, fin, Fh[hh] * Fd[d], (Fh, Fd, names, hh, d)


def restate_prep(cp, bias, geom, dt, slip=None, s=S):
    """cara_factor_prep in fp32 numpy with the products associated the other way round (out factor first, s last), rounded to the
    operand type -> {matrix: [depth, rows, Rp], matrix + "_t": [depth, Rp, rows], bias_*: [depth, n] fp32}"""
    L, dim, H, R, Rp, order = geom
    c = _np(cp)
    s = np.float32(s)
    P1 = c["P1"].reshape(L, 9, R)
    m = {}
    if order == 2:
        m["U_qkv"], m["Vs_qkv"] = np.zeros((L, dim, R), np.float32), np.zeros((L, 3 * dim, R), np.float32)
    else:
        coef, fin, fout, _ = _qkv_factors(geom, c, slip)
        m["U_qkv"] = np.broadcast_to(fin, (L, dim, R))
        m["Vs_qkv"] = (((fout[None, None] * coef[:, :, None, :]) * c["R1"]) * s).reshape(L, 3 * dim, R)
    off = 4 if slip == "fc2_row_off_by_one" else 5
    m["U_proj"] = m["U_fc1"] = np.broadcast_to(c["P3"], (L, dim, R))
    m["Vs_proj"] = ((c["P2"][None] * P1[:, 0, None, :]) * c["R2"]) * s
    m["Vs_fc1"] = (((c["P2"][None, None] * P1[:, 1:5, None, :]) * c["R2"]) * s).reshape(L, 4 * dim, R)
    m["U_fc2"] = (c["P2"][None, None] * P1[:, off:off + 4, None, :]).reshape(L, 4 * dim, R)
    m["Vs_fc2"] = np.broadcast_to((c["P3"] * c["R2"]) * s, (L, dim, R))
    out = {}
    for name, v in m.items():
        assert v.dtype == np.float32
        pad = torch.zeros(L, v.shape[1], Rp)
        pad[..., :R] = torch.from_numpy(np.array(v))
        out[name] = pad.to(dt)
    for name in A.MATS:
        src = "Vs_fc2" if (slip == "transpose_of_wrong_matrix" and name == "Vs_proj") else name
        out[name + "_t"] = out[src].transpose(1, 2).contiguous()
    for name, b, cb in (("bias_proj", bias[0], "bias1"), ("bias_fc1", bias[1], "bias2"), ("bias_fc2", bias[2], "bias3")):
        out[name] = torch.from_numpy(c[cb][None] * s + b.numpy())
    return out


def restate_grad(cp, lg, geom, slip=None, loss_scale=None, s=S):
    """cara_factor_grad_reduce(_ex) in fp32 numpy, another order: sums over layers and over rows are osum's (last to first, runs
    paired), the head / head-dim factors sum over layers BEFORE the rows, the final factors multiply the finished sums, s is applied
    after the row sums -> {name: fp32 tensor} for the tensors the order writes."""
    L, dim, H, R, Rp, order = geom
    hd = dim // H
    c, w = _np(cp), _np(lg)
    s = np.float32(s)
    for k in list(w):
        if w[k].ndim == 3:
            v = w[k][..., :R].copy()
            if slip == "padding_column_read" and R < Rp:
                v[..., R - 1] = w[k][..., R]
            w[k] = v
    nl = 4 * (L // 4) if slip == "groups_drop_remainder" else L
    lsum = lambda x: osum(x[:nl], 0, 2) if nl else np.zeros(x.shape[1:], np.float32)   # noqa: E731

    def rsum(x):   # over the rows (axis -2)
        if slip == "split_piece_left_out":
            x = x.copy()
            x[..., dim * 5 // 8:dim * 6 // 8, :] = 0
        z = osum(x, -2, 16)
        if slip == "rb_first_pass_only":
            z[..., (16 if R <= 16 else 32):] = 0
        return z
    P1 = c["P1"].reshape(L, 9, R)
    sr2 = c["R2"] * s
    out = {}
    Zp = rsum(w["dVs_proj"] * c["P2"]) * s                                          # [L, R]
    Zf1 = rsum(w["dVs_fc1"].reshape(L, 4, dim, R) * c["P2"]) * s                    # [L, 4, R]
    Zf2 = rsum(w["dU_fc2"].reshape(L, 4, dim, R) * c["P2"])
    zv = rsum(w["dVs_fc2"] * c["P3"])
    dP1 = np.empty((L, 9, R), np.float32)
    dP1[:, 0], dP1[:, 1:5] = Zp * c["R2"], Zf1 * c["R2"]
    dP1[:, 5:9] = Zf2 * c["R2"] if slip == "r2_on_fc2_rows" else Zf2
    out["P1"] = dP1.reshape(9 * L, R)
    terms = np.concatenate(((P1[:, 0] * Zp)[:, None], P1[:, 1:5] * Zf1), 1).reshape(5 * L, R)
    zvs = osum(zv, 0, 2)
    out["R2"] = osum(terms, 0, 4) + (zvs if slip == "s_missing_from_zv" else zvs * s)
    off = 4 if slip == "fc2_row_off_by_one" else 5
    out["P3"] = (lsum(w["dU_proj"]) + lsum(w["dU_fc1"])) + lsum(w["dVs_fc2"]) * sr2
    p2 = lsum(w["dVs_proj"] * P1[:, 0, None, :])
    for a in range(4):
        p2 = p2 + lsum(w["dVs_fc1"].reshape(L, 4, dim, R)[:, a] * P1[:, 1 + a, None, :])
    p2 = p2 * sr2
    for a in range(3, -1, -1):
        p2 = p2 + lsum(w["dU_fc2"].reshape(L, 4, dim, R)[:, a] * P1[:, off + a, None, :])
    out["P2"] = p2
    out["bias1"], out["bias2"], out["bias3"] = lsum(w["dc_proj"]) * s, lsum(w["dc_fc1"]) * s, lsum(w["dc_fc2"]) * s
    if order == 2:
        out["R1"] = np.zeros(R, np.float32)
    else:
        coef, fin, fout, heads = _qkv_factors(geom, c, slip)
        Wq = w["dVs_qkv"].reshape(L, 3, dim, R)
        out[A.zero_init_factor(order)] = lsum(w["dU_qkv"])
        Zq = rsum(Wq * fout) * s                                                    # [L, 3, R]
        if order == 5:
            k_of = [1, 2, 0] if slip == "o5_dA1_wrong_k" else [0, 1, 2]
            a1 = osum(Zq * c["A2"][k_of][None], 1, 1)
            out["A1"] = a1 * c["R1"]
            dk = osum(Zq * c["A1"][:, None, :], 0, 2)
            out["A2"] = dk if slip == "o5_dA2_without_R1" else dk * c["R1"]
            out["R1"] = osum((Zq * coef).reshape(3 * L, R), 0, 4)
        else:
            out["A1"] = (Zq * c["R1"]).reshape(3 * L, R)
            out["R1"] = osum((Zq * coef).reshape(3 * L, R), 0, 4)
        sr1 = c["R1"] * s
        if order == 3:
            t = Wq if slip == "o3_dA3_without_A1" else Wq * coef[:, :, None, :]
            out["A3"] = lsum(osum(t, 1, 1)) * sr1
        else:
            Fh, Fd, names, hh, d = heads
            Gq = osum((Wq * coef[:, :, None, :]).reshape(3 * L, dim, R), 0, 4)      # [dim, R]: layers and projections first
            by_head = np.argsort(hh * hd + d, kind="stable")
            by_d = np.argsort(d * H + hh, kind="stable")
            out[names[0]] = osum((Gq * Fd[d])[by_head].reshape(H, hd, R), 1, 4) * sr1
            out[names[1]] = osum((Gq * Fh[hh])[by_d].reshape(hd, H, R), 1, 4) * sr1
    if loss_scale is not None:
        gs = np.float32(1.0) / np.float32(loss_scale)
        for k in out:
            if not (slip == "loss_scale_not_on_R" and k in ("R1", "R2")):
                out[k] = out[k] * gs
    for k, v in out.items():
        assert v.dtype == np.float32, k
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


# --- the rules ----------------------------------------------------------------------------------------------------------------
def pad16(v, Rp, dt):
    """[.., rank] float64 -> round16 into [.., Rp] with zero padding"""
    out = torch.zeros(*v.shape[:-1], Rp, dtype=dt)
    out[..., :v.shape[-1]] = A.round16(v, dt)
    return out


def holds_prep(geom, model, got, dt, quiet=True):
    """every pack entry of `got` (restate_prep's layout) under its rule -> {name: (ok, worst / bound, neighbour share or None)}.
    Copies and the zero matrices: bitwise round16(v).  Products: hold_16 and the cap (all layers of a matrix are one tensor).
    Padding columns exactly +0 in both copies; each transposed copy bitwise the transpose; biases hold_f32."""
    L, dim, H, R, Rp, order = geom
    mats, bias = model
    nm = A.prep_muls(order)
    res = {}
    for name in A.MATS:
        v, d = mats[name]
        g = got[name]
        pad_ok = bool((g[..., R:].contiguous().view(torch.int16) == 0).all())
        tr_ok = bool(torch.equal(got[name + "_t"].view(torch.int16), g.transpose(1, 2).contiguous().view(torch.int16)))
        if nm[name] == 0:
            same = torch.equal(g[..., :R].contiguous().view(torch.int16), A.round16(v, dt).contiguous().view(torch.int16))
            res[name] = (same and pad_ok and tr_ok, 0.0, None)
        else:
            ok, ratio, used = check_16(name, g[..., :R], (v, d + A.TINY), dt, T.ADAPTER_CAPS["pack"], quiet=quiet)
            res[name] = (ok and pad_ok and tr_ok, ratio, used)
    for name, (v, d) in bias.items():
        ok, ratio = A.hold_f32(got[name], v, d)
        res[name] = (bool(ok.all()), ratio, None)
    return res


def holds_grad(model, got):
    """hold_f32 on every element of every tensor the order writes -> {name: (ok, worst / bound)}; a tensor missing from `got` fails"""
    res = {}
    for name, (v, d) in model.items():
        if name not in got:
            res[name] = (False, float("inf"))
            continue
        ok, ratio = A.hold_f32(got[name], v, d)
        res[name] = (bool(ok.all()), ratio)
    return res


def old_bar_fails(got, ref):
    """the bar of tests/test_kernels_gpu.py::test_factor_prep_and_grad_reduce on one gradient: 1e-4 |ref| + 1e-4 max |ref| -> True if
    `got` FAILS it"""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    return not bool((err <= 1e-4 * max(float(ref.abs().max()), 1e-6) + 1e-4 * ref.abs()).all())
