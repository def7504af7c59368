"""Plain float64 restatement of the adapter-side kernels of cara_amd/csrc/factors.hip -- cara_factor_prep (the shared CP tensors
turned into per-layer operands) and cara_factor_grad_reduce(_ex) (the per-layer gradients scattered back onto them,
A.4) -- with a per-element term DERIVED from each kernel's arithmetic, in the convention of oracle/small_kernels.py and
oracle/gemm_model.py (whose U, gamma, f64, round16, hold_f32 and hold_16 are used as they are).

The restatements are written from the mathematics: the factor table is oracle.cara_oracle.build_factored's, stated for all layers
at once, and the gradients are float64 autograd of  sum (U . dU) + sum (Vs . dVs) + sum (c . dc)  through that table -- no loop of
the kernels is transcribed.  The derived term of an fp32 output that is a sum of products is

    d = gamma(kappa) x (the same contraction evaluated on ABSOLUTE values) + 2^-149,

kappa the longest chain of roundings on a path into one output element, counted from the code with every product taken as rounded
(a contracted fma only removes roundings).  Every monomial of these gradients has coefficient +1 and s > 0, so the contraction on
absolute values is the same autograd evaluated at |cp|, |dU|, |dVs|, |dc|.  Nothing here is fitted to a device:
tests/test_adapter_model.py proves on the host that an fp32 restatement in another order stays inside every bound and that the
slips of tests/adapter_common.py do not; tests/test_adapter_contract_gpu.py then holds the device to it.

A geometry is (depth, dim, heads, rank, Rp, order); CP tensors are a dict A1 .. A5, P1, P2, P3, R1, R2, bias1 .. bias3 (the members
of cara_cp), layer gradients a dict with the members of cara_layer_grads, each [depth, rows, Rp] (dc_*: [depth, rows]).
"""
import torch

from oracle.small_kernels import U, gamma, f64, round16, hold_f32, hold_16   # noqa: F401  (re-exported: the two rules)

TINY = 2.0 ** -149
GS_SPLIT = 8          # factors.hip: pieces of a column reduction's rows
ROW_GROUPS = 4        # grad_rowwise: layer groups of a block
MATS = ("U_qkv", "Vs_qkv", "U_proj", "Vs_proj", "U_fc1", "Vs_fc1", "U_fc2", "Vs_fc2")   # pack order (M_U_QKV .. M_VS_FC2)
LG_FIELDS = ("dU_qkv", "dVs_qkv", "dU_proj", "dVs_proj", "dU_fc1", "dVs_fc1", "dU_fc2", "dVs_fc2", "dc_proj", "dc_fc1", "dc_fc2")


def mat_rows(name, dim):
    return {"Vs_qkv": 3 * dim, "Vs_fc1": 4 * dim, "U_fc2": 4 * dim}.get(name, dim)


def cp_names(order):
    """the CP tensors an order has (cara_amd._lib.cp_fields)"""
    a = {2: ("A1", "A2"), 3: ("A1", "A2", "A3"), 4: ("A1", "A2", "A3", "A4"), 5: ("A1", "A2", "A3", "A4", "A5")}[order]
    return a + ("P1", "P2", "P3", "R1", "R2", "bias1", "bias2", "bias3")


def zero_init_factor(order):
    """the factor the reference initialises to zero (the in factor of the QKV adapter): A3 at order 5, else A2"""
    return "A3" if order == 5 else "A2"


def khatri_rao(a, b):
    """row i J + j = a[i] (.) b[j]"""
    return (a[:, None, :] * b[None, :, :]).reshape(-1, a.shape[1])


def s32(s):
    """the scale as the kernels receive it: cara_geom::scale is a float, so the s of the mathematics is that fp32 number"""
    return float(torch.tensor(float(s), dtype=torch.float32))


def factor_table(cp, geom, s):
    """The A.3 table for all layers at once, in the dtype of cp (float64 here; differentiable): name -> [depth, rows, rank].
        qkv:   U = in factor,  Vs[k dim + o] = s R1 coef(l, k) out(o);  order 4: coef = A1[3l + k], in = A2, out = A3 (x) A4 (heads x
               head dim); order 5: coef = A1[l] A2[k], in = A3, out = A4 (x) A5; order 3: coef = A1[3l + k], in = A2, out = A3;
               order 2: no factored QKV adapter (both matrices zero: dense_delta.hip carries it)
        proj:  U = P3,  Vs = s R2 P1[9l] P2             fc1:  U = P3,  Vs[a dim + j] = s R2 P1[9l + 1 + a] P2[j]
        fc2:   U[a dim + j] = P1[9l + 5 + a] P2[j],  Vs = s R2 P3"""
    L, dim, H, R, Rp, order = geom
    t = {}
    if order == 2:
        z = cp["P3"].new_zeros(())
        t["U_qkv"], t["Vs_qkv"] = z.expand(L, dim, R), z.expand(L, 3 * dim, R)
    else:
        if order == 5:
            coef, fin, fout = cp["A1"][:, None, :] * cp["A2"][None, :, :], cp["A3"], khatri_rao(cp["A4"], cp["A5"])
        elif order == 4:
            coef, fin, fout = cp["A1"].reshape(L, 3, R), cp["A2"], khatri_rao(cp["A3"], cp["A4"])
        else:
            coef, fin, fout = cp["A1"].reshape(L, 3, R), cp["A2"], cp["A3"]
        t["U_qkv"] = fin.expand(L, dim, R)
        t["Vs_qkv"] = (s * cp["R1"] * coef[:, :, None, :] * fout[None, None, :, :]).reshape(L, 3 * dim, R)
    P1 = cp["P1"].reshape(L, 9, R)
    g2 = s * cp["R2"]
    t["U_proj"] = t["U_fc1"] = cp["P3"].expand(L, dim, R)
    t["Vs_proj"] = g2 * P1[:, 0, None, :] * cp["P2"][None]
    t["Vs_fc1"] = (g2 * P1[:, 1:5, None, :] * cp["P2"][None, None]).reshape(L, 4 * dim, R)
    t["U_fc2"] = (P1[:, 5:9, None, :] * cp["P2"][None, None]).reshape(L, 4 * dim, R)
    t["Vs_fc2"] = (g2 * cp["P3"]).expand(L, dim, R)
    return t


def prep_muls(order):
    """Multiplications (each one rounding in fp32) behind one pack entry, counted from factor_value() of factors.hip:
        U_qkv, U_proj, U_fc1: `return qkv_in(...)` / `cp.P3[...]`: a copy, 0 -- the entry is round16 of the fp32 number, bitwise.
        Vs_qkv: `g.s * cp.R1[r] * qkv_coef(...) * qkv_out(...)`: three products, one more inside qkv_coef at order 5 (`A1 * A2`), one
            more inside qkv_out at orders 4 and 5 (head x head-dim factor): 3 (order 3), 4 (order 4), 5 (order 5).
        Vs_proj, Vs_fc1: `g.s * cp.R2[r] * cp.P1[...] * cp.P2[...]`: 3.     U_fc2: `cp.P1[...] * cp.P2[...]`: 1.
        Vs_fc2: `g.s * cp.R2[r] * cp.P3[...]`: 2."""
    return {"U_qkv": 0, "U_proj": 0, "U_fc1": 0, "Vs_qkv": {2: 0, 3: 3, 4: 4, 5: 5}[order], "Vs_proj": 3, "Vs_fc1": 3, "U_fc2": 1, "Vs_fc2": 2}


def factor_prep(cp, base_bias, geom, s):
    """cara_factor_prep -> ({matrix: (v, d)} with v [depth, rows, rank] float64 BEFORE the 16-bit rounding, {bias: (v, d)}).
    d = gamma(prep_muls) |v| (0 for a copy and for the zero matrices of order 2: bitwise round16(v)); the conversion `(bf16)f` is the
    one 16-bit rounding hold_16 performs.  Biases (prep_bias_kernel: `bp[...] + g.s * cp.bias1[e]`): the product and the sum one
    rounding each, against b + s c:  d = 2u (|b| + |s c|)."""
    c64 = {k: f64(v) for k, v in cp.items()}
    s = s32(s)
    tab = factor_table(c64, geom, s)
    nm = prep_muls(geom[5])
    mats = {k: (v, gamma(nm[k]) * v.abs() if nm[k] else torch.zeros_like(v)) for k, v in tab.items()}
    bias = {}
    for name, b, c in (("bias_proj", base_bias[0], c64["bias1"]), ("bias_fc1", base_bias[1], c64["bias2"]), ("bias_fc2", base_bias[2], c64["bias3"])):
        b = f64(b)
        sc = float(s) * c
        bias[name] = (b + sc, 2 * U * (b.abs() + sc.abs()) + TINY)
    return mats, bias


def _autograd(cp, lg, geom, s):
    L, dim, H, R, Rp, order = geom
    leaves = {k: v.clone().requires_grad_(True) for k, v in cp.items()}
    tab = factor_table(leaves, geom, s)
    tot = 0.0
    for name in MATS:
        if order == 2 and name.endswith("qkv"):
            continue
        tot = tot + (tab[name] * lg["d" + name][..., :R]).sum()
    for b, dc in (("bias1", "dc_proj"), ("bias2", "dc_fc1"), ("bias3", "dc_fc2")):
        tot = tot + (s * leaves[b][None] * lg[dc]).sum()
    tot.backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def kappa_grad(geom):
    """Roundings on the longest path into one element of each output of cara_factor_grad_reduce, counted from factors.hip.
    L = depth, lg = ceil(L / 4) (grad_rowwise: `l0 = L * grp / 4, l1 = L * (grp + 1) / 4`, the longest of the four layer groups).

    Row-wise outputs (grad_rowwise; `total()` adds the four groups as (g0 + g1) + (g2 + g3): 2):
        in factor (dA2; dA3 at order 5):  `a2 += dU_qkv[...]` lg, the tree 2:                                     lg + 2
        dP3:  `sr2 = g.s * R2` 1, `sr2 * dVs_fc2` 1, the sum inside the statement 1, `p3 +=` lg, the tree 2:      lg + 5
        dP2:  `sr2 * P1 * dVs` 3 products per term, nine `p2 +=` per layer, the tree 2:                           9 lg + 5
        dA3 at order 3:  `A1 * dVs_qkv` 1, three `a3o +=` per layer, the tree 2, `g.s * R1 * ta3` 2:              3 lg + 5
        bias grads:  `b +=` lg, the tree 2, `g.s * tb` 1:                                                         lg + 3
    Column reductions (grad_colred_part): a piece has at most rp = ceil(dim / 8) rows; Rr = 16 (rank <= 16) or 32 lanes of r and
    NP = 256 / Rr row partitions: `z += w * f` over ceil(rp / NP) rows, `s += red[p * Rr + r]` over NP partitions, and stage 2 adds
    the eight pieces (`z += zp[sp * R]`):  kz(m) = m + ceil(rp / NP) + NP + 8  with m the products of one term:
        slots 0 .. 2 (QKV): `f = g.s * qkv_out(...)` (1, and 1 inside qkv_out at orders 4 / 5), `w * f` 1:  m = 3 (order 3: 2)
        slots 3 .. 7 (proj, fc1): `f = g.s * P2`, `w * f`:  m = 2          slots 8 .. 11 (fc2's dU) and zv:  m = 1
    Stage 2, last block: Rr2 = 16 / 32 / 64 lanes, NG = 256 / Rr2 groups walk the 12 L (layer, slot) pairs, `s1 += red1[k * Rr + r]` NG:
        dA1 (orders 3, 4):  `R1 * z`:  kz(mq) + 1            dP1 rows 9l .. 9l + 4:  `R2 * z`:  kz(2) + 1;  rows 9l + 5 .. 8:  kz(1)
        dR1 (orders 3, 4):  `d1 += A1 * z` at most min(3 L, ceil(12 L / NG)) times in a group, then NG:  kz(mq) + 1 + that + NG
        dR2:  `d2 += P1 * z` at most min(5 L, ceil(12 L / NG)) times, `d2 += g.s * zv` 1, NG -- or through zv: a piece's
              1 + ceil(rp / NP) + NP, `zv += zvp` ceil(8 L / NG), `g.s * zv` 1, `d2 +=` 1, NG: the longer of the two
        order 5:  `a1 += A2[k] * z` 1 product and 3 additions;  dA1 = kz(3) + 4 + 1 (`R1 * a1`);
              dR1:  `d1 += A1 * a1` 1, ceil(L / NG) of them, NG:  kz(3) + 4 + 1 + ceil(L / NG) + NG
              dA2[k]:  `dk[k] += A1 * z` 1, ceil(L / NG), NG, `R1 * s3[k]` 1:  kz(3) + 2 + ceil(L / NG) + NG
    Head and head-dim factors (grad_a34_part, orders 4 and 5): `in += W * Fd` 1 product and hd additions (H for the head-dim factor),
        `qkv_coef * in` 1 (and 1 inside qkv_coef at order 5), stage 2 `acc += p[...]` 3 L, `g.s * R1 * acc` 2:  hd (or H) + 3 L + 4 (+ 1).
    Order 2: dR1 is written as zero (0), dA1 and dA2 are not written.
    -> {name: int, or for P1 a [9] list per row of a layer}"""
    L, dim, H, R, Rp, order = geom
    hd = dim // H
    ceil = lambda a, b: -(-a // b)   # noqa: E731
    lg = ceil(L, ROW_GROUPS)
    rp = ceil(dim, GS_SPLIT)
    Rr = 16 if R <= 16 else 32
    NP = 256 // Rr
    kz = lambda m: m + ceil(rp, NP) + NP + GS_SPLIT   # noqa: E731
    Rr2 = 16 if R <= 16 else (32 if R <= 32 else 64)
    NG = 256 // Rr2
    mq = 2 if order == 3 else 3
    k = {"P3": lg + 5, "P2": 9 * lg + 5, "bias1": lg + 3, "bias2": lg + 3, "bias3": lg + 3,
         "P1": [kz(2) + 1] * 5 + [kz(1)] * 4,
         "R2": max(kz(2) + 1 + min(5 * L, ceil(12 * L, NG)) + 1 + NG, 1 + ceil(rp, NP) + NP + ceil(GS_SPLIT * L, NG) + 2 + NG)}
    if order == 2:
        k["R1"] = 0
        return k
    k[zero_init_factor(order)] = lg + 2
    if order == 5:
        k["A1"] = kz(mq) + 5
        k["R1"] = kz(mq) + 5 + ceil(L, NG) + NG
        k["A2"] = kz(mq) + 2 + ceil(L, NG) + NG
        k["A4"], k["A5"] = hd + 3 * L + 5, H + 3 * L + 5
    else:
        k["A1"] = kz(mq) + 1
        k["R1"] = kz(mq) + 1 + min(3 * L, ceil(12 * L, NG)) + NG
        if order == 3:
            k["A3"] = 3 * lg + 5
        else:
            k["A3"], k["A4"] = hd + 3 * L + 4, H + 3 * L + 4
    return k


def factor_grad_reduce(cp, lg, geom, s, loss_scale=None):
    """cara_factor_grad_reduce(_ex) -> {name: (v, d)} for every tensor the order WRITES (order 2: no A1, A2; R1 is exactly zero).
    v: float64 autograd through factor_table of the layer gradients' columns r < rank (the padding is never read);
    d = gamma(kappa_grad) x (the same gradient at absolute values) + 2^-149.
    loss_scale (the _ex entry, gout_of / GOut of factors.hip: `gs = 1.f / *loss_scale`, `r = v * gs`): v / loss_scale; a power of
    two is exact (bitwise 2^-k times the plain result, asserted as such by the device test), any other value rounds the reciprocal
    and the product: d / loss_scale + 2u |v / loss_scale|."""
    L, dim, H, R, Rp, order = geom
    s = s32(s)
    c64 = {k: f64(v) for k, v in cp.items() if k in cp_names(order)}
    l64 = {k: f64(lg[k]) for k in LG_FIELDS}
    v = _autograd(c64, l64, geom, float(s))
    a = _autograd({k: t.abs() for k, t in c64.items()}, {k: t[..., :R].abs() if t.dim() == 3 else t.abs() for k, t in l64.items()}, geom, abs(float(s)))
    kap = kappa_grad(geom)
    out = {}
    for name, k in kap.items():
        if isinstance(k, list):
            g = torch.tensor([gamma(x) for x in k], dtype=torch.float64).repeat(L)[:, None]
        else:
            g = gamma(k)
        val, d = (v[name], g * a[name] + TINY) if not (order == 2 and name == "R1") else (torch.zeros_like(v[name]), torch.full_like(v[name], TINY))
        if loss_scale is not None:
            val = val / loss_scale
            d = d / loss_scale + 2 * U * val.abs() + TINY
        out[name] = (val, d)
    return out
