"""Host model of the mean-pooled readout (timm's ``global_pool="avg"`` with ``fc_norm``): ``head(fc_norm(x[:, 1:].mean(1)))``.

The oracle's ``vit_cara_forward`` ends in the cls readout.  ``forward`` below restates its loop from the oracle's public pieces and
takes ``readout="token" | "avg"``; with ``"token"`` it is the oracle's function bit for bit (tests/test_pool_model.py), so the only
thing that differs under ``"avg"`` is the tail.  Also here: the error bounds of the two pool kernels, derived from fp32 arithmetic
alone, an fp32 restatement of each kernel in ANOTHER summation order (the host check that the bounds are not fitted to one order),
the input families of the kernel tests, and a plain-torch pooled ViT assembled from the oracle's classes.

Not covered: the oracle's ``train`` / ``keep_masks`` arguments (weight-space dropout): the pooled readout runs the factored adapters only.
"""
import types

import torch
import torch.nn.functional as F

from oracle import cara_oracle as O

U32 = 2.0 ** -24          # unit roundoff of fp32


def forward(images, w, cp, *, s, depth=12, num_heads=12, patch=16, eps=1e-6, drop_path_keep=None, factored=False, bf16_sim=False,
            sim_dtype=None, sim_only=None, sim_skip=None, readout="token"):
    """``O.vit_cara_forward`` with a choice of readout.  ``"avg"``: ``w`` carries ``fc_norm.weight`` / ``fc_norm.bias`` and no
    ``norm.*``; no LayerNorm touches the tokens in front of the pool, and like the cls readout the tail is fp32 throughout."""
    if bf16_sim and sim_dtype is None:
        sim_dtype = torch.bfloat16
    r = O.make_rounder(sim_dtype, sim_only, sim_skip)
    B, dim = images.shape[0], w["cls_token"].shape[-1]
    scale = (dim // num_heads) ** -0.5
    gh = images.shape[2] // patch
    cols = images.reshape(B, images.shape[1], gh, patch, gh, patch).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gh, -1)
    x = r(cols, "images") @ r(w["patch_embed.proj.weight"].reshape(dim, -1), "weights").t() + w["patch_embed.proj.bias"]
    x = torch.cat((w["cls_token"].expand(B, -1, -1), x), dim=1) + w["pos_embed"]
    idxs = O.block_indices(depth)
    fac = O.build_factored(cp, s, depth=depth, heads=num_heads) if factored else None
    for l in range(depth):
        p = f"blocks.{l}."
        a_idx, a_aidx, m_idx = idxs[l]
        xn = r(F.layer_norm(x, (dim,), w[p + "norm1.weight"], w[p + "norm1.bias"], eps), "xn")
        if factored:
            y = O._attn_factored(xn, w, p, fac[l], num_heads, scale, r)
        else:
            y = O.attn_as_written(xn, cp, w[p + "attn.qkv.weight"], w[p + "attn.qkv.bias"], w[p + "attn.proj.weight"], w[p + "attn.proj.bias"],
                                  attn_idx=a_aidx, idx=a_idx, s=s, num_heads=num_heads, scale=scale, dp=None)
        if drop_path_keep is not None:
            y = y * drop_path_keep[l, 0].reshape(B, 1, 1)
        x = x + y
        xn = r(F.layer_norm(x, (dim,), w[p + "norm2.weight"], w[p + "norm2.bias"], eps), "xn")
        if factored:
            y = O._mlp_factored(xn, w, p, fac[l], r)
        else:
            y = O.mlp_as_written(xn, cp, w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"], w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"],
                                 idx=m_idx, s=s, dp=None)
        if drop_path_keep is not None:
            y = y * drop_path_keep[l, 1].reshape(B, 1, 1)
        x = x + y
    if readout == "token":
        xc = F.layer_norm(x[:, 0], (dim,), w["norm.weight"], w["norm.bias"], eps)
    elif readout == "avg":
        xc = F.layer_norm(x[:, 1:].mean(1), (dim,), w["fc_norm.weight"], w["fc_norm.bias"], eps)
    else:
        raise ValueError(readout)
    if sim_only is not None and "head" in sim_only:
        return F.linear(r(xc, "head"), r(w["head.weight"], "head"), w["head.bias"])
    return F.linear(xc, w["head.weight"], w["head.bias"])


def pooled_weights(w, seed=5):
    """the token-readout state dict ``w`` as a pooled model's: ``norm.*`` leave, ``fc_norm.*`` arrive with a non-trivial gamma / beta"""
    g = torch.Generator().manual_seed(seed)
    dim = w["cls_token"].shape[-1]
    out = {k: v for k, v in w.items() if not k.startswith("norm.")}
    out["fc_norm.weight"] = 1.0 + 0.3 * torch.randn(dim, generator=g)
    out["fc_norm.bias"] = 0.2 * torch.randn(dim, generator=g)
    return out


def plain_torch_pooled_vit(w, depth, img, num_classes):
    """The oracle's eager VisionTransformer (timm 0.4.12's) turned into timm's pooled model: ``norm`` an Identity, an ``fc_norm``, and
    ``forward_features`` = ``fc_norm(blocks(...)[:, 1:].mean(1))``; loaded from the pooled state dict ``w``."""
    m = O.create_vit("vit_base_patch16_224_in21k", depth=depth, img_size=img, num_classes=num_classes)
    m.norm = torch.nn.Identity()
    m.fc_norm = torch.nn.LayerNorm(m.embed_dim, eps=1e-6)

    def forward_features(self, x):
        x = self.patch_embed(x)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
        x = self.blocks(self.pos_drop(x + self.pos_embed))
        return self.fc_norm(x[:, 1:].mean(1))
    m.forward_features = types.MethodType(forward_features, m)
    missing, unexpected = m.load_state_dict(w, strict=True)
    assert not missing and not unexpected
    return m.eval()


# ---- the two kernels: inputs, bounds, other-order restatements -----------------------------------------------------------------------
FAMILIES = ("gauss", "offset", "outlier", "const", "zero")


def family(kind, B, tokens, D, seed=0):
    """x fp32 [B, tokens, D] of one input family (row 0 of every sample is the cls row: the tests overwrite it with NaN)"""
    g = torch.Generator().manual_seed(seed)
    if kind == "gauss":
        return torch.randn(B, tokens, D, generator=g)
    if kind == "offset":                       # mean 100, spread 1e-2: a sum that carries many more bits than its terms differ in
        return 100.0 + 1e-2 * torch.randn(B, tokens, D, generator=g)
    if kind == "outlier":                      # one token of |x| = 200 among unit Gaussians
        x = torch.randn(B, tokens, D, generator=g)
        t = 1 + int(torch.randint(0, max(tokens - 1, 1), (1,), generator=g)) if tokens > 1 else 0
        x[:, t] = 200.0 * torch.sign(torch.randn(B, D, generator=g))
        return x
    if kind == "const":
        return torch.full((B, tokens, D), 0.7310585975646973)
    if kind == "zero":
        return torch.zeros(B, tokens, D)
    raise ValueError(kind)


def mean_bound(x, first):
    """|out - mean64| <= (n + 2) 2^-24 sum|x_i| / n per element, n = tokens - first.  Any order of n - 1 fp32 additions is off by at
    most gamma(n - 1) sum|x_i| <= n u sum|x_i| (u = 2^-24, first order; the slack of two units covers the second-order terms up
    to n ~ 10^3), the scaling by 1 / n adds one rounding (a correctly rounded division) or two (a rounded reciprocal, then a
    product).  float64 [B, D]."""
    n = x.shape[1] - first
    return (n + 2) * U32 * x[:, first:].double().abs().sum(1) / n


def mean64(x, first):
    return x[:, first:].double().mean(1)


def token_mean_other_order(x, first):
    """fp32, in another order than the kernel's (which strides the tokens over eight groups, ascending): descending, one accumulator,
    then a product with the rounded reciprocal instead of a division"""
    n = x.shape[1] - first
    s = torch.zeros(x.shape[0], x.shape[2], dtype=torch.float32)
    for t in range(x.shape[1] - 1, first - 1, -1):
        s = s + x[:, t]
    return s * torch.tensor(1.0, dtype=torch.float32).div(n)


def bwd64(dpool, rowscale, tokens, first):
    """(dx, v) in float64: dx [B, tokens, D] with zero rows below ``first``; v = rowscale[b] * dx, what dyb rounds"""
    B, D = dpool.shape
    dx = torch.zeros(B, tokens, D, dtype=torch.float64)
    dx[:, first:] = (dpool.double() / (tokens - first)).unsqueeze(1)
    sc = torch.ones(B, dtype=torch.float64) if rowscale is None else rowscale.double()
    return dx, dx * sc.reshape(B, 1, 1)


def token_mean_bwd_other_order(dpool, rowscale, tokens, first, dtype):
    """fp32: dx = dpool / n; the 16-bit image from (dpool * rowscale) / n -- scale first, divide second, the other way round than the
    kernel (which scales dx).  -> (dx fp32 [B, tokens, D], dyb ``dtype`` [B, tokens, D])"""
    B, D = dpool.shape
    n = float(tokens - first)
    dx = torch.zeros(B, tokens, D, dtype=torch.float32)
    dx[:, first:] = (dpool / n).unsqueeze(1)
    sc = torch.ones(B) if rowscale is None else rowscale
    v = torch.zeros(B, tokens, D, dtype=torch.float32)
    v[:, first:] = ((dpool * sc.reshape(B, 1)) / n).unsqueeze(1)
    return dx, v.to(dtype)


def dx_ok(dx, dx64):
    """|dx - v64| <= 2 x 2^-24 |v64|: one rounding of a correctly rounded division, two of a reciprocal and a product"""
    return bool(((dx.double() - dx64).abs() <= 2 * U32 * dx64.abs()).all())


def dyb_ok(dyb, v64, dtype):
    """Each 16-bit element is the rounding of SOME value within 3 x 2^-24 |v| of the float64 value v (division, scaling, and the
    order of the two: three fp32 roundings at most).  Rounding is monotone, so that is the interval [rn(v - t), rn(v + t)];
    interval only -- the term is 2^12 times smaller than a 16-bit step, no share of neighbours is granted beyond it."""
    t = 3 * U32 * v64.abs()
    lo, hi = (v64 - t).to(dtype).double(), (v64 + t).to(dtype).double()
    d = dyb.double()
    return bool(((d >= lo) & (d <= hi)).all())


def to_panels(rowmajor, panels):
    """[rows, D] -> the K-panel-major image [D / 32, panels, 32] (rows beyond ``rows`` left NaN): cara_layernorm_bwd_ex's layout"""
    rows, D = rowmajor.shape
    out = torch.full((D // 32, panels, 32), float("nan"), dtype=rowmajor.dtype)
    out[:, :rows] = rowmajor.reshape(rows, D // 32, 32).permute(1, 0, 2)
    return out


def from_panels(img, rows):
    """the inverse: [D / 32, panels, 32] -> [rows, D]"""
    return img[:, :rows].permute(1, 0, 2).reshape(rows, -1)
