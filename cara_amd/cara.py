"""``cara(config)`` -- the reference's adapter-installation API on the MI355X-native path.

Mirrors ``/root/reference/src/cara/cara.py``:

* ``cara(config)`` (``cara.py:169-188``): same five dict keys (``model, rank, scale, l_mu, l_std``;
  a missing key raises ``KeyError`` exactly like the reference), returns the SAME module, mutated.
* ``set_cara`` (``cara.py:98-166``): same 12 top-level ``nn.Parameter`` names / shapes / inits /
  RNG consumption order, same index walk (``attn.idx = 9l``, ``attn.attn_idx = 3l``,
  ``mlp.idx = 9l+1``; ``model.idx == 108``, ``model.attn_idx == 36`` for depth 12), same child
  attributes ``dp, s, dim, idx, attn_idx`` and a rebound ``forward`` on every Attention / Mlp.

Differences, all deliberate:

* the arithmetic runs in libcara_hip.so (factored form) instead of
  ``tensorly.cp_to_tensor`` + a second dense GEMM; there is no CPU path;
* the shared factors are bound per model instance instead of through the module-level singleton
  ``global_model`` (``cara.py:12,185-186``), so several adapted models can live in one process
  (``global_model`` is still set, for scripts that read it);
* dims are taken from the model (ViT-B = the reference's hard-coded 768/12/12, ``cara.py:112-125``).
"""
from __future__ import annotations

import weakref
from typing import Any, Dict

import torch as th
import torch.nn as nn

from . import vit as _vit
from ._lib import CaraError

global_model: th.nn.Module = None  # kept for API compatibility with cara.py:12


def _owner(child):
    ref = child.__dict__.get("_cara_owner")
    model = ref() if ref is not None else None
    if model is None:
        raise CaraError("adapter owner model is gone")
    return model


def cp_attn(self, x: th.Tensor) -> th.Tensor:
    """Attention with CP parameters (counterpart of ``cara.py:15-60``), module-level entry."""
    return _owner(self)._cara_engine.attn_forward(self, x)


def cp_mlp(self, x: th.Tensor) -> th.Tensor:
    """Mlp with CP parameters (counterpart of ``cara.py:63-95``), module-level entry."""
    return _owner(self)._cara_engine.mlp_forward(self, x)


def _is(obj, *classes) -> bool:
    """Exact-type dispatch like cara.py:110,147,157 (subclasses are skipped), widened from "timm's class object" to
    "a class of that NAME with that structure": timm is not a dependency of this build, so its VisionTransformer /
    Attention / Mlp are recognised by what cp_attn / cp_mlp use of them (cara.py:25,37,44,46,50,59,75,84,85,87)."""
    for c in classes:
        if type(obj) is c:
            return True
        if type(obj).__name__ == c.__name__ and all(hasattr(obj, a) for a in _STRUCTURE[c.__name__]):
            return True
    return False


_STRUCTURE = {
    "VisionTransformer": ("patch_embed", "cls_token", "pos_embed", "blocks", "norm", "head", "embed_dim"),
    "Attention": ("qkv", "proj", "num_heads", "scale"),
    "Mlp": ("fc1", "act", "fc2"),
}


def pooled_readout(model) -> bool:
    """Is this the mean-pooled readout the fused path computes -- ``global_pool == "avg"``, ``norm`` an Identity and ``fc_norm`` an
    affine ``LayerNorm(embed_dim)``: ``head(fc_norm(x[:, 1:].mean(1)))``?  (Anything else with a pool or an fc_norm is refused by
    ``_check_vit``.)"""
    fc = getattr(model, "fc_norm", None)
    return getattr(model, "global_pool", "token") == "avg" and isinstance(getattr(model, "norm", None), nn.Identity) and \
        isinstance(fc, nn.LayerNorm) and fc.weight is not None and fc.bias is not None and \
        tuple(fc.normalized_shape) == (model.embed_dim,)


def _check_vit(model) -> None:
    """What the HIP path supports of a timm-shaped ViT (the reference's configuration, vit_cp.py:155): say so up
    front instead of computing something else."""
    def bad(msg):
        raise CaraError("cara_amd.cara(): unsupported ViT: " + msg)
    blocks = list(model.blocks)
    if not blocks:
        bad("no blocks")
    D = model.embed_dim
    if getattr(model, "dist_token", None) is not None:
        bad("distilled models (dist_token) are not supported")
    if not isinstance(getattr(model, "pre_logits", nn.Identity()), nn.Identity):
        bad("a pre_logits layer is not supported (vit_base_patch16_224_in21k of timm 0.4.12 has none)")
    pe = model.patch_embed.proj
    if not isinstance(pe, nn.Conv2d) or pe.kernel_size != pe.stride or pe.kernel_size[0] != pe.kernel_size[1]:
        bad("patch_embed.proj must be a square Conv2d with kernel == stride")
    for i, b in enumerate(blocks):
        for a in ("norm1", "attn", "norm2", "mlp"):
            if not hasattr(b, a):
                bad(f"blocks[{i}] has no {a}")
        at, ml = b.attn, b.mlp
        if not (_is(at, _vit.Attention) and _is(ml, _vit.Mlp)):
            bad(f"blocks[{i}].attn / .mlp are not timm-shaped Attention / Mlp modules")
        if at.qkv.weight.shape != (3 * D, D) or at.qkv.bias is None or at.proj.weight.shape != (D, D) or at.proj.bias is None:
            bad(f"blocks[{i}].attn: qkv must be Linear(dim, 3 dim) with bias, proj Linear(dim, dim) with bias")
        if D % at.num_heads or D // at.num_heads != 64:
            bad("head dim must be 64")
        if abs(float(at.scale) - 64 ** -0.5) > 1e-9:
            bad("attention scale must be head_dim ** -0.5")
        if ml.fc1.weight.shape != (4 * D, D) or ml.fc2.weight.shape != (D, 4 * D) or ml.fc1.bias is None or ml.fc2.bias is None:
            bad(f"blocks[{i}].mlp: fc1 / fc2 must be Linear(dim, 4 dim) / Linear(4 dim, dim) with bias")
        if not isinstance(ml.act, nn.GELU) or getattr(ml.act, "approximate", "none") != "none":
            bad("mlp.act must be the exact (erf) GELU")
        for dn in ("attn_drop", "proj_drop"):
            if float(getattr(getattr(at, dn, None), "p", 0.0) or 0.0) != 0.0:
                bad(f"attn.{dn} must be 0 (the reference's configuration)")
        if float(getattr(getattr(ml, "drop", None), "p", 0.0) or 0.0) != 0.0:
            bad("mlp.drop must be 0 (the reference's configuration)")
        for nm in (b.norm1, b.norm2):
            if not isinstance(nm, nn.LayerNorm) or nm.weight is None:
                bad("norm1 / norm2 must be affine LayerNorms")
    if float(getattr(getattr(model, "pos_drop", None), "p", 0.0) or 0.0) != 0.0:
        bad("pos_drop must be 0")
    # Features of newer timm releases the fused path does not compute (timm 0.4.12, the reference's pin, has none of
    # them): a model that carries one would silently run a different function
    def live(m):   # a sub-module that does something
        return m is not None and not isinstance(m, nn.Identity)

    def drop_p(m):
        return float(getattr(m, "p", getattr(m, "prob", 0.0)) or 0.0)
    # The one readout besides the cls token: the mean of the patch tokens through fc_norm (timm's global_pool = "avg" with its default
    # fc_norm: norm an Identity, fc_norm an affine LayerNorm).  Every other mix of the three is another function.
    pooled = pooled_readout(model)
    for name in ("fc_norm", "norm_pre", "patch_drop", "attn_pool"):
        m = getattr(model, name, None)
        if live(m) and not (name == "patch_drop" and drop_p(m) == 0.0) and not (name == "fc_norm" and pooled):
            bad(f"{name} is not supported (timm 0.4.12's VisionTransformer has none)" if name != "fc_norm" else
                "fc_norm is supported behind global_pool = 'avg' with norm = Identity only (the cls-token readout has none)")
    if not pooled and getattr(model, "global_pool", "token") not in ("token", "", None):
        bad(f"global_pool = {model.global_pool!r}: only the cls-token readout and 'avg' with norm = Identity and fc_norm = LayerNorm(embed_dim) "
            "(the mean of the patch tokens through fc_norm) are supported")
    if not pooled and (not isinstance(model.norm, nn.LayerNorm) or model.norm.weight is None):
        bad("norm must be an affine LayerNorm (the cls-token readout)")
    if int(getattr(model, "num_prefix_tokens", 1)) != 1 or getattr(model, "no_embed_class", False) or \
            getattr(model, "reg_token", None) is not None:
        bad("exactly one prefix token (cls, with its own position embedding) is supported")
    if getattr(model, "dynamic_img_size", False):
        bad("dynamic_img_size is not supported")
    k = pe.kernel_size[0]
    img = getattr(model.patch_embed, "img_size", None)
    if img is not None:
        side = int(img[0] if isinstance(img, (tuple, list)) else img)
        if model.pos_embed.shape[1] != (side // k) ** 2 + 1:
            bad(f"pos_embed has {model.pos_embed.shape[1]} positions, the patch grid of a {side}-pixel image + cls needs "
                f"{(side // k) ** 2 + 1}")
    if model.pos_embed.shape[-1] != D or model.cls_token.shape[-1] != D:
        bad("pos_embed / cls_token width must equal embed_dim")
    for i, b in enumerate(blocks):
        for name in ("ls1", "ls2"):
            if live(getattr(b, name, None)):
                bad(f"blocks[{i}].{name} (LayerScale) is not supported")
        for name in ("q_norm", "k_norm"):
            if live(getattr(b.attn, name, None)):
                bad(f"blocks[{i}].attn.{name} (qk_norm) is not supported")
        if live(getattr(b.mlp, "norm", None)):
            bad(f"blocks[{i}].mlp.norm is not supported")
        for name in ("drop1", "drop2"):
            if drop_p(getattr(b.mlp, name, None)) != 0.0:
                bad(f"blocks[{i}].mlp.{name} must be 0 (the reference's configuration)")
        if getattr(b.attn, "fused_attn", False) and drop_p(getattr(b.attn, "attn_drop", None)) != 0.0:
            bad("attn_drop must be 0")


def _engine_forward(self, x):
    """Whole-model forward of an adopted (foreign-class) ViT: the fused HIP path instead of the class's eager one."""
    return self.__dict__["_cara_engine"].forward(x)


def set_cara(model: nn.Module, rank: int, scale: float, l_mu: float, l_std: float, _root=None, cp_length: int = 4) -> None:
    """Declare + initialise the CP tensors on the ViT and walk its children (``cara.py:98-166``).

    ``cp_length`` selects the order of the QKV tensorisation as ``image_classification/dim_experiment.py:264-297``
    (``set_CP``) does: 4 is ``src/cara``'s; 2 = ``[3L, dim * dim]`` (A2 ``[dim * dim, R]``, no A3 / A4); 3 = ``[3L, dim, dim]``
    (A3 ``[dim, R]``, no A4); 5 =
    ``[L, 3, dim, heads, dim/heads]`` (A1 ``[L, R]``, A2 ``[3, R]``, A3 ``[dim, R]``, A4 ``[heads, R]``, A5
    ``[dim/heads, R]``; ``attn_idx`` then advances by 1 per block, ``:334``).  Same initialisers in the same order."""
    root = _root
    if _is(model, _vit.VisionTransformer):
        root = model
        dim, heads, depth = model.embed_dim, model.blocks[0].attn.num_heads, len(model.blocks)
        # (name, rows, initialiser) in declaration order; the initialisers run in this order too, so the draws from the
        # global RNG are the reference's (cp_length 4: A1, A3, A4, P1, P3, then R1, R2 -- cara.py:127-139)
        xav, zero, orth = nn.init.xavier_normal_, nn.init.zeros_, nn.init.orthogonal_
        qkv_factors = {
            4: (("A1", 3 * depth, xav), ("A2", dim, zero), ("A3", heads, orth), ("A4", dim // heads, orth)),   # cara.py:112-117
            3: (("A1", 3 * depth, xav), ("A2", dim, zero), ("A3", dim, orth)),                                 # dim_experiment.py:286-292
            2: (("A1", 3 * depth, xav), ("A2", dim * dim, zero)),                                              # dim_experiment.py:293-297
            5: (("A1", depth, xav), ("A2", 3, orth), ("A3", dim, zero), ("A4", heads, orth),
                ("A5", dim // heads, orth)),                                                                   # dim_experiment.py:266-276
        }[cp_length]
        for name, rows, init in qkv_factors + (("P1", 9 * depth, xav), ("P2", dim, zero), ("P3", dim, orth)):   # cara.py:118-120
            p = nn.Parameter(th.empty([rows, rank]), requires_grad=True)
            init(p)
            setattr(model, "CP_" + name, p)
        for name in ("R1", "R2"):
            p = nn.Parameter(th.empty([rank]), requires_grad=True)
            if l_std != 0.0:
                nn.init.normal_(p, mean=l_mu, std=l_std)
            elif l_mu == 1.0 and l_std == 0.0:
                nn.init.ones_(p)
            # (else: left as allocated, like the reference, cara.py:134-139)
            setattr(model, "CP_" + name, p)
        for name, n in (("bias1", dim), ("bias2", dim * 4), ("bias3", dim)):
            setattr(model, "CP_" + name, nn.Parameter(th.zeros([n]), requires_grad=True))
        model.idx = 0
        model.attn_idx = 0
        if cp_length != 4:
            model.cp_l = cp_length
    if root is None:
        return
    for child in model.children():
        if _is(child, _vit.Attention):
            child.dp = nn.Dropout(0.1)
            child.s = scale
            child.dim = rank
            child.idx = root.idx
            child.attn_idx = root.attn_idx
            root.idx += 1
            root.attn_idx += 1 if cp_length == 5 else 3   # dim_experiment.py:334
            child.__dict__["_cara_owner"] = weakref.ref(root)
            setattr(child, "forward", cp_attn.__get__(child, child.__class__))  # noqa: B010
        elif _is(child, _vit.Mlp):
            child.dp = nn.Dropout(0.1)
            child.s = scale
            child.dim = rank
            child.idx = root.idx
            root.idx += 8
            child.__dict__["_cara_owner"] = weakref.ref(root)
            setattr(child, "forward", cp_mlp.__get__(child, child.__class__))  # noqa: B010
        elif len(list(child.children())) != 0:
            set_cara(child, rank, scale, l_mu, l_std, _root=root, cp_length=cp_length)


def cara(config: Dict[str, Any]) -> th.nn.Module:
    """Install CaRA on ``config["model"]`` and return it (``cara.py:169-188``)."""
    model = config["model"]
    rank = config["rank"]
    scale = config["scale"]
    l_mu = config["l_mu"]
    l_std = config["l_std"]
    if not _is(model, _vit.VisionTransformer):
        raise CaraError("cara_amd.cara() needs a timm-shaped VisionTransformer (class of that name with patch_embed, cls_token, "
                        "pos_embed, blocks[i].{norm1, attn.{qkv, proj, num_heads, scale}, norm2, mlp.{fc1, act, fc2}}, norm, head): "
                        "timm.models.create_model(...) output, or cara_amd.create_model(...)")
    _check_vit(model)
    if not (1 <= int(rank) <= 64):
        raise CaraError("rank must be in 1..64 (the K-extension is padded to 32 or 64 columns)")
    # optional sixth key, the `cp_length` of image_classification/dim_experiment.py (its `--dims`): order of the QKV
    # tensorisation.  4 (default) is src/cara's; 3 and 5 are rank-R in (in, out) too and run on the same kernels.
    # 2 parametrises each projection as a sum of R DENSE dim x dim matrices (CP_A2 [dim * dim, R], dim_experiment.py:203-207):
    # not low-rank in (in, out), so the QKV linear runs in the dense-delta form (two products on the same operand,
    # cara_gemm_args::B3; its gradient from the dense dW = X^T dY) while proj / fc1 / fc2 keep the factored kernels.
    cp_length = int(config.get("cp_length", 4))
    if cp_length not in (2, 3, 4, 5):
        raise CaraError("cp_length must be 2, 3, 4 or 5")
    if cp_length == 2 and config.get("weight_dropout", "off") == "exact":
        raise CaraError("cp_length 2 (dense QKV deltas) runs with weight_dropout = 'off' only")
    if pooled_readout(model) and config.get("weight_dropout", "off") == "exact":
        raise CaraError("a mean-pooled readout (global_pool = 'avg') runs with weight_dropout = 'off' only")
    if cp_length == 2 and getattr(model, "embed_dim", 128) % 128:
        raise CaraError("cp_length 2 (dense QKV deltas) needs embed_dim % 128 == 0 (its backward forms the dense x^T dY in 128 x 128 tiles)")
    global global_model
    global_model = model
    set_cara(model, rank, scale, l_mu, l_std, cp_length=cp_length)
    from .engine import CaraEngine
    model.__dict__["_cara_engine"] = CaraEngine(model, rank=int(rank), scale=float(scale), cp_length=cp_length)
    # optional key: how train mode treats the reference's Dropout(0.1) on the materialised dW (cara.py:35,57,81,92).
    # "off" (default): factored adapters, no weight-space dropout (fast); "exact": the reference's arithmetic.
    if type(model) is not _vit.VisionTransformer:
        # a foreign class (timm's own, or any same-shaped one): its parameters are adopted where they are (the engine
        # reads them by attribute and converts them to its HBM layout on the first forward); calling the model runs
        # the fused path, calling a block or a sub-module runs the patched forwards (module-level path)
        import types
        model.__dict__["forward"] = types.MethodType(_engine_forward, model)
    wd = config.get("weight_dropout", "off")
    if wd not in ("off", "exact"):
        raise CaraError("config['weight_dropout'] must be 'off' or 'exact'")
    model._cara_engine.weight_dropout = wd
    # optional key: "fp16" runs forward and backward on the same kernels compiled with IEEE-half MFMA operands (same MFMA rate;
    # logits inside north_star's 1e-3 of the fp32 reference; backward under a dynamic, device-side loss scale); default "bf16" is
    # the path BASELINE.json's metric is quoted on.  (Round 3's split-operand instrument is no precision MODE any more: call
    # cara_amd.precise.forward(model, images) where three-products-per-product logits of a few images are wanted.)
    prec = config.get("precision", "bf16")
    if prec == "bf16x3":
        raise CaraError("'bf16x3' is a parity instrument, not a precision mode: call cara_amd.precise.forward(model, images); "
                        "precision = 'fp16' is the mode that meets the 1e-3 logit tolerance at full speed")
    if prec not in ("bf16", "fp16"):
        raise CaraError("config['precision'] must be 'bf16' or 'fp16'")
    model._cara_engine.precision = prec
    return model
