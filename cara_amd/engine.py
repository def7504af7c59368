"""Engine: binds an adapted VisionTransformer to the whole-model entry points of libcara_hip.so.

torch owns device memory, the stream and autograd bookkeeping; every FLOP of the forward and
backward is issued by ``cara_vit_forward`` / ``cara_vit_backward`` (include/cara_hip.h).
Reference call sites this replaces: ``out = model(x)`` and ``loss.backward()`` of
``/root/reference/image_classification/vit_cp.py:46-49`` with the patched forwards of
``/root/reference/src/cara/cara.py:15-95``.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional

import torch

from . import _lib as L
from ._lib import CaraError, check, ptr, stream
from .feed import TABLES, Feed
from .loss import check_distill, check_loss


def _rp(rank: int) -> int:
    return 32 if rank <= 32 else 64


_MODEL = ("g", "s", "w", "cp", "head_w", "head_b")          # what every cara_vit_forward* entry starts with (include/cara_hip.h)
_RESULT = ("droppath", "workspace", "logits", "bad", "stream")   # ... and ends with


def forward_call(tables, values):
    """Which ``cara_vit_forward*`` entry a forward calls and with what: -> ``(entry, [(parameter, value), ...])``, the parameters
    named and ordered as the entry's prototype in include/cara_hip.h.  ``tables``: {name: table} of the tables present
    (``Feed.tables()``); ``values``: every other parameter by name -- with ``images`` an fp32 batch (``keep`` is then the only
    table there is), with ``pixels`` the rows of a resident split.  The resident entry is the one named after the last table
    present in Feed's order, each taking the tables in front of it too (NULL where not given); ``stat_scratch`` is NULL without
    ``aug``.  Touches no tensor and no library."""
    if "images" in values:
        if set(tables) - {"keep"}:
            raise CaraError(f"an fp32 batch takes a keep table only, not {sorted(tables)}")
        entry = "cara_vit_forward_keep" if tables else "cara_vit_forward"
        names = (*_MODEL, "images", *tables, *(n for n in _RESULT if tables or n != "bad"))
    else:
        level = max((Feed._fields.index(n) for n in tables), default=0)   # 0 rows, 1 boxes, 2 mix, 3 aug, 4 keep, 5 ra
        entry = "cara_vit_forward_u8_rows" + ("", "_crop", "_mix", "_aug", "_keep", "_ra")[level]
        names = (*_MODEL, "pixels", "n_split", *(("Hs", "Ws") if level else ()), "rows", *("boxes", "mix", "aug")[:level],
                 *(("stat_scratch",) if level >= 3 else ()), *(("ra", "ra_scratch") if level == 5 else ()),
                 *(("keep",) if level >= 4 else ()), "mean", "std", *_RESULT)
    got = {**dict.fromkeys(TABLES), **values, **tables}
    if "aug" not in tables:
        got["stat_scratch"] = None
    return entry, [(n, got[n]) for n in names]


class _VitFn(torch.autograd.Function):
    """logits = ViT+CaRA(images); gradients only into the head and the 12 CP tensors."""

    @staticmethod
    def forward(ctx, eng, images, droppath, head_w, head_b, *cp):
        # (grad mode is always off in here: CaraEngine.forward noted beforehand whether a backward can follow)
        logits = eng._run_forward(images, droppath, head_w, head_b, cp, need_backward=eng._need_backward)
        ctx.eng, ctx.droppath, ctx.shape_key = eng, droppath, eng._last_key
        ctx.save_for_backward(head_w, *cp)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        head_w, *cp = ctx.saved_tensors
        eng = ctx.eng
        if eng._last_key != ctx.shape_key or eng._fwd_serial != eng._bwd_ready:
            raise CaraError("backward must follow its own forward: the activation workspace holds one step")
        g = eng._run_backward(dlogits, ctx.droppath, head_w, cp)
        return (None, None, None, g["head_w"], g["head_b"], *[g[n] for n in eng.cp_fields])


class CaraEngine:
    def __init__(self, model, rank: int, scale: float, cp_length: int = 4):
        self._model = weakref.ref(model)
        self.rank, self.Rp, self.scale = rank, _rp(rank), scale
        # order of the QKV tensorisation (dim_experiment.py:188-207): 4 = src/cara's; 3 and 5 run on the same kernels
        self.cp_length = int(cp_length)
        self.cp_fields = L.cp_fields(self.cp_length)
        # Dropout(0.1) on the materialised dW (cara.py:35,57,81,92).  "off": factored adapters, no weight-space
        # dropout (the fast default; a mask on dW's elements does not factor).  "exact": train-mode forwards run on
        # W_eff = W + keep/(1-p) dW with a fresh mask per step and the adapter gradients come from the dense
        # dW = dY^T X, as in the reference (cara_vit_shape::wd_exact; ~1.4x the step time).  Eval is identical in both.
        self.weight_dropout = "off"
        self.weight_dropout_p = 0.1
        self.weight_dropout_seed = None   # tests pin the mask seed; None = a fresh draw from torch's RNG per forward
        # "bf16" (default): the fast path, bf16 MFMA operands.
        # "fp16": the SAME kernels compiled with IEEE-half MFMA operands (libcara_hip_f16.so: 11 significand bits at the bf16 MFMA
        # rate) for forward AND backward -- logits inside north_star's 1e-3 of the fp32 reference (measured: tests/test_model_gpu.py,
        # DESIGN.md section 2); the backward runs under a static loss scale (FP16_LOSS_SCALE: gradients need half's range, not its
        # precision) that is divided out of the flat fp32 gradient buffer before the all-reduce.  Whole-model calls only.
        self.precision = "bf16"
        self._ingested = None
        self._ingest_sig = None
        self._ws = {}
        self._last_key = None
        self._fwd_serial = 0
        self._bwd_ready = -1
        self._need_backward = True
        self._flat_grad = None
        self._grad_views = None
        self._slot = 0          # workspace slot of the call in flight (0 in the product; tools/two_stream_step.py runs two at once)
        # RNG streams of the stochastic parts (DropPath masks on the device, weight-dropout seeds on the host).
        # None = torch's global generators.  Under data parallelism every rank must draw DIFFERENT masks while the
        # parameters stay identical: seed_rank_streams(seed, rank) after the model is built.
        self._gen_dev = None
        self._gen_cpu = None
        self._gen_seed = None
        self._warned_wd = False
        from .modules import FactorPack
        self._factors = FactorPack(self)

    # Loss scaling of precision = "fp16" (half's range, not its precision, is what gradients lack), entirely on the device:
    # the scale lives in a device float (initially FP16_LOSS_SCALE), cara_cross_entropy_ex multiplies dlogits by it, the kernels
    # that WRITE the final gradients divide it out and raise a found-inf word when a value is not finite; that word sits behind
    # the last gradient in the flat buffer, so the step's one all-reduce carries it to every rank; cara_amp_update then halves the
    # scale (or doubles it after AMP_GROWTH_INTERVAL clean steps: torch.amp.GradScaler's rule) and cara_amd.optim.AdamW skips the
    # update of such a step -- no host synchronisation, no extra pass over the gradients.  A foreign optimiser is stepped behind a
    # host-side check of the word instead (one synchronisation per step, fp16 only).
    FP16_LOSS_SCALE = 1024.0
    AMP_GROWTH, AMP_BACKOFF, AMP_GROWTH_INTERVAL, AMP_MAX_SCALE = 2.0, 0.5, 2000, 65536.0
    DROPPATH_AHEAD = 32   # steps of DropPath masks per draw (draw_droppath)

    def _amp(self, dev):
        """device float[4] = {loss scale, clean steps since the last change, steps skipped so far, unused} (fp16 only)"""
        st = self.__dict__.get("_amp_state")
        if st is None or st.device != dev:
            st = torch.tensor([self.FP16_LOSS_SCALE, 0.0, 0.0, 0.0], device=dev)
            self._amp_state = st
        return st

    @property
    def loss_scale(self) -> float:
        """current loss scale of precision = "fp16" (synchronises; diagnostics)"""
        st = self.__dict__.get("_amp_state")
        return float(st[0].item()) if st is not None else self.FP16_LOSS_SCALE

    @property
    def skipped_steps(self) -> int:
        """steps whose gradients overflowed under the loss scale and were skipped (synchronises; diagnostics)"""
        st = self.__dict__.get("_amp_state")
        return int(st[2].item()) if st is not None else 0

    def _operands(self) -> str:
        return "fp16" if self.precision == "fp16" else "bf16"

    def _lib(self):
        return L.lib(self._operands())

    def _refuse_fp16_unfactored(self):
        if self.precision == "fp16" and (self.weight_dropout == "exact" or self.cp_length == 2):
            raise CaraError("precision = 'fp16' runs the factored adapters (weight_dropout = 'off', cp_length 3 / 4 / 5)")

    # ------------------------------------------------------------------ the readout
    @staticmethod
    def _pool(model) -> int:
        """cara_vit_shape::pool of this model: 1 = the mean of the patch tokens through fc_norm, 0 = the cls token through norm"""
        from .cara import pooled_readout
        return 1 if pooled_readout(model) else 0

    @classmethod
    def _readout_norm(cls, model):
        """the LayerNorm in front of the head (cara_vit_weights::norm_g / norm_b): fc_norm of a pooled model, else norm"""
        return model.fc_norm if cls._pool(model) else model.norm

    def _refuse_pooled_exact(self, model):
        if self.weight_dropout == "exact" and self._pool(model):
            raise CaraError("a mean-pooled readout (global_pool = 'avg') runs with weight_dropout = 'off' only")

    # ------------------------------------------------------------------ frozen weights -> HBM layout
    def _backbone_params(self, model):
        return [p for n, p in model.named_parameters() if not n.startswith("CP_") and not n.startswith("head.")]

    def _signature(self, model):
        # (the operand type is part of it: the 16-bit images of the frozen weights are written by the library in use)
        return (self._operands(),) + tuple((p.data_ptr(), p._version) for p in self._backbone_params(model))

    def _ingest(self, model, dev):
        with torch.cuda.device(dev):
            self._ingest_on(model, dev)

    def _ingest_on(self, model, dev):
        """One-time (and after any in-place change / load_state_dict): frozen fp32 parameters ->
        bf16 [depth, out, in] stacks plus transposed copies for the dX GEMMs, fp32 vectors stacked."""
        lib = self._lib()
        stream = lambda: L.stream(dev)   # noqa: E731  (everything below enqueues on dev's current stream)
        blocks = list(model.blocks)
        depth, D = len(blocks), model.embed_dim

        def f32(ts):
            return torch.stack([t.detach().to(dev, torch.float32) for t in ts]).contiguous()

        def bf16_pair(ws, out_f, in_f):
            """-> W, W^T row-major and both once more as K-panel-major images (the layout the GEMMs stage from)."""
            src = f32(ws)  # [depth, out, in]
            w = torch.empty(depth, out_f, in_f, dtype=torch.bfloat16, device=dev)
            wt = torch.empty(depth, in_f, out_f, dtype=torch.bfloat16, device=dev)
            wp, wtp = torch.empty_like(w), torch.empty_like(wt)
            check(lib.cara_f32_to_bf16(ptr(src), ptr(w), C.c_size_t(src.numel()), stream()), "cara_f32_to_bf16")
            for l in range(depth):
                check(lib.cara_transpose_bf16(ptr(w[l]), ptr(wt[l]), out_f, in_f, stream()), "cara_transpose_bf16")
                check(lib.cara_pack_b_panels(ptr(w[l]), in_f, out_f, in_f, ptr(wp[l]), stream()), "cara_pack_b_panels")
                check(lib.cara_pack_b_panels(ptr(wt[l]), out_f, in_f, out_f, ptr(wtp[l]), stream()), "cara_pack_b_panels")
            return w, wt, wp, wtp

        t = {}
        pw = model.patch_embed.proj.weight.detach().to(dev, torch.float32).reshape(D, -1).contiguous()
        t["patch_w"] = torch.empty_like(pw, dtype=torch.bfloat16)
        check(lib.cara_f32_to_bf16(ptr(pw), ptr(t["patch_w"]), C.c_size_t(pw.numel()), stream()), "cara_f32_to_bf16")
        t["patch_b"] = model.patch_embed.proj.bias.detach().to(dev, torch.float32).contiguous()
        t["cls"] = model.cls_token.detach().to(dev, torch.float32).reshape(-1).contiguous()
        t["pos"] = model.pos_embed.detach().to(dev, torch.float32).reshape(-1, D).contiguous()
        t["ln1_g"], t["ln1_b"] = f32([b.norm1.weight for b in blocks]), f32([b.norm1.bias for b in blocks])
        t["ln2_g"], t["ln2_b"] = f32([b.norm2.weight for b in blocks]), f32([b.norm2.bias for b in blocks])
        t["qkv_w"], t["qkv_wt"], t["qkv_wp"], t["qkv_wtp"] = bf16_pair([b.attn.qkv.weight for b in blocks], 3 * D, D)
        t["proj_w"], t["proj_wt"], t["proj_wp"], t["proj_wtp"] = bf16_pair([b.attn.proj.weight for b in blocks], D, D)
        t["fc1_w"], t["fc1_wt"], t["fc1_wp"], t["fc1_wtp"] = bf16_pair([b.mlp.fc1.weight for b in blocks], 4 * D, D)
        t["fc2_w"], t["fc2_wt"], t["fc2_wp"], t["fc2_wtp"] = bf16_pair([b.mlp.fc2.weight for b in blocks], D, 4 * D)
        t["qkv_b"] = f32([b.attn.qkv.bias for b in blocks])
        t["proj_b"] = f32([b.attn.proj.bias for b in blocks])
        t["fc1_b"] = f32([b.mlp.fc1.bias for b in blocks])
        t["fc2_b"] = f32([b.mlp.fc2.bias for b in blocks])
        readout = self._readout_norm(model)   # (fc_norm's parameters are backbone parameters too: _signature sees them change)
        t["norm_g"] = readout.weight.detach().to(dev, torch.float32).contiguous()
        t["norm_b"] = readout.bias.detach().to(dev, torch.float32).contiguous()
        w = L.VitWeights(**{n: ptr(t[n]) for n, _ in L.VitWeights._fields_})
        self._ingested = (t, w)
        self._ingest_sig = self._signature(model)

    def _ensure_ingested(self, model, dev) -> bool:
        """ingest when nothing is ingested yet, the signature moved or the model sits on another device; -> whether it did"""
        if self._ingested is None or self._ingest_sig != self._signature(model) or self._ingested[0]["cls"].device != dev:
            self._ingest(model, dev)
            return True
        return False

    # ------------------------------------------------------------------ per-shape state
    def _pos_rows(self, need, dev):
        """The token assembly adds row ``t`` of ``pos_embed`` to token ``t`` (row ``1 + keep[b][j]`` behind a patch dropout) and is not
        told how many rows there are.  Images of another size than the model's own -- a resident split read without boxes -- ask for
        ``need`` = grid + 1 rows; where the model has fewer, the kernels get a copy padded with zero rows (those tokens carry no
        position), so that nothing is read past the end of the parameter.  Said once per engine."""
        t, w = self._ingested
        have = t["pos"].shape[0]
        if have >= need:
            return
        if not self.__dict__.get("_warned_pos"):
            self._warned_pos = True
            import warnings
            warnings.warn(f"cara_amd: images of {need - 1} patches on a model whose pos_embed has {have - 1}: the patches beyond get no "
                          "position embedding (resize the model, or read the split through crop boxes of the model's size)", stacklevel=4)
        pad = torch.zeros(need, t["pos"].shape[1], dtype=torch.float32, device=dev)
        pad[:have].copy_(t["pos"])
        t["pos"] = pad
        w.pos = ptr(pad)

    def _state(self, model, B, img, dev, tokens=None):
        """``tokens``: 1 + K of a step behind a patch dropout; None = the grid's (img / patch)^2 + 1"""
        self._refuse_pooled_exact(model)   # (before anything is ingested, sized or launched)
        if self._ensure_ingested(model, dev):
            self._ws.clear()
        ncls = model.head.out_features
        exact = self.weight_dropout == "exact"
        if self.weight_dropout not in ("off", "exact"):
            raise CaraError(f"weight_dropout must be 'off' or 'exact', not {self.weight_dropout!r}")
        if exact and self.cp_length == 2:
            raise CaraError("cp_length 2 (dense QKV deltas) runs with weight_dropout = 'off' only")
        pe = model.patch_embed
        self._pos_rows((img // pe.proj.kernel_size[0]) ** 2 + 1, dev)
        if tokens is None:
            tokens = (img // pe.proj.kernel_size[0]) ** 2 + 1
        # (the token count is part of the key: a kept step and a full step of the same batch have workspaces of their own)
        pool = self._pool(model)
        key = (B, img, ncls, str(dev), exact, self._operands(), self._slot, tokens) + ((pool,) if pool else ())
        st = self._ws.get(key)
        if st is None:
            geom = L.Geom(len(model.blocks), model.embed_dim, model.blocks[0].attn.num_heads, self.rank, self.Rp, self.scale,
                          self.cp_length)
            # (sized with the exact-mode regions when that mode is selected; a call with wd_exact = 0 on the same
            # workspace -- eval -- simply does not touch them)
            patch = pe.proj.kernel_size[0]
            shape = L.VitShape(B, img, patch, pe.proj.in_channels, tokens, ncls,
                               float(self._readout_norm(model).eps), 1 if exact else 0, float(self.weight_dropout_p), 0, pool=pool)
            nbytes = self._lib().cara_vit_workspace_bytes(C.byref(geom), C.byref(shape))
            if nbytes == 0:
                raise CaraError(f"unsupported geometry for the HIP path: {geom.depth=} {geom.dim=} {geom.heads=} "
                                f"{shape.tokens=} (needs head dim 64, dim % 256 == 0, chans * patch^2 % 64 == 0, "
                                f"tokens <= 2^20)")
            if self._slot == 0 and not self.__dict__.get("_keep_ws"):
                self._ws.clear()  # one live workspace: activations of one step (slots > 0: the two-stream step's second half)
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            st = {"geom": geom, "shape": shape, "ws": ws, "logits": torch.empty(B, ncls, device=dev)}
            self._ws[key] = st
        self._last_key = key
        return st

    def _cp_ptrs(self, cp):
        return L.cp_ptrs(self.cp_fields, cp)

    # ------------------------------------------------------------------ forward / backward
    def _run_forward(self, images, droppath, head_w, head_b, cp, need_backward=True, keep=None):
        model = self._model()
        if images.ndim != 4 or images.shape[2] != images.shape[3]:
            raise CaraError("images must be [B, C, H, H]")
        images = images.contiguous().float()
        dev = images.device
        with torch.cuda.device(dev):   # the library enqueues on the stream it is given and launches on the current device
            return self._run_forward_on(model, images, Feed(None, keep=keep), droppath, head_w, head_b, cp, need_backward, dev)

    def _patches(self, img: int) -> int:
        """P: the patches of the grid of an ``img`` x ``img`` input"""
        return (img // self._model().patch_embed.proj.kernel_size[0]) ** 2

    @staticmethod
    def _check_table(name, t, batch=None, dev=None, P=None):
        """``t`` is the table ``name`` of ``feed.TABLES``: a contiguous int32 [*, columns] tensor (``keep``: 1 <= K <= ``P``) and, with
        ``batch`` and ``dev``, one of ``batch`` rows on ``dev`` -- refused before anything is enqueued"""
        width, msg = TABLES[name]
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.ndim != 2 or not t.is_contiguous() \
                or (t.shape[1] != width if width else not (1 <= t.shape[1] <= P)) \
                or (batch is not None and (t.device != dev or t.shape[0] != batch)):
            raise CaraError(msg.format(P=P))

    def _run_forward_on(self, model, source, feed, droppath, head_w, head_b, cp, need_backward, dev, teacher=False, bad=None):
        """``source``: an fp32 batch (``feed.rows`` is None and ``keep`` the only table there can be), or the resident uint8 split
        whose images ``feed.rows`` the tables of ``feed`` shape (``train_step_resident``; with ``boxes`` at the model's own input
        size).  Behind a ``keep`` the blocks run on 1 + K tokens, on a workspace of that size.  ``teacher``: the teacher pass of a
        distillation step -- eval semantics whatever ``model.training`` says (no weight dropout; the caller passes no DropPath);
        ``bad``: the counter of refused indices to use in this engine's own place (a model teacher counts into the student's)"""
        resident, keep = feed.rows is not None, feed.keep
        if resident:
            B, img = feed.rows.shape[0], source.pixels.shape[2] if feed.boxes is None else self._model_img(model)
        else:
            B, img = source.shape[0], source.shape[2]
        # (the tables were checked by the caller -- train_step, train_step_resident, forward_resident -- before anything was enqueued)
        st = self._state(model, B, img, dev, None if keep is None else 1 + keep.shape[1])
        if resident and st["shape"].chans != 3:
            raise CaraError("uint8 pixels are normalised with the three ImageNet channel statistics: chans must be 3")
        # weight-space dropout is a train-mode thing (nn.Dropout is the identity in eval); the backward of this
        # forward reads the same struct, i.e. the same seed, and regenerates the masks
        use_exact = self.weight_dropout == "exact" and model.training and self.weight_dropout_p > 0 and not teacher
        if model.training and not use_exact and not self._warned_wd and not teacher:
            self._warned_wd = True
            import warnings
            warnings.warn("cara_amd: train-mode forwards run the FACTORED adapters without the reference's Dropout(0.1) on the "
                          "materialised dW (cara.py:35,57,81,92); set model._cara_engine.weight_dropout = 'exact' (or the "
                          "'weight_dropout' key of cara()'s config) for the reference's train-mode arithmetic", stacklevel=3)
        st["shape"].wd_exact = 1 if use_exact else 0
        st["shape"].wd_p = float(self.weight_dropout_p)
        if use_exact:
            st["shape"].wd_seed = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=self._gen_cpu).item()) \
                if self.weight_dropout_seed is None else int(self.weight_dropout_seed)
        # eval / no_grad: nothing the backward alone reads is kept (cara_vit_shape::inference)
        st["shape"].inference = 0 if need_backward else 1
        cps = self._cp_ptrs([t.detach().contiguous() for t in cp])
        logits = torch.empty_like(st["logits"])
        values = {"g": C.byref(st["geom"]), "s": C.byref(st["shape"]), "w": C.byref(self._ingested[1]), "cp": C.byref(cps),
                  "head_w": head_w.detach().contiguous(), "head_b": head_b.detach().contiguous(), "droppath": droppath,
                  "workspace": st["ws"], "logits": logits, "stream": stream(dev)}
        if resident or keep is not None:   # (the entries that read indices count the bad ones)
            values["bad"] = self._bad_rows(dev) if bad is None else bad
        if resident:
            px, rows = source.pixels, feed.rows
            mean, std = self._eval_norm(dev)
            values.update(pixels=px, n_split=len(source), Hs=px.shape[2], Ws=px.shape[3], rows=rows, mean=mean, std=std)
            if feed.aug is not None:
                values["stat_scratch"] = self._aug_stat(dev, B)
            if feed.ra is not None:
                values["ra_scratch"] = self._ra_stat(dev, B)
        else:
            values["images"] = source
        entry, params = forward_call(feed.tables(), values)
        check(getattr(self._lib(), entry)(*[ptr(v) if v is None or torch.is_tensor(v) else v for _, v in params]), entry)
        self._fwd_serial += 1
        self._bwd_ready = self._fwd_serial if need_backward else -1
        return logits

    def _grad_buffers(self, model, dev):
        names = [(n, getattr(model, "CP_" + n)) for n in self.cp_fields] + [("head_w", model.head.weight), ("head_b", model.head.bias)]
        sizes = [p.numel() for _, p in names]
        if self._flat_grad is None or self._flat_grad.numel() != sum(sizes) + 1 or self._flat_grad.device != dev:
            from .dist import flat_views
            # (one word behind the gradients: "a non-finite gradient was written" -- all-reduced with them, so every rank sees it)
            self._flat_grad, self._grad_views = flat_views([(n, p.shape) for n, p in names] + [("_found_inf", (1,))], dev)
        return self._grad_views

    def _run_backward(self, dlogits, droppath, head_w, cp, prescaled=False):
        model = self._model()
        st = self._ws[self._last_key]
        dev = dlogits.device
        with torch.cuda.device(dev):
            return self._run_backward_on(model, st, dlogits, droppath, head_w, cp, dev, prescaled)

    def _run_backward_on(self, model, st, dlogits, droppath, head_w, cp, dev, prescaled=False):
        g = self._grad_buffers(model, dev)
        cps = self._cp_ptrs([t.detach().contiguous() for t in cp])
        gps = L.cp_ptrs(self.cp_fields, [g[n] for n in self.cp_fields])
        dl = dlogits.contiguous().float()
        if self.precision == "fp16":
            # every 16-bit gradient of the pass is loss-scale times larger; the kernels that write the final fp32 gradients divide
            # the scale out again (cara_vit_shape::loss_scale) and raise found_inf on a non-finite value
            amp = self._amp(dev)
            if not prescaled:   # (train_step's cross-entropy has scaled dlogits and cleared the word already)
                dl = dl * amp[0]
                g["_found_inf"].zero_()
            st["shape"].loss_scale, st["shape"].found_inf = ptr(amp), ptr(g["_found_inf"])
        else:
            st["shape"].loss_scale, st["shape"].found_inf = None, None
        check(self._lib().cara_vit_backward(C.byref(st["geom"]), C.byref(st["shape"]), C.byref(self._ingested[1]), C.byref(cps),
                                            ptr(head_w.detach().contiguous()), ptr(dl), ptr(droppath),
                                            ptr(st["ws"]), C.byref(gps), ptr(g["head_w"]), ptr(g["head_b"]), stream(dev)),
              "cara_vit_backward")
        self._bwd_ready = -1
        return g

    def seed_rank_streams(self, seed: int, rank: int = 0) -> None:
        """Give this replica its own DropPath / weight-dropout random streams: generator seed = seed * 2^20 + rank.
        Parameters are not touched (replicas stay identical); only the per-step masks differ between ranks."""
        self._gen_seed = int(seed) * (1 << 20) + int(rank)
        self._gen_dev = None
        self._dp_buf = None      # (masks drawn ahead from the previous stream are dropped)
        self._gen_cpu = torch.Generator().manual_seed(self._gen_seed)

    @staticmethod
    def _norm_device(dev):
        """torch.device with an explicit index ('cuda' / torch.device('cuda') -> the current device): what generators
        and tensors report, so that comparisons against it hold."""
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return dev

    def _device_generator(self, dev):
        if self._gen_seed is None:
            return None
        dev = self._norm_device(dev)
        if self._gen_dev is None or self._gen_dev.device != dev:
            self._gen_dev = torch.Generator(device=dev).manual_seed(self._gen_seed)
        return self._gen_dev

    def draw_droppath(self, model, B, dev) -> Optional[torch.Tensor]:
        """Per-sample multipliers mask/keep_prob of timm DropPath for both branches of every block,
        [depth, 2, B]; None in eval mode or when every rate is 0."""
        if not model.training:
            return None
        # timm 0.4.12: one `drop_path` per block; newer timm: `drop_path1` / `drop_path2` (same rate for both branches)
        def rate(b):
            r = [float(getattr(getattr(b, n, None), "drop_prob", 0.0) or 0.0) for n in ("drop_path", "drop_path1", "drop_path2")]
            if r[1] != r[2]:
                raise CaraError("drop_path1 and drop_path2 of a block must have the same rate")
            return r[0] if hasattr(b, "drop_path") else r[1]
        rates = [rate(b) for b in model.blocks]
        if not any(r > 0 for r in rates):
            return None
        dev = self._norm_device(dev)
        # the keep probabilities stay on the device: a host -> device copy here would make the host wait for the
        # previous step's kernels at the top of every step (and leave the GPU idle until the queue refills)
        key = (tuple(rates), str(dev))
        if self.__dict__.get("_keep_key") != key:
            self._keep = 1.0 - torch.tensor(rates, device=dev).reshape(-1, 1, 1)
            self._keep_key = key
        keep = self._keep
        gen = self._device_generator(dev)
        if dev.type != "cuda" or torch.cuda.is_current_stream_capturing():
            # (inside a hipGraph capture the draw must be a node of the graph; on the CPU there is nothing to amortise)
            return ((keep + torch.rand(len(rates), 2, B, device=dev, generator=gen)).floor_() / keep).contiguous()
        # DROPPATH_AHEAD steps' masks per draw: the four small torch launches of a draw (rand, add, floor, div: ~5 us each, serial
        # between the optimiser and the next forward) are paid once per DROPPATH_AHEAD steps instead of every step (r05).  Same
        # generator, same distribution; a step takes the next [depth, 2, B] slice (contiguous: no kernel).
        bkey = (key, B, id(gen))
        buf = self.__dict__.get("_dp_buf")
        if buf is None or self._dp_key != bkey or self._dp_next >= buf.shape[0]:
            buf = (keep + torch.rand(self.DROPPATH_AHEAD, len(rates), 2, B, device=dev, generator=gen)).floor_() / keep
            self._dp_buf, self._dp_key, self._dp_next = buf, bkey, 0
        out = buf[self._dp_next]
        self._dp_next += 1
        return out

    def forward(self, images, droppath: Optional[torch.Tensor] = None):
        model = self._model()
        if not images.is_cuda:
            raise CaraError("cara_amd runs on the GPU only: move the model and the images to a ROCm device "
                            "(there is no CPU fallback)")
        if not hasattr(model.head, "weight"):
            raise CaraError("the classifier head must be a Linear (num_classes > 0)")
        if droppath is None:
            droppath = self.draw_droppath(model, images.shape[0], images.device)
        cp = [getattr(model, "CP_" + n) for n in self.cp_fields]
        if model.head.weight.device != images.device or cp[0].device != images.device:
            raise CaraError("model parameters and images must be on the same device")
        params = [model.head.weight, model.head.bias, *cp]
        self._need_backward = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if self.precision not in ("bf16", "fp16"):
            raise CaraError(f"precision must be 'bf16' or 'fp16', not {self.precision!r}")
        self._refuse_fp16_unfactored()
        return _VitFn.apply(self, images, droppath, *params)

    # ------------------------------------------------------------------ fused train step
    def trainable_parameters(self):
        """The selection rule of vit_cp.py:175-183: names containing "CP" or "head"."""
        model = self._model()
        return [getattr(model, "CP_" + n) for n in self.cp_fields] + [model.head.weight, model.head.bias]

    ema = None   # the average recipe.fit(ema_decay=) trains with, left here for the caller

    def make_ema(self, decay: float = 0.9998, warmup: bool = False, capturable: bool = False):
        """``ema.ParamEma`` over ``trainable_parameters()`` (the frozen backbone does not move): hand it to ``train_step(..., ema=)``
        and score it with ``evaluate(..., weights=)``.  ``capturable = True`` for ``GraphedTrainStep``."""
        from .ema import ParamEma
        return ParamEma(self.trainable_parameters(), decay, warmup=warmup, capturable=capturable)

    def _check_ema(self, ema, dev, what):
        """``ema`` is None or a ParamEma whose shadows match trainable_parameters() one by one, on ``dev``"""
        if ema is None:
            return
        from .ema import ParamEma
        params = self.trainable_parameters()
        if not isinstance(ema, ParamEma) or len(ema.tensors) != len(params):
            raise CaraError(f"{what} must be a ParamEma over this model's trainable parameters (CaraEngine.make_ema)")
        for s, p in zip(ema.tensors, params):
            if s.shape != p.shape or s.device != dev or s.dtype != torch.float32 or not s.is_contiguous():
                raise CaraError(f"{what}: a shadow tensor is {tuple(s.shape)} on {s.device}, the model's parameter {tuple(p.shape)} on "
                                f"{dev} (CaraEngine.make_ema builds a matching one)")

    def _forward_weights(self, model, dev, weights):
        """-> (cp tensors, head weight, head bias) a forward reads: the model's own, or the shadows of ``weights``"""
        if weights is None:
            return [getattr(model, "CP_" + n) for n in self.cp_fields], model.head.weight, model.head.bias
        self._check_ema(weights, dev, "weights")
        k = len(self.cp_fields)
        return list(weights.tensors[:k]), weights.tensors[k], weights.tensors[k + 1]

    def _apply_gradients(self, optimizer=None, group=None, prescaled=False, clip_grad=None):
        """Tail of a train step, shared by train_step and the CPU multi-process tests: bind ``p.grad`` of every
        trainable parameter to its view of the flat buffer, ONE all-reduce of that buffer when the group has more than
        one rank -- a plain SUM when the gradients were computed from a dlogits already divided by the world size
        (``prescaled``: train_step), the mean otherwise -- the global-norm clip when ``clip_grad`` is given, and
        ``optimizer.step()``."""
        model = self._model()
        g = self._grad_views
        cp = [getattr(model, "CP_" + n) for n in self.cp_fields]
        for n, p in zip(list(self.cp_fields) + ["head_w", "head_b"], cp + [model.head.weight, model.head.bias]):
            if p.grad is None or p.grad.data_ptr() != g[n].data_ptr():
                p.grad = g[n]
        # the only data-path collective of a step: one RCCL all-reduce over xGMI of the flat buffer
        from .dist import allreduce_mean_, allreduce_sum_
        (allreduce_sum_ if prescaled else allreduce_mean_)(self._flat_grad, group)
        if clip_grad is not None:   # on the all-reduced buffer: every rank clips the same values by the same coefficient
            self._clip_flat(clip_grad)
        if self.precision == "fp16" and self._flat_grad.is_cuda:
            found = g["_found_inf"]
            dev = found.device
            with torch.cuda.device(dev):
                check(self._lib().cara_amp_update(ptr(self._amp(dev)), ptr(found), C.c_float(self.AMP_GROWTH), C.c_float(self.AMP_BACKOFF),
                                                  int(self.AMP_GROWTH_INTERVAL), C.c_float(self.AMP_MAX_SCALE), stream(dev)), "cara_amp_update")
            if optimizer is not None:
                from .optim import AdamW
                if isinstance(optimizer, AdamW):
                    optimizer.skip_flag = found          # the launch changes nothing when the word is set
                    optimizer.step()
                elif float(found.item()) == 0.0:         # a foreign optimiser: the host looks at the word (one sync per step)
                    optimizer.step()
            return
        if optimizer is not None:
            optimizer.step()

    @staticmethod
    def _smoothing(label_smoothing) -> float:
        if not isinstance(label_smoothing, (int, float)) or not (0.0 <= label_smoothing < 1.0):   # (a NaN fails the comparison)
            raise CaraError(f"label_smoothing must be a number in [0, 1), not {label_smoothing!r}")
        return float(label_smoothing)

    @staticmethod
    def _max_norm(clip_grad) -> Optional[float]:
        """``clip_grad``: None (no clip) or the max_norm of ``clip_grad_norm_``, a number > 0 (``inf`` only measures)"""
        if clip_grad is None:
            return None
        if isinstance(clip_grad, bool) or not isinstance(clip_grad, (int, float)) or not (clip_grad > 0.0):   # (a NaN fails the comparison)
            raise CaraError(f"clip_grad must be None or a number > 0, not {clip_grad!r}")
        return float(clip_grad)

    @staticmethod
    def _window(accumulate):
        """``accumulate``: None (every step is an optimiser step) or ``(i, k)``: micro-step ``i`` of a window of ``k``, 0 <= i < k"""
        if accumulate is None:
            return 0, 1
        ok = isinstance(accumulate, (tuple, list)) and len(accumulate) == 2 \
            and all(isinstance(v, int) and not isinstance(v, bool) for v in accumulate)
        if not ok or not (accumulate[1] >= 1 and 0 <= accumulate[0] < accumulate[1]):
            raise CaraError(f"accumulate must be (i, k) with integers 0 <= i < k, not {accumulate!r}")
        return int(accumulate[0]), int(accumulate[1])

    def _enter_window(self, i, k, B):
        """Order and batch size of the micro-steps of a window, checked before anything is launched: i runs 0, 1, ... k - 1, every
        micro-batch has the first one's size.  A refused call closes the window: the next one starts at 0."""
        nxt, k0, B0 = self.__dict__.get("_win") or (0, k, B)
        self._win = None
        if i != nxt or (nxt > 0 and (k != k0 or B != B0)):
            what = f"micro-step {nxt} of {k0} with batch size {B0}" if nxt > 0 else "micro-step 0"
            raise CaraError(f"accumulate = ({i}, {k}) with batch size {B}: the window expects {what} "
                            "(micro-steps come in order and share one batch size)")
        if k > 1 and torch.cuda.is_current_stream_capturing():
            raise CaraError("accumulate with k > 1 cannot be captured: the window spans several graph replays")
        if i + 1 < k:
            self._win = (i + 1, k, B)

    def _accumulate_flat(self, i, k, dev):
        """micro-step i of k > 1, after its backward: acc = flat (i == 0), acc += flat, and flat = acc + flat at the last one --
        left to right in fp32, the found-inf word (the last element) along with the gradients"""
        flat = self._flat_grad
        acc = self.__dict__.get("_acc_grad")
        if acc is None or acc.numel() != flat.numel() or acc.device != flat.device:
            acc = self._acc_grad = torch.empty_like(flat)
        dst, a, b = (acc, flat, None) if i == 0 else (acc, acc, flat) if i < k - 1 else (flat, acc, flat)
        check(self._lib().cara_grad_accumulate(ptr(dst), ptr(a), ptr(b), flat.numel(), stream(dev)), "cara_grad_accumulate")

    grad_norm = None   # device float [2] = (global L2 norm before the clip, coefficient applied) of the last clipped step

    def _clip_flat(self, max_norm):
        """cara_grad_clip over the gradient elements of the flat buffer (the found-inf word behind them stays out of the norm and
        is, in fp16, what leaves an overflowed step's gradients untouched) -> ``grad_norm``; nothing is read on the host"""
        flat = self._flat_grad
        if not flat.is_cuda:
            raise CaraError("clip_grad runs on the GPU only (no CPU path)")
        dev, n = flat.device, flat.numel() - 1
        def make():
            nbytes = int(self._lib().cara_grad_clip_scratch_bytes(n))
            if nbytes == 0:
                raise CaraError(f"cara_grad_clip takes 1 .. 2^31 elements, not {n}")
            return torch.empty(nbytes // 4, device=dev), torch.zeros(2, device=dev)
        scratch, out = self._pinned("clip", dev, n, make)
        found = self._grad_views["_found_inf"] if self.precision == "fp16" else None
        with torch.cuda.device(dev):
            check(self._lib().cara_grad_clip(ptr(flat), n, max_norm, ptr(scratch), ptr(found), ptr(out), stream(dev)), "cara_grad_clip")
        self.grad_norm = out
        return out

    def clip_grad_norm_(self, max_norm):
        """``torch.nn.utils.clip_grad_norm_(trainable_parameters(), max_norm)`` for the autograd path (``model(x); loss.backward()``)
        as two launches and no host read: -> the device tensor ``(norm, coef)``, which is ``grad_norm`` too.  Gradients that are
        not the views of the flat buffer yet (autograd hands out copies) are moved into it and ``p.grad`` is bound to the views,
        as after ``train_step``; like those, they are overwritten by the next backward -- ``zero_grad()`` before it.  Under
        ``precision = "fp16"`` the gradients of an overflowed backward are left as they are.  Inside a train step use
        ``train_step(..., clip_grad=max_norm)``: the clip then runs behind the all-reduce."""
        max_norm = self._max_norm(max_norm)
        if max_norm is None:
            raise CaraError("clip_grad_norm_ needs a max_norm > 0")
        params = self.trainable_parameters()
        if self._flat_grad is None or any(p.grad is None for p in params):
            raise CaraError("clip_grad_norm_ follows a backward: every trainable parameter must have a gradient")
        g = self._grad_views
        with torch.no_grad():
            for n, p in zip(list(self.cp_fields) + ["head_w", "head_b"], params):
                if p.grad.data_ptr() != g[n].data_ptr():
                    g[n].copy_(p.grad)
                    p.grad = g[n]
            return self._clip_flat(max_norm)

    def train_step(self, images, labels, optimizer=None, group=None, droppath: Optional[torch.Tensor] = None,
                   label_smoothing: float = 0.0, accumulate=None, clip_grad=None, ema=None, keep=None, class_weight=None,
                   logit_bias=None, sam_rho=None, loss=None, distill=None):
        """One fine-tuning step of vit_cp.py:45-50 without autograd bookkeeping:
        forward -> mean cross-entropy -> backward straight into ONE flat fp32 gradient buffer
        (12 CP tensors + head) -> a single all-reduce of that buffer when ``group``/the default
        process group has more than one rank -> ``optimizer.step()``.  Returns the loss (device
        scalar, local to this rank).  ``p.grad`` of every trainable parameter is a view of the flat
        buffer, so any torch optimizer consumes it unchanged.
        ``label_smoothing`` = eps in [0, 1): the loss is torch's ``cross_entropy(label_smoothing=eps)``
        (``cara_cross_entropy_mix``; 0 runs ``cara_cross_entropy_ex`` as before).
        ``accumulate = (i, k)``: micro-step ``i`` of a window of ``k`` micro-batches of one size, called in order.  Each runs
        forward, loss and backward with the loss divided by ``k`` as well; the flat buffers are summed left to right in fp32 in a
        second buffer of the same layout (``cara_grad_accumulate``), and only the LAST micro-step runs the tail -- one all-reduce,
        the clip, the loss-scale update, ``optimizer.step()`` -- on the sum.  Before it nothing is communicated and no parameter,
        moment or loss scale changes; in fp16 an overflow in any micro-step skips the whole window once.  The returned loss is
        the micro-batch's own mean.  ``k == 1`` (or None) is the step without a window.  Not under graph capture for ``k > 1``.
        ``clip_grad = max_norm`` (> 0): ``torch.nn.utils.clip_grad_norm_`` over all trainable tensors behind the all-reduce and
        before the optimiser (``cara_grad_clip``: two launches, no host read, bitwise the same on every rank); ``grad_norm`` then
        holds the device tensor (norm before the clip, coefficient).
        ``ema`` (a ``ParamEma`` of ``make_ema``): its one-launch update runs last in the tail, behind ``optimizer.step()`` -- with a
        window, at its last micro-step only.  A step skipped for an fp16 overflow updates the average too (cara_amd/ema.py).
        ``keep`` (device int32 [batch, K], e.g. one step of ``data.PatchDropout.draw``): patch dropout -- sample ``i`` trains on
        its cls token and the K patch tokens ``keep[i]``, each with its own row of the position embedding
        (``cara_vit_forward_keep``); the blocks run on 1 + K tokens.  None runs the step it was.
        ``class_weight`` / ``logit_bias`` (fp32 [classes] on the images' device, e.g. ``data.balanced_class_weight`` and
        ``data.logit_prior``): the loss is ``torch.nn.functional.cross_entropy(logits + logit_bias, q, weight=class_weight,
        reduction="sum") / batch`` on the step's soft target ``q`` (``cara_cross_entropy_bal``) -- divided by the batch size, not by
        the batch's weight mass, so windows, ranks and the all-reduce work as before.  The bias enters the loss only (logit-adjusted
        training): the model's logits and ``evaluate`` are untouched.  A negative or non-finite weight and a non-finite bias are
        refused; the values are read on the host once per tensor and version (an in-place change is checked again at the next
        step).  Both None: the loss launches are the ones they were.
        ``sam_rho`` (None, or a number >= 0): sharpness-aware minimisation (Foret et al.) -- every micro-step runs forward, loss and
        backward TWICE on the same input with the same DropPath multipliers: once at the weights w, which gives g1 and the returned
        loss, and once at w + e, e = sam_rho g1 / (||g1|| + 1e-12) over all trainable tensors, which gives the gradient g2 that the
        unchanged remainder of the step works on (accumulate, all-reduce, clip, loss scale, optimiser, ``ema``).  Between the passes:
        ``cara_grad_clip`` with max_norm = inf measures ||g1|| into buffers of SAM's own, ``cara_sam_perturb`` keeps a backup and moves
        the weights; behind the second backward ``cara_sam_restore`` copies the backup back bit for bit -- three small launches, no
        host read.  ``sam_loss`` is the second pass's loss (device scalar), ``sam_norm`` the device float [4] (carry, ||g1||, scale
        applied, 0).  In a window the perturbation comes from each micro-batch's own gradient.  Data parallel: the perturbation uses
        the rank's LOCAL gradient (m-sharpness with m = the per-rank batch: the direction g / ||g|| depends neither on the
        1 / world and 1 / k pre-division nor on the fp16 loss scale, which is divided out already); there is still one all-reduce
        per optimiser step, and the bitwise restore keeps the replicas identical.  fp16: an overflow in the first pass leaves the
        weights alone and is carried into the found-inf word behind the second pass -- the step is skipped and the scale backed
        off once.  ``sam_rho = 0.0`` runs both passes and leaves the gradients of the plain step, bit for bit.  Refused with
        ``weight_dropout = "exact"`` in train mode: that mode draws a fresh mask seed per forward, so the two passes would not see
        the same masks.  None: the launches are the ones they were.
        ``loss`` (None, a ``cara_amd.loss.BCE`` or a ``cara_amd.loss.Focal``): a sigmoid loss in the cross-entropy's place
        (``cara_sigmoid_loss``) on the same soft target -- labels, ``mix`` table and ``label_smoothing`` -- with the same pre-divided,
        loss-scaled ``dlogits``; it runs in both passes of a SAM step and composes with everything above.  Refused beside
        ``class_weight`` / ``logit_bias``, which are the softmax loss's.  A BCE's ``pos_weight`` is checked like ``class_weight``.
        None: the launches are the ones they were.
        ``distill`` (None or a ``cara_amd.loss.Distill``): knowledge distillation -- every micro-step first runs the TEACHER's forward on
        the same batch and ``keep`` table in eval semantics (no DropPath, no weight dropout, nothing kept for a backward:
        ``cara_vit_shape::inference``), copies its logits into ``teacher_logits``, and the loss launch is ``cara_distill_loss`` on the
        step's labels and ``label_smoothing``: the blended loss is what is returned.  The teacher is a ``ParamEma`` of this engine
        (the mean teacher: the update still runs last, so step n learns from the average after step n - 1), another ``cara()`` model
        (through its own engine and precision; a ``keep`` table needs the same patch grid) or a device fp32 [batch, classes] tensor
        (no pass).  Both passes of a SAM step read the one buffer.  The accumulate step, the all-reduce, the clip, the loss scale,
        the optimiser and the EMA update are untouched.  Refused beside ``loss=``, ``class_weight`` and ``logit_bias``.
        None: the launches are the ones they were."""
        eps = self._smoothing(label_smoothing)
        self._sam_rho(sam_rho)
        check_loss(loss, class_weight, logit_bias)
        check_distill(distill, loss, class_weight, logit_bias)
        if not images.is_cuda:
            raise CaraError("cara_amd runs on the GPU only (no CPU fallback)")
        dev = images.device
        if keep is not None:
            self._check_table("keep", keep, images.shape[0], dev, self._patches(images.shape[-1]))
        if labels.dtype != torch.int64 or labels.device != dev or labels.ndim != 1 or labels.shape[0] != images.shape[0]:
            raise CaraError("labels must be an int64 [batch] tensor on the images' device (the kernel reads 8-byte class indices)")
        teach = None
        if distill is not None:
            self._teacher_of(distill, dev, images.shape[0], keep=keep)
            if images.ndim != 4 or images.shape[2] != images.shape[3]:
                raise CaraError("images must be [B, C, H, H]")
            x32, bad = images.contiguous().float(), self._bad_rows(dev)
            # (the teacher's engine -- this one for an EMA teacher -- on the same batch and keep table, in eval semantics)
            teach = lambda eng, tm, hw, hb, cp: eng._run_forward_on(tm, x32, Feed(None, keep=keep), None, hw, hb, cp, False, dev,   # noqa: E731
                                                                    teacher=True, bad=bad)
        return self._step(dev, images.shape[0], lambda dp, hw, hb, cp: self._run_forward(images, dp, hw, hb, cp, keep=keep),
                          lambda: labels.contiguous(), optimizer, group, droppath, None, eps, accumulate, clip_grad, ema,
                          class_weight, logit_bias, sam_rho, loss, distill, teach)

    def _class_vectors(self, class_weight, logit_bias, ncls, dev):
        """``class_weight`` / ``logit_bias`` of a step, refused here -- before anything is launched -- unless each is None or a
        contiguous fp32 [ncls] tensor on ``dev`` with finite values (weights >= 0 as well).  The values cost a host read: one per
        tensor, remembered by (address, version), so a steady step reads nothing."""
        seen = self.__dict__.setdefault("_class_vec_ok", {})
        for name, t, floor in (("class_weight", class_weight, True), ("logit_bias", logit_bias, False)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.ndim != 1 or t.shape[0] != ncls or t.device != dev \
                    or not t.is_contiguous():
                raise CaraError(f"{name} must be a contiguous fp32 [{ncls}] tensor -- one entry per class of the head -- on the model's device")
            key = (t.data_ptr(), t._version)
            if seen.get(name) != key:
                bad = ~torch.isfinite(t) | (t < 0) if floor else ~torch.isfinite(t)
                if bool(bad.any()):
                    raise CaraError(f"{name} must be finite{' and >= 0' if floor else ''} in every class")
                seen[name] = key

    def _step(self, dev, B, forward, labels_of, optimizer, group, droppath, mix=None, smoothing=0.0, accumulate=None, clip_grad=None,
              ema=None, class_weight=None, logit_bias=None, sam_rho=None, loss=None, distill=None, teach=None):
        """What train_step and train_step_resident share -- everything but the image source: ``forward(droppath, head_w,
        head_b, cp)`` -> logits of the ``B`` samples with the backward's activations kept; ``labels_of()`` -> their int64 labels
        (called inside the step, on ``dev``).  With a ``mix`` table or a ``smoothing`` the loss is the soft-target one, with a
        ``class_weight`` or a ``logit_bias`` the weighted, logit-adjusted one on that target, with a ``loss`` object the sigmoid loss
        it describes on that target.  With a ``distill`` object, ``teach(engine, model, head_w, head_b, cp)`` -> the logits of the SAME
        input through the teacher's engine and weights in eval semantics; it runs before ``forward`` (a tensor teacher needs none).
        ``accumulate``, ``clip_grad``, ``ema`` and ``sam_rho`` as in ``train_step``."""
        model = self._model()
        rho = self._sam_rho(sam_rho)
        check_loss(loss, class_weight, logit_bias)
        plan = self._teacher_of(distill, dev, B, loss, class_weight, logit_bias)
        if rho is not None and self.weight_dropout == "exact" and model.training and self.weight_dropout_p > 0:
            raise CaraError("sam_rho cannot run with weight_dropout = 'exact' in train mode: that mode draws a fresh mask seed per "
                            "forward, so the two passes of a SAM step would see different masks")
        self._check_ema(ema, dev, "ema")
        if ema is not None and not ema.capturable and torch.cuda.is_current_stream_capturing():
            raise CaraError("a captured step needs make_ema(..., capturable=True): the weight would be frozen into the graph")
        win_i, win_k = self._window(accumulate)
        max_norm = self._max_norm(clip_grad)
        cp = [getattr(model, "CP_" + n) for n in self.cp_fields]
        if not hasattr(model.head, "weight"):
            raise CaraError("the classifier head must be a Linear (num_classes > 0)")
        hw, hb = model.head.weight, model.head.bias
        if hw.device != dev or any(t.device != dev for t in cp):
            raise CaraError("model parameters and images must be on the same device")
        self._refuse_fp16_unfactored()
        self._class_vectors(class_weight, logit_bias, hw.shape[0], dev)
        if loss is not None:
            loss.check_pos_weight(hw.shape[0], dev, self.__dict__.setdefault("_class_vec_ok", {}))
        self._enter_window(win_i, win_k, B)
        with torch.no_grad(), torch.cuda.device(dev):
            if droppath is None:
                droppath = self.draw_droppath(model, B, dev)
            if plan is not None:
                # ONE teacher pass per micro-step, before the student's forward (an EMA teacher runs on the student's workspace, which
                # an inference forward leaves free for it); both passes of a SAM step read its buffer
                kind, teng, tmodel = plan
                if kind == "tensor":
                    tlogits = distill.teacher
                else:
                    tcp, thw, thb = teng._forward_weights(tmodel, dev, distill.teacher if kind == "ema" else None)
                    tshape = (B, thw.shape[0])
                    tlogits = self._pinned("teacher_logits", dev, tshape, lambda: torch.empty(*tshape, device=dev))
                    tlogits.copy_(teach(teng, tmodel, thw, thb, tcp))
                self.teacher_logits = tlogits
            logits = forward(droppath, hw, hb, cp)
            labels = labels_of()
            B, ncls = logits.shape
            if self.__dict__.get("_loss_buf") is None or self._loss_buf.numel() != 1 + B or self._loss_buf.device != dev:
                self._loss_buf = torch.empty(1 + B, device=dev)
                self._dlogits = torch.empty(B, ncls, device=dev)
            if self._dlogits.shape != logits.shape:
                self._dlogits = torch.empty(B, ncls, device=dev)
            # dlogits leaves the cross-entropy already divided by the world size (the all-reduce is then a plain SUM) -- and by the
            # micro-steps of an accumulation window -- and, in the IEEE-half build, multiplied by the loss scale; the same launch
            # clears the step's found-inf word
            from .dist import world_size
            fp16 = self.precision == "fp16"
            gv = self._grad_buffers(model, dev)
            tail = (B, ncls, C.c_float(1.0 / (world_size(group) * win_k)), ptr(self._amp(dev)) if fp16 else None,
                    ptr(gv["_found_inf"]) if fp16 else None, stream(dev))

            def loss_and_backward(logits, loss_buf):
                if plan is not None:
                    alpha, temperature, hard = distill.c_args()
                    check(self._lib().cara_distill_loss(ptr(logits), ptr(tlogits), ptr(labels), ptr(mix), C.c_float(smoothing),
                                                        C.c_float(alpha), C.c_float(temperature), hard, ptr(loss_buf), ptr(self._dlogits),
                                                        *tail), "cara_distill_loss")
                elif loss is not None:
                    thr, fgamma, alpha = loss.c_args()
                    check(self._lib().cara_sigmoid_loss(ptr(logits), ptr(labels), ptr(mix), C.c_float(smoothing), C.c_float(thr),
                                                        C.c_float(fgamma), C.c_float(alpha), ptr(loss.pos_weight), int(loss.sum_classes),
                                                        ptr(loss_buf), ptr(self._dlogits), *tail), "cara_sigmoid_loss")
                elif class_weight is not None or logit_bias is not None:
                    check(self._lib().cara_cross_entropy_bal(ptr(logits), ptr(labels), ptr(mix), C.c_float(smoothing), ptr(class_weight),
                                                             ptr(logit_bias), ptr(loss_buf), ptr(self._dlogits), *tail),
                          "cara_cross_entropy_bal")
                elif mix is None and smoothing == 0.0:
                    check(self._lib().cara_cross_entropy_ex(ptr(logits), ptr(labels), ptr(loss_buf), ptr(self._dlogits), *tail),
                          "cara_cross_entropy_ex")
                else:
                    check(self._lib().cara_cross_entropy_mix(ptr(logits), ptr(labels), ptr(mix), C.c_float(smoothing), ptr(loss_buf),
                                                             ptr(self._dlogits), *tail), "cara_cross_entropy_mix")
                self._run_backward(self._dlogits, droppath, hw, cp, prescaled=True)
            loss_and_backward(logits, self._loss_buf)
            if rho is not None:
                # the gradient at w + rho g1 / |g1| in g1's place: measure, move, the same forward / loss / backward again, move back
                # -- before the accumulate and the tail, which then work on g2 as they did on g1
                sam = self._sam_perturb(model, dev, B, rho)
                loss_and_backward(forward(droppath, hw, hb, cp), sam["loss"])
                self._sam_restore(sam, dev)
            if win_k > 1:
                self._accumulate_flat(win_i, win_k, dev)
            if win_i == win_k - 1:
                self._apply_gradients(optimizer, group, prescaled=True, clip_grad=max_norm)
                if ema is not None:
                    ema.update()
        return self._loss_buf[0]

    # ------------------------------------------------------------------ knowledge distillation
    teacher_logits = None   # device fp32 [batch, classes]: what the last distilled micro-step's loss read as the teacher's logits

    @staticmethod
    def _img_of(model):
        img = getattr(model.patch_embed, "img_size", None)
        return tuple(img) if isinstance(img, (tuple, list)) else (img, img)

    def _teacher_of(self, distill, dev, B, loss=None, class_weight=None, logit_bias=None, keep=None):
        """``distill=`` of a step of ``B`` samples on ``dev``, refused here -- before anything is launched -- unless it is None or a
        ``loss.Distill`` this step can run; -> None, or (kind, the engine the teacher pass runs through, the model it runs on):
        ("tensor", None, None), ("ema", self, the model) or ("model", the teacher's engine, the teacher)."""
        d = check_distill(distill, loss, class_weight, logit_bias)
        if d is None:
            return None
        model = self._model()
        if not hasattr(model.head, "weight"):
            raise CaraError("the classifier head must be a Linear (num_classes > 0)")
        ncls, kind, t = model.head.weight.shape[0], d.kind(), d.teacher
        if kind == "fit":
            raise CaraError("Distill('ema') is resolved by recipe.fit(ema_decay=...): hand a step the ParamEma itself")
        if kind == "tensor":
            if t.dtype != torch.float32 or tuple(t.shape) != (B, ncls) or t.device != dev or not t.is_contiguous():
                raise CaraError(f"a tensor teacher must be a contiguous fp32 [{B}, {ncls}] tensor -- the batch's logits, one column per "
                                f"class of the head -- on the step's device, not {t.dtype} {tuple(t.shape)} on {t.device}")
            return kind, None, None
        if kind == "ema":
            self._check_ema(t, dev, "the distillation teacher")
            return kind, self, model
        teng = t._cara_engine
        if not hasattr(t.head, "weight") or t.head.weight.device != dev or getattr(t, "CP_" + teng.cp_fields[0]).device != dev:
            raise CaraError("the teacher model must sit on the step's device (and have a Linear head)")
        if t.head.weight.shape[0] != ncls:
            raise CaraError(f"the teacher model has {t.head.weight.shape[0]} classes, the student {ncls}")
        if self._img_of(t) != self._img_of(model):
            raise CaraError(f"the teacher model's image size {self._img_of(t)} is not the student's {self._img_of(model)}")
        if keep is not None and tuple(t.patch_embed.proj.kernel_size) != tuple(model.patch_embed.proj.kernel_size):
            raise CaraError("keep with a model teacher needs the same patch grid: the table names the student's patches")
        if teng.precision not in ("bf16", "fp16"):
            raise CaraError(f"precision must be 'bf16' or 'fp16', not {teng.precision!r}")
        teng._refuse_fp16_unfactored()
        return kind, teng, t

    # ------------------------------------------------------------------ sharpness-aware minimisation
    sam_loss = None   # device scalar: the loss of the last SAM step's second pass (at the perturbed weights)
    sam_norm = None   # device float [4] of the last SAM step: (found-inf carried over, |g1|, scale applied -- 0: weights left alone, 0)

    @staticmethod
    def _sam_rho(sam_rho) -> Optional[float]:
        """``sam_rho``: None (the plain step) or the radius of SAM's L2 ball, a finite number >= 0"""
        if sam_rho is None:
            return None
        if isinstance(sam_rho, bool) or not isinstance(sam_rho, (int, float)) or not (0.0 <= sam_rho < float("inf")):   # (a NaN fails the comparison)
            raise CaraError(f"sam_rho must be None or a finite number >= 0, not {sam_rho!r}")
        return float(sam_rho)

    def _sam_perturb(self, model, dev, B, rho):
        """between the two passes of a SAM step: |g1| over the gradient elements of the flat buffer (``cara_grad_clip`` with
        max_norm = inf writes no gradient; scratch and result are SAM's own, ``grad_norm`` stays the clip's), then
        ``cara_sam_perturb`` over the trainable tensors -- the backups live in one flat buffer with the gradient buffer's layout.
        -> the step's SAM buffers.  Nothing is read on the host."""
        flat, views = self._flat_grad, self._grad_views
        params = self.trainable_parameters()
        n = flat.numel() - 1

        def make():
            from .dist import flat_views
            nbytes = int(self._lib().cara_grad_clip_scratch_bytes(n))
            if nbytes == 0:
                raise CaraError(f"cara_grad_clip takes 1 .. 2^31 elements, not {n}")
            names = list(self.cp_fields) + ["head_w", "head_b"]
            backup, bviews = flat_views([(nm, views[nm].shape) for nm in names], dev)
            return {"scratch": torch.empty(nbytes // 4, device=dev), "norm": torch.zeros(2, device=dev), "state": torch.zeros(4, device=dev),
                    "backup": backup, "views": [bviews[nm] for nm in names], "grads": [views[nm] for nm in names], "plan": None}
        sam = self._pinned("sam", dev, (n, flat.data_ptr()), make)
        loss = self._pinned("sam_loss", dev, B, lambda: torch.empty(1 + B, device=dev))
        key = tuple(p.data_ptr() for p in params)
        if sam["plan"] is None or sam["plan"][0] != key:   # (the host arrays are kept while no parameter moves, as ParamEma's)
            k = len(params)
            if k > L.ADAMW_MAX_TENSORS:
                raise CaraError(f"sam_rho: {k} trainable tensors, one launch carries {L.ADAMW_MAX_TENSORS}")
            for p, g in zip(params, sam["grads"]):
                if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev or p.numel() != g.numel():
                    raise CaraError("sam_rho moves the trainable tensors in place: contiguous fp32 parameters on the step's device")
            arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])   # noqa: E731
            sam["plan"] = (key, k, arr(params), arr(sam["grads"]), arr(sam["views"]), (C.c_size_t * k)(*[p.numel() for p in params]))
        found = views["_found_inf"] if self.precision == "fp16" else None
        _, k, parr, garr, barr, narr = sam["plan"]
        lib = self._lib()
        check(lib.cara_grad_clip(ptr(flat), n, float("inf"), ptr(sam["scratch"]), ptr(found), ptr(sam["norm"]), stream(dev)), "cara_grad_clip")
        check(lib.cara_sam_perturb(k, parr, garr, barr, narr, rho, ptr(sam["norm"]), ptr(found), ptr(sam["state"]), stream(dev)),
              "cara_sam_perturb")
        sam["loss"] = loss
        self.sam_loss, self.sam_norm = loss[0], sam["state"]
        return sam

    def _sam_restore(self, sam, dev):
        """behind the second backward: the weights back from the backup, bit for bit, and the first pass's found-inf word added to
        the one the second pass's loss launch cleared"""
        _, k, parr, _, barr, narr = sam["plan"]
        found = self._grad_views["_found_inf"] if self.precision == "fp16" else None
        check(self._lib().cara_sam_restore(k, parr, barr, narr, ptr(sam["state"]), ptr(found), stream(dev)), "cara_sam_restore")

    # ------------------------------------------------------------------ training from a resident uint8 split
    def _bad_rows(self, dev):
        """device int32 [1] per device: samples whose row index was outside the split (cara_im2col_patches_u8_rows and
        cara_gather_labels count them instead of reading); never read inside a step -- resident_bad_rows()"""
        dev = self._norm_device(dev)
        bad = self.__dict__.setdefault("_bad", {})
        if dev not in bad:
            bad[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
        return bad[dev]

    def resident_bad_rows(self) -> int:
        """Out-of-range row indices counted since the last call (an image row and its label row count one each); reads and
        clears the counter: one host read."""
        n = 0
        for t in self.__dict__.get("_bad", {}).values():
            n += int(t.item())
            t.zero_()
        return n

    @staticmethod
    def _model_img(model):
        img = getattr(model.patch_embed, "img_size", None)
        img = img[0] if isinstance(img, (tuple, list)) else img
        if not isinstance(img, int) or img <= 0:
            raise CaraError("boxes need a model that states its input size (patch_embed.img_size)")
        return img

    def _pinned(self, kind, dev, size, make):
        """``make()`` once per (kind, device, size), and that buffer ever after, never replaced: a captured step holds its address,
        and a step of another size in between must not free it"""
        bufs = self.__dict__.setdefault("_pinned_bufs", {})
        buf = bufs.get((kind, dev, size))
        if buf is None:
            buf = bufs[(kind, dev, size)] = make()
        return buf

    def _aug_stat(self, dev, B):
        """the jitter kernels' statistic scratch (``cara_aug_stat_bytes``: 68 bytes per sample)"""
        return self._pinned("aug_stat", dev, B, lambda: torch.empty(int(self._lib().cara_aug_stat_bytes(B)) // 4, dtype=torch.float32, device=dev))

    def _ra_stat(self, dev, B):
        """the RandAugment pre-pass' scratch (``cara_ra_stat_bytes``: byte tables and partial histograms)"""
        return self._pinned("ra_stat", dev, B, lambda: torch.empty(int(self._lib().cara_ra_stat_bytes(B)) // 4, dtype=torch.int32, device=dev))

    def _resident_args(self, split, feed):
        """``split`` and ``feed`` (a ``Feed``) are what ``train_step_resident`` takes, refused before anything is enqueued -- what a
        table is before where it lives: a host-made table of the wrong type is refused as such; -> (model, device)"""
        model = self._model()
        rows, boxes = feed.rows, feed.boxes
        tables = {n: t for n, t in feed.tables().items() if n != "keep"}   # (keep's columns need the grid: last)
        for n, t in tables.items():
            self._check_table(n, t)
        dev = model.head.weight.device if hasattr(model.head, "weight") else None
        if dev is None:
            raise CaraError("the classifier head must be a Linear (num_classes > 0)")
        if dev.type != "cuda":
            raise CaraError("cara_amd runs on the GPU only (no CPU fallback)")
        px, lb = getattr(split, "pixels", None), getattr(split, "labels", None)
        if px is None or lb is None or px.dtype != torch.uint8 or px.ndim != 4 or px.shape[1] != 3 \
                or (boxes is None and px.shape[2] != px.shape[3]) or px.device != dev \
                or not px.is_contiguous() or lb.dtype != torch.int64 or lb.device != dev or lb.shape != px.shape[:1] or len(split) != px.shape[0]:
            raise CaraError("split must be a ResidentSplit (uint8 [N,3,H,H] pixels, int64 [N] labels) on the model's device")
        if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.device != dev or rows.ndim != 1 or rows.shape[0] == 0 \
                or not rows.is_contiguous():
            raise CaraError("rows must be a contiguous int64 [batch] tensor on the model's device")
        for n, t in tables.items():
            self._check_table(n, t, rows.shape[0], dev)
        if feed.keep is not None:
            self._check_table("keep", feed.keep, rows.shape[0], dev, self._patches(px.shape[2] if boxes is None else self._model_img(model)))
        return model, dev

    def _gather_labels(self, split, rows):
        dev, B = rows.device, rows.shape[0]
        buf = self._pinned("labels", dev, B, lambda: torch.empty(B, dtype=torch.int64, device=dev))   # (8 bytes per sample)
        check(self._lib().cara_gather_labels(ptr(split.labels.contiguous()), len(split), ptr(rows), ptr(buf), B, ptr(self._bad_rows(dev)),
                                             stream(dev)), "cara_gather_labels")
        return buf

    def train_step_resident(self, split, rows, optimizer=None, group=None, droppath: Optional[torch.Tensor] = None, boxes=None,
                            mix=None, label_smoothing: float = 0.0, accumulate=None, clip_grad=None, ema=None, aug=None, keep=None, ra=None,
                            class_weight=None, logit_bias=None, sam_rho=None, loss=None, distill=None):
        """``train_step`` on the images ``rows`` (device int64 [batch], any order, duplicates allowed) of a
        ``data.ResidentSplit`` on the model's device: the patch rows are built straight from the split's uint8 pixels
        (``cara_vit_forward_u8_rows``: no fp32 batch is written) and the labels gathered by ``cara_gather_labels``; everything
        else is train_step's.  A row outside the split is not read: it trains on a zero image with label 0 and is counted
        (``resident_bad_rows``).
        ``boxes`` (device int32 [batch, 5] = (x0, y0, w, h, flip) in the split's pixels, e.g. ``data.RandomResizedCropFlip.draw``):
        sample ``i`` is the bilinear resize of that box of image ``rows[i]`` to the model's input size, flipped where ``flip`` is
        non-zero (``cara_vit_forward_u8_rows_crop``); the split's pixels may then be [N,3,Hs,Ws] of any size.  A box that is not
        inside the image is not read either: a zero image, counted like a bad row.
        ``mix`` (device int32 [batch, 8], e.g. ``data.MixupCutmix.draw``): Mixup / CutMix by index -- sample ``i`` is blended with,
        or gets a rectangle of, the unmixed sample ``mix[i][0]`` of the same batch (``cara_vit_forward_u8_rows_mix``; with or without
        ``boxes``) and is trained on both labels (``cara_cross_entropy_mix``, ``data.soft_target``).  A table entry the kernel
        refuses -- ``data.check_mix`` -- gives a zero image, counted like a bad row.  ``label_smoothing``, ``accumulate``,
        ``clip_grad`` and ``ema`` as in ``train_step``.
        ``aug`` (device int32 [batch, 16], e.g. ``data.ColorJitterErase.draw``): colour jitter and Random Erasing by index -- each
        sample's brightness / contrast / saturation chain on its unmixed crop (the partner's own chain on the partner), then the
        mix, the normalisation and the erase rectangle (``cara_vit_forward_u8_rows_aug``; with or without ``boxes`` and ``mix``).
        A table entry the kernel refuses -- ``data.check_aug`` -- gives a zero image, counted like a bad row.
        ``keep`` (device int32 [batch, K], e.g. ``data.PatchDropout.draw``): patch dropout as in ``train_step`` -- only the kept
        patches' rows are built, each bit for bit the row the step without ``keep`` builds (``cara_vit_forward_u8_rows_keep``; with
        or without the other tables).  An entry outside the grid gives a zero patch row without a position, counted like a bad row.
        ``ra`` (device int32 [batch, 16], e.g. ``data.RandAugment.draw``): RandAugment by index -- each sample's crop is sampled through
        its 2x3 affine with a fill colour and passes its lookup slots (posterize, solarize, solarize-add, invert, autocontrast,
        equalize) before the jitter chain, the mix and the rest (``cara_vit_forward_u8_rows_ra``; with or without the other tables).
        A table entry the kernel refuses -- ``data.check_ra`` -- gives a zero image, counted like a bad row.
        ``class_weight`` / ``logit_bias`` as in ``train_step``: on the soft target of both labels where there is a ``mix`` table.
        ``sam_rho`` as in ``train_step``: the second pass reads the same rows through the same tables -- the feed is deterministic, erase
        noise included, so its input is bit for bit the first pass's.
        ``loss`` as in ``train_step``: on the soft target of both labels where there is a ``mix`` table.
        ``distill`` as in ``train_step``: the teacher reads the same split, rows and tables (``boxes``, ``mix``, ``aug``, ``ra``, ``keep``) --
        the feed is deterministic, so its input is bit for bit the student's -- and the loss is on the soft target of both labels.
        Without any of them, the step is the one it was."""
        eps = self._smoothing(label_smoothing)
        self._sam_rho(sam_rho)
        check_loss(loss, class_weight, logit_bias)
        check_distill(distill, loss, class_weight, logit_bias)
        feed = Feed(rows, boxes, mix, aug, keep, ra)
        model, dev = self._resident_args(split, feed)
        teach = None
        if distill is not None:
            self._teacher_of(distill, dev, rows.shape[0], keep=keep)
            # (every index the teacher pass refuses is counted into THIS engine's counter, whichever engine runs the pass: a bad row
            # then counts once more per teacher pass, and resident_bad_rows() of the training engine sees all of them)
            bad = self._bad_rows(dev)
            teach = lambda eng, tm, hw, hb, cp: eng._run_forward_on(tm, split, feed, None, hw, hb, cp, False, dev, teacher=True,   # noqa: E731
                                                                    bad=bad)
        return self._step(dev, rows.shape[0], lambda dp, hw, hb, cp: self._run_forward_on(model, split, feed, dp, hw, hb, cp, True, dev),
                          lambda: self._gather_labels(split, rows), optimizer, group, droppath, mix, eps, accumulate, clip_grad, ema,
                          class_weight, logit_bias, sam_rho, loss, distill, teach)

    def forward_resident(self, split, rows, droppath: Optional[torch.Tensor] = None, boxes=None, mix=None, weights=None, aug=None,
                         keep=None, ra=None):
        """logits [batch, classes] of the images ``rows`` of a resident split, without autograd (tests and tools); ``boxes``,
        ``mix``, ``aug``, ``keep`` and ``ra`` as in ``train_step_resident`` (a centre-cropped evaluation by hand); ``weights`` as in ``evaluate``"""
        feed = Feed(rows, boxes, mix, aug, keep, ra)
        model, dev = self._resident_args(split, feed)
        cp, hw, hb = self._forward_weights(model, dev, weights)
        self._refuse_fp16_unfactored()
        with torch.no_grad(), torch.cuda.device(dev):
            if droppath is None:
                droppath = self.draw_droppath(model, rows.shape[0], dev)
            return self._run_forward_on(model, split, feed, droppath, hw, hb, cp, False, dev)

    # ------------------------------------------------------------------ evaluation on the device
    def _eval_state(self, model, B, img, dev):
        """Workspace of the evaluation forwards: sized with cara_vit_shape::inference = 1 (two activation sets, nothing of the
        backward) and kept in ``_eval_ws``, beside the training workspaces of ``_ws``, which this never touches."""
        self._ensure_ingested(model, dev)
        ews = self.__dict__.setdefault("_eval_ws", {})
        self._pos_rows((img // model.patch_embed.proj.kernel_size[0]) ** 2 + 1, dev)
        ncls = model.head.out_features
        pool = self._pool(model)
        key = (B, img, ncls, str(dev), self._operands()) + ((pool,) if pool else ())
        st = ews.get(key)
        if st is None:
            pe = model.patch_embed
            geom = L.Geom(len(model.blocks), model.embed_dim, model.blocks[0].attn.num_heads, self.rank, self.Rp, self.scale,
                          self.cp_length)
            patch = pe.proj.kernel_size[0]
            shape = L.VitShape(B, img, patch, pe.proj.in_channels, (img // patch) ** 2 + 1, ncls, float(self._readout_norm(model).eps),
                               0, float(self.weight_dropout_p), 0, 1, pool=pool)
            nbytes = self._lib().cara_vit_workspace_bytes(C.byref(geom), C.byref(shape))
            if nbytes == 0:
                raise CaraError(f"unsupported geometry for the HIP path: {geom.depth=} {geom.dim=} {geom.heads=} {shape.tokens=}")
            st = {"geom": geom, "shape": shape, "ws": torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                  "logits": torch.empty(B, ncls, device=dev)}
            ews[key] = st
        return st

    def _eval_norm(self, dev):
        """per-channel mean / std of the reference's Normalize (vtab.py:94) as device fp32 vectors"""
        got = self.__dict__.get("_eval_meanstd")
        if got is None or got[0].device != dev:
            from .data import IMAGENET_MEAN, IMAGENET_STD
            got = (torch.tensor(IMAGENET_MEAN, device=dev), torch.tensor(IMAGENET_STD, device=dev))
            self._eval_meanstd = got
        return got

    def eval_workspace_bytes(self) -> int:
        """bytes held by the evaluation workspaces (diagnostics: tools/eval_bench.py)"""
        return sum(st["ws"].numel() for st in self.__dict__.get("_eval_ws", {}).values())

    def _eval_forward(self, model, x, dev, weights=None):
        """logits of one evaluation batch: uint8 pixels -> cara_vit_forward_u8, fp32 images -> cara_vit_forward, both on the
        inference-sized workspace.  The returned tensor is the workspace entry's own: valid until the next batch."""
        if x.ndim != 4 or x.shape[2] != x.shape[3]:
            raise CaraError("images must be [B, C, H, H]")
        st = self._eval_state(model, x.shape[0], x.shape[2], dev)
        cp, hw, hb = weights if weights is not None else self._forward_weights(model, dev, None)
        cps = self._cp_ptrs([t.detach().contiguous() for t in cp])
        hw, hb = hw.detach().contiguous(), hb.detach().contiguous()
        lib, args = self._lib(), (C.byref(st["geom"]), C.byref(st["shape"]), C.byref(self._ingested[1]), C.byref(cps), ptr(hw), ptr(hb))
        if x.dtype == torch.uint8:
            if st["shape"].chans != 3:
                raise CaraError("uint8 pixels are normalised with the three ImageNet channel statistics: chans must be 3")
            mean, std = self._eval_norm(dev)
            check(lib.cara_vit_forward_u8(*args, ptr(x.contiguous()), ptr(mean), ptr(std), None, ptr(st["ws"]), ptr(st["logits"]),
                                          stream(dev)), "cara_vit_forward_u8")
        else:
            check(lib.cara_vit_forward(*args, ptr(x.contiguous().float()), None, ptr(st["ws"]), ptr(st["logits"]), stream(dev)),
                  "cara_vit_forward")
        return st["logits"]

    def _eval_forward_views(self, model, split, rows, boxes, dev, weights):
        """logits [S*V, classes] of the images ``rows`` of a resident split through the crop boxes ``boxes``:
        cara_vit_forward_u8_rows_crop on the inference-sized workspace of that row count.  The returned tensor is the workspace
        entry's own, as in ``_eval_forward``."""
        st = self._eval_state(model, rows.shape[0], self._model_img(model), dev)
        if st["shape"].chans != 3:
            raise CaraError("uint8 pixels are normalised with the three ImageNet channel statistics: chans must be 3")
        cp, hw, hb = weights
        cps = self._cp_ptrs([t.detach().contiguous() for t in cp])
        mean, std = self._eval_norm(dev)
        px = split.pixels
        values = {"g": C.byref(st["geom"]), "s": C.byref(st["shape"]), "w": C.byref(self._ingested[1]), "cp": C.byref(cps),
                  "head_w": hw.detach().contiguous(), "head_b": hb.detach().contiguous(), "droppath": None, "workspace": st["ws"],
                  "logits": st["logits"], "bad": self._bad_rows(dev), "stream": stream(dev), "pixels": px, "n_split": len(split),
                  "Hs": px.shape[2], "Ws": px.shape[3], "rows": rows, "mean": mean, "std": std}
        entry, params = forward_call({"boxes": boxes}, values)
        check(getattr(self._lib(), entry)(*[ptr(v) if v is None or torch.is_tensor(v) else v for _, v in params]), entry)
        return st, st["logits"]

    def _eval_setup(self, what, split_or_batches, views, combine):
        """what ``evaluate`` and ``predict`` check before anything is sized: the arguments, the head, the precision, the device.
        Leaves the model in eval mode -> (model, device)"""
        model = self._model()
        model.eval()
        if combine not in L.EVAL_COMBINE:
            raise CaraError(f"{what}: combine must be one of {tuple(L.EVAL_COMBINE)}, not {combine!r}")
        if views is not None:   # (what the arguments are before where anything lives)
            from .data import EvalViews
            split = split_or_batches
            if not isinstance(views, EvalViews):
                raise CaraError(f"{what}: views must be a data.EvalViews")
            if not hasattr(split, "eval_view_shard") or getattr(split, "pixels", None) is None:
                raise CaraError(f"{what}(views=) reads a data.ResidentSplit by index: batches and callables carry no views")
        if not hasattr(model.head, "weight"):
            raise CaraError("the classifier head must be a Linear (num_classes > 0)")
        if self.precision not in ("bf16", "fp16"):
            raise CaraError(f"precision must be 'bf16' or 'fp16', not {self.precision!r}")
        if self.precision == "fp16" and self.cp_length == 2:
            raise CaraError("precision = 'fp16' runs the factored adapters (weight_dropout = 'off', cp_length 3 / 4 / 5)")
        dev = model.head.weight.device
        if dev.type != "cuda":
            raise CaraError("cara_amd runs on the GPU only: move the model to a ROCm device (there is no CPU fallback)")
        return model, dev

    def _eval_source(self, what, model, split_or_batches, batch_size, group, views):
        """this rank's batches of an evaluation pass -> (batches, shard): ``shard`` is the ``range`` of sample indices they cover
        when the source is a ``ResidentSplit`` (``dist.eval_shard``: contiguous, file order), None for batches that are this rank's
        part already.  With ``views`` a batch is ``(rows, boxes, labels, n_valid)`` of ``batch_size // V`` whole samples."""
        from . import dist as cdist
        rank, world = cdist.get_rank(group), cdist.world_size(group)
        if views is not None:
            split = split_or_batches
            if views.size is not None and views.size != self._model_img(model):
                raise CaraError(f"{what}: the views are made for a {views.size}-pixel input, the model takes {self._model_img(model)}")
            try:
                batches = split.eval_view_shard(views.table(*split.pixels.shape[2:]), batch_size, rank, world)
            except ValueError as e:
                raise CaraError(f"{what}: {e}") from None
            return batches, cdist.eval_shard(len(split), rank, world, int(batch_size) // views.V)
        if hasattr(split_or_batches, "eval_shard"):
            return split_or_batches.eval_shard(batch_size, rank, world), cdist.eval_shard(len(split_or_batches), rank, world, batch_size)
        return (split_or_batches() if callable(split_or_batches) else split_or_batches), None

    def _eval_logits(self, what, model, dev, split, batches, use, views, combine, labels_optional=False):
        """The loop ``evaluate`` and ``predict`` share: per batch the forward on the inference-sized workspace and, with more than
        one view, the combine launch -> yields ``(logits, per_view, labels, n_valid)``: the rows to score (the workspace's own
        tensor, or its ``combined`` buffer: valid until the next batch) and, with views, the per-view logits.  The caller holds
        ``torch.no_grad()`` and the device; nothing here reads the device.  ``labels_optional``: a batch may be the images alone
        or carry None as its labels."""
        lib = self._lib()
        if views is not None:
            V, mode = views.V, L.EVAL_COMBINE[combine]
        for item in batches:
            per_view = None
            if views is not None:
                rows, boxes, y, n_valid = item
                self._resident_args(split, Feed(rows, boxes))
                st, per_view = self._eval_forward_views(model, split, rows, boxes, dev, use)
                logits = per_view
                # one view: its mean logit is its logit, and its log-softmax is scored exactly as its logits are (loss, confidence
                # and ranks do not see a shift of the whole row) -- no combine launch, the pass is bit for bit the plain one
                if V > 1:
                    S = y.shape[0]
                    logits = st.setdefault("combined", {}).get(S)
                    if logits is None:
                        logits = st["combined"][S] = torch.empty(S, per_view.shape[1], device=dev)
                    check(lib.cara_eval_combine_views(ptr(per_view), per_view.shape[1], S, V, per_view.shape[1], mode, ptr(logits),
                                                      logits.shape[1], stream(dev)), "cara_eval_combine_views")
            else:
                if labels_optional and torch.is_tensor(item):
                    item = (item, None)
                x, y = item[0], item[1]
                n_valid = int(item[2]) if len(item) > 2 else x.shape[0]
                if not (labels_optional and y is None) and (
                        x.device != dev or y.device != dev or y.dtype != torch.int64 or y.ndim != 1 or y.shape[0] != x.shape[0]):
                    raise CaraError("a batch is (images or uint8 pixels, int64 [batch] labels[, n_valid]) on the model's device")
                if x.device != dev:
                    raise CaraError("a batch is (images or uint8 pixels[, labels[, n_valid]]) on the model's device")
                logits = self._eval_forward(model, x, dev, use)
            yield logits, per_view, y, n_valid

    def evaluate(self, split_or_batches, batch_size: int = 256, group=None, debug_hook=None, weights=None, report: bool = False,
                 bins: int = 15, views=None, combine: str = "prob") -> dict:
        """Top-1 / top-5 accuracy and mean cross-entropy of a whole split, on the device and sharded over the ranks of
        ``group``: ``test()`` of vit_cp.py:73-82 without its host read per batch.  -> ``dict(top1, top5, loss, n)``, the
        same on every rank; ``n`` is the number of images scored by all ranks together.

        ``split_or_batches``: a ``data.ResidentSplit`` (this rank's ``eval_shard(batch_size)`` is taken), or an iterable --
        or a callable returning one -- of ``(pixels_u8, labels, n_valid)`` / ``(images_fp32, labels)`` batches that are this
        rank's part already.  Each batch is one forward on an inference-sized workspace held beside the training workspace
        and one ``cara_eval_accumulate`` launch into a 40-byte device state; nothing is read back inside the loop.  Then
        one SUM all-reduce of the state and one read-back.  Like the reference's ``test()`` it leaves the model in eval mode.
        ``debug_hook(logits, labels, n_valid)`` (tests) sees every batch's logits; they are overwritten by the next batch.
        ``weights`` (a ``ParamEma`` of ``make_ema``): the pass scores the averaged weights -- the same forward on the same workspace
        is handed the shadow tensors as its CP and head pointers; nothing is copied and the model's parameters are not touched.
        ``report = True``: every batch's launch is ``cara_eval_accumulate_report`` into one more zeroed device buffer, the confusion
        matrix and ``bins`` equal-width confidence bins (include/cara_hip.h); state and report travel as ONE fp64 vector through the
        same single all-reduce and host read.  The dict then also holds ``confusion`` (CPU int64 [C, C], row = label, column =
        predicted class), ``support``, ``per_class`` (recall, NaN without support), ``precision`` (NaN for a class never
        predicted), ``mean_per_class``, ``ece`` and ``calibration = {count, hits, confidence}`` (``evalcount.report_result``).
        A head wider than ``CARA_EVAL_REPORT_MAX_CLASSES`` or a bin count the kernel refuses raises before the first forward.
        ``views`` (a ``data.EvalViews``; the source must be a ``ResidentSplit``, of any stored size): every image is scored through
        the V crop boxes of ``views.table(Hs, Ws)`` -- centre crop, flips, five / ten crops.  A batch is ``S = batch_size // V`` whole
        samples (``ResidentSplit.eval_view_shard``): one ``cara_vit_forward_u8_rows_crop`` of ``S*V`` rows, one
        ``cara_eval_combine_views`` into a ``[S, classes]`` buffer kept with the workspace, and the accumulate launch of above on
        the combined rows.  ``combine = "prob"``: the mean of the views' softmax probabilities, as its logarithm (loss
        ``-log pbar[y]``, confidence ``max pbar``); ``"logit"``: the mean of the views' logits.  One view: no combine launch in
        either mode -- its log-softmax scores exactly as its logits do -- and ``combined`` below is the view's logits themselves.
        ``n`` counts samples, not views; ``debug_hook(logits, labels, n_valid, combined)`` then sees the per-view logits
        ``[S*V, classes]`` and the combined rows.  Resampling is bilinear without an antialias filter (``data.EvalViews``).
        Views on another source, a table that leaves the split, more views than ``batch_size`` or an unknown ``combine`` raise
        before the first forward.  Without ``views`` the pass issues the launches it always did."""
        model, dev = self._eval_setup("evaluate", split_or_batches, views, combine)
        if report:
            ncls = int(model.head.out_features)
            if isinstance(bins, bool) or not isinstance(bins, int):
                raise CaraError(f"evaluate: bins must be an integer, not {bins!r}")
            report_bytes = int(self._lib().cara_eval_report_bytes(ncls, bins))
            if report_bytes == 0:
                raise CaraError(f"evaluate(report=True): {ncls} classes with {bins} bins is outside what cara_eval_accumulate_report "
                                "takes (at most 4096 classes, 1 to 64 bins)")
        from . import dist as cdist
        batches, _ = self._eval_source("evaluate", model, split_or_batches, batch_size, group, views)
        lib = self._lib()
        use = self._forward_weights(model, dev, weights)
        with torch.no_grad(), torch.cuda.device(dev):
            state = torch.zeros(int(lib.cara_eval_state_bytes()) // 8, dtype=torch.int64, device=dev)
            rep = torch.zeros(report_bytes // 8, dtype=torch.int64, device=dev) if report else None
            for logits, per_view, y, n_valid in self._eval_logits("evaluate", model, dev, split_or_batches, batches, use, views, combine):
                if report:
                    check(lib.cara_eval_accumulate_report(ptr(logits), logits.shape[1], ptr(y.contiguous()), logits.shape[0], n_valid,
                                                          logits.shape[1], ptr(state), ptr(rep), bins, stream(dev)),
                          "cara_eval_accumulate_report")
                else:
                    check(lib.cara_eval_accumulate(ptr(logits), logits.shape[1], ptr(y.contiguous()), logits.shape[0], n_valid,
                                                   logits.shape[1], ptr(state), stream(dev)), "cara_eval_accumulate")
                if debug_hook is not None:
                    debug_hook(logits, y, n_valid) if views is None else debug_hook(per_view, y, n_valid, logits)
            # the five words as fp64 (counts are exact up to 2^53): ONE collective carries integers and the loss sum alike
            vec = state.to(torch.float64)
            vec[3] = state.view(torch.float64)[3]
            if report:
                # ... and the report's words behind them: the bin_conf region holds doubles, like the loss word
                words = torch.cat([vec, rep.to(torch.float64)])
                words[-bins:] = rep.view(torch.float64)[-bins:]
                cdist.allreduce_sum_(words, group)
                words = words.cpu()                # the pass's only host read
                n, t1, t5, loss, bad = words[:5].tolist()
            else:
                cdist.allreduce_sum_(vec, group)
                n, t1, t5, loss, bad = vec.tolist()   # the pass's only host read
        if bad:
            raise CaraError(f"evaluate: {int(bad)} label(s) outside [0, {model.head.out_features})")
        if report:
            from . import evalcount
            return evalcount.report_result(words[:5], evalcount.report_from_vector(words[5:], ncls, bins))
        d = max(n, 1.0)
        return {"top1": t1 / d, "top5": t5 / d, "loss": loss / d, "n": int(n)}

    def predict(self, split_or_batches, k: int = 5, batch_size: int = 256, group=None, weights=None, views=None,
                combine: str = "prob"):
        """The model's answer for every image of a split, on the device: the pass of ``evaluate`` -- the same sources, checks,
        inference-sized workspace, ``weights=`` and ``views=`` / ``combine=`` -- with ONE ``cara_eval_predict`` launch per batch
        (on the combined rows with more than one view) instead of the counting launch, and no host read anywhere.
        -> ``evalcount.Predictions``: device tensors ``topk`` int32 [N, k] (the ``k`` best classes, best first, ties to the lowest
        class index), ``prob`` fp32 [N, k] (their softmax probabilities), ``loss`` fp32 [N] (the per-sample cross-entropy), ``rank``
        int32 [N] (the label's position in the sorted row: 0 = a top-1 hit, ``< 5`` = a top-5 hit, -1 = a label outside the
        classes) and ``labels``; include/cara_hip.h has the rules.  ``1 <= k <= 16``; slots beyond the class count hold -1 / 0.

        A ``ResidentSplit``: ``N = len(split)`` and row ``i`` is sample ``i`` in file order.  Every rank of ``group`` fills the
        rows of its (contiguous) shard in one zeroed table -- padded rows are never written -- and ONE integer SUM all-reduce of
        the table's 32-bit words (the floats as their bits: ``x + 0`` is exact on integers) leaves the whole table on every
        rank, bit for bit the one a single rank fills.  An iterable, or a callable returning one, of ``(pixels_u8 or images,
        labels[, n_valid])`` batches: the table holds this rank's valid rows in arrival order and there is no collective; a
        batch may be the images alone or carry None as its labels (every batch alike), then ``loss``, ``rank`` and ``labels``
        are None.  ``Predictions.counts()`` gives ``evaluate``'s dict, ``confusion`` / ``errors`` / ``confident`` / ``save`` the
        per-sample views, each with one host read."""
        from . import dist as cdist
        from .evalcount import Predictions
        model, dev = self._eval_setup("predict", split_or_batches, views, combine)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= L.PREDICT_MAX_K:
            raise CaraError(f"predict: k must be an integer in [1, {L.PREDICT_MAX_K}], not {k!r}")
        batches, shard = self._eval_source("predict", model, split_or_batches, batch_size, group, views)
        lib = self._lib()
        use = self._forward_weights(model, dev, weights)
        with torch.no_grad(), torch.cuda.device(dev):
            if shard is not None:
                # the whole table as ONE buffer of 32-bit words: [N, k] indices, [N, k] probabilities, [N] losses, [N] ranks
                N = len(split_or_batches)
                words = torch.zeros(N * (2 * k + 2), dtype=torch.int32, device=dev)
                topk, prob = words[:N * k].view(N, k), words[N * k:2 * N * k].view(torch.float32).view(N, k)
                loss, rank = words[2 * N * k:2 * N * k + N].view(torch.float32), words[2 * N * k + N:]
                done = shard.start
                for logits, _, y, n_valid in self._eval_logits("predict", model, dev, split_or_batches, batches, use, views, combine):
                    check(lib.cara_eval_predict(ptr(logits), logits.shape[1], ptr(y.contiguous()), logits.shape[0], n_valid,
                                                logits.shape[1], k, done, N, ptr(topk), ptr(prob), ptr(loss), ptr(rank), stream(dev)),
                          "cara_eval_predict")
                    done += n_valid
                cdist.allreduce_sum_(words, group)
                return Predictions(topk, prob, loss, rank, split_or_batches.labels)
            # batches of unknown number: a table per batch, its valid rows joined behind the loop (on the device)
            parts, labelled = [], None
            for logits, _, y, n_valid in self._eval_logits("predict", model, dev, split_or_batches, batches, use, views, combine,
                                                           labels_optional=True):
                if labelled is None:
                    labelled = y is not None
                if labelled != (y is not None):
                    raise CaraError("predict: either every batch carries labels or none does")
                B = logits.shape[0]
                t = (torch.empty(B, k, dtype=torch.int32, device=dev), torch.empty(B, k, device=dev),
                     torch.empty(B, device=dev) if labelled else None, torch.empty(B, dtype=torch.int32, device=dev) if labelled else None,
                     y.contiguous() if labelled else None)
                check(lib.cara_eval_predict(ptr(logits), logits.shape[1], ptr(t[4]), B, n_valid, logits.shape[1], k, 0, B,
                                            ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), stream(dev)), "cara_eval_predict")
                parts.append([c[:n_valid] if c is not None else None for c in t])
            if not parts:
                return Predictions(torch.empty(0, k, dtype=torch.int32, device=dev), torch.empty(0, k, device=dev))
            return Predictions(*[torch.cat(c) if c[0] is not None else None for c in zip(*parts)])

    # module-level entries (cara.cp_attn / cara.cp_mlp): the reference's patched forwards
    def _weights(self, model, dev):
        if self._ensure_ingested(model, dev):
            self._ws.clear()
        return self._ingested

    def _module_args(self, x):
        model = self._model()
        if not x.is_cuda:
            raise CaraError("cara_amd runs on the GPU only (no CPU fallback)")
        if x.ndim != 3 or x.shape[2] != model.embed_dim or x.shape[1] > 2 ** 20:
            raise CaraError("module-level forward expects x of shape [B, N <= 2^20, embed_dim]")
        if self.cp_length == 2:
            raise CaraError("with cp_length 2 (dense QKV deltas) call the whole model: the module-level Attention.forward / "
                            "Mlp.forward entries run the factored adapters only")
        if self.weight_dropout == "exact" and model.training:
            raise CaraError("the module-level forwards (Attention.forward / Mlp.forward called on their own) run the factored "
                            "adapters only: with weight_dropout = 'exact' in train mode call the whole model, or switch to eval()")
        return model, [getattr(model, "CP_" + n) for n in self.cp_fields]

    def attn_forward(self, child, x):
        from .modules import AttnFn
        model, cp = self._module_args(x)
        with torch.cuda.device(x.device):
            return AttnFn.apply(self, child, x, *cp)

    def mlp_forward(self, child, x):
        from .modules import MlpFn
        model, cp = self._module_args(x)
        with torch.cuda.device(x.device):
            return MlpFn.apply(self, child, x, *cp)
