"""The mean-pooled readout on the host: the restated forward of tests/pool_model.py against the oracle (bitwise with the cls readout)
and against a plain-torch pooled ViT, the pool kernels' derived bounds held by an fp32 restatement in another summation order, and
the API: what create_model / cara() accept and refuse.  CPU only."""
import functools

import numpy as np
import pytest
import torch

from tests import pool_model as PM
from tests import tolerances as T

DEPTH, IMG, NCLS, B = 2, 96, 5, 3


@functools.lru_cache(maxsize=None)
def _case():
    from oracle import cara_oracle as O
    w = O.synthetic_backbone(depth=DEPTH, img=IMG, num_classes=NCLS)
    cp = O.synthetic_cp(rank=8, depth=DEPTH)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, IMG, IMG, generator=g)
    return w, cp, x


def _keep():
    g = torch.Generator().manual_seed(11)
    keep = torch.tensor([0.9, 0.8]).reshape(-1, 1, 1)
    return ((keep + torch.rand(DEPTH, 2, B, generator=g)).floor() / keep).float()


@pytest.mark.parametrize("factored", [False, True])
@pytest.mark.parametrize("bf16_sim", [False, True])
@pytest.mark.parametrize("droppath", [False, True])
def test_the_restated_loop_is_the_oracles_with_the_cls_readout(factored, bf16_sim, droppath):
    from oracle import cara_oracle as O
    w, cp, x = _case()
    kw = dict(s=0.1, depth=DEPTH, factored=factored, bf16_sim=bf16_sim, drop_path_keep=_keep() if droppath else None)
    with torch.no_grad():
        a = PM.forward(x, w, cp, readout="token", **kw)
        b = O.vit_cara_forward(x, w, cp, **kw)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_the_pooled_readout_is_the_plain_torch_pooled_model():
    """adapters at zero strength (s = 0: the adapted linears are the frozen ones) against timm's pooled forward, eager"""
    w, cp, x = _case()
    pw = PM.pooled_weights(w)
    m = PM.plain_torch_pooled_vit(pw, DEPTH, IMG, NCLS)
    with torch.no_grad():
        ref = m(x)
        for factored in (False, True):
            got = PM.forward(x, pw, cp, s=0.0, depth=DEPTH, factored=factored, readout="avg")
            assert float((got - ref).abs().max()) <= T.HOST_ATOL, factored
        tok = PM.forward(x, w, cp, s=0.0, depth=DEPTH, readout="token")
    assert float((tok - ref).abs().max()) > 1e-2     # another function, not another rounding


SHAPES = [(b, n, d) for b in (1, 3) for n in (1, 2, 49, 196, 576) for d in (256, 260)] + [(3, 196, 768), (1, 49, 1024)]


@pytest.mark.parametrize("kind", PM.FAMILIES)
def test_the_other_order_restatements_stay_inside_the_bounds(kind):
    for (b, n, d) in SHAPES:
        x = PM.family(kind, b, n + 1, d, seed=n + d)
        x[:, 0] = float("nan")
        out = PM.token_mean_other_order(x, 1)
        err = (out.double() - PM.mean64(x, 1)).abs()
        assert bool((err <= PM.mean_bound(x, 1)).all()), (kind, b, n, d, float(err.max()))
        dpool = PM.family(kind, b, 2, d, seed=7)[:, 1]
        for rs in (None, torch.tensor([1.0 / 0.9, 0.0, 1.0 / 0.7])[:b]):
            dx64, v64 = PM.bwd64(dpool, rs, n + 1, 1)
            for dtype in (torch.bfloat16, torch.float16):
                dx, dyb = PM.token_mean_bwd_other_order(dpool, rs, n + 1, 1, dtype)
                assert PM.dx_ok(dx, dx64) and PM.dyb_ok(dyb, v64, dtype), (kind, b, n, d, dtype)
                assert not dx[:, 0].any() and not dyb[:, 0].float().any()


def test_the_interval_check_refuses_a_neighbour():
    """dyb_ok is not vacuous: the next 16-bit value up is outside the interval of a value that is not near a tie"""
    v = torch.tensor([[[1.0 + 2.0 ** -9]]], dtype=torch.float64)       # a quarter of a bf16 step above 1
    assert PM.dyb_ok(torch.tensor([[[1.0]]], dtype=torch.bfloat16), v, torch.bfloat16)
    assert not PM.dyb_ok(torch.tensor([[[1.0 + 2.0 ** -7]]], dtype=torch.bfloat16), v, torch.bfloat16)
    img = PM.to_panels(torch.arange(6 * 64, dtype=torch.float32).reshape(6, 64), 8)
    assert img.shape == (2, 8, 32) and torch.equal(PM.from_panels(img, 6), torch.arange(6 * 64, dtype=torch.float32).reshape(6, 64))
    assert float(img[1, 2, 3]) == 2 * 64 + 32 + 3


# ---- API -----------------------------------------------------------------------------------------------------------------------------
def _cfg(m, **kw):
    return {"model": m, "rank": 8, "scale": 0.1, "l_mu": 1.5, "l_std": 0.1, **kw}


def _pooled(**kw):
    from cara_amd import create_model
    return create_model("vit_base_patch16_224_in21k", depth=2, img_size=IMG, num_classes=NCLS, global_pool="avg", **kw)


def test_create_model_follows_timms_rule_for_fc_norm():
    from cara_amd import create_model
    keys = set(_pooled().state_dict())
    assert {"fc_norm.weight", "fc_norm.bias"} <= keys and not any(k.startswith("norm.") for k in keys)
    tok = create_model("vit_base_patch16_224_in21k", depth=2, img_size=IMG, num_classes=NCLS)
    assert tok.global_pool == "token" and {"norm.weight", "norm.bias"} <= set(tok.state_dict()) and not hasattr(tok, "fc_norm")
    assert not any(k.startswith("fc_norm") for k in tok.state_dict())
    assert "fc_norm.weight" in _pooled(fc_norm=True).state_dict() and "norm.weight" in _pooled(fc_norm=False).state_dict()
    assert isinstance(_pooled().norm, torch.nn.Identity) and _pooled().fc_norm.eps == 1e-6


def test_cara_accepts_the_pooled_model_and_reads_its_pool():
    from cara_amd import cara
    from cara_amd import _lib
    m = cara(_cfg(_pooled()))
    eng = m._cara_engine
    assert eng._pool(m) == 1 and eng._readout_norm(m) is m.fc_norm
    sig = eng._signature(m)
    with torch.no_grad():
        m.fc_norm.weight.mul_(1.5)
    assert eng._signature(m) != sig                      # a changed fc_norm is ingested again
    from cara_amd import create_model
    t = cara(_cfg(create_model("vit_base_patch16_224_in21k", depth=2, img_size=IMG, num_classes=NCLS)))
    assert t._cara_engine._pool(t) == 0 and t._cara_engine._readout_norm(t) is t.norm
    assert [n for n, _ in _lib.VitShape._fields_][-1] == "pool" and _lib.VitShape().pool == 0


@pytest.mark.parametrize("pool", ["avgmax", "max", "map"])
def test_other_pools_are_refused(pool):
    from cara_amd import cara, create_model
    from cara_amd._lib import CaraError
    with pytest.raises(CaraError, match="global_pool"):
        create_model("vit_base_patch16_224_in21k", depth=1, num_classes=NCLS, global_pool=pool)
    m = _pooled()
    m.global_pool = pool
    with pytest.raises(CaraError):
        cara(_cfg(m))


def test_the_other_mixes_of_pool_and_norms_are_refused():
    from cara_amd import cara
    from cara_amd._lib import CaraError
    with pytest.raises(CaraError, match="global_pool"):
        cara(_cfg(_pooled(fc_norm=False)))                # mean pool behind a live norm, no fc_norm
    m = _pooled()
    m.global_pool = "token"
    with pytest.raises(CaraError, match="fc_norm"):
        cara(_cfg(m))                                     # a live fc_norm on the cls readout
    m = _pooled()
    m.fc_norm = torch.nn.LayerNorm(768, elementwise_affine=False)
    with pytest.raises(CaraError):
        cara(_cfg(m))
    m = _pooled()
    m.fc_norm = torch.nn.LayerNorm(384)
    with pytest.raises(CaraError):
        cara(_cfg(m))


def test_exact_weight_dropout_is_refused_for_a_pooled_model():
    from cara_amd import cara
    from cara_amd._lib import CaraError
    with pytest.raises(CaraError, match="pooled"):
        cara(_cfg(_pooled(), weight_dropout="exact"))
    m = cara(_cfg(_pooled()))
    m._cara_engine.weight_dropout = "exact"               # set behind cara()'s back: refused before anything is ingested or launched
    with pytest.raises(CaraError, match="pooled"):
        m._cara_engine._state(m, 2, IMG, torch.device("cpu"))
    assert m._cara_engine._ingested is None


def test_jax_ingest_and_export_refuse_a_pooled_model(tmp_path):
    from cara_amd import checkpoint
    from cara_amd._lib import CaraError
    m = _pooled()
    with pytest.raises(CaraError, match="encoder_norm"):
        checkpoint.state_dict_to_jax(m)
    with pytest.raises(CaraError, match="encoder_norm"):
        checkpoint.load_jax_npz(m, str(tmp_path / "never_opened.npz"))
    with pytest.raises(CaraError, match="encoder_norm"):
        checkpoint.jax_to_state_dict({}, m)


def test_reset_classifier_never_ignores_a_pool():
    from cara_amd import create_model
    from cara_amd._lib import CaraError
    m = _pooled()
    m.reset_classifier(7)
    m.reset_classifier(4, "")
    m.reset_classifier(3, "avg")
    assert m.head.out_features == 3 and m.global_pool == "avg"
    with pytest.raises(CaraError, match="global_pool"):
        m.reset_classifier(3, "token")
    assert m.head.out_features == 3
    t = create_model("vit_base_patch16_224_in21k", depth=1, num_classes=NCLS)
    t.reset_classifier(2, "token")
    with pytest.raises(CaraError, match="global_pool"):
        t.reset_classifier(2, "avg")


def test_checkpoints_go_through_the_state_dict(tmp_path):
    from cara_amd import cara, recipe
    a, b = cara(_cfg(_pooled())), cara(_cfg(_pooled()))
    with torch.no_grad():
        a.fc_norm.weight.add_(0.25)
        a.fc_norm.bias.add_(0.5)
    path = str(tmp_path / "pooled.pt")
    recipe.save_checkpoint(a, path)
    recipe.load_checkpoint(b, path)
    assert torch.equal(a.fc_norm.weight, b.fc_norm.weight) and torch.equal(a.fc_norm.bias, b.fc_norm.bias)


def test_workspace_size_of_the_token_readout_is_unchanged_and_the_pooled_one_adds_two_rows():
    """on the built library, no GPU: pool = 0 sizes are the parent's by construction (the regions exist only with pool = 1); the
    pooled layouts hold the extra rows in training AND inference form, and the refusals return 0"""
    import ctypes as C
    from cara_amd import _lib
    for operands in ("bf16", "fp16"):
        lib = _lib.lib(operands)
        geom = _lib.Geom(2, 768, 12, 8, 32, 0.1, 4)

        def size(**kw):
            s = _lib.VitShape(3, 96, 16, 3, 37, 5, 1e-6, wd_p=0.1, **kw)
            return int(lib.cara_vit_workspace_bytes(C.byref(geom), C.byref(s)))
        row = (3 * 768 * 4 + 255) // 256 * 256
        assert size(pool=1) == size() + 2 * row and size() > 0
        assert size(pool=1, inference=1) == size(inference=1) + row
        assert size(pool=2) == 0 and size(pool=-1) == 0 and size(pool=1, wd_exact=1) == 0
        assert np.isfinite(size())
