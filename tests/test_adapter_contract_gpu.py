"""The adapter-side kernels of factors.hip on the device, in both operand builds, held to the derived bounds of
oracle/adapter_model.py (proven attainable on the host by tests/test_adapter_model.py, whose inputs and float64 models are shared
here).  cara_factor_prep: every entry of every layer of the pack -- copies bitwise, products under the interval rule and the cap of
tests/tolerances.py (ADAPTER_CAPS), padding columns exactly zero, each transposed copy bitwise the transpose, the bytes between the
last bias and layer_stride and a guard after `total` untouched.  cara_factor_grad_reduce: every element of every tensor the order
writes under hold_f32 with NaN in the inputs' padding columns, outputs and scratch pre-filled with NaN, guards after each of them,
the tensors an order does not write untouched, two calls the same bits.  cara_factor_grad_reduce_ex: the loss scale and the
found-inf word.  Refusals return CARA_E_ARG and write nothing.  Figures are printed (-s) before they are asserted;
docs/findings/adapter_contract.md holds the tables."""
import ctypes as C

import pytest
import torch

from oracle import adapter_model as A
from tests import adapter_common as S
from tests.test_adapter_model import DRAWS, GRAD_RUNS, grad_model, inputs, prep_model
from tests.test_kernels_gpu import DEV, L
from tests.test_small_kernels_gpu import GUARD, is_sentinel, sentinel

pytestmark = pytest.mark.gpu

OPERANDS = ["bf16", "fp16"]
NAN_BITS = 0x7FC00000
PATTERN = 0xA5          # the pack's pre-fill: 0xA5A5 is a finite value in bf16 and in fp16
PACK_GUARD = 4096
E_ARG = 1


def _geom(geom, **over):
    f = dict(depth=geom[0], dim=geom[1], heads=geom[2], rank=geom[3], Rp=geom[4], scale=S.S, cp_length=geom[5])
    f.update(over)
    return L().Geom(**f)


def _dev(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def _ptrs(struct, tensors, **over):
    f = {k: L().ptr(v) for k, v in tensors.items()}
    f.update(over)
    return struct(**f)


def _nan_guarded(n):
    """n NaNs followed by GUARD sentinel words -> (whole allocation, the first n)"""
    full = sentinel((n + GUARD,), torch.float32)
    full[:n] = float("nan")
    return full, full[:n]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _untouched(t):
    return bool((_bits(t) == NAN_BITS).all())


# --- cara_factor_prep -------------------------------------------------------------------------------------------------------
def run_prep(lib, geom, cp, bias, dt):
    """-> (restate_prep's layout read back from the pack, layout, the whole buffer on the host)"""
    Ld, dim, H, R, Rp, order = geom
    g, lay = _geom(geom), L().PackLayout()
    assert lib.cara_pack_offsets(C.byref(g), C.byref(lay)) == 0
    assert lay.layer_stride % 256 == 0 and lay.total == lay.layer_stride * Ld
    buf = torch.full((lay.total + PACK_GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    cpd, bd = _dev(cp), [b.to(DEV).contiguous() for b in bias]
    p = L().ptr
    L().check(lib.cara_factor_prep(C.byref(g), C.byref(_ptrs(L().CpPtrs, cpd)), p(bd[0]), p(bd[1]), p(bd[2]), p(buf), L().stream()), "cara_factor_prep")
    torch.cuda.synchronize()
    host = buf.cpu()
    layers = host[:lay.total].view(Ld, lay.layer_stride)
    got = {}
    for name in A.MATS:
        rows = A.mat_rows(name, dim)
        tname = name.replace("U_", "Ut_").replace("Vs_", "Vst_")
        for key, off, shape in ((name, getattr(lay, name), (Ld, rows, Rp)), (name + "_t", getattr(lay, tname), (Ld, Rp, rows))):
            got[key] = layers[:, off:off + rows * Rp * 2].contiguous().view(dt).reshape(shape)
    for name, n in (("bias_proj", dim), ("bias_fc1", 4 * dim), ("bias_fc2", dim)):
        off = getattr(lay, name)
        got[name] = layers[:, off:off + 4 * n].contiguous().view(torch.float32).reshape(Ld, n)
    return got, lay, host


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("geom", S.GEOMS, ids=S.gid)
def test_factor_prep(geom, operands):
    lib, dt = L().lib(operands), L().act_dtype(operands)
    Ld, dim, H, R, Rp, order = geom
    for early in DRAWS:
        cp, bias = inputs(geom, early)
        got, lay, host = run_prep(lib, geom, cp, bias, dt)
        print(f"\n{S.gid(geom)} {operands} early={early}")
        res = S.holds_prep(geom, prep_model(geom, early), got, dt, quiet=False)
        end = lay.bias_fc2 + 4 * dim
        gap_ok = bool((host[:lay.total].view(Ld, lay.layer_stride)[:, end:] == PATTERN).all())
        guard_ok = bool((host[lay.total:] == PATTERN).all())
        print(f"  gap {lay.layer_stride - end} bytes intact {gap_ok}  guard intact {guard_ok}  biases worst/bound "
              + " ".join(f"{res[b][1]:.3f}" for b in ("bias_proj", "bias_fc1", "bias_fc2")))
        for name, (ok, ratio, used) in res.items():
            assert ok, f"{name}: outside its rule (worst/bound {ratio:.3f}, share {used})"
        assert gap_ok and guard_ok
        if order == 2:
            for name in ("U_qkv", "Vs_qkv", "U_qkv_t", "Vs_qkv_t"):
                assert bool((got[name].view(torch.int16) == 0).all()), name


# --- cara_factor_grad_reduce(_ex) --------------------------------------------------------------------------------------------
class Grad:
    """one geometry's arguments on the device: the CP tensors, a set of layer gradients, NaN-filled guarded outputs and scratch"""

    def __init__(self, lib, geom, cp, lg):
        self.lib, self.geom = lib, geom
        Ld, dim, H, R, Rp, order = geom
        self.g = _geom(geom)
        self.cpd, self.lgd = _dev({k: v for k, v in cp.items() if k in A.cp_names(order)}), _dev(lg)
        shapes = S.cp_shapes(geom)
        if order == 3:
            shapes["A4"] = (dim // H, R)      # no fourth factor at order 3: handed over to see that it is left alone
        self.written = set(A.kappa_grad(geom))
        self.shapes = shapes
        self.nscratch = int(lib.cara_factor_grad_scratch_bytes(C.byref(self.g))) // 4
        assert self.nscratch > 0
        self.fresh()

    def fresh(self):
        self.full, self.out = {}, {}
        for name, shape in self.shapes.items():
            n = 1
            for d in shape:
                n *= d
            self.full[name], flat = _nan_guarded(n)
            self.out[name] = flat.view(*shape)
        self.scratch_full, self.scratch = _nan_guarded(self.nscratch)

    def call(self, loss_scale=None, found=None, ex=False, lgd=None):
        p = L().ptr
        cps, gps, lgs = _ptrs(L().CpPtrs, self.cpd), _ptrs(L().CpPtrs, self.out), _ptrs(L().LayerGrads, lgd or self.lgd)
        if ex or loss_scale is not None or found is not None:
            rc = self.lib.cara_factor_grad_reduce_ex(C.byref(self.g), C.byref(cps), C.byref(lgs), C.byref(gps), p(self.scratch), p(loss_scale), p(found), L().stream())
        else:
            rc = self.lib.cara_factor_grad_reduce(C.byref(self.g), C.byref(cps), C.byref(lgs), C.byref(gps), p(self.scratch), L().stream())
        L().check(rc, "cara_factor_grad_reduce")
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in self.out.items() if k in self.written}

    def guards_intact(self):
        n = len(self.scratch)
        return is_sentinel(self.scratch_full[n:]) and all(is_sentinel(f[self.out[k].numel():]) for k, f in self.full.items())

    def unwritten_untouched(self):
        return all(_untouched(v) for k, v in self.out.items() if k not in self.written)


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("geom", S.GEOMS, ids=S.gid)
def test_factor_grad_reduce(geom, operands):
    lib = L().lib(operands)
    order = geom[5]
    for early, family in GRAD_RUNS:
        cp, _ = inputs(geom, early)
        lg, model = grad_model(geom, early, family)
        run = Grad(lib, geom, cp, lg)
        assert set(run.out) - run.written == {2: {"A1", "A2"}, 3: {"A4"}}.get(order, set())
        got = run.call()
        res = S.holds_grad(model, got)
        intact, alone = run.guards_intact(), run.unwritten_untouched()
        print(f"\n{S.gid(geom)} {operands} early={early} {family}: guards intact {intact}, unwritten untouched {alone}\n  "
              + "  ".join(f"{k} {r:.3f}" for k, (_, r) in res.items()))
        for name, (ok, ratio) in res.items():
            assert ok, f"{name} ({family}, early={early}): worst/bound {ratio:.3f}"
        assert intact and alone
        if order == 2:   # written as zero: cara_dense_delta_grad runs after this kernel and overwrites it with the order-2 gradient
            assert bool((_bits(got["R1"]) == 0).all())
        run.fresh()
        again = run.call()
        for name in got:
            assert torch.equal(_bits(got[name]), _bits(again[name])), f"{name}: two calls differ"


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("geom", S.EX_GEOMS, ids=S.gid)
def test_factor_grad_reduce_ex(geom, operands):
    lib = L().lib(operands)
    Ld, dim, H, R, Rp, order = geom
    cp, _ = inputs(geom, False)
    lg, _ = grad_model(geom, False, "gaussian")
    run = Grad(lib, geom, cp, lg)
    plain = run.call()
    word = lambda v: torch.tensor([v], dtype=torch.float32, device=DEV)   # noqa: E731

    # a power of two: bitwise 2^-k times the plain call; the word stays as it was on finite inputs
    for k, preset in ((10, 0.0), (16, 1.0)):
        run.fresh()
        found = word(preset)
        got = run.call(word(2.0 ** k), found)
        for name in plain:
            assert torch.equal(_bits(got[name]), _bits(plain[name] * 2.0 ** -k)), (name, k)
        assert float(found) == preset and run.guards_intact() and run.unwritten_untouched()
    # 1000: the bound grown by 2u |v|; no word
    run.fresh()
    _, model = grad_model(geom, False, "gaussian", 1000.0)
    res = S.holds_grad(model, run.call(word(1000.0), None))
    print(f"\n{S.gid(geom)} {operands} loss scale 1000: " + "  ".join(f"{k} {r:.3f}" for k, (_, r) in res.items()))
    for name, (ok, ratio) in res.items():
        assert ok, f"{name}: worst/bound {ratio:.3f}"
    # neither: the plain call's bits
    run.fresh()
    got = run.call(ex=True)
    assert all(torch.equal(_bits(got[n]), _bits(plain[n])) for n in plain)

    def raised(name, index, value):
        t = run.lgd[name].clone()
        t[index] = value
        found = word(0.0)
        run.call(word(1.0), found, lgd={**run.lgd, name: t})
        return float(found)
    # one Inf in a live element of each input tensor in turn (the last layer's last row and column) raises the word to exactly 1
    for name in A.LG_FIELDS:
        index = (Ld - 1, -1, R - 1) if run.lgd[name].dim() == 3 else (Ld - 1, -1)
        want = 0.0 if (order == 2 and name in ("dU_qkv", "dVs_qkv")) else 1.0   # order 2 reads neither (dense_delta.hip does)
        assert raised(name, index, float("inf")) == want, name
    assert raised("dVs_fc1", (0, 0, 0), float("nan")) == 1.0
    assert raised("dc_fc1", (0, 3), -float("inf")) == 1.0
    if R < Rp:   # the padding is not read (it already holds NaN in every run above, with the word left at 0)
        assert raised("dU_proj", (0, 0, R), float("inf")) == 0.0 and raised("dVs_fc2", (Ld - 1, -1, Rp - 1), float("inf")) == 0.0
    # finite inputs, a result beyond 3e38: dP3[0, 0] = 1.6e38 + 1.6e38 + O(1)
    t = run.lgd["dU_proj"].clone()
    t[0, 0, 0] = t[1, 0, 0] = 1.6e38
    found = word(0.0)
    got = run.call(word(1.0), found, lgd={**run.lgd, "dU_proj": t})
    assert float(found) == 1.0 and bool(torch.isfinite(got["P3"]).all()) and float(got["P3"][0, 0]) > 3.0e38


# --- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", OPERANDS)
def test_refusals_return_e_arg_and_write_nothing(operands):
    lib = L().lib(operands)
    geom = S.GEOMS[1]                     # (3, 64, 16, 3, 32, 4): every refused variant asks for no more memory than this one has
    cp, bias = inputs(geom, False)
    lg, _ = grad_model(geom, False, "gaussian")
    run = Grad(lib, geom, cp, lg)
    p, st = L().ptr, L().stream
    lay = L().PackLayout()
    assert lib.cara_pack_offsets(C.byref(run.g), C.byref(lay)) == 0
    pack = torch.full((lay.total,), PATTERN, dtype=torch.uint8, device=DEV)
    bd = [b.to(DEV).contiguous() for b in bias]
    cps, gps, lgs = _ptrs(L().CpPtrs, run.cpd), _ptrs(L().CpPtrs, run.out), _ptrs(L().LayerGrads, run.lgd)

    def refused(g=None, cps_=None, lgs_=None, gps_=None, scratch=True, prep=True):
        g = g or run.g
        rc = [lib.cara_factor_grad_reduce(C.byref(g), C.byref(cps_ or cps), C.byref(lgs_ or lgs), C.byref(gps_ or gps), p(run.scratch) if scratch else None, st()),
              lib.cara_factor_grad_reduce_ex(C.byref(g), C.byref(cps_ or cps), C.byref(lgs_ or lgs), C.byref(gps_ or gps), p(run.scratch) if scratch else None, None, None, st())]
        if prep:
            rc.append(lib.cara_factor_prep(C.byref(g), C.byref(cps_ or cps), p(bd[0]), p(bd[1]), p(bd[2]), p(pack), st()))
        return all(r == E_ARG for r in rc)
    bad_geoms = {"dim % 8": dict(dim=60, heads=4), "dim % heads": dict(heads=5), "rank > Rp": dict(rank=33), "Rp 48": dict(Rp=48),
                 "order 1": dict(cp_length=1), "order 6": dict(cp_length=6)}
    for what, over in bad_geoms.items():
        g = _geom(geom, **over)
        assert refused(g), what
        assert lib.cara_pack_offsets(C.byref(g), C.byref(L().PackLayout())) == E_ARG, what
        assert int(lib.cara_factor_grad_scratch_bytes(C.byref(g))) == 0, what
    assert refused(cps_=_ptrs(L().CpPtrs, run.cpd, A3=None)), "A3 missing at order 4"
    assert refused(gps_=_ptrs(L().CpPtrs, run.out, A3=None), prep=False), "A3's gradient missing at order 4"
    assert refused(_geom(geom, cp_length=5), cps_=_ptrs(L().CpPtrs, run.cpd, A5=None)), "A5 missing at order 5"
    for name in A.LG_FIELDS:
        assert refused(lgs_=_ptrs(L().LayerGrads, run.lgd, **{name: None}), prep=False), name
    assert refused(scratch=False, prep=False), "NULL scratch"
    assert lib.cara_factor_prep(C.byref(run.g), C.byref(cps), p(bd[0]), p(bd[1]), p(bd[2]), None, st()) == E_ARG
    assert lib.cara_factor_prep(C.byref(run.g), C.byref(cps), None, p(bd[1]), p(bd[2]), p(pack), st()) == E_ARG
    torch.cuda.synchronize()
    assert all(_untouched(v) for v in run.out.values()) and _untouched(run.scratch) and run.guards_intact()
    assert bool((pack == PATTERN).all())
    # ... and the same arguments are taken once nothing is wrong with them
    assert set(run.call()) == run.written
