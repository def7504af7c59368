"""Cases, input families, the fp32 other-order restatements with their slips and the check helpers shared by
tests/test_exact_modes_model.py (host) and tests/test_exact_modes_contract_gpu.py (device).  The float64 models and their derived
terms: oracle/exact_modes_model.py; the caps on neighbour cases: tests/tolerances.py (EXACT_CAPS)."""
import numpy as np
import torch

from oracle import exact_modes_model as E
from tests import tolerances as T
from tests.gemm_common import check_16, check_32, rider_rows, rms

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
S = 0.3
FAMILIES = ["gaussian", "early", "outlier", "zero"]
# cara_materialize_merge / cara_dropout_grad_contract (out, in): one tile; ragged both ways with an odd `in`; in % 4 == 0 with five
# column tiles (reduce_chunks' 4-loop plus a tail) and a last tile 4 wide; in % 4 == 2 (the scalar path) with five row tiles; one row
# and the 16-column thread run plus one
SHAPES = [(64, 64), (65, 63), (130, 260), (260, 130), (1, 17)]
RPS = [32, 64]
RANK = {32: 17, 64: 64}            # the stated rank inside Rp: columns beyond it are zero in U and Vs (the kernels take Rp only)
PS = [0.0, 0.1, 0.3, 0.5, 0.999]   # 0.3: (float)0.3 * 2^24 is the integer 5033165, the double 0.3 * 2^24 floors to 5033164
SEEDS = [11, 0x9E3779B9]
LINS = [5, 46]
NSLABS = [1, 2, 5]
# cara_colsum_bf16 (M, N, ld): one row; one chunk with N % 8 != 0; the halving loop ending at 10 chunks; a second column block of one
# column; ld % 8 != 0 (the scalar path); the policy's last chunk empty (32 chunks of 17 rows: chunk 31 starts at row 527)
COLSUM = [(1, 8, 8), (255, 100, 104), (256, 768, 768), (300, 257, 264), (333, 264, 271), (513, 8, 8)]
COLSUM_EMPTY = (513, 8, 8)
# dense delta (depth, dim, rank); the last: 3 depth = DD_MAXLK, S[] of the finish kernel and the a2 kernel's dynamic LDS both 48 KiB
DD_GEOMS = [(1, 128, 1), (2, 128, 3), (1, 256, 16), (2, 128, 17), (64, 128, 64)]
SLAB_NS = [1, 2, 3, 5, 8]
SLAB_COUNT, SLAB_STRIDE = 777, 1000


def sid(shape):
    return "x".join(str(v) for v in shape)


def runs():
    """every p x seed x linear id once; the family, the slab count and the gap between slabs cycle against them so that every family
    meets several p and both seeds -> [(p, seed, lin, family, nslab, gap)]"""
    out = []
    for ip, p in enumerate(PS):
        for js, seed in enumerate(SEEDS):
            for jl, lin in enumerate(LINS):
                j = 4 * ip + 2 * js + jl
                out.append((p, seed, lin, FAMILIES[(ip + js + 2 * jl) % 4], NSLABS[j % 3], 4 * ((j // 3) % 2) * 3))
    return out


def _gen(*key):
    return torch.Generator().manual_seed(sum((31 ** i) * int(k) for i, k in enumerate(key)) % (2 ** 31))


def draw_linear(out, inn, Rp, family, dt, seed=0):
    """W [out, in] at 2e-2 (W[0, 0] = -0.0), U [in, Rp] at 0.2, Vs [out, Rp] at 5e-2, all 16-bit.  early: Vs at 1e-6 (the state
    tests/test_exact_dropout.py::test_tiny_adapter_survives_next_to_the_frozen_weight describes); outlier: one row of Vs and one of U
    times 300; zero: Vs all zero."""
    g = _gen(out, inn, Rp, FAMILIES.index(family), seed)
    R = RANK[Rp]
    W = 0.02 * torch.randn(out, inn, generator=g)
    W[0, 0] = -0.0
    Um, Vs = torch.zeros(inn, Rp), torch.zeros(out, Rp)
    Um[:, :R] = 0.2 * torch.randn(inn, R, generator=g)
    Vs[:, :R] = 0.05 * torch.randn(out, R, generator=g)
    if family == "early":
        Vs *= 2e-5
    elif family == "outlier":
        Vs[out // 2] *= 300.0
        Um[inn // 3] *= 300.0
    elif family == "zero":
        Vs.zero_()
    return W.to(dt), Um.to(dt), Vs.to(dt)


def draw_slabs(out, inn, nslab, family, seed=0):
    """the split-K partials of dW, fp32 [nslab, out, in]: slab z at 2^-z (every addition of slabs rounds); outlier: one row times 300"""
    g = _gen(out, inn, nslab, FAMILIES.index(family), seed, 7)
    x = torch.randn(nslab, out, inn, generator=g) * (2.0 ** -torch.arange(nslab).float())[:, None, None]
    if family == "outlier":
        x[:, out // 2] *= 300.0
    return x.contiguous()


def draw_colsum(M, N, dt):
    """gemm_common.rider_rows: Gaussian, zero, outlier, tiny and cancelling rows, so that the additions round"""
    return rider_rows(M, N, _gen(M, N, 3)).to(dt)


def draw_dd(geom, early=False):
    """A1 [3 depth, R] O(1), A2 [dim^2, R] at 0.1 (early: 1e-6, the zero-initialised factor's first steps), R1 about 1, dD
    [depth, 3, dim, dim] Gaussian with ONE entry of the last layer at 1e4 -- an element-wise bound on dA2 / dA1 matters next to it"""
    depth, dim, R = geom
    g = _gen(depth, dim, R, int(early))
    A1 = torch.randn(3 * depth, R, generator=g)
    A2 = (1e-6 if early else 0.1) * torch.randn(dim * dim, R, generator=g)
    R1 = 1.0 + 0.2 * torch.randn(R, generator=g)
    dD = torch.randn(depth, 3, dim, dim, generator=g)
    dD[depth - 1, 1, dim // 2, 5] = 1.0e4
    return A1, A2, R1, dD


# --- fp32 in another order --------------------------------------------------------------------------------------------------
def run_sum(term, n, run, order="A"):
    """fp32 sum of term(0) .. term(n - 1) (arrays of one shape): contiguous runs of `run` indices, each added last to first, then
    adjacent runs pair up -- the kernels' depth, none of their partial sums.  order "B" (the yardstick of the aggregate rule's host
    proof): the runs are cut from the END of the range, each is added first to last from its second index on with its first index
    last, and the runs pair up from the end -- the same depth again, none of order A's partial sums"""
    run = max(int(run), 1)
    pieces = []
    if order == "A":
        for a in range(0, n, run):
            b = min(n, a + run)
            acc = term(b - 1)
            for j in range(b - 2, a - 1, -1):
                acc = acc + term(j)
            pieces.append(acc)
    else:
        for b in range(n, 0, -run):
            a = max(0, b - run)
            acc = term(a + 1) if b - a > 1 else term(a)
            for j in range(a + 2, b):
                acc = acc + term(j)
            pieces.append(acc + term(a) if b - a > 1 else acc)
    while len(pieces) > 1:
        pieces = [pieces[i] + pieces[i + 1] if i + 1 < len(pieces) else pieces[i] for i in range(0, len(pieces), 2)]
    assert pieces[0].dtype == np.float32
    return pieces[0]


def _mask(out, inn, p, seed, lin, slip):
    if slip == "mask_lin_plus_1":
        lin += 1
    if slip == "mask_index_transposed":                 # (15) i * out + o instead of o * in + i
        return E.keep(inn, out, p, seed, lin).t().numpy()
    return E.keep(out, inn, p, seed, lin).numpy()


def _scale(p, slip):
    return np.float32(1.0) if slip == "inv_keep_left_out" else np.float32(E.mask_params(p)[1])


def restate_merge(W, Um, Vs, p, seed, lin, dt, with_w, slip=None, order="A"):
    """cara_materialize_merge in fp32 numpy: the rank sum in runs added last to first, the 16-bit rounding where the kernel has it"""
    u, vs, w = Um.float().numpy(), Vs.float().numpy(), W.float().numpy()
    out, inn, Rp = vs.shape[0], u.shape[0], u.shape[1]
    if slip == "ragged_tile_neighbour_U" and inn % 64 and inn > 64:
        src = np.arange(inn)
        src[inn // 64 * 64:] -= 64
        u = u[src]
    d = run_sum(lambda r: vs[:, r, None] * u[None, :, r], Rp, Rp, order)
    x = np.where(_mask(out, inn, p, seed, lin, slip), d * _scale(p, slip), np.float32(0))
    assert x.dtype == np.float32
    if with_w:
        return torch.from_numpy(w + x).to(dt)
    if slip == "Dm_rounded_next_to_W":                 # the precision loss the mode exists to avoid
        return torch.from_numpy(torch.from_numpy(w + x).to(dt).float().numpy() - w).to(dt)
    return torch.from_numpy(x).to(dt)


def restate_contract(slabs, Um, Vs, p, seed, lin, slip=None, order="A"):
    """cara_dropout_grad_contract in fp32 numpy: slabs last to first, the mask, then 64-index runs (32 in order B) of rounded products
    added last to first and paired up -> {"dVs", "dU"}"""
    x, u, vs = slabs.numpy(), Um.float().numpy(), Vs.float().numpy()
    nslab, out, inn = x.shape
    n = nslab - 1 if (slip == "last_slab_not_summed" and nslab > 1) else nslab
    g = run_sum(lambda z: x[z], n, n, order)
    g = g * np.where(_mask(out, inn, p, seed, lin, slip), _scale(p, slip), np.float32(0))
    if slip == "ragged_last_column_dropped" and inn % 64:   # (16)
        g = g.copy()
        g[:, inn - 1] = 0
    assert g.dtype == np.float32
    dVs = run_sum(lambda i: g[:, i, None] * u[None, i, :], inn, 64, order)
    dU = run_sum(lambda o: g[o, :, None] * vs[None, o, :], out, 64, order)
    return {"dVs": torch.from_numpy(dVs), "dU": torch.from_numpy(dU)}


def restate_colsum(X, M, N, slip=None, order="A"):
    """cara_colsum_bf16 in fp32 numpy: runs as long as a lane's chain under the restated policy, last to first, paired up"""
    x = X.float().numpy()[:M, :N]
    rows = M - 1 if slip == "colsum_m_minus_1" else M     # (17)
    if rows == 0:
        return torch.zeros(N)
    per = -(-M // E.colsum_chunks(M, N))
    return torch.from_numpy(run_sum(lambda m: x[m], rows, -(-per // 8) + 4, order))


def restate_dd_materialize(A1, A2, R1, s, dim, dt, slip=None, order="A"):
    """cara_dense_delta_materialize in fp32 numpy: the coefficient associated the other way round ((A1 R1) s), the rank sum last
    to first -> (Dm [depth, 3 dim, dim], Dmt [depth, dim, 3 dim])"""
    a1, a2, r1 = A1.numpy(), A2.numpy(), R1.numpy()
    depth, R = a1.shape[0] // 3, a1.shape[1]
    coef = (a1 * r1) * np.float32(s)
    t = run_sum(lambda r: coef[:, r, None] * a2[None, :, r], R, R, order)             # [nlk, P], p = e dim + o
    t16 = torch.from_numpy(t).to(dt).reshape(depth, 3, dim, dim)
    Dm = t16.permute(0, 1, 3, 2).reshape(depth, 3 * dim, dim).contiguous()
    if slip == "Dmt_untransposed_per_k":
        Dmt = t16.permute(0, 3, 1, 2).reshape(depth, dim, 3 * dim).contiguous()                # [l][o][k dim + e]
    else:
        Dmt = Dm.transpose(1, 2).contiguous()
    return Dm, Dmt


def _tree(x, run, order="A"):
    """fp32 sum over axis 1 of x [n, P, R]: runs of `run` last to first (order B: first to last, the runs offset by half a run around
    the end of the range), then adjacent runs pair up"""
    n, P, R = x.shape
    if order == "B":
        x = np.roll(x, run // 2, axis=1)
    x = x.reshape(n, P // run, run, R)
    js = list(range(run - 1, -1, -1)) if order == "A" else list(range(run))
    acc = x[:, :, js[0]]
    for j in js[1:]:
        acc = acc + x[:, :, j]
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    return acc[:, 0]


def restate_dd_grad(A1, A2, R1, dD, s, dim, slip=None, order="A"):
    """cara_dense_delta_grad in fp32 numpy: dA2's (layer, projection) sum last to first with c = (A1 R1) s; S over runs of 16 rows
    (8 in order B), last to first, paired up; the final factors the other way round -> {"A2", "A1", "R1"}"""
    a1, a2, r1 = A1.numpy(), A2.numpy(), R1.numpy()
    nlk, R = a1.shape
    P = dim * dim
    dd = dD.numpy().reshape(nlk, P)
    s = np.float32(s)
    c = (a1 * r1) * s
    out = {"A2": run_sum(lambda lk: dd[lk, :, None] * c[lk, None, :], nlk, nlk, order)}
    ds = dd
    if slip == "finish_drops_last_chunk":               # (14)
        ds = dd.copy()
        ds[:, P - 256:] = 0
    S = np.concatenate([_tree(ds[a:a + 8, :, None] * a2[None], 16, order) for a in range(0, nlk, 8)])   # [nlk, R]
    out["A1"] = (S * s) if slip == "dA1_without_R1" else (S * r1) * s
    n1 = nlk // 3 if slip == "dR1_over_depth" else nlk
    out["R1"] = run_sum(lambda lk: a1[lk] * S[lk], n1, nlk, order) * s
    for v in out.values():
        assert v.dtype == np.float32
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


# slips 14 .. 17 are the ones docs/findings/adapter_contract.md lists as "not evaluated"
SLIPS = ["finish_drops_last_chunk", "mask_index_transposed", "ragged_last_column_dropped", "colsum_m_minus_1", "inv_keep_left_out",
         "mask_lin_plus_1", "last_slab_not_summed", "Dm_rounded_next_to_W", "dA1_without_R1", "dR1_over_depth", "Dmt_untransposed_per_k",
         "ragged_tile_neighbour_U"]
SLIP_KERNELS = {"finish_drops_last_chunk": ("dd_grad",), "mask_index_transposed": ("merge", "contract"), "ragged_last_column_dropped": ("contract",),
                "colsum_m_minus_1": ("colsum",), "inv_keep_left_out": ("merge", "contract"), "mask_lin_plus_1": ("merge", "contract"),
                "last_slab_not_summed": ("contract",), "Dm_rounded_next_to_W": ("merge",), "dA1_without_R1": ("dd_grad",),
                "dR1_over_depth": ("dd_grad",), "Dmt_untransposed_per_k": ("dd_materialize",), "ragged_tile_neighbour_U": ("merge",)}


# --- the rules ----------------------------------------------------------------------------------------------------------------
def holds_merge(name, got, model, dt, with_w, frac=1.0, quiet=True):
    """hold_16 and the cap of its kind; without W every dropped element is +0 in bits -> (ok, worst / bound, share)"""
    v, d, keep = model
    ok, ratio, used = check_16(name, got, (v, d), dt, T.EXACT_CAPS["merge_Weff" if with_w else "merge_Dm"], frac=frac, quiet=quiet)
    if not with_w:
        ok = ok and bool((got.cpu().contiguous().view(torch.int16)[~keep] == 0).all())
    return ok, ratio, used


def holds_dd_materialize(got, model, dt, frac=1.0, quiet=True):
    Dm, Dmt = got
    ok, ratio, used = check_16("dd_Dm", Dm, model, dt, T.EXACT_CAPS["dd_Dm"], frac=frac, quiet=quiet)
    same = torch.equal(Dmt.cpu().contiguous().view(torch.int16), Dm.cpu().transpose(1, 2).contiguous().view(torch.int16))
    return ok and same, ratio, used


# The aggregate rule compares two RMS errors.  Over n elements with independent errors of one size their ratio scatters like the
# root of an F(n, n) variable: at n = 256 a factor BWD_VS_MODEL_ORDER = 4 is thirty standard deviations of log-ratio away, at n = 3
# (dA1 of the geometry (1, 128, 1)) two correct orders are 10 apart on the host.  So a group of fewer than AGG_MIN elements is held
# element by element only, and rows that carry an outlier (whose few errors would be the whole RMS of their tensor) form a group
# of their own.  AGG_MIN comes from that reasoning, not from a device.
AGG_MIN = 256


def outlier_rows(kind, shape=None, geom=None, family=None):
    """first-axis indices of the output rows dominated by the inputs' one outlier: dVs row out // 2 (the slabs' and Vs' row), dU row
    in // 3 (U's row) in the outlier family; dA2's row of the 1e4 entry of dD and dA1's (layer, projection) row of it"""
    if kind in ("dVs", "dU"):
        return [] if family != "outlier" else [shape[0] // 2 if kind == "dVs" else shape[1] // 3]
    depth, dim, _ = geom
    return {"A2": [(dim // 2) * dim + 5], "A1": [3 * (depth - 1) + 1]}.get(kind, [])


def holds_f32(model, got, other, rows=None, quiet=True):
    """hold_f32 on every element (gemm_common.check_32) and its aggregate rule -- RMS(got - v) <= BWD_VS_MODEL_ORDER x RMS(other - v)
    -- per group of at least AGG_MIN elements: the rows named in rows[name], and the rest -> {name: (ok, worst / bound, aggregate)}"""
    res = {}
    for name, (v, d) in model.items():
        ok, ratio, _ = check_32(name, got[name], (v, d), None, quiet=True)
        worst = 0.0
        if other is not None:
            e_got, e_oth = E.f64(got[name]) - v, E.f64(other[name]) - v
            mark = torch.zeros(v.shape[0], dtype=torch.bool)
            mark[(rows or {}).get(name, [])] = True
            for idx in (mark, ~mark):
                if e_got[idx].numel() >= AGG_MIN:
                    a, b = rms(e_got[idx]), rms(e_oth[idx])
                    r = a / b if b > 0 else (0.0 if a == 0 else float("inf"))
                    worst = max(worst, r)
                    ok &= a <= T.BWD_VS_MODEL_ORDER * b
        if not quiet:
            print(f"  {name}: worst/bound {ratio:.3f}  rms vs other order {worst:.2f} (<= {T.BWD_VS_MODEL_ORDER})")
        res[name] = (ok, ratio, worst)
    return res
