"""Cases, operand families, the fp32 other-order restatement with its slips and the check helpers shared by
tests/test_gemm_model.py (host) and tests/test_gemm_contract_gpu.py (device).  The float64 restatement and its derived terms:
oracle/gemm_model.py; the caps on neighbour cases: tests/tolerances.py (GEMM_CAPS)."""
import math

import torch

from oracle import gemm_model as G
from tests import tolerances as T
from tests.small_kernels_common import tree_sum, share

FAMILIES = ["gaussian", "zero", "outlier", "tiny", "cancel"]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# flags of cara_debug_gemm_plan's out[6]
F_COLSUM, F_ER, F_DV, F_TWOB, F_HALFT, F_RP64, F_HELPERS = 1, 2, 4, 8, 16, 32, 64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Case:
    """One launch: the shape, the epilogue, the operands it takes, and the plan it was written for (family, tile rows, threads,
    nt, flags -- read off gemm_plan() / cara_gemm8_plan(); the device test asserts them before it launches)."""

    def __init__(self, name, family, rows, block, M, N, K, epi, *, Rp=0, rank=0, inside=False, stated=True, b3=False, batch=1, scratch=False,
                 rps=0, bias=True, nt=0, flags=0, gemm8=-1, helpers=-1, riders=None, er=False, dv=None, host=True, Mts=0):
        self.name, self.family, self.rows, self.block = name, family, rows, block
        self.M, self.N, self.K, self.epi = M, N, K, epi
        self.Rp, self.rank, self.inside, self.stated, self.b3, self.batch, self.scratch = Rp, rank or Rp, inside, stated, b3, batch, scratch
        self.rps, self.bias, self.nt, self.flags, self.gemm8, self.helpers = rps, bias and epi != G.EPI_MULH, nt, flags, gemm8, helpers
        self.riders, self.er, self.dv, self.host, self.Mts = riders, er, dv, host, Mts or M
        self.ldc = (N + 7) // 8 * 8 + 8

    def __repr__(self):
        return self.name


B16, F32, GELU, RESID, DGELU, GELU_DG, MULH = G.EPI_BF16, G.EPI_F32, G.EPI_GELU, G.EPI_RESID, G.EPI_DGELU, G.EPI_GELU_DG, G.EPI_MULH
FT, G32, BAT, FEW, T8, T8_256 = G.FAM_FT, G.FAM_G32, G.FAM_BATCHED, G.FAM_FEW_ROWS, G.FAM_TILE8, G.FAM_TILE8_256

CASES = [
    # --- FAM_G32, the 128-row tile: M around one tile and a 16-row MFMA tile, N around the 64-column wave tile and the 8-column
    # store, K / 32 = 2, 4, 6, 10 (both buffer parities; K = 64: one trip of the loop besides the first stage)
    Case("g32_m1", G32, 128, 256, 1, 8, 64, B16),
    Case("g32_m15", G32, 128, 256, 15, 100, 128, F32),
    Case("g32_m16_gelu", G32, 128, 256, 16, 128, 192, GELU),
    Case("g32_m17_resid", G32, 128, 256, 17, 136, 320, RESID, Rp=32, rps=5),
    Case("g32_m127_dgelu", G32, 128, 256, 127, 264, 64, DGELU),
    Case("g32_m128_geludg", G32, 128, 256, 128, 100, 128, GELU_DG),
    Case("g32_m129_mulh", G32, 128, 256, 129, 136, 192, MULH, Rp=64),
    Case("g32_m257_resid", G32, 128, 256, 257, 264, 320, RESID, Rp=64, rps=197),
    Case("g32_m257_b3", G32, 128, 256, 257, 128, 64, B16, Rp=32, b3=True, flags=F_TWOB),
    Case("g32_m129_f32", G32, 128, 256, 129, 264, 128, F32, bias=False),
    Case("g32_k1088_not_few_rows", G32, 128, 256, 17, 300, 1088, GELU, scratch=True),   # 1088 = 17 x 64: no equal slabs, the tile
    # riding products behind the 128-row tiles: nt = 1, 2, 4
    Case("g32_riders_nt1", G32, 128, 256, 160, 136, 128, B16, Rp=32, nt=1, flags=F_COLSUM, riders=(32, 16, True)),
    Case("g32_riders_nt2", G32, 128, 256, 160, 100, 64, DGELU, nt=2, riders=(32, 32, False)),
    Case("g32_riders_nt4", G32, 128, 256, 192, 136, 128, MULH, Rp=64, nt=4, flags=F_COLSUM, riders=(64, 64, True)),
    # --- the 160-row tile (N >= 3072, M > 1024) and the supertile order (tiles_n >= 20)
    Case("g160_m1028_gelu", G32, 160, 256, 1028, 3072, 64, GELU, host=False),
    Case("g160_m1120_f32", G32, 160, 256, 1120, 3080, 64, F32, host=False),
    Case("g160_m1124_dgelu", G32, 160, 256, 1124, 3080, 64, DGELU, host=False),
    Case("g32_tiles_n19", G32, 128, 256, 257, 2432, 64, B16, host=False),
    Case("g32_tiles_n20_ragged_supertile", G32, 128, 256, 257, 2560, 64, B16, host=False),
    Case("g32_epilogue_riders", G32, 128, 256, 1028, 3072, 64, MULH, Rp=32, flags=F_ER, er=True, host=False),
    # --- FAM_FT: the adapter inside
    Case("ft_rank5_half", FT, 128, 256, 129, 100, 64, B16, Rp=32, rank=5, inside=True, flags=F_HALFT),
    Case("ft_rank16_unstated", FT, 128, 256, 197, 384, 192, GELU, Rp=32, rank=16, inside=True, stated=False),
    Case("ft_rank17", FT, 128, 256, 333, 100, 192, RESID, Rp=32, rank=17, inside=True, rps=197),
    Case("ft_rank32", FT, 128, 256, 129, 384, 64, F32, Rp=32, rank=32, inside=True),
    Case("ft_rank33_rp64", FT, 128, 256, 197, 100, 64, DGELU, Rp=64, rank=33, inside=True, flags=F_RP64),
    Case("ft_rank64", FT, 128, 256, 333, 384, 192, B16, Rp=64, rank=64, inside=True, flags=F_RP64),
    Case("ft_riders_nt1", FT, 128, 256, 160, 100, 64, B16, Rp=32, rank=16, inside=True, nt=1, flags=F_HALFT | F_COLSUM, riders=(32, 16, True)),
    Case("ft_riders_nt2", FT, 128, 256, 160, 384, 64, B16, Rp=32, rank=32, inside=True, nt=2, riders=(32, 32, False)),
    Case("ft_riders_nt4", FT, 128, 256, 192, 100, 192, B16, Rp=64, rank=64, inside=True, nt=4, flags=F_RP64 | F_COLSUM, riders=(64, 64, True)),
    # --- FAM_BATCHED
    Case("batched2_f32", BAT, 128, 256, 17, 72, 64, F32, batch=2),
    Case("batched3_bf16", BAT, 128, 256, 130, 72, 64, B16, batch=3),
    # --- FAM_FEW_ROWS (caller scratch, K >= 512): 4 waves up to K = 1024, 8 above; every epilogue
    Case("few_m1", FEW, 16, 256, 1, 16, 512, B16, scratch=True),
    Case("few_m16_f32", FEW, 16, 256, 16, 100, 1024, F32, Rp=32, scratch=True),
    Case("few_m17_gelu", FEW, 16, 512, 17, 300, 1152, GELU, scratch=True),
    Case("few_m64_resid", FEW, 16, 512, 64, 300, 2304, RESID, rps=5, scratch=True),
    Case("few_m128_dgelu", FEW, 16, 512, 128, 16, 1152, DGELU, Rp=64, scratch=True),
    Case("few_m17_geludg", FEW, 16, 256, 17, 100, 512, GELU_DG, scratch=True),
    Case("few_m64_mulh", FEW, 16, 256, 64, 16, 1024, MULH, Rp=32, scratch=True),
    # --- FAM_TILE8 under cara_debug_set_gemm8(160), FAM_TILE8_256 under (256)
    Case("tile8_plain", T8, 160, 512, 1024, 16, 128, B16, gemm8=160, host=False),
    Case("tile8_ext_resid", T8, 160, 512, 1040, 256, 192, RESID, Rp=32, rps=197, gemm8=160, host=False),
    Case("tile8_inside_gelu", T8, 160, 512, 1280, 272, 320, GELU, Rp=32, rank=16, inside=True, flags=F_HALFT, gemm8=160, host=False),
    Case("tile8_helpers", T8, 160, 768, 1040, 272, 128, B16, Rp=32, rank=16, inside=True, flags=F_HALFT | F_HELPERS, gemm8=160, helpers=1, host=False),
    Case("tile8_riders", T8, 160, 512, 1024, 256, 192, DGELU, Rp=32, nt=1, flags=F_COLSUM, gemm8=160, helpers=0, riders=(32, 16, True), Mts=352, host=False),
    Case("tile8_dv_colsum", T8, 160, 512, 1040, 256, 128, B16, Rp=32, flags=F_DV, gemm8=160, dv=True, host=False),
    Case("tile8_dv_inside", T8, 160, 512, 1280, 16, 192, B16, Rp=32, rank=16, inside=True, flags=F_DV | F_HALFT, gemm8=160, dv=False, host=False),
    Case("tile8_256_plain", T8_256, 256, 512, 1024, 256, 128, F32, gemm8=256, host=False),
]
HOST_CASES = [c for c in CASES if c.host]


def row_families(M):
    return [(i + M) % 5 for i in range(M)]


def rider_rows(M, K1, g):
    """The X [M, K1] of a riding product D = X^T G, whose sums run over the ROWS: the same five families by row, (M - 1 - i) % 5 (the
    last row Gaussian) -- Gaussian; all zero; one outlier of 300; tiny (1e-4); cancelling (+-1, the sign alternating from one such
    row to the next, so that they cancel in a column's sum).  Sixteen-bit values of O(1) alone would not do: a bf16 value carries 8
    bits, and 192 of them of like size add EXACTLY in fp32 but for a few in ten thousand, so the column sums would hold nothing for
    the aggregate rule to compare; the tiny rows under the O(1) and the 300s make every addition round."""
    X = torch.randn(M, K1, generator=g)
    for i in range(M):
        f = (M - 1 - i) % 5
        if f == 1:
            X[i] = 0.0
        elif f == 2:
            X[i, (17 * i + 5) % K1] = 300.0
        elif f == 3:
            X[i] *= 1e-4
        elif f == 4:
            X[i] = (1.0 + 2.0 ** -6 * torch.randn(K1, generator=g).round()) * (1.0 - 2.0 * ((i // 5) % 2))
    return X


def operands(c, dt, seed=0):
    """All families in ONE operand pair: row i of A is of family (i + M) % 5 -- Gaussian; all zero; one outlier of 300 among O(1);
    tiny (1e-4); cancelling (+-1 alternating along K: against the columns n % 8 == 1 of B, which are positive and nearly constant,
    |acc| << sum |a b|).  B Gaussian of scale 0.4 / sqrt(K).  The bias puts the columns n % 8 == 5 at u = -6 +- O(1) (the negative
    tail of the GELU) and the columns n % 8 == 2, whose B rows are zero, at exactly 0; the row scale takes 0, 1 and 1 / 0.9 per sample."""
    g = _gen(1000 * seed + 7 * c.M + 3 * c.N + c.K)
    M, N, K = c.M, c.N, c.K
    fam = row_families(M)
    A = torch.randn(c.batch, M, K, generator=g)
    for i, f in enumerate(fam):
        if f == 1:
            A[:, i] = 0.0
        elif f == 2:
            A[:, i, (17 * i + 5) % K] = 300.0
        elif f == 3:
            A[:, i] *= 1e-4
        elif f == 4:
            A[:, i] = (1.0 + 2.0 ** -6 * torch.randn(K, generator=g).round()) * (1.0 - 2.0 * (torch.arange(K) % 2))
    B = torch.randn(c.batch, N, K, generator=g) * (0.4 / math.sqrt(K))
    n = torch.arange(N)
    B[:, n % 8 == 1] = (0.05 * (1.0 + 2.0 ** -6 * torch.randn(int((n % 8 == 1).sum()), K, generator=g).round()))
    B[:, n % 8 == 2] = 0.0
    o = {"fam": fam, "A": A.to(dt), "B": B.to(dt)}
    if c.batch == 1:
        o["A"], o["B"] = o["A"][0], o["B"][0]
    if c.bias:
        b = 0.3 * torch.randn(N, generator=g)
        b[n % 8 == 5] = -6.0
        b[n % 8 == 2] = 0.0
        o["bias"] = b
    if c.Rp:
        B2 = 0.3 * torch.randn(N, c.Rp, generator=g)
        B2[:, c.rank:] = 0
        B2[n % 8 == 2] = 0.0
        o["B2"] = B2.to(dt)
        if c.inside:
            Ut = torch.randn(c.Rp, K, generator=g) * (1.0 / math.sqrt(K))
            Ut[c.rank:] = 0
            o["Ut"] = Ut.to(dt)
        else:
            A2 = torch.randn(M, c.Rp, generator=g)
            A2[:, c.rank:] = 0
            A2[[i for i, f in enumerate(fam) if f == 1]] = 0
            o["A2"] = A2.to(dt)
    if c.b3:
        B3 = torch.randn(N, K, generator=g) * (2.0 ** -9 * 0.4 / math.sqrt(K))     # (a correction below B's 16-bit step)
        B3[n % 8 == 2] = 0.0
        o["B3"] = B3.to(dt)
    if c.epi == RESID:
        o["aux"] = torch.randn(M, N, generator=g)
        ns = (M + c.rps - 1) // c.rps
        o["rowscale"] = torch.tensor([0.0, 1.0, 1.0 / 0.9])[(torch.arange(ns) + 1) % 3]
    elif c.epi == DGELU:   # the saved pre-activation: [-9, 9], the tail band, +0 and -0
        u32 = torch.rand(M, N, generator=g) * 18 - 9
        u32[:, n % 8 == 5] = -3 - 6 * torch.rand(M, int((n % 8 == 5).sum()), generator=g)
        u32[:, n % 8 == 2] = 0.0
        u32[:, n % 16 == 2] = -0.0
        o["aux32"], o["aux"] = u32, u32.to(dt)
    elif c.epi == MULH:    # the saved derivative, IEEE half in both builds, [-0.13, 1.13]
        o["aux"] = (torch.rand(M, N, generator=g) * 1.26 - 0.13).to(torch.float16)
    if c.riders or c.er or c.dv is not None:
        Rp, rank = (c.riders[0], c.riders[1]) if c.riders else (32, 16)
        Mts = c.Mts
        ldg = (Mts + 31) // 32 * 32
        for nm in ("Tt", "Gt"):
            t = torch.zeros(Rp, ldg)
            t[:rank, :Mts] = 0.5 * torch.randn(rank, Mts, generator=g)
            o[nm] = t.to(dt)
        o["Xa"], o["Xb"] = rider_rows(Mts, 128, g).to(dt), rider_rows(Mts, 64, g).to(dt)
        if c.er:
            o["h"] = rider_rows(M, N, g).to(dt)
    return o


# --- fp32 in another order -------------------------------------------------------------------------------------------------
def dot_f32(A, B, lanes=32, budget=1 << 25):
    """fp32 A B^T over the shared last index: `lanes` lanes own contiguous runs of it, add their (exact) products last to first, then
    adjacent lanes pair up (small_kernels_common.tree_sum): the kernels' depth, none of their partial sums"""
    A, B = A.float(), B.float()
    M, Kc = A.shape
    N = B.shape[0]
    run = Kc // lanes
    assert run * lanes == Kc
    Ar, Br = A.view(M, lanes, run), B.view(N, lanes, run)
    out = torch.empty(M, N)
    step = max(1, budget // (N * lanes))
    for r0 in range(0, M, step):
        a = Ar[r0:r0 + step]
        acc = a[:, None, :, run - 1] * Br[None, :, :, run - 1]
        for j in range(run - 2, -1, -1):
            acc = acc + a[:, None, :, j] * Br[None, :, :, j]
        while acc.shape[-1] > 1:
            acc = acc[..., 0::2] + acc[..., 1::2]
        out[r0:r0 + step] = acc[..., 0]
    return out


def _f(c):
    return torch.tensor(c, dtype=torch.float32)


def gelu_f32(u, grad=False, slip=None):
    """gelu_erf / gelu_erf_grad of common.h in fp32 torch operations, unfused"""
    u = u.float()
    if slip == "tanh_gelu" and not grad:
        return 0.5 * u * (1 + torch.tanh(_f(math.sqrt(2 / math.pi)) * (u + _f(0.044715) * u * u * u)))
    au = u.abs()
    t = 1.0 / (1.0 + _f(G.C1) * au)
    e = torch.exp2(u * u * _f(G.C2))
    hp = torch.zeros_like(t)
    for cf in reversed(G.POLY):
        hp = t * (_f(cf) + hp)
    if not grad:
        return u.clamp_min(0) - (au * hp) * e
    half_erf = 0.5 - hp * e
    return (u * _f(G.C3)) * e + (0.5 + torch.copysign(half_erf, u))


def lanes_for(n, want=32):
    while n % want:
        want //= 2
    return want


def restate(c, o, dt, slip=None, lanes=32):
    """The launch in fp32, another order, 16-bit roundings where the kernel has them -> {name: tensor}.  slip: one of SLIPS."""
    outs = {}
    res = []
    for z in range(c.batch):
        A, B = (o["A"][z], o["B"][z]) if c.batch > 1 else (o["A"], o["B"])
        A, B = A.float(), B.float()
        if slip == "drop_last_k":
            A = A.clone()
            A[:, -32:] = 0
        As, Bs = [A], [B]
        if c.b3 and slip != "drop_b3":
            As.append(A)
            Bs.append(o["B3"].float())
        if c.Rp:
            if c.inside:
                T32 = dot_f32(A, o["Ut"].float(), lanes_for(c.K, lanes))
                outs["T"] = T32.to(dt)
                T2 = T32 if slip == "t_fp32" else outs["T"].float()
            else:
                T2 = o["A2"].float()
            if slip == "drop_ext2" and c.Rp == 64:
                T2 = T2.clone()
                T2[:, 32:] = 0
            As.append(T2)
            Bs.append(o["B2"].float())
        Ac, Bc = torch.cat(As, 1), torch.cat(Bs, 1)
        acc = dot_f32(Ac, Bc, lanes_for(Ac.shape[1], lanes))
        bias = o.get("bias")
        u = acc + bias.float() if bias is not None else acc
        epi = c.epi
        if epi == B16:
            C = u.to(dt)
        elif epi == F32:
            C = u
        elif epi in (GELU, GELU_DG):
            C = gelu_f32(u.to(dt).float() if slip == "gelu_of_rounded_u" else u, slip=slip).to(dt)
            outs["C2"] = u.to(dt) if epi == GELU else gelu_f32(u, grad=True).to(torch.float16)
        elif epi == RESID:
            rps = c.rps + 1 if slip == "rowscale_rps_plus_1" else c.rps
            rs = o["rowscale"].float()[(torch.arange(c.M) // rps).clamp_max(len(o["rowscale"]) - 1)][:, None]
            C = (o["aux"] + rs * acc) + bias.float() if (slip == "resid_bias_outside" and bias is not None) else o["aux"] + rs * u
        elif epi == DGELU:
            C = (u * gelu_f32(o["aux32"] if slip == "dgelu_unrounded_u" else o["aux"].float(), grad=True)).to(dt)
        else:
            aux = o["aux"].view(torch.int16).view(torch.bfloat16).float() if slip == "mulh_as_bf16" else o["aux"].float()
            C = (u * aux).to(dt)
        if slip == "last_column" and c.N > 1:
            C = C.clone()
            C[:, -1] = C[:, -2]
        res.append(C)
    outs["C"] = torch.stack(res) if c.batch > 1 else res[0]
    if c.riders:
        Mts = c.Mts
        ln = lanes_for(Mts, lanes)
        outs["Da"] = dot_f32(o["Xa"].float().t().contiguous(), o["Gt"][:, :Mts].float(), ln)
        outs["Db"] = dot_f32(o["Xb"].float().t().contiguous(), o["Tt"][:, :Mts].float(), ln)
        Xb = o["Xb"].float()
        if slip == "colsum_m_minus_1":
            Xb = torch.cat((Xb[:-1], torch.zeros_like(Xb[:1])))
        outs["cs"] = tree_sum(Xb.t().contiguous(), ln)
    return outs


def restate_rider(X, Gt, M, rank=16):
    """D = X^T G and the column sums of X over its first M rows in fp32, another order (the rows padded with zeros to a multiple of 32:
    32 lanes own contiguous runs of rows, last to first, then pair up) -> (D [K1, rank], colsum [K1]): the yardstick of the aggregate
    rule for the products of the epilogue riders and of DV, whose X is an operand or the C the launch wrote"""
    Mp = (M + 31) // 32 * 32
    Xt = torch.zeros(X.shape[1], Mp)
    Xt[:, :M] = X[:M].float().t()
    G_ = torch.zeros(rank, Mp)
    G_[:, :M] = Gt[:rank, :M].float()
    return dot_f32(Xt, G_, 32), tree_sum(Xt, 32)


SLIPS = ["drop_last_k", "drop_ext2", "t_fp32", "resid_bias_outside", "rowscale_rps_plus_1", "tanh_gelu", "gelu_of_rounded_u",
         "dgelu_unrounded_u", "mulh_as_bf16", "last_column", "drop_b3", "colsum_m_minus_1"]


def slip_applies(c, slip):
    return {"drop_ext2": c.Rp == 64, "t_fp32": c.inside, "resid_bias_outside": c.epi == RESID and c.bias, "rowscale_rps_plus_1": c.epi == RESID,
            "tanh_gelu": c.epi in (GELU, GELU_DG), "gelu_of_rounded_u": c.epi in (GELU, GELU_DG), "dgelu_unrounded_u": c.epi == DGELU,
            "mulh_as_bf16": c.epi == MULH, "drop_b3": c.b3, "colsum_m_minus_1": bool(c.riders and c.riders[2])}.get(slip, True)


# --- the float64 model of a case ------------------------------------------------------------------------------------------------
def model(c, o, dt, T_dev=None, z=0):
    """{name: (v, d)} of product z of the case.  T_dev: the T the launch wrote (adapter inside): the extension's operand."""
    A, B = (o["A"][z], o["B"][z]) if c.batch > 1 else (o["A"], o["B"])
    outs = {}
    A2 = o.get("A2")
    if c.inside:
        outs["T"] = G.adapter_T(A, o["Ut"])
        A2 = T_dev
    acc = G.accumulate(A, B, A2, o.get("B2") if c.Rp else None, o.get("B3") if c.b3 else None, family=c.family, block=c.block)
    outs.update(G.epilogue(c.epi, acc, dt, bias=o.get("bias"), aux=o.get("aux"), rowscale=o.get("rowscale"), rows_per_sample=max(c.rps, 1)))
    return outs


def model_riders(c, o):
    k = G.kappa_ts_form("tskinny", c.Mts)
    a, b = G.rider_products(o["Xa"], o["Gt"], c.Mts, k), G.rider_products(o["Xb"], o["Tt"], c.Mts, k)
    return {"Da": a["D"], "Db": b["D"], "cs": b["colsum"]}


# --- the rules ----------------------------------------------------------------------------------------------------------------
def kind(c, name):
    """the output kind a cap is recorded for"""
    if name == "T":
        return "T"
    return {B16: "bf16", GELU: "gelu_h" if name == "C" else "gelu_u", GELU_DG: "gelu_h" if name == "C" else "gelu_dg", DGELU: "dgelu", MULH: "mulh"}[c.epi]


def step16(v, dt):
    """the spacing of the 16-bit grid at |v|: 2^(floor(log2 |v|) - 7) in bf16, - 10 in fp16, the denormal spacing below the normals"""
    bits, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -200))).clamp_min(emin)
    return torch.exp2(e - bits)


def check_16(name, dev, vd, dt, cap, frac=1.0, quiet=False):
    """oracle hold_16; the neighbour share is taken over the elements whose derived term is below A QUARTER of their own 16-bit step --
    where it is not (the cancelling rows, the GELU's negative tail, sums near zero) the interval alone holds the element, as it
    does the offset LayerNorm rows (tests/tolerances.py) -> (inside, worst / bound, share)"""
    v, d = vd
    ok, nb, ratio = G.hold_16(dev, v, d, dt)
    capped = d < 0.25 * step16(v, dt)
    s = share(nb[capped])
    if not quiet:
        print(f"  {name}: worst/bound {ratio:.3f}  neighbours {s:.4f}/{cap} over {int(capped.sum())}/{capped.numel()}")
    # (ONE neighbour case never breaks a cap: in a tensor of 8 elements it is already 12 %)
    # (a cap is in force only over elements it applies to: an output none of whose elements is capped fails here, not silently)
    return bool(ok.all()) and int(capped.sum()) > 0 and (s <= cap * frac or int(nb[capped].sum()) <= 1), ratio, s


def rms(t):
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0


def check_32(name, dev, vd, other, fam=None, quiet=False):
    """hold_f32 element by element, and per row family RMS(dev - v) <= BWD_VS_MODEL_ORDER x RMS(other - v), `other` the fp32
    restatement of the same case in another order -> (inside, worst / bound, worst aggregate ratio)"""
    v, d = vd
    ok, ratio = G.hold_f32(dev, v, d)
    good, worst = bool(ok.all()), 0.0
    if other is not None:
        e_dev, e_oth = G.f64(dev) - v, G.f64(other) - v
        groups = {None: slice(None)} if fam is None else {f: [i for i, g in enumerate(fam) if g == f] for f in sorted(set(fam))}
        for f, idx in groups.items():
            a, b = rms(e_dev[idx]), rms(e_oth[idx])
            r = a / b if b > 0 else (0.0 if a == 0 else float("inf"))
            worst = max(worst, r)
            good &= a <= T.BWD_VS_MODEL_ORDER * b
    if not quiet:
        print(f"  {name}: worst/bound {ratio:.3f}  rms vs other order {worst:.2f} (<= {T.BWD_VS_MODEL_ORDER})")
    return good, ratio, worst


def is16(c, name):
    return G.out_dtype(c.epi, name, torch.bfloat16) != torch.float32 or name == "T"


def holds(c, o, dt, got, other, quiet=True):
    """every output of `got` under its rule -> ({name: (ok, ratio, share or aggregate)})"""
    res = {}
    for z in range(c.batch):
        md = model(c, o, dt, T_dev=got.get("T"), z=z)
        for name, vd in md.items():
            g = got[name][z] if (c.batch > 1 and name != "T") else got[name]
            ot = None if other is None else (other[name][z] if (c.batch > 1 and name != "T") else other[name])
            if is16(c, name):
                odt = torch.float16 if (c.epi == GELU_DG and name == "C2") else dt
                res[name if c.batch == 1 else f"{name}@{z}"] = check_16(name, g, vd, odt, T.GEMM_CAPS[kind(c, name)], quiet=quiet)
            else:
                res[name if c.batch == 1 else f"{name}@{z}"] = check_32(name, g, vd, ot, o["fam"], quiet=quiet)
    if c.riders:
        for name, vd in model_riders(c, o).items():
            if name == "cs" and not c.riders[2]:
                continue
            rk = c.riders[1]
            g, ot = got[name], None if other is None else other[name]
            if name != "cs":
                vd, g, ot = (vd[0][:, :rk], vd[1][:, :rk]), g[:, :rk], None if ot is None else ot[:, :rk]
            res[name] = check_32(name, g, vd, ot, quiet=quiet)
    return res
