"""The GEMM front end's plan (gemm.hip: gemm_plan) without a GPU: cara_debug_gemm_plan answers, from made-up addresses, which kernel
family a cara_gemm_bf16 / cara_gemm_with_tskinny_r call gets, with which tile, grid, block, dynamic LDS and riders -- or the status
that refuses it.  The expected rows (tests/golden/gemm_plan.json) were read off the launch trace of the commit BEFORE the plan
existed: the kernel each call launched there, its grid / block / LDS and its tiles_n / nwg / gm arguments, and what the three query
functions answered.  Headline shape M = 12 608, dim 768, Rp 32, rank 16: a block's four forwards and four dX launches with their
riders, the few-row products at M = 64, rank 64, M = 2 048 (below the tile's 4 096), a batched and a two-B-operand product,
epilogue riders, dVs from the A tiles, and every refusal the plan owns."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan.json")
GOLD = json.load(open(GOLDEN))
CASES = GOLD["cases"]
SETTER_CASES = [(s["set_gemm8"], s["set_helpers"], c) for s in GOLD["setters"] for c in s["cases"]]
POINTERS = ("A2", "B2", "Ut", "T_out", "Tt_out", "Bp", "B3", "scratch", "bias", "aux", "C2", "rowscale", "er_Tt", "er_Gt", "er_h", "er_slabs_v", "er_slabs_u")


def _args(spec):
    """cara_gemm_args from a golden row: integers as given, every pointer the row names a made-up address (never dereferenced)."""
    from cara_amd import _lib
    a = _lib.GemmArgs()
    a.A, a.B, a.C = 0x100000000, 0x200000000, 0x300000000
    for i, name in enumerate(POINTERS):
        if spec.get(name):
            setattr(a, name, 0x400000000 + i * 0x10000000)
    for name, v in spec.items():
        if name not in POINTERS:
            setattr(a, name, v)
    if spec.get("scratch"):
        a.scratch_bytes = _lib.lib().cara_gemm_scratch_bytes()
    if a.batch > 1:
        a.strideA = a.strideB = a.M * a.K
        a.strideC = a.M * a.N
    return a


def test_golden_table_covers_what_the_plan_decides():
    ok = [c for c in CASES if c["status"] == 0]
    assert {c["plan"][0] for c in ok} == {1, 3, 4, 5, 6}          # every family the default policy reaches
    under = [c for _, _, c in SETTER_CASES if c["status"] == 0]
    assert any(c["plan"][0] == 2 and c["plan"][1] == 256 for c in under)     # the yardstick tile: cara_debug_set_gemm8(256)
    assert any(c["plan"][6] & 64 and c["plan"][3] == 768 for c in under)     # helper waves
    assert {c["plan"][1] for c in ok} == {16, 128, 160}
    assert any(c["plan"][6] & 2 for c in ok) and any(c["plan"][6] & 4 for c in ok) and any(c["plan"][6] & 8 for c in ok)
    assert any(c["plan"][6] & 32 for c in ok) and {c["plan"][5] for c in ok} == {0, 1, 2, 4}
    assert sum(1 for c in CASES if c["status"] != 0) >= 20


def _check(lib, case):
    a = _args(case["args"])
    out = (C.c_int * 8)(*([-1] * 8))
    rc = int(lib.cara_debug_gemm_plan(C.byref(a), case["riders_nt"], case["riders_colsum"], out))
    assert rc == case["status"], (rc, list(out))
    if rc == 0:
        assert list(out) == case["plan"], (list(out), case["kernel"])
    else:
        assert list(out) == [-1] * 8            # a refusal writes nothing
    # the queries callers lay memory out by answer as they did
    rd = case["riders"] or {"Rp": 32, "rank": 16}
    assert int(lib.cara_gemm_rider_slab_format(C.byref(a), rd["Rp"], rd["rank"])) == case["slab_format"]
    assert int(lib.cara_gemm_epi_rider_chunks(C.byref(a))) == case["epi_rider_chunks"]
    assert [int(lib.cara_gemm_dv_chunks(C.byref(a), r)) for r in (0, 1)] == case["dv_chunks"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_is_what_the_launch_trace_showed(case):
    from cara_amd import _lib
    _check(_lib.lib(), case)


@pytest.mark.parametrize("gemm8,helpers,case", SETTER_CASES, ids=[f"gemm8={g}-helpers={h}-{c['name']}" for g, h, c in SETTER_CASES])
def test_plan_under_the_debug_setters(gemm8, helpers, case):
    """The rows that change under cara_debug_set_gemm8 (0: never the tile, 160: the tile for all it takes, 256: the yardstick form,
    plain products only) and under helper waves, from the parent's trace under the same setters (tests/conftest.py lets the setters
    take effect).  The overrides are put back whatever happens."""
    from cara_amd import _lib
    lib = _lib.lib()
    assert lib.cara_debug_set_gemm8(gemm8) == 0 and lib.cara_debug_set_gemm8_helpers(helpers if helpers else -1) == 0
    try:
        _check(lib, case)
    finally:
        assert lib.cara_debug_set_gemm8(-1) == 0 and lib.cara_debug_set_gemm8_helpers(-1) == 0


def test_plan_refuses_what_only_the_hook_can_ask():
    """Riders of one column tile beside an adapter inside whose rank is not stated: cara_gemm_with_tskinny_r never asks for that
    (its riders then compute all Rp / 16 tiles), the plan's own check refuses it."""
    from cara_amd import _lib
    spec = next(c for c in CASES if c["name"] == "ut_rank_unstated_riders_all_columns")
    a = _args(spec["args"])
    out = (C.c_int * 8)()
    assert int(_lib.lib().cara_debug_gemm_plan(C.byref(a), 2, 1, out)) == 0 and out[5] == 2 and not out[6] & 16
    assert int(_lib.lib().cara_debug_gemm_plan(C.byref(a), 1, 1, out)) != 0
    assert int(_lib.lib().cara_debug_gemm_plan(None, 0, 0, out)) != 0
