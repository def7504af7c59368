"""Host side of the optimiser-side features: that the bound derived in tests/optim_model.py holds for the kernel's own summation
order (its numpy-fp32 restatement against float64: the bound is proved here, without a device, and is not vacuous), and that the
engine's argument validators refuse what they must.  CPU only."""
import math

import numpy as np
import pytest

from cara_amd._lib import CaraError
from cara_amd.engine import CaraEngine
from oracle.small_kernels import U
from tests import optim_model as M


def test_the_path_count_and_the_bound_are_the_documented_ones():
    assert M.CHUNK == 8192 and M.SIZES == (1, 8191, 8192, 8193, 121925)
    assert [M.chunks(n) for n in M.SIZES] == [1, 1, 1, 2, 15]
    assert all(M.additions(n) == 31 + 6 + 3 + 1 + 6 + 3 for n in M.SIZES)
    assert M.additions(256 * 8192 + 1) == 51 and M.additions(2 ** 31) == 49 + 1024
    k = M.additions(1) + 2
    assert M.norm_bound(1) == k * U / (1 - k * U) and M.elem_bound(1) == M.norm_bound(1) + 3 * U
    assert 3.0e-6 < M.norm_bound(M.FLAT_R16_C100) < 3.2e-6          # 52 u: a few fp32 ulps, not a tolerance


@pytest.mark.parametrize("n", M.SIZES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_fp32_restatement_stays_inside_the_derived_bound(n, seed):
    g = M.buffer(n, seed)
    assert 1e-6 * (1 - 1e-6) <= float(np.abs(g).min()) and float(np.abs(g).max()) <= 1e3
    norm64, _, _ = M.clip64(g, 1.0)
    for max_norm in (0.5 * norm64, 2.0 * norm64, math.inf):
        n64, c64, g64 = M.clip64(g, max_norm)
        n32, c32, g32 = M.clip_f32(g, max_norm)
        assert abs(float(n32) - n64) <= M.norm_bound(n) * n64, (n, seed, float(n32), n64)
        assert abs(float(c32) - c64) <= M.elem_bound(n) * c64
        err = np.abs(g32.astype(np.float64) - g64)
        assert bool((err <= np.abs(g.astype(np.float64)) * M.elem_bound(n)).all()), float((err / np.abs(g)).max())
        if max_norm > norm64:
            assert float(c32) == 1.0 and c64 == 1.0 and np.array_equal(g32, g)
        else:
            assert float(c32) < 1.0 and not np.array_equal(g32, g)


def test_the_bound_is_not_vacuous():
    """the restatement's error is a sizeable part of the bound somewhere (or the bound would hold anything), and a summation that
    loses a term -- the last element dropped -- is outside it"""
    n = M.FLAT_R16_C100
    g = M.buffer(n, 3)
    g[-1] = np.float32(0.05) * np.float32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    n64, _, _ = M.clip64(g, math.inf)
    short, _, _ = M.clip_f32(g[:-1], math.inf)
    assert abs(float(short) - n64) > 100 * M.norm_bound(n) * n64
    full, _, _ = M.clip_f32(g, math.inf)
    assert abs(float(full) - n64) <= M.norm_bound(n) * n64


def test_partials_follow_the_element_to_thread_map():
    """one non-zero element per position class: the partial of its chunk alone holds its square"""
    n = 2 * M.CHUNK + 5
    for at in (0, 3, 4, 1023, 1024, M.CHUNK - 1, M.CHUNK, 2 * M.CHUNK + 4):
        g = np.zeros(n, dtype=np.float32)
        g[at] = 3.0
        p = M.partials_f32(g)
        assert p.shape == (3,) and p[at // M.CHUNK] == 9.0 and p.sum() == 9.0
        assert float(M.total_f32(p)) == 9.0


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), -float("inf"), "1", True, [1.0]])
def test_clip_grad_must_be_positive(bad):
    with pytest.raises(CaraError):
        CaraEngine._max_norm(bad)


def test_clip_grad_accepts_none_numbers_and_infinity():
    assert CaraEngine._max_norm(None) is None
    assert CaraEngine._max_norm(1) == 1.0 and CaraEngine._max_norm(0.5) == 0.5 and CaraEngine._max_norm(math.inf) == math.inf


@pytest.mark.parametrize("bad", [(2, 2), (-1, 2), (0, 0), (0,), (0, 1, 2), (0.0, 2), (0, 2.0), "01", 1, (True, 2), (3, 2), (0, -1)])
def test_accumulate_must_be_a_micro_step_of_a_window(bad):
    with pytest.raises(CaraError):
        CaraEngine._window(bad)


def test_accumulate_accepts_none_and_every_micro_step():
    assert CaraEngine._window(None) == (0, 1) and CaraEngine._window((0, 1)) == (0, 1)
    assert [CaraEngine._window((i, 3)) for i in range(3)] == [(0, 3), (1, 3), (2, 3)] and CaraEngine._window([1, 2]) == (1, 2)


def test_fit_refuses_a_window_under_a_graph_and_a_bad_window_length():
    from cara_amd.recipe import fit
    for kw in ({"accum_steps": 2, "graph": True}, {"accum_steps": 0}, {"accum_steps": 1.5}, {"accum_steps": True}):
        with pytest.raises(CaraError):
            fit(None, None, **kw)
