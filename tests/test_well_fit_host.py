"""CPU: host side of the device superellipse search (tmat_amd/well_mask_generation.py): the candidate table against the oracle's own
draw and expressions, and the merge of the device's answer with the candidates the host adjudicates."""
import numpy as np
import pytest
from scipy.special import gamma

from oracle import wellmask as ow
from tmat_amd import well_mask_generation as wm


def _oracle_candidates(seed, num_iters):
    """oracle/wellmask.py:get_superellipse_hull's draw, as that function makes it"""
    w = np.random.RandomState(seed).rand(num_iters, 6)
    pv = (ow.SUPERELLIPSE_BOUNDS[:, 1] - ow.SUPERELLIPSE_BOUNDS[:, 0]) * w + ow.SUPERELLIPSE_BOUNDS[:, 0]
    return pv.T[..., np.newaxis]


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("n", [2, 8, 3])
def test_candidate_table_reproduces_the_oracle_bit_for_bit(seed, n):
    num_iters = 25000
    t, d, s_a, s_b, c_x, c_y = _oracle_candidates(seed, num_iters)
    table = wm.superellipse_table(n, seed, num_iters)
    assert table.shape == (num_iters, 7) and table.dtype == np.float64 and table.flags.c_contiguous
    want = [c_x, c_y, np.cos(t), np.sin(t), d * s_a, d * s_b, 4 * d ** 2 * s_a * s_b * gamma(1 + 1 / n) ** 2 / gamma(1 + 2 / n)]
    for col, ref in enumerate(want):
        assert np.array_equal(table[:, col].view(np.uint64), np.ascontiguousarray(ref[:, 0]).view(np.uint64)), col
    cand = wm.superellipse_candidates(seed, num_iters)
    for key, ref in zip(("t", "d", "s_a", "s_b", "c_x", "c_y"), (t, d, s_a, s_b, c_x, c_y)):
        assert np.array_equal(cand[key], ref), key


@pytest.mark.parametrize("seed", [0, 7])
def test_the_oracles_answer_is_the_tables_smallest_enclosing_row(seed):
    """the table's parameters and areas pick the candidate oracle.wellmask.get_superellipse_hull returns (n = 2: exact on any host)"""
    ang = np.linspace(0, 2 * np.pi, 40, endpoint=False)
    x, y = 0.55 * np.cos(ang) + 0.03, 0.5 * np.sin(ang) - 0.02
    table = wm.superellipse_table(2, seed)
    val = ((x - table[:, 0:1]) / table[:, 4:5]) ** 2 + ((y - table[:, 1:2]) / table[:, 5:6]) ** 2
    ok = np.where(val.max(axis=1) < 1)[0]
    j = ok[np.argmin(table[ok, 6])]
    cand = wm.superellipse_candidates(seed)
    assert tuple(cand[q][j][0] for q in ("t", "d", "s_a", "s_b", "c_x", "c_y")) == ow.get_superellipse_hull(x, y, 2, seed)


def test_merge_band_picks_the_lower_area_then_the_lower_index():
    area = np.array([5.0, 3.0, 4.0, 3.0, 2.0, 9.0])
    assert wm.merge_band(2, [], area) == 2                       # nothing banded: the device's answer
    assert wm.merge_band(2, [5], area) == 2                      # an accepted banded candidate of larger area loses
    assert wm.merge_band(2, [1], area) == 1                      # ... of smaller area wins
    assert wm.merge_band(3, [1], area) == 1                      # equal areas: the lower index, as np.argmin
    assert wm.merge_band(1, [3], area) == 1
    assert wm.merge_band(-1, [5, 0], area) == 0                  # the device found none: the best accepted banded one
    assert wm.merge_band(0, [4, 2, 3], area) == 4
    with pytest.raises(ValueError):
        wm.merge_band(-1, [], area)


def test_banded_candidates_are_judged_by_the_reference_expression():
    """_reference_max on a few rows equals the rows of the oracle's full evaluation"""
    seed, n = 7, 8
    cand = wm.superellipse_candidates(seed)
    t, d, s_a, s_b, c_x, c_y = _oracle_candidates(seed, 25000)
    ang = np.linspace(0, 2 * np.pi, 17, endpoint=False)
    x, y = 0.6 * np.cos(ang), 0.6 * np.sin(ang)
    full = ((((x - c_x) * np.cos(t) - ((y - c_y) * np.sin(t))) / (d * s_a)) ** n + (((x - c_x) * np.sin(t) + (y - c_y) * np.cos(t)) / (d * s_b)) ** n)
    rows = [0, 11, 4097, 24999]
    got = wm._reference_max(cand, rows, x, y, n)
    assert np.allclose(got, full.max(axis=1)[rows], rtol=1e-15, atol=0)
