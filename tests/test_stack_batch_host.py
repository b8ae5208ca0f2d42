"""Host logic of the Z-stack batch path (no GPU): how scripts/compute_branches.py groups stacks into batch calls
(tmat_amd/sato.py:chunk_stacks) and how many stacks a pass of tmat_analyze_stack_batch takes (include/tmat.h: the K rule)."""
import numpy as np
import pytest

from tmat_amd import _lib, sato

A, B = ((24, 1024, 1024), 1000.0), ((24, 512, 512), 1000.0)


def test_equal_shape_runs_form_chunks_in_order():
    keys = [A, A, A, B, B, A]
    assert sato.chunk_stacks(keys, [1] * 6) == [[0, 1, 2], [3, 4], [5]]
    assert sato.chunk_stacks([], []) == []
    assert sato.chunk_stacks([A], [1]) == [[0]]


def test_a_unique_shape_stands_alone_and_does_not_join_across():
    keys = [A, B, A, A]
    assert sato.chunk_stacks(keys, [1] * 4) == [[0], [1], [2, 3]]      # the two A runs are not merged: consecutive stacks only


def test_width_in_microns_is_part_of_the_key():
    keys = [A, (A[0], 800.0), A]
    assert sato.chunk_stacks(keys, [1] * 3) == [[0], [1], [2]]


def test_at_most_eight_stacks_per_chunk():
    chunks = sato.chunk_stacks([A] * 19, [1] * 19)
    assert [len(c) for c in chunks] == [8, 8, 3]
    assert [i for c in chunks for i in c] == list(range(19))


def test_the_byte_budget_ends_a_chunk():
    gib = 1 << 30
    assert [len(c) for c in sato.chunk_stacks([A] * 7, [3 * gib] * 7)] == [2, 2, 2, 1]         # 3 x 3 GiB would pass 8 GiB
    assert [len(c) for c in sato.chunk_stacks([A] * 4, [4 * gib] * 4)] == [2, 2]               # exactly the budget still fits
    assert [len(c) for c in sato.chunk_stacks([A] * 3, [9 * gib] * 3)] == [1, 1, 1]            # a stack above the budget goes alone
    assert [len(c) for c in sato.chunk_stacks([A] * 5, [10] * 5, budget=25)] == [2, 2, 1]


def test_order_is_preserved_for_any_mix():
    rs = np.random.RandomState(0)
    keys = [(A, B)[v] for v in rs.randint(0, 2, 60)]
    chunks = sato.chunk_stacks(keys, [1] * 60)
    assert [i for c in chunks for i in c] == list(range(60))
    for c in chunks:
        assert len({keys[i] for i in c}) == 1 and len(c) <= 8
    for c, d in zip(chunks, chunks[1:]):
        assert keys[c[0]] != keys[d[0]] or len(c) == 8                  # a chunk ends only at a key change or when it is full


def test_stacks_per_pass_rule():
    gib = 1 << 30
    assert _lib.STACK_PASS_BUDGET == 8 * gib and _lib.STACK_PASS_MAX == 8
    assert sato.stacks_per_pass(20, 100) == 8                   # the cap
    assert sato.stacks_per_pass(3, 100) == 3                    # n
    assert sato.stacks_per_pass(20, 3 * gib) == 2               # the budget
    assert sato.stacks_per_pass(20, 9 * gib) == 1               # at least one
    assert sato.stacks_per_pass(20, 100, pass_stacks=5) == 5    # the override
    assert sato.stacks_per_pass(3, 100, pass_stacks=5) == 3
    assert sato.stacks_per_pass(20, 9 * gib, pass_stacks=4) == 4


@pytest.mark.parametrize("n,Z,H,W", [(8, 24, 1024, 1024), (20, 24, 2048, 2048), (20, 40, 4096, 4096), (2, 2, 150, 202), (5, 3, 128, 160)])
def test_the_library_plans_by_the_same_rule(n, Z, H, W):
    """tmat_stack_pass_plan (host only): bytes per stack cover at least the blocks that dominate -- the u16 stack and three Z H W f64
    planes (the per-slice gaussian's and the resize's two) -- and K follows the rule from them"""
    k, nbytes = sato.stack_pass_plan(n, Z, H, W)
    assert nbytes >= Z * H * W * (2 + 3 * 8)
    assert nbytes < Z * H * W * (2 + 3 * 8) + 64 * (Z + 40) * 384 * max(384, round(H * 384 / W)) + 3 * H * W + (1 << 22)
    assert k == sato.stacks_per_pass(n, nbytes)
    for ps in (1, 3, 50):
        assert sato.stack_pass_plan(n, Z, H, W, pass_stacks=ps)[0] == min(n, ps)


def test_plan_refuses_bad_geometry():
    for bad in ((0, 3, 64, 64), (2, 1, 64, 64), (2, 3, 1, 64)):
        with pytest.raises(_lib.TmatError):
            sato.stack_pass_plan(*bad)
