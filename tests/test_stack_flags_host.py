"""Host-only checks of what the Z-stack batch path gained for --detect-well and --tree-visualizations: the small-shape rule of the well
front end, the two sizes of tmat_stack_opts, the chunk accounting of compute_branches.py."""
import ctypes as C

import numpy as np
import pytest


@pytest.mark.parametrize("shape", [(307, 384), (411, 384), (384, 384), (20, 20), (200, 200), (201, 200), (199, 3), (288, 384), (1000, 25), (385, 1155)])
def test_small_shape_rule_is_the_oracles(shape):
    """oracle/wellmask.py:generate_well_mask: round(shape * min(1, 200 / max(shape))), numpy's round (half to even)"""
    from tmat_amd import well_mask_generation as wmg
    ratio = min(1, 200 / np.max(shape))
    want = tuple(int(v) for v in np.round(np.asarray(shape) * ratio))
    assert wmg.small_shape_of(shape) == want
    assert max(want) <= 200


def test_small_shape_refuses_empty_shapes():
    from tmat_amd import _lib
    a, b = C.c_int(), C.c_int()
    L = _lib.lib()
    assert L.tmat_well_small_shape(0, 5, C.byref(a), C.byref(b)) == _lib.E_ARG
    assert L.tmat_well_small_shape(5, 5, None, C.byref(b)) == _lib.E_ARG


def test_python_struct_has_the_sizes_the_library_accepts():
    """include/tmat.h: sizeof(tmat_stack_opts) as this build has it, and TMAT_STACK_OPTS_SIZE_V1, the struct up to pass_stacks"""
    import re
    from pathlib import Path
    from tmat_amd import _lib
    hdr = (Path(__file__).resolve().parents[1] / "include" / "tmat.h").read_text()
    v1 = int(re.search(r"#define TMAT_STACK_OPTS_SIZE_V1 (\d+)u", hdr).group(1))
    assert _lib.STACK_OPTS_SIZE_V1 == v1 == 88

    class V1(C.Structure):
        _fields_ = _lib.StackOpts._fields_[:[f[0] for f in _lib.StackOpts._fields_].index("vis_width")]
    assert C.sizeof(V1) == v1
    assert _lib.StackOpts.vis_width.offset + 4 == v1          # the first new field lies in what was padding
    assert C.sizeof(_lib.StackOpts) == 120
    names = [f[0] for f in _lib.StackOpts._fields_]
    assert names[-5:] == ["vis_width", "rgb_out", "bars_out", "cap_b", "n_bars"]
    body = hdr[hdr.index("typedef struct tmat_stack_opts {"):hdr.index("} tmat_stack_opts;")]
    declared = re.findall(r"\b(\w+)\s*(?:;|,)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert declared == names


def test_a_chunk_counts_its_resident_copy():
    """compute_branches.py's stack_chunk_ends: every held stack counts its pass bytes plus its uint16 copy in the resident chunk"""
    from tmat_amd import sato
    shape = (24, 1024, 1024)
    plan = sato.stack_pass_plan(1, *shape, 384)[1]
    nb = sato.stack_chunk_bytes(shape, 384)
    assert nb == plan + 24 * 1024 * 1024 * 2
    key = (shape, 800.0, 16)
    for held in range(1, 9):
        for budget in (plan * (held + 1), nb * (held + 1) - 1, nb * (held + 1)):
            want = sato.chunk_ends(key, held, nb * held, key, nb, budget)
            assert sato.stack_chunk_ends([key] * held, key, shape, 384, budget) == want
    # a budget the pass bytes alone would fit but the resident copies do not
    assert not sato.chunk_ends(key, 3, plan * 3, key, plan, plan * 4)
    assert sato.stack_chunk_ends([key] * 3, key, shape, 384, plan * 4)
    assert not sato.stack_chunk_ends([key] * 3, key, shape, 384, nb * 4)
    assert sato.stack_chunk_ends([key] * 3, ((24, 1024, 1000), 800.0, 16), (24, 1024, 1000), 384, 1 << 60)      # another key
    assert sato.stack_chunk_ends([key] * 8, key, shape, 384, 1 << 60)                                            # eight stacks
