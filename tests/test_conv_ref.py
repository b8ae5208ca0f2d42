"""CPU: the bit-exact oracle of the convolution kernel (oracle/unet.py:_conv, _conv_subpixel -- oracle/unet_exact.c) against the
independent float64 restatement tests/helpers/conv_ref.py, on every case tests/test_gpu_conv_shapes.py sends to the GPU: shapes off the
networks' grid (one row, widths 2 / 5 / 7, odd widths behind a stride, M at 127 / 129 / 255 / 257, Cout 192 / 384, Cin 192, the
sub-pixel form at Cin 32, non-square images).  The GPU test asserts the kernel's bits against the oracle; this file is what makes the
oracle worth that trust at these shapes.

Tolerance, derived and not measured (conv_ref.bound): |f32 - v| <= gamma_(K + 2) mag, K = taps Cin, gamma_n = n u / (1 - n u),
u = 2^-24; gamma_(K + 5) for the sub-pixel form.  It is loose for rounding (the oracle uses a few per cent of it) and tight for
structure: the three mutation checks below show a misplaced tap, a shifted residual and the wrong stride-2 samples at tens of bounds."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import conv_cases as cc  # noqa: E402


def _worst(c, mutation=None):
    """max over the outputs of |oracle - reference| / bound"""
    o = cc.operands(c)
    got = cc.oracle(c, o).astype(np.float64)
    v, _ = cc.reference(c, o, mutation=mutation)
    _, bound = cc.reference(c, o)
    assert got.shape == v.shape and np.isfinite(got).all() and (bound > 0).all()
    return float((np.abs(got - v) / bound).max())


@pytest.mark.parametrize("group", ["a", "b", "c"])
def test_oracle_within_the_derived_bound_of_the_float64_reference(group):
    cases = {"a": cc.cases_a, "b": cc.cases_b, "c": lambda: [c for c, _ in cc.cases_c()]}[group]()
    assert len({c["id"] for c in cases}) == len(cases) and len({c["seed"] for c in cases}) == len(cases)
    worst = [(_worst(c), c["id"]) for c in cases]
    for r, name in worst:
        print(f"{name}: max |oracle - ref64| / bound = {r:.4f}")
    bad = [(r, name) for r, name in worst if not r <= 1.0]
    assert not bad, bad


def _pick(cases, **kw):
    (c,) = [c for c in cases if all(c[k] == v for k, v in kw.items())]
    return c


MUTANTS = [
    ("right tap wraps", lambda: _pick(cc.cases_a(), ksize=3, cout=128, hh=5, ww=7, resid=False)),
    ("resid shift", lambda: _pick(cc.cases_b(), rs=1, copy=False, cout=64, hh=6, ww=10)),
    ("odd samples", lambda: _pick(cc.cases_a(), stride=2, cout=192, resid=False)),
]


@pytest.mark.parametrize("mutation,pick", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_the_bound_rejects_a_wrong_reference(mutation, pick):
    """the last column's right tap not zero-padded / the residual read with rs off by one / stride 2 taking the odd indices: each is far
    outside the bound that the right reference meets"""
    c = pick()
    right, wrong = _worst(c), _worst(c, mutation)
    print(f"{c['id']}, {mutation}: {wrong:.1f} bounds (the right reference: {right:.4f})")
    assert right <= 1.0 < wrong
    assert wrong > 10.0, "a structural error is tens of bounds, not a near miss"
