"""Cases and predictors of the general smooth-tiling fixture (tests/golden/smooth_general.npz), shared by its generator
(tools/make_goldens.py:gen_smooth_general) and the tests (tests/test_smooth_general_host.py, tests/test_gpu_smooth_general.py).

The predictor is `pred = batch[..., None] * R + T` with R, T of shape (ws, ws, 1) from a seeded RandomState: it is not symmetric under
D4, so a wrong orientation, tile order or transposition changes the result.  Every call is logged: the batch shapes, and one SHA-256
over the batch bytes in call order."""
import hashlib

import numpy as np

# name, image shape, window_size, subdivisions, predictor kind
CASES = [
    ("s2", (23, 37), 16, 2, "f32"),             # subdivisions 2 through the general kernels
    ("s4", (23, 37), 16, 4, "f32"),
    ("s3", (20, 31), 12, 3, "f32"),
    ("aug_half_down", (9, 14), 6, 4, "f32"),    # aug 4.5 -> 4, step 1
    ("aug_half_up", (17, 11), 10, 4, "f32"),    # aug 7.5 -> 8
    ("tiny", (5, 3), 16, 4, "f32"),             # image smaller than a step
    ("odd_window", (30, 30), 15, 3, "f32"),
    ("step_rest", (30, 41), 16, 3, "f32"),      # step 5, aug 11: the step does not divide the frame
    ("identity", (24, 36), 16, 4, "identity"),  # every pixel covered
    ("f64", (20, 31), 12, 3, "f64"),            # float64 predictor
]
NAMES = [c[0] for c in CASES]
WINDOWS = (6, 10, 12, 15, 16, 64, 320)


def case_image(name):
    i = NAMES.index(name)
    return np.random.RandomState(100 + i).uniform(0, 1, CASES[i][1]).astype(np.float32)


class Predictor:
    """pred_func of a case: logs its calls"""

    def __init__(self, ws, kind, seed=5):
        rs = np.random.RandomState(seed)
        self.kind = kind
        self.R = rs.uniform(0.5, 1.5, (ws, ws, 1)).astype(np.float32)
        self.T = rs.uniform(-0.5, 0.5, (ws, ws, 1)).astype(np.float32)
        self.shapes = []
        self._sha = hashlib.sha256()

    def __call__(self, batch, verbose=0):
        b = np.ascontiguousarray(batch)
        assert b.dtype == np.float32, b.dtype
        self.shapes.append(b.shape)
        self._sha.update(b.tobytes())
        if self.kind == "identity":
            return b[..., None]
        if self.kind == "f64":
            return b[..., None].astype(np.float64) * self.R.astype(np.float64) + self.T.astype(np.float64)
        return b[..., None] * self.R + self.T

    def log(self):
        """(calls, 3) int64 batch shapes, 32 digest bytes"""
        return np.array(self.shapes, np.int64).reshape(-1, 3), np.frombuffer(self._sha.digest(), np.uint8)


def predictor_of(name):
    _, _, ws, _, kind = CASES[NAMES.index(name)]
    return Predictor(ws, kind)
