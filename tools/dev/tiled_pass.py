#!/usr/bin/env python3
"""One tiled pass of 8 images at 640 x 640 (1600 patches) through tmat_predict_smooth, twice (dev tool): under `rocprofv3 --kernel-trace` the
second pass gives the per-layer table of the TILED path (tools/gpu_layers.sh times the raw full-frame forward).  TMAT_ROI=0: whole patches."""
import sys
from pathlib import Path
REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO / "tissue-model-analysis-tools_amd"))
import numpy as np
from tmat_amd import synth, _lib
h = _lib.Handle(synth.pack_weights(synth.synth_weights(0)), 0, 1600)
x = np.random.RandomState(0).uniform(0, 1, (8, 640, 640)).astype(np.float32)
h.predict_smooth(x)
y = h.predict_smooth(x)
print("ok", float(y.min()), float(y.max()))
