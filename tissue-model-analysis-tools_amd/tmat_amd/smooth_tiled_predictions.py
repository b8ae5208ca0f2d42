"""Mirror of fl_tissue_model_tools.smooth_tiled_predictions (reference :220-267).

The reference tiles, predicts, windows and blends in numpy around `pred_func`.  Here the driver is a device pipeline in one of
three forms:

* `pred_func` is the `.predict` of a device model (models.UNetXceptionPatchSegmentor.model) and `subdivisions == 2`: tile gather ->
  UNet -> f64 window blend in one call (tmat_predict_smooth, csrc/blend_kernels.hip), as before;
* a device model and any other `subdivisions`: tmat_predict_smooth_ex;
* any other callable (a Keras `model.predict`, say) with a handle -- `handle=`, or the one `use_handle` has set, so that a call site
  with the reference's four arguments works: the session route (csrc/smooth_kernels.hip).  The device gathers the tiles, `pred_func`
  is called exactly as the reference calls it (:174-182), the device windows and blends what it returned.

Without a handle an arbitrary predictor is a TypeError: there is no numpy fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib

INFERENCE_BATCH_SIZE = 16   # the reference's chunk of predictor calls (:23); the device-model forms batch whole images

_handle = None


def use_handle(handle):
    """The handle (`_lib.Handle`; one without a model is enough) that calls with an arbitrary predictor and no `handle=` use; None
    clears it."""
    global _handle
    _handle = handle


def _session(handle, img, window_size, subdivisions, pred_func):
    """:227-265 around pred_func: one orientation after the other, chunks [i : i + 16] when an orientation has more than 16 tiles,
    otherwise one call, each `pred_func(batch (k, ws, ws) float32, verbose=0)` -> (k, ws, ws, 1)"""
    ws = int(window_size)
    _, _, counts, _ = _lib.smooth_plan(img.shape[0], img.shape[1], ws, subdivisions)
    handle.smooth_begin(img, ws, subdivisions)
    wide = False            # the session holds float64 predictions
    first = 0
    for g in range(8):
        n = counts[2 * (g & 1)] * counts[2 * (g & 1) + 1]
        tiles = handle.smooth_tiles(first, n)
        chunks = [tiles[i:i + INFERENCE_BATCH_SIZE] for i in range(0, n, INFERENCE_BATCH_SIZE)] if n > INFERENCE_BATCH_SIZE else [tiles]
        at = first
        for batch in chunks:
            pred = np.asarray(pred_func(batch, verbose=0))
            if pred.shape != (len(batch), ws, ws, 1):
                raise TypeError(f"pred_func returned shape {pred.shape} for a batch of shape {batch.shape}: expected "
                                f"{(len(batch), ws, ws, 1)} (single-channel predictions, as the reference's reshape :189 needs)")
            if pred.dtype != np.float32 or wide:        # float32 and float64 go through as they are; anything else, and float32 once
                pred = pred.astype(np.float64, copy=False)      # the session is float64, is widened (no bit of the result changes)
                wide = True
            handle.smooth_put(at, pred)
            at += len(batch)
        first += n
    return handle.smooth_end(img.shape)


def predict_img_with_smooth_windowing(input_img, window_size, subdivisions, pred_func, handle=None):
    model = getattr(pred_func, "__self__", None)
    device = getattr(model, "handle", None)
    handle = handle if handle is not None else _handle
    if device is None and handle is None:
        raise TypeError("tmat_amd.predict_img_with_smooth_windowing needs pred_func = <segmentor>.model.predict (a device model), or "
                        "handle= (or smooth_tiled_predictions.use_handle) for any other predictor: arbitrary Python predictors are "
                        "not supported without a device handle, there is no numpy path")
    if device is not None and window_size != model.patch_size:
        raise ValueError("window_size must equal the model's patch size")
    img = np.asarray(input_img)
    if img.ndim == 3 and img.shape[-1] == 1:
        img = img[..., 0]
    if img.ndim != 2:
        raise ValueError("expected a 2-D single-channel image")
    img = img.astype(np.float32)
    if device is None:
        return _session(handle, img, window_size, subdivisions, pred_func)
    if subdivisions == 2:
        return device.predict_smooth(img)
    return device.predict_smooth_ex(img, subdivisions)
