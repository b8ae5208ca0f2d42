// Well detection (--detect-well): device stages of fl_tissue_model_tools/well_mask_generation.py (wellmask_kernels.hip)
// Every stage but the float32 rescale takes n_img images of one shape in one launch; per-image quantities are indexed by the image.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace tmat {
// rescale_intensity(blur, out_range=(0, 255)).astype(uint8) of a float32 image whose extrema are mn[0], mx[0] (device)
void launch_wm_rescale_u8(const float *blur, size_t n, const float *mn, const float *mx, uint8_t *out, hipStream_t s);
// the same for float64 images of n values each; mm: 2 n_img doubles of device scratch (extrema are computed here, per image)
void launch_wm_rescale_u8_f64(const double *blur, int n_img, size_t n, double *mm, uint8_t *out, hipStream_t s);
// hist: per image 5 x 256 counts (whole image, then the four 5 % corners: top-left, top-right, bottom-left, bottom-right); zeroed here
void launch_wm_hist(const uint8_t *img, int n_img, int H, int W, unsigned *hist, hipStream_t s);
// per image: decision[0] = Otsu threshold of the (possibly inverted) image, decision[1] = invert flag (auto_threshold_well :244-273)
void launch_wm_decide(const unsigned *hist, int n_img, int H, int W, int *decision, hipStream_t s);
void launch_wm_threshold(const uint8_t *img, int n_img, size_t n, const int *decision, uint8_t *out, hipStream_t s);
// binary erosion with the offsets `off` (noff pairs dy, dx), pixels outside the image count as set (border_value=True)
void launch_wm_erode(const uint8_t *m, int n_img, int H, int W, const int *off, int noff, uint8_t *out, hipStream_t s);
// canny's smoothing of a 0 / 1 mask with mode="constant": pad (zeros, and a second padded image of ones inside), crop + divide
void launch_wm_pad(const uint8_t *m, int n_img, int H, int W, int r, double *img_pad, double *ones_pad, hipStream_t s);
void launch_wm_crop_div(const double *img_pad, const double *ones_pad, int n_img, int H, int W, int r, double *out, hipStream_t s);
// img_as_float of n unsigned integer values (widened to u16): out = (double)v * inv_max, inv_max = 1.0 / 65535.0 or 1.0 / 255.0
void launch_wm_unit_f64(const uint16_t *img, size_t n, double inv_max, double *out, hipStream_t s);
// edges |= the mask's pixels in the first / last row and column (:165-170)
void launch_wm_border(const uint8_t *m, int n_img, int H, int W, uint8_t *edges, hipStream_t s);
// well_mask_generation.py:_resize_nearest of n_img masks (wellfit_kernels.hip)
void launch_resize_nearest_u8(const uint8_t *in, int n_img, int H, int W, int oh, int ow, uint8_t *out, hipStream_t s);
}  // namespace tmat
