// GPU binary morphology (morph_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
namespace tmat {
size_t morph_workspace_bytes(int k, int H, int W);
// device pointer to the k per-image "thinning converged" flags inside the workspace (1 = converged)
const int *morph_done_flags(void *workspace, int k, int H, int W);
// Where filter_mask_dev keeps its intermediate results inside the workspace (device pointers, valid after the call until the
// workspace's next one): med, skA (k, H, W) u8 -- the mask that gets labelled and the converged Zhang skeleton (skB holds the same
// once `done` is set); ML (k, H, W) int -- root pixel index of the mask component, -1 on the background (SL: the same of the
// skeleton); area, n1, n2, n3 (k, H, W) int, consecutive planes -- pixel count and perimeter code counts at each root's index, 0
// elsewhere; done (k) as morph_done_flags; changed (launches, k) -- 1 where a thinning launch removed something from that image.
struct MorphLayout {
    uint8_t *seg, *med, *skA, *skB;
    int *ML, *SL, *g, *area, *n1, *n2, *n3, *fork, *drop, *st, *flags, *done, *changed, *tflags;
    int launches, tiles_x, tiles_y;
    size_t flag_ints;                  // ints from `flags` to the end of the per-tile flags
    size_t bytes;                      // what the layout needs from `workspace` on (morph_workspace_bytes adds slack)
};
MorphLayout morph_layout(void *workspace, int k, int H, int W);       // workspace null: launches, tiles, flag_ints and bytes only
// pred (k, H, W) f64 device -> filtered mask (k, H, W) u8 device, EDT of it (k, H, W) f64 device; all async on `s`
int filter_edt_dev(const double *pred, int k, int H, int W, int remove_isolated, void *workspace, uint8_t *filt_out,
                   double *dist_out, hipStream_t s);
int filter_mask_dev(const double *pred, const uint8_t *mask_in, int k, int H, int W, int use_median, int remove_isolated,
                    void *workspace, uint8_t *filt_out, double *dist_out, hipStream_t s);
void launch_ccl(const uint8_t *mask, int k, int H, int W, int *L, hipStream_t s);
void launch_edt(const uint8_t *mask, int k, int H, int W, int *g, int *st, int *any_zero, double *dist, hipStream_t s);
// finish_kernels.hip: EDT(~skel), centre-line weighting, anti-aliased resize, rescale to 0..255
size_t finish_workspace_bytes(int k, int H, int W, int oh, int ow);
int finish_dev(const double *pred, const double *dist, const uint8_t *skel, int k, int H, int W, int oh, int ow, void *workspace,
               float *field_out, float *f255_out, hipStream_t s);
void launch_rescale255(const float *field, int k, int npx, float *mn, float *mx, float *out, hipStream_t s);
// the weighted prediction (k, H, W) f64 and its per-image minimum / maximum inside finish_dev's workspace: valid from finish_dev until
// the workspace's next finish_dev (the gaussian passes work in the other two f64 planes)
void finish_weighted_view(void *workspace, int k, int H, int W, const double **wt, const double **lo, const double **hi);
// vis_kernels.hip: save_vis pictures of (k, per) images of dtype TMAT_PIC_* in HBM -> (k, per) u8; 0, -1 (argument) or -2 (launch)
size_t vis_scratch_bytes(int k);
double *vis_scratch_lo(void *scratch, int k);          // lo [k] then hi [k], written by vis_minmax_dev
int vis_minmax_dev(const void *a, int dtype, int k, size_t per, void *scratch, hipStream_t s);
int vis_picture_dev(const void *a, int dtype, int k, size_t per, const double *lo, const double *hi, uint8_t *out, hipStream_t s);
int vis_picture_u16_dev(const uint16_t *a, int k, size_t per, const int *mn, const int *mx, uint8_t *out, hipStream_t s);
// postproc.cpp: the host twin of vis_minmax_dev + vis_picture_dev, the same bytes
void vis_pictures_host(const void *a, int dtype, int n, size_t per, uint8_t *out);
// zproj_kernels.hip: Z projection of n stacks (n, Z, H, W) u16 device -> (n, H, W) u16 (fs / min / max) or f64 (avg / med)
int zproj_dev(const uint16_t *stacks, int n, int Z, int H, int W, int method, void *out, hipStream_t s);
}  // namespace tmat
