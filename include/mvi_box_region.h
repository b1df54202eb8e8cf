/*
 * mvi_box_region.h — C-ABI of the MI355X (gfx950) box-region ops: rays against the hand-made bounding-box mesh of the
 * multi-view inpainting pipeline (gs-simp/utils/bounding.py torchMesh.intersect), the inpaint masks of gen_seq.py:46-52
 * and the point deletion of del.py:104-111.
 *
 * Conventions as in mvi_raster.h: every pointer is a DEVICE pointer, fp32 contiguous unless stated; `stream` is a
 * hipStream_t passed as void*; nothing synchronises; the library owns no memory. Returns 0 or a negative MVI_E* code
 * (mvi_raster.h); mvi_box_region_last_error() gives the message.
 *
 * The ray-face rule is the reference's, literally (bounding.py:62-99), in fp32 with its operation order:
 *   d = d / max(|d|, 1e-12)                          (F.normalize)
 *   h = d x e2, a = e1 . h, f = 1 / (a + 1e-8), s = o - v0, u = f (s . h), q = s x e1, v = f (d . q), t = f (e2 . q)
 *   invalid = (-1e-8 < a < 1e-8) | u < 0 | u > 1 | v < 0 | u + v > 1 | t < 1e-8
 *   max_t = max over ALL faces of t; int_t = min over faces of (invalid ? max_t + 1 : t), t_ind = its first index;
 *   cond = (max_t + 1 - int_t) > 0; where !cond: int_t = 0, int_p = 0; else int_p = o + int_t d.
 * The cross product is taken over the last axis (the reference's torch.cross without `dim` crosses over the first axis of
 * length 3, wrong for a chunk of exactly 3 rays or a 3-face mesh). The cross product, the norm and the camera rotation are
 * evaluated in the fused multiply-add forms PyTorch's CPU kernels use, so results equal the reference bit for bit.
 */
#ifndef MVI_BOX_REGION_H
#define MVI_BOX_REGION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* rays o [n,3], d [n,3] (not necessarily unit) against the triangles f_v [F,3,3] (F >= 1). Writes int_p [n,3], int_t [n],
 * t_ind [n] (int64), cond [n] (uint8 0/1). One launch. */
int mvi_mesh_intersect(const float* o, const float* d, int64_t n, const float* f_v, int32_t F, float* int_p, float* int_t,
                       int64_t* t_ind, uint8_t* cond, void* stream);

/* del.py:104-111: inside[i] = 1 when the rays from xyz[i] along +x and along -x both hit (int_t > 0), else 0.
 * xyz [N,3], inside [N] (uint8). One launch. */
int mvi_mesh_points_inside(const float* xyz, int64_t N, const float* f_v, int32_t F, uint8_t* inside, void* stream);

/* gen_seq.py:46-52 for V views of one size H x W in one launch. Per view: c2w [V,4,4] camera-to-world, fx, fy [V]
 * (W / (2 tan(FoVx / 2)), H / (2 tan(FoVy / 2))), depth [V,1,H,W]. The ray of pixel (x, y) is built as
 * scene/helpers.py:107-140 builds it: origin c2w[:3,3], direction R ((x + 0.5 - W/2) / fx, (y + 0.5 - H/2) / fy, 1) with
 * integer W/2, H/2. Writes mask [V,1,H,W] = (t > 0) & ((t < depth) | (depth == 15)) as 0/1 floats; optionally (NULL =
 * skip) masked [V,3,H,W] = render * (1 - mask) + mask from render [V,3,H,W] (both NULL or both set), and disparity
 * [V,1,H,W] = 1 / max(depth, 1e-3) (render_depth.py:37). No ray is stored. */
int mvi_mesh_view_masks(const float* c2w, const float* fx, const float* fy, int32_t V, int32_t H, int32_t W,
                        const float* f_v, int32_t F, const float* depth, const float* render, float* mask, float* masked,
                        float* disparity, void* stream);

const char* mvi_box_region_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MVI_BOX_REGION_H */
