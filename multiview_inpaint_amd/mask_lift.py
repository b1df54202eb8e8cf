"""Lifting 2-D masks onto the Gaussians: the mask-driven counterpart of box_region.delete_inside.

The inpainting pipeline has per-view object masks from its Segment-and-Track step (the reference only masks the loss with them,
gs-simp/inpaint_rec.py:114-123) and picks the Gaussians to delete with a hand-made box mesh (gs-simp/del.py). Here the masks
themselves say which Gaussians are the object, by a vote weighted with what every Gaussian contributes to every pixel:

    total_i = sum over views and pixels of alpha_i(p) T_i(p)             (the blend weight the forward gave Gaussian i)
    hit_i,c = sum over views and pixels of alpha_i(p) T_i(p) w_c(p)      (the same, weighted by channel c of a per-pixel image)

over exactly the (pixel, Gaussian) pairs the forward composites (raster.lift_weights, csrc/raster_lift.hip). A Gaussian belongs
to mask c when hit / total exceeds a ratio; `total` alone is the visibility / importance score that pruning schemes use.
Building cameras from a dataset stays the caller's job: a view is (GaussianRasterizationSettings, weights).
"""
import numpy as np
import torch

from . import raster


def lift_views(views, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None):
    """Sums raster.GaussianRasterizer.lift over `views`, an iterable of (GaussianRasterizationSettings, weights) with weights
    [C,H,W] | [H,W] (CUDA fp32; C the same in every view, the image size need not be). Returns acc [P, 1 + C] fp32:
    acc[:, 0] = total, acc[:, 1 + c] = hit of channel c."""
    acc = None
    for rs, weights in views:
        acc = raster.GaussianRasterizer(rs).lift(weights, means3D, opacities, scales=scales, rotations=rotations,
                                                 cov3D_precomp=cov3D_precomp, acc=acc)
    if acc is None:
        raise ValueError("lift_views: no views")
    return acc


def select(acc, channel=0, ratio=0.5, min_total=0.0):
    """bool [P]: total > min_total and hit[channel] > ratio * total. A Gaussian no view composited (total 0) is never selected.
    Pure torch; works on CPU tensors too."""
    if acc.ndim != 2 or not 0 <= channel < acc.shape[1] - 1:
        raise ValueError(f"select: acc must be [P, 1 + C] with channel < C, got {tuple(acc.shape)} and channel {channel}")
    total = acc[:, 0]
    return (total > min_total) & (acc[:, 1 + channel] > ratio * total)


def delete_by_masks(ply_in, ply_out, views, ratio=0.5, min_total=0.0, device="cuda"):
    """Drops the Gaussians of ply_in that the masks of `views` select (channel 0 of every view's weights; select's ratio and
    min_total), writes the rest to ply_out with every attribute kept. Returns (kept, total)."""
    from . import gaussian_io, train_ops
    from .box_region import _ply_sh_degree
    g = gaussian_io.load_ply(ply_in, _ply_sh_degree(ply_in))
    P = g["xyz"].shape[0]
    names = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
    ts = [torch.from_numpy(g[k]).to(device) for k in names]
    xyz, f_dc, f_rest, raw_opacity, raw_scaling, raw_rotation = ts
    # the activations of gs-simp/scene/gaussian_model.py:95-115, as the training loop applies them
    scales, rotations, opacities, _ = train_ops.activate_gaussians(raw_scaling, raw_rotation, raw_opacity, f_dc, f_rest)
    acc = lift_views(views, xyz, opacities, scales=scales, rotations=rotations)
    keep = ~select(acc, 0, ratio, min_total)
    rows = train_ops.compact_rows(keep, [t.reshape(P, int(np.prod(t.shape[1:]))) for t in ts])
    out = [r.reshape((r.shape[0],) + t.shape[1:]) for r, t in zip(rows, ts)]
    gaussian_io.save_ply(ply_out, *out)
    return out[0].shape[0], P
