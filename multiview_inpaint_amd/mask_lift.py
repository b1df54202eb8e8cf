"""Lifting 2-D masks onto the Gaussians: the mask-driven counterpart of box_region.delete_inside.

The inpainting pipeline has per-view object masks from its Segment-and-Track step (the reference only masks the loss with them,
gs-simp/inpaint_rec.py:114-123) and picks the Gaussians to delete with a hand-made box mesh (gs-simp/del.py). Here the masks
themselves say which Gaussians are the object, by a vote weighted with what every Gaussian contributes to every pixel:

    total_i = sum over views and pixels of alpha_i(p) T_i(p)             (the blend weight the forward gave Gaussian i)
    hit_i,c = sum over views and pixels of alpha_i(p) T_i(p) w_c(p)      (the same, weighted by channel c of a per-pixel image)

over exactly the (pixel, Gaussian) pairs the forward composites (raster.lift_weights, csrc/raster_lift.hip). A Gaussian belongs
to mask c when hit / total exceeds a ratio; `total` alone is the visibility / importance score that pruning schemes use.
Building cameras from a dataset stays the caller's job: a view is (GaussianRasterizationSettings, weights).

The other direction carries a selection of Gaussians (or any per-Gaussian weights) into a view:

    soft_c(p) = sum_i alpha_i(p) T_i(p) m_i,c                             (raster.splat_features, csrc/raster_splat.hip)

the transpose of the vote, over the same (pixel, Gaussian) pairs. Its use: hint masks for views that have no 2-D mask. The views
the SVD stage inpaints are synthesised sequence and orbit cameras (gs-simp/gen_seq.py, scene/__init__.py:129-255); the reference
gets their hint mask from the hand-made box mesh (gen_seq.py:47-54, box_region here). With project_selection a selection made
from masks serves instead, and propagate_masks is the whole way in one call: masks in some views -> selection -> masks in any view.
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


def _selection_features(selection, normalize):
    """selection [P] | [P, K], bool or float -> (fp32 [P, K (+ 1)] features, K); with normalize a column of ones rides along."""
    if not torch.is_tensor(selection) or selection.ndim not in (1, 2) or (selection.ndim == 2 and selection.shape[1] < 1):
        raise ValueError("project_selection: selection must be a [P] or [P, K] tensor with K >= 1, got "
                         f"{tuple(selection.shape) if torch.is_tensor(selection) else type(selection).__name__}")
    if selection.dtype != torch.bool and not selection.dtype.is_floating_point:
        raise TypeError(f"project_selection: selection must be bool or floating point, got {selection.dtype}")
    m = selection.to(torch.float32)
    if m.ndim == 1:
        m = m[:, None]
    K = int(m.shape[1])
    if normalize:
        m = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
    return m, K


def normalize_soft_masks(soft, alpha):
    """soft [K,H,W] / alpha [H,W] where alpha > 0, 0 elsewhere: the share of a pixel's composited weight the selection owns.
    Pure torch; works on CPU tensors too."""
    if soft.ndim != 3 or alpha.ndim != 2 or tuple(soft.shape[1:]) != tuple(alpha.shape):
        raise ValueError(f"normalize_soft_masks: soft must be [K,H,W] and alpha [H,W], got {tuple(soft.shape)} and {tuple(alpha.shape)}")
    pos = alpha > 0
    return torch.where(pos[None], soft / torch.where(pos, alpha, torch.ones_like(alpha))[None], torch.zeros_like(soft))


def project_selection(selection, views, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, normalize=False):
    """Soft masks of a selection of Gaussians in `views`, an iterable of GaussianRasterizationSettings: a list of fp32 [K,H,W]
    images sum_i alpha_i(p) T_i(p) m_i,k (raster.GaussianRasterizer.splat), one per view. selection: [P] or [P, K], bool
    (membership) or float (soft weights), on the Gaussians' device. normalize: every mask is divided by the view's alpha image
    sum alpha T (a column of ones splatted as one more channel) where that is > 0 and is 0 elsewhere: the share of the pixel's
    composited weight that the selection owns, in [0, 1] for weights in [0, 1]."""
    m, K = _selection_features(selection, normalize)
    P = int(means3D.reshape(-1, 3).shape[0])
    if int(m.shape[0]) != P:
        raise ValueError(f"project_selection: selection has {int(m.shape[0])} rows for {P} Gaussians")
    m = m.to(means3D.device)
    masks = []
    for rs in views:
        img = raster.GaussianRasterizer(rs).splat(m, means3D, opacities, scales=scales, rotations=rotations,
                                                  cov3D_precomp=cov3D_precomp)
        masks.append(normalize_soft_masks(img[:K], img[K]) if normalize else img)
    return masks


def propagate_masks(src_views, dst_views, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, channel=0,
                    ratio=0.5, min_total=0.0, normalize=False):
    """Masks in some views -> selection -> masks in any view: lift_views over src_views (as in lift_views: (settings, weights)
    pairs), select(channel, ratio, min_total), project_selection into dst_views (settings). Returns (selection bool [P], masks:
    a list of fp32 [1,H,W], one per destination view)."""
    acc = lift_views(src_views, means3D, opacities, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    selection = select(acc, channel, ratio, min_total)
    masks = project_selection(selection, dst_views, means3D, opacities, scales=scales, rotations=rotations,
                              cov3D_precomp=cov3D_precomp, normalize=normalize)
    return selection, masks


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
