"""Box-region layer without a GPU: the OBJ reader against the reference-parsed golden meshes, and the drop-in hook of
utils.bounding.torchMesh.intersect on a stand-in module tree (CPU tensors must reach the stand-in's own method)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import box_region_helpers as H
from multiview_inpaint_amd.box_region import BoxMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", sorted(H.MESHES))
def test_from_obj_equals_the_reference_parse(kind):
    m = BoxMesh.from_obj(H.mesh_path(kind), device="cpu")
    g = np.load(H.golden_path(f"mesh_{kind}.npz"))
    for k in ("v", "f", "f_v", "axes", "origin", "center"):
        got = getattr(m, k)
        assert got.dtype == torch.from_numpy(g[k]).dtype, k
        assert np.array_equal(got.numpy(), g[k]), k
    assert m.f_v.shape == (12, 3, 3)


def _stand_in_tree(tmp_path, with_bounding):
    for d in ("utils", "scene", "gaussian_renderer"):
        (tmp_path / d).mkdir()
    (tmp_path / "utils" / "__init__.py").write_text("")
    (tmp_path / "scene" / "__init__.py").write_text("")
    (tmp_path / "utils" / "loss_utils.py").write_text("def l1_loss(a, b):\n    return 0\ndef ssim(a, b):\n    return 0\n")
    (tmp_path / "scene" / "gaussian_model.py").write_text("class GaussianModel:\n    pass\n")
    (tmp_path / "gaussian_renderer" / "__init__.py").write_text("def render(*a, **k):\n    return None\n")
    if with_bounding:
        (tmp_path / "utils" / "bounding.py").write_text(textwrap.dedent("""
            import torch
            class torchMesh():
                def __init__(self):
                    self.f_v = torch.zeros(12, 3, 3)
                def intersect(self, rayo, rayd, bs=10000):
                    return ("stand-in intersect", tuple(rayo.shape), bs)
        """))
    (tmp_path / "seq_like.py").write_text(textwrap.dedent("""
        import torch
        from utils.bounding import torchMesh
        m = torchMesh()
        print("PATCHED", getattr(torchMesh.intersect, "_mvi_patched", False), torchMesh._reference_intersect is not torchMesh.intersect)
        print("CALL", m.intersect(torch.zeros(5, 3), torch.ones(5, 3), bs=7))
    """))


def _run(tmp_path, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)


def test_runner_hooks_torchmesh_intersect_and_cpu_rays_reach_the_reference(tmp_path):
    _stand_in_tree(tmp_path, with_bounding=True)
    p = _run(tmp_path, ["-m", "multiview_inpaint_amd.dropin.patch_gs_simp", str(tmp_path / "seq_like.py")])
    assert p.returncode == 0, p.stderr[-2000:]
    out = dict(line.split(" ", 1) for line in p.stdout.strip().splitlines())
    assert "utils.bounding.torchMesh.intersect" in p.stderr
    assert out["PATCHED"] == "True True"
    assert out["CALL"] == "('stand-in intersect', (5, 3), 7)"        # CPU rays: the stand-in's own method, with its bs


def test_no_bounding_module_no_mesh_hook(tmp_path):
    _stand_in_tree(tmp_path, with_bounding=False)
    code = ("import sys; sys.path.insert(0, '.'); from multiview_inpaint_amd.dropin import patch_gs_simp as p; "
            "done = p.install(); print(done); assert not [d for d in done if 'bounding' in d], done; "
            "assert p.install(loss=False, optimizer=False, render=False, stats=False, surgery=False) == []")
    r = _run(tmp_path, ["-c", code])
    assert r.returncode == 0, r.stderr[-2000:]
