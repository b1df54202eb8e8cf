"""Mechanical drop-in contract: the reference's own call sites and YAML `target:` strings are checked against the
replacement's surface. The reference's tree does not travel with the repository; what the test needs of it is recorded under
tests/golden/dropin/ by tools/gen_golden_dropin.py (the renderer's call sites as names and counts, the two YAML files as they are).

Path A — gs-simp/gaussian_renderer/__init__.py:36-49 (GaussianRasterizationSettings(...) keywords) and :85-93
(rasterizer(...) keywords, 3-tuple result) against multiview_inpaint_amd.dropin.diff_gaussian_rasterization.
Path B — every `target:` of svd_inpaint1/configs/test/svd_f_est_ctrl_simp1.yaml and scripts/sampling/configs/svd.yaml:
each in-scope one must import from multiview_inpaint_amd/dropin under the same dotted name and accept the YAML's
`params` keys; every other one must be on the explicit out-of-scope list below, so a new target in the
reference cannot go unnoticed."""
import importlib
import inspect
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "multiview_inpaint_amd", "dropin")
if DROPIN not in sys.path:
    sys.path.insert(0, DROPIN)

GOLDEN = os.path.join(ROOT, "tests", "golden", "dropin")
RENDERER_CALLS = os.path.join(GOLDEN, "gs_simp_renderer_call_sites.json")      # gs-simp/gaussian_renderer/__init__.py
YAMLS = [os.path.join(GOLDEN, "svd_f_est_ctrl_simp1.yaml"),                      # svd_inpaint1/configs/test/
         os.path.join(GOLDEN, "svd.yaml")]                                       # svd_inpaint1/scripts/sampling/configs/

# targets that are callers / conditioners / training-only (SURVEY.md §2 out-of-scope rows) — not part of the hot path
OUT_OF_SCOPE = {
    "models.csvd.SVDEngine", "sgm.models.diffusion.DiffusionEngine",                 # Lightning engines (callers)
    "sgm.data.my_dataset.DataModuleFromConfig", "sgm.data.my_dataset.GS_VideoForwardDatasetSimp",
    "sgm.modules.GeneralConditioner", "sgm.modules.encoders.modules.ConcatTimestepEmbedderND",
    "sgm.modules.encoders.modules.FrozenOpenCLIPImageEmbedder",
    "sgm.modules.encoders.modules.FrozenOpenCLIPImagePredictionEmbedder",
    "sgm.modules.encoders.modules.VideoPredictionEmbedderWithEncoder",
    "sgm.models.autoencoder.AutoencoderKLModeOnly",                                  # image VAE inside the conditioner
    "sgm.modules.diffusionmodules.loss.InpaintDiffusionLoss", "sgm.modules.diffusionmodules.loss_weighting.EDMWeighting",
    "sgm.modules.diffusionmodules.sigma_sampling.EDMSampling",                       # training half
    "torch.nn.Identity",
}


def test_rasterizer_call_sites_match_the_replacement():
    import diff_gaussian_rasterization as dgr
    rec = json.load(open(RENDERER_CALLS))
    # the import the reference performs
    imp = rec["imports_from_diff_gaussian_rasterization"]
    assert imp and all(hasattr(dgr, a) for a in imp)
    # GaussianRasterizationSettings(...): keyword set == NamedTuple fields, same order, nothing positional
    (call,) = rec["calls"]["GaussianRasterizationSettings"]
    assert not call["positional_args"]
    assert tuple(call["keywords"]) == dgr.GaussianRasterizationSettings._fields
    # GaussianRasterizer(raster_settings=...)
    (ctor,) = rec["calls"]["GaussianRasterizer"]
    assert ctor["keywords"] == ["raster_settings"]
    assert "raster_settings" in inspect.signature(dgr.GaussianRasterizer.__init__).parameters
    # rasterizer(...): all keywords are parameters of forward, every parameter without a default is supplied
    (fwd,) = rec["calls"]["rasterizer"]
    assert not fwd["positional_args"]
    kws = fwd["keywords"]
    sig = inspect.signature(dgr.GaussianRasterizer.forward)
    params = {n: p for n, p in sig.parameters.items() if n != "self"}
    assert set(kws) <= set(params), set(kws) - set(params)
    required = {n for n, p in params.items() if p.default is inspect.Parameter.empty}
    assert required <= set(kws), required - set(kws)
    sig.bind(None, **{k: None for k in kws})
    # ... and its result is unpacked into exactly three names (color, radii, depth)
    assert fwd["assigned_to"] == [3]
    # the consumers of the result: `radii > 0` and the screen-space tensor's .grad (gaussian_model.py:482-484)
    assert rec["uses_radii_gt_0"]


def _targets(node, out):
    if isinstance(node, dict):
        if "target" in node and isinstance(node["target"], str):
            out.append((node["target"], node.get("params") or {}))
        for v in node.values():
            _targets(v, out)
    elif isinstance(node, list):
        for v in node:
            _targets(v, out)
    return out


def _construct(cls, params):
    """Builds the object with exactly the YAML's params, on the meta device (no memory, no initialisation cost): an
    unexpected keyword or a missing required one raises TypeError here, as it would in the reference engine."""
    import torch
    with torch.device("meta"):
        return cls(**params)


@pytest.mark.parametrize("path", YAMLS, ids=[os.path.basename(p) for p in YAMLS])
def test_every_yaml_target_is_in_scope_and_importable_or_listed_out_of_scope(path):
    import yaml
    cfg = yaml.safe_load(open(path))
    if os.path.basename(path) == "svd.yaml":
        # the stock script fills these two in before instantiating (scripts/sampling/simple_video_sample.py:342-345)
        sp = cfg["model"]["params"]["sampler_config"]["params"]
        sp["num_steps"] = 25
        sp["guider_config"]["params"]["num_frames"] = 14
    found = _targets(cfg, [])
    assert len(found) >= 10
    in_scope = 0
    for target, params in found:
        if target in OUT_OF_SCOPE:
            continue
        mod, cls = target.rsplit(".", 1)
        m = importlib.import_module(mod)
        assert os.path.realpath(m.__file__).startswith(os.path.realpath(DROPIN)), (target, m.__file__)
        obj = getattr(m, cls)
        if "device" in inspect.signature(obj.__init__).parameters and "device" not in params:
            params = dict(params, device="cpu")            # samplers default to "cuda" (sampling.py:29); no GPU here
        built = _construct(obj, params)
        assert type(built).__name__ == cls
        in_scope += 1
    assert in_scope >= 8, in_scope
    hot = {t for t, _ in found}
    for must in ("sgm.modules.diffusionmodules.denoiser.Denoiser", "sgm.modules.diffusionmodules.sampling.EulerEDMSampler",
                 "sgm.modules.diffusionmodules.guiders.LinearPredictionGuider",
                 "sgm.modules.diffusionmodules.discretizer.EDMDiscretization"):
        assert must in hot


def test_hot_path_yaml_blocks_instantiate_through_the_dropin():
    """The denoiser / sampler / network blocks of the test config build through instantiate_from_config exactly as the
    reference engine does it (sgm/util.py:168-185) — with the network shrunk (same keys, small widths) so it fits a test."""
    import yaml
    from sgm.util import instantiate_from_config
    cfg = yaml.safe_load(open(YAMLS[0]))["model"]["params"]
    den = instantiate_from_config(cfg["denoiser_config"])
    samp = instantiate_from_config({**cfg["sampler_config"], "params": {**cfg["sampler_config"]["params"], "device": "cpu"}})
    assert type(den).__name__ == "Denoiser" and type(samp).__name__ == "EulerEDMSampler"
    net = dict(cfg["network_config"])
    small = dict(net["params"], model_channels=32, num_head_channels=16, channel_mult=[1, 2], attention_resolutions=[2, 1],
                 num_res_blocks=1, context_dim=24, adm_in_channels=12, use_checkpoint=False)
    unet = instantiate_from_config({"target": net["target"], "params": small})
    ctrl = dict(cfg["control_config"]) if "control_config" in cfg else None
    assert type(unet).__name__ == "ControlledVideoUNet"
    if ctrl is not None:
        csmall = dict(ctrl["params"], model_channels=32, num_head_channels=16, channel_mult=[1, 2], attention_resolutions=[2, 1],
                      num_res_blocks=1, context_dim=24, adm_in_channels=12, use_checkpoint=False)
        cnet = instantiate_from_config({"target": ctrl["target"], "params": csmall})
        assert type(cnet).__name__ == "ControlNet"
