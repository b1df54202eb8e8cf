"""Fixtures of tests/test_dropin_contract.py from a checkout of the reference project (whose tree the test cannot read):

  * tests/golden/dropin/gs_simp_renderer_call_sites.json — what gs-simp/gaussian_renderer/__init__.py asks of
    diff_gaussian_rasterization: the imported names, the keywords of its GaussianRasterizationSettings(...),
    GaussianRasterizer(...) and rasterizer(...) calls, how the rasterizer's result is unpacked, and whether `radii > 0`
    is what it consumes. Names and counts only; none of the file's text.
  * tests/golden/dropin/svd_f_est_ctrl_simp1.yaml, svd.yaml — the two configuration files (settings only) whose
    `target:` strings the test instantiates through the drop-in packages, copied unchanged.

Usage: python tools/gen_golden_dropin.py <reference checkout>
"""
import ast
import json
import os
import shutil
import sys

REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "dropin")
RENDERER = os.path.join("gs-simp", "gaussian_renderer", "__init__.py")
YAMLS = [os.path.join("svd_inpaint1", "configs", "test", "svd_f_est_ctrl_simp1.yaml"),
         os.path.join("svd_inpaint1", "scripts", "sampling", "configs", "svd.yaml")]

src = open(os.path.join(REF, RENDERER)).read()
tree = ast.parse(src)


def calls(name):
    out = []
    for c in ast.walk(tree):
        if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == name:
            assigns = [n for n in ast.walk(tree) if isinstance(n, ast.Assign) and n.value is c]
            out.append({"positional_args": len(c.args), "keywords": [k.arg for k in c.keywords],
                        # one entry per assignment of the call's result: tuple length, or null for a plain name
                        "assigned_to": [len(a.targets[0].elts) if isinstance(a.targets[0], ast.Tuple) else None for a in assigns]})
    return out


record = {
    "source": RENDERER.replace(os.sep, "/"),
    "imports_from_diff_gaussian_rasterization": [a.name for n in ast.walk(tree)
                                                 if isinstance(n, ast.ImportFrom) and n.module == "diff_gaussian_rasterization"
                                                 for a in n.names],
    "calls": {n: calls(n) for n in ("GaussianRasterizationSettings", "GaussianRasterizer", "rasterizer")},
    "uses_radii_gt_0": "radii > 0" in src,
}
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "gs_simp_renderer_call_sites.json"), "w") as fh:
    json.dump(record, fh, indent=1)
    fh.write("\n")
for y in YAMLS:
    shutil.copyfile(os.path.join(REF, y), os.path.join(OUT, os.path.basename(y)))
print("wrote", sorted(os.listdir(OUT)))
