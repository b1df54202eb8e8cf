#!/usr/bin/env python3
"""Device-code diff of two checkouts, kernel by kernel. Needs hipcc, no GPU.

    tools/kernel_isa_diff.py A B [--rename REGEX=REPL ...] [-j N]

Every csrc/*.hip of both checkouts is compiled device-only to assembly with the flags that checkout's own build.py gives the
file. Per kernel symbol the instruction stream and the descriptor (.amdhsa_* block and the code-object metadata: registers,
LDS, scratch, spills, arguments) are compared after symbol names and local labels have been normalised. One line per kernel:
identical / differs / only-in-A / only-in-B, with B's (else A's) size and registers, then the totals and the registers spilled on
either side. Exit status 1 on any `differs` or `only-in-B`; an `only-in-A` is a removal for the caller to judge.
--rename rewrites A's mangled names before matching, for instantiations whose template parameters changed, e.g.
    --rename '(attn_flash8m16_kernelI\\w+?Lb[01]E)Lb1E(Lb[01]EE)=\\1\\2'        # <T, kExact, true, kLse> -> <T, kExact, kLse>
The acceptance check of a refactor of csrc/: a `differs` line means the refactor changed device code.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import yaml


def load_build(root):
    spec = importlib.util.spec_from_file_location("_mvi_build", os.path.join(root, "multiview_inpaint_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(b, src, tmp):
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    subprocess.run([b.HIPCC, *b.FLAGS, *b.EXTRA.get(os.path.basename(src), []), "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    with open(out) as f:
        return f.read()


def kernels(text):
    """{mangled name: (normalised instruction lines, descriptor dict)} of one assembly file"""
    meta = yaml.safe_load(text.split(".amdgpu_metadata\n", 1)[1].split(".end_amdgpu_metadata", 1)[0].strip())
    names = [k[".name"] for k in meta["amdhsa.kernels"]]
    # longest first, so that a name that is a prefix of another never eats part of it
    sym = re.compile("|".join(re.escape(n) for n in sorted(names, key=len, reverse=True)))
    res = {}
    for k in meta["amdhsa.kernels"]:
        name = k[".name"]
        body = text.split("\n%s:" % name, 1)[1].split("\n.Lfunc_end", 1)[0]
        code, desc = body.split("\t.amdhsa_kernel ", 1) if "\t.amdhsa_kernel " in body else (body, "")
        ins = []
        for line in code.split("\n")[1:]:
            line = line.split(";", 1)[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")) or line.startswith(".Ltmp"):
                continue                                    # comments, directives, debug labels
            line = re.sub(r"\.L([A-Za-z_]+)\d+_(\d+)", r".L\1_\2", line)      # .LBB<function>_<block>
            ins.append(sym.sub("<kernel>", line))
        d = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_(\w+) (\S+)", desc)}
        d.update({key: sym.sub("<kernel>", str(v)) for key, v in k.items() if key not in (".name", ".symbol")})
        res[name] = (ins, d)
    return res


def collect(root, jobs):
    b = load_build(root)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(jobs) as ex:
        texts = list(ex.map(lambda s: assembly(b, s, tmp), b.sources()))
    res = {}
    for src, text in zip(b.sources(), texts):
        for name, k in kernels(text).items():
            res[name] = (os.path.basename(src),) + k
    return res


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"\(.*", "", d).replace("void ", "") for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    A = collect(os.path.abspath(args.a), args.j)
    B = collect(os.path.abspath(args.b), args.j)
    renamed = {}
    for name, k in A.items():
        new = name
        for r in args.rename:
            pat, repl = r.split("=", 1)
            new = re.sub(pat, repl, new)
        if new in renamed:
            sys.exit("rename map sends two kernels of A to " + new)
        renamed[new] = (name,) + k
    nice = demangle(sorted(set(renamed) | set(B)))
    count = {"identical": 0, "differs": 0, "only-in-A": 0, "only-in-B": 0}
    spills = {"A": 0, "B": 0}
    for name in sorted(set(renamed) | set(B), key=lambda n: ((renamed.get(n) or (0,) + B[n])[1], nice[n])):
        a, b = renamed.get(name), B.get(name)
        f, ins, d = b or a[1:]
        info = "%s %d lines, %s VGPR, %s SGPR, %s B LDS, %s B scratch, spills %s+%s" % (
            f, len(ins), d[".vgpr_count"], d[".sgpr_count"], d[".group_segment_fixed_size"], d[".private_segment_fixed_size"],
            d[".sgpr_spill_count"], d[".vgpr_spill_count"])
        for side, k in (("A", a and a[1:]), ("B", b)):
            if k:
                spills[side] += int(k[2][".sgpr_spill_count"]) + int(k[2][".vgpr_spill_count"])
        if a and b:
            what = "identical" if a[2:] == b[1:] else "differs"
            if what == "differs":
                keys = sorted(x for x in set(a[3]) | set(d) if a[3].get(x) != d.get(x))
                first = next((i for i, (x, y) in enumerate(zip(a[2], ins)) if x != y), min(len(a[2]), len(ins)))
                info += " | A: %d lines; first difference at line %d; descriptor keys %s" % (len(a[2]), first, keys or "none")
            if a[0] != name:
                info += " | was " + demangle([a[0]])[a[0]]
        else:
            what = "only-in-A" if a else "only-in-B"
        count[what] += 1
        print("%-10s %s  [%s]" % (what, nice[name], info))
    print("total: " + ", ".join("%d %s" % (v, k) for k, v in count.items()) + "; spilled registers: %(A)d in A, %(B)d in B" % spills)
    return 1 if count["differs"] or count["only-in-B"] else 0


if __name__ == "__main__":
    sys.exit(main())
