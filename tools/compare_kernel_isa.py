"""Is the device code of the existing kernels the same in two trees?  compare_kernel_isa.py TREE_A TREE_B [NAME ...]

Compiles csrc/NAME.hip of both trees for the device only, with the flags the Makefile gives it, to assembly, and compares the text after removing
what names the compilation unit and nothing else: the unit's id symbol (__hip_cuid_<hash>) and the .file / .ident lines.  NAME defaults to every
translation unit with kernels that both trees have.  Prints one line per unit and exits 1 if any differs."""
import os
import re
import subprocess
import sys
import tempfile

EXACT = ["-ffp-contract=off"]
FLAGS = {"shade": EXACT + ["-mllvm", "-disable-machine-licm"], "env_light": [], "exchange": [], "antialias": []}
DEFAULT = ["shade", "geometry", "trace", "ray_refit", "ray_resplit", "ray_ao", "hit_shade", "compose", "skin", "morph", "antialias", "texture_mips", "env_light", "exchange"]


def isa(tree, name, out):
    src = os.path.join(tree, "arctic-renderer_amd", "csrc", name + ".hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"] + FLAGS.get(name, EXACT) + [src, "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, cwd=os.path.dirname(src))
    text = open(out).read()
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", text)
    return "\n".join(l for l in text.splitlines() if not re.match(r"\s*\.(file|ident)\b", l))


def main():
    a, b, names = sys.argv[1], sys.argv[2], sys.argv[3:] or DEFAULT
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            x, y = isa(a, name, os.path.join(tmp, "a.s")), isa(b, name, os.path.join(tmp, "b.s"))
            kernels = len(re.findall(r"^\s*\.amdhsa_kernel\b", x, flags=re.M))
            same = x == y
            differ += not same
            print(f"{name}.hip: {kernels} kernels, {len(x.splitlines())} lines of device assembly: {'identical' if same else 'DIFFERENT'}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
