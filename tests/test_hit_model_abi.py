"""ARCTIC_OPT_HIT_MODEL on a machine without a GPU: the option in the header, the binding, the C++ mirror and the Python surface; the text in
front of arctic_shade_hits that says what value 1 adds and what stays out; the range check as it stands in the source of arctic_set_option (a
handle cannot be made here: the refusal of values 2, -1 and 7 on a live handle is asserted by tests/test_gpu_hit_model.py);
the new unit's build rule; and the resource figures of k_shade_hits_ext (make asm-hit-ext) next to those of the base kernels (make asm-hit)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def test_the_option_in_header_binding_and_mirrors(pkg, lib):
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    ids = [int(v) for v in re.findall(r"#define\s+ARCTIC_OPT_HIT_MODEL\s+(\d+)", text)]
    assert ids == [lib.OPTIONS["hit_model"]]                                      # defined once, and the binding agrees (whatever the number is)
    every = [int(v) for v in re.findall(r"#define\s+ARCTIC_OPT_\w+\s+(\d+)", text)]
    dist = [int(v) for v in re.findall(r"#define\s+ARCTIC_OPT_\w+\s+(\d+)", open(os.path.join(ROOT, "include", "arctic_dist.h")).read())]
    assert len(every + dist) == len(set(every + dist)) and len(set(lib.OPTIONS.values())) == len(lib.OPTIONS)   # a number nobody else has
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    assert re.search(r"\[\[nodiscard\]\]\s+bool\s+set_hit_model\s*\(int \w+\)\s*\{[^}]*ARCTIC_OPT_HIT_MODEL", hpp)
    assert callable(getattr(pkg.renderer.Renderer, "set_hit_model"))
    # no device here, so no handle: the range check is read where it stands, in arctic_set_option
    src = open(os.path.join(CSRC, "renderer.cpp")).read()
    case = src[src.index("case ARCTIC_OPT_HIT_MODEL:"):]
    case = case[:case.index("break;")]
    assert "value < 0 || value > 1" in case and "ARCTIC_E_INVALID" in case and "r->hit_model = (int)value" in case


def test_the_header_says_what_the_option_adds_and_what_stays_out(pkg):
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    at = text.index("ARCTIC_OPT_HIT_MODEL = 1 (hit_shade_ext.hip: k_shade_hits_ext)")
    assert text.index("2. HIT SHADING") < at < text.index("int arctic_shade_hits(")
    body = text[at:text.index("int arctic_shade_hits(")]
    for phrase in ("eye := rays[k].origin", "sum(spot: colour att window / d2)", "sum(cube: colour v / d2)", "rgb   = Lo (1 - shadow) + A ao + E",
                   "not multiplied by (1 - shadow)", "ambient term only","att = sat(cd scale + offset)^2", "window = sat(1 - (d2 ir2)^2)",
                   "ties x, then y, then z", "compare then bilinear", "never multiplied by the sun's shadow", "Mip chains STAY OUT", "no pixel footprint",
                   "sampled at level 0", "gets the base model's bytes", "arctic_trace_gi, arctic_pass_gi", "allocates nothing", "neither drawn",
                   "arctic_write_point_shadow"):
        assert phrase in body, phrase
    # the base model's text, every phrase tests/test_hit_shading_abi.py pins, still stands
    for phrase in ("OUT OF SCOPE at hits", "spot lights, shadow-casting point lights, image-based ambient", "never\n *   drawn or written", "ARCTIC_OPT_SHADOW_SHARDED"):
        assert phrase in text, phrase


def test_the_build_rule_and_the_documents(pkg):
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^hit_shade_ext\.o:.*hit_shade_ext\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) -c ", make, flags=re.M)     # hit_shade.o's flags
    assert re.search(r"^OBJS\s*\+=.*\bhit_shade_ext\.o\b", make, flags=re.M) and "asm-hit-ext:" in make
    assert "k_shade_hits_ext" not in open(os.path.join(CSRC, "hit_shade.hip")).read().split("#include")[1]       # a unit of its own
    assert os.path.exists(os.path.join(CSRC, "hit_shade_ext.h")) and "launch_shade_hits_ext" in open(os.path.join(CSRC, "hit_shade_ext.h")).read()
    assert "ARCTIC_OPT_HIT_MODEL" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ 6ab\b", design, flags=re.M) and "k_shade_hits_ext" in design


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_kernel_uses_no_scratch_and_the_base_unit_keeps_its_three(tmp_path):
    """k_shade_hits_ext: ONE kernel holds all four features without scratch (no runtime-indexed array, no call) and without LDS; hit_shade.hip
    still compiles to exactly its three kernels"""
    log = subprocess.run(["make", "-C", CSRC, "asm-hit-ext", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    assert len(names) == 1 and "k_shade_hits_ext" in names[0], names
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)] == [0]
    assert [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)] == [0]
    path = str(tmp_path / "hit_shade_ext-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert [int(line.split(":")[1].split()[0]) for line in open(path) if line.startswith("; ScratchSize:")] == [0]
    print({k: int(re.search(k + r": (\d+)", remarks).group(1)) for k in ("VGPRs", "AGPRs", "TotalSGPRs", r"Occupancy \[waves/SIMD\]")})
    log = subprocess.run(["make", "-C", CSRC, "asm-hit", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", log.stdout + log.stderr)
    assert len(names) == 3 and all(sum(k in n for n in names) == 1 for k in ("k_hit_attributes", "k_shade_hits", "k_reflect_rays")), names
