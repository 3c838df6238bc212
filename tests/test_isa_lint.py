"""tools/isa_lint.py over the shading kernels' ISA: the two hazards the compiler cannot see inside shade.hip's asm statements (a scalar
load's destination touched before its s_waitcnt; a transcendental's result read by the very next VALU instruction).  CPU-only: hipcc
cross-compiles.  The first test proves the lint sees both on hand-made snippets, the second runs it on the real kernels."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(ROOT, "tools", "isa_lint.py"))
isa_lint = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_lint)

HEAD = "_ZN6arctic12_GLOBAL__N_110k_materialILi2ELb0EEEvNS_11ShadeParamsE:\n"
TAIL = "\t.end_amdhsa_kernel\n"


def _lint(tmp_path, body):
    p = tmp_path / "k.s"
    p.write_text(HEAD + body + TAIL)
    return isa_lint.lint(str(p)).problems


def test_lint_sees_the_hazards(tmp_path):
    clean = ("\t;;#ASMSTART\n\ts_load_dwordx4 s[8:11], s[2:3], 0x0\n\t;;#ASMEND\n\tv_mov_b32_e32 v1, v2\n\ts_waitcnt lgkmcnt(0)\n"
             "\tv_pk_add_f32 v[4:5], s[8:9], v[6:7]\n\tv_rsq_f32_e32 v8, v9\n\tv_mul_f32_e32 v10, v11, v12\n\tv_mul_f32_e32 v13, v8, v8\n")
    assert _lint(tmp_path, clean) == []
    early = clean.replace("\tv_mov_b32_e32 v1, v2\n", "\tv_pk_add_f32 v[4:5], s[8:9], v[6:7]\n")
    assert len(_lint(tmp_path, early)) == 1 and "before s_waitcnt" in _lint(tmp_path, early)[0]
    hot = clean.replace("\tv_mul_f32_e32 v10, v11, v12\n", "")
    assert len(_lint(tmp_path, hot)) == 1 and "transcendental" in _lint(tmp_path, hot)[0]
    nop = clean.replace("\tv_mul_f32_e32 v10, v11, v12\n", "\ts_nop 0\n")
    assert _lint(tmp_path, nop) == []
    other_order = early.replace("\tv_pk_add_f32 v[4:5], s[8:9], v[6:7]\n", "\ts_waitcnt lgkmcnt(0) vmcnt(1)\n\tv_pk_add_f32 v[4:5], s[8:9], v[6:7]\n", 1)
    assert _lint(tmp_path, other_order) == []        # the wait clears whatever else the instruction names, in any order
    plain_zero = early.replace("\tv_pk_add_f32 v[4:5], s[8:9], v[6:7]\n", "\ts_waitcnt 0\n\tv_pk_add_f32 v[4:5], s[8:9], v[6:7]\n", 1)
    assert _lint(tmp_path, plain_zero) == []


def test_lint_follows_a_load_across_labels_and_branches(tmp_path):
    """the split descriptor load of the fast tile (tex_desc_issue / tex_desc_wait) is waited for several basic blocks behind its issue: the walk
    follows fall-through edges and branch targets from the load to the wait on every path (the per-block scan stopped at the first label)"""
    load = "\t;;#ASMSTART\n\ts_load_dwordx8 s[24:31], s[4:5], 0x0\n\t;;#ASMEND\n"
    wait = "\t;;#ASMSTART\n\ts_waitcnt lgkmcnt(0)\n\t;;#ASMEND\n\ts_cmp_gt_i32 s26, -1\n"
    clean = load + "\ts_cbranch_scc1 .LBB0_2\n\tv_mov_b32_e32 v1, v2\n.LBB0_2:\n\tv_mov_b32_e32 v3, v4\n" + wait
    p = tmp_path / "k.s"
    p.write_text(HEAD + clean + TAIL)
    rep = isa_lint.lint(str(p))
    assert rep.problems == [] and rep.kernels == 1 and rep.asm_loads == 1 and rep.loads_across_labels == 1
    # a copy of a destination register on the fall-through path, two blocks behind the load
    spill = clean.replace("\tv_mov_b32_e32 v3, v4\n", "\tv_writelane_b32 v60, s25, 3\n")
    assert len(_lint(tmp_path, spill)) == 1 and "s[25]" in _lint(tmp_path, spill)[0]
    # ... or only on the path a branch takes (the wait on the fall-through path does not cover it)
    side = load + "\ts_cbranch_scc1 .LBB0_5\n" + wait + "\ts_endpgm\n.LBB0_5:\n\ts_mov_b32 s30, 0\n\ts_waitcnt lgkmcnt(0)\n"
    found = _lint(tmp_path, side)
    assert len(found) == 1 and "s_mov_b32 s30, 0" in found[0]
    # a wait that leaves scalar loads outstanding (lgkmcnt(1)) is no wait for this purpose
    weak = clean.replace("\tv_mov_b32_e32 v3, v4\n", "\ts_waitcnt lgkmcnt(1)\n\ts_add_u32 s0, s24, 1\n")
    assert len(_lint(tmp_path, weak)) == 1
    # a loop: the walk ends at instructions it has seen
    loop = load + ".LBB0_7:\n\tv_mov_b32_e32 v1, v2\n\ts_cbranch_scc1 .LBB0_7\n" + wait
    assert _lint(tmp_path, loop) == []


@pytest.fixture(scope="module")
def shade_isa(tmp_path_factory):
    """the shading kernels' ISA, compiled into a directory of this test run's own (concurrent runs do not share /tmp files)"""
    out = tmp_path_factory.mktemp("isa")
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "asm", f"OUT={out}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return str(out / "shade-hip-amdgcn-amd-amdhsa-gfx950.s")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_shading_kernels_are_clean(shade_isa):
    rep = isa_lint.lint(shade_isa)
    assert rep.problems == [], "\n".join(rep.problems)
    # ... and the lint looked at what it claims to (round 3's matched no kernel for a whole round): every instantiation of k_material /
    # k_material_vis, the asm scalar loads of the light pairs and of the split descriptor load, the latter followed across basic blocks
    assert rep.kernels >= 4 and rep.asm_loads >= 4 * rep.kernels // 2 and rep.loads_across_labels >= rep.kernels, rep._replace(problems=[])
    assert rep.visited > 50 * rep.kernels, rep._replace(problems=[])


def _kernel_resources(path):
    """{kernel symbol: {vgprs, sgprs, scratch, lds}} from the `; NumVgprs:` ... comments the assembler file carries behind every kernel"""
    import re
    out, name = {}, None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1); out[name] = {}
        for key, tag in (("vgprs", "; NumVgprs:"), ("sgprs", "; TotalNumSgprs:"), ("scratch", "; ScratchSize:"), ("lds", "; LDSByteSize:")):
            if name and line.startswith(tag):
                out[name][key] = int(line[len(tag):].split()[0])
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_shading_kernels_keep_their_register_budgets(shade_isa):
    """What decides the occupancy of the pass (measured by tools/experiments/occupancy2.hip, profiles/r4_occupancy_*):
    7 waves per SIMD need <= 72 VGPRs AND <= 96 SGPRs (VCC and the like included), and any scratch use costs more than a wave.  The
    compiler's counts move with unrelated edits: the default kernels are pinned here (round 3 shipped 72 VGPRs + 16 bytes of scratch;
    a day of round 4 saw 82 ... 102 SGPRs)."""
    res = _kernel_resources(shade_isa)
    for loop in (1, 2):
        k = res[f"_ZN6arctic12_GLOBAL__N_110k_materialILi{loop}ELb0EEEvNS_11ShadeParamsE"]       # the pass over a G-buffer: 7 waves per SIMD
        assert k["vgprs"] <= 72 and k["sgprs"] <= 96 and k["scratch"] == 0, (loop, k)
        assert k["lds"] <= 20 * 1024, (loop, k)       # 8 workgroups per CU must fit the 160 KiB
    for loop in (1, 2):
        k = res[f"_ZN6arctic12_GLOBAL__N_114k_material_visILi{loop}ELb0EEEvNS_11ShadeParamsE"]   # whole frames: 6 waves (7 measured slower)
        assert k["vgprs"] <= 80 and k["scratch"] == 0, (loop, k)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_geometry_ab_switches_still_compile(tmp_path):
    """the same for geometry.hip's switches: the shadow raster's 32-bit pixel evaluation (measured slower: profiles/r5_t_*), another bounding-box
    limit of the set-up kernel's small-triangle path, the prepass kernels without a wave priority"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "arctic-renderer_amd", "csrc", "geometry.hip")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-ffp-contract=off", "-DARCTIC_RASTER_I32=1", "-DSMALL_PX=256",
                          "-DARCTIC_PREPASS_PRIO=0", "-DARCTIC_RASTER_WGW=1", "-c", src, "-o", str(tmp_path / "geometry_variant.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
