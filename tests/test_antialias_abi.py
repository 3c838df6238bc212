"""ARCTIC_OPT_ANTIALIAS / arctic_antialias / arctic_antialias_device on a machine without a GPU: the entry points in the header, the library,
the ctypes binding and the C++ mirror; the option constant; the version; the normative text in the header; what the wrappers refuse before
any device is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"arctic_antialias_device": 5, "arctic_antialias": 5}


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def _header_text():
    return open(os.path.join(ROOT, "include", "arctic_hip.h")).read()


def test_symbols_option_and_version(pkg, lib):
    header = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    L = lib.lib()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == arity, name
        assert name in lib.header_symbols() and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == arity
        call = re.search(name + r"\s*\(([^;]*)\)\s*[;)=]", hpp)
        assert call and len(call.group(1).split(",")) == arity, name
    ids = {n: int(v) for n, v in re.findall(r"#define\s+(ARCTIC_OPT_\w+)\s+(\d+)", _header_text())}
    assert ids["ARCTIC_OPT_ANTIALIAS"] == lib.OPTIONS["antialias"]
    assert list(ids.values()).count(ids["ARCTIC_OPT_ANTIALIAS"]) == 1 and list(lib.OPTIONS.values()).count(lib.OPTIONS["antialias"]) == 1
    assert L.arctic_version() >= 330
    for method in ("antialias", "antialias_device"):
        assert re.search(r"\[\[nodiscard\]\]\s+bool\s+" + method + r"\s*\(", hpp), method
        assert callable(getattr(pkg.renderer.Renderer, method))


def test_header_carries_the_definition():
    """the constants and the tie rules the reference restates are in the header's text"""
    text = re.sub(r"\s*\n \*\s*", " ", _header_text())
    for phrase in ("Y(p) = 77 R + 150 G + 29 B", "K = 12, T_MIN = 4096", "rng < max(T_MIN, hi >> 3)", "horizontal iff eh >= ev", "iff ga >= gb",
                   "2 |e| >= g", "floor(128 (span - 2 d) / span)", "min(256, floor(256 A / (12 rng)))", "(s1 s1 (768 - 2 s1)) >> 16", "(s2 s2 3) >> 10",
                   "(C (256 - off) + Cn off + 128) >> 8", "Alpha is copied", "does NOT apply it", "NOT filtered"):
        assert phrase in text, phrase
    import antialias_reference as AR
    assert (AR.K, AR.T_MIN) == (12, 4096)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no C++ compiler")
def test_cpp_mirror_compiles(lib, tmp_path):
    src = tmp_path / "aa_mirror.cpp"
    src.write_text('#include "renderer.hpp"\n'
                   "bool drive(ArcticAMD::Renderer::Renderer &r, const uint8_t *in, uint8_t *out, const void *d_in, void *d_out) {\n"
                   "    return r.set_antialias(true) && r.antialias(in, 8, 8, out) && r.antialias_device(d_in, d_out, 8, 8) && r.set_antialias(false);\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "arctic-renderer_amd", "host"),
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_handle_and_wrapper_errors(pkg, lib):
    L = lib.lib()
    buf = np.zeros((4, 4, 4), np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.arctic_antialias(None, p, 4, 4, p) == -1
    assert L.arctic_antialias_device(None, p, p, 4, 4) == -1
    assert L.arctic_set_option(None, lib.OPTIONS["antialias"], 1) == -1
    # the wrapper turns ARCTIC_E_INVALID into ArcticError: a handle-less Renderer reaches the entry points' first check
    r = object.__new__(pkg.renderer.Renderer)
    r.L, r.h = L, None
    for call in (lambda: r.antialias(buf), lambda: r.antialias_device(1024, 4096, 4, 4), lambda: r.antialias_device(0, 0, 4, 4)):
        with pytest.raises(pkg.renderer.ArcticError) as e:
            call()
        assert e.value.code == -1
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.uint8), np.zeros((0, 4, 4), np.uint8)):   # refused before the library is called
        with pytest.raises(pkg.renderer.ArcticError) as e:
            r.antialias(bad)
        assert e.value.code == -1


def test_kernel_tile_matches_the_tests():
    """tests/test_gpu_antialias.py sizes three of its inputs by the kernel's tile"""
    text = open(os.path.join(ROOT, "arctic-renderer_amd", "csrc", "common.h")).read()
    m = re.search(r"ANTIALIAS_TILE_W\s*=\s*(\d+)\s*,\s*ANTIALIAS_TILE_H\s*=\s*(\d+)", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (64, 16)
