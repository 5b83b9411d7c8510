"""The whole-grid 3-D view is wired through every layer: the Rust engine and its C++ twin call
thz_group_session_voxels (not the per-slab thz_session_voxels of local member 0), the twin declares `voxels`, and the
host Makefile builds the twin's voxel self-test (tests/test_gpu_group_voxels.py runs it on the GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _method(src, signature_start):
    i = src.index(signature_start)
    j = src.find("\n    pub fn ", i + 1)
    return src[i:j if j > 0 else len(src)]


def test_rust_engine_voxels_cover_the_whole_group():
    body = _method(_read("rust", "engine.rs"), "pub fn voxels(")
    assert "thz_group_session_voxels(self.session" in body
    assert "thz_session_voxels" not in body.replace("thz_group_session_voxels", "")
    assert "thz_group_session_member" not in body


def test_cpp_twin_has_voxels():
    hpp = _read("thz_image_explorer_amd", "host", "thz_engine.hpp")
    assert re.search(r"\bbool voxels\s*\(", hpp)
    cpp = _read("thz_image_explorer_amd", "host", "thz_engine.cpp")
    body = cpp[cpp.index("bool GpuEngine::voxels("):cpp.index("bool GpuEngine::download_final(")]
    assert body.count("thz_group_session_voxels(session_") == 2


def test_voxel_selftest_is_built_and_ignored():
    mk = _read("thz_image_explorer_amd", "host", "Makefile")
    all_line = next(line for line in mk.splitlines() if line.startswith("all:"))
    assert "../engine_voxel_selftest" in all_line.split()
    assert "engine_voxel_selftest" in _read(".gitignore").split()


def test_ffi_declares_the_group_call():
    ffi = _read("rust", "ffi.rs")
    assert re.search(r"pub fn thz_group_session_voxels\(gs: \*mut ThzGroupSession, cfg: \*const ThzVoxelCfg", ffi)
