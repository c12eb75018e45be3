"""re_query_boxes_around / re_query_spheres_around at the drop-in boundary, without a GPU: the symbols are exported and declared, the record layout and the
status values are the header's, and the ctypes layer, the Rust binding and the C++ mirror carry them.  The C++ mirror test itself needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("re_query_boxes_around", "re_query_spheres_around")
VALUES = (("RE_AROUND_INCLUDE_SELF", 1), ("RE_AROUND_OK", 0), ("RE_AROUND_NOT_IN_TREE", 1), ("RE_AROUND_TOO_LARGE", 2))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbols_are_exported_and_declared():
    from render_engine_amd import _capi
    L = _capi.load()
    header = re.sub(r"/\*.*?\*/", "", read("include", "re_hip.h"), flags=re.S)
    for call, hit in zip(CALLS, ("re_box_hit", "re_sphere_hit")):
        assert hasattr(L, call) and call in _capi.EXPORTS
        assert re.search(r"\bint\s+" + call + r"\s*\(\s*re_ctx\s*\*ctx,\s*const\s+re_around\s*\*asks,\s*uint32_t\s+n,\s*const\s+re_box_query_args\s*\*args,"
                         r"\s*" + hit + r"\s*\*hits,\s*uint32_t\s+capacity,\s*uint32_t\s*\*n_total,\s*uint8_t\s*\*status\s*\)\s*;", header), call
    for name, value in VALUES:
        assert f"#define {name} {value}u" in header
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+entity_id;\s*float\s+reach;\s*uint32_t\s+flags\s*,\s*reserved\s*;\s*\}\s*re_around\s*;", header)
    assert L.re_abi_version() == 3                                   # additions only, as the siblings'
    tq = read("render_engine_amd", "csrc", "re_treequery.hip")
    assert "k_around_build_boxes" in tq and "k_around_build_spheres" in tq and "k_box_query_around" in tq
    # one record arithmetic for the host builders and the device builder
    assert "box_query_record(" in read("render_engine_amd", "csrc", "re_kernels.h") and "box_query_record(" in tq
    assert "box_query_record(" in read("render_engine_amd", "csrc", "re_api.hip").split("static uint64_t make_box_query(")[1].split("\n}\n")[0]


def test_record_size_and_values():
    from render_engine_amd import _capi
    assert C.sizeof(_capi.Around) == 16 == _capi.AROUND_DT.itemsize
    want = [("entity_id", 0), ("reach", 4), ("flags", 8), ("reserved", 12)]
    assert [(n, _capi.AROUND_DT.fields[n][1]) for n in _capi.AROUND_DT.names] == want
    assert [(n, getattr(_capi.Around, n).offset) for n, _ in _capi.Around._fields_] == want
    assert (_capi.AROUND_INCLUDE_SELF, _capi.AROUND_OK, _capi.AROUND_NOT_IN_TREE, _capi.AROUND_TOO_LARGE) == (1, 0, 1, 2)
    api = read("render_engine_amd", "csrc", "re_api.hip")
    assert "sizeof(re_around) == 16 && sizeof(AroundAsk) == 16" in api      # ... and the library asserts the same of the header's struct
    for name, _ in VALUES:
        assert f"{name} == " in api                                  # ... and that the kernels' constants are the header's


def test_rust_binding_and_cpp_mirror_carry_them():
    ffi = read("integration", "rust", "src", "gpu_visible_set", "ffi.rs")
    assert "pub struct ReAround " in ffi and "// 16 bytes" in ffi.split("pub struct ReAround ")[1].split("\n")[0]
    for call in CALLS:
        assert f"pub fn {call}(" in ffi
    for name, value in VALUES:
        assert re.search(r"pub const " + name + r": u(8|32) = " + str(value) + ";", ffi), name
    mod = read("integration", "rust", "src", "gpu_visible_set", "mod.rs")
    assert "pub fn entities_around" in mod and "ffi::re_query_boxes_around" in mod and "pub fn entities_within_reach" in mod and "ffi::re_query_spheres_around" in mod
    hpp = read("include", "render_engine_hip.hpp")
    assert "struct Around " in hpp and "find_entities_around(" in hpp and "find_entities_within_reach(" in hpp
    for name in CALLS + ("RE_AROUND_INCLUDE_SELF",):
        assert name in hpp
    assert ffi.rstrip() in read("INTEGRATION.md")                    # the block of INTEGRATION.md is the file, verbatim
    assert "(e7)" in read("INTEGRATION.md")
    import render_engine_amd as R
    assert callable(R.Pipeline.find_entities_around) and callable(R.Pipeline.find_entities_within_reach)


def build_shim_test():
    from render_engine_amd import build as libbuild
    here = os.path.join(ROOT, "tests")
    exe = os.path.join(here, "cpp", "_build", "around_query_shim_test")
    lib_dir = os.path.dirname(libbuild.build_library())
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(here, "cpp", "around_query_shim_test.cpp"), "-o", exe, "-L", lib_dir, "-lrender_engine_hip", "-Wl,-rpath," + lib_dir])
    return exe


def test_cpp_mirror_test_compiles():
    assert os.path.exists(build_shim_test())


@pytest.mark.gpu
def test_cpp_mirror_find_entities_around():
    """include/render_engine_hip.hpp: Pipeline::find_entities_around and find_entities_within_reach -- before the first frame, keeping the asker, filtered,
    with an instance registered after frames have run, an ask beyond the cap among answered ones, refused batches (tests/cpp/around_query_shim_test.cpp)"""
    out = subprocess.run([build_shim_test()], capture_output=True, text=True)
    assert out.returncode == 0 and "OK queries asked by entity" in out.stdout, out.stdout + out.stderr
