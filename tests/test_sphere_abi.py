"""re_query_spheres at the drop-in boundary, without a GPU: the symbol is exported and declared, the record layouts are the header's, and the Rust
binding and the C++ mirror carry it."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbol_is_exported_and_declared():
    from render_engine_amd import _capi
    L = _capi.load()
    assert hasattr(L, "re_query_spheres") and "re_query_spheres" in _capi.EXPORTS
    header = re.sub(r"/\*.*?\*/", "", read("include", "re_hip.h"), flags=re.S)
    assert re.search(r"\bint\s+re_query_spheres\s*\(\s*re_ctx\s*\*ctx,\s*const\s+re_sphere\s*\*spheres,\s*uint32_t\s+n,\s*const\s+re_box_query_args\s*\*args,"
                     r"\s*re_sphere_hit\s*\*hits,\s*uint32_t\s+capacity,\s*uint32_t\s*\*n_total\s*\)\s*;", header)
    assert "#define RE_SPHERE_NO_ENTITY 0xFFFFFFFFu" in header
    assert L.re_abi_version() == 3                                   # additions only
    assert "re_treequery.hip" in __import__("render_engine_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "k_sphere_query" in read("render_engine_amd", "csrc", "re_treequery.hip")


def test_record_sizes():
    from render_engine_amd import _capi
    assert C.sizeof(_capi.Sphere) == 24 == _capi.SPHERE_DT.itemsize
    assert C.sizeof(_capi.SphereHit) == 16 == _capi.SPHERE_HIT_DT.itemsize
    assert [(n, _capi.SPHERE_DT.fields[n][1]) for n in _capi.SPHERE_DT.names] == [("centre", 0), ("radius", 12), ("exclude_entity", 16), ("reserved", 20)]
    assert [(n, _capi.SPHERE_HIT_DT.fields[n][1]) for n in _capi.SPHERE_HIT_DT.names] == [("query", 0), ("entity_id", 4), ("dist_sq", 8), ("side", 12)]
    assert [(n, getattr(_capi.Sphere, n).offset) for n, _ in _capi.Sphere._fields_] == [("centre", 0), ("radius", 12), ("exclude_entity", 16), ("reserved", 20)]
    assert [(n, getattr(_capi.SphereHit, n).offset) for n, _ in _capi.SphereHit._fields_] == [("query", 0), ("entity_id", 4), ("dist_sq", 8), ("side", 12)]
    assert _capi.SPHERE_NO_ENTITY == 0xFFFFFFFF
    api = read("render_engine_amd", "csrc", "re_api.hip")
    assert "sizeof(re_sphere) == 24 && sizeof(re_sphere_hit) == 16 && sizeof(SphQuery) == 64" in api      # ... and the library asserts the same of the header's structs


def test_rust_binding_and_cpp_mirror_carry_it():
    ffi = read("integration", "rust", "src", "gpu_visible_set", "ffi.rs")
    assert "pub fn re_query_spheres(" in ffi and "pub struct ReSphere " in ffi and "pub struct ReSphereHit " in ffi and "RE_SPHERE_NO_ENTITY" in ffi
    assert "// 24 bytes" in ffi.split("pub struct ReSphere ")[1].split("\n")[0] and "// 16 bytes" in ffi.split("pub struct ReSphereHit ")[1].split("\n")[0]
    mod = read("integration", "rust", "src", "gpu_visible_set", "mod.rs")
    assert "pub fn entities_within_radius" in mod and "ffi::re_query_spheres" in mod and "pub fn nearest_hits" in mod
    hpp = read("include", "render_engine_hip.hpp")
    assert "struct Sphere " in hpp and "find_entities_within_radius(" in hpp and "nearest_hits(" in hpp and "re_query_spheres(" in hpp
    assert ffi.rstrip() in read("INTEGRATION.md")                    # the block of INTEGRATION.md is the file, verbatim
    import render_engine_amd as R
    assert callable(R.Pipeline.find_entities_within_radius) and callable(R.nearest_hits)
