"""re_query_segments at the drop-in boundary, without a GPU: the symbol is exported and declared, the record layouts are the header's, and the Rust
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
    assert hasattr(L, "re_query_segments") and "re_query_segments" in _capi.EXPORTS
    header = re.sub(r"/\*.*?\*/", "", read("include", "re_hip.h"), flags=re.S)
    assert re.search(r"\bint\s+re_query_segments\s*\(\s*re_ctx\s*\*ctx,\s*const\s+re_segment\s*\*segments,\s*uint32_t\s+n,\s*const\s+re_box_query_args\s*\*args,"
                     r"\s*re_segment_hit\s*\*hits,\s*uint32_t\s+capacity,\s*uint32_t\s*\*n_total\s*\)\s*;", header)
    assert "#define RE_SEGMENT_NO_ENTITY 0xFFFFFFFFu" in header
    assert L.re_abi_version() == 3                                   # additions only
    assert "re_treequery.hip" in __import__("render_engine_amd.build", fromlist=["SOURCES"]).SOURCES


def test_record_sizes():
    from render_engine_amd import _capi
    assert C.sizeof(_capi.Segment) == 32 == _capi.SEGMENT_DT.itemsize
    assert C.sizeof(_capi.SegmentHit) == 16 == _capi.SEGMENT_HIT_DT.itemsize
    assert [(n, _capi.SEGMENT_DT.fields[n][1]) for n in _capi.SEGMENT_DT.names] == [("p0", 0), ("p1", 12), ("exclude_entity", 24), ("reserved", 28)]
    assert [(n, _capi.SEGMENT_HIT_DT.fields[n][1]) for n in _capi.SEGMENT_HIT_DT.names] == [("query", 0), ("entity_id", 4), ("t_enter", 8), ("t_exit", 12)]
    assert _capi.SEGMENT_NO_ENTITY == 0xFFFFFFFF
    api = read("render_engine_amd", "csrc", "re_api.hip")
    assert "sizeof(re_segment) == 32 && sizeof(re_segment_hit) == 16" in api      # ... and the library asserts the same of the header's structs


def test_rust_binding_and_cpp_mirror_carry_it():
    ffi = read("integration", "rust", "src", "gpu_visible_set", "ffi.rs")
    assert "pub fn re_query_segments(" in ffi and "pub struct ReSegment " in ffi and "pub struct ReSegmentHit " in ffi and "RE_SEGMENT_NO_ENTITY" in ffi
    assert "// 32 bytes" in ffi.split("pub struct ReSegment ")[1].split("\n")[0] and "// 16 bytes" in ffi.split("pub struct ReSegmentHit ")[1].split("\n")[0]
    mod = read("integration", "rust", "src", "gpu_visible_set", "mod.rs")
    assert "pub fn entities_along_segments" in mod and "ffi::re_query_segments" in mod and "pub fn first_hits" in mod
    hpp = read("include", "render_engine_hip.hpp")
    assert "find_entities_along_segments(" in hpp and "first_hits(" in hpp and "re_query_segments(" in hpp
    assert ffi.rstrip() in read("INTEGRATION.md")                    # the block of INTEGRATION.md is the file, verbatim
    import render_engine_amd as R
    assert callable(R.Pipeline.find_entities_along_segments) and callable(R.first_hits)
