"""CPU-side checks of the entity-logic surface (include/re_hip.h: re_set_entity_types, re_get_entity_type, re_set_entity_logic, re_logic_list): the
built library exports it, the ctypes mirror has the header's record sizes, and the Rust and C++ shims carry it.  No compute calls are made here."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("re_set_entity_types", "re_get_entity_type", "re_set_entity_logic", "re_logic_list")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_library_exports_the_logic_entry_points():
    from render_engine_amd import _capi
    L = _capi.load()
    header = re.sub(r"/\*.*?\*/", "", read("include", "re_hip.h"), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the built library"
        assert name in _capi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/re_hip.h"
        assert getattr(L, name).argtypes is not None
    assert L.re_abi_version() == 3                                   # additions only


def test_record_layouts_match_the_header():
    import numpy as np
    from render_engine_amd import _capi
    assert C.sizeof(_capi.LogicCall) == 8 and C.sizeof(_capi.EntityLogic) == 16
    assert _capi.LOGIC_CALL_DT.itemsize == 8
    assert [_capi.LOGIC_CALL_DT.fields[k][1] for k in ("entity_id", "logic_index", "which", "times")] == [0, 4, 6, 7]
    assert [getattr(_capi.LogicCall, k).offset for k in ("entity_id", "logic_index", "which", "times")] == [0, 4, 6, 7]
    assert (_capi.EntityLogic.type_identifier.offset, _capi.EntityLogic.which.offset) == (0, 8)
    assert (_capi.LOGIC_ENTITY, _capi.LOGIC_RANDOM) == (1, 2)
    header = read("include", "re_hip.h")
    assert "#define RE_LOGIC_ENTITY 1u" in header and "#define RE_LOGIC_RANDOM 2u" in header
    rec = np.zeros(1, _capi.LOGIC_CALL_DT); rec["entity_id"] = 7; rec["logic_index"] = 0x0201; rec["which"] = 3; rec["times"] = 2
    assert rec.tobytes() == bytes([7, 0, 0, 0, 1, 2, 3, 2])             # the 8 bytes k_logic_list stores as one word


def test_shims_carry_the_logic_surface():
    ffi = read("integration", "rust", "src", "gpu_visible_set", "ffi.rs")
    declared = set(re.findall(r"pub fn (re_[a-z_0-9]+)", ffi))
    assert set(SYMBOLS) <= declared, sorted(set(SYMBOLS) - declared)
    assert "pub struct ReLogicCall" in ffi and "pub struct ReEntityLogic" in ffi
    mod = read("integration", "rust", "src", "gpu_visible_set", "mod.rs")
    assert "pub fn logic_calls" in mod and "ffi::re_logic_list" in mod
    hpp = read("include", "render_engine_hip.hpp")
    for name in ("write_entity_type", "remove_entity_type", "register_entity_logic", "logic_calls"):
        assert name in hpp, name
    doc = read("INTEGRATION.md")
    assert "re_logic_list" in doc and "logic_flow.rs:245" in doc


def test_pipeline_mirror_has_the_methods():
    import render_engine_amd as R
    for name in ("set_entity_types", "get_entity_type", "set_entity_logic", "logic_calls"):
        assert callable(getattr(R.Pipeline, name))
    src = read("render_engine_amd", "build.py")
    assert '"re_logic.hip"' in src
