"""The owners of device and pinned host memory (csrc/re_own.h: DevBuf, Pinned, the live-allocation counter) as a stand-alone g++ program that defines the
HIP allocation functions itself, over malloc: no device, no HIP runtime library.  The cases are in tests/cpp/own_test.cpp."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "render_engine_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "own_test.cpp")


def build_and_run(name, extra):
    from render_engine_amd import build as libbuild
    assert "re_own.h" in libbuild.HEADERS
    # re_own.h includes the HIP runtime API header (declarations only): taken from the toolchain the library is built with
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(hipcc))), "include")
    exe = os.path.join(HERE, "cpp", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-Wno-unknown-pragmas", "-I", CSRC, "-I", rocm_include, *extra, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


def test_buffers_book_count_move_and_free_themselves():
    build_and_run("own_test", [])


def test_the_same_under_address_and_undefined_behaviour_sanitizers():
    build_and_run("own_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"])
