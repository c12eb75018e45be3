"""The host half of the publication protocol (csrc/re_wait.h: poll_word, settle_seal, wait_word, wait_sealed) and the seals and sign-off counts
the kernels share with the host (csrc/re_kernels.h: tick_seal, col_seal, logic_seal, signoff_expect, signoff_top), as a stand-alone g++ program:
no device, no library.  The cases are in tests/cpp/wait_test.cpp."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "render_engine_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "wait_test.cpp")


def build_and_run(name, extra):
    exe = os.path.join(HERE, "cpp", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", CSRC, *extra, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


def test_poll_and_settle_with_the_standard_library_only():
    build_and_run("wait_test", [])


def test_seals_match_their_written_out_formulas():
    # re_kernels.h includes the HIP runtime header (host side only here): taken from the toolchain the library is built with
    from render_engine_amd import build as libbuild
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(hipcc))), "include")
    assert "re_wait.h" in libbuild.HEADERS
    build_and_run("wait_test_seals", ["-DRE_TEST_SEALS", "-D__HIP_PLATFORM_AMD__", "-Wno-unknown-pragmas", "-I", rocm_include])
