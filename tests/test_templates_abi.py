"""The template gallery (frt_matcher_build_templates), the part that needs no GPU: the entry point exists and rejects a NULL source, the shells
offer it, the grouping header (csrc/frt_templates.hpp) groups like a brute-force pass, and the shell demo is well-formed C++11."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd", "csrc")


def test_build_templates_is_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    s = "frt_matcher_build_templates"
    assert s + "(" in header
    assert hasattr(frt.lib, s), "libfrt.so does not export %s" % s
    assert s in frt.ABI and len(frt.ABI[s][1]) == 7, "python binding misses %s" % s
    assert callable(frt.MatMul.buildTemplates)


def test_build_templates_rejects_a_null_source(frt):
    assert frt.lib.frt_matcher_build_templates(None, None, None, None, None, None, None) == frt.FRT_ERR_INVALID
    assert b"null source" in frt.lib.frt_last_error()


def test_shell_headers_offer_the_template_methods():
    mm = open(os.path.join(ROOT, "include", "frt", "matmul.h")).read()
    arc = open(os.path.join(ROOT, "include", "frt", "arcface.h")).read()
    assert "void buildTemplates(MatMul *dst" in mm
    assert "matchTemplates(int k)" in arc and "auditTemplates()" in arc
    assert "frt_matcher_generation(matmul.handle())" in arc.split("void ensureTemplates()")[1].split("}")[0]


def test_kernel_file_is_part_of_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_templates" in mk and "frt_templates.hpp" in mk
    src = open(os.path.join(CSRC, "kernels_templates.hip")).read()
    assert "template_build_kernel" in src
    assert not any(a in src for a in ("atomicAdd", "atomicMax", "atomicMin", "atomicCAS", "atomicExch"))  # the sum order is part of the definition


def test_grouping_header_against_brute_force_under_sanitizers(tmp_path):
    """tests/cpp/template_groups_test.cpp: the header the host side of the build uses, compiled for the host alone with ASan + UBSan."""
    exe = str(tmp_path / "template_groups_test")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "template_groups_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("template groups ok"), (out.returncode, out.stdout, out.stderr)


def test_owned_buffer_type_under_sanitizers(tmp_path):
    """tests/cpp/owned_buf_test.cpp: the buffer type behind every resizable device / pinned allocation (csrc/frt_owned.hpp) on a counting
    malloc policy, as a stand-alone host program with ASan + UBSan (and ASan's leak check at exit)."""
    exe = str(tmp_path / "owned_buf_test")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "owned_buf_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("owned buf ok"), (out.returncode, out.stdout, out.stderr)


def test_template_demo_is_well_formed_cpp11(tmp_path):
    """tests/cpp/template_demo.cpp (run on the GPU by tests/test_gpu_templates.py) under -Wall -Wextra -Werror."""
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "template_demo.cpp"), "-o", str(tmp_path / "template_demo.o")])
