"""frt_embedder_set_flip / _get_flip (include/frt.h, DESIGN "Flip-augmented embeddings"), the part that needs no GPU: the two entry points as the
header, the library and the Python binding declare them, the drop-in shell's methods as C++11, and the kernel file's place in the build."""
import ctypes
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd", "csrc")
GXX = ["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]


def test_flip_is_declared_exported_and_bound(frt):
    header = open(os.path.join(ROOT, "include", "frt.h")).read()
    assert "int frt_embedder_set_flip(frt_embedder *e, int enable);" in header
    assert "int frt_embedder_get_flip(const frt_embedder *e, int *enabled_out);" in header
    for s in ("frt_embedder_set_flip", "frt_embedder_get_flip"):
        assert hasattr(frt.lib, s), "libfrt.so does not export %s" % s
        assert s in frt.ABI and frt.ABI[s][0] is ctypes.c_int and len(frt.ABI[s][1]) == 2, "python binding misses %s" % s
    assert callable(frt.ArcFaceIR50.setFlip) and isinstance(frt.ArcFaceIR50.flip, property)
    # the contract, in the header: one mode for gallery and probes
    block = header[header.index("Flip-augmented embeddings"):header.index("int frt_embedder_set_flip(")]
    assert "Gallery and probes must be embedded in the same mode" in " ".join(block.replace("\n *", " ").split())


def test_flip_rejects_null_arguments(frt):
    on = ctypes.c_int(7)
    assert frt.lib.frt_embedder_set_flip(None, 1) == frt.FRT_ERR_INVALID
    assert b"null argument" in frt.lib.frt_last_error()
    assert frt.lib.frt_embedder_get_flip(None, ctypes.byref(on)) == frt.FRT_ERR_INVALID
    assert frt.lib.frt_embedder_get_flip(None, None) == frt.FRT_ERR_INVALID
    assert on.value == 7


def test_shell_methods_compile_as_cpp11(tmp_path):
    src = tmp_path / "flip_shell.cpp"
    src.write_text('#include "frt/arcface.h"\n'
                   "bool flipOnThenOff(ArcFaceIR50 &rec) {\n"
                   "    rec.setFlipAugment(true);\n"
                   "    const ArcFaceIR50 &c = rec;\n"
                   "    const bool on = c.flipAugment();\n"
                   "    rec.setFlipAugment(false);\n"
                   "    return on && !rec.flipAugment();\n"
                   "}\n")
    subprocess.check_call(GXX + ["-c", str(src), "-o", str(tmp_path / "flip_shell.o")])


def test_kernel_file_is_part_of_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_arc_flip" in mk
    src = open(os.path.join(CSRC, "kernels_arc_flip.hip")).read()
    for k in ("arc_flip_pair_kernel", "fc_finalize_pair_kernel", "void launch_arc_flip_pair(", "void launch_arc_flip_mirror(", "void launch_fc_finalize_pair("):
        assert k in src
