"""The recogniser's dispatch over its whole launch space, without a GPU: tests/cpp/conv_plan_dump.cpp (host code against libfrt.so's
conv_plan) must print tests/golden/arc_conv_plan.txt line for line.  The golden file was written by the same enumeration built against the
commit before conv_plan existed, asking that commit's three walks (conv_kernel_label, conv_small_applies || conv_s2_applies, conv_se_fused
with the per-device occupancy gate taken as passed): a kernel family or instantiation that moves, for any unit shape, launch description
or batch from 1 to 256, changes a line."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")


def test_conv_plan_matches_the_recorded_dispatch(tmp_path):
    exe = str(tmp_path / "conv_plan_dump")
    # host side only, but with hipcc: frt_kernels.h uses clang's vector types
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(PKG, "csrc"),
                           "-x", "c++", os.path.join(ROOT, "tests", "cpp", "conv_plan_dump.cpp"), "-x", "none", "-o", exe, os.path.join(PKG, "libfrt.so"),
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "arc_conv_plan.txt")).read().splitlines()
    assert len(want) > 100
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
