"""What the launch-alone checks share on the Python side (the C++ side: tests/cpp/check_common.hpp): the one compile line for the host programs
under tests/cpp/, the runner that starts a harness process under its own timeout and ends a module at the first process error, the reader of
results.txt, and the writer of the op list that the named-guarded-buffer programs (det_tail_check, match_stage_check, match_exact_check) run."""
import os
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "face-recognition-cpp-tensorrt_amd")


def build(outdir, program, opt="-O1"):
    """Compiles tests/cpp/<program>.cpp (host C++ against libfrt.so) into outdir; returns the path."""
    exe = os.path.join(str(outdir), program)
    # host side only, but with hipcc: frt_kernels.h uses clang's vector types
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", opt, "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(PKG, "csrc"),
                           "-x", "c++", os.path.join(ROOT, "tests", "cpp", program + ".cpp"), "-x", "none", "-o", exe, os.path.join(PKG, "libfrt.so"),
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


class Runner:
    """One per test module: a harness process that ends on a HIP error, a signal or its timeout ends the module - the tests behind it fail with
    its message and launch nothing."""

    def __init__(self):
        self.stopped = []  # the message of the harness process that ended on an error

    def require_running(self):
        assert not self.stopped, "not run: an earlier harness process ended on an error: " + self.stopped[0]

    def run(self, exe, workdir, label, timeout):
        """Runs `exe workdir`; the caller reads what the process left, then calls require_ended_well()."""
        try:
            run = subprocess.run([exe, str(workdir)], capture_output=True, text=True, timeout=timeout)
            if run.returncode != 0:
                self.stopped.append("%s: exit status %d: %s" % (label, run.returncode, run.stderr.strip()[-500:]))
        except subprocess.TimeoutExpired:
            self.stopped.append("%s: no end after %d s" % (label, timeout))

    def require_ended_well(self):
        assert not self.stopped, self.stopped[0]


def read_results(dirname):
    """results.txt of a harness process: id -> the remaining columns (strings); {} when the process wrote none."""
    path = os.path.join(str(dirname), "results.txt")
    if not os.path.exists(path):
        return {}
    return {ln.split("\t")[0]: ln.split("\t")[1:] for ln in open(path).read().splitlines()}


def rng(*what):
    return np.random.default_rng([zlib.crc32(str(w).encode()) for w in what])


def fbits(x):
    return int(np.array(x, np.float32).view(np.uint32))


def bit_diff(name, got, want):
    """[] or one message: two arrays compared bit for bit"""
    if got is None:
        return ["%s was not written" % name]
    want = np.ascontiguousarray(want)
    if got.size != want.size:
        return ["%s: %d elements, expected %d" % (name, got.size, want.size)]
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    ne = got.view(bits).reshape(-1) != want.view(bits).reshape(-1)
    if ne.any():
        i = int(np.argmax(ne))
        return ["%s: %d of %d values differ, first at flat index %d: %r, reference %r" % (name, ne.sum(), ne.size, i, got.reshape(-1)[i], want.reshape(-1)[i])]
    return []


class Ops:
    """The operation list of one harness process (DIR/ops.txt, read by run_ops in tests/cpp/check_common.hpp) and the files it names."""

    def __init__(self, dirname):
        self.dir, self.lines, self.cases = str(dirname), [], []

    def case(self, cid):
        self.cases.append(cid)
        self.lines.append("case " + cid)
        self.cid = cid

    def _file(self, name, arr):
        fn = "%s.%s.in" % (self.cid, name)
        np.ascontiguousarray(arr).tofile(os.path.join(self.dir, fn))
        return fn

    def buf(self, name, nbytes, arr=None):
        self.lines.append("buf %s %d %s" % (name, nbytes, "-" if arr is None else self._file(name, arr)))

    def rbuf(self, name, arr):
        self.lines.append("rbuf %s %d %s" % (name, arr.nbytes, self._file(name, arr)))

    def op(self, *a):
        self.lines.append(" ".join(str(v) for v in a))

    def dump(self, name, tag=""):
        fn = "%s.%s%s.out" % (self.cid, name, tag)
        self.lines.append("dump %s %s" % (name, fn))
        return fn

    def end(self):
        self.lines.append("end")

    def write(self):
        with open(os.path.join(self.dir, "ops.txt"), "w") as f:
            f.write("\n".join(self.lines) + "\n")

    def read(self, fn, dtype):
        p = os.path.join(self.dir, fn)
        return np.fromfile(p, dtype) if os.path.exists(p) else None

    def results(self):
        return {cid: int(cols[0]) for cid, cols in read_results(self.dir).items()}
