"""bench.py's --dump-outputs writer and its --steps check, without a device."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_writes_float_arrays_exactly(tmp_path):
    b = _bench_module()
    rd = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("score", "<f4"), ("frame", "<i4"),
                   ("match_idx", "<i4"), ("match_sim", "<f4"), ("valid", "<i4")])
    recs = np.zeros(3, rd)
    recs["x1"], recs["y2"] = [1, -2, 2 ** 31 - 1], [7, 8, 9]
    recs["score"], recs["match_idx"], recs["match_sim"], recs["valid"] = [0.5, 0.25, 0.0], [999_999, -1, 0], [0.125, 0.0, -1.0], [1, 0, 1]
    arrays = b.record_arrays(recs)
    arrays["half"] = np.array([1.5, -2.0], np.float16)
    arrays["wide"] = np.array([1e300], np.float64)
    b.dump_outputs(str(tmp_path / "d"), arrays)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert sorted(got) == sorted(arrays)
    assert got["boxes"].dtype == np.float64 and got["boxes"].shape == (3, 4)
    assert np.array_equal(got["boxes"][:, 0], [1, -2, 2 ** 31 - 1]) and np.array_equal(got["boxes"][:, 3], [7, 8, 9])
    assert got["match_idx"].dtype == np.float64 and np.array_equal(got["match_idx"], recs["match_idx"])
    assert got["score"].dtype == np.float32 and np.array_equal(got["score"], recs["score"])
    assert got["match_sim"].dtype == np.float32 and np.array_equal(got["match_sim"], recs["match_sim"])
    assert got["half"].dtype == np.float32 and got["wide"].dtype == np.float64 and got["wide"][0] == 1e300


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    b = _bench_module()
    with pytest.raises(SystemExit):
        b.dump_outputs(str(tmp_path / "d"), {"big": np.zeros((b.DUMP_LIMIT_BYTES // 4) + 1, np.float32)})
    assert not list((tmp_path / "d").glob("*.npy"))


def test_bench_refuses_fewer_than_one_step():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    o = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert o.returncode != 0 and "--steps must be >= 1" in o.stderr and not o.stdout.strip()
