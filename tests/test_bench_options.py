"""bench.py's options that need no GPU: --dump-outputs' sample (fixed, paired, bounded) and the --steps check."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("esp_bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_a_fixed_paired_sample(tmp_path):
    bench = _bench()
    n = 100000
    arrays = {"colptr": np.arange(1, n // 4 + 2, dtype=np.int64), "rowval": np.arange(n, dtype=np.int64) % 97 + 1,
              "nzval": np.random.default_rng(3).standard_normal(n)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, sample=1000)
    for name, a in arrays.items():
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float64 and 0 < len(x) <= 1000
        assert np.array_equal(x, y)                                  # the same positions from run to run
        assert x[0] == a[0] and x[-1] == a[-1]                       # the first and the last position are always kept
    # rowval and nzval (same length) are sampled at the same positions
    rv, nz = np.load(tmp_path / "a" / "rowval.npy"), np.load(tmp_path / "a" / "nzval.npy")
    pos = np.flatnonzero(np.isin(arrays["nzval"], nz))
    assert np.array_equal(arrays["rowval"][pos].astype(np.float64), rv)
    # short arrays are written whole
    bench.dump_outputs(str(tmp_path / "c"), {"colptr": np.array([1, 3, 4])}, sample=1000)
    assert np.array_equal(np.load(tmp_path / "c" / "colptr.npy"), [1.0, 3.0, 4.0])


def test_dump_outputs_stay_under_64_mib():
    assert 3 * _bench().DUMP_SAMPLE * 8 <= 64 << 20


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--steps" in (r.stderr + r.stdout)
