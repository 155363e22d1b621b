"""The two things every per-op GPU test leans on, checked without a GPU:

  * tests/gpu_util.assert_close rejects NaN (a NaN compares false with every bound, so "err > tol" let an all-NaN
    output pass);
  * every tests/test_gpu_*.py module runs under tests/guard_util.device_guard (guard bands and 0xFF poison around every
    device buffer), and the guard's negative controls (tests/test_gpu_guard.py) pass against the CPU backend."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import guard_util
from tests.gpu_util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "theanet_amd", "lib", "libtheanet_cpu.so")


def test_assert_close_rejects_nan():
    want = np.ones((3, 4))
    with pytest.raises(AssertionError, match=r"12/12 mismatches, 12 of them NaN \(an element never written\?\)"):
        assert_close(np.full((3, 4), np.nan, np.float32), want, what="all NaN")
    got = np.ones((3, 4), np.float32)
    got[1, 2] = np.nan
    with pytest.raises(AssertionError, match=r"one NaN: 1/12 mismatches, 1 of them NaN .* worst at \(1, 2\)"):
        assert_close(got, want, what="one NaN")
    with pytest.raises(AssertionError, match=r"NaN"):
        assert_close(np.float32(np.nan), np.float64(1.0))                   # 0-d, as the cost comparisons are
    with pytest.raises(AssertionError, match=r"NaN"):
        assert_close(got.astype(np.float16), want)
    with pytest.raises(AssertionError):
        assert_close(got, got)                              # a NaN the reference has too is still no match


def test_assert_close_rejects_inf_and_what_is_out_of_tolerance():
    want = np.ones((3, 4))
    for v in (np.inf, -np.inf):
        got = np.ones((3, 4), np.float32)
        got[2, 0] = v
        with pytest.raises(AssertionError, match=r"1/12 mismatches, worst at \(2, 0\)"):
            assert_close(got, want)
    got = np.ones((3, 4), np.float32)
    got[0, 3] = 1.0 + 3e-4                                  # tol = 1e-5 + 1e-4 * 1
    got[0, 1] = 1.0 + 2e-4
    with pytest.raises(AssertionError, match=r"2/12 mismatches, worst at \(0, 3\)"):
        assert_close(got, want)
    got[0, 0] = np.nan                                      # the NaN is the worst of them
    with pytest.raises(AssertionError, match=r"3/12 mismatches, 1 of them NaN .* worst at \(0, 0\)"):
        assert_close(got, want)


def test_assert_close_accepts_exact_and_in_tolerance_values():
    want = np.linspace(-3, 3, 12).reshape(3, 4)
    assert_close(want.astype(np.float32), want.astype(np.float32))
    assert_close(want.astype(np.float32), want)             # float32 rounding of the reference: within rtol 1e-4
    assert_close(want * (1 + 9e-5), want)
    assert_close(want + 9e-6, want, rtol=0)
    assert_close(np.zeros(5), np.full(5, 1e-5))             # on the bound
    assert_close(np.array([np.inf, -np.inf, 1.0]), np.array([np.inf, -np.inf, 1.0]))    # equal infinities match
    with pytest.raises(AssertionError):
        assert_close(np.array([np.inf, 1.0]), np.array([-np.inf, 1.0]))
    with pytest.raises(AssertionError):
        assert_close(want * (1 + 2e-4), want)


def test_assert_close_rejects_a_shape_mismatch():
    with pytest.raises(AssertionError):
        assert_close(np.ones((3, 4)), np.ones((4, 3)))
    with pytest.raises(AssertionError):
        assert_close(np.ones((3, 4)), np.ones((3, 4, 1)))
    with pytest.raises(AssertionError):
        assert_close(np.ones(12), np.ones((3, 4)))


def test_every_gpu_test_module_runs_under_the_device_guard():
    """A module added later cannot silently opt out: the fixture is autouse only where it is imported."""
    modules = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    assert len(modules) >= 21
    missing = []
    for path in modules:
        with open(path) as fh:
            src = fh.read()
        if not re.search(r"^from tests\.guard_util import (?:[\w ,]*\b)?device_guard\b", src, re.M):
            missing.append(os.path.basename(path))
    assert not missing, "no `from tests.guard_util import device_guard` in: %s" % ", ".join(missing)


def test_the_guard_bands_keep_the_allocators_alignment():
    assert guard_util.BAND % 256 == 0 and guard_util.BAND >= 64 * 1024 and guard_util.POISON == 0xFF
    assert np.isnan(np.frombuffer(b"\xff" * 4, np.float32)[0]) and np.isnan(np.frombuffer(b"\xff" * 2, np.float16)[0])
    assert np.frombuffer(b"\xff" * 4, np.int32)[0] == -1


@pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")
def test_guard_negative_controls_on_the_cpu_backend():
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_guard.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 10 and "skipped" not in r.stdout and "error" not in r.stdout.lower(), tail
