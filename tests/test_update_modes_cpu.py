"""tests/test_gpu_update_modes.py without a GPU, on the C++ backend behind the same C-ABI (THEANET_BACKEND=cpu).  That
library writes the update's roundings with std::fma, so this run checks the reference of tests/upd_ref.py and its
correctly-rounded bound themselves -- every mode and flag, the step counter, the cost rider, tn_step_tail -- before a GPU
is involved.  Nothing is ever recorded in a reductions window there: tn_defer_pending reads 0 and the slab cases carry on
with the gradient the op finished itself."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "theanet_amd", "lib", "libtheanet_cpu.so")
pytestmark = pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")

N_TESTS = 81        # 17 flat + 15 alignment + 17 counter + 4 cost rider + 27 slab cases + 1 step tail


def test_update_modes_match_the_reference_on_the_cpu_backend():
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_update_modes.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == N_TESTS and "skipped" not in r.stdout and "failed" not in r.stdout, tail


def test_cpu_backend_records_nothing():
    """tn_defer_pending of the C++ backend: always 0, and the record is left alone."""
    import ctypes
    from theanet_amd import _lib
    lib = _lib.bind(CPU_LIB, ctypes.RTLD_LOCAL)
    rec = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    assert lib.tn_defer_pending(None, 0, rec) == 0 and list(rec) == [1, 2, 3, 4]
    assert lib.tn_defer_pending(None, -1, None) == 0
