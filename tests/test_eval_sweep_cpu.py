"""``sweep(indices)`` of the test functions without a GPU, on the C++ backend behind the same C-ABI (THEANET_BACKEND=cpu):
the float32 cases of the GPU test file run against it, and two data-parallel ranks get from one sweep (one collective
over all rows) what they get from one call per minibatch, the same on both ranks."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "theanet_amd", "lib", "libtheanet_cpu.so")
pytestmark = pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")


def _env(**kw):
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    env.update(kw)
    return env


def test_sweep_suite_runs_against_the_cpu_backend():
    """(the CPU backend computes in float32 only: the two 16-bit nets are MI355X-only)"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_eval_sweep.py", "-k", "not float16"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 8, tail             # 3 nets of test_sweep_equals_calls + the 5 other tests


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_two_ranks_sweep_equals_calls(tmp_path, pipe):
    worker = os.path.join(ROOT, "tests", "dp_eval_worker.py")
    stem, port = str(tmp_path / "eval"), _free_port()
    procs = []
    for rank in range(2):
        e = _env(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                 TN_DP_CHECK_ORDER="1", OMP_NUM_THREADS="2", TN_PIPELINE=pipe)
        procs.append(subprocess.Popen([sys.executable, worker, stem, "32", "3"], env=e,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, o.decode()[-3000:]
    r0, r1 = (np.load("%s.rank%d.npz" % (stem, rank)) for rank in range(2))
    for phase in ("a", "b"):
        for r in (r0, r1):
            np.testing.assert_array_equal(r["sweep_" + phase], r["calls_" + phase])
        np.testing.assert_array_equal(r0["sweep_" + phase], r1["sweep_" + phase])
    assert not np.array_equal(r0["sweep_a"], r0["sweep_b"])        # (the steps in between moved the weights)
    assert len(set(r0["sweep_a"][:4, 1].tolist())) == 4            # (rows that cannot be told apart would pin nothing)
