"""WT_AVG without a GPU, on the C++ backend behind the same C-ABI (THEANET_BACKEND=cpu): the net-level cases of
tests/test_gpu_wt_avg.py (the rule step by step, every schedule against one step at a time, evaluation, the switch being
off, checkpoints; the backend computes in float32, so the 16-bit nets stay with the GPU) and the op, and two data-parallel
ranks, each of which keeps the average on its own."""
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

FP32_ONLY = "not float16"           # (matches bfloat16 too)


def _env(**kw):
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    for k in ("TN_DP_FORCE", "TN_DP_OVERLAP", "TN_PIPELINE", "TN_NET_PLAN", "RANK", "WORLD_SIZE"):
        env.pop(k, None)
    env.update(kw)
    return env


def _suite(select, count):
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_wt_avg.py", "-k", select],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == count and "skipped" not in r.stdout and "failed" not in r.stdout, tail


def test_the_op_on_the_cpu_backend():
    _suite("test_avg_net", 24 + 8 + 1)


def test_schedules_keep_the_same_average_on_the_cpu_backend():
    """nine schedules, the plain and the weight-cost net: averages and weights after 40 steps, bit for bit"""
    _suite("test_schedules_keep_the_same_average_bit_for_bit and " + FP32_ONLY, 18)


def test_the_rest_of_the_wt_avg_suite_runs_against_the_cpu_backend():
    _suite("not test_avg_net and not test_schedules_keep_the_same_average_bit_for_bit and " + FP32_ONLY, 10)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


STEPS = 6


def _ranks(prefix, world, port, **env):
    worker = os.path.join(ROOT, "tests", "dp_wt_avg_worker.py")
    procs = []
    for rank in range(world):
        e = _env(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                 MASTER_PORT=str(port), TN_DP_CHECK_ORDER="1", OMP_NUM_THREADS="2", **env)
        procs.append(subprocess.Popen([sys.executable, worker, prefix, str(STEPS)], env=e, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, o.decode()[-3000:]
    return [np.load("%s.r%d.npz" % (prefix, r)) for r in range(world)]


@pytest.mark.parametrize("sched,env", [("pipelined", {"TN_PIPELINE": "1"}),
                                       ("delayed", {"TN_PIPELINE": "0", "TN_DP_OVERLAP": "2"})])
def test_two_ranks_keep_identical_averages_equal_to_one_ranks(tmp_path, sched, env):
    """Every rank applies the rule to its own replica of the weights and exchanges nothing: both ranks hold the same bits
    after every step, and each step's average is the rule applied to that rank's previous average and current weights
    (tests/upd_ref.check_rounded's half-ulp bound).  Against the one-rank run the weights agree up to the order in which
    the all-reduce adds the shards' gradients (tests/test_cpu_backend.py: 1e-5 relative, 1e-6 absolute); an average is a
    convex combination of weight iterates that each meet that bound, so it meets it too."""
    from tests.test_gpu_wt_avg import D, _c, _want
    from tests.upd_ref import check_rounded
    port = _free_port()
    one, = _ranks(str(tmp_path / "w1"), 1, port + 1, TN_DP_FORCE="1", **env)
    two = _ranks(str(tmp_path / "w2"), 2, port + 2, **env)
    assert all(bool(r["dp"]) for r in [one] + two) and str(two[0]["schedule"]) == sched
    averaged = list(one["averaged"])
    assert True in averaged and False in averaged
    for r in [one] + two:
        for s in range(1, STEPS + 1):
            for k, on in enumerate(averaged):
                p, a, prev = r["p%d_%d" % (s, k)], r["a%d_%d" % (s, k)], r["a%d_%d" % (s - 1, k)]
                if on:
                    check_rounded(a, _want(p, prev, _c(D)), what="step %d tensor %d" % (s, k))
                else:
                    np.testing.assert_array_equal(a, p)
    moved = False
    for key in one.files:
        if key[0] in "ap" and key[1].isdigit():
            np.testing.assert_array_equal(two[0][key].view(np.uint32), two[1][key].view(np.uint32), err_msg=key)
            np.testing.assert_allclose(two[0][key], one[key], rtol=1e-5, atol=1e-6, err_msg=key)
            moved = moved or (key.startswith("a%d_" % STEPS) and not np.array_equal(one[key], one["a0_" + key.split("_")[1]]))
    assert moved
