"""Nets with weight costs without a GPU, on the C++ backend behind the same C-ABI (THEANET_BACKEND=cpu): the schedules'
host logic of tests/test_gpu_wtcost_net.py (two steps in flight against one at a time bit for bit, the cost ring, the
optimiser state, the op and the update form) and the data-parallel step, whose weight costs are one tn_wtcost_net call
behind the all-reduce."""
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


def _suite(select, count):
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_wtcost_net.py", "-k", select],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == count and "skipped" not in r.stdout and "failed" not in r.stdout, tail


def test_pipelined_weight_cost_mlp_equals_sequential_on_the_cpu_backend():
    """pipe 1 against 0, both ways of driving the function: every cost, log-probability and weight bit for bit"""
    _suite("test_pipelined_steps_of_weight_cost_nets_equal_sequential and mlp", 2)


def test_cost_ring_of_the_weight_cost_mlp_on_the_cpu_backend():
    _suite("test_cost_ring_of_weight_cost_nets and mlp", 2)


def test_the_rest_of_the_weight_cost_suite_runs_against_the_cpu_backend():
    _suite("not test_pipelined_steps_of_weight_cost_nets_equal_sequential and not test_cost_ring_of_weight_cost_nets", 26)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ranks(prefix, world, port, **env):
    worker = os.path.join(ROOT, "tests", "dp_wtcost_worker.py")
    procs = []
    for rank in range(world):
        e = _env(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                 MASTER_PORT=str(port), TN_DP_CHECK_ORDER="1", OMP_NUM_THREADS="2", **env)
        procs.append(subprocess.Popen([sys.executable, worker, prefix, "4"], env=e, stdout=subprocess.PIPE,
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


def test_two_ranks_with_weight_costs_equal_one(tmp_path):
    """The row losses travel through the all-reduce, every rank adds the weight costs behind it in ONE call: the costs are
    the same on both ranks and those of the one-rank run up to the order of the sums."""
    port = _free_port()
    one, = _ranks(str(tmp_path / "w1"), 1, port + 1, TN_DP_FORCE="1")
    two = _ranks(str(tmp_path / "w2"), 2, port + 2)
    assert all(bool(r["dp"]) for r in [one] + two)
    np.testing.assert_array_equal(two[0]["costs"].view(np.uint32), two[1]["costs"].view(np.uint32))
    np.testing.assert_allclose(two[0]["costs"], one["costs"], rtol=1e-6)
    for r in [one] + two:
        names = list(r["names"])
        assert names.count("tn_wtcost_net") == 1 and "tn_wtcost" not in names
        assert names.index("tn_wtcost_net") > names.index("tn_reduce_sum")
    # ... and a single process without the data-parallel step computes the same costs
    alone, = _ranks(str(tmp_path / "w0"), 1, port + 3)
    assert not bool(alone["dp"]) and "tn_reduce_sum" not in list(alone["names"])
    np.testing.assert_allclose(one["costs"], alone["costs"], rtol=1e-6)
    for k in one.files:
        if k.startswith("w"):
            np.testing.assert_allclose(two[0][k], one[k], rtol=1e-5, atol=1e-6, err_msg=k)
