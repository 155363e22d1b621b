"""Worker of tests/test_wt_avg_cpu.py: one rank of a data-parallel job training the small WT_AVG net of
tests/test_gpu_wt_avg.py.  After every step the rank reads its weights and its averages; it stores all of them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_prefix, steps):
    from tests.test_gpu_wt_avg import _flat, _net, _weights
    from theanet_amd import comm
    net, x, y = _net("small")
    world = comm.get_world()
    out = {"a0_%d" % k: a for k, a in enumerate(_flat(net.get_avg_wts()))}
    fn = net.get_trin_model(x, y)
    for s in range(steps):
        fn.enqueue(s % 4)
        for k, (p, a) in enumerate(zip(_weights(net), _flat(net.get_avg_wts()))):
            out["p%d_%d" % (s + 1, k)], out["a%d_%d" % (s + 1, k)] = p, a
    if world.size > 1:
        net._group().verify_order()
    np.savez("%s.r%d.npz" % (out_prefix, world.rank), dp=bool(net._dp), schedule=str(net.dp_schedule),
             averaged=np.array([a is not None for lyr, a in zip(net.tr_layers, net._avg) for _ in lyr.params]), **out)


if __name__ == "__main__":
    from tests import guard_util
    guard_util.install()            # guard bands and 0xFF poison around every device buffer of this rank
    main(sys.argv[1], int(sys.argv[2]))
    guard_util.check_all()
