"""Worker of tests/test_wtcost_cpu.py: one rank of a data-parallel job training a net with weight costs (the 3flat-like
MLP of tests/test_gpu_wtcost_net.py).  Every rank stores the costs of its steps; rank 0 the weights after the last one and
the entry points its last step called."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_prefix, steps):
    from tests.test_gpu_wtcost_net import _net
    from theanet_amd import comm
    net, x, y = _net("mlp")
    fn = net.get_trin_model(x, y)
    world = comm.get_world()
    costs = [float(fn(s % 4)[0]) for s in range(steps - 1)]
    names, real = [], net.ctx.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    net.ctx.call = spy
    costs.append(float(fn((steps - 1) % 4)[0]))
    net.ctx.call = real
    wts = [w for l in net.tr_layers for w in l.get_wts()]
    if world.size > 1:
        net._group().verify_order()
    np.savez("%s.r%d.npz" % (out_prefix, world.rank), costs=np.array(costs, np.float32), names=np.array(names),
             dp=bool(net._dp), **{"w%d" % i: w for i, w in enumerate(wts)})


if __name__ == "__main__":
    from tests import guard_util
    guard_util.install()            # guard bands and 0xFF poison around every device buffer of this rank
    main(sys.argv[1], int(sys.argv[2]))
    guard_util.check_all()
