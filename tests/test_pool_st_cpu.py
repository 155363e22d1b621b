"""PoolLayer ``stride`` (Theano's pool_2d(..., st=): overlapping or gapped max-pooling), the parts that need no GPU: the
output-side rule against torch, the numpy STATEMENT of forward and backward that the GPU tests (tests/test_gpu_pool_st.py,
tests/test_gpu_pool_st_net.py) hold the kernels against, the stack's grammar with and without the keyword, and an fp32
net on the C++ backend (THEANET_BACKEND=cpu, a child process: tests/test_wtcost_cpu.py's manner).

The statement.  Window (i, j) of a p x p, stride st pool covers rows i*st .. min(S, i*st + p) - 1 and the same columns.
Forward: the maximum of the clipped window.  Backward: a position receives gout[i, j] from every window that covers it
and whose maximum equals its value (-0 == +0: a tie; every tied element gets the whole gradient); the terms are added in
the array's own precision in row-major window order, the running sum STARTING from the first term; no term: +0."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "theanet_amd", "lib", "libtheanet_cpu.so")


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def out_side(S, p, st, ignore_border):
    """Theano's Pool.out_shape for S pixels, window p, stride st."""
    if ignore_border:
        assert S >= p
        return (S - p) // st + 1
    if st >= p:
        return (S - 1) // st + 1
    return max(0, (S - 1 - p + st) // st) + 1


def pool_st_fwd(x, p, st, ignore_border=False):
    """(N, C, H, W) -> (N, C, Ho, Wo): the maximum of every clipped window."""
    N, C, H, W = x.shape
    Ho, Wo = out_side(H, p, st, ignore_border), out_side(W, p, st, ignore_border)
    y = np.empty((N, C, Ho, Wo), x.dtype)
    for i in range(Ho):
        for j in range(Wo):
            y[:, :, i, j] = x[:, :, i * st:min(H, i * st + p), j * st:min(W, j * st + p)].max(axis=(2, 3))
    return y


def pool_st_bwd(x, dy, p, st, ignore_border=False):
    """The gradient w.r.t. x, in x's dtype: window by window in row-major order, the sum started by the first term."""
    N, C, H, W = x.shape
    y = pool_st_fwd(x, p, st, ignore_border)
    dy = np.asarray(dy, x.dtype).reshape(y.shape)
    dx = np.zeros_like(x)
    have = np.zeros(x.shape, bool)
    for i in range(y.shape[2]):
        for j in range(y.shape[3]):
            sl = (slice(None), slice(None), slice(i * st, min(H, i * st + p)), slice(j * st, min(W, j * st + p)))
            tie = x[sl] == y[:, :, i:i + 1, j:j + 1]
            term = np.broadcast_to(dy[:, :, i:i + 1, j:j + 1], tie.shape)
            dx[sl] = np.where(tie, np.where(have[sl], dx[sl] + term, term), dx[sl])
            have[sl] |= tie
    return dx


def covered(S, p, st, So):
    """How many windows cover each pixel along one axis."""
    n = np.zeros(S, int)
    for i in range(So):
        n[i * st:min(S, i * st + p)] += 1
    return n


# ---------------------------------------------------------------------------------------------------------------------
# the output side
# ---------------------------------------------------------------------------------------------------------------------
def test_output_side_rule_is_torchs():
    """S = 1..40, p = 2..7, st = 1..8, S >= p (torch refuses a window larger than the map), both border modes: the rule,
    PoolLayer's own function and torch's max_pool2d agree; nothing else is left out."""
    import torch
    import torch.nn.functional as F
    from theanet_amd.layer.convpool import pool_out_sz
    n = 0
    for S in range(1, 41):
        x = torch.zeros(1, 1, S, S)
        for p in range(2, 8):
            for st in range(1, 9):
                if S < p:
                    continue
                for ib in (False, True):
                    want = F.max_pool2d(x, p, st, ceil_mode=not ib).shape[-1]
                    assert out_side(S, p, st, ib) == want == pool_out_sz(S, p, st, ib), (S, p, st, ib)
                    # (a window always starts inside the map)
                    assert (want - 1) * st < S
                    n += 1
    assert n == 3504


def test_output_side_reduces_to_the_old_rule():
    from theanet_amd.layer.convpool import pool_out_sz
    for S in range(1, 41):
        for p in range(1, 9):
            assert pool_out_sz(S, p, p, False) == pool_out_sz(S, p, None, False) == -(-S // p)
            assert pool_out_sz(S, p, p, True) == pool_out_sz(S, p, None, True) == S // p
            if S >= p:
                assert out_side(S, p, p, True) == S // p and out_side(S, p, p, False) == -(-S // p)


# ---------------------------------------------------------------------------------------------------------------------
# the statement against torch, and on ties
# ---------------------------------------------------------------------------------------------------------------------
GEOMS = [(7, 3, 2, False), (7, 3, 2, True), (6, 3, 1, False), (7, 2, 3, False), (7, 2, 3, True), (11, 5, 2, False),
         (8, 2, 1, True), (9, 4, 4, False), (10, 3, 5, False)]


@pytest.mark.parametrize("S,p,st,ib", GEOMS)
def test_statement_equals_torch_on_distinct_values(S, p, st, ib):
    """Distinct inputs: one maximum per window, so torch's autograd states the same sum.  The gradients are small
    multiples of 1/8: their fp32 sums are exact in any order, so the comparison is an equality."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(S * 100 + p * 10 + st)
    x = rng.permutation(2 * 3 * S * (S + 2)).reshape(2, 3, S, S + 2).astype(np.float32) - 50      # (H != W as well)
    xt = torch.tensor(x, requires_grad=True)
    yt = F.max_pool2d(xt, p, st, ceil_mode=not ib)
    y = pool_st_fwd(x, p, st, ib)
    np.testing.assert_array_equal(y, yt.detach().numpy())
    dy = (rng.integers(-16, 17, y.shape) / 8).astype(np.float32)
    yt.backward(torch.tensor(dy))
    np.testing.assert_array_equal(pool_st_bwd(x, dy, p, st, ib), xt.grad.numpy())


@pytest.mark.parametrize("S,p,st,ib", GEOMS)
def test_statement_on_ties(S, p, st, ib):
    """A constant map ties everywhere: every position is credited by every window that covers it, the terms are added
    in row-major window order in fp32 (gradients of mixed exponents make the order visible), uncovered positions are +0."""
    So = out_side(S, p, st, ib)
    x = np.full((1, 1, S, S), -0.0, np.float32)
    x[0, 0, ::2] = 0.0                                         # -0 == +0: still a tie
    rng = np.random.default_rng(S + p + st)
    dy = (rng.standard_normal((1, 1, So, So)) * 10.0 ** rng.integers(-4, 5, (1, 1, So, So))).astype(np.float32)
    got = pool_st_bwd(x, dy, p, st, ib)
    cov = covered(S, p, st, So)
    order_seen = False
    for h in range(S):
        for w in range(S):
            terms = [dy[0, 0, i, j] for i in range(So) for j in range(So)
                     if i * st <= h < i * st + p and j * st <= w < j * st + p]
            assert len(terms) == cov[h] * cov[w]
            if not terms:
                assert got[0, 0, h, w] == 0 and not np.signbit(got[0, 0, h, w])
                continue
            s = terms[0]
            for t in terms[1:]:
                s = np.float32(s + t)
            assert got[0, 0, h, w].tobytes() == np.float32(s).tobytes(), (h, w)
            if len(terms) > 2:
                r = terms[-1]
                for t in terms[-2::-1]:
                    r = np.float32(r + t)
                order_seen |= r != s
    if st > p:
        assert (cov == 0).any()
    if p >= 2 * st:
        assert order_seen                                       # (three or more terms: the order really matters)


def test_single_term_is_copied_bit_for_bit():
    """stride = window: one window per position, and a -0 gradient stays -0 (the sum starts from the term, not from 0)."""
    x = np.arange(16, dtype=np.float32).reshape(1, 1, 4, 4)
    dy = np.array([[[[-0.0, 1.5], [2.5, -0.0]]]], np.float32)
    got = pool_st_bwd(x, dy, 2, 2, False)
    assert np.signbit(got[0, 0, 1, 1]) and np.signbit(got[0, 0, 3, 3]) and got[0, 0, 1, 3] == 1.5
    assert not np.signbit(got[0, 0, 0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# the layer's grammar
# ---------------------------------------------------------------------------------------------------------------------
def _below(kind, out_sz=None, **kw):
    return type(kind, (), dict(out_sz=out_sz, **kw))()


def test_pool_stands_alone_with_and_without_the_keyword():
    from theanet_amd.layer.c8 import pool_stands_alone
    for p in (2, 3, 5):
        for fused in (True, False):
            old = pool_stands_alone(p, fused)
            assert old == (not fused or p != 2)
            assert pool_stands_alone(p, fused, stride=None) == old and pool_stands_alone(p, fused, stride=p) == old
            for st in (1, 2, 3, 4):
                if st != p:
                    assert pool_stands_alone(p, fused, stride=st) is True
    conv = _below("ConvLayer", 8, c8_fam=None)
    assert pool_stands_alone(2, True, conv, True) is False and pool_stands_alone(2, True, conv, True, stride=2) is False
    assert pool_stands_alone(2, True, conv, True, stride=1) is True


def test_check_follows_with_and_without_the_keyword():
    from theanet_amd.layer.c8 import check_follows
    from tests.test_c8_pool_cpu import GRAMMAR
    for below, kind, pool_sz, fused, refusal in GRAMMAR:            # every old answer, spelled three ways
        for kw in ({}, {"stride": None}, {"stride": pool_sz}):
            if refusal is None:
                check_follows("bfloat16", _below(*below), kind, pool_sz, fused, **kw)
            else:
                with pytest.raises(AssertionError, match=refusal):
                    check_follows("bfloat16", _below(*below), kind, pool_sz, fused, **kw)
    # a strided pool stands alone: it follows a Conv, Pool or DropOut layer, whatever the window and the map
    for below in (("ConvLayer", 7), ("ConvLayer", 8), ("PoolLayer", 8), ("DropOutLayer", None)):
        for p, st in ((2, 1), (3, 2), (2, 3)):
            check_follows("bfloat16", _below(*below), "PoolLayer", p, True, stride=st)
    with pytest.raises(AssertionError, match="a stand-alone PoolLayer follows a Conv, Pool or DropOut layer"):
        check_follows("bfloat16", _below("HiddenLayer"), "PoolLayer", 3, True, stride=2)
    # a ConvLayer's own ``stride`` argument is not a pool's
    check_follows("bfloat16", _below("PoolLayer", 4), "ConvLayer", None, True, stride=2)


def test_can_fuse_with_refuses_a_strided_pool():
    """The question is answered before any capability query: neither the fp32 blocks nor the 16-bit block takes it."""
    from theanet_amd.layer.convpool import ConvLayer

    class Lib:
        def __getattr__(self, name):
            raise AssertionError("asked the library: " + name)

    for f16 in (False, True):
        conv = object.__new__(ConvLayer)
        conv.f16, conv.out_sz, conv.stride = f16, 8, 1
        conv.ctx = type("Ctx", (), {"lib": Lib()})()
        conv.c8_fam = type("Fam", (), {"pools": True})()
        assert conv.can_fuse_with(type("Pool", (), dict(pool_sz=2, stride=1, strided=True, c8_alone=True, out_sz=7))()) is None
        if f16:     # ... and the old answer for a 2x2 stride-2 pool, with and without the attribute
            assert conv.can_fuse_with(type("Pool", (), dict(pool_sz=2, c8_alone=False))()) is True
            assert conv.can_fuse_with(type("Pool", (), dict(pool_sz=2, stride=2, strided=False, c8_alone=False))()) is True


# ---------------------------------------------------------------------------------------------------------------------
# an fp32 net on the C++ backend
# ---------------------------------------------------------------------------------------------------------------------
def _suite(select, count):
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_pool_st_net.py", "-k", select],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == count and "skipped" not in r.stdout and "failed" not in r.stdout, tail


@pytest.mark.skipif(not os.path.isfile(CPU_LIB), reason="libtheanet_cpu.so not built")
def test_fp32_strided_pool_net_on_the_cpu_backend():
    """Net b (a (3, 2) pool above a conv, a (2, 3) ignore_border pool): three training steps and the test mode against the
    taught oracle at the fp32 bounds; and the same net with stride = window issues only the old entry points."""
    _suite("(test_strided_pool_nets_match_oracle and float32 and b_) or test_stride_equal_to_window_is_the_old_layer", 2)
