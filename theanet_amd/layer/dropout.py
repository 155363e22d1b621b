"""Dropout -- host mirror of theanet/layer/dropout.py.

mask ~ Bernoulli(1 - pdrop), output * mask, NO 1/(1-p) rescale in training;
the test version multiplies by (1 - pdrop) (:28-31).  The stream seed is drawn
from ``rand_gen.randint(1e6)`` at construction exactly like the reference (:10)
so the numpy seed chain stays in step; the mask itself comes from an on-device
Philox4x32-10 generator keyed by (seed, step, GLOBAL element index) -- so it does
not depend on how the batch is sharded over GPUs -- or is injected for parity
tests (``inject_mask``).

DTYPE 'float16' / 'bfloat16': a DropOutLayer between the blocks of the 16-bit-resident conv stack takes and returns
``device.C8Array`` tensors (tn_c8_dropout_fwd / _bwd, tn_c8_scale; theanet_amd/csrc/drop_c8.hip).  The mask is the one the
fp32 layer draws for the same seed, step and LOGICAL (N, C, S, S) shape, kept packed (a byte per 16-byte cell) and drawn
inside the forward launch.  The backward only applies the mask: ``act_info`` looks through to the block below, so the
producer of the incoming gradient has already applied that block's act' (from this layer's own output, which differs from
the block's only where the mask is zero) and rounded once.
"""
import numpy as np

from .. import _lib
from ..device import C8Array, is_c8
from .layer import Layer, below_info


class DropStream:
    """Device-side replacement of ``RandomStreams(seed).binomial(n=1, p=1-pdrop)``."""

    def __init__(self, ctx, shape, pdrop, rand_gen=None):
        self.ctx, self.shape, self.pdrop = ctx, tuple(shape), float(pdrop)
        self.seed = int(rand_gen.randint(1e6)) if rand_gen is not None \
            else int(np.random.randint(0, 1e6))
        self.mask = self._new_mask()
        self.injected = False
        self.ready = False          # mask of the current step already generated (side stream)
        self.d_step = None          # device step counter (set by the net)
        self.elem0 = 0              # global index of this shard's first element

    def _new_mask(self):
        return self.ctx.empty(self.shape, np.uint8)

    def inject(self, mask):
        """Parity hook: use this host mask (0/1) instead of the device RNG.
        Pass None to return to the generator."""
        if mask is None:
            self.injected = False
        else:
            self.mask.set_value(np.asarray(mask).reshape(self.shape).astype(np.uint8))
            self.injected = True

    def generate(self):
        if self.injected:
            return
        if self.ready:              # produced ahead of time by NeuralNet._train_step
            self.ready = False
            return
        self.ctx.call("tn_dropout_mask", self.mask.ptr, self.mask.size, self.pdrop, self.seed,
                      0, self.d_step.ptr if self.d_step is not None else None, self.elem0)


class C8DropStream(DropStream):
    """The stream of a DropOutLayer on a c8 tensor: ``shape`` is the logical (N, C, S, S) one (it keys the numbers and the
    shard offset), ``mask`` the packed bytes (N, ceil(C/8), P, P), bit k = channel 8 * octet + k kept, pad cells 0.  The
    draw happens inside tn_c8_dropout_fwd: nothing is generated ahead of the forward."""

    def __init__(self, ctx, shape, pitch, pdrop, rand_gen=None):
        self.pitch = int(pitch)
        DropStream.__init__(self, ctx, shape, pdrop, rand_gen)

    def _new_mask(self):
        n, c, s, _ = self.shape
        return self.ctx.zeros((n, (c + 7) // 8, self.pitch, self.pitch), np.uint8)

    def inject(self, mask):
        """Parity hook: the same NCHW 0/1 host array the fp32 layer takes, packed to cell bytes.  None: back to the
        generator."""
        if mask is None:
            self.injected = False
            return
        n, c, s, _ = self.shape
        m = np.zeros((n, 8 * ((c + 7) // 8), self.pitch, self.pitch), np.uint8)
        m[:, :c, :s, :s] = np.asarray(mask).reshape(self.shape) != 0
        packed = np.packbits(m.reshape(n, -1, 8, self.pitch, self.pitch), axis=2, bitorder="little")
        self.mask.set_value(np.ascontiguousarray(packed.reshape(self.mask.shape)))
        self.injected = True

    def unpacked(self):
        """The mask of the last forward as the logical NCHW 0/1 array."""
        n, c, s, _ = self.shape
        b = np.asarray(self.mask.get_value(), np.uint8)
        bits = np.unpackbits(b[:, :, None], axis=2, bitorder="little")          # (n, C8, 8, P, P)
        return bits.reshape(n, -1, self.pitch, self.pitch)[:, :c, :s, :s]

    def generate(self):
        raise RuntimeError("the mask of a DropOutLayer on the 16-bit stack is drawn by its forward launch")


def drop_output(layer, output, pdrop, rand_gen=None):
    """dropout.py:9-13 -- attaches a DropStream to ``layer`` for ``output``."""
    layer.drop = DropStream(output.ctx, output.shape, pdrop, rand_gen)
    return layer.drop


class DropOutLayer(Layer):
    def __init__(self, inpt, rand_gen=None, n_in=None, pdrop=0):
        self.ctx = inpt.ctx
        self.inpt = inpt
        self.params = []
        self.n_in, self.n_out = n_in, n_in
        self.pdrop = pdrop
        self.test_scale = 1.0
        self.drop = None
        # 16-bit stack: a 16-bit-resident tensor of the conv stack in, one of the same geometry out
        self.c8 = inpt.c8 if is_c8(inpt) else None
        self.below = None           # (c8) the layer below, set by the net: act_info() looks through to it
        if pdrop and self.c8 is not None:
            c, s, _ = self.c8
            self.drop = C8DropStream(self.ctx, (inpt.shape[0], c, s, s), inpt.pitch, pdrop, rand_gen)
            self.output = C8Array.like(inpt)
        elif pdrop:
            drop_output(self, inpt, pdrop, rand_gen)
            self.output = self.ctx.empty(inpt.shape)
        else:
            self.output = inpt
        self.gin = None
        self.representation = "Drop:{:.0%} Out:{:3d}".format(pdrop, n_in)

    def TestVersion(self, inpt):
        test_version = DropOutLayer(inpt, n_in=self.n_in, pdrop=0)
        if self.pdrop:
            test_version.test_scale = 1 - self.pdrop
            test_version.output = C8Array.like(inpt) if is_c8(inpt) else self.ctx.empty(inpt.shape)
        return test_version

    def _c8_geom(self):
        c, s, _ = self.c8
        return self.inpt.shape[0], c, s, self.inpt.pitch

    def act_info(self):
        """On the 16-bit stack the layer stands for the block below it, the way a fused PoolLayer stands for its block:
        the producer of this layer's incoming gradient applies that block's act', taken from THIS layer's output (the
        block's stored output where the mask keeps it; zero, and a zero gradient after the mask, elsewhere)."""
        if self.c8 is None or self.below is None:
            return Layer.act_info(self)
        _, b_act, b_prm, b_mask = self.below.act_info()
        assert b_mask is None
        return self.output, b_act, b_prm, None

    def forward(self, train=True):
        if self.c8 is not None:
            if self.drop is not None:
                d = self.drop
                self.ctx.call("tn_c8_dropout_fwd", self.inpt.ptr, self.output.ptr, d.mask.ptr, *self._c8_geom(), d.pdrop,
                              d.seed, 0, d.d_step.ptr if d.d_step is not None else None, d.elem0, 0 if d.injected else 1)
            elif self.test_scale != 1.0:
                self.ctx.call("tn_c8_scale", self.inpt.ptr, self.output.ptr, *self._c8_geom(), float(self.test_scale))
            return
        if self.drop is not None:
            self.drop.generate()
            self.ctx.call("tn_scale_mask", self.inpt.ptr, self.drop.mask.ptr, 1.0,
                          self.output.ptr, self.inpt.size, None, _lib.TN_ACT_LINEAR, 0.0)
        elif self.test_scale != 1.0:
            self.ctx.call("tn_scale_mask", self.inpt.ptr, None, float(self.test_scale),
                          self.output.ptr, self.inpt.size, None, _lib.TN_ACT_LINEAR, 0.0)

    def backward(self, gout, need_gin, below):
        if not need_gin:
            return None
        if self.c8 is not None:
            # mask only, in place on the producer's gradient tensor: act' of the block below is already in it (act_info)
            if self.drop is not None:
                self.ctx.call("tn_c8_dropout_bwd", gout.ptr, self.drop.mask.ptr, gout.ptr, *self._c8_geom())
            return gout
        b_ptr, b_act, b_prm, b_mask = below_info(below)
        if self.drop is None and b_ptr is None and b_mask is None:
            return gout
        if self.gin is None:
            self.gin = self.ctx.empty(self.inpt.shape)
        src = gout
        if b_mask is not None:      # layer below is a Hidden layer with its own dropout
            self.ctx.call("tn_scale_mask", src.ptr, b_mask.ptr, 1.0, self.gin.ptr, self.inpt.size,
                          None, _lib.TN_ACT_LINEAR, 0.0)
            src = self.gin
        self.ctx.call("tn_scale_mask", src.ptr, self.drop.mask.ptr if self.drop else None, 1.0,
                      self.gin.ptr, self.inpt.size, b_ptr, b_act, b_prm)
        return self.gin
