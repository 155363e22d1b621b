"""Conv / Pool / Mean layers -- host mirror of theanet/layer/convpool.py.
Same constructor arguments, shape rules and ``representation`` strings; the
compute is enqueued on the HIP backend (include/theanet_hip.h)."""
import math
import numbers
import os
from collections import namedtuple

import numpy as np

from .. import _lib
from ..device import C8_DTYPES, C8Array, c8_pool_pitch, is_c8
from .c8 import DenseDetour, choose_conv
from .layer import Layer, activation_by_name, below_info
from .weights import init_wb


def pool_mask_enabled():
    """TN_POOL_MASK (default on; "0": off): the training forward of a fused fp32 3x3 conv + 2x2 pool block records where
    every pooled value came from, and the backward runs from that mask instead of recomputing the conv outputs.  Read
    where a block is fused (ConvLayer.fuse); NeuralNet puts the same answer into the ranks' agreement."""
    return os.environ.get("TN_POOL_MASK", "1") != "0"


# A fused fp32 conv + act + pool block.  family: whose kernels run it -- "convpool" (the register-resident kernels of
# convpool.hip, few input channels) or "tile" (the LDS-tile matrix-core kernels, wide 3x3 'same' layers); mask: its
# training forward records the pooling mask.  (A 16-bit block -- ConvLayer.c8_fam -- carries None.)
ConvBlock = namedtuple("ConvBlock", "family mask")
# ... its backward, decided when it first runs (ConvLayer._block_route): the entry point, whether that writes the
# gradient w.r.t. the block's input itself (else it leaves dz for tn_conv2d_dgrad), and what the decision was made from
BlockBwd = namedtuple("BlockBwd", "entry writes_dx inputs")
# ... and the geometry arguments every tn_convpool_* / tn_convblock_* entry point ends with
FusedGeom = namedtuple("FusedGeom", "N C H W K f pad Ho Wo p Hp Wp act prm")


class ConvLayer(Layer):
    def __init__(self, inpt, wts, rand_gen,
                 batch_sz, num_prev_maps, in_sz,
                 num_maps, filter_sz, stride,
                 mode='valid',
                 actvn='relu50',
                 reg=(),
                 dtype='float32',
                 conv_shapes='tiled'):
        assert (wts is not None or rand_gen is not None)
        assert mode in ("valid", "full", "same")
        if mode == "full":
            raise NotImplementedError(
                "ConvLayer mode 'full': the reference computes out_sz = in+f+1 "
                "(convpool.py:63-64), which no backend can honour")

        filter_shape = (num_maps, num_prev_maps, filter_sz, filter_sz)
        fan_in = num_prev_maps * filter_sz * filter_sz
        fan_out = num_maps * filter_sz * filter_sz
        self.W, self.b = init_wb(wts, rand_gen, filter_shape, (filter_shape[0], ),
                                 fan_in, fan_out, actvn, 'Conv')

        if mode == 'same':
            assert stride == 1, "For Same mode stride should be 1"
            shift = (filter_sz - 1) // 2
            self.pad_lo, pad_hi = filter_sz - 1 - shift, shift
            self.out_sz = in_sz
        else:
            self.pad_lo, pad_hi = 0, 0
            self.out_sz = in_sz - filter_sz + 1
        self.out_sz //= stride
        theano_out = (in_sz + self.pad_lo + pad_hi - filter_sz) // stride + 1
        assert self.out_sz == theano_out, (
            "stride {} must divide the stride-1 output size {}".format(
                stride, in_sz + self.pad_lo + pad_hi - filter_sz + 1))

        self.act = activation_by_name(actvn)
        assert self.act.kind is not None, "softmax is not a conv activation"
        self.ctx = self.W.ctx
        # ``dtype`` (the net's DTYPE training param; BASELINE configs[4]) 'float16' / 'bfloat16': activations and
        # gradients live in HBM as halfs / bf16 in the c8 layout (device.C8Array), 16-bit MFMA operands / fp32
        # accumulation, fp32 master weights.  Every conv layer of the net runs that way or construction fails -- no
        # silent fp32 run of an unsupported shape.  f16: "16-bit resident", either of the two.
        self.f16 = dtype in C8_DTYPES
        self.c8_dtype = dtype if self.f16 else None
        self.inpt = inpt
        self.batch_sz, self.num_prev_maps, self.in_sz = batch_sz, num_prev_maps, in_sz
        self.filter_sz, self.stride = filter_sz, stride
        if self.f16:
            lib = self.ctx.lib
            # which of the stack's conv families runs the layer, at which pitches its maps are stored (c8.choose_conv:
            # construction fails there for a shape the net's CONV_SHAPES does not let onto the stack)
            self.c8_fam, self.c8_1x1, P, Po = choose_conv(
                lib, dtype, conv_shapes, batch_sz, num_prev_maps, in_sz, inpt.pitch if is_c8(inpt) else None, num_maps,
                filter_sz, stride, mode, self.pad_lo, self.out_sz)
            self.pitch = P
            # the first conv layer of the net gets NCHW fp32 images: packed into a c8 tensor in front of the kernel
            self.x16 = None if is_c8(inpt) else C8Array(self.ctx, batch_sz, num_prev_maps, in_sz, in_sz, dtype, pitch=P)
            self.output = C8Array(self.ctx, batch_sz, num_maps, self.out_sz, self.out_sz, dtype, pitch=Po)
            # the weights as MFMA operand tiles (forward / input gradient): the net arranges every layer's in one launch
            # per step (c8.OperandTiles) and marks them valid until the next update; otherwise the ops do it per call
            self.wt_fwd = self.ctx.empty((lib.tn_c8_wt_elems(num_maps, num_prev_maps, 0),), np.uint16) \
                if self.c8_fam.tiles else None
            self.wt_bwd, self.wt_valid = None, False
        else:
            self.c8_1x1, self.c8_fam = False, None
            self.output = self.ctx.empty((batch_sz, num_maps, self.out_sz, self.out_sz))
        self.gin = None
        self.fused_pool = None     # set by fuse(): conv+act+pool run as ONE kernel
        self.block = None          # ... fp32: the ConvBlock it is
        self._bwd_route = None     # ... and the BlockBwd its backward takes
        self.dz = None

        self.params = [self.W, self.b]
        self.num_maps = num_maps
        self.mode = mode
        self.n_out = num_maps * self.out_sz ** 2
        self.reg = {"L1": 0, "L2": 0,
                    "momentum": .95,
                    "rate": 1,
                    "maxnorm": 0, }
        self.reg.update(reg)

        self.args = (batch_sz, num_prev_maps, in_sz, num_maps, filter_sz,
                     stride, mode, actvn, reg, dtype, conv_shapes)
        self.representation = (
            "Conv Maps:{:2d} Filter:{} Stride:{} Mode:{} Output:{:2d} "
            "Act:{}\n\t  L1:{L1} L2:{L2} Momentum:{momentum} Rate:{rate} Max Norm:{maxnorm}"
            "".format(num_maps, filter_sz, stride, mode, self.out_sz,
                      actvn, **self.reg))

    def TestVersion(self, inpt):
        return ConvLayer(inpt, (self.W, self.b), None, *self.args)

    def act_info(self):
        return self.output, self.act.kind, self.act.prm, None

    def _geom(self):
        return (self.batch_sz, self.num_prev_maps, self.in_sz, self.in_sz, self.num_maps,
                self.filter_sz, self.stride, self.pad_lo, self.out_sz, self.out_sz)

    def can_fuse_with(self, pool):
        """conv -> act -> 2x2 max-pool as one fused kernel pair -- the conv activation never reaches HBM.  Returns the
        family of kernels that runs the block (ConvBlock.family; True on the 16-bit stack), None if it cannot be fused.
        A pool whose stride differs from its window is never fused: the blocks pool with stride = window."""
        if getattr(pool, "strided", False):
            return None
        if self.f16:
            # what the fused block takes; any other PoolLayer of the stack stands alone (c8.check_follows)
            return True if pool.pool_sz == 2 and self.out_sz % 2 == 0 and not pool.c8_alone and self.c8_fam.pools else None
        if self.stride == 1 and self.ctx.lib.tn_convpool_supported(self.num_prev_maps, self.filter_sz, self.stride, pool.pool_sz):
            return "convpool"            # small channel counts (tn_convpool_fwd / tn_convpool_bwd)
        # wide 3x3 'same' layers: the LDS-tile matrix-core kernels pool in their epilogue and run the
        # backward from the pooling mask (tn_convpool_fwd_mask / tn_convpool_bwd_mask_dx)
        if self.ctx.lib.tn_convpool_tile_supported(
                self.batch_sz, self.num_prev_maps, self.in_sz, self.in_sz, self.num_maps, self.filter_sz,
                self.stride, self.pad_lo, self.out_sz, self.out_sz, pool.pool_sz, pool.out_sz, pool.out_sz):
            return "tile"
        return None

    def fuse(self, pool, family):
        """Make this layer and ``pool`` one block of ``family`` (what can_fuse_with answered)."""
        self.fused_pool, pool.fused_conv = pool, self
        if not self.f16:
            # the mask kernels are the 3x3 / 2x2 ones; a tile block has no backward without its mask
            self.block = ConvBlock(family, self.filter_sz == 3 and pool.pool_sz == 2 and
                                   (family == "tile" or pool_mask_enabled()))

    def unfuse(self):
        """Back to two layers with a conv map between them (NeuralNet.get_data_test_model reads it)."""
        assert not self.f16, "DTYPE {}: the conv map of a fused conv + pool block is never materialised".format(self.c8_dtype)
        self.fused_pool.fused_conv = None
        self.fused_pool = self.block = self._bwd_route = None

    def _fused_geom(self):
        pool = self.fused_pool
        return FusedGeom(self.batch_sz, self.num_prev_maps, self.in_sz, self.in_sz, self.num_maps,
                         self.filter_sz, self.pad_lo, self.out_sz, self.out_sz, pool.pool_sz,
                         pool.out_sz, pool.out_sz, self.act.kind, self.act.prm)

    # -- the 16-bit stack: the 16-bit-resident kernels (include/theanet_hip.h, tn_c8_*) ---------------------------
    _c8_prefilled = False

    def _c8_input(self, below=None):
        """The layer's input as a c8 tensor: the layer below's output, or -- first conv layer of the net -- the NCHW
        fp32 minibatch packed on the way in (straight from the dataset window when the layer below is an InputLayer)."""
        if self.x16 is None:
            return self.inpt
        if self._c8_prefilled:
            return self.x16             # written by the distortion stage below (tn_c8_elastic_apply)
        src, row0 = self.inpt, 0
        slot = getattr(self, "_pack_from", None)
        if slot is not None:
            src, row0 = slot.data, int(slot.row0)
        if self.x16.padded:
            self.ctx.call("tn_c8_pack_pitch", src.ptr, row0, self.x16.ptr, self.batch_sz, self.num_prev_maps, self.in_sz,
                          self.pitch, 1.0)
        else:
            self.ctx.call("tn_c8_pack", src.ptr, row0, self.x16.ptr, self.batch_sz, self.num_prev_maps,
                          self.in_sz * self.in_sz, 1.0)
        return self.x16

    def _c8_pad_zero(self, t):
        """After a product that wrote a padded tensor: its pad cells back to zero (tn_c8_pad_zero)."""
        if t.padded:
            self.ctx.call("tn_c8_pad_zero", t.ptr, self.batch_sz, t.c8[0], t.c8[1], t.pitch)

    def _c8_tiles(self, wt):
        """The trailing argument of a product that takes the weights as arranged operand tiles: the tiles while valid."""
        return (wt.ptr if self.wt_valid and wt is not None else None,) if self.c8_fam.tiles else ()

    def _c8_forward(self, out, mask):
        x, fam = self._c8_input(), self.c8_fam
        pooled = out is not self.output
        assert fam.pools or not pooled
        self.ctx.call(fam.fwd, x.ptr, self.W.ptr, self.b.ptr, out.ptr, *((mask.ptr if mask is not None else None,) if fam.pools else ()),
                      *fam.geom, self.act.kind, self.act.prm, *((1 if pooled else 0,) if fam.pools else ()),
                      *self._c8_tiles(self.wt_fwd))
        if fam.pad_zero:
            self._c8_pad_zero(out)

    def _c8_backward(self, gout, need_gin, below):
        """gout: d cost / d z of this layer as a c8 tensor carrying the gradient scale -- or, for a fused block, the
        gradient w.r.t. the POOLED output (act' already applied by its producer), dz being formed from it and the
        pooling mask inside the kernels."""
        pool, fam = self.fused_pool, self.c8_fam
        assert fam.pools or pool is None
        # (a family that pools: whether gout is a pooled gradient, and the block's mask)
        pooled = ((1, pool.mask.ptr) if pool is not None else (0, None)) if fam.pools else ()
        x = self.x16 if self.x16 is not None else self.inpt
        if self.has_updates():
            self.ctx.call(fam.wgrad, x.ptr, gout.ptr, self.grads[0].ptr, self.grads[1].ptr, *fam.geom, *pooled)
        if not need_gin:
            return None
        assert self.x16 is None, "DTYPE {}: no trainable layer below the first conv layer".format(self.c8_dtype)
        if self.gin is None:
            self.gin = C8Array.like(self.inpt)
        b_ptr, b_act, b_prm, b_mask = below_info(below)
        assert b_mask is None
        self.ctx.call(fam.dgrad, gout.ptr, self.W.ptr, self.gin.ptr, *fam.geom, b_ptr, b_act, b_prm, *pooled,
                      *self._c8_tiles(self.wt_bwd))
        if fam.pad_zero:
            self._c8_pad_zero(self.gin)
        return self.gin

    def forward(self, train=True):
        if self.fused_pool is not None:
            return                       # the pool layer launches the fused kernel
        if self.f16:
            return self._c8_forward(self.output, None)
        self.ctx.call("tn_conv2d_fwd", self.inpt.ptr, self.W.ptr, self.b.ptr, self.output.ptr,
                      *self._geom(), self.act.kind, self.act.prm)

    def _block_route(self, need_gin, below):
        """Which backward the fused fp32 block takes.  Decided once, from whether the layer below wants a gradient and an
        activation gradient on it, whether the forward records the pooling mask, and the library's capability queries."""
        pool, lib, g = self.fused_pool, self.ctx.lib, self._fused_geom()
        has_mask = pool.mask is not None
        below_act = need_gin and below_info(below)[0] is not None     # act' of the layer below rides on dx
        inputs = (need_gin, below_act, has_mask)
        if self._bwd_route is not None:
            assert self._bwd_route.inputs == inputs, (self._bwd_route, inputs)
            return self._bwd_route
        if self.block.family == "tile":
            assert has_mask
            route = ("tn_convpool_bwd_mask_dx", True)    # wide block: dW, db and dx from the pooled gradient + mask
        elif has_mask:
            # the forward recorded where every pooled value came from: no conv recompute.  Small maps: weight and input
            # gradients as matrix-core products over an LDS-resident dz, one kernel; else dW, db and dz
            one = self.stride == 1 and lib.tn_convblock_mask_supported(g.C, g.K, g.f, self.stride, g.p, g.H, g.W, g.pad,
                                                                       g.Ho, g.Wo, g.Hp, g.Wp) and not below_act
            route = ("tn_convblock_bwd_mask", True) if one else ("tn_convpool_bwd_mask", False)
            if one:
                # its lane table, complete before the first launch (two steps in flight, a graph capture) reads it.  Host
                # work like an allocation on first use, not a call of the step's schedule: not through ctx.call
                _lib.check(self.ctx.h, lib.tn_convblock_table(self.ctx.h, g.C, g.H, g.W, g.K, g.f, g.pad, g.Ho, g.Wo, g.p,
                                                             g.Hp, g.Wp), "tn_convblock_table")
        elif lib.tn_convblock_supported(g.C, g.K, g.f, self.stride, g.p, g.Ho, g.Wo) and not below_act:
            route = ("tn_convblock_bwd", True)       # LDS-resident recompute: dW, db AND dx in one kernel
        else:
            route = ("tn_convpool_bwd", False)       # recompute; dz only when the layer below needs a gradient
        self._bwd_route = BlockBwd(*route, inputs)
        return self._bwd_route

    def _backward_fused(self, gpool, need_gin, below):
        """gpool = d cost / d (pooled output).  One kernel routes the gradient through max-pool and activation (from
        the pooling mask, or recomputing the windows) and reduces dW/db.  Returns the route and what it wrote: the
        gradient w.r.t. the block's input (route.writes_dx) or dz, None when the layer below needs no gradient."""
        pool, route = self.fused_pool, self._block_route(need_gin, below)
        if need_gin and route.writes_dx and self.gin is None:
            self.gin = self.ctx.empty(self.inpt.shape)
        if need_gin and not route.writes_dx and self.dz is None:
            self.dz = self.ctx.empty(self.output.shape)
        out = (self.gin if route.writes_dx else self.dz) if need_gin else None
        x, W, b, g, y = self.inpt.ptr, self.W.ptr, self.b.ptr, gpool.ptr, pool.output.ptr
        mask = pool.mask.ptr if pool.mask is not None else None
        tile = route.entry == "tn_convpool_bwd_mask_dx"
        head = {"tn_convpool_bwd_mask_dx": (x, W, g, y, mask), "tn_convblock_bwd_mask": (x, W, g, y, mask),
                "tn_convpool_bwd_mask": (x, g, y, mask), "tn_convblock_bwd": (x, W, b, g), "tn_convpool_bwd": (x, W, b, g)}
        # (only the tile block's entry point takes a block without updates -- no dW, db -- and applies act' of the layer below)
        dW, db = (None, None) if tile and not self.has_updates() else (self.grads[0].ptr, self.grads[1].ptr)
        b_ptr, b_act, b_prm, b_mask = below_info(below if need_gin else None)
        assert b_mask is None or not tile
        self.ctx.call(route.entry, *head[route.entry], out.ptr if need_gin else None, dW, db, *self._fused_geom(),
                      *((b_ptr, b_act, b_prm) if tile else ()))
        return route, out

    def backward(self, gout, need_gin, below):
        """gout = d cost / d z of this layer (activation gradient already fused in)."""
        if self.f16:
            return self._c8_backward(gout, need_gin, below)
        if self.fused_pool is not None:
            route, gout = self._backward_fused(gout, need_gin, below)
            if not need_gin or route.writes_dx:
                return gout
        elif self.has_updates():
            self.ctx.call("tn_conv2d_wgrad", self.inpt.ptr, gout.ptr, self.grads[0].ptr,
                          self.grads[1].ptr, *self._geom())
        if not need_gin:
            return None
        if self.gin is None:
            self.gin = self.ctx.empty(self.inpt.shape)
        b_ptr, b_act, b_prm, b_mask = below_info(below)
        assert b_mask is None
        self.ctx.call("tn_conv2d_dgrad", gout.ptr, self.W.ptr, self.gin.ptr, *self._geom(), b_ptr, b_act, b_prm)
        return self.gin


def pool_out_sz(in_sz, pool_sz, stride=None, ignore_border=False):
    """The output side of a PoolLayer on maps of ``in_sz`` pixels (Theano's Pool.out_shape): windows of ``pool_sz`` at
    ``stride`` (None: the window), the last one clipped at the map edge or -- ignore_border -- dropped.  With stride =
    window: in_sz // pool_sz and ceil(in_sz / pool_sz)."""
    st = pool_sz if stride is None else stride
    if st == pool_sz:
        return in_sz // pool_sz if ignore_border else math.ceil(in_sz / pool_sz)
    if ignore_border:
        return (in_sz - pool_sz) // st + 1
    if st >= pool_sz:
        return (in_sz - 1) // st + 1
    return max(0, (in_sz - 1 - pool_sz + st) // st) + 1


class PoolLayer(Layer):
    def __init__(self, inpt, num_maps, in_sz, pool_sz, ignore_border=False, c8_alone=False, stride=None):
        """Max-pool, stride = window.  ignore_border=False keeps the partial last
        window: (5,5) with pool 2 -> (3,3); True -> (2,2) (convpool.py:98-112).
        ``c8_alone`` (16-bit stack, the net's to say: c8.pool_stands_alone): not the second half of a fused conv + pool
        block but a layer of its own (tn_c8_pool_fwd / tn_c8_pool_bwd) -- any window on any map.
        ``stride`` (pool_2d's st=; None: the window): an integer >= 1.  A stride that differs from the window -- windows
        that overlap or leave gaps, clipped at the map edge, never padded -- runs on ops of its own (tn_pool_st_* /
        tn_c8_pool_st_*), never inside a fused block; a stride equal to the window is the layer without the argument."""
        assert stride is None or (isinstance(stride, numbers.Integral) and not isinstance(stride, bool) and stride >= 1), \
            "PoolLayer stride must be an integer >= 1 (None: the window), not {!r}".format(stride)
        self.stride = pool_sz if stride is None else int(stride)
        self.strided = self.stride != pool_sz
        assert not (ignore_border and in_sz < pool_sz and self.strided), (
            "PoolLayer with ignore_border: a window of {} pixels does not fit a map of {}".format(pool_sz, in_sz))
        self.out_sz = pool_out_sz(in_sz, pool_sz, self.stride, ignore_border)

        self.ctx = inpt.ctx
        self.params = []
        self.inpt = inpt
        self.num_maps = num_maps
        self.in_sz, self.pool_sz = in_sz, pool_sz
        self.ignore_border = ignore_border
        self.args = (num_maps, in_sz, pool_sz, ignore_border, c8_alone, stride)
        self.n_out = num_maps * self.out_sz ** 2
        self.batch_sz = inpt.shape[0]
        self.f16 = is_c8(inpt)      # 16-bit stack: pooled c8 tensor (of a fused block, or this layer's own)
        self.c8_alone = self.f16 and c8_alone
        self.below = None           # (stand-alone) the layer below, set by the net: act_info() looks through to it
        assert not (self.f16 and self.strided and not self.c8_alone), \
            "DTYPE {}: a PoolLayer whose stride differs from its window stands alone (c8.pool_stands_alone)".format(inpt.elem)
        if self.c8_alone and self.strided:
            pitch = c8_pool_pitch(self.out_sz)
            self.c8_geom = (self.batch_sz, num_maps, in_sz, inpt.pitch, pool_sz, self.stride, self.out_sz, pitch)
            assert self.ctx.lib.tn_c8_pool_st_supported(*self.c8_geom), (
                "DTYPE {}: a stand-alone PoolLayer takes a window of 2 to 64 pixels at a stride of 1 to 64 that leaves at "
                "least one output pixel, on tensors of fewer than 2^32 - 256 cells (got {} maps of {} pixels at pitch {}, "
                "window {} stride {}, {} border: {} pixels at pitch {})".format(
                    inpt.elem, num_maps, in_sz, inpt.pitch, pool_sz, self.stride, "ignored" if ignore_border else "kept",
                    self.out_sz, pitch))
            self.output = C8Array(self.ctx, self.batch_sz, num_maps, self.out_sz, self.out_sz, inpt.elem, pitch=pitch)
        elif self.c8_alone:
            pitch = c8_pool_pitch(self.out_sz)
            self.c8_geom = (self.batch_sz, num_maps, in_sz, inpt.pitch, pool_sz, self.out_sz, pitch)
            assert self.ctx.lib.tn_c8_pool_supported(*self.c8_geom), (
                "DTYPE {}: a stand-alone PoolLayer takes a window of 2 to 64 pixels that leaves at least one output pixel, "
                "on tensors of fewer than 2^32 - 256 cells (got {} maps of {} pixels at pitch {}, window {}, {} border: "
                "{} pixels at pitch {})".format(inpt.elem, num_maps, in_sz, inpt.pitch, pool_sz,
                                                "ignored" if ignore_border else "kept", self.out_sz, pitch))
            self.output = C8Array(self.ctx, self.batch_sz, num_maps, self.out_sz, self.out_sz, inpt.elem, pitch=pitch)
        elif self.f16:
            self.output = C8Array(self.ctx, self.batch_sz, num_maps, self.out_sz, self.out_sz, inpt.elem,
                                  pitch=inpt.pitch // 2 if inpt.padded else None)
        else:
            self.output = self.ctx.empty((self.batch_sz, num_maps, self.out_sz, self.out_sz))
        self.gin = None
        self.fused_conv = None
        self.mask = None           # uint8 pooling mask of the fused forward (training graphs only)
        self.fused_elastic = None  # ElasticLayer whose resampling this block's forward performs
        self.representation = (
            "Pool Maps:{:2d} Pool_sz:{} Border:{} Output:{:2d}"
            "".format(num_maps, pool_sz,
                      "Ignore" if ignore_border else "Keep",
                      self.out_sz))
        if self.strided:
            self.representation += " Stride:{}".format(self.stride)

    def TestVersion(self, inpt):
        return PoolLayer(inpt, *self.args)

    def act_info(self):
        """16-bit stack: the gradient a pooled block receives carries act'(pooled output) (applied by whichever kernel
        produces it, from the block's stored output); fp32 blocks take the derivative from the pooling mask's sign
        bits inside their own backward kernels instead.  A stand-alone PoolLayer of the stack looks through, the way a
        DropOutLayer does: its own output, with the activation of the block below -- every element its backward hands the
        gradient to equals its window's maximum, so act' taken from the pooled output is act' of that element."""
        if self.c8_alone and self.below is not None:
            _, b_act, b_prm, b_mask = self.below.act_info()
            assert b_mask is None
            return self.output, b_act, b_prm, None
        if self.f16:
            act = self.fused_conv.act
            return self.output, act.kind, act.prm, None
        return Layer.act_info(self)

    def forward(self, train=True):
        conv = self.fused_conv
        if self.c8_alone:
            return self.ctx.call("tn_c8_pool_st_fwd" if self.strided else "tn_c8_pool_fwd", self.inpt.ptr, self.output.ptr,
                                 *self.c8_geom)
        if self.f16:
            if train and self.mask is None:
                self.mask = self.ctx.empty(self.output.shape, np.uint8)
            return conv._c8_forward(self.output, self.mask if train else None)
        if conv is not None:
            if train and self.mask is None and conv.block.mask:
                self.mask = self.ctx.empty(self.output.shape, np.uint8)
            el = self.fused_elastic
            if el is not None and train and el._apply_args is not None:
                # ElasticLayer -> conv -> act -> pool in one launch (the resampled image is still
                # written to el.output for the backward pass)
                a, g = el._apply_args, conv._fused_geom()      # (single channel: the entry point takes no C)
                self.ctx.call("tn_elastic_convpool_fwd_mask", *a.source(), a.N, *a.sample(), conv.W.ptr, conv.b.ptr,
                              self.output.ptr, self.mask.ptr if self.mask is not None else None, g.K, g.f, g.pad, g.Ho,
                              g.Wo, g.p, g.Hp, g.Wp, g.act, g.prm)
                return
            self.ctx.call("tn_convpool_fwd_mask", conv.inpt.ptr, conv.W.ptr, conv.b.ptr,
                          self.output.ptr, self.mask.ptr if (train and self.mask is not None) else None,
                          *conv._fused_geom())
            return
        if self.strided:
            return self.ctx.call("tn_pool_st_fwd", self.inpt.ptr, self.output.ptr, self.batch_sz * self.num_maps, self.in_sz,
                                 self.in_sz, self.pool_sz, self.stride, self.out_sz, self.out_sz)
        self.ctx.call("tn_pool_fwd", self.inpt.ptr, self.output.ptr,
                      self.batch_sz * self.num_maps, self.in_sz, self.in_sz, self.pool_sz,
                      self.out_sz, self.out_sz)

    def backward(self, gout, need_gin, below):
        if not need_gin:
            return None
        if self.fused_conv is not None:
            return gout               # the conv layer's fused backward consumes d cost / d y
        if self.c8_alone:
            # selection only: act' of the block below is already in gout (act_info)
            if self.gin is None:
                self.gin = C8Array.like(self.inpt)
            self.ctx.call("tn_c8_pool_st_bwd" if self.strided else "tn_c8_pool_bwd", self.inpt.ptr, self.output.ptr, gout.ptr,
                          self.gin.ptr, *self.c8_geom)
            return self.gin
        if self.gin is None:
            self.gin = self.ctx.empty(self.inpt.shape)
        _, b_act, b_prm, b_mask = below_info(below)
        assert b_mask is None
        # below.output IS self.inpt, so the activation gradient rides along for free
        if self.strided:
            self.ctx.call("tn_pool_st_bwd", self.inpt.ptr, self.output.ptr, gout.ptr, self.gin.ptr,
                          self.batch_sz * self.num_maps, self.in_sz, self.in_sz, self.pool_sz, self.stride,
                          self.out_sz, self.out_sz, b_act, b_prm)
            return self.gin
        self.ctx.call("tn_pool_bwd", self.inpt.ptr, self.output.ptr, gout.ptr, self.gin.ptr,
                      self.batch_sz * self.num_maps, self.in_sz, self.in_sz, self.pool_sz,
                      self.out_sz, self.out_sz, b_act, b_prm)
        return self.gin


class MeanLayer(Layer):
    def __init__(self, inpt, num_maps, in_sz):
        self.ctx = inpt.ctx
        self.params = []
        self.inpt = inpt
        self.num_maps = num_maps
        self.in_sz = in_sz
        self.out_sz = 1
        self.n_out = num_maps
        self.batch_sz = inpt.shape[0]
        # 16-bit stack: the input is the 16-bit-resident c8 tensor of the conv stack (tn_c8_mean_*); the output stays
        # the fp32 (N, C) matrix the dense layers above take
        self.f16 = is_c8(inpt)
        # ... a padded one (S < pitch) goes through a dense copy, the gradient back into the padded layout
        self.detour = DenseDetour(inpt) if self.f16 else None
        self.output = self.ctx.empty((self.batch_sz, num_maps))
        self.gin = None
        self.representation = (
            "Mean Maps:{:2d} Output:{:2d}"
            "".format(num_maps, self.out_sz))

    def TestVersion(self, inpt):
        return MeanLayer(inpt, self.num_maps, self.in_sz)

    def forward(self, train=True):
        if self.f16:
            self.ctx.call("tn_c8_mean_fwd", self.detour.crop().ptr, self.output.ptr, self.batch_sz, self.num_maps,
                          self.in_sz, self.in_sz)
            return
        self.ctx.call("tn_mean_fwd", self.inpt.ptr, self.output.ptr,
                      self.batch_sz * self.num_maps, self.in_sz * self.in_sz)

    def backward(self, gout, need_gin, below):
        if not need_gin:
            return None
        b_ptr, b_act, b_prm, b_mask = below_info(below)
        assert b_mask is None
        if self.f16:
            # the c8 gradient of the block below (an unpooled ConvLayer, or a fused 2x2 PoolLayer standing for its
            # block): grad_scale * gout / (H W) * act'(its stored output), rounded when stored
            self.ctx.call("tn_c8_mean_bwd", gout.ptr, self.detour.dense_gin().ptr, self.batch_sz, self.num_maps,
                          self.in_sz, self.in_sz, self.detour.act_ptr(b_ptr), b_act, b_prm)
            return self.detour.embed()
        if self.gin is None:
            self.gin = self.ctx.empty(self.inpt.shape)
        self.ctx.call("tn_mean_bwd", gout.ptr, self.gin.ptr, self.batch_sz * self.num_maps,
                      self.in_sz * self.in_sz, b_ptr, b_act, b_prm)
        return self.gin
