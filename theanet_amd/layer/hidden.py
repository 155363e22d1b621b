"""Fully-connected layer -- host mirror of theanet/layer/hidden.py.

a = act(x . W + b), W is (n_in, n_out); optional non-inverted dropout on the
output (:31-32); the test version drops the mask and scales by (1 - pdrop)
(:50-55).  Note the reference's init quirk: fan_in = fan_out = n_in + n_out (:21-27).
"""
from .. import _lib
from ..device import is_c8
from .c8 import DenseDetour
from .dropout import drop_output
from .layer import Layer, activation_by_name, below_info
from .weights import init_wb


class HiddenLayer(Layer):

    def __init__(self, inpt, wts,
                 rand_gen=None,
                 n_in=None,
                 n_out=None,
                 pdrop=0,
                 actvn='relu01',
                 reg=()):
        assert wts is not None or rand_gen is not None

        try:
            fan_in_out = n_in + n_out
        except TypeError:
            fan_in_out = None

        self.w, self.b = init_wb(wts, rand_gen, (n_in, n_out), (n_out,),
                                 fan_in_out, fan_in_out, actvn, 'Hid')
        n_in, n_out = self.w.shape
        self.ctx = self.w.ctx

        self.act = activation_by_name(actvn)
        # 16-bit stack: the layer above the conv stack consumes the c8 tensor as it is stored (tn_c8_fc_* / tn_c8_fcg_*:
        # 16-bit operands through the NCHW row map, fp32 output); further dense layers are fp32 like the reference
        self.c8 = inpt.c8 if is_c8(inpt) else None
        self.c8_head = False
        if self.c8 is not None:
            c, h, wd = self.c8
            assert c * h * wd == n_in, (self.c8, n_in)
            # the family is picked once: the tiled products where they take the shape (a multiple of 64 c8 inputs and of
            # 32 outputs), the general ones (tn_c8_fcg_*: any shape) otherwise -- same arguments, same arithmetic
            lib, shape = self.ctx.lib, (inpt.shape[0], c, h * wd, n_out)
            self.c8_fc = "tn_c8_fc" if lib.tn_c8_fc_supported(*shape) else \
                "tn_c8_fcg" if lib.tn_c8_fcg_supported(*shape) else None
            assert self.c8_fc is not None, (
                "DTYPE {}: a dense layer of {} samples on {} maps of {}x{} with {} outputs is beyond what the 16-bit dense "
                "products index (tn_c8_fcg_supported: fewer than 2^31 input, output and weight elements)".format(
                    inpt.elem, inpt.shape[0], c, h, wd, n_out))
            # an output head (OutputLayer.is_head) of at most 16 outputs: the affine map on the head kernels (head_c8.hip;
            # TN_C8_HEAD 0: never).  A plain HiddenLayer never takes them; the gradients are the family's above either way
            self.c8_head = bool(getattr(self, "is_head", False) and lib.tn_c8_head_supported(*shape))
            # a padded stack tensor (maps stored at a pitch > their side): the products read a dense copy, cropped in
            # front of them; the input gradient is embedded back into the padded layout
            self.detour = DenseDetour(inpt)
            self.inpt = self.detour.dense
            self.c8_src = inpt if inpt.padded else None
        else:
            self.inpt = inpt.flatten(2)
            assert self.inpt.shape[1] == n_in, (self.inpt.shape, n_in)
        self.batch_sz = self.inpt.shape[0]
        # the forward ops and the shape they take
        self._fc = (self.c8_fc, (self.batch_sz, c, h * wd, n_out)) if self.c8 is not None else \
            ("tn_fc", (self.batch_sz, n_in, n_out))
        self.output = self.ctx.empty((self.batch_sz, n_out))
        self.drop = None
        self.test_scale = 1.0
        if pdrop:
            drop_output(self, self.output, pdrop, rand_gen)
        self.gin = None
        self.wgrad_ws = None

        self.params = [self.w, self.b]
        self.n_in, self.n_out = n_in, n_out
        self.actvn = actvn
        self.pdrop = pdrop
        self.reg = {"L1": 0, "L2": 0,
                    "momentum": .95,
                    "maxnorm": 0,
                    "rate": 1}
        self.reg.update(reg)

        self.representation = (
            "Hidden In:{:3d} Out:{:3d} Act:{} Drop%:{}"
            "\n\t  L1:{L1} L2:{L2} Momentum:{momentum} Max Norm:{maxnorm} "
            "Rate:{rate}".format(n_in, n_out, actvn, pdrop, **self.reg))

    def TestVersion(self, inpt):
        test_version = HiddenLayer(inpt, (self.w, self.b),
                                   pdrop=0,
                                   actvn=self.actvn)
        test_version.test_scale = 1 - self.pdrop
        return test_version

    def act_info(self):
        return (self.output, self.act.kind, self.act.prm,
                self.drop.mask if self.drop is not None else None)

    def forward(self, train=True):
        drop, (op, shape) = self.drop, self._fc
        if self.c8 is not None:
            self.detour.crop()
        if drop is not None and not drop.injected and not drop.ready:
            # the mask is drawn inside the layer's own launch (and kept for the backward pass)
            self.ctx.call(op + "_fwd_dropout", self.inpt.ptr, self.w.ptr, self.b.ptr, self.output.ptr, *shape,
                          self.act.kind, self.act.prm, drop.mask.ptr, drop.pdrop, drop.seed, 0,
                          drop.d_step.ptr if drop.d_step is not None else None, drop.elem0)
        else:
            if drop is not None:
                drop.generate()
            self.ctx.call(op + "_fwd", self.inpt.ptr, self.w.ptr, self.b.ptr, self.output.ptr, *shape,
                          self.act.kind, self.act.prm, drop.mask.ptr if drop is not None else None)
        if self.test_scale != 1.0:
            self.ctx.call("tn_scale_mask", self.output.ptr, None, float(self.test_scale),
                          self.output.ptr, self.output.size, None, _lib.TN_ACT_LINEAR, 0.0)

    def affine(self, act_kind, act_prm):
        """output = act(x . W + b) for an output head built on this layer (its row kernel follows): tn_fc_fwd on an fp32
        input; on a stack tensor the layer's 16-bit product -- the head kernel (``c8_head``) or the dense family's forward
        -- in front of which a padded tensor is cropped."""
        if self.c8 is None:
            self.ctx.call("tn_fc_fwd", self.inpt.ptr, self.w.ptr, self.b.ptr, self.output.ptr,
                          self.batch_sz, self.n_in, self.n_out, act_kind, act_prm, None)
            return
        self.detour.crop()
        if self.c8_head:
            self.ctx.call("tn_c8_head_fwd", self.inpt.ptr, self.w.ptr, self.b.ptr, self.output.ptr, *self._fc[1],
                          act_kind, act_prm)
        else:
            self.ctx.call(self.c8_fc + "_fwd", self.inpt.ptr, self.w.ptr, self.b.ptr, self.output.ptr, *self._fc[1],
                          act_kind, act_prm, None)

    def backward(self, gout, need_gin, below):
        """gout = d cost / d z (activation gradient and dropout mask already applied)."""
        if self.c8 is not None:
            shape = self._fc[1]
            if self.has_updates():
                self.ctx.call(self.c8_fc + "_wgrad", self.inpt.ptr, gout.ptr, self.grads[0].ptr, self.grads[1].ptr, *shape)
            if not need_gin:
                return None
            b_ptr, b_act, b_prm, b_mask = below_info(below)
            assert b_mask is None
            self.ctx.call(self.c8_fc + "_dgrad", gout.ptr, self.w.ptr, self.detour.dense_gin().ptr, *shape,
                          self.detour.act_ptr(b_ptr), b_act, b_prm)
            return self.detour.embed()
        upd = self.has_updates()
        if upd and self.wgrad_ws is None:
            nbytes = self.ctx.lib.tn_fc_wgrad_ws_bytes(self.batch_sz, self.n_in, self.n_out)
            self.wgrad_ws = self.ctx.empty((nbytes + 3) // 4)
        if not need_gin:
            if upd:
                self.ctx.call("tn_fc_wgrad", self.inpt.ptr, gout.ptr, self.grads[0].ptr,
                              self.grads[1].ptr, self.batch_sz, self.n_in, self.n_out, self.wgrad_ws.ptr)
            return None
        if self.gin is None:
            self.gin = self.ctx.empty(self.inpt.shape)
        b_ptr, b_act, b_prm, b_mask = below_info(below)
        b_mask = b_mask.ptr if b_mask is not None else None
        if upd:
            # weight gradient and input gradient only share dz: one op, one launch
            self.ctx.call("tn_fc_bwd", self.inpt.ptr, gout.ptr, self.w.ptr, self.grads[0].ptr,
                          self.grads[1].ptr, self.gin.ptr, self.batch_sz, self.n_in, self.n_out,
                          self.wgrad_ws.ptr, b_ptr, b_act, b_prm, b_mask)
        else:
            self.ctx.call("tn_fc_dgrad", gout.ptr, self.w.ptr, self.gin.ptr, self.batch_sz, self.n_in,
                          self.n_out, b_ptr, b_act, b_prm, b_mask)
        return self.gin
