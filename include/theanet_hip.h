/*
 * theanet_hip.h -- C-ABI of libtheanet_hip.so: the MI355X (gfx950) compute backend
 * that replaces Theano underneath theanet's convolutional training hot path.
 *
 * The reference (rakeshvar/theanet) has no FFI: its boundary to the compute
 * backend is "build a Theano graph, call theano.function".  Every entry point
 * below therefore cites the *reference call site into Theano* it replaces
 * (paths relative to the reference root).  The Python host package
 * (theanet_amd/) binds these with ctypes; see INTEGRATION.md for the stub.
 *
 * Conventions
 *  - plain C symbols, plain pointers and sizes; no C++/torch types.
 *  - every function returns int: 0 = ok, <0 = error (TN_E_*); the message is
 *    available from tn_last_error(ctx) (ctx may be NULL for creation errors).
 *  - one ctx <-> one device <-> one HIP stream.  All ops ENQUEUE on that stream
 *    and return immediately; tn_sync / tn_d2h wait.  A ctx is not thread-safe;
 *    distinct ctxs are independent.
 *  - all tensors float32, NCHW, row-major, device pointers from tn_alloc.
 *    Labels int32.  Masks uint8 (0/1).
 *  - "d_*" scalar-pointer arguments are DEVICE pointers (may be NULL -> the
 *    by-value sibling is used) so a captured HIP graph can be replayed with
 *    per-step values changed on the device.
 */
#ifndef THEANET_HIP_H
#define THEANET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TN_OK 0
#define TN_E_HIP (-1)     /* a HIP runtime call failed            */
#define TN_E_ARG (-2)     /* invalid argument / unsupported shape */
#define TN_E_COMM (-3)    /* RCCL failure                         */
#define TN_E_NOMEM (-4)

/* activation kinds -- theanet/layer/layer.py:27-39 (activation_list) */
enum tn_act {
    TN_ACT_LINEAR = 0,
    TN_ACT_LEAKY = 1,       /* relu / relu00..relu99: max(0,z)+min(0,z)*slope   */
    TN_ACT_TANH = 2,
    TN_ACT_SIGMOID = 3,
    TN_ACT_SOFTPLUS = 4,
    TN_ACT_SCALED_TANH = 5  /* 1.7*tanh(2z/3)                                   */
};

typedef struct tn_ctx tn_ctx;

/* ---- lifecycle (replaces: theano device init; neuralnet.py:236 theano.function) ---- */
int tn_version(void);
/* "TN_<name>=<value>" of every environment switch (theanet_amd/csrc/knobs.h) that data-parallel ranks must agree on,
 * as this process resolved it: space-separated, in table order, NUL-terminated.  TN_E_ARG if len is too small. */
int tn_knobs(char* buf, int len);
int tn_device_count(int* count);
int tn_ctx_create(int device, tn_ctx** ctx);
int tn_ctx_destroy(tn_ctx* ctx);
const char* tn_last_error(tn_ctx* ctx);
int tn_sync(tn_ctx* ctx);
/* Two streams per context: 0 = main (the dependent chain), 1 = side (leaf work such as weight
 * gradients, which only the update needs).  tn_stream_select picks the stream the following
 * ops are enqueued on; tn_stream_wait(w, s) makes stream w wait for everything enqueued on s
 * so far.  Both calls are legal inside tn_graph_begin/_end (cross-stream capture).           */
int tn_stream_select(tn_ctx* ctx, int idx);
int tn_stream_wait(tn_ctx* ctx, int waiter, int signaler);
/* name_len bytes are written to name; cus = compute units; hbm_bytes = total memory */
int tn_device_info(tn_ctx* ctx, char* name, int name_len, int* cus, size_t* hbm_bytes);

/* ---- memory (replaces: theano.shared / get_value; train.py:18-19, weights.py:18-22,78-79) ---- */
int tn_alloc(tn_ctx* ctx, size_t bytes, void** dptr);
int tn_free(tn_ctx* ctx, void* dptr);
int tn_h2d(tn_ctx* ctx, void* dst, const void* src, size_t bytes);   /* returns after the copy */
int tn_d2h(tn_ctx* ctx, void* dst, const void* src, size_t bytes);   /* returns after the copy */
/* Outputs a caller reads every step (the [cost, features, logprob] of neuralnet.py:236-240's function) leave
 * as soon as they exist: tn_d2h_early orders a copy into page-locked host memory (tn_host_alloc) behind the
 * work enqueued so far on the current stream and runs it on a copy stream, under the kernels enqueued
 * afterwards; tn_copy_sync waits for every such copy.                                                   */
int tn_host_alloc(tn_ctx* ctx, size_t bytes, void** out);
int tn_host_free(tn_ctx* ctx, void* p);
int tn_d2h_early(tn_ctx* ctx, void* host_dst, const void* src, size_t bytes);
int tn_copy_sync(tn_ctx* ctx);
/* the same copy with an event (tn_event_create) recorded behind it on the copy stream: the host waits for THAT copy
 * (tn_event_sync) instead of for all of them -- a step's cost picked up a few steps later by train.py's loop
 * (theanet_amd/trainfn.py _CostLedger; polling the destination instead is not an option: a 4-byte copy was observed
 * half-written from the host) */
int tn_d2h_early_ev(tn_ctx* ctx, void* host_dst, const void* src, size_t bytes, void* done_event);
int tn_d2d(tn_ctx* ctx, void* dst, const void* src, size_t bytes);   /* enqueued                */
int tn_memset(tn_ctx* ctx, void* dst, int byte_value, size_t bytes); /* enqueued                */
int tn_set_u32(tn_ctx* ctx, uint32_t* d_dst, uint32_t value);        /* enqueued scalar store   */
int tn_set_i64(tn_ctx* ctx, int64_t* d_dst, int64_t value);
int tn_set_f32(tn_ctx* ctx, float* d_dst, float value);
int tn_add_u32(tn_ctx* ctx, uint32_t* d_dst, uint32_t inc);          /* *d_dst += inc (step counter) */

/* ---- a whole step as ONE call (the coarse entry point for launch-bound steps) ----
 * A plan is the flat list of the C-ABI calls a step makes -- entry point + argument block -- built once by the host
 * (theanet_amd/plan.py records the calls of a few ordinary steps of a NeuralNet function, checks that they repeat and
 * which integer arguments follow the minibatch index) and replayed by tn_net_step without the interpreter: what the
 * reference's compiled theano.function does for fn(i) (neuralnet.py:236-241).  tn_net_plan_add: name = an entry point
 * of this header taking the context first (the context is not in the list); kinds[k] = 0 pointer / integer (vals[k] =
 * the value as 64 bits, strides[k] added per unit of tn_net_step's index), 1 float (its 32 bits), 2 double (its 64
 * bits); at most 48 integer and 8 floating-point arguments.  tn_net_step issues the calls in order and stops at the
 * first error.  The plan holds raw pointers: it lives no longer than the buffers of the net it was recorded from. */
int tn_net_plan_create(tn_ctx* ctx, void** plan);
int tn_net_plan_add(tn_ctx* ctx, void* plan, const char* name, int nargs, const uint8_t* kinds, const uint64_t* vals,
                    const int64_t* strides);
int tn_net_step(tn_ctx* ctx, void* plan, int64_t index);
int tn_net_plan_size(tn_ctx* ctx, void* plan);
int tn_net_plan_destroy(tn_ctx* ctx, void* plan);

/* ---- HIP graph capture of an op sequence issued through this ABI ---- */
int tn_graph_begin(tn_ctx* ctx);                   /* start stream capture            */
int tn_graph_end(tn_ctx* ctx, void** graph_exec);  /* stop, instantiate               */
int tn_graph_launch(tn_ctx* ctx, void* graph_exec);
int tn_graph_destroy(tn_ctx* ctx, void* graph_exec);

/* ---- timing with HIP events on the ctx stream (bench.py roofline leg) ---- */
int tn_event_create(tn_ctx* ctx, void** ev);
int tn_event_record(tn_ctx* ctx, void* ev);
int tn_event_wait(tn_ctx* ctx, void* ev);            /* the current stream waits for the event */
int tn_event_elapsed_ms(tn_ctx* ctx, void* ev_start, void* ev_stop, float* ms); /* syncs on stop */
int tn_event_destroy(tn_ctx* ctx, void* ev);
/* non-blocking: *done = 1 once everything recorded in front of the event has finished, else 0 (watchdogs
 * that must raise instead of hanging: the communicator self-test of theanet_amd/comm.py)              */
int tn_event_query(tn_ctx* ctx, void* ev, int* done);
int tn_event_sync(tn_ctx* ctx, void* ev);            /* the HOST waits for the event */

/* ---- conv (replaces nnconv.conv2d + tt.grad through it; convpool.py:54-72, layer.py:83) ----
 * True convolution (kernel flipped), W layout (K,C,f,f):
 *   z[n,k,i,j] = b[k] + sum_{c,u,v} xpad[n,c,i*s+u,j*s+v] * W[k,c,f-1-u,f-1-v]
 * pad_lo zeros are virtually prepended to rows/cols (0 for 'valid', f-1-(f-1)/2 for
 * 'same'); Ho/Wo are the output sizes the caller computed (convpool.py:57-70).
 * fwd fuses bias + activation:  a = act(z).                                         */
int tn_conv2d_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a,
                  int N, int C, int H, int Wd, int K, int f, int stride, int pad_lo,
                  int Ho, int Wo, int act, float act_param);
/* dW (K,C,f,f) and db (K) from dz = dcost/dz (activation gradient already applied by
 * the kernel that produced dz).  OVERWRITES dW/db.                                   */
int tn_conv2d_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db,
                    int N, int C, int H, int Wd, int K, int f, int stride, int pad_lo,
                    int Ho, int Wo);
/* dx (N,C,H,W) = full correlation of dz with W.  If prev_a != NULL the gradient of the
 * producing layer's activation is fused:  dx *= act'(prev_a)  (prev_a = that layer's
 * OUTPUT, same shape as dx) -- i.e. the result is already dcost/dz of the layer below. */
int tn_conv2d_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx,
                    int N, int C, int H, int Wd, int K, int f, int stride, int pad_lo,
                    int Ho, int Wo, const float* prev_a, int prev_act, float prev_act_param);

/* ---- DTYPE 'float16' / 'bfloat16' (BASELINE configs[4]; the reference is float32-only, weights.py:8 `floatX`: opt-in
 * training params of this build, default off) ----
 * dtype 0: every tensor fp32 (reference arithmetic).  dtype 1: the conv stack of the net lives in HBM as halfs and is
 * served by the tn_c8_* / tn_fc8_* entry points below; the fp32-tensor conv entry points (tn_conv2d_*, tn_convpool_*)
 * REFUSE to run in this mode (TN_E_ARG: never a silent fp32 run inside a float16 net).  grad_scale (a power of two,
 * e.g. 4096): gradient tensors of the stack hold fp16(grad_scale * g) so that small gradients do not fall into
 * fp16's subnormal range; the fp32 epilogues of the weight gradients remove the factor.
 * dtype 2: the same with bf16 cells -- every tn_c8_* / tn_fc8_* entry point reads and writes bf16 (same signatures,
 * layout, kernels and schedule; bf16 MFMA, round-to-nearest-even when a tensor is stored), the fp32-tensor conv entry
 * points refuse as in dtype 1.  bf16 has fp32's exponent range: grad_scale is still honoured (a power of two scales
 * exactly), the host passes 1.  In dtypes 0 and 1 the c8 entry points use halfs; the CPU backend refuses dtypes != 0. */
int tn_set_matmul_dtype(tn_ctx* ctx, int dtype, float grad_scale);
int tn_get_matmul_dtype(tn_ctx* ctx);
/* MATMUL 'bf16x3' (opt-in, this build's extension; the reference is float32, weights.py:8): mode 1 runs the products of
 * tn_fc_fwd / tn_fc_wgrad / tn_fc_dgrad / tn_fc_bwd of layers with more than 16 outputs as six bf16 MFMA products of
 * exactly split operands (x = x0 + x1 + x2, 8 mantissa bits each) with fp32 accumulation -- fp32-grade accuracy
 * (the same tolerances hold), not the same bits as mode 0's exact fp32 MFMA.  theanet_amd/csrc/gemm_b3.hip.
 * MATMUL 'bfloat16' (opt-in): mode 2 runs the products of tn_fc_fwd / tn_fc_fwd_dropout / tn_fc_wgrad / tn_fc_dgrad /
 * tn_fc_bwd of EVERY shape (ragged edges are masked in the kernel; nothing falls back to fp32) with both operands
 * rounded to bf16 (nearest even) as they are staged, exact products, fp32 accumulation on v_mfma_f32_32x32x16_bf16 and
 * the fp32 epilogues of mode 0 -- the arithmetic of the 16-bit conv stack; tensors in memory stay fp32, db is the fp32
 * column sum of dz, tn_fc_fwd_dropout draws tn_dropout_mask's bits.  A reduced-precision mode (~2^-9 relative per
 * operand).  The output heads stay fp32 by design: tn_fc_softmax_train / tn_fc_softmax_nll (also where they fall back
 * to the generic products), tn_softmax_nll*, tn_head_rows.  theanet_amd/csrc/gemm_bf16.hip.
 * Modes other than 0 / 1 / 2 are refused; the CPU backend accepts 0 only.                                          */
int tn_set_fc_matmul(tn_ctx* ctx, int mode);
/* CONV 'bfloat16' (opt-in, this build's extension; the reference's conv products are float32, convpool.py:54-72): mode 2
 * runs tn_conv2d_fwd / tn_conv2d_wgrad / tn_conv2d_dgrad -- the call sites convpool.py:54-72 and their gradients -- of
 * EVERY geometry those entry points take (any N, C, K, any square filter, 'valid' / 'same', any stride, any map size;
 * nothing falls back to the fp32 kernels) with both operands rounded to bf16 (nearest even) as they are staged, exact
 * products, fp32 accumulation on v_mfma_f32_32x32x16_bf16 and the fp32 epilogues of mode 0 (bias + activation; act' of
 * prev_a, NULL: none).  Tensors in memory stay fp32 NCHW; db is the fp32 sum of the unrounded dz; the weight gradient's
 * pixel slabs meet in context scratch and are summed in slab order (no atomics: the same call gives the same bits).  A
 * reduced-precision mode (~2^-9 relative per operand).  theanet_amd/csrc/conv_bf16.hip.  In mode 2 the three entry points
 * answer TN_E_ARG by name, nothing launched, for a NULL tensor, a dimension < 1 and shapes whose index arithmetic would
 * overflow 32 bits (N*C*H*W, N*K*Ho*Wo or K*C*f*f >= 2^31).  Mode 0 issues exactly the calls issued without this entry
 * point.  The fused block entry points (tn_convpool_*, tn_convblock_*, tn_elastic_convpool_*) are NOT part of the mode:
 * they compute in fp32 whatever it is, and a net under CONV 'bfloat16' does not use them.  Mode 2 is refused (TN_E_ARG)
 * while a 16-bit DTYPE is set (tn_set_matmul_dtype 1 / 2: that stack already runs 16-bit products); modes other than
 * 0 / 2 are refused (they are numbered as tn_set_fc_matmul numbers them); the CPU backend accepts 0 only.           */
int tn_set_conv_matmul(tn_ctx* ctx, int mode);

/* ---- DTYPE 'float16' on fp16-RESIDENT tensors (theanet_amd/csrc/conv_c8.hip, fc_c8.hip) --------------------
 * (DTYPE 'bfloat16', tn_set_matmul_dtype mode 2: everything below with bf16 in place of half; the shape predicates and
 * tn_c8_conv_plan do not depend on the element type.)
 * BASELINE.json configs[4]: "fp16 inputs / fp32 accum MFMA".  The reference is float32-only (weights.py:8); these
 * entry points replace the same Theano call sites as tn_conv2d_* / tn_fc_* (convpool.py:54-72,106-107; hidden.py:30;
 * layer.py:83) for nets built with training param DTYPE = 'float16'.  Activations and the gradients flowing down
 * the net live in HBM as IEEE halfs in the "c8" layout: logical (N, C, H, W) stored [N][ceil(C/8)][H][W][8]
 * (16-byte cell = the 8 channels of an octet at one pixel; channels beyond C are zero).  Master weights, biases,
 * weight gradients, velocities stay fp32.  Gradient tensors hold grad_scale * g (tn_set_matmul_dtype's grad_scale, a
 * power of two; scaled where the first fp16 gradient is produced, removed in the fp32 epilogues of the weight
 * gradients).  Arithmetic: operands rounded to half (nearest-even), exact products, fp32 accumulation; bias,
 * activation and pooling on the fp32 sums; one rounding when a tensor is stored.  Pooling masks: one byte per pooled
 * value in the same [N][K/8][H/2][W/2][8] order, bits 0-3 = window elements (2*di+dj) equal to the maximum (all of
 * them on a tie, Theano's MaxPoolGrad), bit 4 / 5 = pooled value > 0 / < 0.                                      */
int tn_c8_conv_supported(int N, int C, int H, int W, int K, int f, int stride, int pad);
int tn_c8_conv_wgrad_supported(int N, int C, int H, int W, int K);
/* wt (tn_c8_conv_fwd / _dgrad): the layer's weights as fp16 MFMA operand tiles, prepared beforehand by
 * tn_c8_arrange_multi into a buffer of tn_c8_wt_elems halfs -- every conv product of a step in ONE launch -- or NULL:
 * the op arranges them itself (one small launch per call).  The arrangement is a function of W only: redo it after
 * every update.                                                                                                    */
typedef struct tn_c8_wt_seg {
    const float* W;  /* (K, C, 3, 3) master weights */
    void* wt;        /* tn_c8_wt_elems(K, C, dgrad) halfs */
    int K, C, dgrad; /* dgrad != 0: the operand tiles of the input-gradient product */
    int pad_;
} tn_c8_wt_seg;
size_t tn_c8_wt_elems(int K, int C, int dgrad);
int tn_c8_arrange_multi(tn_ctx* ctx, const tn_c8_wt_seg* segs, int nseg);
int tn_c8_conv_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, uint8_t* mask, int N, int C,
                   int H, int Wd, int K, int act, float prm, int pool, const void* wt);
/* dx = conv^T(dz, W) * act'(prev_a) (prev_a NULL: none; for a pooled block below, prev_a is its POOLED output and dx
 * has that shape: the gradient a pooled block receives always carries act'(pooled output)).  pooled != 0: dz is not a
 * tensor: the `dz` argument is the pooled gradient (N, K, H/2, W/2) and dz = (bit of the window element in the block's
 * mask) ? pooled gradient : 0 is formed while staging: the conv activation, MaxPoolGrad's output and dz never exist
 * in HBM                                                                                                            */
int tn_c8_conv_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int H, int Wd, int K,
                     const void* prev_a, int prev_act, float prev_prm, int pooled, const uint8_t* mask, const void* wt);
int tn_c8_conv_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int H, int Wd,
                     int K, int pooled, const uint8_t* mask);
/* Which kernel instantiation a call of this shape launches -- the launchers' own selection, made without a context
 * (the current device's CU count; 256 where no GPU answers).  op 0: tn_c8_conv_fwd, 1: tn_c8_conv_dgrad (act / prm:
 * the layer below's), 2: tn_c8_conv_wgrad (act / prm unused); pool: the fused 2x2 max-pool / pooled-gradient form.
 * Writes up to nout ints to out and returns how many the plan has; TN_E_ARG when the call would refuse the shape
 * (and always on the CPU backend).
 *   op 0, 1: FT, MODE, NS, LK, TK (c8_conv_kernel<FT, MODE, NS, LK, TK>), NI images per pixel tile, RT pixel tiles per
 *            image, KT filter tiles, MT pixel tiles
 *   op 2:    form (1: c8_wgrad_tr_kernel<NCT, NGX, POOL, ROLL>, 0: c8_wgrad_kernel<NFT, NCT, POOL, NGX, TM, ROLL>), NFT,
 *            NCT, NGX, TM, ROLL, nstage, NI, S slabs, tiles per slab, tiles, KG filter groups, CG channel groups */
int tn_c8_conv_plan(int op, int N, int C, int H, int W, int K, int pool, int act, float prm, int* out, int nout);
/* fully-connected products on an fp16-resident input (replaces hidden.py:30 and its gradients, layer.py:83, for the
 * first dense layer above a c8 conv stack; theanet_amd/csrc/fc_c8.hip): x16 (B, ceil(C/8)*HW*8) halfs is the flattened
 * c8 tensor of C maps of HW pixels (HW = 1: a plain half matrix), W (C*HW, n_out) fp32 keeps the reference's
 * NCHW-flattened row order (neuralnet.py:168-173) and is walked through the row map; the layer output a and dz are
 * fp32.  dgrad writes fp16(grad_scale * dz . W^T * act'(y16)) in x's order (y16 = output of the layer below, NULL:
 * none); wgrad removes the scale.                                                                                */
int tn_c8_fc_supported(int B, int C, int HW, int n_out);
int tn_c8_fc_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C, int HW, int n_out,
                 int act, float act_param, const uint8_t* mask);
/* ... with the layer's dropout mask drawn in the same launch (dropout.py:10-13; the numbers of tn_dropout_mask with the
 * same seed / step / elem0) and written to mask_out for the backward pass.                                          */
int tn_c8_fc_fwd_dropout(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C, int HW,
                         int n_out, int act, float act_param, uint8_t* mask_out, float pdrop, uint64_t seed, uint32_t step,
                         const uint32_t* d_step, uint64_t elem0);
int tn_c8_fc_dgrad(tn_ctx* ctx, const float* dz, const float* W, void* dx, int B, int C, int HW, int n_out, const void* y,
                   int act, float act_param);
int tn_c8_fc_wgrad(tn_ctx* ctx, const void* x, const float* dz, float* dW, float* db, int B, int C, int HW, int n_out);
/* The same products for ANY layer shape (theanet_amd/csrc/fcg_c8.hip): the tiled family above wants the c8 input length
 * ceil(C/8)*HW*8 a multiple of 64 and n_out a multiple of 32 (tn_c8_fc_supported) and keeps those shapes; a HiddenLayer
 * whose shape it refuses (n_out 500, 32 maps of 7x7, ...) takes tn_c8_fcg_*.  Argument for argument tn_c8_fc_*, and the same
 * arithmetic: x as stored, W rounded nearest-even to the element type E (half or bf16) while it is loaded through the row
 * map k -> (8 o + e) * HW + p, dz as E(grad_scale * dz), exact products, fp32 accumulation on the 32x32x16 matrix core; a,
 * dW, db fp32 (OVERWRITE, the gradient scale removed); dgrad stores E(acc * act'(y16)) (y16 NULL: E(acc)) in c8 order and
 * writes EVERY c8 cell of dx, channels past C as exact +0.  A ragged reduction tail is fed as zeros, a ragged output tail
 * is not stored, rows of W for channels past C are never read, and no alignment of n_out is assumed for W, b, mask, a
 * or dz.  fwd_dropout draws tn_dropout_mask's bits for the logical (B, n_out) matrix at any elem0 and any n_out; its
 * masked output equals tn_c8_fcg_fwd with that mask bit for bit.  No atomics: K slabs (forward) and sample slabs (weight
 * gradient) meet in context scratch in a fixed order, the same call gives the same bits.
 * supported: 1 for every B, C, HW, n_out >= 1 with, Kc = ceil(C/8)*HW*8: B*Kc, B*n_out and C*HW*n_out < 2^31,
 * (Kc/8)*HW < 2^32, B and n_out at most 65535 * 64.  Anything else, or a NULL x, W, b, a, dz, dx, dW, db (mask_out for
 * fwd_dropout): TN_E_ARG by name, nothing launched.                                                                  */
int tn_c8_fcg_supported(int B, int C, int HW, int n_out);
int tn_c8_fcg_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C, int HW, int n_out,
                  int act, float act_param, const uint8_t* mask);
int tn_c8_fcg_fwd_dropout(tn_ctx* ctx, const void* x, const float* W, const float* b, float* a, int B, int C, int HW,
                          int n_out, int act, float act_param, uint8_t* mask_out, float pdrop, uint64_t seed, uint32_t step,
                          const uint32_t* d_step, uint64_t elem0);
int tn_c8_fcg_dgrad(tn_ctx* ctx, const float* dz, const float* W, void* dx, int B, int C, int HW, int n_out, const void* y,
                    int act, float act_param);
int tn_c8_fcg_wgrad(tn_ctx* ctx, const void* x, const float* dz, float* dW, float* db, int B, int C, int HW, int n_out);
/* An output head on the 16-bit stack (training param STACK_HEAD 'any'; theanet_amd/csrc/head_c8.hip): the affine map of a
 * head with at most 16 outputs read straight from the c8 tensor, each op ONE launch (no slab scratch, no finishing kernel)
 * -- the stack's counterpart of tn_fc_fwd / tn_fc_softmax_nll for <= 16 classes.  tn_c8_fcg_fwd's arithmetic, argument for
 * argument: x the dense flattened c8 tensor as stored, (B, Kc) elements, Kc = ceil(C/8)*HW*8; W (C*HW, n_out) fp32 in NCHW
 * row order, walked through the row map k -> (8 o + e) * HW + p and rounded nearest-even to the element type as it is
 * loaded; exact products, fp32 accumulation on the 16x16x32 matrix core; bias and activation on the fp32 sum; z fp32.  Rows
 * of W for channels past C are never read, nothing is read or written past an operand, no alignment of n_out is assumed.
 * No atomics: the same call gives the same bits.
 * head_fwd: z = act(x . W16 + b) (the heads' activations: linear, sigmoid, scaled_tanh; any TN_ACT_* code).
 * head_softmax_nll: logits = x . W16 + b -- tn_c8_head_fwd's linear z bit for bit -- and tn_softmax_nll's statement on
 *   them in the same launch: logprob, rowloss, pred (the first maximum), rowp, dz = (softmax - onehot) * inv_batch; labels
 *   y[y_row0 + *d_row0 + row] (d_row0 NULL: 0); y, rowloss, rowp and dz may be NULL as in tn_fc_softmax_nll (without y
 *   the other three must be).
 * supported: 1 for 1 <= n_out <= 16 within tn_c8_fcg_supported's index limits (0 for every shape with TN_C8_HEAD=0 in the
 *   environment: heads then take the dense families' forward and the row kernels).  Anything else, or a NULL x, W, b, z /
 *   logits, logprob or pred: TN_E_ARG by name, nothing launched.
 * plan (no device): op 0 (head_fwd) / 1 (head_softmax_nll) -> instantiation (= op), row tiles of 16 samples (blocks),
 *   reduction steps of 4 cells, waves of a block (1 to 16, from the steps alone: they split the steps into contiguous runs
 *   and meet in a fixed order), steps of the busiest wave, padding rows of the last tile, padding cells of the last step,
 *   padding channels of the last octet, HW == 1; returns how many values the plan has, TN_E_ARG for a refused shape (and
 *   always on the CPU backend).                                                                                       */
int tn_c8_head_supported(int B, int C, int HW, int n_out);
int tn_c8_head_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, float* z, int B, int C, int HW, int n_out,
                   int act, float act_param);
int tn_c8_head_softmax_nll(tn_ctx* ctx, const void* x, const float* W, const float* b, float* logits, int B, int C, int HW,
                           int n_out, const int32_t* y, int64_t y_row0, const int64_t* d_row0, float* logprob,
                           float* rowloss, int32_t* pred, float* rowp, float* dz, float inv_batch);
int tn_c8_head_plan(int op, int B, int C, int HW, int n_out, int* out, int nout);
/* NCHW fp32 (rows row0.. of a dataset) -> c8 fp16 and back; values are multiplied by scale                        */
int tn_c8_pack(tn_ctx* ctx, const float* x, int64_t row0, void* out, int N, int C, int HW, float scale);
/* tn_elastic_apply (below; inlayers.py:126-142) whose output is the c8 tensor the first conv layer consumes: the same
 * values, rounded to halfs when stored -- the resampled fp32 minibatch is neither written nor re-read by tn_c8_pack.  */
int tn_c8_elastic_apply(tn_ctx* ctx, const float* x, int64_t x_row0, const int64_t* d_row0, void* out16,
                        int N, int C, int h, int w, int invert, int nearest, const int32_t* map_idx,
                        const float* map_fy, const float* map_fx, float pflip, const uint8_t* flipmask,
                        uint64_t seed, uint32_t step, const uint32_t* d_step, int64_t row_global0);
int tn_c8_unpack(tn_ctx* ctx, const void* x, float* out, int N, int C, int HW, float scale);
/* MeanLayer on a c8 tensor (replaces tt.mean(inpt, axis=(2,3)) and its gradient, convpool.py:129-144, for a Mean layer
 * on top of the 16-bit stack; theanet_amd/csrc/mean_c8.hip).  fwd: y (N, C) fp32 row-major = the fp32 mean over H x W of
 * the STORED values of x (not rounded: the input of the fp32 dense layers above).  bwd: dx (c8, same shape as x) =
 * R(grad_scale * dy[n, c] / (H W) * act'(b_out)), R = rounding to the context's 16-bit type, act' taken from b_out =
 * the stored output of the block below (its pooled output for a pooled block; NULL: linear) as in tn_c8_fc_dgrad;
 * channels past C are written as 0.  Any N, C, H, W >= 1 (bwd: fewer than 2^32 cells).  Deterministic: no atomics. */
int tn_c8_mean_fwd(tn_ctx* ctx, const void* x, float* y, int N, int C, int H, int W);
int tn_c8_mean_bwd(tn_ctx* ctx, const float* dy, void* dx, int N, int C, int H, int W, const void* b_out, int b_act,
                   float b_prm);
/* DropOutLayer on a c8 tensor (replaces srng.binomial(n=1, p=1-pdrop) * output, dropout.py:10-13 and :21-26, and the test
 * version's (1 - pdrop) * inpt, dropout.py:28-31, for a DropOut layer between the blocks of the 16-bit stack;
 * theanet_amd/csrc/drop_c8.hip).  x, y, gout, gin: c8 tensors of N x C maps of S pixels a side stored at pitch P (P == S,
 * or a power of two > S), either element type; mask8: one byte per 16-byte cell, N * ceil(C/8) * P * P bytes, bit k =
 * channel 8 * octet + k of that pixel kept.
 * fwd: y = x (.) m, a stored value or +0 (exact); pad cells and channels past C are written as 0.  draw != 0: m is drawn
 *   in the same launch and written to mask8 -- element (n, c, h, w) is kept iff tn_dropout_mask(seed, step, d_step, elem0)
 *   keeps element ((n C + c) S + h) S + w of the logical (N, C, S, S) tensor (dropout.py:10-12; no 1/(1-p) rescale, :13),
 *   whatever the element type, the pitch or elem0's alignment.  draw == 0: m is read from mask8 (injected masks).
 * bwd: gin = gout (.) m (the gradient of :13), exact; the activation derivative of the block below is NOT applied here
 *   (the producer of gout has applied it: DropOutLayer.act_info looks through).  y may be x, gin may be gout.
 * scale: y = R(scale * x), the product in fp32, one nearest-even rounding to the context's 16-bit type (dropout.py:28-31
 *   with scale = 1 - pdrop).  Bad geometry, NULL tensors, pdrop outside [0, 1] or 2^32 cells: TN_E_ARG, nothing launched.
 * No atomics: deterministic.                                                                                          */
int tn_c8_dropout_fwd(tn_ctx* ctx, const void* x, void* y, uint8_t* mask8, int N, int C, int S, int P, float pdrop,
                      uint64_t seed, uint32_t step, const uint32_t* d_step, uint64_t elem0, int draw);
int tn_c8_dropout_bwd(tn_ctx* ctx, const void* gout, const uint8_t* mask8, void* gin, int N, int C, int S, int P);
int tn_c8_scale(tn_ctx* ctx, const void* x, void* y, int N, int C, int S, int P, float scale);
/* A stand-alone PoolLayer on a c8 tensor (replaces pool_2d(inpt, (p, p), ignore_border) and its gradient, convpool.py:97-127,
 * for every pool the fused conv + pool block does not take; theanet_amd/csrc/pool_c8.hip).  x, gin: N x C maps of S pixels
 * a side at pitch P; y, gout: maps of So pixels at pitch Po; either element type (the ops compare by value through an
 * ordered integer key that serves halfs and bf16 alike).  Window p x p, stride p, clipped at the map edge; So = S / p
 * (ignore_border) or ceil(S / p).
 * fwd: y = max over the clipped window of the STORED values -- a stored value, never rounded; the window is scanned
 *   row-major and replaced on strict >, so of equal values the first one's pattern is kept.  Pad cells of y and channels
 *   past C are written as 0: every cell of y is written.  Also the test version.  Inputs are NaN-free.
 * bwd: gin[pos] = value(x[pos]) == value(y[window(pos)]) ? gout[window(pos)] : +0: every tied maximum receives the whole
 *   gradient (tn_pool_bwd, Theano's MaxPoolGrad; -0 == +0 ties), copied bit for bit; positions no window covers (the
 *   ignore_border remainder, pad cells, channels past C) get +0; every cell of gin is written.  The activation derivative
 *   of the block below is NOT applied here (the producer of gout has applied act'(y): PoolLayer.act_info looks through).
 * supported: 1 for 2 <= p <= 64, So one of the two sides above and >= 1, Po >= So, P and Po equal to their side or a power
 *   of two above it, every tensor below 2^32 - 256 cells.  Anything else, or a NULL tensor: TN_E_ARG naming the arguments,
 *   nothing launched.  No atomics: deterministic.
 * plan (no device): op 0 (fwd) / 1 (bwd) -> PW (the window instantiation: 2, 3, or 0 = the run-time loop), SH (the pitch
 *   the lanes are laid over -- fwd: Po, bwd: P -- is a power of two), blocks; returns how many values the plan has,
 *   TN_E_ARG for a refused geometry (and always on the CPU backend).                                                  */
int tn_c8_pool_supported(int N, int C, int S, int P, int p, int So, int Po);
int tn_c8_pool_fwd(tn_ctx* ctx, const void* x, void* y, int N, int C, int S, int P, int p, int So, int Po);
int tn_c8_pool_bwd(tn_ctx* ctx, const void* x, const void* y, const void* gout, void* gin, int N, int C, int S, int P,
                   int p, int So, int Po);
int tn_c8_pool_plan(int op, int N, int C, int S, int P, int p, int So, int Po, int* out, int nout);
/* A stand-alone PoolLayer with a stride of its own on a c8 tensor (Theano's pool_2d(inpt, (p, p), ignore_border, st=(st, st))
 * and its gradient MaxPoolGrad: overlapping, st < p, or gapped, st > p, max-pooling; theanet_amd/csrc/pools_c8.hip).
 * Tensors as in tn_c8_pool_*.  Window (i, j) covers rows i * st .. min(S, i * st + p) - 1 and the same columns: clipped at
 * the map edge, never padded.  So = (S - p) / st + 1 (ignore_border; needs S >= p), else (S - 1) / st + 1 for st >= p and
 * max(0, (S - 1 - p + st) / st) + 1 for st < p (Theano's Pool.out_shape); st = p gives tn_c8_pool_*'s sides and bits.
 * fwd: tn_c8_pool_fwd's on those windows -- the maximum of the STORED values through the ordered integer key, row-major
 *   scan, replaced on strict >, a stored pattern, never rounded; pad cells of y and channels past C written as 0, every cell
 *   of y written.  Also the test version.  Inputs are NaN-free.
 * bwd: gin[pos] = the sum of gout[i, j] over the windows that cover pos and whose maximum equals x[pos] by value (-0 == +0
 *   ties; every tied element gets the whole gradient).  The windows covering row h are i = max(0, ceil((h - p + 1) / st)) ..
 *   min(So - 1, h / st), columns likewise; terms are added in fp32 in row-major window order starting from the first term
 *   (a single term is copied bit for bit), and the sum is rounded once, to nearest even, to the context's 16-bit type.  No
 *   term (uncovered or untied positions, pad cells, channels past C): +0; every cell of gin is written.  A gather: a lane
 *   per input cell, no atomics, deterministic.  The activation derivative of the block below is NOT applied (as tn_c8_pool_bwd).
 * supported: 1 for 2 <= p <= 64, 1 <= st <= 64, So one of the two sides above and >= 1, and the pitch and cell-count rules of
 *   tn_c8_pool_supported.  Anything else, or a NULL tensor: TN_E_ARG naming the arguments, nothing launched.
 * plan (no device): op 0 (fwd) / 1 (bwd) -> PW, ST (the compile-time window and stride: (3, 2), (2, 1), or (0, 0) = the
 *   run-time loops), SH (the pitch the lanes are laid over -- fwd: Po, bwd: P -- is a power of two), blocks; returns how
 *   many values the plan has, TN_E_ARG for a refused geometry (and always on the CPU backend).                        */
int tn_c8_pool_st_supported(int N, int C, int S, int P, int p, int st, int So, int Po);
int tn_c8_pool_st_fwd(tn_ctx* ctx, const void* x, void* y, int N, int C, int S, int P, int p, int st, int So, int Po);
int tn_c8_pool_st_bwd(tn_ctx* ctx, const void* x, const void* y, const void* gout, void* gin, int N, int C, int S, int P,
                      int p, int st, int So, int Po);
int tn_c8_pool_st_plan(int op, int N, int C, int S, int P, int p, int st, int So, int Po, int* out, int nout);
/* 1x1 stride-1 ConvLayers on c8 tensors (replace conv2d(inpt, W) + b, the activation and -- fused -- the 2x2 max-pool of
 * convpool.py:54-72, 106-107 with filter_sz 1, and their gradients, for a 1x1 layer on the 16-bit stack;
 * theanet_amd/csrc/conv1_c8.hip).  Tensors: N x C (x, dx) / N x K (y, dz) maps of S pixels a side stored at pitch P (P == S,
 * or a power of two > S) as in tn_c8_dropout_*, either element type; W (K, C, 1, 1) fp32 master weights, b (K) fp32.  C and K
 * need not be multiples of 8: channels past C read as zero (the layout's contract), channels past K are WRITTEN as zero.
 * Arithmetic: tn_c8_conv_fwd's -- operands rounded to the 16-bit type (nearest even), exact products, fp32 accumulation on
 * the matrix core, bias / activation / pooling on the fp32 sums, one rounding on store.  Every op writes the pad cells of
 * its output as zero itself (no tn_c8_pad_zero).
 * fwd: y = act(W . x + b); pool != 0 (S even): followed by the 2x2 max-pool, y (N, K, S/2, S/2) at pitch P / 2, and mask
 *   (NULL: none) gets tn_c8_conv_fwd's bytes (bits 0-3 window elements equal to the maximum, bit 4 / 5 pooled value > 0 /
 *   < 0; pad cells and channels past K: 0) in y's cell order.
 * dgrad: dx = R(W^T . dz * act'(prev_a)), pad cells and channels past C zero; prev_a as in tn_c8_conv_dgrad (the stored
 *   output of the block below, dx's shape; NULL: no derivative).  pooled != 0: `dz` is the pooled gradient (N, K, S/2, S/2)
 *   at pitch P / 2 and dz = (bit of the window element in the block's mask) ? pooled gradient : 0 is formed while loading.
 * wgrad: dW (K, C), db (K) fp32, OVERWRITE, the gradient scale removed in the fp32 epilogue; db is summed from the stored dz.
 *   Slab sums in context scratch finished by the context's reduction: no atomics, one order, the same bits every run.
 * supported: 1 for every N, C, K >= 1 and geometry above whose tensors have fewer than 2^32 cells.  Bad geometry, NULL
 * tensors, pool / pooled with odd S, a pooled gradient without its mask, or 2^32 cells: TN_E_ARG, nothing launched.      */
int tn_c8_conv1_supported(int N, int C, int S, int P, int K);
int tn_c8_conv1_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, uint8_t* mask, int N, int C, int S,
                    int P, int K, int act, float prm, int pool);
int tn_c8_conv1_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K,
                      const void* prev_a, int prev_act, float prev_prm, int pooled, const uint8_t* mask);
int tn_c8_conv1_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int K,
                      int pooled, const uint8_t* mask);
/* ConvLayers of any filter, mode and stride on c8 tensors (replace conv2d(inpt, W, subsample=(stride, stride)) + b on the
 * padded input and the activation of convpool.py:54-72, and their gradients, for every conv shape the two tiled families
 * above refuse; the training param CONV_SHAPES 'any'; theanet_amd/csrc/convg_c8.hip).  Tensors: x / dx N x C maps of S
 * pixels a side stored at pitch P, y / dz N x K maps of So pixels stored at pitch Po (a pitch is the side itself, any size,
 * or a power of two above it: tn_c8_pool_supported's rule), either element type; W (K, C, f, f) fp32 master weights in
 * tn_conv2d_*'s orientation (Theano's conv2d), b (K) fp32.  `pad` is the low padding as in tn_conv2d_*; the high padding
 * follows from So, (So - 1) stride + f - pad - S (negative: the last window ends before the map does), so an even filter
 * in 'same' mode works (f = 4: 2 low, 1 high, as ConvLayer computes it).  C and K need not be multiples of 8.
 * Arithmetic: tn_c8_conv_fwd's -- x and dz as stored, W rounded to the 16-bit type (nearest even), exact products, fp32
 * accumulation on the matrix core, bias / activation on the fp32 sums, one rounding on store.
 * fwd: y = act(conv(x, W) + b).  dgrad: dx = R(conv^T(dz, W) * act'(prev_a)); prev_a: the stored output of the layer below
 *   (dx's shape; NULL: no derivative).  EVERY cell of y / dx is written by the op (no tn_c8_pad_zero): pad cells, channels
 *   past K / C and -- with a stride -- input pixels no window touches as exact +0.
 * wgrad: dW (K, C, f, f), db (K) fp32, OVERWRITE, the gradient scale removed in the fp32 epilogue; db is summed from the
 *   stored dz.  Slab sums in context scratch finished by the context's reduction: no atomics, a slab count that depends on
 *   the geometry alone, one order, the same bits every run and on every device.
 * supported: 1 for every N, C, K, f, stride >= 1 whose geometry is consistent -- pitches as above, pad <= f / 2,
 *   -stride < high padding <= pad (So is the number of windows that fit, no more padding than a 'same' layer's) -- with
 *   fewer than 2^32 cells per tensor, K C f f < 2^28 and f, stride < 2^15.  Anything else, and any NULL tensor:
 *   TN_E_ARG naming the entry point, nothing launched.
 * plan (no device; TN_E_ARG for a refused geometry and on the CPU backend): what call `op` (0 fwd, 1 dgrad, 2 wgrad) takes,
 *   8 values: kernel (0 forward, 1 input gradient stride 1, 2 input gradient strided, 3 weight gradient), leaky-ReLU
 *   epilogue, octets of the reduced maps (fwd: channels, dgrad: filters; wgrad: channels), reduction steps of 2 cells
 *   (wgrad: tiles of 64 output pixels), ragged reduction tail (bit 0: half a step past the last (tap, octet) cell, bit 1: a
 *   ragged octet; wgrad: a partial last pixel tile), 32-row tiles (wgrad: column groups x filter groups), blocks of 256
 *   pixels (wgrad: slabs), ragged output (bit 0: a partial last pixel block -- wgrad: column group --, bit 1: a partial row
 *   tile -- wgrad: filter group).  Returns 8.                                                                             */
int tn_c8_convg_supported(int N, int C, int S, int P, int K, int f, int stride, int pad, int So, int Po);
int tn_c8_convg_fwd(tn_ctx* ctx, const void* x, const float* W, const float* b, void* y, int N, int C, int S, int P, int K,
                    int f, int stride, int pad, int So, int Po, int act, float prm);
int tn_c8_convg_dgrad(tn_ctx* ctx, const void* dz, const float* W, void* dx, int N, int C, int S, int P, int K, int f,
                      int stride, int pad, int So, int Po, const void* prev_a, int prev_act, float prev_prm);
int tn_c8_convg_wgrad(tn_ctx* ctx, const void* x, const void* dz, float* dW, float* db, int N, int C, int S, int P, int K,
                      int f, int stride, int pad, int So, int Po);
int tn_c8_convg_plan(int op, int N, int C, int S, int P, int K, int f, int stride, int pad, int So, int Po, int act,
                     float prm, int* out, int nout);
/* Padded pitch: a c8 tensor of S x S maps may be stored at a power-of-two side P > S (4 <= P <= 64), rows and columns
 * S..P-1 of every octet plane zero.  The conv entry points above then run on the P x P shape (their 'same' products
 * read zeros where the logical ones read padding) and the forward / input gradient are followed by tn_c8_pad_zero on
 * their output; tn_c8_conv_plan_pitch reports that whole sequence (theanet_amd/csrc/conv_c8.hip).
 * pack_pitch: NCHW fp32 (N, C, S, S) rows row0.. -> c8 of pitch P, values times scale, pad and channels past C zero.
 * pad_zero: clears the pad cells of x (S == P: nothing).  crop: padded -> dense (N, ceil(C/8), S, S, 8), the layout
 * tn_c8_fc_* / tn_c8_mean_* read; embed: dense -> padded, pad zero.
 * plan_pitch: S == P: tn_c8_conv_plan's answer; S < P (8 <= P <= 64, pool: S even): tn_c8_conv_plan(op, N, C, P, P, ...)
 * followed by one more value, 1 (the output's pad cleared after op 0 / 1); TN_E_ARG otherwise.                      */
int tn_c8_pack_pitch(tn_ctx* ctx, const float* x, int64_t row0, void* out, int N, int C, int S, int P, float scale);
int tn_c8_pad_zero(tn_ctx* ctx, void* x, int N, int C, int S, int P);
int tn_c8_crop(tn_ctx* ctx, const void* x, void* out, int N, int C, int S, int P);
int tn_c8_embed(tn_ctx* ctx, const void* x, void* out, int N, int C, int S, int P);
int tn_c8_conv_plan_pitch(int op, int N, int C, int S, int P, int K, int pool, int act, float prm, int* out, int nout);

/* 1 if tn_conv2d_* run this shape on the implicit-im2col fp32-MFMA kernels (stride 1, reduction
 * C*f*f >= 32, >= 16 output maps); otherwise the direct VALU kernels are used.              */
int tn_conv_mfma_supported(int C, int K, int f, int stride);
/* Which kernel a tn_conv2d_* call of this shape launches in CONV mode 0 (fp32; CONV 'bfloat16' has kernels of its own) --
 * the launchers' own selection (conv_route and the plan functions of theanet_amd/csrc/conv.hip, conv_mfma.hip and
 * conv_tile.hip, which the entry points run), made without a context or a device.
 *   prod     0 tn_conv2d_fwd, 1 tn_conv2d_wgrad, 2 tn_conv2d_dgrad; the geometry is the LAYER's, as the entry points take it
 *   num_cus  the CU count the selection assumes; 0: the current device's, 256 where no GPU answers
 *   flags    everything else the selection looks at; 0 is the common case
 *            bit 0  the gathered operand(s) are NOT 16-byte aligned (forward x; weight gradient x and dz; input gradient dz)
 *            bit 1  no prev_a (input gradient)
 *            bit 2  out / prev_a NOT 16-byte aligned (forward a; input gradient dx, prev_a)
 *            bit 3  W NOT 16-byte aligned (forward)
 *   The knobs (TN_CONV_TILE*) are read as the library loaded them.
 * One record of 16 ints:
 *    0 route    1 LDS-tile kernels, 2 their few-channel weight gradient, 3 MFMA implicit GEMM, 4 conv_dgrad_lds, 5 direct
 *               kernels, 6 generic weight gradient (ConvRoute; 0, CONV 'bfloat16', is never reported)
 *    1 kernel   0 conv_fwd_direct, 1 conv_wgrad_direct, 2 conv_dgrad_direct, 3 conv_dgrad_lds, 4 conv_wgrad_generic (+
 *               conv_bgrad_generic), 5 conv_mfma_fwd_kernel, 6 conv_mfma_wgrad_kernel, 7 conv_tile_kernel,
 *               8 conv_tile_wgrad_kernel, 9 conv_tile_wgrad_smallc_kernel
 *    2-5        the kernel's template arguments, in order, 0 beyond them: 0 <F, KT>; 1 <F, KT, CT>; 2 <F, CT>; 3 <F>; 4 none;
 *               5 <PADDED, DGRAD>; 6 <PADDED>; 7 <FT, DGRAD, NCP> (POOL = false); 8 <NFT> (POOL = false); 9 none (POOL = false)
 *    6-15       launch geometry, 0 beyond what the kernel has:
 *               0  pixel blocks of 256 (grid x), filter groups of KT (grid y)
 *               1  slabs nblk (grid x; the slab sum follows), filter groups of KT, channel groups of CT
 *               2  pixel blocks of 256, channel groups of CT, prev_a given
 *               3  G images per block, image groups, channel groups of 4, bytes of LDS, prev_a given
 *               4  blocks (K*C*f*f)
 *               5  KT row tiles of 64, MT pixel tiles of 64, Kd reduction depth, M pixels, a_vec (A rows loaded 16 bytes
 *                  at a time), prev_a given
 *               6  KT filter tiles of 64, MT tiles of 64 over Kd, Kd, M pixels, S pixel slabs, mchunk pixels per slab
 *               7  KT filter tiles of 32 FT, MT pixel tiles, RT row tiles per image, NI images per tile, TH rows per tile,
 *                  chunks of 8 gathered channels, vec_out (16-byte epilogue), the kernel's padding (input gradient:
 *                  2 - pad_lo), prev_a given
 *               8  KG filter groups of 32 NFT, CG channel groups of 32, S image slabs, ipb images per slab, NI images per
 *                  tile, RT row tiles per image, NT tiles per slab
 *               9  KG filter groups of 32, S image slabs, ipb, NI, RT, NT as for 8
 * Writes up to nout ints to out and returns the record's length; TN_E_ARG where the call would refuse the shape (and
 * always on the CPU backend).                                                                                       */
int tn_conv_plan(int prod, int N, int C, int H, int W, int K, int f, int stride, int pad_lo, int Ho, int Wo, int num_cus,
                 unsigned flags, int* out, int nout);

/* ---- fused conv + bias + act + max-pool for small feature maps (same reference call sites as
 * tn_conv2d_* followed by tn_pool_*: convpool.py:54-72 then :106-107).  The conv activation
 * never reaches HBM: fwd writes only the pooled map y (N,K,Hp,Wp); bwd takes g = dcost/dy,
 * recomputes the window, routes g to every maximal element (MaxPoolGrad tie rule) times
 * act'(a), and produces dW/db (OVERWRITE) and -- only if dz != NULL -- dz (N,K,Ho,Wo) for a
 * following tn_conv2d_dgrad.  Supported: stride 1, p == 2, f == 3 with C <= 4, f == 5 with
 * C <= 2 (tn_convpool_supported); anything else uses the unfused ops.                      */
int tn_convpool_supported(int C, int f, int stride, int p);
int tn_convpool_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* y,
                    int N, int C, int H, int Wd, int K, int f, int pad_lo, int Ho, int Wo,
                    int p, int Hp, int Wp, int act, float act_param);
int tn_convpool_bwd(tn_ctx* ctx, const float* x, const float* W, const float* b, const float* g,
                    float* dz, float* dW, float* db, int N, int C, int H, int Wd, int K, int f,
                    int pad_lo, int Ho, int Wo, int p, int Hp, int Wp, int act, float act_param);
/* tn_convpool_fwd that also records WHERE each pooled value came from: bit 2*di+dj of
 * mask[n,k,i,j] (uint8, shape of y) is set iff window element (di,dj) exists and attains the
 * maximum -- all of them on a tie, the elements Theano's MaxPoolGrad routes the gradient to
 * (convpool.py:106-107); bits 4 / 5 hold y > 0 / y < 0.  mask == NULL is plain tn_convpool_fwd.
 * tn_convpool_bwd_mask is tn_convpool_bwd driven by that record (f == 3 only): dz = mask bit ?
 * g * act'(y) : 0 with no conv recompute (y is read only when act is not leaky-relu).        */
int tn_convpool_fwd_mask(tn_ctx* ctx, const float* x, const float* W, const float* b, float* y,
                         uint8_t* mask, int N, int C, int H, int Wd, int K, int f, int pad_lo,
                         int Ho, int Wo, int p, int Hp, int Wp, int act, float act_param);
int tn_convpool_bwd_mask(tn_ctx* ctx, const float* x, const float* g, const float* y,
                         const uint8_t* mask, float* dz, float* dW, float* db, int N, int C, int H,
                         int Wd, int K, int f, int pad_lo, int Ho, int Wo, int p, int Hp, int Wp,
                         int act, float act_param);

/* LDS-resident backward of the same fused block for MANY filter elements (K*C*f*f in the
 * hundreds, e.g. mnist.prms conv2): a block keeps G whole images' x and dz in LDS, so dz never
 * reaches HBM and dx (= dcost/dx, may be NULL) comes out of the same kernel as dW/db.
 * tn_convblock_supported returns the group size G (0 = use tn_convpool_bwd + tn_conv2d_dgrad). */
int tn_convblock_supported(int C, int K, int f, int stride, int p, int Ho, int Wo);
int tn_convblock_bwd(tn_ctx* ctx, const float* x, const float* W, const float* b, const float* g,
                     float* dx, float* dW, float* db, int N, int C, int H, int Wd, int K, int f,
                     int pad_lo, int Ho, int Wo, int p, int Hp, int Wp, int act, float act_param);
/* Wide conv + act + 2x2 max-pool blocks (3x3 'same', C*9 >= 32, K >= 16, even maps, rows % 4 == 0)
 * on the LDS-tile matrix-core kernels: tn_convpool_fwd_mask pools in the conv kernel's epilogue (the
 * conv activation never reaches HBM) and tn_convpool_bwd_mask_dx forms dz = mask bit ? g*act'(y) : 0
 * while it stages the operands of the weight- and input-gradient products -- MaxPoolGrad, the
 * activation gradient, CorrMM_gradWeights and CorrMM_gradInputs (convpool.py:54-72,106 under
 * theano.grad, layer.py:83) without dz ever existing.  prev_a / prev_act: output and activation of
 * the layer below, whose gradient is applied to dx in the epilogue (NULL: none); dx NULL: weight
 * gradients only.                                                                               */
int tn_convpool_tile_supported(int N, int C, int H, int Wd, int K, int f, int stride, int pad_lo, int Ho,
                               int Wo, int p, int Hp, int Wp);
int tn_convpool_bwd_mask_dx(tn_ctx* ctx, const float* x, const float* W, const float* g, const float* y,
                            const uint8_t* mask, float* dx, float* dW, float* db, int N, int C, int H,
                            int Wd, int K, int f, int pad_lo, int Ho, int Wo, int p, int Hp, int Wp, int act,
                            float act_param, const float* prev_a, int prev_act, float prev_act_param);

/* The same backward driven by the forward's record instead of a conv recompute: y and mask are
 * tn_convpool_fwd_mask's outputs, so dz = mask bit ? g * act'(y) : 0.  One wave per image on
 * the fp32 matrix cores (wgrad and dgrad products), dz lives in LDS only.  dx may be NULL;
 * dW/db are OVERWRITTEN.  Shapes: f == 3, stride 1, p == 2 keeping the border, C <= 4, K <= 32,
 * Wo <= 14, image and pooled map <= 768 elements (tn_convblock_mask_supported).             */
int tn_convblock_mask_supported(int C, int K, int f, int stride, int p, int H, int Wd, int pad_lo,
                                int Ho, int Wo, int Hp, int Wp);
int tn_convblock_bwd_mask(tn_ctx* ctx, const float* x, const float* W, const float* g,
                          const float* y, const uint8_t* mask, float* dx, float* dW, float* db,
                          int N, int C, int H, int Wd, int K, int f, int pad_lo, int Ho, int Wo,
                          int p, int Hp, int Wp, int act, float act_param);
/* The kernel's lane set-up (tile offsets, window table, the filter operand's sources and validity)
 * depends on the geometry alone and comes from a device table the context owns, one per geometry,
 * freed with the context.  tn_convblock_table builds the table of a supported geometry unless the
 * context has it, and returns when it is complete in device memory (a blocking copy, no stream
 * work).  tn_convblock_bwd_mask entered cold does the same; a caller that captures a graph or runs
 * two steps side by side calls this first (ConvLayer._block_route does, when it picks the route). */
int tn_convblock_table(tn_ctx* ctx, int C, int H, int Wd, int K, int f, int pad_lo, int Ho, int Wo,
                       int p, int Hp, int Wp);

/* ---- pool / mean (replaces pool.pool_2d + MaxPoolGrad, tt.mean; convpool.py:106-107,131) ----
 * max over p x p, stride p, no padding; Ho = ceil(H/p) unless ignore_border (floor).   */
int tn_pool_fwd(tn_ctx* ctx, const float* x, float* y, int NC, int H, int Wd, int p,
                int Ho, int Wo);
/* dx = (x == y[window]) ? dy[window] : 0  (every tie gets the full gradient), then the
 * producing layer's activation gradient is fused exactly as in tn_conv2d_dgrad
 * (x IS that layer's output).  prev_act = TN_ACT_LINEAR disables it.                    */
int tn_pool_bwd(tn_ctx* ctx, const float* x, const float* y, const float* dy, float* dx,
                int NC, int H, int Wd, int p, int Ho, int Wo, int prev_act, float prev_act_param);
/* The same with a stride st of its own (pool_2d's st=): window (i, j) covers rows i*st .. min(H, i*st + p) - 1, columns
 * likewise, clipped and never padded; Ho, Wo by Theano's Pool.out_shape (tn_c8_pool_st_supported), the ops validate
 * (Ho - 1) * st < H and (Wo - 1) * st < Wd.  fwd: fmaxf over the window.  bwd: dx = the sum of dy over the covering
 * windows whose maximum the element equals, in fp32, row-major window order, starting from the first term (+0 where there
 * is none), then the producing layer's activation gradient as in tn_pool_bwd.  A gather, no atomics.  st = p: the bits of
 * tn_pool_fwd / tn_pool_bwd.  Bad geometry or a NULL tensor: TN_E_ARG, nothing launched.                              */
int tn_pool_st_fwd(tn_ctx* ctx, const float* x, float* y, int NC, int H, int Wd, int p, int st,
                   int Ho, int Wo);
int tn_pool_st_bwd(tn_ctx* ctx, const float* x, const float* y, const float* dy, float* dx,
                   int NC, int H, int Wd, int p, int st, int Ho, int Wo, int prev_act, float prev_act_param);
int tn_mean_fwd(tn_ctx* ctx, const float* x, float* y, int NC, int HW);
int tn_mean_bwd(tn_ctx* ctx, const float* dy, float* dx, int NC, int HW,
                const float* prev_a, int prev_act, float prev_act_param);

/* ---- fully connected (replaces tt.dot + bias + act + drop_output; hidden.py:30-32) ----
 * a = act(x(B,n_in) . W(n_in,n_out) + b) ; if mask != NULL: a *= mask (uint8 B x n_out,
 * non-inverted dropout, dropout.py:12-13).  fp32 MFMA (v_mfma_f32_32x32x2_f32).         */
int tn_fc_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a,
              int B, int n_in, int n_out, int act, float act_param, const uint8_t* mask);
/* dW = x^T . dz, db = sum_rows dz (OVERWRITE).  ws: workspace of tn_fc_wgrad_ws_bytes.   */
size_t tn_fc_wgrad_ws_bytes(int B, int n_in, int n_out);
int tn_fc_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db,
                int B, int n_in, int n_out, void* ws);
/* dx = dz . W^T, with the layer-below's activation gradient and dropout mask fused:
 * dx *= act'(prev_a) * prev_mask   (either may be NULL).                                */
int tn_fc_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx,
                int B, int n_in, int n_out,
                const float* prev_a, int prev_act, float prev_act_param, const uint8_t* prev_mask);

/* tn_fc_wgrad + tn_fc_dgrad of one layer as ONE op.  The two products only share dz, so their
 * blocks are interleaved in a single launch (a kernel boundary less, and the prologue / epilogue
 * of one product overlaps the main loop of the other).  Same arguments and results as the two
 * ops; shapes the paired kernel cannot take run them one after the other.                    */
int tn_fc_bwd(tn_ctx* ctx, const float* x, const float* dz, const float* W, float* dW, float* db,
              float* dx, int B, int n_in, int n_out, void* ws, const float* prev_a, int prev_act,
              float prev_act_param, const uint8_t* prev_mask);

/* The whole SoftmaxLayer forward (outlayers.py:87-95 + :50-51) as one op: logits = x W + b
 * followed by tn_softmax_nll on them.  With at most 16 classes it is one launch (the class
 * logits of a row sit in one 16-lane DPP row of the matrix-core epilogue); wider heads run
 * tn_fc_fwd + tn_softmax_nll.  Argument meaning as in those two.                            */
int tn_fc_softmax_nll(tn_ctx* ctx, const float* x, const float* W, const float* b, float* logits, int B,
                      int n_in, int n_out, const int32_t* y, int64_t y_row0, const int64_t* d_row0,
                      float* logprob, float* rowloss, int32_t* pred, float* rowp, float* dz,
                      float inv_batch);
/* ... and the training step of that layer as ONE op: tn_fc_softmax_nll followed by tn_fc_bwd with
 * dz = dlogits (dW, db OVERWRITTEN, dx = d cost / d (input) times act'(prev_a) * prev_mask of the
 * layer below; prev_a, if given, is x itself).  With at most 16 classes the whole thing is one launch
 * per 32 rows: logits, log-softmax / NLL, the input gradient and the rows' weight-gradient slab
 * (ws >= tn_fc_wgrad_ws_bytes).                                                               */
int tn_fc_softmax_train(tn_ctx* ctx, const float* x, const float* W, const float* b, float* logits, int B,
                        int n_in, int n_out, const int32_t* y, int64_t y_row0, const int64_t* d_row0,
                        float* logprob, float* rowloss, int32_t* pred, float* rowp, float* dz,
                        float inv_batch, float* dW, float* db, float* dx, void* ws, const float* prev_a,
                        int prev_act, float prev_act_param, const uint8_t* prev_mask);
/* tn_fc_fwd with the dropout mask DRAWN in the same launch: mask_out[i] is exactly what
 * tn_dropout_mask(seed, step, d_step, elem0) would produce for a (B, n_out) tensor, the output is
 * multiplied by it, and mask_out stays behind for the backward pass (hidden.py:40-43 + dropout.py:
 * 9-13 as one op).  Shapes the fused epilogue cannot take run tn_dropout_mask + tn_fc_fwd.   */
int tn_fc_fwd_dropout(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int B,
                      int n_in, int n_out, int act, float act_param, uint8_t* mask_out, float pdrop,
                      uint64_t seed, uint32_t step, const uint32_t* d_step, uint64_t elem0);
/* Which kernels a tn_fc_* call of this shape launches in MATMUL mode 0 (fp32; the 'bf16x3' and 'bfloat16' modes have
 * kernels of their own) -- the launchers' own selection (the plan functions of theanet_amd/csrc/gemm.hip and
 * fc_skinny.hip, which the entry points run), made without a context or a device.
 *   op       0 tn_fc_fwd, 1 tn_fc_fwd_dropout, 2 tn_fc_wgrad, 3 tn_fc_dgrad, 4 tn_fc_bwd, 5 tn_fc_softmax_nll,
 *            6 tn_fc_softmax_train
 *   num_cus  the CU count the selection assumes; 0: the current device's, 256 where no GPU answers
 *   flags    everything else the selection looks at; 0 is the common case
 *            bit 0  the operand pointers (workspace included) are NOT 16-byte aligned, the byte masks not 4-byte aligned
 *            bit 1  no mask and no prev_a (ops 0, 3, 4, 6; op 6 otherwise passes prev_a = x)
 *            bit 2  a rider is pending in the context (tn_rider_elastic_field; ops 4, 6); it needs 256 * (flags >> 8)
 *                   bytes of LDS
 *            bit 3  elem0 is not a multiple of 4 (op 1)
 *   The knobs (TN_GEMM_*, TN_FC_*, TN_PAIR_DMA, TN_SOFTMAX_TRAIN) are read as the library loaded them.
 * A call launches up to three products (op 6 on a wide head: forward, weight gradient, input gradient; op 4: weight
 * gradient, input gradient; the skinny pair and train kernels count as one).  Per product 17 ints:
 *    0 family   0 skinny matrix-core (fc_skinny.hip), 1 scalar (fc_skinny_*_kernel), 2 tiled, 3 deep, 4 pair,
 *               5 pair-DMA
 *    1 kernel   0 gemm_f32_generic, 1 gemm_f32_fast, 2 gemm_f32_dma, 3 gemm_f32_deep, 4 gemm_f32_pair,
 *               5 gemm_f32_pair_dma, 6 / 7 / 8 fc_skinny_fwd / wgrad / dgrad_kernel, 9 fc_skinny_fwd_mfma,
 *               10 fc_skinny_wgrad_mfma, 11 fc_skinny_dgrad_v4, 12 fc_skinny_bwd_pair, 13 fc_skinny_softmax_train
 *    2-4        AKC, BKC, BSUM (the gemm kernels' operand form: forward 1 0 0, weight gradient 0 0 1, input gradient 1 1 0)
 *    5 tile rows (gemm kernels: 64 or 128; deep: 32; skinny and scalar kernels: rows per block or slab)
 *    6 ring stages (DMA kernels) or waves (deep kernel), else 0
 *    7 c_vec    the 16-byte epilogue
 *    8, 9       K slabs launched, slab depth (gemm kernels)
 *   10, 11      MT, NT: row / column tiles (deep: 32 x 32; else 64 columns; skinny: blocks)
 *   12          a finishing or reduction launch follows
 *   13          the dropout mask is drawn in the epilogue
 *   14, 15      NOUT, RB template arguments of the skinny kernels (0: the kernel has none)
 *   16          the pending rider travels in this (pair) launch
 * Writes up to nout ints to out and returns how many the plan has; TN_E_ARG where the call would refuse the shape (and
 * always on the CPU backend).                                                                                       */
int tn_fc_plan(int op, int B, int n_in, int n_out, int num_cus, unsigned flags, int* out, int nout);

/* ---- dropout (replaces RandomStreams.binomial; dropout.py:9-31) ----
 * mask[i] = uniform(seed, *d_step + step, elem0 + i) >= pdrop  (Philox4x32-10), i < n.
 * elem0 = global index of element 0 so masks do not depend on how a batch is sharded.  */
int tn_dropout_mask(tn_ctx* ctx, uint8_t* mask, size_t n, float pdrop, uint64_t seed,
                    uint32_t step, const uint32_t* d_step, uint64_t elem0);
/* stand-alone DropOutLayer: y = x * mask (fwd);  dx = dy * mask * act'(prev_a) (bwd).   */
int tn_scale_mask(tn_ctx* ctx, const float* x, const uint8_t* mask, float scale, float* y,
                  size_t n, const float* prev_a, int prev_act, float prev_act_param);

/* ---- softmax + NLL (replaces tt.nnet.softmax, log, argmax, -mean; outlayers.py:50-51,69-95) ----
 * logprob = log_softmax(z); rowloss[n] = -logprob[n,y[n]]; pred[n] = argmax (first max);
 * rowp[n] = exp(logprob[n,y[n]]); dz = (softmax - onehot) * inv_batch (NULL to skip).
 * y is read at y[y_row0 + (d_row0 ? *d_row0 : 0) + n].                                  */
int tn_softmax_nll(tn_ctx* ctx, const float* z, const int32_t* y, int64_t y_row0,
                   const int64_t* d_row0, float* logprob, float* rowloss, int32_t* pred,
                   float* rowp, float* dz, int B, int n_out, float inv_batch);
/* Same, plus cost[0] = cost_scale * sum(rowloss) produced by the LAST block to finish (fixed
 * summation order: deterministic), which saves a separate reduction launch.  ws: scratch of
 * tn_softmax_cost_ws_bytes(B) bytes that must be zero before the first call (the kernel leaves
 * it ready for the next one).                                                               */
size_t tn_softmax_cost_ws_bytes(int B);
int tn_softmax_nll_cost(tn_ctx* ctx, const float* z, const int32_t* y, int64_t y_row0,
                        const int64_t* d_row0, float* logprob, float* rowloss, int32_t* pred,
                        float* rowp, float* dz, int B, int n_out, float inv_batch,
                        float cost_scale, float* cost, void* ws);
/* ---- the other output heads and losses (replaces outlayers.py:38-64 losses, :105-126 ExpLossLayer, :129-147
 * HingeLayer, :153-224 CenteredOutLayer) as one row kernel.  head: 0 SOFTMAX (a = logits), 1 EXPLOSS (a = linear
 * output; feat receives a - mean(a)), 2 HINGE (a = linear output), 3 LOGIT / 4 RBF (a = the hidden layer's
 * activated features (B, n), centers (ncls, n); logprob has ncls / ncls+1 columns).  loss (head SOFTMAX only;
 * the other heads have their own): 0 nll, 1 nllsq, 2 nll truncated (loss_param = log threshold), 3 hinge and
 * 4 exp on the softmax output.  rowloss[n]: cost = mean(rowloss); pred = argmax (first maximum); rowstat[n]: the
 * reference's second error statistic per row (P(label); raw output for HINGE; share of wrong bits for LOGIT);
 * da = d cost / d a scaled by inv_batch -- for the centered heads already multiplied by act'(a) (act, act_param =
 * the hidden activation: sigmoid / scaled_tanh), i.e. d cost / d z; dcenters (RBF, may be NULL) accumulates
 * d cost / d centers into a buffer the caller zeroed.  Outputs other than logprob may be NULL.            */
int tn_head_rows(tn_ctx* ctx, int head, int loss, float loss_param, const float* a, const float* centers,
                 int ncls, const int32_t* y, int64_t y_row0, const int64_t* d_row0, float* feat,
                 float* logprob, float* rowloss, int32_t* pred, float* rowstat, float* da, float* dcenters,
                 int B, int n, float inv_batch, float junk_dist, int act, float act_param);
/* out[0] = scale * sum(v[0..n))  (+ out[0] if accumulate) -- cost and error-rate scalars */
int tn_reduce_sum(tn_ctx* ctx, const float* v, size_t n, float scale, float* out, int accumulate);
/* out[0] (+)= L1*sum|p| + L2*sum p^2  (layer.py:109-117)                                 */
int tn_wtcost(tn_ctx* ctx, const float* p, size_t n, float L1, float L2, float* out, int accumulate);
/* The cost of a step of a net with weight costs as ONE launch (layer.py:109-117 summed over the layers,
 * neuralnet.py:208-210, plus the minibatch cost of outlayers.py:50-51):
 *   *d_cost = cost_scale * sum(rowloss[0:nrow]) + sum over rows of (L1 * sum|p| + L2 * sum p^2)
 * h_tab: HOST array of ntab rows, one per parameter tensor of every layer with a non-zero L1 or L2 (frozen layers
 * included); rows with n == 0 or L1 == L2 == 0 add nothing.  Up to 32 rows travel by value with one launch; a longer
 * table takes one launch per 32 rows.  Every (row, TN_WTCOST_CHUNK-element chunk) pair is summed by one block in a
 * fixed order (strided per-thread sums, wave shuffles, the four wave sums), its partial goes to a scratch array of the
 * context's current stream, and the block that finishes last adds the partials in index order, the row losses in the
 * order of tn_sgd_update_net's cost rider, and stores the result: no floating-point atomics, the result depends on
 * the inputs only.  rowloss == NULL: no minibatch cost term.  accumulate != 0: the sum is added to *d_cost (the
 * data-parallel step: the row losses have travelled through the all-reduce).  With ntab == 0 and accumulate == 0 the
 * result has the bits of the rider.                                                                              */
typedef struct tn_wc_seg {
    const float* p;
    uint64_t n;
    float L1, L2;
} tn_wc_seg;
#define TN_WTCOST_CHUNK 16384
int tn_wtcost_net(tn_ctx* ctx, const tn_wc_seg* h_tab, int ntab, const float* rowloss, int nrow, float cost_scale,
                  float* d_cost, int accumulate);
/* out2[0] = mean(pred != y) ; out2[1] = mean(rowp)   (outlayers.py:69-80)
 * out2 is ANY two floats of device memory, written with plain stores by one block: an evaluation of several
 * minibatches (the reference calls its compiled test function once per minibatch, train.py:185-190,238-241, and reads two
 * floats back each time) passes row k of a (len, 2) float array, d_stats + 2*k, for minibatch k and reads the array
 * back once (_TestFn.sweep, theanet_amd/trainfn.py).  Same kernel, same summation order: a row holds the bits a call
 * with its own out2 gets.  There is no separate entry point taking a row number.                                */
int tn_error_stats(tn_ctx* ctx, const int32_t* pred, const int32_t* y, int64_t y_row0,
                   const float* rowp, int B, float* out2);

/* ---- finishing reductions of the weight-gradient ops ----
 * tn_conv2d_wgrad, tn_convpool_bwd*, tn_convblock_bwd* and tn_fc_wgrad end with a fixed-order sum
 * of partial slabs.  Between tn_defer_reductions(ctx, 1) and tn_defer_reductions(ctx, 0) those
 * sums are only recorded; the closing call runs all of them as ONE launch (dW/db are valid after
 * it, in stream order).  Outside such a window every op finishes its own gradient.          */
int tn_defer_reductions(tn_ctx* ctx, int on);
/* tn_defer_reductions(ctx, 0) that also advances a device counter (the RNG step counter) in the same
 * launch, so that everything enqueued afterwards already sees the next step's value.            */
int tn_defer_flush_step(tn_ctx* ctx, uint32_t* d_step);
/* A pipelined step may leave its window open (tn_sgd_update_net in TN_UPD_PIPE mode closes it a step later; the window
 * travels with its stream across tn_stream_select).  tn_defer_discard forgets the recorded sums of both
 * streams without running them -- for windows whose owner (its gradient buffers) is gone.               */
int tn_defer_discard(tn_ctx* ctx);
/* number of finishing sums recorded in the current stream's open tn_defer_reductions window; if rec4 != NULL and
 * 0 <= i < that number, rec4 = {n, S, stride, flip} of record i.  Enqueues nothing. */
int tn_defer_pending(tn_ctx* ctx, int i, uint32_t* rec4);

/* ---- momentum SGD + maxnorm (replaces Layer.get_updates; layer.py:70-107) ----
 * g' = g*gscale + L1*sign(p) + 2*L2*p ; v_new = m*v + (1-m)*g' ; p_new = p - rate*lr*v_OLD
 * (simultaneous Theano update: the OLD velocity moves p).  lr is read from *d_lr.
 * Then maxnorm (0 = off): ndim 1 -> clip ; ndim 2 (rows x cols) -> per-column L2 ;
 * ndim 4 (d0 x rest) -> per-d0 L2, scale (1e-7+clip(n,0,M))/(1e-7+n).                    */
int tn_sgd_update(tn_ctx* ctx, float* p, float* v, const float* g, size_t n,
                  float momentum, float rate, const float* d_lr, float L1, float L2, float gscale);
int tn_maxnorm(tn_ctx* ctx, float* p, int ndim, int d0, int rest, float maxnorm);
/* The same projection for EVERY tensor of the net in one call (layer.py:88-103 runs once per parameter): the 1-D and
 * 4-D tensors -- biases and conv kernels, a few hundred to a few thousand values each -- share ONE launch instead
 * of one launch per tensor (13 launch-bound kernels per step of wide6.prms), 2-D tensors take tn_maxnorm's two-pass
 * path.  h_segs: HOST array of nseg <= 32 descriptors.                                                     */
typedef struct tn_mn_seg {
    float* p;
    int32_t ndim, d0, rest;
    float maxnorm;
} tn_mn_seg;
int tn_maxnorm_multi(tn_ctx* ctx, const tn_mn_seg* h_segs, int nseg);
/* The update of EVERY parameter tensor of the net in one launch, in the form the step's schedule needs -- ONE entry
 * point, `mode` selects the form (all of them: Layer.get_updates, layer.py:70-107, bit-identical weight trajectories):
 *
 *   TN_UPD_PLAIN    d_segs = device array of nseg tn_sgd_seg; max_n = largest n among them (sizes the grid).
 *                   g' = g*gscale + L1*sign(p) + 2*L2*p ; v_new = m*v + (1-m)*g' ; p_new = p - rate*lr*v_OLD.
 *   TN_UPD_LAZY     PLAIN that also ENDS a tn_defer_reductions window: a segment whose gradient is still a stack of
 *                   deferred partial slabs sums them on the fly (same order as the reduction launch), stores the
 *                   gradient and applies the update -- one launch less per step.  h_segs = HOST copy of d_segs (matches
 *                   pending sums to segments; the others are finished by the ordinary reduction launch first).
 *                   nseg <= 32.
 *   TN_UPD_DELAYED  data-parallel "delayed" schedule: layer.py:82-86 applies the OLD velocity, so the weights of step
 *                   t+1 do not depend on the gradient of step t and its all-reduce may overlap the whole next step.
 *                   seg.g = the REDUCED gradient of the PREVIOUS step; flags 1: v = m v + (1-m) g, then p -= rate*lr*v
 *                   (steady state); 2: p only (first delayed step); 3: v only (leaving the schedule).  No L1 / L2
 *                   terms (they need the weights the gradient was taken at) unless flags bit 2 (+4) is set: then
 *                   g' = g*gscale + L1*sign(p) + 2*L2*p with the segment's L1 / L2 at seg.p -- for a caller whose
 *                   seg.p still IS what the gradient was taken at (the pipelined schedule catching its velocity
 *                   up).  No cost rider.
 *   TN_UPD_PIPE     pipelined single-GPU schedule: two steps in flight on the context's two streams, each with its own
 *                   weights / activations / gradients.  d_segs / h_segs = tn_pipe_seg (device array / host copy or
 *                   NULL): p = the stepping stream's own copy, psrc = the other stream's copy (p_{t-1}, read-only
 *                   there), g = the stepping stream's gradient of two steps ago, v shared; flags bit 0 = update v (0
 *                   for the first two steps: no gradient yet).  Also CLOSES the stream's parked tn_defer_reductions
 *                   window like TN_UPD_LAZY (h_segs != NULL, nseg <= 32).  gscale is not used.
 *   TN_UPD_PIPE_REG TN_UPD_PIPE for nets with weight costs: d_segs / h_segs = tn_pipe_reg_seg.  The stepping stream's
 *                   own copy p still holds p_{t-2}, the weights its gradient of two steps ago was taken at, so a
 *                   segment with a non-zero L1 or L2 reads it before it is overwritten and updates v with
 *                   g' = g + L1*sign(p_{t-2}) + 2*L2*p_{t-2} (PLAIN's expression, same bits).
 *
 * d_step != NULL: *d_step += step_inc in the same launch (the RNG step counter; step_inc must be 1 outside
 * TN_UPD_PIPE / TN_UPD_PIPE_REG).  rowloss != NULL: one more block computes *d_cost = cost_scale * sum(rowloss[0:nrow]) in a fixed order
 * -- the minibatch cost tt.mean(nll) of outlayers.py:50-51 (TN_UPD_PIPE: of the stream's PREVIOUS step) -- instead
 * of a reduction kernel of its own; with nseg == 0 the launch is that block alone.                                 */
typedef struct tn_sgd_seg {
    float* p;
    float* v;
    const float* g;
    uint64_t n;
    float momentum, rate, L1, L2;
} tn_sgd_seg;
typedef struct tn_pipe_seg {
    float* p;
    const float* psrc;
    float* v;
    const float* g;
    uint64_t n;
    float momentum, rate;
} tn_pipe_seg;
typedef struct tn_pipe_reg_seg {
    float* p;
    const float* psrc;
    float* v;
    const float* g;
    uint64_t n;
    float momentum, rate, L1, L2;
} tn_pipe_reg_seg;
#define TN_UPD_PLAIN 0
#define TN_UPD_LAZY 1
#define TN_UPD_DELAYED 2
#define TN_UPD_PIPE 3
#define TN_UPD_PIPE_REG 4
int tn_sgd_update_net(tn_ctx* ctx, int mode, const void* d_segs, const void* h_segs, int nseg, size_t max_n,
                      const float* d_lr, float gscale, uint32_t* d_step, uint32_t step_inc, int flags,
                      const float* rowloss, int nrow, float cost_scale, float* d_cost);
/* tn_sgd_update_net followed by tn_maxnorm_multi(h_mn, nmn) -- the whole update expression of layer.py:82-103 -- as one
 * call: in the TN_UPD_LAZY / TN_UPD_PIPE forms the update launch walks a 2-D max-norm tensor in tn_maxnorm's tiles and
 * leaves its column sums of squares (same partial sums, same order: same bits), so the matrix is not read a second
 * time; only the rescaling pass (which touches nothing while every column is within the bound) follows.  Tensors the
 * walk cannot take, and the other modes (TN_UPD_PIPE_REG among them), run the two calls back to back.  nmn <= 32.      */
int tn_sgd_update_net_maxnorm(tn_ctx* ctx, int mode, const void* d_segs, const void* h_segs, int nseg, size_t max_n,
                              const float* d_lr, float gscale, uint32_t* d_step, uint32_t step_inc, int flags,
                              const float* rowloss, int nrow, float cost_scale, float* d_cost, const tn_mn_seg* h_mn,
                              int nmn);

/* ---- averaged weights (training param WT_AVG: d, 0 < d < 1; Polyak averaging) ----
 * Every tensor of a layer with updates has an fp32 average a of its own shape; a_0 = the weights the net starts from.
 * Let p_t (t >= 1) be the weights the forward pass of step t+1 reads, i.e. after the momentum step and after the
 * max-norm projection.  Every p_t enters the average exactly once, in order, wherever the schedule produces it:
 *     c   = fl(1 - d)                            rounded once on the host
 *     a_t = fma(c, fl(p_t - a_{t-1}), a_{t-1})   (__fsub_rn / __fmaf_rn, the way tn_vel is spelled)
 * p is never written.  No atomics: the same bits every run; data-parallel ranks each keep the identical average and
 * exchange nothing.
 * tn_avg_net: d_segs = DEVICE array of nseg tn_avg_seg (built once, like the update's segment table); max_n = the
 * largest n among them (sizes the grid).  mode TN_AVG_UPDATE: the rule above for every segment.  mode TN_AVG_EXCHANGE:
 * p and a change places, a bit copy both ways (c is not used) -- an evaluation at the averaged weights runs between two
 * of them.  One launch for any nseg; a segment may start at any 4-byte boundary.  TN_E_ARG and nothing launched for a
 * NULL table with nseg > 0, max_n == 0 with nseg > 0, c outside [0, 1] or an unknown mode; nseg == 0 does nothing.  */
typedef struct tn_avg_seg {
    float* p;
    float* a;
    uint64_t n;
    uint64_t reserved;      /* pads the row to 32 bytes */
} tn_avg_seg;
#define TN_AVG_UPDATE 0
#define TN_AVG_EXCHANGE 1
int tn_avg_net(tn_ctx* ctx, const tn_avg_seg* d_segs, int nseg, size_t max_n, float c, int mode);

/* ---- elastic input stage (replaces ElasticLayer's graph; inlayers.py:63-144) ----
 * draws layout (float32, device): [0:2] translation u(-1,1) ; [2:4] origin u(.25,.75) ;
 * [4:6] zoom u(-1,1) ; [6] theta u(-1,1) ; [7] pad ; [8 : 8+2hw] N(0,1) noise planes.
 * tn_elastic_draws fills it from Philox (seed, step); parity runs upload it instead.    */
size_t tn_elastic_draws_count(int h, int w);
int tn_elastic_draws(tn_ctx* ctx, float* draws, int h, int w, uint64_t seed,
                     uint32_t step, const uint32_t* d_step);
/* Field -> sample map (one per call, shared by the whole batch; coordinates in float64
 * like the Theano CPU path).  map_idx[h*w] int32 = top*w+left (nearest: the rounded
 * pixel), map_fy/map_fx[h*w] = bilinear fractions (unused for nearest).  target (2hw
 * float64, may be NULL) receives the un-clipped coordinates (debugout, inlayers.py:146). */
int tn_elastic_field(tn_ctx* ctx, const float* draws, int h, int w,
                     double translation, double zoom, double magnitude, int sigma, double angle,
                     int nearest, int32_t* map_idx, float* map_fy, float* map_fx, double* target);
/* out[n,c,:] = resample(invert ? 1-x : x) then flip noise: with flipmask (uint8, N*C*h*w)
 * if given, else Philox(seed, step, global element index) < pflip, else none (pflip=0).
 * x rows are read at x_row0 + (d_row0 ? *d_row0 : 0) + n ; row_global0 is the global
 * index of the first row (for sharding-independent noise).  map_idx == NULL -> identity. */
/* tn_elastic_draws + tn_elastic_field in ONE launch: every block regenerates the (tiny) draws in
 * LDS from Philox (seed, step [+ *d_step]); draws_out (may be NULL for h*w small enough to fit
 * LDS) receives the same values tn_elastic_draws would have written.                         */
int tn_elastic_field_gen(tn_ctx* ctx, float* draws_out, uint64_t seed, uint32_t step,
                         const uint32_t* d_step, int h, int w, double translation, double zoom,
                         double magnitude, int sigma, double angle, int nearest, int32_t* map_idx,
                         float* map_fy, float* map_fx, double* target);
/* tn_elastic_apply fused into the forward of the conv block that consumes it (single-channel
 * images, f == 3, p == 2, at most 16 filters): out (N,1,h,w) is still written (the backward pass
 * reads it), y / mask are tn_convpool_fwd_mask's outputs.  Arguments as in the two ops.        */
int tn_elastic_convpool_supported(int h, int w, int K, int f, int pad_lo, int Ho, int Wo, int p, int Hp,
                                  int Wp);
int tn_elastic_convpool_fwd_mask(tn_ctx* ctx, const float* x, int64_t x_row0, const int64_t* d_row0,
                                 float* out, int N, int h, int w, int invert, int nearest,
                                 const int32_t* map_idx, const float* map_fy, const float* map_fx,
                                 float pflip, const uint8_t* flipmask, uint64_t seed, uint32_t step,
                                 const uint32_t* d_step, int64_t row_global0, const float* W,
                                 const float* b, float* y, uint8_t* mask, int K, int f, int pad_lo, int Ho,
                                 int Wo, int p, int Hp, int Wp, int act, float act_param);

/* Rider: the same field computation, not launched but left with the context; the next paired
 * GEMM launch (tn_fc_bwd) carries it as extra blocks, so it costs no kernel boundary of its own.
 * step is the offset added to *d_step (1 = the minibatch after the one in flight).  tn_rider_pending
 * tells whether it is still waiting, tn_rider_cancel drops it (the caller then runs tn_step_tail or
 * tn_elastic_field_gen itself).                                                              */
int tn_rider_elastic_field(tn_ctx* ctx, float* draws_out, uint64_t seed, uint32_t step,
                           const uint32_t* d_step, int h, int w, double translation, double zoom,
                           double magnitude, int sigma, double angle, int nearest, int32_t* map_idx,
                           float* map_fy, float* map_fx, double* target);
int tn_rider_pending(tn_ctx* ctx);
int tn_rider_cancel(tn_ctx* ctx);
/* The closing launch of a training step: tn_sgd_update_net in TN_UPD_PLAIN mode (without the counter increment)
 * and tn_elastic_field_gen for the NEXT minibatch side by side in one kernel -- the field depends only
 * on *d_step, which the caller has already advanced (tn_defer_flush_step).  Arguments as in the two. */
int tn_step_tail(tn_ctx* ctx, const tn_sgd_seg* d_segs, int nseg, size_t max_n, const float* d_lr,
                 float gscale, const float* rowloss, int nrow, float cost_scale, float* d_cost,
                 float* draws_out, uint64_t seed, const uint32_t* d_step, int h, int w,
                 double translation, double zoom, double magnitude, int sigma, double angle, int nearest,
                 int32_t* map_idx, float* map_fy, float* map_fx, double* target);
int tn_elastic_apply(tn_ctx* ctx, const float* x, int64_t x_row0, const int64_t* d_row0,
                     float* out, int N, int C, int h, int w, int invert, int nearest,
                     const int32_t* map_idx, const float* map_fy, const float* map_fx,
                     float pflip, const uint8_t* flipmask, uint64_t seed, uint32_t step,
                     const uint32_t* d_step, int64_t row_global0);
/* Backward of tn_elastic_apply for an ElasticLayer in the MIDDLE of a net (neuralnet.py:132-142; Theano
 * differentiates through the gather, the inversion and the flip): dx[n,c,src] = sum_p g[n,c,p] * w(p,src)
 * * (invert ? -1 : 1) * (flipped(p) ? -1 : 1), then * act'(prev_a) of the layer below (NULL: none).  The flip
 * noise is regenerated from the same (seed, step, global index) as in the forward.                     */
int tn_elastic_apply_bwd(tn_ctx* ctx, const float* g, float* dx, int N, int C, int h, int w, int invert, int nearest,
                         const int32_t* map_idx, const float* map_fy, const float* map_fx, float pflip,
                         const uint8_t* flipmask, uint64_t seed, uint32_t step, const uint32_t* d_step,
                         int64_t row_global0, const float* prev_a, int prev_act, float prev_act_param);

/* ---- ElasticLayer per_image: a distortion field for EVERY image of the minibatch (theanet_amd/csrc/elastic_img.hip) ----
 * The reference draws one coordinate field per call and shares it among the images of the minibatch
 * (inlayers.py:77-127); with per_image every image n gets its own draws -- translation (2), origin (2), zoom (2),
 * theta (1) and the two N(0,1) noise planes of h*w values: the draws layout above, once per image -- and its field is
 * the reference's chain applied to them: translate, smoothed displacement, un-centre, zoom, rotate, re-centre, clip,
 * nearest / bilinear resample.  All channels of an image share its field; inversion and flip noise are
 * tn_elastic_apply's (same keying of the flip draws).
 *   Draws.  draws_in (N x tn_elastic_draws_count(h, w) floats) injects them; NULL: image n's element i comes from
 * Philox(seed; counter = (i / 4, row_global0 + n, step + *d_step, stream 7)) -- a stream of its own, so a per-image draw
 * never coincides with the batch field's (stream 3) -- through the forms of tn_elastic_draws (header uniforms of one word,
 * both Box-Muller outputs of the word pairs (x, y) and (z, w) for the noise).  They depend on the seed, the step counter,
 * the GLOBAL index of the image in the minibatch and the element only: not on N, the shard or the schedule.
 *   Smoothing.  The separable form of the reference's filter: g[i] = fl32(exp(-i^2 / (2 sigma^2)) / sqrt(2 pi sigma^2)),
 * i = -sigma .. sigma; a row pass then a column pass over el = fl32(magnitude * noise), zero beyond the borders, fp32
 * fused multiply-adds in ascending tap order.  Mathematically elastic_filter's 'full' convolution cropped; not
 * bit-identical to tn_elastic_field's 2-D sum with fp64 accumulation: per pixel the two differ by at most about
 * 2 (2 sigma + 1) 2^-23 (|el| * filter) (tests/test_gpu_elastic_img.py bounds it).
 *   Coordinates.  From the addition of the smoothed displacement on, the float64 chain of tn_elastic_field: origin,
 * zoom as exp(log(zoom) u), rotation as R^T, clip at h - 1 - .001, rint for nearest, truncation + fractions for bilinear.
 *   target (N x 2 x h x w doubles, may be NULL) receives the un-clipped coordinates and draws_out (layout of draws_in,
 * may be NULL) the draws used: both exist for tests and debugging, training passes NULL.  No sample map is written.
 *   tn_elastic_img_supported: C >= 1, h, w >= 2, sigma >= 0 and one block's LDS -- 4 doubles + (4 h (w | 1) +
 * 2 sigma + 2 + 8) floats: two noise planes and two temporaries at an odd pitch, the 1-D filter (padded to even),
 * the header -- within the CU's 160 KiB (64 x 64, sigma 32: 66 888 bytes, above the 64 KiB a launch gets by default: the
 * entry points raise the kernel's limit).  True at least for every h = w <= 64, C <= 4, sigma <= 32.
 *   tn_c8_elastic_apply_img: the same with the c8 tensor of the first conv layer as output ([N][ceil(C/8)][h*w][8], element
 * type of the context, zero beyond C), under tn_c8_elastic_apply's condition ((h*w) % 4 == 0, unpadded maps, 16-byte
 * aligned output); it stores exactly the rounded value of what tn_elastic_apply_img computes.
 *   Unsupported shapes, NULL x / out, N < 1, zoom <= 0 or magnitude != 0 with sigma == 0: TN_E_ARG, nothing launched.  */
int tn_elastic_img_supported(int C, int h, int w, int sigma);
int tn_elastic_apply_img(tn_ctx* ctx, const float* x, int64_t x_row0, const int64_t* d_row0, float* out, int N, int C,
                         int h, int w, int invert, int nearest, double translation, double zoom, double magnitude,
                         int sigma, double angle, float pflip, const uint8_t* flipmask, uint64_t seed, uint32_t step,
                         const uint32_t* d_step, int64_t row_global0, const float* draws_in, float* draws_out,
                         double* target);
int tn_c8_elastic_apply_img(tn_ctx* ctx, const float* x, int64_t x_row0, const int64_t* d_row0, void* out16, int N, int C,
                            int h, int w, int invert, int nearest, double translation, double zoom, double magnitude,
                            int sigma, double angle, float pflip, const uint8_t* flipmask, uint64_t seed, uint32_t step,
                            const uint32_t* d_step, int64_t row_global0, const float* draws_in, float* draws_out,
                            double* target);

/* ---- ColorLayer (replaces color.py:9-52) ----
 * fac[(n*C+c)*3 + k] = exp(ln(balance|gamma|gamma) * u_k), u_k ~ U(-1,1): three random variables of shape
 * (N, C).  draws (float32, [3][N][C]) injects the uniforms (parity runs); NULL -> Philox(seed, step + *d_step,
 * global image index * C + c).  tn_color_apply: out = x/maxval*b -> clip(0,1) -> **g1 -> 1-(1-.)**g2 -> *maxval,
 * rows read from x_row0.  tn_color_apply_bwd: dx = g * d out/d x (Clip's gradient is inclusive) * act'(prev_a). */
int tn_color_factors(tn_ctx* ctx, float* fac, int N, int C, double balance, double gamma, const float* draws,
                     uint64_t seed, uint32_t step, const uint32_t* d_step, int64_t row_global0);
int tn_color_apply(tn_ctx* ctx, const float* x, int64_t x_row0, const float* fac, float* out,
                   int N, int C, int hw, float maxval);
int tn_color_apply_bwd(tn_ctx* ctx, const float* x, int64_t x_row0, const float* fac, const float* g, float* dx, int N,
                       int C, int hw, float maxval, const float* prev_a, int prev_act, float prev_act_param);

/* ---- aux-input layers (replaces auxiliary.py:14-160; their two small dense maps run on tn_fc_*) ----
 * tn_aux_mix: LocationInfo's input (:27-36).  aux (N, 2, d) float32, rows from row0: train: out[n,:] =
 * boost * (aux[n,0,:]*u_n + aux[n,1,:]*(1-u_n)), u_n ~ U(0,1) (u_inj (B) injected, or Philox(seed, step + *d_step,
 * row_global0 + n)); test: boost * mean of the two.  tn_copy_cols: dst[n, col_dst+j] = src[n, col_src+j] for j <
 * ncols (* act'(prev_a[n, col_dst+j])): the concatenation of AuxConcatLayer and the split of its gradient.   */
int tn_aux_mix(tn_ctx* ctx, const float* aux, int64_t row0, float* out, int B, int d, float boost, int train,
               const float* u_inj, uint64_t seed, uint32_t step, const uint32_t* d_step, int64_t row_global0);
int tn_copy_cols(tn_ctx* ctx, const float* src, int ld_src, int col_src, float* dst, int ld_dst, int col_dst, int ncols,
                 int B, const float* prev_a, int prev_act, float prev_act_param);

/* extras/deformer.py:7-18 -- per-IMAGE deformation, in place semantics of Deformer:
 * trans = indices + scale*noise ; each plane gaussian_filter(sigma, truncate 2, nearest) ;
 * bilinear map_coordinates(mode constant, cval).  noise (N,2,h,w) float32 U(-1,1) given,
 * or NULL -> Philox(seed, image index).  imgs float32 (N,h,w) -> out.                    */
int tn_deformer_transform(tn_ctx* ctx, const float* imgs, float* out, int N, int h, int w,
                          double scale, double sigma, double cval, const float* noise,
                          uint64_t seed, int64_t img_global0);

/* ---- minibatch gather (replaces x_data[indx]; neuralnet.py:228-234) ---- */
int tn_gather_rows(tn_ctx* ctx, const void* src, const int32_t* d_index, void* dst,
                   int nrows, size_t row_bytes);
/* The minibatch of a shuffled epoch in ONE launch on the ctx stream (new; the reference's TODO item 18: "a different
 * permutation vector for each epoch"): the epoch's row order stays on the device and for r < nrows, with
 * s = order[row0 + r]: row r of x_out = row s of x (x_row_bytes each), y_out[r] = y[s], row r of aux_out = row s of aux
 * (aux_row_bytes each).  y / y_out and aux / aux_out may be NULL in pairs.  A bit copy (NaN payloads survive): 16 bytes
 * per lane where a row size is a multiple of 16 and both bases are 16-byte aligned, dwords otherwise.  row0 is an
 * int64 like every other row0 of this header, so a recorded step (tn_net_plan_add) advances it with the minibatch
 * index.  Row sizes must be multiples of 4; order entries are NOT range-checked here (the caller checks an order
 * once, when it uploads it).  nrows == 0: no launch.                                                              */
int tn_gather_batch(tn_ctx* ctx, const int32_t* order, int64_t row0, int nrows, const void* x, void* x_out,
                    size_t x_row_bytes, const int32_t* y, int32_t* y_out, const void* aux, void* aux_out,
                    size_t aux_row_bytes);

/* ---- data-parallel gradient exchange over RCCL/xGMI (new) ---- */
#define TN_UNIQUE_ID_BYTES 128
int tn_comm_unique_id(tn_ctx* ctx, void* id128);                 /* rank 0 */
int tn_comm_init(tn_ctx* ctx, const void* id128, int rank, int world);
int tn_comm_destroy(tn_ctx* ctx);
int tn_allreduce_sum(tn_ctx* ctx, float* buf, size_t n);         /* in place, on the ctx stream */
int tn_allreduce_max(tn_ctx* ctx, float* buf, size_t n);
/* The same sum on the context's COMMUNICATION stream (a third stream, so that a bucket of gradients can travel while
 * the compute stream carries on with the backward pass; SURVEY.md 8e "bucket by layer ... to overlap with conv
 * backward"): ordered behind everything enqueued so far on the current compute stream and behind every earlier
 * collective of this entry point (one stream = one order of collectives on the communicator, the same on every rank).
 * done_event (tn_event_create; may be NULL) is recorded on the communication stream behind the collective: the
 * consumer -- the update that opens the stream's next step -- waits for it with tn_event_wait.  tn_sync also waits
 * for the communication stream.                                                                                  */
int tn_allreduce_sum_async(tn_ctx* ctx, float* buf, size_t n, void* done_event);
/* The same in-place sum as a DIRECT reduce-scatter + all-gather (ncclReduceScatter then ncclAllGather, in place: rank r
 * owns elements [r q, (r+1) q), q = n / world; the n % world elements behind them travel in a small all-reduce).
 * MI355X's xGMI is fully connected, so for the large buckets (wide6: 67 MB of dense-layer gradients)
 * the two half-collectives move 2 (S / world) per link pair against a ring's 2 (world - 1) / world * S through every
 * link in turn.  Every element is summed once, at its owner, and broadcast: all ranks hold the same bits.
 * on_comm_stream != 0: ordered and signalled like tn_allreduce_sum_async (done_event may be NULL); 0: on the ctx
 * stream like tn_allreduce_sum (done_event ignored).  theanet_amd/comm.py picks the form per bucket (TN_DP_ALGO,
 * TN_DP_RSAG_MIN_BYTES); the reference has no counterpart (single process; the batch mean of outlayers.py:50-51 is what
 * makes the sum of shard gradients the gradient).                                                                   */
int tn_allreduce_sum_rsag(tn_ctx* ctx, float* buf, size_t n, int on_comm_stream, void* done_event);
int tn_axpby(tn_ctx* ctx, float* y, const float* x, size_t n, float a, float b); /* y = a*x + b*y */

#ifdef __cplusplus
}
#endif
#endif /* THEANET_HIP_H */
