// Shared internals of libtheanet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/theanet_hip.h"
#include "knobs.h"

// arguments of the elastic field computation (elastic_field.h)
struct ElField {       // arguments of the field computation (shared by its two launchers)
    const float* draws_in;
    float* draws_out;
    uint32_t k0, k1, step;
    const uint32_t* d_step;
    int h, w;
    double translation, zoom, magnitude;
    int sigma;
    double angle;
    int nearest;
    int32_t* map_idx;
    float* map_fy;
    float* map_fx;
    double* target;
};

// one finishing reduction out[i] = sum_{s<S} src[s*stride + i] (reduce.hip)
#define TN_RED_MAX 32
struct tn_red_rec {
    const float* src;
    float* out;
    uint32_t n, S, stride, flip;
};

// one geometry's lane table of the matrix-core conv-block backwards (convblock_mfma.hip: cm_table builds, looks up and
// frees them).  The context owns the list; a table lives as long as the context, because a captured graph may hold its
// address.
struct tn_cm_tab {
    int key[9];                            // C, H, Wd, K, pad, Ho, Wo, Hp, Wp
    int* dev;
    tn_cm_tab* next;
};

struct tn_ctx {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream ops are currently issued on
    hipStream_t streams[2] = {nullptr, nullptr};   // [0] main, [1] side (leaf work: weight gradients)
    hipStream_t copy_stream = nullptr;     // device-to-host copies that run under later kernels (tn_d2h_early)
    hipEvent_t copy_ev = nullptr;
    hipEvent_t sync_ev[2] = {nullptr, nullptr};
    hipStream_t comm_stream = nullptr;     // collectives that travel beside the backward pass (tn_allreduce_sum_async)
    hipEvent_t comm_ev = nullptr;
    int num_cus = 256;
    // heavy launches since the second stream was last selected: small = two steps in flight share the GPU
    // (tn_fc_bwd then leaves the other stream's kernels a share of the register file), large = this stream has it alone
    int heavy_since_side = 1 << 20;
    // matmul operand precision of the 3x3 conv products (tn_set_matmul_dtype): 0 fp32, 1 fp16 / 2 bf16 operands and
    // fp32 accumulate (nonzero: the conv stack is 16-bit resident -- several places test it as a boolean); grad_scale:
    // power of two applied to dz before it is rounded to the 16-bit type
    int mm_f16 = 0;
    int fc_b3 = 0;                         // tn_set_fc_matmul: 1 = FC products as bf16 triplets (gemm_b3.hip)
    int fc_bf16 = 0;                       // tn_set_fc_matmul: 2 = FC products on bf16-rounded operands (gemm_bf16.hip)
    int conv_bf16 = 0;                     // tn_set_conv_matmul: 2 = tn_conv2d_* on bf16-rounded operands (conv_bf16.hip)
    float grad_scale = 1.f;
    char err[512] = {0};
    // RCCL (loaded lazily, comm.hip)
    void* rccl_lib = nullptr;
    void* comm = nullptr;
    int rank = 0, world = 1;
    // small persistent scratch (reductions)
    float* scratch = nullptr;              // scratch of the stream ops are currently issued on
    size_t scratch_bytes = 0;
    float* scratch_slot[2] = {nullptr, nullptr};   // parked scratch of the other stream (tn_stream_select):
    size_t scratch_slot_bytes[2] = {0, 0};         // two pipelined steps never share slab memory
    void* tmp[2] = {nullptr, nullptr};             // per stream: a tensor that lives from one launch to the next (tn_tmp_get)
    size_t tmp_bytes[2] = {0, 0};
    // ... and its parked deferral window: a pipelined step leaves its slab sums pending, the update that
    // opens the stream's NEXT step folds them in (tn_sgd_update_net, TN_UPD_PIPE)
    bool defer_slot[2] = {false, false};
    size_t scratch_off_slot[2] = {0, 0};
    int npend_slot[2] = {0, 0};
    tn_red_rec pend_slot[2][TN_RED_MAX];
    // deferred finishing reductions (reduce.hip)
    bool defer = false;
    size_t scratch_off = 0;
    int npend = 0;
    tn_red_rec pend[TN_RED_MAX];
    unsigned long long scratch_gen = 0;    // bumped by every tn_scratch_get: "nobody has asked for scratch since" checks
    // tn_wtcost_net (wtcost.hip), per stream (two pipelined steps sum their costs side by side): the blocks' partial
    // sums and, at wc_part[k][-4 .. -1] (a 16-byte block of its own at the allocation's start), the finishing ticket
    float* wc_part[2] = {nullptr, nullptr};
    size_t wc_cap[2] = {0, 0};             // partials the array holds
    tn_cm_tab* cm_tabs = nullptr;          // lane tables of the conv-block backwards, one per geometry seen (newest first)
    // a light independent job waiting for a heavy launch to ride in (tn_rider_elastic_field)
    bool rider_valid = false;
    ElField rider;
    size_t rider_lds = 0;
};

int tn_scratch_get(tn_ctx* ctx, size_t bytes, float** out);
// a buffer of the current stream that only has to survive until the launches enqueued right after it have run
int tn_tmp_get(tn_ctx* ctx, size_t bytes, float** out);
int tn_tmp_get(tn_ctx* ctx, size_t bytes, float** out);
int tn_red_push(tn_ctx* ctx, const float* src, float* out, uint32_t n, uint32_t S, uint32_t stride,
                uint32_t flip);
int tn_red_commit(tn_ctx* ctx);
// the end of every split weight gradient: record the sums of S_w slabs into dW and of S_b slabs into db (the two
// tn_red_push calls, dW first; flip_w as tn_red_push's flip for dW), then tn_red_commit
int tn_red_wgrad(tn_ctx* ctx, const float* w_slabs, float* dW, uint32_t n_w, uint32_t S_w, uint32_t stride_w,
                 const float* b_slabs, float* db, uint32_t n_b, uint32_t S_b, uint32_t stride_b, uint32_t flip_w = 0);
// Fully-connected layers with n_out <= SK_MAX outputs: the 16-byte-access kernels of fc_skinny.hip where tn_fc_skinny_ok
// holds (TN_FC_SKINNY, n_in % 4 == 0, aligned pointers), else the scalar kernels of gemm.hip; the tn_fc_* entry points
// (gemm.hip) dispatch to both
#define SK_MAX 16
#define SK_WROWS 64      // rows per slab of the scalar weight gradient (fc_skinny_wgrad_kernel)
// rows per block (= per slab) of the one-launch SoftmaxLayer training step (fc_skinny_softmax_train; tn_fc_wgrad_ws_bytes
// sizes the workspace from it)
__host__ __device__ inline int sk_train_rb(int B) { return B < 2048 ? 4 : 16; }
bool tn_fc_skinny_ok(int n_in, int n_out, const void* p0, const void* p1, const void* p2);
// What one product of a dense layer launches.  The plan functions of gemm.hip (fc_*_plan, gemm_plan, deep_plan) and
// tn_fc_skinny_plan (fc_skinny.hip) make the whole choice and fill this; the launchers only map it onto templates, and
// tn_fc_plan (include/theanet_hip.h, which documents the fields) reports it.
enum FcFamily { FCF_SKINNY, FCF_SCALAR, FCF_TILED, FCF_DEEP, FCF_PAIR, FCF_PAIR_DMA };
enum FcKernel {
    FCK_GENERIC, FCK_FAST, FCK_DMA, FCK_DEEP, FCK_PAIR, FCK_PAIR_DMA,      // gemm_f32_*
    FCK_SC_FWD, FCK_SC_WGRAD, FCK_SC_DGRAD,                                // fc_skinny_*_kernel (scalar)
    FCK_SK_FWD, FCK_SK_WGRAD, FCK_SK_DGRAD, FCK_SK_PAIR, FCK_SK_TRAIN      // fc_skinny.hip (matrix core)
};
struct FcProd {
    int family, kernel;
    int akc, bkc, bsum;        // the gemm kernels' operand form
    int tile_m;                // rows of an output tile
    int stages;                // ring stages (DMA kernels) or waves (deep kernel)
    int c_vec;                 // 16-byte epilogue
    int S, kchunk;             // K slabs launched and the slab depth
    int MT, NT;                // output tiles
    int finish;                // a finishing / reduction launch follows
    int drop;                  // dropout drawn in the epilogue
    int nout, rb;              // skinny kernels: the NOUT / RB template arguments (0: none)
    int rider;                 // pair launches: a pending rider travels in this launch
};
#define FC_PROD_INTS 17
// kernel: FCK_SK_FWD / _WGRAD / _DGRAD / _PAIR / _TRAIN (the softmax head's forward is FCK_SK_FWD)
FcProd tn_fc_skinny_plan(int kernel, int B, int n_in, int n_out);
int tn_fc_skinny_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int B,
                     int n_in, int n_out, int act, float prm, const uint8_t* mask);
int tn_fc_skinny_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int B,
                       int n_in, int n_out, float* ws);
int tn_fc_skinny_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int B, int n_in,
                       int n_out, const float* prev_a, int act, float prm, const uint8_t* mask);
int tn_fc_skinny_bwd(tn_ctx* ctx, const float* x, const float* dz, const float* W, float* dW, float* db,
                     float* dx, int B, int n_in, int n_out, float* ws, const float* prev_a, int act,
                     float prm, const uint8_t* mask);
int tn_fc_skinny_softmax_train(tn_ctx* ctx, const float* x, const float* W, const float* b, float* logits,
                               int B, int n_in, int n_out, const int32_t* y, int64_t y_row0,
                               const int64_t* d_row0, float* logprob, float* rowloss, int32_t* pred,
                               float* rowp, float* dz, float inv_batch, float* dW, float* db, float* dx,
                               float* ws, int fuse_act, int act, float prm, const uint8_t* mask);
int tn_fc_skinny_softmax(tn_ctx* ctx, const float* x, const float* W, const float* b, float* logits,
                         int B, int n_in, int n_out, const int32_t* y, int64_t y_row0,
                         const int64_t* d_row0, float* logprob, float* rowloss, int32_t* pred,
                         float* rowp, float* dz, float inv_batch);
// MATMUL 'bf16x3' products of a fully-connected layer (gemm_b3.hip); the tn_fc_* entry points dispatch here when
// tn_set_fc_matmul(ctx, 1) is in force and tn_b3_fc_ok says the shape qualifies
int tn_b3_fc_ok(const float* x, const float* W, int B, int n_in, int n_out);
int tn_b3_fc_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int B, int n_in, int n_out, int act,
                 float prm, const uint8_t* mask);
int tn_b3_fc_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int B, int n_in, int n_out, const float* prev_a,
                   int act, float prm, const uint8_t* mask);
int tn_b3_fc_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int B, int n_in, int n_out, float* ws,
                   int S);
// MATMUL 'bfloat16' products of a fully-connected layer (gemm_bf16.hip): operands rounded to bf16 as they are staged,
// fp32 accumulation; the tn_fc_* entry points dispatch here for EVERY shape while tn_set_fc_matmul(ctx, 2) is in force
int tn_bf_fc_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int B, int n_in, int n_out, int act,
                 float prm, const uint8_t* mask);
int tn_bf_fc_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int B, int n_in, int n_out, const float* prev_a,
                   int act, float prm, const uint8_t* mask);
int tn_bf_fc_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int B, int n_in, int n_out, float* ws,
                   int S);
// CONV 'bfloat16' products of a conv layer (conv_bf16.hip): operands rounded to bf16 as they are staged, fp32
// accumulation; tn_conv2d_fwd / _wgrad / _dgrad dispatch here for EVERY geometry while tn_set_conv_matmul(ctx, 2) is in force
int tn_cb_conv_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int N, int C, int H, int Wd, int K,
                   int f, int stride, int pad, int Ho, int Wo, int act, float prm);
int tn_cb_conv_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int N, int C, int H, int Wd, int K, int f,
                     int stride, int pad, int Ho, int Wo, const float* prev_a, int act, float prm);
int tn_cb_conv_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C, int H, int Wd, int K,
                     int f, int stride, int pad, int Ho, int Wo);
// The fp32 conv family: what one of its files calls in another.  conv_route (conv.hip) decides which of these a tn_conv2d_*
// product runs; the fused blocks' entry points (convpool.hip, convblock*.hip) test their own *_supported functions.
enum ConvProduct { CONV_FWD, CONV_WGRAD, CONV_DGRAD };
enum ConvRoute {
    CONV_BF16,         // CONV 'bfloat16' (conv_bf16.hip): every geometry while the mode is in force
    CONV_TILE,         // LDS-resident-tile matrix-core kernels, 3x3 (conv_tile.hip)
    CONV_TILE_SMALLC,  // ... their weight gradient for few input channels, C*9 <= 32 (first layers)
    CONV_MFMA,         // MFMA implicit GEMM (conv_mfma.hip)
    CONV_LDS_DGRAD,    // conv_dgrad_lds: 3x3 input gradient over an LDS-resident dz
    CONV_DIRECT,       // conv_*_direct
    CONV_GENERIC       // conv_wgrad_generic + conv_bgrad_generic: filter sizes without a direct weight gradient
};
// What one tn_conv2d_* product launches.  Every choice a launcher of the family makes beyond the route -- template arguments,
// grids, slabs, the 16-byte forms -- is made by a plain host function of (shape, alignment bits, CU count) that fills this
// (conv_direct_plan in conv.hip, tn_conv_mfma_plan, tn_conv_tile_*plan); the launchers switch on what those functions
// chose, and tn_conv_plan (include/theanet_hip.h, which documents t[] and v[] per kernel) reports it.
enum ConvKernel {
    CVK_FWD_DIRECT, CVK_WGRAD_DIRECT, CVK_DGRAD_DIRECT, CVK_DGRAD_LDS, CVK_WGRAD_GENERIC,      // conv.hip
    CVK_MFMA, CVK_MFMA_WGRAD,                                                                  // conv_mfma.hip
    CVK_TILE, CVK_TILE_WGRAD, CVK_TILE_SMALLC                                                  // conv_tile.hip
};
// the alignment bits of a product (tn_conv_plan's flags): what the selection reads of the operand pointers
enum {
    CONV_UNAL_GATHER = 1,      // the gathered operand(s) -- forward x, weight gradient x and dz, input gradient dz
    CONV_BARE = 2,             // input gradient without prev_a
    CONV_UNAL_OUT = 4,         // out / prev_a
    CONV_UNAL_W = 8            // W
};
struct ConvPlan {
    int route, kernel;
    int t[4];                  // the kernel's template arguments
    int v[10];                 // launch geometry
};
#define CONV_PLAN_INTS 16
static inline unsigned conv_unal(const void* p, const void* q = nullptr) {
    return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15) != 0;
}
int tn_current_cus();          // gemm.hip: the current device's CU count, 256 where no GPU answers (the plan queries' num_cus 0)
// conv.hip: the end of the family's split weight gradients (slabs in correlation layout: the sum flips every f x f block)
int tn_conv_wgrad_finish(tn_ctx* ctx, const float* partial, const float* dbpartial, float* dW, float* db, int nblk, int K,
                         int C, int f);
// conv_mfma.hip: MFMA implicit GEMM, any f at stride 1 (tn_conv_mfma_supported)
int tn_conv_mfma_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int N, int C, int H, int Wd, int K,
                     int f, int pad, int Ho, int Wo, int act, float prm);
int tn_conv_mfma_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int N, int C, int H, int Wd, int K, int f,
                       int pad, int Ho, int Wo, const float* prev_a, int act, float prm);
int tn_conv_mfma_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C, int H, int Wd, int K,
                       int f, int pad, int Ho, int Wo);
// the *_plan functions take the LAYER's geometry and fill p as the product's launcher would choose; 0: the launcher refuses
int tn_conv_mfma_plan(ConvProduct prod, int num_cus, unsigned al, int N, int C, int H, int Wd, int K, int f, int pad, int Ho,
                      int Wo, ConvPlan* p);
// conv_tile.hip: the LDS-resident-tile kernels for 3x3 windows ...
// (unal: the gathered operand(s) are not 16-byte aligned)
int tn_conv_tile_ok(unsigned unal, int N, int C, int H, int Wd, int K, int f, int pad, int Ho, int Wo);
int tn_conv_tile_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* a, int N, int C, int H, int Wd, int K,
                     int pad, int Ho, int Wo, int act, float prm);
int tn_conv_tile_dgrad(tn_ctx* ctx, const float* dz, const float* W, float* dx, int N, int C, int H, int Wd, int K, int pad,
                       int Ho, int Wo, const float* prev_a, int act, float prm);
int tn_conv_tile_plan(ConvProduct prod, unsigned al, int N, int C, int H, int Wd, int K, int pad, int Ho, int Wo, ConvPlan* p);
int tn_conv_tile_wgrad_ok(int num_cus, unsigned unal, int N, int C, int H, int Wd, int K, int f, int pad,
                          int Ho, int Wo);
int tn_conv_tile_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C, int H, int Wd, int K);
int tn_conv_tile_wgrad_plan(int num_cus, int N, int C, int H, int Wd, int K, ConvPlan* p);
// ... their weight gradient for few input channels (first layers), from a plain dz or from a block's pooling mask ...
int tn_conv_tile_smallc_ok(unsigned unal, int N, int C, int H, int Wd, int K, int f, int pad, int Ho, int Wo);
int tn_conv_tile_smallc_wgrad(tn_ctx* ctx, const float* x, const float* dz, float* dW, float* db, int N, int C, int H, int Wd,
                              int K);
int tn_conv_tile_smallc_plan(int num_cus, int N, int C, int H, int Wd, int K, ConvPlan* p);
extern "C" int tn_convpool_smallc_supported(int N, int C, int H, int Wd, int K, int f, int pad, int Ho, int Wo, int p, int Hp,
                                            int Wp);
int tn_conv_tile_smallc_bwd(tn_ctx* ctx, const float* x, const float* g_, const float* y, const uint8_t* mask, float* dW,
                            float* db, int N, int C, int H, int Wd, int K, int act, float prm);
// ... and wide conv + act + 2x2 max-pool blocks on them (tn_convpool_tile_supported)
int tn_conv_tile_pool_fwd(tn_ctx* ctx, const float* x, const float* W, const float* b, float* y, uint8_t* mask, int N, int C,
                          int H, int Wd, int K, int act, float prm);
int tn_conv_tile_pool_bwd(tn_ctx* ctx, const float* x, const float* W, const float* g_, const float* y, const uint8_t* mask,
                          float* dx, float* dW, float* db, int N, int C, int H, int Wd, int K, int act, float prm,
                          const float* prev_a, int prev_act, float prev_prm);
// convblock_mfma.hip: matrix-core variant of tn_convblock_bwd
int tn_convblock_mfma_supported(int C, int K, int f, int stride, int p, int H, int Wd, int pad_lo, int Ho, int Wo, int Hp,
                                int Wp);
int tn_convblock_mfma_bwd(tn_ctx* ctx, const float* x, const float* W, const float* b, const float* g, float* dx, float* dW,
                          float* db, int N, int C, int H, int Wd, int K, int pad_lo, int Ho, int Wo, int Hp, int Wp, int act,
                          float act_param);
void tn_cm_tables_free(tn_ctx* ctx);       // tn_ctx_destroy: the context's lane tables
int tn_red_flush(tn_ctx* ctx);
int tn_red_flush_inc(tn_ctx* ctx, uint32_t* inc);

extern char g_tn_err[512];

inline int tn_fail(tn_ctx* ctx, int code, const char* fmt, ...) {
    char* dst = ctx ? ctx->err : g_tn_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}

#define TN_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return tn_fail(ctx, TN_E_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call,    \
                           hipGetErrorString(e_));                                        \
    } while (0)

#define TN_LAUNCH_CHECK()                                                                 \
    do {                                                                                  \
        hipError_t e_ = hipGetLastError();                                                \
        if (e_ != hipSuccess)                                                             \
            return tn_fail(ctx, TN_E_HIP, "%s:%d launch -> %s", __FILE__, __LINE__,       \
                           hipGetErrorString(e_));                                        \
    } while (0)

#define TN_REQUIRE(cond, ...)                                                             \
    do {                                                                                  \
        if (!(cond)) return tn_fail(ctx, TN_E_ARG, __VA_ARGS__);                          \
    } while (0)

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// the entry points that take fp32 activations refuse to run while a 16-bit DTYPE mode is in force
#define TN_FP32_ONLY(ctx, name) \
    TN_REQUIRE(!(ctx)->mm_f16, name ": fp32 tensors in a 16-bit DTYPE mode (the mode's entry points are tn_c8_*)")

// The slab prologue of the fp32 conv family's split weight gradients: scratch for nslab (the caller's rule) slabs of
// KCFF = K*C*f*f weight sums, then nslab slabs of K bias sums (tn_conv_wgrad_finish adds them up)
inline int conv_slabs(tn_ctx* ctx, int nslab, size_t KCFF, int K, float** partial, float** dbpartial) {
    int rc = tn_scratch_get(ctx, (size_t)nslab * (KCFF + K) * sizeof(float), partial);
    if (rc) return rc;
    *dbpartial = *partial + (size_t)nslab * KCFF;
    return TN_OK;
}

// Launch Kern with `lds` bytes of dynamic LDS: the grow-only opt-in (not a stream op: once per size), then the launch, which
// the caller checks.  The high-water mark is per KERNEL: Kern is a template argument because all ACT instantiations of a
// kernel share one function type, and a static keyed on that type would skip the second one's opt-in.
template <auto Kern, class... Args>
static int tn_launch_lds(tn_ctx* ctx, dim3 grid, dim3 block, size_t lds, Args... args) {
    static size_t set_for = 0;
    if (set_for < lds) {
        TN_HIP(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        set_for = lds;
    }
    Kern<<<grid, block, lds, ctx->stream>>>(args...);
    return TN_OK;
}

// ---------------------------------------------------------------------------
// activations (theanet/layer/layer.py:27-39).  The backward pass only keeps the
// layer OUTPUT a, so act'(z) is expressed through a:
//   leaky(s): a>0 -> 1 ; a<0 -> s ; a==0 -> 1+s  (Theano's Maximum/Minimum tie rule;
//             for s==0 an exact a==0 is read as z<0 -> 0: documented in DESIGN.md)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float tn_act_fwd(float z, int act, float prm) {
    switch (act) {
        case TN_ACT_LEAKY: return fmaxf(0.f, z) + fminf(0.f, z) * prm;
        case TN_ACT_TANH: return tanhf(z);
        case TN_ACT_SIGMOID: return 1.f / (1.f + expf(-z));
        case TN_ACT_SOFTPLUS: return z > 20.f ? z : log1pf(expf(z));
        case TN_ACT_SCALED_TANH: return 1.7f * tanhf(2.f * z / 3.f);
        default: return z;
    }
}

__device__ __forceinline__ float tn_act_grad_from_out(float a, int act, float prm) {
    switch (act) {
        case TN_ACT_LEAKY:
            if (a > 0.f) return 1.f;
            if (a < 0.f) return prm;
            return prm > 0.f ? 1.f + prm : 0.f;
        case TN_ACT_TANH: return 1.f - a * a;
        case TN_ACT_SIGMOID: return a * (1.f - a);
        case TN_ACT_SOFTPLUS: return 1.f - expf(-a);
        case TN_ACT_SCALED_TANH: {
            float t = a * (1.f / 1.7f);
            return (1.7f * 2.f / 3.f) * (1.f - t * t);
        }
        default: return 1.f;
    }
}

// The fused conv blocks' form (convpool.hip, convblock.hip, convblock_mfma.hip): ACT == TN_ACT_LEAKY compiles the
// leaky-ReLU expressions in line, any other ACT (-1) takes the run-time switch above.
template <int ACT>
__device__ __forceinline__ float cb_act(float z, int act, float prm) {
    if (ACT == TN_ACT_LEAKY) return fmaxf(0.f, z) + fminf(0.f, z) * prm;
    return tn_act_fwd(z, act, prm);
}
template <int ACT>
__device__ __forceinline__ float cb_actg(float a, int act, float prm) {
    if (ACT == TN_ACT_LEAKY) return a > 0.f ? 1.f : (a < 0.f ? prm : (prm > 0.f ? 1.f + prm : 0.f));
    return tn_act_grad_from_out(a, act, prm);
}

// Four values behind ONE wave-uniform test of the activation kind.  Epilogues that called the two functions above
// per element paid the whole switch every time (fc_skinny_softmax_train's input-gradient phase: 401 scalar branches
// for 32 elements, 5.5 of the block's 12.6 us); the leaky-ReLU family -- every default of the reference
// (convpool.py:19, hidden.py:16) -- is straight-line code here, same expressions, same bits.
// LK (the caller has established act is TN_ACT_LEAKY or TN_ACT_LINEAR): the transcendental kinds are not even compiled in.
// The GEMM epilogues call these once per unrolled pass; with every kind inlined each time a GEMM kernel was 150-300 KB
// of code, its leaky-ReLU path a chain of jumps over tanhf / expf bodies -- an epilogue of ~10 k cycles, most of them
// instruction-cache misses (round 5, tools/dbg_gemm.py).
template <bool LK = false>
__device__ __forceinline__ void tn_act_fwd4(float4& v, int act, float prm) {
    if (act == TN_ACT_LEAKY) {
        v.x = fmaxf(0.f, v.x) + fminf(0.f, v.x) * prm;
        v.y = fmaxf(0.f, v.y) + fminf(0.f, v.y) * prm;
        v.z = fmaxf(0.f, v.z) + fminf(0.f, v.z) * prm;
        v.w = fmaxf(0.f, v.w) + fminf(0.f, v.w) * prm;
    } else if (!LK && act != TN_ACT_LINEAR) {
        v.x = tn_act_fwd(v.x, act, prm);
        v.y = tn_act_fwd(v.y, act, prm);
        v.z = tn_act_fwd(v.z, act, prm);
        v.w = tn_act_fwd(v.w, act, prm);
    }
}
// s *= act'(a), a = the layer's OUTPUT
template <bool LK = false>
__device__ __forceinline__ void tn_act_grad4(float4& s, const float4& a, int act, float prm) {
    if (act == TN_ACT_LEAKY) {
        const float tie = prm > 0.f ? 1.f + prm : 0.f;
        s.x *= a.x > 0.f ? 1.f : (a.x < 0.f ? prm : tie);
        s.y *= a.y > 0.f ? 1.f : (a.y < 0.f ? prm : tie);
        s.z *= a.z > 0.f ? 1.f : (a.z < 0.f ? prm : tie);
        s.w *= a.w > 0.f ? 1.f : (a.w < 0.f ? prm : tie);
    } else if (!LK && act != TN_ACT_LINEAR) {
        s.x *= tn_act_grad_from_out(a.x, act, prm);
        s.y *= tn_act_grad_from_out(a.y, act, prm);
        s.z *= tn_act_grad_from_out(a.z, act, prm);
        s.w *= tn_act_grad_from_out(a.w, act, prm);
    }
}

// ---------------------------------------------------------------------------
// The two expressions of the momentum-SGD update (layer.py:82-86), with their roundings spelled out:
// several kernels apply them (one step at a time / lazy slabs / delayed / two steps in flight) and the
// weight trajectories of all schedules must agree bit for bit, so the compiler must not be free to
// contract them differently from kernel to kernel.
//   v' = m*v + (1-m)*g  := fma(m, v, rn((1-m)*g))          p' = p - step*v  := fma(-step, v, p)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float tn_vel(float m, float v, float g) { return __fmaf_rn(m, v, __fmul_rn(1.f - m, g)); }
__device__ __forceinline__ float tn_stepped(float p, float step, float v) { return __fmaf_rn(-step, v, p); }

// ---------------------------------------------------------------------------
// Philox4x32-10 counter RNG: key = seed, counter = (lo(idx), hi(idx), step, stream)
// ---------------------------------------------------------------------------
struct u32x4 {
    uint32_t x, y, z, w;
};

__host__ __device__ __forceinline__ u32x4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2,
                                                     uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return {c0, c1, c2, c3};
}

// uniform in [0,1) with 24 bits
__host__ __device__ __forceinline__ float tn_u01(uint32_t r) { return (r >> 8) * (1.0f / 16777216.0f); }

enum { TN_STREAM_DROPOUT = 1, TN_STREAM_FLIP = 2, TN_STREAM_ELASTIC = 3, TN_STREAM_DEFORMER = 4 };
