// ElasticLayer per_image: a distortion field for every image of the minibatch, built and consumed in ONE launch.
//   tn_elastic_apply_img / tn_c8_elastic_apply_img   (include/theanet_hip.h)
// One 256-thread block per image:
//   A  the image's draws (header + two N(0,1) planes; Philox keyed by the image's GLOBAL index, or injected) -> LDS
//   B  row pass    of the separable gaussian: noise planes -> temporaries   (fp32, zero padded)
//   C  column pass                          : temporaries  -> noise planes
//   D  per pixel: the float64 coordinate chain of elastic_field_block from `ty += (double)(float)s0` on, then the gather
//      of all C channels (1 or 4 taps), inversion, flip noise, store -- fp32 NCHW or the first conv layer's c8 cells.
// No sample map goes to memory, and the smoothing has no fp64: the batch kernel (elastic_field.h) spends a wave per
// pixel on the (2s+1)^2 correlation with fp64 accumulation, which repeated per image would cost more than the step.
// Both 1-D passes are register-blocked along the pass direction: a thread owns EI_R consecutive outputs and slides a
// window of EI_R inputs along the taps, so a tap is read from LDS once (plus one broadcast read of the filter value)
// for EI_R fused multiply-adds.  The planes are stored at an odd pitch: neighbouring threads walk neighbouring rows in
// the row pass (stride = pitch) and neighbouring columns in the column pass (stride 1), both free of bank conflicts.
#include <type_traits>

#include "c8_elem.h"
#include "common.h"

#define EI_HDR 8          // draws of one image: the layout of tn_elastic_draws (header of 8, then the two noise planes)
#define EI_R 8            // outputs per thread along the pass direction
enum { TN_STREAM_ELASTIC_IMG = 7 };      // a Philox stream of its own: never the batch field's draws

struct EiArgs {
    const float* x;
    int64_t x_row0;
    const int64_t* d_row0;
    void* out;
    int N, C, h, w, invert, nearest;
    double translation, zoom, magnitude;
    int sigma;
    double angle;
    float pflip;
    const uint8_t* flipmask;
    uint32_t k0, k1, step;
    const uint32_t* d_step;
    int64_t row_global0;
    const float* draws_in;
    float* draws_out;
    double* target;
};

// LDS of one block: 4 doubles (zoom factors, cos, sin), then floats: 2 noise planes + 2 temporaries at pitch (w | 1),
// the 1-D filter (2 sigma + 1, padded to even) and the 8 header draws.
__host__ __device__ static inline int ei_pitch(int w) { return w | 1; }
static inline size_t ei_lds_bytes(int h, int w, int sigma) {
    return 4 * sizeof(double) + ((size_t)4 * h * ei_pitch(w) + (size_t)(2 * sigma + 2) + EI_HDR) * sizeof(float);
}

// draws quad q = elements 4q .. 4q+3 of image `img` (global index): elastic_draw4's forms, keyed per image
__device__ __forceinline__ void ei_draw4(int q, uint32_t img, uint32_t st, uint32_t k0, uint32_t k1, float (&v)[4]) {
    const u32x4 r = philox4x32((uint32_t)q, img, st, TN_STREAM_ELASTIC_IMG, k0, k1);
    const uint32_t wd[4] = {r.x, r.y, r.z, r.w};
    if (4 * q < EI_HDR) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * q + e;
            const float u = tn_u01(wd[e]);
            v[e] = (i == 2 || i == 3) ? .25f + .5f * u : -1.f + 2.f * u;     // origin U(.25,.75), else U(-1,1)
        }
        return;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((wd[2 * h] >> 8) + 1) * (1.0f / 16777216.0f);
        const float a = 6.28318530717958647692f * tn_u01(wd[2 * h + 1]);
        const float rad = sqrtf(-2.f * logf(u1));
        v[2 * h] = rad * cosf(a);
        v[2 * h + 1] = rad * sinf(a);
    }
}

// acc[r] = sum_{t = 0 .. 2 sigma} g[t] * (scale * line[pos0 + r + t - sigma]), r = 0 .. EI_R-1, taps in ascending order,
// fused multiply-adds; line = n elements `stride` floats apart, zero outside.  win[] holds the EI_R inputs under the
// current tap; moving to the next tap drops one and reads one (the rotation is resolved at compile time).
__device__ __forceinline__ void ei_pass(const float* __restrict__ line, int stride, int n, int pos0,
                                        const float* __restrict__ g, int sigma, float scale, float (&acc)[EI_R]) {
    const int ks = 2 * sigma + 1;
    float win[EI_R];
#pragma unroll
    for (int r = 0; r < EI_R; ++r) {
        const int i = pos0 + r - sigma;
        win[r] = (unsigned)i < (unsigned)n ? scale * line[i * stride] : 0.f;
        acc[r] = 0.f;
    }
    int nxt = pos0 + EI_R - sigma;
    for (int tb = 0; tb < ks; tb += EI_R) {
#pragma unroll
        for (int u = 0; u < EI_R; ++u) {
            if (tb + u < ks) {
                const float gt = g[tb + u];
#pragma unroll
                for (int r = 0; r < EI_R; ++r) acc[r] = fmaf(gt, win[(r + u) % EI_R], acc[r]);
                win[u] = (unsigned)nxt < (unsigned)n ? scale * line[nxt * stride] : 0.f;
                ++nxt;
            }
        }
    }
}

// E = void: out is fp32 (N, C, h, w); E = C8H / C8B: out is the c8 tensor [N][C8][pixel][8 channels], zero beyond C
template <typename E>
__global__ __launch_bounds__(256) void elastic_img_kernel(EiArgs a) {
    extern __shared__ double ei_smem[];
    const int h = a.h, w = a.w, hw = h * w, C = a.C, sigma = a.sigma;
    const int P = ei_pitch(w), PS = h * P, ks = 2 * sigma + 1;
    double* aux = ei_smem;
    float* nz = reinterpret_cast<float*>(ei_smem + 4);       // [2][PS] noise, then the smoothed displacement
    float* tp = nz + 2 * PS;                                  // [2][PS] after the row pass
    float* g = tp + 2 * PS;                                   // [ks]
    float* hdr = g + ks + 1;                                  // [EI_HDR]
    const int n = blockIdx.x;
    const int total = EI_HDR + 2 * hw;
    const uint32_t st = a.step + (a.d_step ? *a.d_step : 0u);
    const bool smooth = a.magnitude != 0.0;

    // ---- A: draws -> LDS (and draws_out), the 1-D filter
    if (a.draws_in) {
        const float* din = a.draws_in + (size_t)n * total;
        for (int i = threadIdx.x; i < total; i += 256) {
            const float v = din[i];
            if (i < EI_HDR) {
                hdr[i] = v;
            } else {
                const int k = i - EI_HDR, pl = k >= hw, p = k - pl * hw, y = p / w;
                nz[pl * PS + y * P + (p - y * w)] = v;
            }
            if (a.draws_out) a.draws_out[(size_t)n * total + i] = v;
        }
    } else {
        const uint32_t img = (uint32_t)(a.row_global0 + n);
        for (int q = threadIdx.x; 4 * q < total; q += 256) {
            float v[4];
            ei_draw4(q, img, st, a.k0, a.k1, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 4 * q + e;
                if (i >= total) break;
                if (i < EI_HDR) {
                    hdr[i] = v[e];
                } else {
                    const int k = i - EI_HDR, pl = k >= hw, p = k - pl * hw, y = p / w;
                    nz[pl * PS + y * P + (p - y * w)] = v[e];
                }
                if (a.draws_out) a.draws_out[(size_t)n * total + i] = v[e];
            }
        }
    }
    if (smooth) {
        // g[i] = fl32(exp(-i^2 / (2 sigma^2)) / sqrt(2 pi sigma^2)): g (x) g is the reference's filter (elastic_filter)
        const double var = (double)sigma * sigma;
        for (int t = threadIdx.x; t < ks; t += 256) {
            const double i = t - sigma;
            g[t] = (float)(exp(-.5 * i * i / var) / sqrt(2.0 * 3.14159265358979323846 * var));
        }
    }
    __syncthreads();

    // ---- B: zoom factors and rotation (four threads), row pass (everybody)
    if (threadIdx.x >= 252 && (a.zoom != 1.0 || a.angle != 0.0)) {
        const int j = threadIdx.x - 252;
        double r;
        if (j < 2) {
            r = a.zoom != 1.0 ? exp(log(a.zoom) * (double)hdr[4 + j]) : 1.0;
        } else {
            const double theta = (a.angle * 3.14159265358979323846 / 180.0) * (double)hdr[6];
            r = j == 2 ? cos(theta) : sin(theta);
        }
        aux[j] = r;
    }
    if (smooth) {
        const float mag = (float)a.magnitude;
        const int nrun = (w + EI_R - 1) / EI_R;
        for (int it = threadIdx.x; it < 2 * nrun * h; it += 256) {
            const int row = it % h, rest = it / h, run = rest % nrun, pl = rest / nrun;
            float acc[EI_R];
            ei_pass(nz + pl * PS + row * P, 1, w, run * EI_R, g, sigma, mag, acc);      // el = fl32(mag * noise)
            float* dst = tp + pl * PS + row * P + run * EI_R;
#pragma unroll
            for (int r = 0; r < EI_R; ++r)
                if (run * EI_R + r < w) dst[r] = acc[r];
        }
        __syncthreads();
        // ---- C: column pass
        const int ncr = (h + EI_R - 1) / EI_R;
        for (int it = threadIdx.x; it < 2 * ncr * w; it += 256) {
            const int col = it % w, rest = it / w, run = rest % ncr, pl = rest / ncr;
            float acc[EI_R];
            ei_pass(tp + pl * PS + col, P, h, run * EI_R, g, sigma, 1.f, acc);
            float* dst = nz + pl * PS + run * EI_R * P + col;
#pragma unroll
            for (int r = 0; r < EI_R; ++r)
                if (run * EI_R + r < h) dst[r * P] = acc[r];
        }
    }
    __syncthreads();

    // ---- D: coordinates (float64, as elastic_field_block), gather, store
    const int64_t row_off = a.x_row0 + (a.d_row0 ? *a.d_row0 : 0);
    const float* xn = a.x + (size_t)(row_off + n) * C * hw;
    const bool affine = a.zoom != 1.0 || a.angle != 0.0;
    for (int p = threadIdx.x; p < hw; p += 256) {
        const int y = p / w, xx = p - y * w;
        double ty = y, tx = xx;
        if (a.translation != 0.0) {
            ty += (double)((float)a.translation * hdr[0]);
            tx += (double)((float)a.translation * hdr[1]);
        }
        if (smooth) {
            ty += (double)nz[y * P + xx];
            tx += (double)nz[PS + y * P + xx];
        }
        if (affine) {
            const double oy = (double)hdr[2] * h, ox = (double)hdr[3] * w;
            ty -= oy;
            tx -= ox;
            if (a.zoom != 1.0) {
                ty *= aux[0];          // exp(log(zoom) * draws[4])
                tx *= aux[1];          // exp(log(zoom) * draws[5])
            }
            if (a.angle != 0.0) {
                const double c = aux[2], s = aux[3];      // cos / sin(angle * pi/180 * draws[6])
                // tensordot(R, target, axes=(0,0)) with R=[[c,-s],[s,c]] -> R^T applied
                const double ry = c * ty + s * tx;
                const double rx = -s * ty + c * tx;
                ty = ry;
                tx = rx;
            }
            ty += oy;
            tx += ox;
        }
        if (a.target) {
            a.target[((size_t)n * 2) * hw + p] = ty;
            a.target[((size_t)n * 2 + 1) * hw + p] = tx;
        }
        const double cy = fmin(fmax(ty, 0.0), (double)h - 1 - .001);
        const double cx = fmin(fmax(tx, 0.0), (double)w - 1 - .001);
        int m;
        float fy = 0.f, fx = 0.f;
        if (a.nearest) {
            m = (int)rint(cy) * w + (int)rint(cx);
        } else {
            const int top = (int)cy, left = (int)cx;
            m = top * w + left;
            fy = (float)(cy - top);
            fx = (float)(cx - left);
        }
        // one channel of this pixel: the expressions of elastic_apply_kernel
        auto sample = [&](int c) -> float {
            const float* xi = xn + (size_t)c * hw;
            float v;
            if (a.nearest) {
                v = xi[m];
                if (a.invert) v = 1.f - v;
            } else {
                float q0 = xi[m], q1 = xi[m + 1], q2 = xi[m + w], q3 = xi[m + w + 1];
                if (a.invert) {
                    q0 = 1.f - q0;
                    q1 = 1.f - q1;
                    q2 = 1.f - q2;
                    q3 = 1.f - q3;
                }
                // same association as inlayers.py:134-137
                v = q0 * (1.f - fy) * (1.f - fx) + q1 * (1.f - fy) * fx + q2 * fy * (1.f - fx) + q3 * fy * fx;
            }
            const uint64_t t = ((uint64_t)n * C + c) * hw + p;           // element of the local (N, C, h, w) batch
            if (a.flipmask) {
                if (a.flipmask[t]) v = 1.f - v;
            } else if (a.pflip > 0.f) {
                const uint64_t e = (uint64_t)a.row_global0 * C * hw + t;
                const uint64_t cq = e >> 2;
                const u32x4 r = philox4x32((uint32_t)cq, (uint32_t)(cq >> 32), st, TN_STREAM_FLIP, a.k0, a.k1);
                const uint32_t wd = ((e & 3) == 0) ? r.x : ((e & 3) == 1) ? r.y : ((e & 3) == 2) ? r.z : r.w;
                if (tn_u01(wd) < a.pflip) v = 1.f - v;
            }
            return v;
        };
        if constexpr (std::is_void<E>::value) {
            float* out = static_cast<float*>(a.out) + (size_t)n * C * hw + p;
            for (int c = 0; c < C; ++c) out[(size_t)c * hw] = sample(c);
        } else {
            const int C8 = (C + 7) / 8;
            typename E::v8* out = static_cast<typename E::v8*>(a.out) + (size_t)n * C8 * hw + p;
            for (int o = 0; o < C8; ++o) {
                typename E::v8 cell;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = 8 * o + e;
                    cell[e] = (typename E::T)(c < C ? sample(c) : 0.f);
                }
                out[(size_t)o * hw] = cell;
            }
        }
    }
}

template <typename E>
static int ei_launch(tn_ctx* ctx, const EiArgs& a) {
    const size_t lds = ei_lds_bytes(a.h, a.w, a.sigma);
    if (lds > 64 * 1024) {
        TN_HIP(hipFuncSetAttribute((const void*)elastic_img_kernel<E>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    }
    elastic_img_kernel<E><<<a.N, 256, lds, ctx->stream>>>(a);
    TN_LAUNCH_CHECK();
    return TN_OK;
}

extern "C" {

int tn_elastic_img_supported(int C, int h, int w, int sigma) {
    if (C < 1 || h < 2 || w < 2 || sigma < 0 || h > 4096 || w > 4096 || sigma > 4096) return 0;
    return ei_lds_bytes(h, w, sigma) <= 160 * 1024;
}

#define EI_CHECK(name)                                                                                              \
    TN_REQUIRE(N > 0 && x && out, name ": bad arguments");                                                          \
    TN_REQUIRE(tn_elastic_img_supported(C, h, w, sigma), name ": %d maps of %d x %d, sigma %d: not supported "      \
               "(tn_elastic_img_supported)", C, h, w, sigma);                                                       \
    TN_REQUIRE(zoom > 0 && (magnitude == 0.0 || sigma >= 1), name ": zoom %g / sigma %d with magnitude %g", zoom,   \
               sigma, magnitude)
#define EI_ARGS(outp)                                                                                               \
    EiArgs a{x, x_row0, d_row0, outp, N, C, h, w, invert, nearest, translation, zoom, magnitude, sigma, angle, pflip, \
             flipmask, (uint32_t)seed, (uint32_t)(seed >> 32), step, d_step, row_global0, draws_in, draws_out, target}

int tn_elastic_apply_img(tn_ctx* ctx, const float* x, int64_t x_row0, const int64_t* d_row0, float* out, int N, int C,
                         int h, int w, int invert, int nearest, double translation, double zoom, double magnitude,
                         int sigma, double angle, float pflip, const uint8_t* flipmask, uint64_t seed, uint32_t step,
                         const uint32_t* d_step, int64_t row_global0, const float* draws_in, float* draws_out,
                         double* target) {
    EI_CHECK("tn_elastic_apply_img");
    EI_ARGS(out);
    return ei_launch<void>(ctx, a);
}

int tn_c8_elastic_apply_img(tn_ctx* ctx, const float* x, int64_t x_row0, const int64_t* d_row0, void* out, int N, int C,
                            int h, int w, int invert, int nearest, double translation, double zoom, double magnitude,
                            int sigma, double angle, float pflip, const uint8_t* flipmask, uint64_t seed, uint32_t step,
                            const uint32_t* d_step, int64_t row_global0, const float* draws_in, float* draws_out,
                            double* target) {
    EI_CHECK("tn_c8_elastic_apply_img");
    TN_REQUIRE((h * w) % 4 == 0 && ((uintptr_t)out & 15) == 0,
               "tn_c8_elastic_apply_img: maps of %d x %d pixels / unaligned output", h, w);
    EI_ARGS(out);
    if (tn_c8_bf16(ctx)) return ei_launch<C8B>(ctx, a);
    return ei_launch<C8H>(ctx, a);
}

}  // extern "C"
