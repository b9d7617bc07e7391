// Batch-statistics BatchNorm for gfx950: Keras 2.3.1 BatchNormalization.call(
// training=True) on the TF backend's non-fused path, as the reference's head
// training graph runs it (fpn_classifier_graph / build_fpn_mask_graph with
// train_bn=True, core/models.py:1121-1234, 5602-5668).  TimeDistributed folds
// [B,N,...] to [B*N,...], so the statistics run over all M rows of z [M, C].
//
//   forward   mean = sum z / M;  var = sum (z - mean)^2 / M  (two passes);
//             rstd = 1/sqrt(var + eps);  y = act(gamma (z - mean) rstd + beta);
//             moving_mean     = moving_mean mom + mean (1 - mom)
//             moving_variance = moving_variance mom + var M/(M - (1 + eps)) (1 - mom)
//   backward  dpre = dy (y > 0);  dbeta = sum dpre;  dgamma = sum dpre xhat;
//             dz = gamma rstd (dpre - dbeta/M - xhat dgamma/M)
//
// Thread layout of every reducing kernel: T threads across channel quads
// (float4), R = 256/T row groups; thread (tx, ty) adds rows ty, ty + step, ...
// into four accumulators in turn, the row groups are folded by a fixed LDS
// tree.  No float atomics anywhere: results are bit-identical run to run.
//
// Two regimes, switched on M3D_BN_TRAIN_FEW_ROWS_MAX:
//   few rows   (M <= it; the classifier head: 128..1024 ROIs x 512..1024
//              channels): one workgroup owns a strip of 16 channels (T = 4,
//              R = 64) and makes every pass itself -- statistics and output in
//              one launch, no partials round trip; grid = C/16 workgroups.
//              The strip (64 B x M) stays in L2 between the passes.
//   many rows  (the mask head: ~10^5..10^6 ROI voxels x 256 channels): a
//              (row block, channel group) grid writes per-block partial sums,
//              a second kernel folds them in block order, a grid-stride
//              elementwise kernel applies the result.
#include "common.h"

namespace m3d {

constexpr int BNT_FEW_T = 4;            // few rows: channel quads per workgroup (16 channels)
constexpr int BNT_MANY_BLOCKS = 2048;   // many rows: cap of row blocks x channel groups

struct BntGeo {
    int few, T, R, groups;
    int64_t gx;
};

static BntGeo bnt_geo(int64_t M, int64_t C) {
    BntGeo g{};
    const int quads = (int)(C / 4);
    g.few = M <= M3D_BN_TRAIN_FEW_ROWS_MAX;
    if (g.few) {
        g.T = BNT_FEW_T;
        g.gx = 1;
    } else {
        g.T = 1;
        while (g.T < quads && g.T < 64) g.T <<= 1;
    }
    g.R = 256 / g.T;
    g.groups = (quads + g.T - 1) / g.T;
    if (!g.few) {
        g.gx = (M + g.R - 1) / g.R;
        const int64_t cap = BNT_MANY_BLOCKS / g.groups > 0 ? BNT_MANY_BLOCKS / g.groups : 1;
        if (g.gx > cap) g.gx = cap;
    }
    return g;
}

__device__ __forceinline__ float4 f4add(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// Fold the block's R row groups (thread = ty * T + tx) in a fixed tree; every
// thread returns the total of its channel quad tx.  All 256 threads call it.
__device__ __forceinline__ float4 bnt_block_fold(float4 v, int T, float4* red) {
    const int R = 256 / T, ty = threadIdx.x / T, tx = threadIdx.x % T;
    red[threadIdx.x] = v;
    __syncthreads();
    for (int step = R / 2; step > 0; step >>= 1) {
        if (ty < step) red[threadIdx.x] = f4add(red[threadIdx.x], red[threadIdx.x + step * T]);
        __syncthreads();
    }
    const float4 r = red[tx];
    __syncthreads();                    // red is reused by the next fold
    return r;
}

// Per-thread sums over rows r0, r0 + step, ... < M of its channel quad at c:
// four accumulators taken in turn, combined pairwise (fixed order).
template <typename F>
__device__ __forceinline__ float4 bnt_rows(int64_t M, int64_t r0, int64_t step, F f) {
    float4 a[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
    int64_t r = r0;
    for (; r + 3 * step < M; r += 4 * step) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = f4add(a[u], f(r + u * step));
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)          // at most three rows are left
        if (r + u * step < M) a[u] = f4add(a[u], f(r + u * step));
    return f4add(f4add(a[0], a[1]), f4add(a[2], a[3]));
}

struct F4x2 {
    float4 a, b;
};
// two sums from one pass over the rows (same order as bnt_rows for each)
template <typename F>
__device__ __forceinline__ F4x2 bnt_rows2(int64_t M, int64_t r0, int64_t step, F f) {
    float4 a[4] = {f4zero(), f4zero(), f4zero(), f4zero()}, b[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
    int64_t r = r0;
    for (; r + 3 * step < M; r += 4 * step) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const F4x2 v = f(r + u * step);
            a[u] = f4add(a[u], v.a);
            b[u] = f4add(b[u], v.b);
        }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {        // at most three rows are left
        if (r + u * step < M) {
            const F4x2 v = f(r + u * step);
            a[u] = f4add(a[u], v.a);
            b[u] = f4add(b[u], v.b);
        }
    }
    return F4x2{f4add(f4add(a[0], a[1]), f4add(a[2], a[3])), f4add(f4add(b[0], b[1]), f4add(b[2], b[3]))};
}

__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }

__device__ __forceinline__ float4 bnt_var_to_rstd(float4 var, float eps) {
    return make_float4(1.0f / sqrtf(var.x + eps), 1.0f / sqrtf(var.y + eps), 1.0f / sqrtf(var.z + eps),
                       1.0f / sqrtf(var.w + eps));
}

// save_mean / save_rstd and the moving statistics of one channel quad (one thread per quad)
__device__ __forceinline__ void bnt_store_stats(int c, float4 mean, float4 var, float4 rstd, int64_t M, float eps,
                                                float mom, float* __restrict__ save_mean,
                                                float* __restrict__ save_rstd, float* __restrict__ mm,
                                                float* __restrict__ mv) {
    *(float4*)(save_mean + c) = mean;
    *(float4*)(save_rstd + c) = rstd;
    if (!mm) return;
    // Keras: unbiased = var * sample_size / (sample_size - (1 + eps)), '1 + eps' kept literally
    const float unb = (float)M / ((float)M - (1.0f + eps));
    const float keep = 1.0f - mom;
    const float m4[4] = {mean.x, mean.y, mean.z, mean.w}, v4[4] = {var.x, var.y, var.z, var.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        mm[c + q] = mm[c + q] * mom + m4[q] * keep;
        mv[c + q] = mv[c + q] * mom + (v4[q] * unb) * keep;
    }
}

__device__ __forceinline__ float4 bnt_norm(float4 z, float4 mean, float4 rstd, float4 g, float4 b, int relu) {
    float4 y = make_float4(g.x * ((z.x - mean.x) * rstd.x) + b.x, g.y * ((z.y - mean.y) * rstd.y) + b.y,
                           g.z * ((z.z - mean.z) * rstd.z) + b.z, g.w * ((z.w - mean.w) * rstd.w) + b.w);
    if (relu) {
        y.x = smax(y.x, 0.f); y.y = smax(y.y, 0.f); y.z = smax(y.z, 0.f); y.w = smax(y.w, 0.f);
    }
    return y;
}

__device__ __forceinline__ float4 bnt_sq(float4 z, float4 mean) {
    const float a = z.x - mean.x, b = z.y - mean.y, c = z.z - mean.z, d = z.w - mean.w;
    return make_float4(a * a, b * b, c * c, d * d);
}

// dpre of one quad: dy masked by y > 0
__device__ __forceinline__ float4 bnt_dpre(const float* dy, const float* y, int64_t off, int relu) {
    float4 g = ld4(dy + off);
    if (relu) {
        const float4 v = ld4(y + off);
        if (!(v.x > 0.f)) g.x = 0.f;
        if (!(v.y > 0.f)) g.y = 0.f;
        if (!(v.z > 0.f)) g.z = 0.f;
        if (!(v.w > 0.f)) g.w = 0.f;
    }
    return g;
}

__device__ __forceinline__ float4 bnt_xhat(float4 z, float4 mean, float4 rstd) {
    return make_float4((z.x - mean.x) * rstd.x, (z.y - mean.y) * rstd.y, (z.z - mean.z) * rstd.z,
                       (z.w - mean.w) * rstd.w);
}

// (dpre, dpre * xhat) of one quad
__device__ __forceinline__ F4x2 bnt_dpre_xhat(const float* dy, const float* y, const float* z, int64_t off, int relu,
                                              float4 mean, float4 rstd) {
    const float4 d = bnt_dpre(dy, y, off, relu), xh = bnt_xhat(ld4(z + off), mean, rstd);
    return F4x2{d, make_float4(d.x * xh.x, d.y * xh.y, d.z * xh.z, d.w * xh.w)};
}

__device__ __forceinline__ float4 bnt_dz(float4 dpre, float4 xh, float4 gr, float4 mb, float4 mg) {
    return make_float4(gr.x * ((dpre.x - mb.x) - xh.x * mg.x), gr.y * ((dpre.y - mb.y) - xh.y * mg.y),
                       gr.z * ((dpre.z - mb.z) - xh.z * mg.z), gr.w * ((dpre.w - mb.w) - xh.w * mg.w));
}

// ---- few rows: one workgroup per 16-channel strip, every pass in one launch ----
// y may alias z: a workgroup reads its whole strip (both statistics passes, a
// barrier after each) before it writes any of it, and no other workgroup
// touches the strip.
__global__ __launch_bounds__(256) void bnt_few_fwd_kernel(const float* z, int64_t M, int C,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float mom,
                                                          int relu, float* y, float* __restrict__ save_mean,
                                                          float* __restrict__ save_rstd, float* __restrict__ mm,
                                                          float* __restrict__ mv) {
    __shared__ float4 red[256];
    const int tx = threadIdx.x % BNT_FEW_T, ty = threadIdx.x / BNT_FEW_T;
    const int R = 256 / BNT_FEW_T;
    const int c = (blockIdx.x * BNT_FEW_T + tx) * 4;
    const bool in = c < C;
    const float* zc = z + (in ? c : 0);
    float4 s = f4zero();
    if (in) s = bnt_rows(M, ty, R, [&](int64_t r) { return ld4(zc + r * C); });
    s = bnt_block_fold(s, BNT_FEW_T, red);
    const float fm = (float)M;
    const float4 mean = make_float4(s.x / fm, s.y / fm, s.z / fm, s.w / fm);
    float4 q = f4zero();
    if (in) q = bnt_rows(M, ty, R, [&](int64_t r) { return bnt_sq(ld4(zc + r * C), mean); });
    q = bnt_block_fold(q, BNT_FEW_T, red);
    if (!in) return;
    const float4 var = make_float4(q.x / fm, q.y / fm, q.z / fm, q.w / fm);
    const float4 rstd = bnt_var_to_rstd(var, eps);
    if (ty == 0) bnt_store_stats(c, mean, var, rstd, M, eps, mom, save_mean, save_rstd, mm, mv);
    const float4 g = ld4(gamma + c), b = ld4(beta + c);
    for (int64_t r = ty; r < M; r += R) *(float4*)(y + r * C + c) = bnt_norm(ld4(zc + r * C), mean, rstd, g, b, relu);
}

// dz may alias dy (same argument as the forward's y / z).
__global__ __launch_bounds__(256) void bnt_few_bwd_kernel(const float* dy, const float* __restrict__ y,
                                                          const float* __restrict__ z, int64_t M, int C,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ save_mean,
                                                          const float* __restrict__ save_rstd, int relu,
                                                          float* dz, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta) {
    __shared__ float4 red[256];
    const int tx = threadIdx.x % BNT_FEW_T, ty = threadIdx.x / BNT_FEW_T;
    const int R = 256 / BNT_FEW_T;
    const int c = (blockIdx.x * BNT_FEW_T + tx) * 4;
    const bool in = c < C;
    float4 mean = f4zero(), rstd = f4zero();
    if (in) { mean = ld4(save_mean + c); rstd = ld4(save_rstd + c); }
    float4 sb = f4zero(), sg = f4zero();
    if (in) {
        const F4x2 v = bnt_rows2(M, ty, R, [&](int64_t r) { return bnt_dpre_xhat(dy, y, z, r * C + c, relu, mean, rstd); });
        sb = v.a;
        sg = v.b;
    }
    sb = bnt_block_fold(sb, BNT_FEW_T, red);
    sg = bnt_block_fold(sg, BNT_FEW_T, red);
    if (!in) return;
    if (ty == 0) {
        dbeta[c] += sb.x; dbeta[c + 1] += sb.y; dbeta[c + 2] += sb.z; dbeta[c + 3] += sb.w;
        dgamma[c] += sg.x; dgamma[c + 1] += sg.y; dgamma[c + 2] += sg.z; dgamma[c + 3] += sg.w;
    }
    const float fm = (float)M;
    const float4 g = ld4(gamma + c);
    const float4 gr = make_float4(g.x * rstd.x, g.y * rstd.y, g.z * rstd.z, g.w * rstd.w);
    const float4 mb = make_float4(sb.x / fm, sb.y / fm, sb.z / fm, sb.w / fm);
    const float4 mg = make_float4(sg.x / fm, sg.y / fm, sg.z / fm, sg.w / fm);
    for (int64_t r = ty; r < M; r += R) {
        const int64_t off = r * C + c;
        *(float4*)(dz + off) = bnt_dz(bnt_dpre(dy, y, off, relu), bnt_xhat(ld4(z + off), mean, rstd), gr, mb, mg);
    }
}

// ---- many rows: per-block partials, fixed-order fold, elementwise apply --------
// MODE 0: sum z -> part[0];  1: sum (z - mean)^2 -> part[0];
// MODE 2: sum dpre -> part[0], sum dpre xhat -> part[1]   (part[a] is [gx][C])
template <int MODE>
__global__ __launch_bounds__(256) void bnt_part_kernel(const float* __restrict__ a, const float* __restrict__ y,
                                                       const float* __restrict__ z, int64_t M, int C, int T,
                                                       const float* __restrict__ mean_,
                                                       const float* __restrict__ rstd_, int relu,
                                                       float* __restrict__ part) {
    __shared__ float4 red[256];
    const int R = 256 / T, tx = threadIdx.x % T, ty = threadIdx.x / T;
    const int c = (blockIdx.y * T + tx) * 4;
    const bool in = c < C;
    const int64_t r0 = (int64_t)blockIdx.x * R + ty, step = (int64_t)gridDim.x * R;
    float4 mean = f4zero(), rstd = f4zero();
    if (in && MODE >= 1) mean = ld4(mean_ + c);
    if (in && MODE == 2) rstd = ld4(rstd_ + c);
    float4 s0 = f4zero(), s1 = f4zero();
    if (in) {
        if (MODE == 0) s0 = bnt_rows(M, r0, step, [&](int64_t r) { return ld4(a + r * C + c); });
        if (MODE == 1) s0 = bnt_rows(M, r0, step, [&](int64_t r) { return bnt_sq(ld4(a + r * C + c), mean); });
        if (MODE == 2) {
            const F4x2 v =
                bnt_rows2(M, r0, step, [&](int64_t r) { return bnt_dpre_xhat(a, y, z, r * C + c, relu, mean, rstd); });
            s0 = v.a;
            s1 = v.b;
        }
    }
    s0 = bnt_block_fold(s0, T, red);
    if (MODE == 2) s1 = bnt_block_fold(s1, T, red);
    if (ty == 0 && in) {
        *(float4*)(part + (int64_t)blockIdx.x * C + c) = s0;
        if (MODE == 2) *(float4*)(part + ((int64_t)gridDim.x + blockIdx.x) * C + c) = s1;
    }
}

// Fold part[a][gx][C] over the gx row blocks: 16 channels per workgroup (4
// quads x 64 block groups, then the LDS tree).
// MODE 0: save_mean = total / M
// MODE 1: var = total / M -> save_rstd, moving statistics (mean from save_mean)
// MODE 2: sums[0] = dbeta total, sums[1] = dgamma total (this call's, for dz);
//         dbeta += , dgamma +=
template <int MODE>
__global__ __launch_bounds__(256) void bnt_fold_kernel(const float* __restrict__ part, int gx, int64_t M, int C,
                                                       float eps, float mom, float* __restrict__ save_mean,
                                                       float* __restrict__ save_rstd, float* __restrict__ mm,
                                                       float* __restrict__ mv, float* __restrict__ sums,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float4 red[256];
    const int tx = threadIdx.x % 4, ty = threadIdx.x / 4;
    const int c = (blockIdx.x * 4 + tx) * 4;
    const bool in = c < C;
    float4 s0 = f4zero(), s1 = f4zero();
    if (in) {
        s0 = bnt_rows(gx, ty, 64, [&](int64_t b) { return ld4(part + b * C + c); });
        if (MODE == 2) s1 = bnt_rows(gx, ty, 64, [&](int64_t b) { return ld4(part + ((int64_t)gx + b) * C + c); });
    }
    s0 = bnt_block_fold(s0, 4, red);
    if (MODE == 2) s1 = bnt_block_fold(s1, 4, red);
    if (!in || ty != 0) return;
    const float fm = (float)M;
    if (MODE == 0) *(float4*)(save_mean + c) = make_float4(s0.x / fm, s0.y / fm, s0.z / fm, s0.w / fm);
    if (MODE == 1) {
        const float4 var = make_float4(s0.x / fm, s0.y / fm, s0.z / fm, s0.w / fm);
        bnt_store_stats(c, ld4(save_mean + c), var, bnt_var_to_rstd(var, eps), M, eps, mom, save_mean, save_rstd,
                        mm, mv);
    }
    if (MODE == 2) {
        *(float4*)(sums + c) = s0;
        *(float4*)(sums + C + c) = s1;
        dbeta[c] += s0.x; dbeta[c + 1] += s0.y; dbeta[c + 2] += s0.z; dbeta[c + 3] += s0.w;
        dgamma[c] += s1.x; dgamma[c + 1] += s1.y; dgamma[c + 2] += s1.z; dgamma[c + 3] += s1.w;
    }
}

// elementwise over the M*C/4 quads (grid-stride); in-place safe (one thread
// reads then writes each quad)
__global__ __launch_bounds__(256) void bnt_apply_fwd_kernel(const float* z, int64_t nq, int qc,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ mean_,
                                                            const float* __restrict__ rstd_, int relu, float* y) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += step) {
        const int c = (int)(i % qc) * 4;
        *(float4*)(y + i * 4) =
            bnt_norm(ld4(z + i * 4), ld4(mean_ + c), ld4(rstd_ + c), ld4(gamma + c), ld4(beta + c), relu);
    }
}

__global__ __launch_bounds__(256) void bnt_apply_bwd_kernel(const float* dy, const float* __restrict__ y,
                                                            const float* __restrict__ z, int64_t nq, int qc,
                                                            int64_t M, const float* __restrict__ gamma,
                                                            const float* __restrict__ mean_,
                                                            const float* __restrict__ rstd_,
                                                            const float* __restrict__ sums, int relu, float* dz) {
    const int64_t step = (int64_t)gridDim.x * 256;
    const float fm = (float)M;
    const int C = qc * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += step) {
        const int c = (int)(i % qc) * 4;
        const float4 g = ld4(gamma + c), mean = ld4(mean_ + c), rstd = ld4(rstd_ + c);
        const float4 sb = ld4(sums + c), sg = ld4(sums + C + c);
        const float4 gr = make_float4(g.x * rstd.x, g.y * rstd.y, g.z * rstd.z, g.w * rstd.w);
        const float4 mb = make_float4(sb.x / fm, sb.y / fm, sb.z / fm, sb.w / fm);
        const float4 mg = make_float4(sg.x / fm, sg.y / fm, sg.z / fm, sg.w / fm);
        *(float4*)(dz + i * 4) =
            bnt_dz(bnt_dpre(dy, y, i * 4, relu), bnt_xhat(ld4(z + i * 4), mean, rstd), gr, mb, mg);
    }
}

static size_t bnt_ws_bytes(const BntGeo& g, int64_t C) {
    // backward: part[2][gx][C] + sums[2][C]; the forward needs part[gx][C] of it
    return g.few ? 0 : sizeof(float) * (2 * (size_t)g.gx + 2) * (size_t)C;
}

static int bnt_check(const char* what, int64_t M, int64_t C) {
    if (M < 0 || C <= 0) {
        set_error("%s: M and C must be positive", what);
        return M3D_EINVAL;
    }
    if (C % 4) {
        set_error("%s: C must be a multiple of 4", what);
        return M3D_EINVAL;
    }
    if (M < 2) {
        set_error("%s: batch statistics need M >= 2 rows (Keras' variance correction divides by M - (1 + eps))",
                  what);
        return M3D_EINVAL;
    }
    if (C > 0x7FFFFFF0) {
        set_error("%s: C too large", what);
        return M3D_EINVAL;
    }
    return M3D_OK;
}

}  // namespace m3d

using namespace m3d;

extern "C" int64_t m3d_bn_train_few_rows_max(void) { return M3D_BN_TRAIN_FEW_ROWS_MAX; }

extern "C" size_t m3d_bn_train_workspace_bytes(int64_t M, int64_t C) {
    if (M < 2 || C <= 0 || C % 4) return 0;
    return bnt_ws_bytes(bnt_geo(M, C), C);
}

extern "C" int m3d_bn_train_fwd(const float* z, int64_t M, int64_t C, const float* gamma, const float* beta,
                                float eps, float momentum, int32_t relu, float* y, float* save_mean,
                                float* save_rstd, float* moving_mean, float* moving_variance, void* workspace,
                                size_t ws_bytes, m3d_stream_t s) {
    if (int rc = bnt_check("bn_train_fwd", M, C)) return rc;
    if ((moving_mean == nullptr) != (moving_variance == nullptr))
        return einval("bn_train_fwd: moving_mean and moving_variance must be given together (both NULL: no update)");
    if (!(eps > 0.0f)) return einval("bn_train_fwd: eps must be positive");
    const BntGeo g = bnt_geo(M, C);
    if (ws_bytes < bnt_ws_bytes(g, C) || (!g.few && !workspace)) return einval("bn_train_fwd: workspace too small");
    const int r = relu ? 1 : 0;
    if (g.few) {
        hipLaunchKernelGGL(bnt_few_fwd_kernel, dim3((unsigned)g.groups), dim3(256), 0, st(s), z, M, (int)C, gamma,
                           beta, eps, momentum, r, y, save_mean, save_rstd, moving_mean, moving_variance);
        return check_launch("bnt_few_fwd_kernel");
    }
    float* part = static_cast<float*>(workspace);
    const dim3 pg((unsigned)g.gx, (unsigned)g.groups), fg((unsigned)((C + 15) / 16));
    hipLaunchKernelGGL(bnt_part_kernel<0>, pg, dim3(256), 0, st(s), z, nullptr, nullptr, M, (int)C, g.T, nullptr,
                       nullptr, 0, part);
    hipLaunchKernelGGL(bnt_fold_kernel<0>, fg, dim3(256), 0, st(s), part, (int)g.gx, M, (int)C, eps, momentum,
                       save_mean, save_rstd, nullptr, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(bnt_part_kernel<1>, pg, dim3(256), 0, st(s), z, nullptr, nullptr, M, (int)C, g.T, save_mean,
                       nullptr, 0, part);
    hipLaunchKernelGGL(bnt_fold_kernel<1>, fg, dim3(256), 0, st(s), part, (int)g.gx, M, (int)C, eps, momentum,
                       save_mean, save_rstd, moving_mean, moving_variance, nullptr, nullptr, nullptr);
    const int64_t nq = M * (C / 4);
    hipLaunchKernelGGL(bnt_apply_fwd_kernel, dim3(grid_for(nq, 256, 2048)), dim3(256), 0, st(s), z, nq,
                       (int)(C / 4), gamma, beta, save_mean, save_rstd, r, y);
    return check_launch("bn_train_fwd (many rows)");
}

extern "C" int m3d_bn_train_bwd(const float* dy, const float* y, const float* z, int64_t M, int64_t C,
                                const float* gamma, const float* save_mean, const float* save_rstd, int32_t relu,
                                float* dz, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                                m3d_stream_t s) {
    if (int rc = bnt_check("bn_train_bwd", M, C)) return rc;
    if (relu && !y) return einval("bn_train_bwd: relu needs y");
    const BntGeo g = bnt_geo(M, C);
    if (ws_bytes < bnt_ws_bytes(g, C) || (!g.few && !workspace)) return einval("bn_train_bwd: workspace too small");
    const int r = relu ? 1 : 0;
    if (g.few) {
        hipLaunchKernelGGL(bnt_few_bwd_kernel, dim3((unsigned)g.groups), dim3(256), 0, st(s), dy, y, z, M, (int)C,
                           gamma, save_mean, save_rstd, r, dz, dgamma, dbeta);
        return check_launch("bnt_few_bwd_kernel");
    }
    float* part = static_cast<float*>(workspace);
    float* sums = part + 2 * g.gx * C;
    hipLaunchKernelGGL(bnt_part_kernel<2>, dim3((unsigned)g.gx, (unsigned)g.groups), dim3(256), 0, st(s), dy, y, z,
                       M, (int)C, g.T, save_mean, save_rstd, r, part);
    hipLaunchKernelGGL(bnt_fold_kernel<2>, dim3((unsigned)((C + 15) / 16)), dim3(256), 0, st(s), part, (int)g.gx, M,
                       (int)C, 0.0f, 0.0f, nullptr, nullptr, nullptr, nullptr, sums, dgamma, dbeta);
    const int64_t nq = M * (C / 4);
    hipLaunchKernelGGL(bnt_apply_bwd_kernel, dim3(grid_for(nq, 256, 2048)), dim3(256), 0, st(s), dy, y, z, nq,
                       (int)(C / 4), M, gamma, save_mean, save_rstd, sums, r, dz);
    return check_launch("bn_train_bwd (many rows)");
}
