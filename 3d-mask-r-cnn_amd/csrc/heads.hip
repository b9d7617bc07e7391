// Mask R-CNN head glue for gfx950: the small per-ROI ops between the head
// GEMMs/convs (which run on conv3d.hip's MFMA kernels) and the 2-D NMS
// (nms3d.hip, mode 1).
//
//   head_outputs_kernel   fpn_classifier_graph tail (core/models.py:1146-1186):
//                         clip(logits, -10, 10), softmax, bbox reshape
//   head_outputs_bwd_kernel  its backward into the Dense GEMM's output layout
//                         (clip gradient, bbox reshape, zero padding columns)
//   max_norm_kernel       keras.constraints.MaxNorm(axis=0) of the two Dense
//                         kernels after an optimizer step (core/models.py:1160, 1175)
//   refine_kernel         refine_detections_graph per-ROI part
//                         (core/models.py:1415-1500): confidence filter, class-1
//                         deltas, denorm, apply_box_deltas_3d_graph
//                         (core/utils.py:412-458), clip, min size
//   detections_kernel     NMS gather, re-normalise, [max_inst, 8] rows, zero pad
//                         (core/models.py:1503-1524)
//   mask_out_bwd_kernel + mask_out_fold_kernel  backward of mrcnn_mask (1^3 conv,
//                         sigmoid) joined with mrcnn_mask_deconv's ReLU
//                         (core/models.py:1229-1237): g_up and three parameter
//                         gradients in one HBM pass, ordered partial sums
//   add4_kernel           KL.Add of mrcnn_mask_res3 in training mode (core/models.py:1222)
// Compiled with -ffp-contract=off like the other exact-order kernels.
#include <float.h>

#include "common.h"

namespace m3d {

__global__ void head_outputs_kernel(const float* __restrict__ raw, int64_t N, int ldr, int C,
                                    float* __restrict__ logits, float* __restrict__ probs,
                                    float* __restrict__ bbox) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* r = raw + i * ldr;
    float mx = -FLT_MAX;
    for (int c = 0; c < C; ++c) {
        const float v = smin(smax(r[c], -10.0f), 10.0f);     // tf.clip_by_value
        logits[i * C + c] = v;
        mx = smax(mx, v);
    }
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) sum += expf(logits[i * C + c] - mx);
    for (int c = 0; c < C; ++c) probs[i * C + c] = expf(logits[i * C + c] - mx) / sum;
    for (int q = 0; q < 6 * C; ++q) bbox[i * 6 * C + q] = r[C + q];
}

// Backward of head_outputs_kernel into the layout of raw: column c < C takes
// g_logits through tf.clip_by_value's gradient (passes where -10 <= raw <= 10,
// taken on the pre-clip raw), columns [C, 7C) take g_bbox, the padding columns
// [7C, ldr) are zero.  One thread per element of g_raw, written whole.
__global__ void head_outputs_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ g_logits,
                                        const float* __restrict__ g_bbox, int64_t N, int ldr, int C,
                                        float* __restrict__ g_raw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * ldr) return;
    const int64_t n = i / ldr;
    const int c = (int)(i - n * ldr);
    float g = 0.0f;
    if (c < C) {
        const float r = raw[i];
        g = (r >= -10.0f && r <= 10.0f) ? g_logits[n * C + c] : 0.0f;
    } else if (c < 7 * C) {
        g = g_bbox[n * 6 * C + (c - C)];
    }
    g_raw[i] = g;
}

// keras.constraints.MaxNorm(max_value, axis=0) on w [rows][cols] in place: one
// workgroup per column j; n_j = sqrt(sum_i w_ij^2) summed in a fixed order
// (thread t adds rows t, t + 256, ...; LDS tree), then
// w_ij *= clip(n_j, 0, max) / (1e-7 + n_j)   (K.epsilon() = 1e-7).
__global__ __launch_bounds__(256) void max_norm_kernel(float* __restrict__ w, int64_t rows, int64_t cols,
                                                       float max_value) {
    __shared__ float red[256];
    const int64_t j = blockIdx.x;
    float s = 0.0f;
    for (int64_t i = threadIdx.x; i < rows; i += 256) {
        const float v = w[i * cols + j];
        s += v * v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) red[threadIdx.x] += red[threadIdx.x + step];
        __syncthreads();
    }
    const float n = sqrtf(red[0]);
    const float scale = smin(smax(n, 0.0f), max_value) / (1e-7f + n);
    for (int64_t i = threadIdx.x; i < rows; i += 256) w[i * cols + j] *= scale;
}

struct F6 { float v[6]; };

// boxes_px [N,6] refined pixel boxes; nms_boxes [N,4] = (y1,x1,y2,x2) of the
// (y,x) footprint; scores [N] = fg prob if the ROI survives the confidence and
// min-size filters, else -FLT_MAX (skipped by m3d_nms3d), so NMS indices are
// the original ROI indices and the survivors keep their order.
__global__ void refine_kernel(const float* __restrict__ rois, const float* __restrict__ probs,
                              const float* __restrict__ deltas, int64_t N, int C,
                              const float* __restrict__ meta, F6 sd, float min_conf,
                              float* __restrict__ boxes_px, float* __restrict__ nms_boxes,
                              float* __restrict__ scores) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float H = meta[5], W = meta[6], D = meta[7];
    const float fg = probs[i * C + 1];
    const float* dl = deltas + (i * C + 1) * 6;                // class id 1
    const float* r = rois + i * 6;
    const float y1 = r[0] * H, x1 = r[1] * W, z1 = r[2] * D;
    const float y2 = r[3] * H, x2 = r[4] * W, z2 = r[5] * D;
    const float dy = dl[0] * sd.v[0], dx = dl[1] * sd.v[1], dz = dl[2] * sd.v[2];
    float dh = dl[3] * sd.v[3], dw = dl[4] * sd.v[4], dd = dl[5] * sd.v[5];
    const float h = y2 - y1, w = x2 - x1, d = z2 - z1;
    const float cy = y1 + 0.5f * h, cx = x1 + 0.5f * w, cz = z1 + 0.5f * d;
    const float lim = (float)log(1000.0 / 16.0);                // LOG_SCALE_LIMIT (float64 log, as the oracle)
    dh = smin(smax(dh, -lim), lim);
    dw = smin(smax(dw, -lim), lim);
    dd = smin(smax(dd, -lim), lim);
    const float cy2 = cy + dy * h, cx2 = cx + dx * w, cz2 = cz + dz * d;
    // exp through float64 (the oracle's form, oracle/heads_ref.py): bit-identical boxes
    const float h2 = h * (float)exp((double)dh), w2 = w * (float)exp((double)dw), d2 = d * (float)exp((double)dd);
    const float ny1 = cy2 - 0.5f * h2, nx1 = cx2 - 0.5f * w2, nz1 = cz2 - 0.5f * d2;
    float b[6] = {ny1, nx1, nz1, ny1 + h2, nx1 + w2, nz1 + d2};
    const float lo[6] = {H, W, D, H, W, D};
#pragma unroll
    for (int q = 0; q < 6; ++q) b[q] = smin(smax(b[q], 0.0f), lo[q]);
    const bool ok = fg >= min_conf && (b[3] - b[0]) >= 1.0f && (b[4] - b[1]) >= 1.0f &&
                    (b[5] - b[2]) >= 0.5f;
#pragma unroll
    for (int q = 0; q < 6; ++q) boxes_px[i * 6 + q] = b[q];
    nms_boxes[i * 4 + 0] = b[0];
    nms_boxes[i * 4 + 1] = b[1];
    nms_boxes[i * 4 + 2] = b[3];
    nms_boxes[i * 4 + 3] = b[4];
    scores[i] = ok ? fg : -FLT_MAX;
}

__global__ void detections_kernel(const float* __restrict__ boxes_px,
                                  const float* __restrict__ scores,
                                  const int32_t* __restrict__ keep,
                                  const int32_t* __restrict__ num_keep, int max_inst,
                                  const float* __restrict__ meta, float* __restrict__ det) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= max_inst) return;
    float* o = det + (int64_t)j * 8;
    if (j >= *num_keep) {
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = 0.0f;
        return;
    }
    const int i = keep[j];
    const float s[6] = {meta[5], meta[6], meta[7], meta[5], meta[6], meta[7]};
#pragma unroll
    for (int q = 0; q < 6; ++q) o[q] = smin(smax(boxes_px[(int64_t)i * 6 + q] / s[q], 0.0f), 1.0f);
    o[6] = 1.0f;
    o[7] = scores[i];
}

// ---- backward of mrcnn_mask (1^3 conv ch -> C, sigmoid) joined with the ReLU of
// mrcnn_mask_deconv (core/models.py:1229-1237) ---------------------------------
// A rank-C update (C = 2 in the reference) over V = T (2p)^3 rows of ch channels:
// HBM-bound, up read once and g_up written once.  A workgroup owns a contiguous
// run of `rpb` rows (a multiple of MOB_TILE) and walks it in tiles of MOB_TILE
// rows:
//   phase A: thread t forms gl[v][k] = g_mask out (1 - out) of row v = tile + t
//            into LDS and adds it to its running db[k];
//   phase B: TPR = 2^ceil(log2(ch/4)) threads span a row (one float4 of channels
//            each, held for the whole kernel: its 4 x C weights stay in
//            registers), 256 / TPR rows per pass: g_up = (gl . w[c]) (up > 0)
//            stored, dW[c][k] += up gl[k] and dbd[c] += g_up in registers.
// At the end the row groups' registers are summed through LDS in row-group
// order and the workgroup writes one row of partials [ch*C dW | ch dbd | C db];
// mask_out_fold_kernel adds the rows to the three gradients in workgroup order
// (16 slices of consecutive workgroups, then the slices in order).  No atomics:
// the result depends on V, ch and C alone.  CT = 2: the reference's class
// count, unrolled; CT = 8: any C <= 8 (a runtime bound inside the unrolled loops).
// All addresses are 64-bit (no buffer descriptors): no 4 GiB operand bound.
constexpr int MOB_TILE = 256;
constexpr int MOB_FOLD_E = 16, MOB_FOLD_S = 16;

template <int CT>
__global__ __launch_bounds__(256) void mask_out_bwd_kernel(const float* __restrict__ g_mask,
                                                           const float* __restrict__ out,
                                                           const float* __restrict__ up,
                                                           const float* __restrict__ w, int64_t V, int ch, int C,
                                                           int tpr, int64_t rpb, float* __restrict__ g_up,
                                                           float* __restrict__ part) {
    __shared__ float sgl[MOB_TILE * CT];
    __shared__ __attribute__((aligned(16))) float red[1024 * (CT + 1)];
    const int tid = threadIdx.x;
    const int q = tid % tpr, rg = tid / tpr, nrg = 256 / tpr;
    const int L4 = ch >> 2;
    const bool qok = q < L4;
    const int64_t v_begin = (int64_t)blockIdx.x * rpb;
    const int64_t v_end = v_begin + rpb < V ? v_begin + rpb : V;
    float wr[4][CT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < CT; ++k) wr[j][k] = (qok && k < C) ? w[(int64_t)(4 * q + j) * C + k] : 0.0f;
    float dwa[4][CT], dba[4], dbk[CT];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dba[j] = 0.0f;
#pragma unroll
        for (int k = 0; k < CT; ++k) dwa[j][k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < CT; ++k) dbk[k] = 0.0f;
    for (int64_t t0 = v_begin; t0 < v_end; t0 += MOB_TILE) {
        {
            const int64_t v = t0 + tid;
#pragma unroll
            for (int k = 0; k < CT; ++k) {
                float gl = 0.0f;
                if (v < v_end && k < C) {
                    const float o = out[v * C + k];
                    gl = g_mask[v * C + k] * o * (1.0f - o);
                }
                sgl[tid * CT + k] = gl;
                dbk[k] += gl;
            }
        }
        __syncthreads();
        const int rows = (int)(v_end - t0 < MOB_TILE ? v_end - t0 : MOB_TILE);
        if (qok) {
#pragma unroll 4
            for (int r = rg; r < rows; r += nrg) {
                const int64_t off = (t0 + r) * ch + 4 * q;
                const float4 u = *reinterpret_cast<const float4*>(up + off);
                float gl[CT];
#pragma unroll
                for (int k = 0; k < CT; ++k) gl[k] = sgl[r * CT + k];
                const float uu[4] = {u.x, u.y, u.z, u.w};
                float gg[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float s = 0.0f;
#pragma unroll
                    for (int k = 0; k < CT; ++k) {
                        s += gl[k] * wr[j][k];
                        dwa[j][k] += uu[j] * gl[k];
                    }
                    gg[j] = uu[j] > 0.0f ? s : 0.0f;
                    dba[j] += gg[j];
                }
                *reinterpret_cast<float4*>(g_up + off) = make_float4(gg[0], gg[1], gg[2], gg[3]);
            }
        }
        __syncthreads();
    }
    // fold the row groups (fixed order) and the 256 db rows; one partial row per workgroup
    const int nE = ch * (CT + 1);                 // per row group: [c][k < CT | dbd]
    if (qok) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < CT; ++k) red[rg * nE + (4 * q + j) * (CT + 1) + k] = dwa[j][k];
            red[rg * nE + (4 * q + j) * (CT + 1) + CT] = dba[j];
        }
    }
#pragma unroll
    for (int k = 0; k < CT; ++k) sgl[tid * CT + k] = dbk[k];
    __syncthreads();
    float* prow = part + (int64_t)blockIdx.x * ((int64_t)ch * C + ch + C);
    for (int e = tid; e < nE; e += 256) {
        const int c = e / (CT + 1), k = e - c * (CT + 1);
        float s = red[e];
        for (int g = 1; g < nrg; ++g) s += red[g * nE + e];
        if (k == CT) prow[(int64_t)ch * C + c] = s;
        else if (k < C) prow[(int64_t)c * C + k] = s;
    }
    if (tid < C) {
        float s = 0.0f;
        for (int t = 0; t < 256; ++t) s += sgl[t * CT + tid];
        prow[(int64_t)ch * C + ch + tid] = s;
    }
}

// dst[e] += sum over workgroup rows of part[row][e]: MOB_FOLD_S slices of
// consecutive rows summed in row order, then the slices in order.
// e < ch*C -> dW, < ch*C + ch -> the deconv bias gradient, else db.
__global__ __launch_bounds__(256) void mask_out_fold_kernel(const float* __restrict__ part, int64_t nrows, int ne,
                                                            int n_dw, int n_dbd, float* __restrict__ dW,
                                                            float* __restrict__ dbd, float* __restrict__ db) {
    __shared__ float red[MOB_FOLD_S][MOB_FOLD_E];
    const int el = threadIdx.x % MOB_FOLD_E, sl = threadIdx.x / MOB_FOLD_E;
    const int e = blockIdx.x * MOB_FOLD_E + el;
    const int64_t per = (nrows + MOB_FOLD_S - 1) / MOB_FOLD_S;
    const int64_t r0 = sl * per, r1 = r0 + per < nrows ? r0 + per : nrows;
    float s = 0.0f;
    if (e < ne)
        for (int64_t r = r0; r < r1; ++r) s += part[r * ne + e];
    red[sl][el] = s;
    __syncthreads();
    if (sl == 0 && e < ne) {
        for (int g = 1; g < MOB_FOLD_S; ++g) s += red[g][el];
        if (e < n_dw) dW[e] += s;
        else if (e < n_dw + n_dbd) dbd[e - n_dw] += s;
        else db[e - n_dw - n_dbd] += s;
    }
}

// KL.Add of two activated branches (mrcnn_mask_res3, core/models.py:1222) where
// the second comes out of a batch-statistics BN and cannot ride a conv epilogue:
// out = a + b over n floats (n % 4 == 0), float4 lanes, grid-stride.
__global__ __launch_bounds__(256) void add4_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                   float4* __restrict__ out, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 x = a[i], y = b[i];
        out[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
    }
}

// rows per workgroup: a function of V alone (the partial sums' grouping is part of the result's bits)
static int64_t mask_out_rpb(int64_t V) { return V >= ((int64_t)1 << 18) ? 4 * MOB_TILE : MOB_TILE; }

}  // namespace m3d

using namespace m3d;

extern "C" int m3d_add_f32(const float* a, const float* b, float* out, int64_t n, m3d_stream_t s) {
    if (n < 0 || n % 4) return einval("add_f32: n must be a non-negative multiple of 4");
    if (n == 0) return M3D_OK;
    if (!a || !b || !out) return einval("add_f32: null tensor");
    hipLaunchKernelGGL(add4_kernel, dim3(grid_for(n / 4, 256, 1 << 16)), dim3(256), 0, st(s),
                       reinterpret_cast<const float4*>(a), reinterpret_cast<const float4*>(b),
                       reinterpret_cast<float4*>(out), n / 4);
    return check_launch("add4_kernel");
}

static int mask_out_check(int64_t V, int64_t ch, int32_t C) {
    if (V <= 0 || ch <= 0 || C <= 0) return einval("mask_out_bwd: V, ch and C must be positive");
    if (C > 8) return einval("mask_out_bwd: at most 8 classes");
    if (ch % 4 || ch > 1024) return einval("mask_out_bwd: ch must be a multiple of 4, at most 1024");
    if ((V + MOB_TILE - 1) / MOB_TILE > 0x7FFFFFFF) return einval("mask_out_bwd: too many rows");
    return M3D_OK;
}

extern "C" size_t m3d_mask_out_bwd_workspace_bytes(int64_t V, int64_t ch, int32_t C) {
    if (V <= 0 || ch <= 0 || C <= 0 || C > 8 || ch % 4 || ch > 1024) return 0;
    const int64_t rpb = mask_out_rpb(V);
    return sizeof(float) * (size_t)((V + rpb - 1) / rpb) * (size_t)(ch * C + ch + C);
}

extern "C" int m3d_mask_out_bwd(const float* g_mask, const float* out, const float* up, const float* w, int64_t V,
                                int64_t ch, int32_t C, float* g_up, float* dW, float* db, float* d_deconv_bias,
                                void* workspace, size_t ws_bytes, m3d_stream_t s) {
    const int rc = mask_out_check(V, ch, C);
    if (rc) return rc;
    if (!g_mask || !out || !up || !w || !g_up || !dW || !db || !d_deconv_bias)
        return einval("mask_out_bwd: null tensor");
    if (!workspace || ws_bytes < m3d_mask_out_bwd_workspace_bytes(V, ch, C))
        return einval("mask_out_bwd: workspace too small (m3d_mask_out_bwd_workspace_bytes)");
    const int64_t rpb = mask_out_rpb(V);
    const int64_t nblk = (V + rpb - 1) / rpb;
    int tpr = 1;
    while (tpr < ch / 4) tpr <<= 1;
    float* part = static_cast<float*>(workspace);
    if (C == 2)
        hipLaunchKernelGGL(mask_out_bwd_kernel<2>, dim3((unsigned)nblk), dim3(256), 0, st(s), g_mask, out, up, w, V,
                           (int)ch, (int)C, tpr, rpb, g_up, part);
    else
        hipLaunchKernelGGL(mask_out_bwd_kernel<8>, dim3((unsigned)nblk), dim3(256), 0, st(s), g_mask, out, up, w, V,
                           (int)ch, (int)C, tpr, rpb, g_up, part);
    int rc2 = check_launch("mask_out_bwd_kernel");
    if (rc2) return rc2;
    const int ne = (int)(ch * C + ch + C);
    hipLaunchKernelGGL(mask_out_fold_kernel, dim3((unsigned)((ne + MOB_FOLD_E - 1) / MOB_FOLD_E)), dim3(256), 0, st(s),
                       part, nblk, ne, (int)(ch * C), (int)ch, dW, d_deconv_bias, db);
    return check_launch("mask_out_fold_kernel");
}

extern "C" int m3d_head_outputs(const float* raw, int64_t N, int64_t ldr, int32_t num_classes,
                                float* logits, float* probs, float* bbox, m3d_stream_t s) {
    if (N < 0 || num_classes <= 0 || ldr < 7 * (int64_t)num_classes)
        return einval("head_outputs: raw rows must hold num_classes logits + 6*num_classes deltas");
    if (N == 0) return M3D_OK;
    hipLaunchKernelGGL(head_outputs_kernel, dim3(grid_for(N, 256)), dim3(256), 0, st(s), raw, N,
                       (int)ldr, (int)num_classes, logits, probs, bbox);
    return check_launch("head_outputs_kernel");
}

extern "C" int m3d_head_outputs_bwd(const float* raw, const float* g_logits, const float* g_bbox, int64_t N,
                                    int64_t ldr, int32_t num_classes, float* g_raw, m3d_stream_t s) {
    if (N < 0 || num_classes <= 0 || ldr < 7 * (int64_t)num_classes || ldr > 0x7FFFFFFF)
        return einval("head_outputs_bwd: raw rows must hold num_classes logits + 6*num_classes deltas");
    if (N == 0) return M3D_OK;
    hipLaunchKernelGGL(head_outputs_bwd_kernel, dim3(grid_for(N * ldr, 256)), dim3(256), 0, st(s), raw, g_logits,
                       g_bbox, N, (int)ldr, (int)num_classes, g_raw);
    return check_launch("head_outputs_bwd_kernel");
}

extern "C" int m3d_max_norm(float* w, int64_t rows, int64_t cols, float max_value, m3d_stream_t s) {
    if (rows <= 0 || cols <= 0 || cols > 0x7FFFFFFF) return einval("max_norm: rows and cols must be positive");
    if (!(max_value >= 0.0f)) return einval("max_norm: max_value must be non-negative");
    hipLaunchKernelGGL(max_norm_kernel, dim3((unsigned)cols), dim3(256), 0, st(s), w, rows, cols, max_value);
    return check_launch("max_norm_kernel");
}

extern "C" int m3d_refine_detections(const float* rois, const float* probs, const float* deltas,
                                     int64_t N, int32_t num_classes, const float* image_meta,
                                     const float bbox_std_dev[6], float min_conf,
                                     float* boxes_px, float* nms_boxes, float* scores,
                                     m3d_stream_t s) {
    if (N < 0 || num_classes < 2) return einval("refine_detections: need num_classes >= 2");
    if (N == 0) return M3D_OK;
    F6 sd{};
    for (int q = 0; q < 6; ++q) sd.v[q] = bbox_std_dev[q];
    hipLaunchKernelGGL(refine_kernel, dim3(grid_for(N, 256)), dim3(256), 0, st(s), rois, probs, deltas,
                       N, (int)num_classes, image_meta, sd, min_conf, boxes_px, nms_boxes, scores);
    return check_launch("refine_kernel");
}

extern "C" int m3d_detections_gather(const float* boxes_px, const float* scores,
                                     const int32_t* keep, const int32_t* num_keep,
                                     int32_t max_inst, const float* image_meta, float* det,
                                     m3d_stream_t s) {
    if (max_inst < 0) return einval("detections_gather: negative DETECTION_MAX_INSTANCES");
    if (max_inst == 0) return M3D_OK;
    hipLaunchKernelGGL(detections_kernel, dim3(grid_for(max_inst, 256)), dim3(256), 0, st(s), boxes_px,
                       scores, keep, num_keep, max_inst, image_meta, det);
    return check_launch("detections_kernel");
}
