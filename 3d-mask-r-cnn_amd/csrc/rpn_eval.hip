// RPN evaluation: one image's proposals scored against its ground-truth boxes
// (m3d_rpn_eval_proposals, include/m3d.h; the restatement is tests/rpnevalref.py).
//
// Three launches on the caller's stream:
//   re_init_kernel    assoc = -1, first_hit = INT32_MAX, counts = {0, INT32_MAX}
//   re_score_kernel   one proposal per thread, RE_CHUNK proposals per workgroup.  The
//                     GT boxes (corner-normalised, with their volumes) are staged in LDS
//                     and every thread walks all G of them; the row minima are taken in
//                     LDS first and each workgroup sends at most one atomic per (t, g).
//   re_finish_kernel  matched[g] = the clamped pixel box of row assoc[g]
// Every cross-thread result is an integer minimum or an integer count, so the outputs
// do not depend on which wave or workgroup arrives first.  All float arithmetic is
// scalar float32 in a pinned order; the build's -ffp-contract=off keeps the products
// and sums apart.
#include "common.h"

namespace m3d {

constexpr int RE_CHUNK = 256;       // proposals (= threads) per workgroup
constexpr int RE_MAX_G = 512;
constexpr int RE_MAX_T = 8;
constexpr int RE_NONE = 0x7FFFFFFF;

// the clamp of np.clip on float32: NaN stays NaN (and fails the validity compare)
__device__ __forceinline__ float re_clip(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// row j's pixel box: float32(roi * (H,W,D,H,W,D)), the low corner clamped to [0, size],
// the high corner to [1, size]; true when every extent is strictly positive
__device__ __forceinline__ bool re_pixel_box(const float* __restrict__ roi, float fH, float fW, float fD, float b[6]) {
    b[0] = re_clip(roi[0] * fH, 0.0f, fH);
    b[1] = re_clip(roi[1] * fW, 0.0f, fW);
    b[2] = re_clip(roi[2] * fD, 0.0f, fD);
    b[3] = re_clip(roi[3] * fH, 1.0f, fH);
    b[4] = re_clip(roi[4] * fW, 1.0f, fW);
    b[5] = re_clip(roi[5] * fD, 1.0f, fD);
    return b[3] > b[0] && b[4] > b[1] && b[5] > b[2];
}

__global__ void re_init_kernel(int32_t* __restrict__ assoc, int32_t* __restrict__ first_hit,
                               int32_t* __restrict__ counts, int G, int TG) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < G) assoc[i] = -1;
    if (i < TG) first_hit[i] = RE_NONE;
    if (i == 0) {
        counts[0] = 0;
        counts[1] = RE_NONE;
    }
}

__global__ __launch_bounds__(RE_CHUNK) void re_score_kernel(
    const float* __restrict__ rois, const float* __restrict__ gt, int R, int G, float fH, float fW, float fD,
    int kmatch, double match_thr, const float* __restrict__ grid, int T, unsigned* __restrict__ assoc,
    int32_t* __restrict__ first_hit, int32_t* __restrict__ counts, float* __restrict__ iou) {
    __shared__ float s_gt[RE_MAX_G * 7];                 // y1 x1 z1 y2 x2 z2 (normalised corners), volume
    __shared__ int s_min[(RE_MAX_T + 1) * RE_MAX_G];     // [0,G): assoc, then first_hit [T,G]
    __shared__ float s_grid[RE_MAX_T];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x;
    for (int g = tid; g < G; g += RE_CHUNK) {
        const float* p = gt + (size_t)g * 6;
        const float y1 = fminf(p[0], p[3]), y2 = fmaxf(p[0], p[3]);
        const float x1 = fminf(p[1], p[4]), x2 = fmaxf(p[1], p[4]);
        const float z1 = fminf(p[2], p[5]), z2 = fmaxf(p[2], p[5]);
        float* q = s_gt + g * 7;
        q[0] = y1, q[1] = x1, q[2] = z1, q[3] = y2, q[4] = x2, q[5] = z2;
        q[6] = ((y2 - y1) * (x2 - x1)) * (z2 - z1);
    }
    for (int i = tid; i < (T + 1) * G; i += RE_CHUNK) s_min[i] = RE_NONE;
    if (tid < T) s_grid[tid] = grid[tid];
    if (tid == 0) {
        s_cnt[0] = 0;
        s_cnt[1] = RE_NONE;
    }
    __syncthreads();

    const int j = blockIdx.x * RE_CHUNK + tid;
    float b[6];
    const bool valid = j < R && re_pixel_box(rois + (size_t)j * 6, fH, fW, fD, b);
    if (valid) {
        // a valid row's corners are ordered already: its corner normalisation is the identity
        const float vol = ((b[3] - b[0]) * (b[4] - b[1])) * (b[5] - b[2]);
        float best = 0.0f;
        int best_g = 0;
        for (int g = 0; g < G; ++g) {
            const float* q = s_gt + g * 7;               // every lane reads the same words: an LDS broadcast
            const float h = fmaxf(fminf(q[3], b[3]) - fmaxf(q[0], b[0]), 0.0f);
            const float w = fmaxf(fminf(q[4], b[4]) - fmaxf(q[1], b[1]), 0.0f);
            const float d = fmaxf(fminf(q[5], b[5]) - fmaxf(q[2], b[2]), 0.0f);
            const float inter = (h * w) * d;
            const float uni = fmaxf((q[6] + vol) - inter, 1e-10f);
            const float v = fminf(fmaxf(inter / uni, 0.0f), 1.0f);
            if (iou != nullptr) iou[(size_t)g * R + j] = v;
            if (g == 0 || v > best) best = v, best_g = g;              // the first maximum
            for (int t = 0; t < T; ++t)
                if (v >= s_grid[t] && j < s_min[(t + 1) * G + g]) atomicMin(&s_min[(t + 1) * G + g], j);
        }
        if (j < kmatch) {
            atomicAdd(&s_cnt[0], 1);
            if ((double)best > match_thr) atomicMin(&s_min[best_g], j);
        }
        atomicMin(&s_cnt[1], j);
    } else if (j < R && iou != nullptr) {
        for (int g = 0; g < G; ++g) iou[(size_t)g * R + j] = 0.0f;
    }
    __syncthreads();

    // one atomic per (t, g) this workgroup has a row for; -1 is the largest unsigned, so
    // the unsigned minimum over row indices leaves assoc at -1 where nothing matched
    for (int i = tid; i < (T + 1) * G; i += RE_CHUNK) {
        const int v = s_min[i];
        if (v == RE_NONE) continue;
        if (i < G)
            atomicMin(&assoc[i], (unsigned)v);
        else
            atomicMin(&first_hit[i - G], v);
    }
    if (tid == 0) {
        if (s_cnt[0] != 0) atomicAdd(&counts[0], s_cnt[0]);
        if (s_cnt[1] != RE_NONE) atomicMin(&counts[1], s_cnt[1]);
    }
}

__global__ void re_finish_kernel(const float* __restrict__ rois, const int32_t* __restrict__ assoc, int G, float fH,
                                 float fW, float fD, float* __restrict__ matched) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    float b[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int a = assoc[g];
    if (a >= 0) re_pixel_box(rois + (size_t)a * 6, fH, fW, fD, b);
    for (int k = 0; k < 6; ++k) matched[(size_t)g * 6 + k] = b[k];
}

}  // namespace m3d

using namespace m3d;

extern "C" int m3d_rpn_eval_proposals(const float* rois, int64_t R, const float* gt, int64_t G, int64_t H, int64_t W,
                                      int64_t D, int64_t topk, double match_thr, const float* grid, int64_t T,
                                      int32_t* assoc, float* matched, int32_t* first_hit, int32_t* counts, float* iou,
                                      m3d_stream_t s) {
    if (H <= 0 || W <= 0 || D <= 0) return einval("rpn_eval_proposals: H, W and D must be positive");
    if (R < 0) return einval("rpn_eval_proposals: R must not be negative");
    if (topk < 0) return einval("rpn_eval_proposals: topk must not be negative");
    if (G < 1 || G > RE_MAX_G) return einval("rpn_eval_proposals: G must be in [1, 512]");
    if (T < 0 || T > RE_MAX_T) return einval("rpn_eval_proposals: T must be in [0, 8]");
    if (R > 0x7FFFFFFF / G) return einval("rpn_eval_proposals: R * G must fit 31 bits");
    if (gt == nullptr || assoc == nullptr || matched == nullptr || counts == nullptr)
        return einval("rpn_eval_proposals: NULL pointer");
    if (R > 0 && rois == nullptr) return einval("rpn_eval_proposals: rois must not be NULL when R > 0");
    if (T > 0 && (grid == nullptr || first_hit == nullptr))
        return einval("rpn_eval_proposals: grid and first_hit must not be NULL when T > 0");
    const int g = (int)G, tg = (int)(T * G);
    const float fH = (float)H, fW = (float)W, fD = (float)D;
    hipLaunchKernelGGL(re_init_kernel, dim3(grid_for(tg > g ? tg : g, 256)), dim3(256), 0, st(s), assoc, first_hit,
                       counts, g, tg);
    if (int rc = check_launch("re_init_kernel")) return rc;
    hipLaunchKernelGGL(re_score_kernel, dim3(grid_for(R, RE_CHUNK)), dim3(RE_CHUNK), 0, st(s), rois, gt, (int)R, g, fH,
                       fW, fD, (int)(topk < R ? topk : R), match_thr, grid, (int)T,
                       reinterpret_cast<unsigned*>(assoc), first_hit, counts, iou);
    if (int rc = check_launch("re_score_kernel")) return rc;
    hipLaunchKernelGGL(re_finish_kernel, dim3(grid_for(G, 256)), dim3(256), 0, st(s), rois, assoc, g, fH, fW, fD,
                       matched);
    return check_launch("re_finish_kernel");
}
