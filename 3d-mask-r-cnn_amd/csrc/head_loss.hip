// The three Mask R-CNN head losses of core/models.py on gfx950, values and
// gradients w.r.t. the head outputs:
//   mrcnn_class_loss_graph (core/models.py:1676-1807): logits clipped to
//     [-10, 10], focal softmax CE (1 - p_t)^gamma * CE with p_t clipped to
//     [eps, 1 - eps], alpha / (1 - alpha) for foreground / background rows, x2
//     for a background row whose best foreground probability passes 0.5, masked
//     by the image's active classes, divided by max(sum of the weights, eps);
//   mrcnn_bbox_loss_graph (core/models.py:1810-1877): positives only, the
//     target class's deltas soft-clipped by 3 tanh(x / 3), Huber (threshold 1),
//     mean over the 6 P values;
//   mrcnn_mask_loss_graph (core/models.py:1881-1960): positives whose target
//     mask is not empty, the target class's channel clipped to [eps, 1 - eps],
//     0.3 * mean BCE + 0.7 * (1 - mean Dice).
// R = B * T rows; row r belongs to image r / T.
//   K1 hl_rows_kernel       one lane per row: class numerator / weight, Huber sum
//   K2 hl_mask_sums_kernel  the one pass over mask pred + target: per row
//                           sum y, sum q, sum y q, sum bce as `split` ordered
//                           partials (several workgroups per row); rows that
//                           are not positive are not read
//   K3 hl_final_kernel      one workgroup: every sum in a fixed order -> the
//                           three losses, the weighted total, and the state:
//                           gradient scales + per-row mask coefficients
//   backward: hl_rows_bwd_kernel (d / d logits, d / d bbox, written whole) and
//             hl_mask_bwd_kernel (d / d mask, written whole, zeros included --
//             no memset needed), both scaled by the upstream scalar read
//             through a device pointer.
// fp32 terms, fixed-order sums (no atomics): run-to-run bit-identical.  Nothing
// allocates or synchronises; every launch is ordered on the caller's stream.
// The mask pass is HBM-bound: forward 4 R V (C + 1) bytes, backward the same
// read plus 4 R V C written (less: only positive rows are read).
#include <math.h>

#include "common.h"

namespace m3d {

constexpr int HL_BLOCK = 256;
constexpr int HL_VOX_PER_BLOCK = 2048;   // mask voxels per workgroup (8 per lane)
constexpr int HL_MAX_SPLIT = 64;         // workgroups per row at most
constexpr float HL_EPS = 1e-7f;          // K.epsilon()
constexpr float HL_HI = 1.0f - 1e-7f;
constexpr int64_t HL_MAX_V = 0x7FFFFFFF;
constexpr int64_t HL_MAX_R = 0x7FFFFFFF / HL_MAX_SPLIT;

static int hl_split(int64_t V) {
    int64_t n = (V + HL_VOX_PER_BLOCK - 1) / HL_VOX_PER_BLOCK;
    return (int)(n < 1 ? 1 : (n > HL_MAX_SPLIT ? HL_MAX_SPLIT : n));
}

__device__ __forceinline__ float hl_clamp(float v, float lo, float hi) { return smin(smax(v, lo), hi); }

// One row of the class loss.  num = focal * fp * w * a, wa = w * a; GRAD: g[k] =
// gs * d num / d logits[k] (fp, w, a constant).
template <bool GRAD>
__device__ __forceinline__ void hl_class_row(const float* __restrict__ x, int C, int t, float act, float alpha,
                                             float gamma, float& num, float& wa, float gs, float* __restrict__ g) {
    float mx = -INFINITY, mfg = -INFINITY;
    for (int k = 0; k < C; ++k) {
        const float z = hl_clamp(x[k], -10.0f, 10.0f);
        mx = smax(mx, z);
        if (k >= 1) mfg = smax(mfg, z);
    }
    float s = 0.0f, so = 0.0f;                                  // sum of exp; the same without the target class
    for (int k = 0; k < C; ++k) {
        const float e = expf(hl_clamp(x[k], -10.0f, 10.0f) - mx);
        s += e;
        if (k != t) so += e;
    }
    const float zt = hl_clamp(x[t], -10.0f, 10.0f);
    const float pt = expf(zt - mx) / s;
    const float qr = so / s;                                    // 1 - p_t without the cancellation
    const bool pass = pt >= HL_EPS && pt <= HL_HI;              // the p_t clip passes gradient inside only
    const float q = pass ? qr : (pt < HL_EPS ? 1.0f - HL_EPS : 1.0f - HL_HI);
    const float ce = logf(s) - (zt - mx);                       // sparse softmax CE
    const float fw = powf(q, gamma);
    const float w = t > 0 ? alpha : 1.0f - alpha;
    const float fp = (t == 0 && expf(mfg - mx) / s > 0.5f) ? 2.0f : 1.0f;   // confident false positive
    wa = w * act;
    num = fw * ce * fp * wa;
    if (GRAD) {
        // d/dz_k [q^g ce] = (p_k - [k == t]) (q^g + g q^(g-1) p_t ce [pass])
        const float b = fp * wa * (fw + (pass ? gamma * powf(q, gamma - 1.0f) * pt * ce : 0.0f));
        for (int k = 0; k < C; ++k) {
            const float xk = x[k];
            const float d = k == t ? -qr : expf(hl_clamp(xk, -10.0f, 10.0f) - mx) / s;
            // clip_by_value passes the gradient on [-10, 10] (ends included)
            g[k] = (xk >= -10.0f && xk <= 10.0f) ? gs * (b * d) : 0.0f;
        }
    }
}

// One positive row of the bbox loss: Huber sum over the 6 coordinates; GRAD:
// gb[c] = gs * d sum / d pred[c].
template <bool GRAD>
__device__ __forceinline__ float hl_bbox_row(const float* __restrict__ p, const float* __restrict__ tg, float gs,
                                             float* gb) {
    float h = 0.0f;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const float u = p[c] / 3.0f;
        const float y = 3.0f * tanhf(u);
        const float diff = tg[c] - y;
        const float d = fabsf(diff);
        h += d <= 1.0f ? 0.5f * (d * d) : d - 0.5f;
        if (GRAD) {
            const float sg = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
            const float e = expf(-2.0f * fabsf(u));             // 1 - tanh^2 = 4 e / (1 + e)^2, no cancellation
            const float sech2 = 4.0f * e / ((1.0f + e) * (1.0f + e));
            gb[c] = gs * (-(sg * smin(d, 1.0f)) * sech2);
        }
    }
    return h;
}

// active_class_ids row of loss row r.  The reference tiles the [B,C] table as
// tf.tile(active, [T,1]) and gathers row r of the result, so row r reads the
// active row r mod B, not its own image's r / T (core/models.py:1702-1705).
// Reproduced as is.  Background (t == 0) is always active.
__device__ __forceinline__ float hl_active(const float* __restrict__ active, int64_t r, int64_t B, int C, int t) {
    if (t == 0 || active == nullptr) return 1.0f;
    return active[(r % B) * C + t];
}

__device__ __forceinline__ int hl_class_index(int t, int C) { return t < 0 ? 0 : (t >= C ? C - 1 : t); }

// rows[r] = {class numerator, class weight, Huber sum, 0}
__global__ __launch_bounds__(HL_BLOCK) void hl_rows_kernel(
        const float* __restrict__ logits, const float* __restrict__ bbox, const int32_t* __restrict__ ids,
        const float* __restrict__ tbox, const float* __restrict__ active, int64_t R, int64_t B, int C,
        float alpha, float gamma, float4* __restrict__ rows) {
    const int64_t r = (int64_t)blockIdx.x * HL_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int t = hl_class_index(ids[r], C);
    float num = 0.0f, wa = 0.0f, h = 0.0f;
    if (logits != nullptr)
        hl_class_row<false>(logits + r * C, C, t, hl_active(active, r, B, C, t), alpha, gamma, num, wa, 0.0f,
                            nullptr);
    if (bbox != nullptr && t > 0) h = hl_bbox_row<false>(bbox + (r * C + t) * 6, tbox + r * 6, 0.0f, nullptr);
    rows[r] = make_float4(num, wa, h, 0.0f);
}

__device__ __forceinline__ void hl_mask_acc(float p, float y, float& sy, float& sq, float& si, float& sb) {
    const float q = hl_clamp(p, HL_EPS, HL_HI);
    sy += y;
    sq += q;
    si += y * q;
    // K.binary_crossentropy on probabilities (TF 2.2): its own clip is the identity on q
    sb -= y * logf(q + HL_EPS) + (1.0f - y) * logf(1.0f - q + HL_EPS);
}

__device__ __forceinline__ float hl_sel4(const float4& v, int t) {
    return t == 0 ? v.x : (t == 1 ? v.y : (t == 2 ? v.z : v.w));
}

// Unit range of workgroup b of a row: n units in `split` equal chunks.
__device__ __forceinline__ void hl_chunk(int64_t n, int split, int b, int64_t& lo, int64_t& hi) {
    const int64_t chunk = (n + split - 1) / split;
    lo = chunk * b;
    hi = lo + chunk;
    if (lo > n) lo = n;
    if (hi > n) hi = n;
}

// MODE 2 / 4: C == MODE, every lane loads contiguous 16-byte vectors of pred
// (two voxels x 2 channels / one voxel x 4 channels) and selects the target
// class's channel in registers; the row base must be 16-byte aligned (the host
// checks).  MODE 0: any C, a stride-C scalar gather.
template <int MODE>
__global__ __launch_bounds__(HL_BLOCK) void hl_mask_sums_kernel(
        const float* __restrict__ pred, const float* __restrict__ tgt, const int32_t* __restrict__ ids,
        int64_t V, int C, int split, float4* __restrict__ part) {
    const int64_t r = blockIdx.x / (unsigned)split;
    const int b = (int)(blockIdx.x % (unsigned)split);
    float sy = 0.0f, sq = 0.0f, si = 0.0f, sb = 0.0f;
    const int t = hl_class_index(ids[r], C);
    if (t > 0) {                                                // uniform over the workgroup
        const float* __restrict__ p = pred + r * V * C;
        const float* __restrict__ y = tgt + r * V;
        int64_t lo, hi;
        hl_chunk(MODE == 2 ? V / 2 : V, split, b, lo, hi);
        if (MODE == 2) {
            const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
            const float2* __restrict__ y2 = reinterpret_cast<const float2*>(y);
#pragma unroll 4
            for (int64_t i = lo + threadIdx.x; i < hi; i += HL_BLOCK) {
                const float4 v = p4[i];
                const float2 yy = y2[i];
                hl_mask_acc(t ? v.y : v.x, yy.x, sy, sq, si, sb);
                hl_mask_acc(t ? v.w : v.z, yy.y, sy, sq, si, sb);
            }
        } else if (MODE == 4) {
            const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
#pragma unroll 4
            for (int64_t i = lo + threadIdx.x; i < hi; i += HL_BLOCK)
                hl_mask_acc(hl_sel4(p4[i], t), y[i], sy, sq, si, sb);
        } else {
#pragma unroll 4
            for (int64_t i = lo + threadIdx.x; i < hi; i += HL_BLOCK)
                hl_mask_acc(p[i * C + t], y[i], sy, sq, si, sb);
        }
    }
    // fixed-order workgroup reduction: wave butterflies, then the 4 waves in order
    for (int o = 32; o > 0; o >>= 1) {
        sy += __shfl_xor(sy, o);
        sq += __shfl_xor(sq, o);
        si += __shfl_xor(si, o);
        sb += __shfl_xor(sb, o);
    }
    __shared__ float4 wp[HL_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wp[wave] = make_float4(sy, sq, si, sb);
    __syncthreads();
    if (threadIdx.x == 0) {
        float4 a = wp[0];
        for (int w = 1; w < HL_BLOCK / 64; ++w) {
            a.x += wp[w].x; a.y += wp[w].y; a.z += wp[w].z; a.w += wp[w].w;
        }
        part[blockIdx.x] = a;
    }
}

struct HLMaskRow { double sy, sq, si, sb; };

__device__ __forceinline__ HLMaskRow hl_mask_row(const float4* __restrict__ part, int64_t r, int split) {
    HLMaskRow m = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < split; ++b) {
        const float4 a = part[r * split + b];
        m.sy += a.x; m.sq += a.y; m.si += a.z; m.sb += a.w;
    }
    return m;
}

constexpr int HL_NSUM = 7;   // class num, class weight, Huber, positives, bce, dice, valid rows

// state[0..3] = {w_cls / den, w_box / (6 P), w_mask 0.3 / (Pv V), Pv};
// state[4 + 4 r ..] = {kb, ky, k0, valid} of row r: d total / d q_v =
// kb (-(y / (q + eps)) + (1 - y) / (1 - q + eps)) + ky y + k0 on valid rows.
__global__ __launch_bounds__(1024) void hl_final_kernel(
        const float4* __restrict__ rows, const float4* __restrict__ part, const int32_t* __restrict__ ids,
        int64_t R, int64_t V, int C, int split, int has_cls, int has_box, int has_mask, float w_cls, float w_box,
        float w_mask, float* __restrict__ total, float* __restrict__ cls_loss, float* __restrict__ box_loss,
        float* __restrict__ mask_loss, float* __restrict__ state) {
    __shared__ double sw[HL_NSUM][1024 / 64];
    __shared__ double tot[HL_NSUM];
    const int t = threadIdx.x;
    double a[HL_NSUM] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t r = t; r < R; r += 1024) {
        const float4 v = rows[r];
        a[0] += v.x; a[1] += v.y; a[2] += v.z;
        if (hl_class_index(ids[r], C) > 0) {
            a[3] += 1.0;
            if (has_mask) {
                const HLMaskRow m = hl_mask_row(part, r, split);
                if (m.sy > 0.0) {                               // rows with an empty target mask are dropped
                    a[4] += m.sb;
                    a[5] += (2.0 * m.si + 1.0) / (m.sy + m.sq + 1.0);
                    a[6] += 1.0;
                }
            }
        }
    }
    // fixed order: wave butterflies, the 16 waves in order
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < HL_NSUM; ++i) a[i] += __shfl_xor(a[i], o);
    if ((t & 63) == 0)
#pragma unroll
        for (int i = 0; i < HL_NSUM; ++i) sw[i][t >> 6] = a[i];
    __syncthreads();
    if (t < HL_NSUM) {
        double s = sw[t][0];
        for (int w = 1; w < 1024 / 64; ++w) s += sw[t][w];
        tot[t] = s;
    }
    __syncthreads();
    const double P = tot[3], Pv = tot[6];
    if (t == 0) {
        const double den = tot[1] > (double)HL_EPS ? tot[1] : (double)HL_EPS;
        const float lc = has_cls ? (float)(tot[0] / den) : 0.0f;
        const float lb = (has_box && P > 0.0) ? (float)(tot[2] / (6.0 * P)) : 0.0f;
        const float lm = (has_mask && Pv > 0.0)
                             ? (float)(0.3 * (tot[4] / (Pv * (double)V)) + 0.7 * (1.0 - tot[5] / Pv)) : 0.0f;
        *total = lc * w_cls + lb * w_box + lm * w_mask;
        *cls_loss = lc;
        *box_loss = lb;
        *mask_loss = lm;
        state[0] = has_cls ? (float)(w_cls / den) : 0.0f;
        state[1] = (has_box && P > 0.0) ? (float)(w_box / (6.0 * P)) : 0.0f;
        state[2] = (has_mask && Pv > 0.0) ? (float)(w_mask * 0.3 / (Pv * (double)V)) : 0.0f;
        state[3] = (float)Pv;
    }
    float4* __restrict__ coef = reinterpret_cast<float4*>(state) + 1;
    for (int64_t r = t; r < R; r += 1024) {
        float4 k = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (has_mask && hl_class_index(ids[r], C) > 0) {
            const HLMaskRow m = hl_mask_row(part, r, split);
            if (m.sy > 0.0) {
                const double u1 = m.sy + m.sq + 1.0;
                k.x = (float)(w_mask * 0.3 / (Pv * (double)V));
                k.y = (float)(-w_mask * 0.7 / Pv * 2.0 / u1);
                k.z = (float)(w_mask * 0.7 / Pv * (2.0 * m.si + 1.0) / (u1 * u1));
                k.w = 1.0f;
            }
        }
        coef[r] = k;
    }
}

__global__ __launch_bounds__(HL_BLOCK) void hl_rows_bwd_kernel(
        const float* __restrict__ logits, const float* __restrict__ bbox, const int32_t* __restrict__ ids,
        const float* __restrict__ tbox, const float* __restrict__ active, int64_t R, int64_t B, int C,
        float alpha, float gamma, const float* __restrict__ state, const float* __restrict__ g_total,
        float* __restrict__ g_logits, float* __restrict__ g_bbox) {
    const int64_t r = (int64_t)blockIdx.x * HL_BLOCK + threadIdx.x;
    if (r >= R) return;
    const int t = hl_class_index(ids[r], C);
    const float g = *g_total;
    if (g_logits != nullptr) {
        float num, wa;
        hl_class_row<true>(logits + r * C, C, t, hl_active(active, r, B, C, t), alpha, gamma, num, wa,
                           g * state[0], g_logits + r * C);
    }
    if (g_bbox != nullptr) {
        float gb[6] = {0, 0, 0, 0, 0, 0};
        if (t > 0) hl_bbox_row<true>(bbox + (r * C + t) * 6, tbox + r * 6, g * state[1], gb);
        for (int k = 0; k < C; ++k)
#pragma unroll
            for (int c = 0; c < 6; ++c) g_bbox[(r * C + k) * 6 + c] = (k == t && t > 0) ? gb[c] : 0.0f;
    }
}

__device__ __forceinline__ float hl_mask_grad(float p, float y, const float4& k, float g) {
    if (!(p >= HL_EPS && p <= HL_HI)) return 0.0f;              // K.clip passes the gradient inside only
    return g * (k.x * (-(y / (p + HL_EPS)) + (1.0f - y) / (1.0f - p + HL_EPS)) + k.y * y + k.z);
}

// The whole mask gradient [R,V,C], zeros included; same modes and chunks as
// hl_mask_sums_kernel.
template <int MODE>
__global__ __launch_bounds__(HL_BLOCK) void hl_mask_bwd_kernel(
        const float* __restrict__ pred, const float* __restrict__ tgt, const int32_t* __restrict__ ids,
        int64_t V, int C, int split, const float* __restrict__ state, const float* __restrict__ g_total,
        float* __restrict__ g_mask) {
    const int64_t r = blockIdx.x / (unsigned)split;
    const int b = (int)(blockIdx.x % (unsigned)split);
    const int t = hl_class_index(ids[r], C);
    const float4 k = reinterpret_cast<const float4*>(state)[1 + r];
    const bool live = t > 0 && k.w != 0.0f;                     // uniform over the workgroup
    const float g = *g_total;
    const float* __restrict__ p = pred + r * V * C;
    const float* __restrict__ y = tgt + r * V;
    float* __restrict__ o = g_mask + r * V * C;
    int64_t lo, hi;
    hl_chunk(MODE == 2 ? V / 2 : V, split, b, lo, hi);
    if (MODE == 2 || MODE == 4) {
        float4* __restrict__ o4 = reinterpret_cast<float4*>(o);
        if (!live) {
            for (int64_t i = lo + threadIdx.x; i < hi; i += HL_BLOCK) o4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            return;
        }
        const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
        if (MODE == 2) {
            const float2* __restrict__ y2 = reinterpret_cast<const float2*>(y);
#pragma unroll 4
            for (int64_t i = lo + threadIdx.x; i < hi; i += HL_BLOCK) {
                const float4 v = p4[i];
                const float2 yy = y2[i];
                const float ga = hl_mask_grad(t ? v.y : v.x, yy.x, k, g);
                const float gb = hl_mask_grad(t ? v.w : v.z, yy.y, k, g);
                o4[i] = t ? make_float4(0.0f, ga, 0.0f, gb) : make_float4(ga, 0.0f, gb, 0.0f);
            }
        } else {
#pragma unroll 4
            for (int64_t i = lo + threadIdx.x; i < hi; i += HL_BLOCK) {
                const float gv = hl_mask_grad(hl_sel4(p4[i], t), y[i], k, g);
                o4[i] = make_float4(t == 0 ? gv : 0.0f, t == 1 ? gv : 0.0f, t == 2 ? gv : 0.0f,
                                    t == 3 ? gv : 0.0f);
            }
        }
    } else {
        // flat elements [lo C, hi C): consecutive lanes write consecutive floats
        for (int64_t e = lo * C + threadIdx.x; e < hi * C; e += HL_BLOCK) {
            const int64_t v = e / C;
            const int c = (int)(e - v * C);
            o[e] = (live && c == t) ? hl_mask_grad(p[e], y[v], k, g) : 0.0f;
        }
    }
}

// 2 / 4: the 16-byte vector kernels apply (C, row stride and base alignment); else 0
static int hl_mask_mode(const void* pred, const void* tgt, const void* out, int64_t V, int64_t C) {
    const uintptr_t a = (uintptr_t)pred | (uintptr_t)out;
    if ((a & 15) != 0) return 0;
    if (C == 4 && ((uintptr_t)tgt & 3) == 0) return 4;
    if (C == 2 && V % 2 == 0 && ((uintptr_t)tgt & 7) == 0) return 2;
    return 0;
}

static int hl_check(int64_t B, int64_t T, int64_t C, int64_t V, float gamma) {
    if (B < 0 || T < 0 || V < 0) return einval("head_loss: negative size");
    if (C < 2) return einval("head_loss: C must be >= 2");
    if (C > 0x7FFFFFFF) return einval("head_loss: too many classes");
    if (!(gamma >= 1.0f)) return einval("head_loss: gamma must be >= 1");
    if (T > 0 && B > HL_MAX_R / T) return einval("head_loss: too many rows");
    if (V > HL_MAX_V) return einval("head_loss: mask volume too large");
    return M3D_OK;
}

}  // namespace m3d

using namespace m3d;

extern "C" size_t m3d_head_loss_workspace_bytes(int64_t R, int64_t V) {
    if (R < 0 || V < 0 || R > HL_MAX_R || V > HL_MAX_V) return 0;
    return sizeof(float4) * (size_t)(R * (1 + hl_split(V)) + 1);
}

extern "C" int m3d_head_loss_fwd(const float* class_logits, const float* bbox_pred, const float* mask_pred,
                                 const int32_t* target_class_ids, const float* target_bbox,
                                 const float* target_mask, const float* active_class_ids, int64_t B, int64_t T,
                                 int64_t C, int64_t V, float alpha, float gamma, float w_cls, float w_box,
                                 float w_mask, float* total, float* cls_loss, float* box_loss, float* mask_loss,
                                 float* state, void* workspace, size_t ws_bytes, m3d_stream_t s) {
    if (int rc = hl_check(B, T, C, V, gamma)) return rc;
    const int64_t R = B * T;
    if (workspace == nullptr || ws_bytes < m3d_head_loss_workspace_bytes(R, V))
        return einval("head_loss: workspace too small");
    if (((uintptr_t)workspace & 15) != 0 || ((uintptr_t)state & 15) != 0)
        return einval("head_loss: workspace and state must be 16-byte aligned");
    if (target_class_ids == nullptr || total == nullptr || cls_loss == nullptr || box_loss == nullptr ||
        mask_loss == nullptr || state == nullptr)
        return einval("head_loss: target_class_ids, the loss scalars and state must not be NULL");
    if (bbox_pred != nullptr && target_bbox == nullptr) return einval("head_loss: bbox_pred without target_bbox");
    if (mask_pred != nullptr && target_mask == nullptr) return einval("head_loss: mask_pred without target_mask");
    const int split = hl_split(V);
    float4* rows = (float4*)workspace;
    float4* part = rows + R;
    const bool has_mask = mask_pred != nullptr && V > 0;
    if (R > 0) {
        hipLaunchKernelGGL(hl_rows_kernel, dim3(grid_for(R, HL_BLOCK)), dim3(HL_BLOCK), 0, st(s), class_logits,
                           bbox_pred, target_class_ids, target_bbox, active_class_ids, R, B, (int)C, alpha, gamma,
                           rows);
        if (int rc = check_launch("hl_rows_kernel")) return rc;
    }
    if (R > 0 && has_mask) {
        const dim3 grid((unsigned)(R * split));
        const int mode = hl_mask_mode(mask_pred, target_mask, nullptr, V, C);
        if (mode == 2)
            hipLaunchKernelGGL(hl_mask_sums_kernel<2>, grid, dim3(HL_BLOCK), 0, st(s), mask_pred, target_mask,
                               target_class_ids, V, (int)C, split, part);
        else if (mode == 4)
            hipLaunchKernelGGL(hl_mask_sums_kernel<4>, grid, dim3(HL_BLOCK), 0, st(s), mask_pred, target_mask,
                               target_class_ids, V, (int)C, split, part);
        else
            hipLaunchKernelGGL(hl_mask_sums_kernel<0>, grid, dim3(HL_BLOCK), 0, st(s), mask_pred, target_mask,
                               target_class_ids, V, (int)C, split, part);
        if (int rc = check_launch("hl_mask_sums_kernel")) return rc;
    }
    hipLaunchKernelGGL(hl_final_kernel, dim3(1), dim3(1024), 0, st(s), rows, part, target_class_ids, R, V, (int)C,
                       split, class_logits != nullptr ? 1 : 0, bbox_pred != nullptr ? 1 : 0, has_mask ? 1 : 0,
                       w_cls, w_box, w_mask, total, cls_loss, box_loss, mask_loss, state);
    return check_launch("hl_final_kernel");
}

extern "C" int m3d_head_loss_bwd(const float* class_logits, const float* bbox_pred, const float* mask_pred,
                                 const int32_t* target_class_ids, const float* target_bbox,
                                 const float* target_mask, const float* active_class_ids, int64_t B, int64_t T,
                                 int64_t C, int64_t V, float alpha, float gamma, const float* state,
                                 const float* g_total, float* g_logits, float* g_bbox, float* g_mask,
                                 m3d_stream_t s) {
    if (int rc = hl_check(B, T, C, V, gamma)) return rc;
    const int64_t R = B * T;
    if (target_class_ids == nullptr || state == nullptr || g_total == nullptr)
        return einval("head_loss: target_class_ids, state and g_total must not be NULL");
    if (((uintptr_t)state & 15) != 0) return einval("head_loss: workspace and state must be 16-byte aligned");
    if ((g_logits != nullptr && class_logits == nullptr) ||
        (g_bbox != nullptr && (bbox_pred == nullptr || target_bbox == nullptr)) ||
        (g_mask != nullptr && (mask_pred == nullptr || target_mask == nullptr)))
        return einval("head_loss: a gradient was asked for a branch whose inputs are NULL");
    if (R == 0) return M3D_OK;
    if (g_logits != nullptr || g_bbox != nullptr) {
        hipLaunchKernelGGL(hl_rows_bwd_kernel, dim3(grid_for(R, HL_BLOCK)), dim3(HL_BLOCK), 0, st(s), class_logits,
                           bbox_pred, target_class_ids, target_bbox, active_class_ids, R, B, (int)C, alpha, gamma,
                           state, g_total, g_logits, g_bbox);
        if (int rc = check_launch("hl_rows_bwd_kernel")) return rc;
    }
    if (g_mask != nullptr && V > 0) {
        const int split = hl_split(V);
        const dim3 grid((unsigned)(R * split));
        const int mode = hl_mask_mode(mask_pred, target_mask, g_mask, V, C);
        if (mode == 2)
            hipLaunchKernelGGL(hl_mask_bwd_kernel<2>, grid, dim3(HL_BLOCK), 0, st(s), mask_pred, target_mask,
                               target_class_ids, V, (int)C, split, state, g_total, g_mask);
        else if (mode == 4)
            hipLaunchKernelGGL(hl_mask_bwd_kernel<4>, grid, dim3(HL_BLOCK), 0, st(s), mask_pred, target_mask,
                               target_class_ids, V, (int)C, split, state, g_total, g_mask);
        else
            hipLaunchKernelGGL(hl_mask_bwd_kernel<0>, grid, dim3(HL_BLOCK), 0, st(s), mask_pred, target_mask,
                               target_class_ids, V, (int)C, split, state, g_total, g_mask);
        return check_launch("hl_mask_bwd_kernel");
    }
    return M3D_OK;
}
