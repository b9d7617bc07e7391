// Detection unmolding and mask-IoU evaluation on gfx950: unmold_detections /
// unmold_small_3d_mask (core/models.py:7198-7419) and compute_overlaps_masks
// (core/utils.py:312-334) without the reference's full-size [H,W,D,N] masks.
// A predicted mask is non-zero only inside its box and its value at a voxel is
// a function of the detection's m^3 grid, so one pass over each box's voxels,
// reading the G contiguous ground-truth bytes of every set voxel, gives the
// reference's intersection counts as integers.
//   K1 um_prepare_kernel   one workgroup per detection: box + keep filter, the
//                          grid's channel sorted in LDS (bitonic), min / max /
//                          mean / std / percentiles, the threshold branch (0.5,
//                          percentile of the active values, Otsu), binarise,
//                          face-connected components by min-label propagation
//                          in LDS, small components dropped -> small, box_i,
//                          status, stats
//   K2 um_overlaps_kernel  grid (detection, slab): the binary grid staged in
//                          LDS, the trilinear resize evaluated per box voxel in
//                          fp64, set voxels counted, their GT bytes read with
//                          lanes laid out (voxel, 4-byte group); per-lane
//                          counts -> LDS -> one integer atomic per (n, g)
//   K3 um_finalize_kernel  the after-resize rejection (SPARSE), rejected rows
//                          zeroed, IoU = inter / (area_pred + area_gt - inter)
//   K4 um_paste_kernel     the same traversal writing 1 into dense / seg_union
//   K5 um_areas_kernel     column counts of the [V,G] GT bytes
//   K6 um_label_of_kernel  numbers the listed rows (one workgroup, a scan);
//      um_labels_kernel    K4's traversal, a 32-bit atomic max of the row's
//                          label per set voxel -> the instance label volume
//   K7 um_pixelwise_kernel one streaming pass over labels + GT bytes -> tp /
//                          fp / fn of "any instance" against "any GT mask"
//   K8 um_stack_kernel     labels [H,W,D] int32 -> the TIFF page order [D,H,W]
//                          uint8 / uint16, a tiled transpose through LDS
// All scalar arithmetic is fp64 on the fp32 inputs in the order of
// tests/unmoldref.py (no contraction: the Makefile's -ffp-contract=off), so the
// thresholds and every integer output equal that restatement bit for bit.  The
// sums are integers (order-independent): run-to-run bit-identical.  Nothing
// allocates or synchronises; every launch is ordered on the caller's stream.
#include <math.h>

#include "common.h"

namespace m3d {

constexpr int UM_PREP_BLOCK = 1024;
constexpr int UM_MAX_N = 32768;          // m^3 at most: 128 KiB of sort keys in LDS
// UM_BLOCK, UM_SLAB_VOX and UM_MAX_SLABS fix how many workgroups stage a grid:
// scripts/time_unmold.py restates them for the algorithmic-byte count (keep in step).
constexpr int UM_BLOCK = 256;
constexpr int UM_SLAB_VOX = 2048;        // volume voxels per slab of the (detection, slab) grid ...
constexpr int UM_MAX_SLABS = 64;         // ... up to this many slabs per detection
constexpr int UM_GPASS = 4 * UM_BLOCK;   // GT bytes of a voxel taken per pass (4 per lane)
constexpr unsigned UM_NONE = 0xFFFFu;    // label of an unset voxel

__device__ __forceinline__ uint32_t um_key(float v) {          // unsigned order = float order
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ double um_val(uint32_t k) {
    return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ double um_clip(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// Fixed tree: wave butterfly, then the 16 waves in order; every thread gets the sum.
__device__ __forceinline__ double um_block_sum(double v, double* sc) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sc[0];
    for (int w = 1; w < UM_PREP_BLOCK / 64; ++w) s += sc[w];
    return s;
}
__device__ __forceinline__ int um_block_sum_i(int v, int* sc) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = sc[0];
    for (int w = 1; w < UM_PREP_BLOCK / 64; ++w) s += sc[w];
    return s;
}

// percentile(q) of the sorted keys s[off .. off + L)
__device__ __forceinline__ double um_pct(const uint32_t* s, int off, int L, double q) {
    const double h = (double)(L - 1) * (q / 100.0);
    const double fi = floor(h);
    const int i = (int)fi;
    const double g = h - fi;
    const int i1 = i + 1 < L - 1 ? i + 1 : L - 1;
    const double a = um_val(s[off + i]);
    return a + (um_val(s[off + i1]) - a) * g;
}

__device__ __forceinline__ void um_reject(uint8_t* __restrict__ sm, int n, int32_t* __restrict__ box_i,
                                          int32_t* __restrict__ status, double* __restrict__ stats, int64_t nd,
                                          int code, const int* bx, const double* st) {
    for (int i = threadIdx.x; i < n; i += UM_PREP_BLOCK) sm[i] = 0;
    if (threadIdx.x == 0) {
        status[nd] = code;
        for (int k = 0; k < 6; ++k) box_i[nd * 6 + k] = bx[k];
        for (int k = 0; k < 8; ++k) stats[nd * 8 + k] = st[k];
    }
}

__global__ __launch_bounds__(UM_PREP_BLOCK) void um_prepare_kernel(
        const float* __restrict__ det, const float* __restrict__ mask, int m, int C, int H, int W, int D,
        int min_size, uint8_t* __restrict__ small, int32_t* __restrict__ box_i, int32_t* __restrict__ status,
        double* __restrict__ stats) {
    __shared__ uint32_t buf[UM_MAX_N];                          // sort keys, then labels + component sizes
    __shared__ double sc[UM_PREP_BLOCK / 64];
    __shared__ int sci[UM_PREP_BLOCK / 64];
    __shared__ int hist[256];
    __shared__ double m2[256];
    __shared__ double bc;
    __shared__ int flag;
    const int t = threadIdx.x;
    const int64_t nd = blockIdx.x;
    const int n = m * m * m;
    uint8_t* __restrict__ sm = small + nd * n;
    int bx[6] = {0, 0, 0, 0, 0, 0};
    double st[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // (a) box and keep filter
    const float* __restrict__ dr = det + nd * 8;
    const int dims[3] = {H, W, D};
    float b[6];
    for (int k = 0; k < 6; ++k) b[k] = dr[k] * (float)dims[k % 3];
    const float cf = dr[6];
    const int cid = (cf >= 1.0f && cf < 2.0e9f) ? (int)cf : 0;
    const bool keep = cid > 0 && (b[3] - b[0]) > 0.5f && (b[4] - b[1]) > 0.5f && (b[5] - b[2]) > 0.5f;
    if (!keep) {
        um_reject(sm, n, box_i, status, stats, nd, M3D_UNMOLD_NOT_KEPT, bx, st);
        return;
    }
    for (int a = 0; a < 3; ++a) {
        const double lo = fmin(fmax(floor((double)b[a]), 0.0), (double)dims[a] - 1.0);
        const double hi = fmin(fmax(ceil((double)b[a + 3]), lo + 1.0), (double)dims[a]);
        bx[a] = (int)lo;
        bx[a + 3] = (int)hi;
    }
    const int ch = C == 1 ? 0 : (cid < C - 1 ? cid : C - 1);
    const float* __restrict__ mp = mask + nd * n * C + ch;

    // (b) sort the channel in LDS (bitonic on the next power of two, padded with the largest key)
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = t; i < P; i += UM_PREP_BLOCK) buf[i] = i < n ? um_key(mp[(int64_t)i * C]) : 0xFFFFFFFFu;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P / 2; i += UM_PREP_BLOCK) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                const int hi = lo | j;
                const uint32_t x = buf[lo], y = buf[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    buf[lo] = y;
                    buf[hi] = x;
                }
            }
            __syncthreads();
        }
    double part = 0.0;
    for (int i = t; i < n; i += UM_PREP_BLOCK) part += um_val(buf[i]);
    const double mean = um_block_sum(part, sc) / (double)n;
    part = 0.0;
    for (int i = t; i < n; i += UM_PREP_BLOCK) {
        const double d = um_val(buf[i]) - mean;
        part += d * d;
    }
    const double sd = sqrt(um_block_sum(part, sc) / (double)n);
    const double lo = um_val(buf[0]), hi = um_val(buf[n - 1]);
    const double p50 = um_pct(buf, 0, n, 50.0), p95 = um_pct(buf, 0, n, 95.0);
    st[0] = lo; st[1] = hi; st[2] = mean; st[3] = sd; st[4] = p50; st[5] = p95;
    const int code = (lo < -0.1 || hi > 1.1) ? M3D_UNMOLD_RANGE
                     : (sd < 1e-6 ? M3D_UNMOLD_FLAT : (p95 < 0.10 ? M3D_UNMOLD_FAINT : M3D_UNMOLD_OK));
    if (code != M3D_UNMOLD_OK) {                                // uniform: every thread holds the same values
        um_reject(sm, n, box_i, status, stats, nd, code, bx, st);
        return;
    }

    // (c) threshold
    double thr;
    if (mean > 0.4) {
        thr = 0.5;
    } else if (mean < 0.1) {
        int a0 = 0, a1 = n;                                     // first sorted index whose value is > p50
        while (a0 < a1) {
            const int mid = (a0 + a1) >> 1;
            if (um_val(buf[mid]) > p50) a1 = mid; else a0 = mid + 1;
        }
        const int L = n - a0;
        thr = L > 10 ? um_clip(um_pct(buf, a0, L, 30.0), 0.15, 0.45) : 0.30;
    } else {
        if (t < 256) hist[t] = 0;
        __syncthreads();
        for (int i = t; i < n; i += UM_PREP_BLOCK) {
            const double f = floor(((um_val(buf[i]) - lo) / (hi - lo)) * 256.0);
            atomicAdd(&hist[f < 255.0 ? (int)f : 255], 1);
        }
        __syncthreads();
        if (t == 0) {                                           // the order-sensitive sums, in one lane
            const double bw = (hi - lo) / 256.0;
            double acc = 0.0;
            for (int k = 255; k >= 0; --k) {
                const double cc = (double)hist[k] * (lo + ((double)k + 0.5) * bw);
                acc = k == 255 ? cc : acc + cc;
                m2[k] = acc;
            }
            double w1 = 0.0, m1 = 0.0, best = -INFINITY;
            int kb = 0;
            for (int k = 0; k < 255; ++k) {
                const double c = (double)hist[k];
                const double cc = c * (lo + ((double)k + 0.5) * bw);
                w1 += c;
                m1 = k == 0 ? cc : m1 + cc;
                const double w2 = (double)n - w1;
                const double d = m1 / w1 - m2[k + 1] / w2;
                const double v = (w1 * w2) * (d * d);
                if (v > best) {                                 // NaN never wins; the first maximum stays
                    best = v;
                    kb = k;
                }
            }
            bc = um_clip(lo + ((double)kb + 0.5) * bw, 0.20, 0.6);
        }
        __syncthreads();
        thr = bc;
    }
    st[6] = thr;
    st[7] = mean < 0.15 ? 0.3 : 0.4;
    __syncthreads();                                            // the sorted keys are dead from here

    // binarise into 16-bit labels (the flat index, or UM_NONE) over the first half of buf
    volatile uint16_t* lab = reinterpret_cast<volatile uint16_t*>(buf);
    uint32_t* cnt = buf + UM_MAX_N / 2;                         // two 16-bit component sizes per word
    int mine = 0;
    for (int i = t; i < n; i += UM_PREP_BLOCK) {
        const bool set = (double)mp[(int64_t)i * C] >= thr;
        lab[i] = set ? (uint16_t)i : (uint16_t)UM_NONE;
        mine += set;
    }
    const int nset = um_block_sum_i(mine, sci);
    const double density = (double)nset / (double)n;
    if (density < 0.0001) {
        um_reject(sm, n, box_i, status, stats, nd, M3D_UNMOLD_EMPTY, bx, st);
        return;
    }

    // (d) cleaning: min-label propagation until a pass changes nothing.  Labels
    // only decrease and stay inside their component, so the racing in-place
    // updates end at the one fixed point: the component's smallest index.
    bool drop_small = false;
    if (density > 0.0001 && density < 0.95) {
        const int mm = m * m;
        for (;;) {
            __syncthreads();
            if (t == 0) flag = 0;
            __syncthreads();
            int changed = 0;
            for (int i = t; i < n; i += UM_PREP_BLOCK) {
                const unsigned cur = lab[i];
                if (cur == UM_NONE) continue;
                const int z = i % m, x = (i / m) % m, y = i / mm;
                unsigned best = cur, l;
                if (z > 0 && (l = lab[i - 1]) < best) best = l;
                if (z < m - 1 && (l = lab[i + 1]) < best) best = l;
                if (x > 0 && (l = lab[i - m]) < best) best = l;
                if (x < m - 1 && (l = lab[i + m]) < best) best = l;
                if (y > 0 && (l = lab[i - mm]) < best) best = l;
                if (y < m - 1 && (l = lab[i + mm]) < best) best = l;
                if ((l = lab[best]) < best) best = l;           // one pointer jump (a label is a set voxel)
                if (best < cur) {
                    lab[i] = (uint16_t)best;
                    changed = 1;
                }
            }
            if (changed) flag = 1;
            __syncthreads();
            if (flag == 0) break;
        }
        for (int i = t; i < (n + 1) / 2; i += UM_PREP_BLOCK) cnt[i] = 0;
        __syncthreads();
        mine = 0;
        for (int i = t; i < n; i += UM_PREP_BLOCK) {
            const unsigned r = lab[i];
            if (r == UM_NONE) continue;
            atomicAdd(&cnt[r >> 1], 1u << (16 * (r & 1)));      // a size is at most 32768: no carry
            mine += r == (unsigned)i;
        }
        drop_small = um_block_sum_i(mine, sci) > 1;             // (its barriers also order the counts)
    }
    for (int i = t; i < n; i += UM_PREP_BLOCK) {
        const unsigned r = lab[i];
        bool set = r != UM_NONE;
        if (set && drop_small) set = (int)((cnt[r >> 1] >> (16 * (r & 1))) & 0xFFFFu) >= min_size;
        sm[i] = set ? 1 : 0;
    }
    if (t == 0) {
        status[nd] = M3D_UNMOLD_OK;
        for (int k = 0; k < 6; ++k) box_i[nd * 6 + k] = bx[k];
        for (int k = 0; k < 8; ++k) stats[nd * 8 + k] = st[k];
    }
}

// ---- (e): the resized value at one box voxel ---------------------------------
__device__ __forceinline__ double um_tap(const uint8_t* sm, int m, int y, int x, int z) {
    if ((unsigned)y >= (unsigned)m || (unsigned)x >= (unsigned)m || (unsigned)z >= (unsigned)m) return 0.0;
    return (double)sm[(y * m + x) * m + z];
}

__device__ __forceinline__ bool um_set(const uint8_t* sm, int m, double ry, double rx, double rz, int oy, int ox,
                                       int oz, double rthr) {
    const double cy = ((double)oy + 0.5) * ry - 0.5, cx = ((double)ox + 0.5) * rx - 0.5,
                 cz = ((double)oz + 0.5) * rz - 0.5;
    const double fy = floor(cy), fx = floor(cx), fz = floor(cz);
    const int y0 = (int)fy, x0 = (int)fx, z0 = (int)fz;
    const double ty = cy - fy, tx = cx - fx, tz = cz - fz;
    double vx[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        double vz[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double v0 = um_tap(sm, m, y0 + a, x0 + c, z0), v1 = um_tap(sm, m, y0 + a, x0 + c, z0 + 1);
            vz[c] = v0 + (v1 - v0) * tz;
        }
        vx[a] = vz[0] + (vz[1] - vz[0]) * tx;
    }
    return vx[0] + (vx[1] - vx[0]) * ty >= rthr;
}

struct UmBox {
    int y1, x1, z1, hh, ww, dd, nvox;
    bool ok;
};

__device__ __forceinline__ UmBox um_box(const int32_t* __restrict__ box_i, int64_t nd, int H, int W, int D) {
    const int32_t* b = box_i + nd * 6;
    UmBox r = {};
    r.y1 = b[0]; r.x1 = b[1]; r.z1 = b[2];
    r.hh = b[3] - b[0]; r.ww = b[4] - b[1]; r.dd = b[5] - b[2];
    r.ok = b[0] >= 0 && b[1] >= 0 && b[2] >= 0 && r.hh > 0 && r.ww > 0 && r.dd > 0 && b[3] <= H && b[4] <= W &&
           b[5] <= D;                                           // never index outside the volume
    r.nvox = r.ok ? r.hh * r.ww * r.dd : 0;
    return r;
}

__device__ __forceinline__ void um_stage(uint8_t* sm, const uint8_t* __restrict__ src, int n) {
    if (((uintptr_t)src & 3) == 0) {
        const uint32_t* __restrict__ s4 = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d4 = reinterpret_cast<uint32_t*>(sm);
        for (int i = threadIdx.x; i < n / 4; i += UM_BLOCK) d4[i] = s4[i];
        for (int i = (n & ~3) + threadIdx.x; i < n; i += UM_BLOCK) sm[i] = src[i];
    } else {
        for (int i = threadIdx.x; i < n; i += UM_BLOCK) sm[i] = src[i];
    }
}

__global__ __launch_bounds__(UM_BLOCK) void um_overlaps_kernel(
        const uint8_t* __restrict__ small, const int32_t* __restrict__ box_i, const int32_t* __restrict__ status,
        const double* __restrict__ stats, int m, int H, int W, int D, const uint8_t* __restrict__ gt, int G,
        int slabs, int32_t* __restrict__ area_pred, int32_t* __restrict__ inter) {
    extern __shared__ __attribute__((aligned(16))) uint8_t um_sm[];   // the detection's m^3 binary grid
    __shared__ uint8_t flag[UM_BLOCK];
    __shared__ int vlin[UM_BLOCK];
    __shared__ int cnt[UM_GPASS];
    __shared__ int area;
    const int t = threadIdx.x;
    const int64_t nd = blockIdx.x / (unsigned)slabs;
    const int sl = (int)(blockIdx.x % (unsigned)slabs);
    if (status[nd] != M3D_UNMOLD_OK) return;                    // uniform over the workgroup
    const UmBox bx = um_box(box_i, nd, H, W, D);
    const int nchunks = (bx.nvox + UM_BLOCK - 1) / UM_BLOCK;
    if (sl >= nchunks) return;
    const int n = m * m * m;
    um_stage(um_sm, small + nd * n, n);
    if (t == 0) area = 0;
    const double ry = (double)m / (double)bx.hh, rx = (double)m / (double)bx.ww, rz = (double)m / (double)bx.dd;
    const double rthr = stats[nd * 8 + 7];
    int myarea = 0;
    for (int g0 = 0; g0 == 0 || g0 < G; g0 += UM_GPASS) {
        const int Gp = G - g0 < UM_GPASS ? G - g0 : UM_GPASS;   // 0 when G == 0: the area alone
        const int gpv = Gp > 0 ? (Gp + 3) / 4 : 1;              // 4-byte groups per voxel
        const int vpi = UM_BLOCK / gpv;                         // voxels per sweep of the workgroup
        const int j = t % gpv, slot0 = t / gpv;
        const bool active = Gp > 0 && slot0 < vpi;
        const int nb = Gp - j * 4 < 4 ? Gp - j * 4 : 4;
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        for (int i = t; i < UM_GPASS; i += UM_BLOCK) cnt[i] = 0;
        for (int c = sl; c < nchunks; c += slabs) {
            const int q = c * UM_BLOCK + t;
            bool set = false;
            int lin = 0;
            __syncthreads();                                    // staging done / last sweep's readers done
            if (q < bx.nvox) {
                const int oz = q % bx.dd, r = q / bx.dd;
                const int ox = r % bx.ww, oy = r / bx.ww;
                set = um_set(um_sm, m, ry, rx, rz, oy, ox, oz, rthr);
                lin = ((bx.y1 + oy) * W + (bx.x1 + ox)) * D + (bx.z1 + oz);
            }
            if (g0 == 0) myarea += set;
            if (Gp == 0) continue;
            flag[t] = set;
            vlin[t] = lin;
            __syncthreads();
            if (active) {
                for (int s = slot0; s < UM_BLOCK; s += vpi) {
                    if (!flag[s]) continue;
                    const uint8_t* __restrict__ p = gt + (int64_t)vlin[s] * G + g0 + j * 4;
                    if (nb == 4) {
                        uint32_t w;
                        __builtin_memcpy(&w, p, 4);
                        c0 += (w & 0xFFu) != 0;
                        c1 += (w & 0xFF00u) != 0;
                        c2 += (w & 0xFF0000u) != 0;
                        c3 += (w & 0xFF000000u) != 0;
                    } else {                                    // the row's tail group: never read past it
                        c0 += p[0] != 0;
                        if (nb > 1) c1 += p[1] != 0;
                        if (nb > 2) c2 += p[2] != 0;
                    }
                }
            }
        }
        if (Gp > 0) {
            __syncthreads();
            if (active) {
                if (c0) atomicAdd(&cnt[j * 4], c0);
                if (nb > 1 && c1) atomicAdd(&cnt[j * 4 + 1], c1);
                if (nb > 2 && c2) atomicAdd(&cnt[j * 4 + 2], c2);
                if (nb > 3 && c3) atomicAdd(&cnt[j * 4 + 3], c3);
            }
            __syncthreads();
            for (int g = t; g < Gp; g += UM_BLOCK)
                if (cnt[g]) atomicAdd(&inter[nd * G + g0 + g], cnt[g]);
            __syncthreads();
        }
    }
    for (int o = 32; o > 0; o >>= 1) myarea += __shfl_xor(myarea, o);
    __syncthreads();
    if ((t & 63) == 0 && myarea) atomicAdd(&area, myarea);
    __syncthreads();
    if (t == 0 && area) atomicAdd(&area_pred[nd], area);
}

__global__ __launch_bounds__(64) void um_finalize_kernel(
        const int32_t* __restrict__ box_i, int32_t* __restrict__ status, int G, int32_t* __restrict__ area_pred,
        int32_t* __restrict__ inter, const int32_t* __restrict__ area_gt, float* __restrict__ iou) {
    const int64_t nd = blockIdx.x;
    const int t = threadIdx.x;
    const int32_t* b = box_i + nd * 6;
    int ap = area_pred[nd];
    bool zero = status[nd] != M3D_UNMOLD_OK;
    bool sparse = false;
    if (!zero) {
        const double vol = (double)(b[3] - b[0]) * (double)(b[4] - b[1]) * (double)(b[5] - b[2]);
        sparse = (double)ap / vol < 0.00001;                    // (f)
        zero = sparse;
    }
    __syncthreads();                                            // every lane has read the row's state
    if (zero) ap = 0;
    if (t == 0) {
        if (sparse) status[nd] = M3D_UNMOLD_SPARSE;
        if (zero) area_pred[nd] = 0;
    }
    for (int g = t; g < G; g += 64) {
        int in = inter[nd * G + g];
        if (zero) {
            in = 0;
            inter[nd * G + g] = 0;
        }
        if (iou != nullptr) {
            const float fi = (float)in;
            iou[nd * G + g] = fi / (((float)ap + (float)area_gt[g]) - fi);   // 0 / 0 stays NaN
        }
    }
}

__global__ __launch_bounds__(UM_BLOCK) void um_paste_kernel(
        const uint8_t* __restrict__ small, const int32_t* __restrict__ box_i, const int32_t* __restrict__ status,
        const double* __restrict__ stats, int m, int H, int W, int D, int slabs, uint8_t* __restrict__ dense,
        uint8_t* __restrict__ seg_union) {
    extern __shared__ __attribute__((aligned(16))) uint8_t um_sm[];
    const int t = threadIdx.x;
    const int64_t nd = blockIdx.x / (unsigned)slabs;
    const int sl = (int)(blockIdx.x % (unsigned)slabs);
    if (status[nd] != M3D_UNMOLD_OK) return;
    const UmBox bx = um_box(box_i, nd, H, W, D);
    const int nchunks = (bx.nvox + UM_BLOCK - 1) / UM_BLOCK;
    if (sl >= nchunks) return;
    const int n = m * m * m;
    um_stage(um_sm, small + nd * n, n);
    __syncthreads();
    const double ry = (double)m / (double)bx.hh, rx = (double)m / (double)bx.ww, rz = (double)m / (double)bx.dd;
    const double rthr = stats[nd * 8 + 7];
    const int64_t vol = (int64_t)H * W * D;
    for (int c = sl; c < nchunks; c += slabs) {
        const int q = c * UM_BLOCK + t;
        if (q >= bx.nvox) continue;
        const int oz = q % bx.dd, r = q / bx.dd;
        const int ox = r % bx.ww, oy = r / bx.ww;
        if (!um_set(um_sm, m, ry, rx, rz, oy, ox, oz, rthr)) continue;
        const int64_t lin = ((int64_t)(bx.y1 + oy) * W + (bx.x1 + ox)) * D + (bx.z1 + oz);
        if (dense != nullptr) dense[nd * vol + lin] = 1;
        if (seg_union != nullptr) seg_union[lin] = 1;           // racing writers all write 1
    }
}

// area_gt[g] += the number of non-zero bytes of column g of gt [V,G].  Lanes are
// (voxel, 4-byte group) as in um_overlaps_kernel: a wave's loads are contiguous.
__global__ __launch_bounds__(UM_BLOCK) void um_areas_kernel(const uint8_t* __restrict__ gt, int64_t V, int G,
                                                            int32_t* __restrict__ area_gt) {
    __shared__ int cnt[UM_GPASS];
    const int t = threadIdx.x;
    for (int g0 = 0; g0 < G; g0 += UM_GPASS) {
        const int Gp = G - g0 < UM_GPASS ? G - g0 : UM_GPASS;
        const int gpv = (Gp + 3) / 4, vpi = UM_BLOCK / gpv;
        const int j = t % gpv, slot0 = t / gpv;
        const int nb = Gp - j * 4 < 4 ? Gp - j * 4 : 4;
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        for (int i = t; i < UM_GPASS; i += UM_BLOCK) cnt[i] = 0;
        __syncthreads();
        if (slot0 < vpi) {
            const uint8_t* __restrict__ base = gt + g0 + j * 4;
            const int64_t step = (int64_t)gridDim.x * vpi;
            if (nb == 4) {
#pragma unroll 4
                for (int64_t v = (int64_t)blockIdx.x * vpi + slot0; v < V; v += step) {
                    uint32_t w;
                    __builtin_memcpy(&w, base + v * G, 4);
                    c0 += (w & 0xFFu) != 0;
                    c1 += (w & 0xFF00u) != 0;
                    c2 += (w & 0xFF0000u) != 0;
                    c3 += (w & 0xFF000000u) != 0;
                }
            } else {
                for (int64_t v = (int64_t)blockIdx.x * vpi + slot0; v < V; v += step) {
                    const uint8_t* __restrict__ p = base + v * G;
                    c0 += p[0] != 0;
                    if (nb > 1) c1 += p[1] != 0;
                    if (nb > 2) c2 += p[2] != 0;
                }
            }
            if (c0) atomicAdd(&cnt[j * 4], c0);
            if (nb > 1 && c1) atomicAdd(&cnt[j * 4 + 1], c1);
            if (nb > 2 && c2) atomicAdd(&cnt[j * 4 + 2], c2);
            if (nb > 3 && c3) atomicAdd(&cnt[j * 4 + 3], c3);
        }
        __syncthreads();
        for (int g = t; g < Gp; g += UM_BLOCK)
            if (cnt[g]) atomicAdd(&area_gt[g0 + g], cnt[g]);
        __syncthreads();
    }
}

// ---- instance labels, pixelwise counts, the TIFF page order --------------------
constexpr int UM_SCAN_BLOCK = 1024;      // one workgroup numbers the rows: 64 rows per lane at 65535
constexpr int UM_MAX_LABEL = 65535;      // a label fits the widest sample m3d_labels_stack writes
constexpr int UM_PX_UNROLL = 8;          // voxels per (voxel, group) lane between two barriers
constexpr int UM_TR_TILE = 64;           // the [W,D] -> [D,W] transpose tile (64 x 64 labels in LDS)

// label_of[row] = 1 + the row's index among the listed rows (status != NOT_KEPT
// and keep[row] != 0), 0 for the others: an exclusive scan in one workgroup.
__global__ __launch_bounds__(UM_SCAN_BLOCK) void um_label_of_kernel(const int32_t* __restrict__ status,
                                                                    const uint8_t* __restrict__ keep, int n,
                                                                    int32_t* __restrict__ label_of) {
    __shared__ int ws[UM_SCAN_BLOCK / 64];
    const int t = threadIdx.x;
    const int per = (n + UM_SCAN_BLOCK - 1) / UM_SCAN_BLOCK;
    const int lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int c = 0;
    for (int i = lo; i < hi; ++i) c += status[i] != M3D_UNMOLD_NOT_KEPT && (keep == nullptr || keep[i] != 0);
    int v = c;                                                  // inclusive scan of the wave
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(v, o);
        if ((t & 63) >= o) v += x;
    }
    if ((t & 63) == 63) ws[t >> 6] = v;
    __syncthreads();
    int run = v - c;
    for (int w = 0; w < (t >> 6); ++w) run += ws[w];
    for (int i = lo; i < hi; ++i) {
        const bool listed = status[i] != M3D_UNMOLD_NOT_KEPT && (keep == nullptr || keep[i] != 0);
        label_of[i] = listed ? ++run : 0;
    }
}

// um_paste_kernel's traversal; a set voxel takes the largest label of the
// detections set there (the reference paints in ascending order: the later
// detection wins).  The maximum does not depend on the order of arrival.
__global__ __launch_bounds__(UM_BLOCK) void um_labels_kernel(
        const uint8_t* __restrict__ small, const int32_t* __restrict__ box_i, const int32_t* __restrict__ status,
        const double* __restrict__ stats, const int32_t* __restrict__ label_of, int m, int H, int W, int D,
        int slabs, int32_t* __restrict__ labels) {
    extern __shared__ __attribute__((aligned(16))) uint8_t um_sm[];
    const int t = threadIdx.x;
    const int64_t nd = blockIdx.x / (unsigned)slabs;
    const int sl = (int)(blockIdx.x % (unsigned)slabs);
    const int lab = label_of[nd];
    if (lab <= 0 || status[nd] != M3D_UNMOLD_OK) return;        // unlisted, or listed without a mask
    const UmBox bx = um_box(box_i, nd, H, W, D);
    const int nchunks = (bx.nvox + UM_BLOCK - 1) / UM_BLOCK;
    if (sl >= nchunks) return;
    const int n = m * m * m;
    um_stage(um_sm, small + nd * n, n);
    __syncthreads();
    const double ry = (double)m / (double)bx.hh, rx = (double)m / (double)bx.ww, rz = (double)m / (double)bx.dd;
    const double rthr = stats[nd * 8 + 7];
    for (int c = sl; c < nchunks; c += slabs) {
        const int q = c * UM_BLOCK + t;
        if (q >= bx.nvox) continue;
        const int oz = q % bx.dd, r = q / bx.dd;
        const int ox = r % bx.ww, oy = r / bx.ww;
        if (!um_set(um_sm, m, ry, rx, rz, oy, ox, oz, rthr)) continue;
        const int64_t lin = ((int64_t)(bx.y1 + oy) * W + (bx.x1 + ox)) * D + (bx.z1 + oz);
        atomicMax(&labels[lin], lab);
    }
}

// counts[0..2] += tp, fp, fn of (labels > 0) against (any GT byte of the voxel
// set).  Lanes are (voxel, 4-byte group) as in um_areas_kernel; a lane whose
// groups hold a set byte raises its voxel's flag in LDS, then one lane per
// voxel takes the label and the flag.  A tile is UM_PX_UNROLL sweeps of the
// workgroup, all its loads in flight at once.  G == 0: no GT byte is read.
__global__ __launch_bounds__(UM_BLOCK) void um_pixelwise_kernel(const int32_t* __restrict__ labels,
                                                                const uint8_t* __restrict__ gt, int64_t V, int G,
                                                                unsigned long long* __restrict__ counts) {
    __shared__ int flags[2 * UM_BLOCK * UM_PX_UNROLL];          // two tiles of voxel flags, used in turn
    __shared__ int part[3][UM_BLOCK / 64];
    const int t = threadIdx.x;
    const int ng = (G + 3) / 4;                                 // 4-byte groups of a voxel's GT row
    const int gpv = ng < 1 ? 1 : (ng < UM_BLOCK ? ng : UM_BLOCK);   // lanes per voxel
    const int vpi = UM_BLOCK / gpv;                             // voxels per sweep of the workgroup
    const int T = vpi * UM_PX_UNROLL;                           // voxels per tile
    const int j = t % gpv, slot0 = t / gpv;
    // 4 <= G <= 1024: a lane has one group and loads it as one dword; the lane
    // of the row's tail group takes the row's last four bytes instead (they
    // overlap the group before it, which an "any" does not mind): no lane reads
    // past its row and none loops over bytes.
    const bool one = ng <= UM_BLOCK && G >= 4;
    const int off = j * 4 < G - 4 ? j * 4 : G - 4;
    int tp = 0, fp = 0, fn = 0;
    for (int i = t; i < 2 * UM_BLOCK * UM_PX_UNROLL; i += UM_BLOCK) flags[i] = 0;
    __syncthreads();
    int buf = 0;
    for (int64_t base = (int64_t)blockIdx.x * T; base < V; base += (int64_t)gridDim.x * T, buf ^= 1) {
        int* fl = flags + buf * (UM_BLOCK * UM_PX_UNROLL);
        int lab[UM_PX_UNROLL];                                  // the tile's labels, in flight with the GT loads
#pragma unroll
        for (int k = 0; k < UM_PX_UNROLL; ++k) {
            const int i = t + k * UM_BLOCK;
            lab[k] = (i < T && base + i < V) ? labels[base + i] : 0;
        }
        if (slot0 < vpi && one) {
            uint32_t w[UM_PX_UNROLL];
#pragma unroll
            for (int u = 0; u < UM_PX_UNROLL; ++u) {            // every load of the tile goes out before the first use
                const int64_t v = base + u * vpi + slot0;
                w[u] = 0;
                if (v < V) __builtin_memcpy(&w[u], gt + v * G + off, 4);        // 64-bit byte offset
            }
#pragma unroll
            for (int u = 0; u < UM_PX_UNROLL; ++u)
                if (w[u]) fl[u * vpi + slot0] = 1;              // LDS; every writer of a flag writes 1
        } else if (slot0 < vpi) {                               // G > 1024: a lane walks its groups; G < 4: byte loads
            for (int u = 0; u < UM_PX_UNROLL; ++u) {
                const int64_t v = base + u * vpi + slot0;
                if (v >= V) break;
                const uint8_t* __restrict__ row = gt + v * G;
                bool any = false;
                for (int g = j; g < ng; g += gpv) {
                    if (g * 4 + 4 <= G) {
                        uint32_t w;
                        __builtin_memcpy(&w, row + g * 4, 4);
                        any |= w != 0;
                    } else {                                    // the row's tail group: never read past it
                        for (int b = g * 4; b < G; ++b) any |= row[b] != 0;
                    }
                }
                if (any) fl[u * vpi + slot0] = 1;
            }
        }
        // One barrier per tile: the next tile raises flags in the other half, and
        // the one after it passes the next barrier first, behind every reader here.
        lds_barrier();
#pragma unroll
        for (int k = 0; k < UM_PX_UNROLL; ++k) {
            const int i = t + k * UM_BLOCK;
            if (i < T && base + i < V) {
                const bool p = lab[k] > 0, g = fl[i] != 0;
                fl[i] = 0;
                tp += p && g;
                fp += p && !g;
                fn += !p && g;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        tp += __shfl_xor(tp, o);
        fp += __shfl_xor(fp, o);
        fn += __shfl_xor(fn, o);
    }
    if ((t & 63) == 0) {
        part[0][t >> 6] = tp;
        part[1][t >> 6] = fp;
        part[2][t >> 6] = fn;
    }
    __syncthreads();
    if (t < 3) {
        unsigned long long sum = 0;                             // a workgroup sees fewer than 2^31 voxels
        for (int w = 0; w < UM_BLOCK / 64; ++w) sum += (unsigned long long)part[t][w];
        if (sum) atomicAdd(&counts[t], sum);
    }
}

// stack[d,h,w] = (T)labels[h,w,d]: each h plane's [W,D] -> [D,W] through a
// padded LDS tile, reads contiguous along D, writes contiguous along W.
template <typename T>
__global__ __launch_bounds__(UM_BLOCK) void um_stack_kernel(const int32_t* __restrict__ labels, int H, int W, int D,
                                                            int tw, int td, T* __restrict__ stack) {
    __shared__ int32_t tile[UM_TR_TILE][UM_TR_TILE + 1];        // [w][d], padded: no bank conflict either way
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const unsigned b = blockIdx.x;
    const int d0 = (int)(b % (unsigned)td) * UM_TR_TILE;
    const int w0 = (int)((b / (unsigned)td) % (unsigned)tw) * UM_TR_TILE;
    const int h = (int)(b / ((unsigned)td * (unsigned)tw));
    if (d0 + tx < D)
        for (int r = ty; r < UM_TR_TILE && w0 + r < W; r += UM_BLOCK / 64)
            tile[r][tx] = labels[((int64_t)h * W + (w0 + r)) * D + (d0 + tx)];
    __syncthreads();
    if (w0 + tx < W)
        for (int r = ty; r < UM_TR_TILE && d0 + r < D; r += UM_BLOCK / 64)
            stack[((int64_t)(d0 + r) * H + h) * W + (w0 + tx)] = (T)tile[tx][r];
}

static int um_slabs(int64_t vol) {
    int64_t s = (vol + UM_SLAB_VOX - 1) / UM_SLAB_VOX;
    return (int)(s < 1 ? 1 : (s > UM_MAX_SLABS ? UM_MAX_SLABS : s));
}

// shapes shared by every entry: 0 = fine
static int um_check(int64_t max_inst, int64_t m, int64_t H, int64_t W, int64_t D) {
    if (max_inst < 0 || max_inst > (1 << 24)) return einval("unmold: max_inst must be in [0, 2^24]");
    if (m <= 0 || H <= 0 || W <= 0 || D <= 0) return einval("unmold: m, H, W and D must be positive");
    if (m > 32 || m * m * m > UM_MAX_N) return einval("unmold: m^3 must be <= 32768 (the grid is sorted in LDS)");
    if (H > 0x7FFFFFFF / W || H * W > 0x7FFFFFFF / D) return einval("unmold: H * W * D must fit 31 bits");
    return M3D_OK;
}

}  // namespace m3d

using namespace m3d;

extern "C" int m3d_unmold_prepare(const float* detections, const float* mrcnn_mask, int64_t max_inst, int64_t m,
                                  int64_t C, int64_t H, int64_t W, int64_t D, uint8_t* small, int32_t* box_i,
                                  int32_t* status, double* stats, m3d_stream_t s) {
    if (int rc = um_check(max_inst, m, H, W, D)) return rc;
    if (C <= 0 || C > 0x7FFFFFFF) return einval("unmold_prepare: C must be positive");
    if (detections == nullptr || mrcnn_mask == nullptr || small == nullptr || box_i == nullptr ||
        status == nullptr || stats == nullptr)
        return einval("unmold_prepare: NULL pointer");
    if (max_inst == 0) return M3D_OK;
    const int n = (int)(m * m * m);
    const int frac = (int)((double)n * 0.0002);
    hipLaunchKernelGGL(um_prepare_kernel, dim3((unsigned)max_inst), dim3(UM_PREP_BLOCK), 0, st(s), detections,
                       mrcnn_mask, (int)m, (int)C, (int)H, (int)W, (int)D, frac > 2 ? frac : 2, small, box_i, status,
                       stats);
    return check_launch("um_prepare_kernel");
}

extern "C" int m3d_unmold_overlaps(const uint8_t* small, const int32_t* box_i, const int32_t* status,
                                   const double* stats, int64_t max_inst, int64_t m, int64_t H, int64_t W,
                                   int64_t D, const uint8_t* gt_masks, int64_t G, int32_t* area_pred,
                                   int32_t* inter, m3d_stream_t s) {
    if (int rc = um_check(max_inst, m, H, W, D)) return rc;
    if (G < 0 || G > 0x7FFFFFFF) return einval("unmold_overlaps: G must be in [0, 2^31)");
    if (small == nullptr || box_i == nullptr || status == nullptr || stats == nullptr || area_pred == nullptr)
        return einval("unmold_overlaps: NULL pointer");
    if (G > 0 && (gt_masks == nullptr || inter == nullptr))
        return einval("unmold_overlaps: gt_masks and inter must not be NULL when G > 0");
    if (max_inst == 0) return M3D_OK;
    if (hipMemsetAsync(area_pred, 0, sizeof(int32_t) * (size_t)max_inst, st(s)) != hipSuccess ||
        (G > 0 && hipMemsetAsync(inter, 0, sizeof(int32_t) * (size_t)(max_inst * G), st(s)) != hipSuccess))
        return check_launch("unmold_overlaps: memset");
    const int slabs = um_slabs(H * W * D);
    hipLaunchKernelGGL(um_overlaps_kernel, dim3((unsigned)(max_inst * slabs)), dim3(UM_BLOCK),
                       (size_t)((m * m * m + 15) & ~(int64_t)15), st(s), small, box_i, status, stats, (int)m, (int)H,
                       (int)W, (int)D, gt_masks, (int)G, slabs, area_pred, inter);
    return check_launch("um_overlaps_kernel");
}

extern "C" int m3d_unmold_finalize(const int32_t* box_i, int32_t* status, int64_t max_inst, int64_t G,
                                   int32_t* area_pred, int32_t* inter, const int32_t* area_gt, float* iou,
                                   m3d_stream_t s) {
    if (max_inst < 0 || max_inst > (1 << 24)) return einval("unmold: max_inst must be in [0, 2^24]");
    if (G < 0 || G > 0x7FFFFFFF) return einval("unmold_finalize: G must be in [0, 2^31)");
    if (box_i == nullptr || status == nullptr || area_pred == nullptr)
        return einval("unmold_finalize: NULL pointer");
    if (G > 0 && inter == nullptr) return einval("unmold_finalize: inter must not be NULL when G > 0");
    if (iou != nullptr && area_gt == nullptr) return einval("unmold_finalize: iou needs area_gt");
    if (max_inst == 0) return M3D_OK;
    hipLaunchKernelGGL(um_finalize_kernel, dim3((unsigned)max_inst), dim3(64), 0, st(s), box_i, status, (int)G,
                       area_pred, inter, area_gt, iou);
    return check_launch("um_finalize_kernel");
}

extern "C" int m3d_unmold_paste(const uint8_t* small, const int32_t* box_i, const int32_t* status,
                                const double* stats, int64_t max_inst, int64_t m, int64_t H, int64_t W, int64_t D,
                                uint8_t* dense, uint8_t* seg_union, m3d_stream_t s) {
    if (int rc = um_check(max_inst, m, H, W, D)) return rc;
    if (small == nullptr || box_i == nullptr || status == nullptr || stats == nullptr)
        return einval("unmold_paste: NULL pointer");
    if (max_inst == 0 || (dense == nullptr && seg_union == nullptr)) return M3D_OK;
    const int slabs = um_slabs(H * W * D);
    hipLaunchKernelGGL(um_paste_kernel, dim3((unsigned)(max_inst * slabs)), dim3(UM_BLOCK),
                       (size_t)((m * m * m + 15) & ~(int64_t)15), st(s), small, box_i, status, stats, (int)m, (int)H,
                       (int)W, (int)D, slabs, dense, seg_union);
    return check_launch("um_paste_kernel");
}

extern "C" int m3d_mask_areas(const uint8_t* gt_masks, int64_t H, int64_t W, int64_t D, int64_t G,
                              int32_t* area_gt, m3d_stream_t s) {
    if (H <= 0 || W <= 0 || D <= 0) return einval("mask_areas: H, W and D must be positive");
    if (H > 0x7FFFFFFF / W || H * W > 0x7FFFFFFF / D) return einval("mask_areas: H * W * D must fit 31 bits");
    if (G < 0 || G > 0x7FFFFFFF) return einval("mask_areas: G must be in [0, 2^31)");
    if (G == 0) return M3D_OK;
    if (gt_masks == nullptr || area_gt == nullptr) return einval("mask_areas: NULL pointer");
    if (hipMemsetAsync(area_gt, 0, sizeof(int32_t) * (size_t)G, st(s)) != hipSuccess)
        return check_launch("mask_areas: memset");
    const int64_t V = H * W * D;
    const int gp = G < UM_GPASS ? (int)G : UM_GPASS;
    const int vpi = UM_BLOCK / ((gp + 3) / 4);
    hipLaunchKernelGGL(um_areas_kernel, dim3(grid_for(V, vpi * 8, 4096)), dim3(UM_BLOCK), 0, st(s), gt_masks, V,
                       (int)G, area_gt);
    return check_launch("um_areas_kernel");
}

extern "C" int m3d_unmold_labels(const uint8_t* small, const int32_t* box_i, const int32_t* status,
                                 const double* stats, const uint8_t* keep, int64_t max_inst, int64_t m, int64_t H,
                                 int64_t W, int64_t D, int32_t* label_of, int32_t* labels, m3d_stream_t s) {
    if (int rc = um_check(max_inst, m, H, W, D)) return rc;
    if (max_inst > UM_MAX_LABEL) return einval("unmold_labels: max_inst must be <= 65535 (a label fits 16 bits)");
    if (small == nullptr || box_i == nullptr || status == nullptr || stats == nullptr || label_of == nullptr ||
        labels == nullptr)
        return einval("unmold_labels: NULL pointer");
    if (hipMemsetAsync(labels, 0, sizeof(int32_t) * (size_t)(H * W * D), st(s)) != hipSuccess)
        return check_launch("unmold_labels: memset");
    if (max_inst == 0) return M3D_OK;
    hipLaunchKernelGGL(um_label_of_kernel, dim3(1), dim3(UM_SCAN_BLOCK), 0, st(s), status, keep, (int)max_inst,
                       label_of);
    if (int rc = check_launch("um_label_of_kernel")) return rc;
    const int slabs = um_slabs(H * W * D);
    hipLaunchKernelGGL(um_labels_kernel, dim3((unsigned)(max_inst * slabs)), dim3(UM_BLOCK),
                       (size_t)((m * m * m + 15) & ~(int64_t)15), st(s), small, box_i, status, stats, label_of,
                       (int)m, (int)H, (int)W, (int)D, slabs, labels);
    return check_launch("um_labels_kernel");
}

// shapes shared by the two label-volume entries: 0 = fine
static int um_check_volume(const char* who, int64_t H, int64_t W, int64_t D) {
    if (H <= 0 || W <= 0 || D <= 0) return (set_error("%s: H, W and D must be positive", who), M3D_EINVAL);
    if (H > 0x7FFFFFFF / W || H * W > 0x7FFFFFFF / D)
        return (set_error("%s: H * W * D must fit 31 bits", who), M3D_EINVAL);
    return M3D_OK;
}

extern "C" int m3d_label_pixelwise(const int32_t* labels, const uint8_t* gt_masks, int64_t H, int64_t W, int64_t D,
                                   int64_t G, int64_t* counts, m3d_stream_t s) {
    if (int rc = um_check_volume("label_pixelwise", H, W, D)) return rc;
    if (G < 0 || G > 0x7FFFFFFF) return einval("label_pixelwise: G must be in [0, 2^31)");
    if (labels == nullptr || counts == nullptr) return einval("label_pixelwise: NULL pointer");
    if (G > 0 && gt_masks == nullptr) return einval("label_pixelwise: gt_masks must not be NULL when G > 0");
    if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 3, st(s)) != hipSuccess)
        return check_launch("label_pixelwise: memset");
    const int64_t V = H * W * D;
    const int64_t ng = (G + 3) / 4;
    const int vpi = UM_BLOCK / (int)(ng < 1 ? 1 : (ng < UM_BLOCK ? ng : UM_BLOCK));
    hipLaunchKernelGGL(um_pixelwise_kernel, dim3(grid_for(V, vpi * UM_PX_UNROLL, 4096)), dim3(UM_BLOCK), 0, st(s),
                       labels, gt_masks, V, (int)G, reinterpret_cast<unsigned long long*>(counts));
    return check_launch("um_pixelwise_kernel");
}

extern "C" int m3d_labels_stack(const int32_t* labels, int64_t H, int64_t W, int64_t D, int64_t bytes_per_sample,
                                void* stack, m3d_stream_t s) {
    if (int rc = um_check_volume("labels_stack", H, W, D)) return rc;
    if (bytes_per_sample != 1 && bytes_per_sample != 2)
        return einval("labels_stack: bytes_per_sample must be 1 or 2");
    if (labels == nullptr || stack == nullptr) return einval("labels_stack: NULL pointer");
    const int tw = (int)((W + UM_TR_TILE - 1) / UM_TR_TILE), td = (int)((D + UM_TR_TILE - 1) / UM_TR_TILE);
    const dim3 grid((unsigned)(H * tw * td));                   // <= H * W * D < 2^31
    if (bytes_per_sample == 1)
        hipLaunchKernelGGL(um_stack_kernel<uint8_t>, grid, dim3(UM_BLOCK), 0, st(s), labels, (int)H, (int)W, (int)D,
                           tw, td, static_cast<uint8_t*>(stack));
    else
        hipLaunchKernelGGL(um_stack_kernel<uint16_t>, grid, dim3(UM_BLOCK), 0, st(s), labels, (int)H, (int)W,
                           (int)D, tw, td, static_cast<uint16_t*>(stack));
    return check_launch("um_stack_kernel");
}
