// ---- the RPN head's backward on the sampled anchors' rows ---------------------
// Everything above rpn_conv_shared1 is 1x1x1, so the head's output gradient is
// row-sparse from the loss down to the 3x3x3 conv: the active voxel rows are
// found once, from the loss gradient itself (dlogits [R][2 apl], dbbox
// [R][6 apl], R the level-concatenated rows, B = 1), and the whole chain
//   rpn_class_raw + rpn_bbox_pred -> ReLU -> rpn_conv_shared2 -> ReLU -> rpn_conv_shared1
// runs on compact [cap][C] matrices (rows n..cap zero).  rpn_conv_shared1 takes
// the compact gradient and the row list directly, all levels in one set of
// launches: the tap gather of rs_pack_kernel and one 27-batch split GEMM for
// dw, one GEMM ct = dz1c w and rs_dgrad_out_kernel per level for dx (slots are
// global over the levels).  Launch shapes are fixed by (R, cap): a graph replay
// follows the data.  More than cap active rows is an error of the caller's
// bound, made loud: the sticky word h[HC_OVERFLOW] counts it and dz3c is filled
// with NaN, which every gradient of the step inherits.
// Workspace: the header of rs_hdr (h[RS_SKIP_SPARSE] = 0, h[RS_N] = min(n, cap);
// beside it h[HC_NRAW] = n, h[HC_OVERFLOW], h[HC_LEVEL0 + l] = first slot of
// level l, l = 0..nlevels), then dz3c [cap][npad], s2c [cap][C2], s1c [cap][C1],
// dz2c [cap][C2], dz1c [cap][C1], the planes of w1, ct [cap][27 C0], xg [27][cap][C0]
// and the dw24 / dw2 chunk partials (double [cap / 64][C2][max(npad, C1)]).
#include "conv_types.h"

namespace m3d {

enum { HC_NRAW = 8, HC_OVERFLOW = 16, HC_LEVEL0 = 32 };
constexpr int HC_CHUNK = 64;               // compact rows per dw24 / dw2 partial

struct HcLevels {
    const float* p[M3D_RPN_HEAD_MAX_LEVELS];
    const float* s1[M3D_RPN_HEAD_MAX_LEVELS];
    const float* s2[M3D_RPN_HEAD_MAX_LEVELS];
    int row0[M3D_RPN_HEAD_MAX_LEVELS + 1];     // first row of each level; [n] = R
    int H[M3D_RPN_HEAD_MAX_LEVELS], W[M3D_RPN_HEAD_MAX_LEVELS], D[M3D_RPN_HEAD_MAX_LEVELS];
    int n;
};

struct HcWs {
    RsHdr hd{};
    float *dz3c, *s2c, *s1c, *dz2c, *dz1c, *ct, *xg;
    double* part;
    unsigned short* w1p;
    size_t bytes;
};
static HcWs hc_ws(void* base, int64_t R, int cap, int npad, int64_t C0, int64_t C1, int64_t C2) {
    HcWs w{};
    char* p = static_cast<char*>(base);             // (NULL: the size only)
    size_t o = 0;
    auto take = [&](size_t b) { char* q = p ? p + o : nullptr; o += rs_al(b); return q; };
    char* hdr = take(rs_hdr_bytes(R));
    if (hdr) w.hd = rs_hdr(hdr, R);
    w.dz3c = reinterpret_cast<float*>(take(4 * (size_t)cap * npad));
    w.s2c = reinterpret_cast<float*>(take(4 * (size_t)cap * C2));
    w.s1c = reinterpret_cast<float*>(take(4 * (size_t)cap * C1));
    w.dz2c = reinterpret_cast<float*>(take(4 * (size_t)cap * C2));
    w.dz1c = reinterpret_cast<float*>(take(4 * (size_t)cap * C1));
    w.w1p = reinterpret_cast<unsigned short*>(take(6 * 27 * (size_t)C0 * C1));
    w.ct = reinterpret_cast<float*>(take(4 * (size_t)cap * 27 * C0));
    w.xg = reinterpret_cast<float*>(take(4 * 27 * (size_t)cap * C0));
    w.part = reinterpret_cast<double*>(take(8 * (size_t)(cap / HC_CHUNK) * C2 * (C1 > npad ? C1 : npad)));
    w.bytes = o;
    return w;
}

// slot[row] = row active (0 / 1), blk[group] = active rows of the group's RS_BLK rows; one thread per
// row (the rule of rs_lane_active: any element != 0.0f, so -0.0f is not and a NaN is)
__global__ __launch_bounds__(256) void hc_flag_kernel(const float* __restrict__ dl, const float* __restrict__ db,
                                                      int R, int nl, int nb, int* __restrict__ blk,
                                                      int* __restrict__ slot) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool a = false;
    if (r < R) {
        const float* pl = dl + (int64_t)r * nl;
        const float* pb = db + (int64_t)r * nb;
        for (int j = 0; j < nl; ++j) a |= pl[j] != 0.0f;
        for (int j = 0; j < nb; ++j) a |= pb[j] != 0.0f;
        slot[r] = a ? 1 : 0;
    }
    const unsigned long long m = __ballot(a);
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && (int64_t)g * RS_BLK < R) blk[g] = __popcll(m);
}

// the prefix of rs_pack_kernel over the flags: slot[row] = compact slot or -1, idx[slot] = row
// (ascending), the count, the levels' first slots and the overflow word.  Every workgroup sums blk
// itself; a workgroup owns 4 groups of RS_BLK rows.
__global__ __launch_bounds__(256) void hc_index_kernel(int R, int cap, HcLevels lv, int* __restrict__ h,
                                                       const int* __restrict__ blk, int* __restrict__ slot,
                                                       int* __restrict__ idx) {
    __shared__ int red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = (R + RS_BLK - 1) / RS_BLK;
    const int g0 = blockIdx.x * 4;
    int tot = 0, pre = 0;
    for (int i = tid; i < nblk; i += 256) {
        const int c = blk[i];
        tot += c;
        if (i < g0) pre += c;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        tot += __shfl_xor(tot, o);
        pre += __shfl_xor(pre, o);
    }
    if (lane == 0) { red[0][wave] = tot; red[1][wave] = pre; }
    __syncthreads();
    const int n = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const int nn = n < cap ? n : cap;
    if (blockIdx.x == 0 && tid == 0) {
        h[RS_STATE] = RS_SPARSE;
        h[RS_SKIP_DENSE] = 1;
        h[RS_SKIP_SPARSE] = 0;
        h[RS_N] = nn;
        h[RS_PROBE] = 0;
        h[HC_NRAW] = n;
        if (n > cap) h[HC_OVERFLOW] += 1;          // sticky: only the caller clears it
        h[HC_LEVEL0 + lv.n] = nn;
    }
    const int g = g0 + wave;
    if (g >= nblk) return;
    int base = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    for (int q = 0; q < wave; ++q) base += blk[g0 + q];
    const int r = g * RS_BLK + lane;
    const bool act = r < R && slot[r] != 0;
    const unsigned long long m = __ballot(act);
    const int s = base + __popcll(m & ((1ull << lane) - 1ull));    // active rows before r
    if (r < R) {
        slot[r] = act && s < cap ? s : -1;
        if (act && s < cap) idx[s] = r;
        for (int l = 0; l < lv.n; ++l)
            if (lv.row0[l] == r) h[HC_LEVEL0 + l] = s < cap ? s : cap;
    }
}

__device__ __forceinline__ int hc_level_of(const HcLevels& lv, int row) {
    int l = 0;
    while (l + 1 < lv.n && row >= lv.row0[l + 1]) ++l;
    return l;
}

// one wave per compact row r: dz3c[r] = [dlogits | dbbox | 0] of row idx[r], s2c[r] / s1c[r] that row
// of its level's rpn_conv_shared2 / rpn_conv_shared1 output; rows n..cap zero; overflow: dz3c = NaN
__global__ __launch_bounds__(256) void hc_gather_kernel(const float* __restrict__ dl, const float* __restrict__ db,
                                                        int nl, int nb, int npad, int cap, int C1, int C2,
                                                        HcLevels lv, const int* __restrict__ h,
                                                        const int* __restrict__ idx, float* __restrict__ dz3c,
                                                        float* __restrict__ s2c, float* __restrict__ s1c) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= cap) return;
    const int n = h[HC_NRAW];
    const bool on = r < n;                         // (overflow: n > cap, every row on)
    int row = 0, l = 0;
    if (on) {
        row = idx[r];
        l = hc_level_of(lv, row);
    }
    if (lane < npad) {
        float v = 0.0f;
        if (on && lane < nl) v = dl[(int64_t)row * nl + lane];
        else if (on && lane < nl + nb) v = db[(int64_t)row * nb + lane - nl];
        if (n > cap) v = __builtin_nanf("");
        dz3c[(int64_t)r * npad + lane] = v;
    }
    const int64_t local = row - lv.row0[l];
    rs_copy_row(lv.s2[l] + local * C2, s2c + (int64_t)r * C2, C2, lane, on);
    rs_copy_row(lv.s1[l] + local * C1, s1c + (int64_t)r * C1, C1, lane, on);
}

// out[c] += sum over the rows of x [rows][C], in a fixed order: a workgroup owns 64 columns, its 16
// waves every 16th row each, then the 16 partials in wave order.  (These small reductions keep their
// running sums in double: a handful of adds per thread, and the compact rows' sums round once.)
__global__ __launch_bounds__(1024) void hc_colsum_kernel(const float* __restrict__ x, int rows, int C,
                                                         float* __restrict__ out) {
    __shared__ double part[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    double a = 0.0;
    if (c < C)
        for (int r = wave; r < rows; r += 16) a += (double)x[(int64_t)r * C + c];
    part[wave][lane] = a;
    __syncthreads();
    if (wave == 0 && c < C) {
        double s = part[0][lane];
        for (int q = 1; q < 16; ++q) s += part[q][lane];
        out[c] += (float)s;
    }
}

// dz2c[r][k] = [s2c[r][k] > 0] sum_j dz3c[r][j] w24[k][j]  (j < n8, ascending)
__global__ __launch_bounds__(256) void hc_dz2_kernel(const float* __restrict__ dz3c, const float* __restrict__ w24,
                                                     const float* __restrict__ s2c, int cap, int C2, int n8, int npad,
                                                     float* __restrict__ dz2c) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)cap * C2) return;
    const int r = (int)(i / C2), k = (int)(i % C2);
    double a = 0.0;
    for (int j = 0; j < n8; ++j) a += (double)dz3c[(int64_t)r * npad + j] * (double)w24[(int64_t)k * n8 + j];
    dz2c[i] = s2c[i] > 0.0f ? (float)a : 0.0f;
}

// dz1c[r][n] = [s1c[r][n] > 0] sum_k dz2c[r][k] w2[n][k], the running sum in double (k ascending), so
// each element is the correctly rounded product row: the compact 1x1x1 products are a few hundred MFLOP,
// and rounding them once keeps the compact chain no further from float64 than the dense launches, whose
// split GEMM on the same rows differs from it only in its last roundings.  A workgroup owns 16 compact
// rows x 64 columns n: the rows' dz2c in LDS (256 k at a time), lane = n, wave w rows 4w..4w+3; the
// lane walks its w2 row in float4s.  Row tiles at or past n store zeros.
constexpr int HC_DZ1_ROWS = 16;
__global__ __launch_bounds__(256) void hc_dz1_kernel(const float* __restrict__ dz2c, const float* __restrict__ w2,
                                                     const float* __restrict__ s1c, int K, int N,
                                                     const int* __restrict__ h, float* __restrict__ dz1c) {
    __shared__ __attribute__((aligned(16))) float a[HC_DZ1_ROWS][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x * 64 + lane, r0 = blockIdx.y * HC_DZ1_ROWS;
    if (r0 >= h[RS_N]) {                            // (uniform over the workgroup)
        for (int i = 0; i < 4; ++i) dz1c[(int64_t)(r0 + wave * 4 + i) * N + n] = 0.0f;
        return;
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < K; kc += 256) {
        __syncthreads();
        for (int rr = 0; rr < HC_DZ1_ROWS; ++rr)
            a[rr][tid] = kc + tid < K ? dz2c[(int64_t)(r0 + rr) * K + kc + tid] : 0.0f;
        __syncthreads();
        const int kn = K - kc < 256 ? K - kc : 256;
        for (int k = 0; k < kn; k += 4) {
            const float4 wv = *reinterpret_cast<const float4*>(w2 + (int64_t)n * K + kc + k);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 x = *reinterpret_cast<const float4*>(&a[wave * 4 + i][k]);
                acc[i] += (double)x.x * (double)wv.x;
                acc[i] += (double)x.y * (double)wv.y;
                acc[i] += (double)x.z * (double)wv.z;
                acc[i] += (double)x.w * (double)wv.w;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t o = (int64_t)(r0 + wave * 4 + i) * N + n;
        dz1c[o] = s1c[o] > 0.0f ? (float)acc[i] : 0.0f;
    }
}

// part[chunk][k][j] = sum over the chunk's HC_CHUNK compact rows of A[r][k] B[r][j] (A [cap][K],
// B [cap][N]; double, rows ascending); a thread owns four consecutive k of one column j.  Chunks at or
// past n are left out here and in the fold.
__global__ __launch_bounds__(256) void hc_wg_part_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                         int K, int N, const int* __restrict__ h,
                                                         double* __restrict__ part) {
    const int r0 = blockIdx.y * HC_CHUNK;
    if (r0 >= h[RS_N]) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)(K / 4) * N) return;
    const int k = (int)(i / N) * 4, j = (int)(i % N);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = r0; r < r0 + HC_CHUNK; ++r) {
        const float4 av = *reinterpret_cast<const float4*>(A + (int64_t)r * K + k);
        const double b = (double)B[(int64_t)r * N + j];
        acc[0] += (double)av.x * b;
        acc[1] += (double)av.y * b;
        acc[2] += (double)av.z * b;
        acc[3] += (double)av.w * b;
    }
    double* o = part + ((int64_t)blockIdx.y * K + k) * N + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(int64_t)q * N] = acc[q];
}

// dw[i] += sum over the chunks that hold an active row, in chunk order
__global__ __launch_bounds__(256) void hc_wg_reduce_kernel(const double* __restrict__ part, int kn,
                                                           const int* __restrict__ h, float* __restrict__ dw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int chunks = (h[RS_N] + HC_CHUNK - 1) / HC_CHUNK;
    if (i >= kn || chunks == 0) return;
    double s = part[i];
    for (int q = 1; q < chunks; ++q) s += part[(int64_t)q * kn + i];
    dw[i] += (float)s;
}

// xg[tap][r] = the tap's input row of compact row r (the tap gather of rs_pack_kernel, on the level
// of idx[r]; 'same' padding: zero outside; rows n..cap zero), one wave per compact row
__global__ __launch_bounds__(256) void hc_xg_kernel(HcLevels lv, int cap, int C, const int* __restrict__ h,
                                                    const int* __restrict__ idx, float* __restrict__ xg) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= cap) return;
    const bool on = r < h[RS_N];
    int H = 1, W = 1, D = 1, yo = 0, xo = 0, zo = 0;
    const float* x = lv.p[0];
    if (on) {
        const int row = idx[r], l = hc_level_of(lv, row);
        int t = row - lv.row0[l];
        H = lv.H[l]; W = lv.W[l]; D = lv.D[l];
        x = lv.p[l];
        zo = t % D; t /= D;
        xo = t % W;
        yo = t / W;
    }
    for (int c = lane * 4; c < C; c += 256) {
        float4 v[27];
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
            const int yi = yo + tap / 9 - 1, xi = xo + (tap / 3) % 3 - 1, zi = zo + tap % 3 - 1;
            const bool in = on && (unsigned)yi < (unsigned)H && (unsigned)xi < (unsigned)W && (unsigned)zi < (unsigned)D;
            v[tap] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (in) v[tap] = *reinterpret_cast<const float4*>(x + (((int64_t)yi * W + xi) * D + zi) * C + c);
        }
#pragma unroll
        for (int tap = 0; tap < 27; ++tap)
            *reinterpret_cast<float4*>(xg + ((int64_t)tap * cap + r) * C + c) = v[tap];
    }
}

// the argument checks of both entry points (no launch before them) and the level table
static int hc_check(const m3d_rpn_head_bwd_t* a, bool weight, HcLevels& lv, int64_t& R, int& npad) {
    if (!a) return einval("rpn_head_compact: NULL argument block");
    if (a->nlevels < 1 || a->nlevels > M3D_RPN_HEAD_MAX_LEVELS)
        return einval("rpn_head_compact: nlevels must be in [1, 8]");
    if (a->apl < 1 || 8 * a->apl > 64) return einval("rpn_head_compact: apl must be in [1, 8]");
    if (a->cap < 256 || a->cap > RS_CAP_MAX || a->cap % 256)
        return einval("rpn_head_compact: cap must be a multiple of 256 in [256, 4096]");
    if (a->C0 <= 0 || a->C1 <= 0 || a->C2 <= 0 || a->C0 % 64 || a->C1 % 64 || a->C2 % 64 || a->C0 > 4096 ||
        a->C1 > 4096 || a->C2 > 4096)
        return einval("rpn_head_compact: channel counts must be multiples of 64 in [64, 4096]");
    if ((int64_t)a->cap * 27 * a->C0 * 4 >= 0xFFFFFFF0LL || 27 * a->C0 * a->C1 * 2 >= 0xFFFFFFF0LL)
        return einval("rpn_head_compact: operand larger than 4 GiB (32-bit buffer offsets)");
    npad = (8 * a->apl + 31) / 32 * 32;
    R = 0;
    lv = HcLevels{};
    lv.n = a->nlevels;
    for (int l = 0; l < a->nlevels; ++l) {
        const m3d_rpn_head_level_t& q = a->levels[l];
        if (q.H <= 0 || q.W <= 0 || q.D <= 0) return einval("rpn_head_compact: level extents must be positive");
        if (!q.p || !q.s1 || !q.s2 || (!weight && !q.dp)) return einval("rpn_head_compact: NULL level pointer");
        if (!weight && (q.accumulate & ~1)) return einval("rpn_head_compact: accumulate must be 0 or 1");
        lv.p[l] = q.p; lv.s1[l] = q.s1; lv.s2[l] = q.s2;
        lv.H[l] = q.H; lv.W[l] = q.W; lv.D[l] = q.D;
        lv.row0[l] = (int)R;
        R += (int64_t)q.H * q.W * q.D;
        if (R > 0x7FFFFFFF / 64) return einval("rpn_head_compact: more than 2^25 voxel rows");
    }
    lv.row0[a->nlevels] = (int)R;
    if (!a->workspace || a->ws_bytes < m3d_rpn_head_compact_workspace_bytes(R, a->cap, a->apl, a->C0, a->C1, a->C2))
        return einval("rpn_head_compact: workspace missing or too small");
    if (weight) {
        if (!a->dw1 || !a->dw2 || !a->dw24) return einval("rpn_head_compact: NULL weight gradient");
    } else if (!a->dlogits || !a->dbbox || !a->w1 || !a->w2 || !a->w24 || !a->db1 || !a->db2 || !a->db24) {
        return einval("rpn_head_compact: NULL pointer");
    } else if (reinterpret_cast<uintptr_t>(a->w2) & 15) {
        return einval("rpn_head_compact: w2 must be 16-byte aligned");
    }
    return M3D_OK;
}

}  // namespace m3d

using namespace m3d;

extern "C" size_t m3d_rpn_head_compact_workspace_bytes(int64_t rows, int32_t cap, int32_t apl, int64_t C0,
                                                       int64_t C1, int64_t C2) {
    if (rows <= 0 || rows > 0x7FFFFFFF / 64 || cap < 256 || cap > RS_CAP_MAX || cap % 256 || apl < 1 || apl > 8 ||
        C0 <= 0 || C1 <= 0 || C2 <= 0 || C0 > 4096 || C1 > 4096 || C2 > 4096)
        return 0;
    return hc_ws(nullptr, rows, cap, (8 * apl + 31) / 32 * 32, C0, C1, C2).bytes;
}

// scan, gather, the 1x1x1 chain's data path with its bias sums, and rpn_conv_shared1's data gradient
extern "C" int m3d_rpn_head_compact_bwd_data(const m3d_rpn_head_bwd_t* a, m3d_stream_t s_) {
    HcLevels lv{};
    int64_t R;
    int npad;
    if (int rc = hc_check(a, false, lv, R, npad)) return rc;
    hipStream_t s = st(s_);
    const int cap = a->cap, nl = 2 * a->apl, nb = 6 * a->apl;
    const int C0 = (int)a->C0, C1 = (int)a->C1, C2 = (int)a->C2;
    const HcWs w = hc_ws(a->workspace, R, cap, npad, C0, C1, C2);
    const int nblk = (int)((R + RS_BLK - 1) / RS_BLK);
    hipLaunchKernelGGL(hc_flag_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, a->dlogits, a->dbbox, (int)R,
                       nl, nb, w.hd.blk, w.hd.slot);
    hipLaunchKernelGGL(hc_index_kernel, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, s, (int)R, cap, lv, w.hd.h,
                       w.hd.blk, w.hd.slot, w.hd.idx);
    hipLaunchKernelGGL(hc_gather_kernel, dim3((unsigned)(cap / 4)), dim3(256), 0, s, a->dlogits, a->dbbox, nl, nb, npad,
                       cap, C1, C2, lv, w.hd.h, w.hd.idx, w.dz3c, w.s2c, w.s1c);
    // rpn_class_raw + rpn_bbox_pred: bias sums, dz2c = (dz3c w24^T) [s2c > 0]
    hipLaunchKernelGGL(hc_colsum_kernel, dim3(1), dim3(1024), 0, s, w.dz3c, cap, npad, a->db24);
    hipLaunchKernelGGL(hc_dz2_kernel, dim3(grid_for((int64_t)cap * C2, 256)), dim3(256), 0, s, w.dz3c, a->w24, w.s2c,
                       cap, C2, nl + nb, npad, w.dz2c);
    hipLaunchKernelGGL(hc_colsum_kernel, dim3((unsigned)(C2 / 64)), dim3(1024), 0, s, w.dz2c, cap, C2, a->db2);
    // rpn_conv_shared2: dz1c = (dz2c w2^T) [s1c > 0]
    hipLaunchKernelGGL(hc_dz1_kernel, dim3((unsigned)(C1 / 64), (unsigned)(cap / HC_DZ1_ROWS)), dim3(256), 0, s, w.dz2c,
                       a->w2, w.s1c, C2, C1, w.hd.h, w.dz1c);
    hipLaunchKernelGGL(hc_colsum_kernel, dim3((unsigned)(C1 / 64)), dim3(1024), 0, s, w.dz1c, cap, C1, a->db1);
    // rpn_conv_shared1: ct[r][tap * C0 + c] = sum_n dz1c[r][n] w1[tap][c][n] (row tiles past n return),
    // then every level's dx from its slice of slot
    const int64_t nw = (int64_t)27 * C0 * C1;
    launch_split3(a->w1, nw, w.w1p, s);
    launch_gemm_x3(w.dz1c, reinterpret_cast<const float*>(w.w1p), w.ct, cap, C1, 27 * C0, 1, s, true, nullptr,
                   w.hd.h + RS_N);
    for (int l = 0; l < lv.n; ++l) {
        launch_rs_dgrad_out(w.ct, (int64_t)lv.H[l] * lv.W[l] * lv.D[l], lv.H[l], lv.W[l], lv.D[l], lv.D[l], 1, C0,
                            a->levels[l].accumulate, w.hd.h, w.hd.slot + lv.row0[l], a->levels[l].dp, s);
    }
    return check_launch("rpn_head_compact_bwd_data");
}

// the three weight gradients, from the compact matrices m3d_rpn_head_compact_bwd_data left in the
// workspace (enqueued after it: the same stream, or one that waits for it)
extern "C" int m3d_rpn_head_compact_bwd_weight(const m3d_rpn_head_bwd_t* a, const m3d_det_t* det, m3d_stream_t s_) {
    M3D_DET_SCOPE(det);
    HcLevels lv{};
    int64_t R;
    int npad;
    if (int rc = hc_check(a, true, lv, R, npad)) return rc;
    hipStream_t s = st(s_);
    const int cap = a->cap, C0 = (int)a->C0, C1 = (int)a->C1, C2 = (int)a->C2;
    const HcWs w = hc_ws(a->workspace, R, cap, npad, C0, C1, C2);
    // dw24 += s2c^T dz3c, dw2 += s1c^T dz2c: chunk partials, then the chunks in order
    const unsigned chunks = (unsigned)(cap / HC_CHUNK);
    hipLaunchKernelGGL(hc_wg_part_kernel, dim3(grid_for((int64_t)(C2 / 4) * npad, 256), chunks), dim3(256), 0, s, w.s2c,
                       w.dz3c, C2, npad, w.hd.h, w.part);
    hipLaunchKernelGGL(hc_wg_reduce_kernel, dim3(grid_for((int64_t)C2 * npad, 256)), dim3(256), 0, s, w.part, C2 * npad,
                       w.hd.h, a->dw24);
    hipLaunchKernelGGL(hc_wg_part_kernel, dim3(grid_for((int64_t)(C1 / 4) * C2, 256), chunks), dim3(256), 0, s, w.s1c,
                       w.dz2c, C1, C2, w.hd.h, w.part);
    hipLaunchKernelGGL(hc_wg_reduce_kernel, dim3(grid_for((int64_t)C1 * C2, 256)), dim3(256), 0, s, w.part, C1 * C2,
                       w.hd.h, a->dw2);
    // dw1[tap] += xg[tap]^T dz1c
    hipLaunchKernelGGL(hc_xg_kernel, dim3((unsigned)(cap / 4)), dim3(256), 0, s, lv, cap, C0, w.hd.h, w.hd.idx, w.xg);
    const int fe = launch_wgrad_x3(w.xg, w.dz1c, a->dw1, cap, C0, C1, 27, (int64_t)cap * C0, 0, (int64_t)C0 * C1, s);
    if (fe) {
        set_error("rpn_head_compact_bwd_weight: %s", hipGetErrorString((hipError_t)fe));
        return M3D_EHIP;
    }
    return check_launch("rpn_head_compact_bwd_weight");
}
