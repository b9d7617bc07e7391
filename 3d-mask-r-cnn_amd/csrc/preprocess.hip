// The input pipeline on the device, for gfx950: image normalisation and the
// training augmentations.
//
// Replaces the host numpy of ToyDataset.load_image (core/data_generators.py:
// 1603-1630: transpose, np.percentile, clip, mean / std, tanh), of
// MrcnnGenerator.get_input_prediction's second normalisation (1227-1242) and of
// apply_minimal_augs_3d (13-86: flips of image, masks and boxes, the brightness
// and the Gaussian noise legs).
//
//   normalize: the four order statistics behind the 1st and 99th percentile
//           (numpy's `linear` method) by radix selection on order-preserving
//           32-bit keys -- digit passes of 11, 11, 10 bits for float32, 8, 8
//           for uint16 and 8 for uint8, so a pass's four LDS histograms take
//           at most 4 x 2048 x 4 B = 32 KiB (a 65,536-bin histogram of 32-bit
//           counters does not fit the 160 KiB of a CU); the selection state
//           stays on the device between the passes, as in topk.hip.  Then one
//           pass for the sums of the clipped volume (exact integers for the
//           integer inputs, fp64 partials pivoted on p1 for float32; per-block
//           partials folded in a fixed order, no atomics), one thread forms
//           mean and std, and one pass writes tanh(0.5 (x - mean) / std)
//           evaluated in fp64 (a per-level table for the integer inputs)
//           through a 64 x 64 LDS tile that turns (Z,Y,X) into [Y,X,Z].
//   augment: flips folded into the read index, then the brightness leg (a
//           min / max reduction first) and the Gaussian leg from Philox4x32-10
//           keyed by the seed and counted by the output voxel's linear index,
//           so a voxel's value does not depend on the launch geometry.
//   flips of the [H,W,D,G] mask bytes (the widest vector the group or line
//           length and the pointers allow) and of the [N,6] boxes.
//
// Every entry point works on the caller's stream and workspace: no allocation,
// no synchronisation, no host round trip.
#include <math.h>
#include <string.h>

#include <type_traits>

#include "common.h"

namespace m3d {

constexpr int NP_BLOCK = 256;
constexpr int NP_GRID_CAP = 2048;          // 2048 x 256 threads, then grid-stride
constexpr int NP_MAX_PASSES = 3;
constexpr int NP_MAX_BINS = 2048;
constexpr int NP_SEL = 4;                  // s[lo1], s[lo1 + 1], s[lo99], s[lo99 + 1]
constexpr int NP_HIST_WORDS = NP_SEL * NP_MAX_BINS;
constexpr int NP_PARTS = 5;                // below, above, sum, sum of squares, non-finite
constexpr int NP_TILE = 64;
constexpr int NP_LEVELS = 65536;

enum { NP_U8 = 0, NP_U16 = 1, NP_F32 = 2 };

// Selection state after each digit pass, per order statistic: the digits found
// so far (bits at and above the pass's shift), the 0-based rank still wanted
// among the keys that share them, and the first statistic with the same prefix
// (statistics that share a prefix share its histogram).
struct NpState {
    uint32_t prefix[NP_SEL];
    uint32_t need[NP_SEL];
    uint32_t slot[NP_SEL];
    uint32_t pad[NP_SEL];
};

struct NpRanks {
    uint32_t k[NP_SEL];
    double gamma[2];
};

struct NpPlan {
    int passes;
    int shift[NP_MAX_PASSES];
    int width[NP_MAX_PASSES];
};

static NpPlan np_plan(int dtype) {
    if (dtype == NP_U8) return NpPlan{1, {0, 0, 0}, {8, 0, 0}};
    if (dtype == NP_U16) return NpPlan{2, {8, 0, 0}, {8, 8, 0}};
    return NpPlan{3, {21, 10, 0}, {11, 11, 10}};
}

__device__ __forceinline__ uint32_t np_key(uint8_t x) { return x; }
__device__ __forceinline__ uint32_t np_key(uint16_t x) { return x; }
// unsigned order of the keys == numeric order of the floats (-0 below +0)
__device__ __forceinline__ uint32_t np_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ double np_key_value(uint32_t key, int dtype) {
    if (dtype != NP_F32) return (double)key;
    return (double)__uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// f(element) over raw[0, n): 16-byte loads over the aligned body, the fewer
// than 2 x 16 / sizeof(T) elements before and after it one per thread.  The
// trip count is the same for every thread of the grid's block (f may use wave
// ballots); f gets live = false where a thread has no element.
template <typename T, typename F>
__device__ __forceinline__ void np_for_each(const T* __restrict__ raw, int64_t n, F&& f) {
    constexpr int E = 16 / (int)sizeof(T);
    const uintptr_t a = reinterpret_cast<uintptr_t>(raw);
    int64_t head = (int64_t)(((16 - (a & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    const int64_t nvec = (n - head) / E;
    const uint4* v = reinterpret_cast<const uint4*>(raw + head);
    const int64_t stride = (int64_t)gridDim.x * NP_BLOCK;
    for (int64_t i0 = (int64_t)blockIdx.x * NP_BLOCK; i0 < nvec; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < nvec;
        T e[E];
        if (live) {
            const uint4 q = v[i];
            memcpy(e, &q, 16);
        } else {
            memset(e, 0, 16);
        }
#pragma unroll
        for (int j = 0; j < E; ++j) f(e[j], live);
    }
    const int64_t tail0 = head + nvec * E;
    const int64_t rest = head + (n - tail0);              // < 2 E <= 32
    if (blockIdx.x == 0 && threadIdx.x < 64) {            // one whole wave
        const int64_t t = threadIdx.x;
        const bool live = t < rest;
        T x;
        memset(&x, 0, sizeof(T));
        if (live) x = raw[t < head ? t : tail0 + (t - head)];
        f(x, live);
    }
}

// LDS histograms of the pass's digit, one per distinct prefix among the four
// statistics, over the keys that share that prefix; a wave's adds to its
// first live lane's bin are aggregated (readfirstlane + ballot, as topk.hip): a
// volume's background level puts most of a wave into one bin.
template <typename T>
__global__ __launch_bounds__(NP_BLOCK) void np_hist_kernel(const T* __restrict__ raw, int64_t n,
                                                           const NpState* __restrict__ st,
                                                           uint32_t* __restrict__ hists, int pass, int shift,
                                                           int width, int hsh) {
    __shared__ uint32_t lh[NP_HIST_WORDS];
    const int nb = 1 << width;
    for (int b = threadIdx.x; b < NP_SEL * nb; b += NP_BLOCK) lh[b] = 0;
    NpState cur{};                                     // pass 0: no prefix yet, every statistic on slot 0
    if (pass) cur = st[pass];
    __syncthreads();
    const uint32_t dmask = (uint32_t)nb - 1;
    const int lane = threadIdx.x & 63;
    np_for_each(raw, n, [&](T x, bool live) {
        const uint32_t key = np_key(x);
        int sel = -1;
        if (!pass) {
            sel = 0;
        } else {
#pragma unroll
            for (int j = 0; j < NP_SEL; ++j)
                if (cur.slot[j] == (uint32_t)j && (key >> hsh) == (cur.prefix[j] >> hsh)) sel = j;
        }
        live = live && sel >= 0;
        const uint32_t bin = (uint32_t)(sel < 0 ? 0 : sel) * (uint32_t)nb + ((key >> shift) & dmask);
#pragma unroll
        for (int round = 0; round < 1; ++round) {
            const uint64_t act = __ballot(live);
            if (!act) break;
            const int leader = __ffsll((long long)act) - 1;
            const uint32_t lb = (uint32_t)__shfl((int)bin, leader);
            const uint64_t same = __ballot(live && bin == lb);
            if (lane == leader) atomicAdd(&lh[lb], (uint32_t)__popcll(same));
            if (live && bin == lb) live = false;
        }
        if (live) atomicAdd(&lh[bin], 1u);
    });
    __syncthreads();
    uint32_t* gh = hists + (size_t)pass * NP_HIST_WORDS;
    for (int b = threadIdx.x; b < NP_SEL * nb; b += NP_BLOCK)
        if (lh[b]) atomicAdd(&gh[b], lh[b]);
}

// One 256-thread block, wave j for statistic j: the smallest digit whose
// cumulative count passes the wanted rank (an inclusive scan over the lanes,
// each owning nb / 64 bins), written to st[pass + 1].  After the last pass
// thread 0 decodes the four keys and forms p1 and p99 (numpy's two-branch lerp
// in fp64) into stats[0], stats[1].
__global__ __launch_bounds__(NP_BLOCK) void np_state_kernel(const uint32_t* __restrict__ hists, int pass, int last,
                                                            int shift, int width, NpRanks rk, int dtype,
                                                            NpState* __restrict__ st, double* __restrict__ stats) {
    __shared__ NpState nxt;
    const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nb = 1 << width;
    const uint32_t prefix = pass ? st[pass].prefix[j] : 0u;
    const uint32_t need = pass ? st[pass].need[j] : rk.k[j];
    const uint32_t slot = pass ? st[pass].slot[j] : 0u;
    const uint32_t* h = hists + (size_t)pass * NP_HIST_WORDS + (size_t)slot * nb;
    const int per = nb / 64;
    uint32_t sum = 0;
    for (int b = lane * per; b < (lane + 1) * per; ++b) sum += h[b];
    uint32_t incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += v;
    }
    const uint32_t before = incl - sum;
    if (before <= need && need < incl) {
        uint32_t c = before;
        for (int b = lane * per; b < (lane + 1) * per; ++b) {
            if (need < c + h[b]) {
                nxt.prefix[j] = prefix | ((uint32_t)b << shift);
                nxt.need[j] = need - c;
                break;
            }
            c += h[b];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int a = 0; a < NP_SEL; ++a) {
            uint32_t s = (uint32_t)a;
            for (int b = a - 1; b >= 0; --b)
                if (nxt.prefix[b] == nxt.prefix[a]) s = (uint32_t)b;
            nxt.slot[a] = s;
            nxt.pad[a] = 0;
        }
        st[pass + 1] = nxt;
        if (last) {
            for (int q = 0; q < 2; ++q) {
                const double a = np_key_value(nxt.prefix[2 * q], dtype);
                const double b = np_key_value(nxt.prefix[2 * q + 1], dtype);
                const double g = rk.gamma[q];
                stats[q] = g < 0.5 ? a + (b - a) * g : b - (b - a) * (1.0 - g);
            }
        }
    }
}

__device__ __forceinline__ double np_clip(double x, double lo, double hi) {
    return x < lo ? lo : (x > hi ? hi : x);
}

// Fold five 8-byte words per thread over the block in a fixed (tree) order;
// the block's sums land in thread 0's acc.
template <typename A>
__device__ __forceinline__ void np_block_fold(A (&acc)[NP_PARTS], A (*red)[NP_BLOCK]) {
    for (int k = 0; k < NP_PARTS; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int off = NP_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int k = 0; k < NP_PARTS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
        __syncthreads();
    }
    for (int k = 0; k < NP_PARTS; ++k) acc[k] = red[k][0];
}

// The block's partial sums of the clipped volume into parts[k * NP_GRID_CAP +
// block].  Integer inputs: exact 64-bit integers -- the voxels below p1 and
// above p99 are counted, the others add x - c and (x - c)^2 with c = floor(p1).
template <typename T>
__global__ __launch_bounds__(NP_BLOCK) void np_sums_int_kernel(const T* __restrict__ raw, int64_t n,
                                                               const double* __restrict__ stats,
                                                               uint64_t* __restrict__ parts) {
    __shared__ uint64_t red[NP_PARTS][NP_BLOCK];
    const double p1 = stats[0], p99 = stats[1];
    const int64_t c = (int64_t)floor(p1);
    uint64_t acc[NP_PARTS] = {0, 0, 0, 0, 0};
    np_for_each(raw, n, [&](T x, bool live) {
        if (!live) return;
        const double v = (double)x;
        if (v < p1) {
            acc[0] += 1;
        } else if (v > p99) {
            acc[1] += 1;
        } else {
            const uint64_t d = (uint64_t)((int64_t)x - c);
            acc[2] += d;
            acc[3] += d * d;
        }
    });
    np_block_fold(acc, red);
    if (threadIdx.x == 0)
        for (int k = 0; k < NP_PARTS; ++k) parts[(size_t)k * NP_GRID_CAP + blockIdx.x] = acc[k];
}

// float32: fp64 sums of d = clip(x) - p1 and d^2 (the pivot keeps the
// cancellation of the variance relative to the clip range), and the count of
// non-finite inputs.
__global__ __launch_bounds__(NP_BLOCK) void np_sums_f32_kernel(const float* __restrict__ raw, int64_t n,
                                                               const double* __restrict__ stats,
                                                               double* __restrict__ parts) {
    __shared__ double red[NP_PARTS][NP_BLOCK];
    const double p1 = stats[0], p99 = stats[1];
    double acc[NP_PARTS] = {0, 0, 0, 0, 0};
    np_for_each(raw, n, [&](float x, bool live) {
        if (!live) return;
        const double d = np_clip((double)x, p1, p99) - p1;
        acc[2] += d;
        acc[3] += d * d;
        if (!isfinite(x)) acc[4] += 1.0;
    });
    np_block_fold(acc, red);
    if (threadIdx.x == 0)
        for (int k = 0; k < NP_PARTS; ++k) parts[(size_t)k * NP_GRID_CAP + blockIdx.x] = acc[k];
}

// One block: the blocks' partials in block order (thread t takes t, t + 256,
// ...), then one thread forms mean and population std in fp64.
template <typename A>
__global__ __launch_bounds__(NP_BLOCK) void np_final_kernel(const A* __restrict__ parts, int nblocks, int64_t n,
                                                            double* __restrict__ stats) {
    __shared__ A red[NP_PARTS][NP_BLOCK];
    A acc[NP_PARTS];
    for (int k = 0; k < NP_PARTS; ++k) {
        acc[k] = 0;
        for (int b = threadIdx.x; b < nblocks; b += NP_BLOCK) acc[k] += parts[(size_t)k * NP_GRID_CAP + b];
    }
    np_block_fold(acc, red);
    if (threadIdx.x != 0) return;
    const double p1 = stats[0], p99 = stats[1], dn = (double)n;
    double c, m, q;
    if constexpr (std::is_integral<A>::value) {                          // uint64_t: the integer inputs
        c = floor(p1);
        const double dlo = p1 - c, dhi = p99 - c, nb = (double)acc[0], na = (double)acc[1];
        m = (nb * dlo + na * dhi + (double)acc[2]) / dn;
        q = (nb * dlo * dlo + na * dhi * dhi + (double)acc[3]) / dn;
    } else {
        c = p1;
        m = (double)acc[2] / dn;
        q = (double)acc[3] / dn;
    }
    const double var = q - m * m;
    stats[2] = c + m;
    stats[3] = var > 0.0 ? sqrt(var) : 0.0;
    stats[4] = (double)acc[4];
    stats[5] = 0.0;
}

__device__ __forceinline__ float np_value(double x, double p1, double p99, double mean, double sd) {
    const double v = np_clip(x, p1, p99) - mean;
    const double y = sd > 0.0 ? v / sd : v;
    return (float)tanh(0.5 * y);
}

__global__ __launch_bounds__(NP_BLOCK) void np_table_kernel(const double* __restrict__ stats, int levels,
                                                            float* __restrict__ table) {
    const int l = blockIdx.x * NP_BLOCK + threadIdx.x;
    if (l < levels) table[l] = np_value((double)l, stats[0], stats[1], stats[2], stats[3]);
}

template <typename T>
struct NpMap {
    const float* table;
    double p1, p99, mean, sd;
    __device__ __forceinline__ NpMap(const double* stats, const float* t)
        : table(t), p1(stats[0]), p99(stats[1]), mean(stats[2]), sd(stats[3]) {}
    __device__ __forceinline__ float operator()(T x) const {
        if constexpr (sizeof(T) == 4) return np_value((double)x, p1, p99, mean, sd);
        else return table[x];
    }
};

// (Z,Y,X) -> [Y,X,Z]: per y, tiles of up to 64 x by 64 z through LDS; the
// tile's elements are dealt to the threads in run order on both sides, so the
// reads run along X and the writes along Z whatever the extents (a tile that
// spans all of Z writes one contiguous stretch).
template <typename T>
__global__ __launch_bounds__(NP_BLOCK) void np_apply_tr_kernel(const T* __restrict__ raw, int Z, int Y, int X,
                                                               const double* __restrict__ stats,
                                                               const float* __restrict__ table,
                                                               float* __restrict__ out) {
    __shared__ float tile[NP_TILE][NP_TILE + 1];                  // [z][x], padded
    const NpMap<T> map(stats, table);
    const int tx = (X + NP_TILE - 1) / NP_TILE, tz = (Z + NP_TILE - 1) / NP_TILE;
    const int64_t ntiles = (int64_t)Y * tx * tz;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int z0 = (int)(t % tz) * NP_TILE;
        const int x0 = (int)((t / tz) % tx) * NP_TILE;
        const int y = (int)(t / ((int64_t)tz * tx));
        const int xl = X - x0 < NP_TILE ? X - x0 : NP_TILE;
        const int zl = Z - z0 < NP_TILE ? Z - z0 : NP_TILE;
        const int cnt = xl * zl;
        for (int i = threadIdx.x; i < cnt; i += NP_BLOCK) {
            const int r = i / xl, c = i - r * xl;
            tile[r][c] = map(raw[((int64_t)(z0 + r) * Y + y) * X + (x0 + c)]);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += NP_BLOCK) {
            const int c = i / zl, r = i - c * zl;
            out[((int64_t)y * X + (x0 + c)) * Z + (z0 + r)] = tile[r][c];
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(NP_BLOCK) void np_apply_flat_kernel(const T* __restrict__ raw, int64_t n,
                                                                 const double* __restrict__ stats,
                                                                 const float* __restrict__ table,
                                                                 float* __restrict__ out) {
    const NpMap<T> map(stats, table);
    const int64_t stride = (int64_t)gridDim.x * NP_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * NP_BLOCK + threadIdx.x; i < n; i += stride) out[i] = map(raw[i]);
}

struct NpWs {
    uint32_t* hists;
    NpState* st;
    void* parts;
    float* table;
    size_t bytes;
};

static NpWs np_ws(void* base) {
    NpWs w{};
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t b) {
        size_t o = off;
        off += (b + 255) & ~(size_t)255;
        return p ? p + o : nullptr;
    };
    w.hists = (uint32_t*)take(sizeof(uint32_t) * NP_MAX_PASSES * NP_HIST_WORDS);
    w.st = (NpState*)take(sizeof(NpState) * (NP_MAX_PASSES + 1));
    w.parts = take(sizeof(uint64_t) * NP_PARTS * NP_GRID_CAP);
    w.table = (float*)take(sizeof(float) * NP_LEVELS);
    w.bytes = off;
    return w;
}

static int np_check_volume(const char* who, int64_t a, int64_t b, int64_t c, const char* names) {
    if (a <= 0 || b <= 0 || c <= 0) {
        set_error("%s: %s must be positive", who, names);
        return M3D_EINVAL;
    }
    if (a > 0x7FFFFFFF / b || a * b > 0x7FFFFFFF / c) {
        set_error("%s: the voxel count must fit 31 bits", who);
        return M3D_EINVAL;
    }
    return M3D_OK;
}

template <typename T, typename A>
static int np_run(const T* raw, int dtype, int64_t Z, int64_t Y, int64_t X, int transpose, float* out, double* stats,
                  const NpWs& w, hipStream_t s) {
    const int64_t n = Z * Y * X;
    const NpPlan plan = np_plan(dtype);
    // numpy's `linear` method: v = q / 100 (n - 1), lo = floor(v), g = v - lo
    NpRanks rk{};
    const double qs[2] = {1.0 / 100.0, 99.0 / 100.0};
    for (int q = 0; q < 2; ++q) {
        const double v = qs[q] * (double)(n - 1);
        const double lo = floor(v);
        rk.k[2 * q] = (uint32_t)lo;
        rk.k[2 * q + 1] = (uint32_t)((int64_t)lo + 1 < n ? (int64_t)lo + 1 : n - 1);
        rk.gamma[q] = v - lo;
    }
    if (hipMemsetAsync(w.hists, 0, sizeof(uint32_t) * NP_MAX_PASSES * NP_HIST_WORDS, s) != hipSuccess)
        return check_launch("normalize_image: memset");
    // four 16-byte loads per thread, then the cap: a block's LDS histograms are zeroed and flushed once
    const int64_t vecs = (n * (int64_t)sizeof(T) + 15) / 16;
    const unsigned grid = grid_for((vecs + 3) / 4, NP_BLOCK, NP_GRID_CAP);
    for (int p = 0; p < plan.passes; ++p) {
        const int hsh = p ? plan.shift[p - 1] : 32;
        hipLaunchKernelGGL(np_hist_kernel<T>, dim3(grid), dim3(NP_BLOCK), 0, s, raw, n, w.st, w.hists, p,
                           plan.shift[p], plan.width[p], hsh);
        hipLaunchKernelGGL(np_state_kernel, dim3(1), dim3(NP_BLOCK), 0, s, w.hists, p, p == plan.passes - 1 ? 1 : 0,
                           plan.shift[p], plan.width[p], rk, dtype, w.st, stats);
        if (int rc = check_launch("np_hist_kernel")) return rc;
    }
    A* parts = static_cast<A*>(w.parts);
    if constexpr (sizeof(T) == 4)
        hipLaunchKernelGGL(np_sums_f32_kernel, dim3(grid), dim3(NP_BLOCK), 0, s, raw, n, stats, parts);
    else
        hipLaunchKernelGGL(np_sums_int_kernel<T>, dim3(grid), dim3(NP_BLOCK), 0, s, raw, n, stats, parts);
    hipLaunchKernelGGL(np_final_kernel<A>, dim3(1), dim3(NP_BLOCK), 0, s, parts, (int)grid, n, stats);
    if (int rc = check_launch("np_sums_kernel")) return rc;
    if constexpr (sizeof(T) != 4) {
        const int levels = 1 << (8 * (int)sizeof(T));
        hipLaunchKernelGGL(np_table_kernel, dim3(grid_for(levels, NP_BLOCK)), dim3(NP_BLOCK), 0, s, stats, levels,
                           w.table);
    }
    if (transpose) {
        const int64_t ntiles = Y * ((X + NP_TILE - 1) / NP_TILE) * ((Z + NP_TILE - 1) / NP_TILE);
        hipLaunchKernelGGL(np_apply_tr_kernel<T>, dim3(grid_for(ntiles, 1, NP_GRID_CAP)), dim3(NP_BLOCK), 0, s, raw,
                           (int)Z, (int)Y, (int)X, stats, w.table, out);
    } else {
        hipLaunchKernelGGL(np_apply_flat_kernel<T>, dim3(grid_for(n, NP_BLOCK, NP_GRID_CAP)), dim3(NP_BLOCK), 0, s,
                           raw, n, stats, w.table, out);
    }
    return check_launch("np_apply_kernel");
}

// ---- augmentation -----------------------------------------------------------

struct Philox4 {
    uint32_t r[4];
};

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between them
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// 53 random bits -> [0, 1)
__device__ __forceinline__ double philox_u53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

__global__ __launch_bounds__(NP_BLOCK) void aug_minmax_kernel(const float* __restrict__ in, int64_t n,
                                                              float* __restrict__ parts) {
    __shared__ float lo_s[NP_BLOCK], hi_s[NP_BLOCK];
    float lo = in[0], hi = in[0];
    const int64_t stride = (int64_t)gridDim.x * NP_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * NP_BLOCK + threadIdx.x; i < n; i += stride) {
        const float x = in[i];
        lo = smin(lo, x);
        hi = smax(hi, x);
    }
    lo_s[threadIdx.x] = lo;
    hi_s[threadIdx.x] = hi;
    __syncthreads();
    for (int off = NP_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            lo_s[threadIdx.x] = smin(lo_s[threadIdx.x], lo_s[threadIdx.x + off]);
            hi_s[threadIdx.x] = smax(hi_s[threadIdx.x], hi_s[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = lo_s[0];
        parts[2 * blockIdx.x + 1] = hi_s[0];
    }
}

__global__ __launch_bounds__(NP_BLOCK) void aug_minmax_final_kernel(const float* __restrict__ parts, int nblocks,
                                                                    float* __restrict__ mm) {
    __shared__ float lo_s[NP_BLOCK], hi_s[NP_BLOCK];
    float lo = parts[0], hi = parts[1];
    for (int b = threadIdx.x; b < nblocks; b += NP_BLOCK) {
        lo = smin(lo, parts[2 * b]);
        hi = smax(hi, parts[2 * b + 1]);
    }
    lo_s[threadIdx.x] = lo;
    hi_s[threadIdx.x] = hi;
    __syncthreads();
    for (int off = NP_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            lo_s[threadIdx.x] = smin(lo_s[threadIdx.x], lo_s[threadIdx.x + off]);
            hi_s[threadIdx.x] = smax(hi_s[threadIdx.x], hi_s[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mm[0] = lo_s[0];
        mm[1] = hi_s[0];
    }
}

// out[h,w,d] = in[flipped (h,w,d)] (+ brightness noise, clipped to the image's
// range) (+ Gaussian noise).  The random numbers are counted by the OUTPUT
// voxel's linear index: stream 0 brightness, stream 1 Gaussian.
__global__ __launch_bounds__(NP_BLOCK) void aug_apply_kernel(const float* __restrict__ in, int H, int W, int D,
                                                             int flip, float bd, double noise_std, uint32_t seed_lo,
                                                             uint32_t seed_hi, const float* __restrict__ mm,
                                                             float* __restrict__ out) {
    const int64_t n = (int64_t)H * W * D;
    float vmin = 0.f, vmax = 0.f;
    double scale = 0.0;
    if (bd > 0.f) {
        vmin = mm[0];
        vmax = mm[1];
        scale = (double)bd * ((double)vmax - (double)vmin + 1e-6);
    }
    const int64_t stride = (int64_t)gridDim.x * NP_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * NP_BLOCK + threadIdx.x; i < n; i += stride) {
        int d = (int)(i % D);
        const int64_t t = i / D;
        int w = (int)(t % W), h = (int)(t / W);
        if (flip & 1) h = H - 1 - h;
        if (flip & 2) w = W - 1 - w;
        if (flip & 4) d = D - 1 - d;
        float v = in[((int64_t)h * W + w) * D + d];
        const uint32_t lo = (uint32_t)i, hi = (uint32_t)((uint64_t)i >> 32);
        if (bd > 0.f) {
            const Philox4 r = philox4x32_10(lo, hi, 0u, 0u, seed_lo, seed_hi);
            const float noise = (float)(-scale + 2.0 * scale * philox_u53(r.r[0], r.r[1]));
            v = smin(smax(v + noise, vmin), vmax);
        }
        if (noise_std > 0.0) {
            const Philox4 r = philox4x32_10(lo, hi, 1u, 0u, seed_lo, seed_hi);
            const double u1 = philox_u53(r.r[0], r.r[1]), u2 = philox_u53(r.r[2], r.r[3]);
            v += (float)(noise_std * sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2));
        }
        out[i] = v;
    }
}

// [H,W,D,G] bytes as R = H W rows of Dg groups of gv vectors of sizeof(V)
// bytes (without a z flip a row is one group: whole lines move)
template <typename V>
__global__ __launch_bounds__(NP_BLOCK) void flip_vec_kernel(const V* __restrict__ in, int H, int W, int64_t Dg,
                                                            int64_t gv, int flip, int64_t total, V* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * NP_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * NP_BLOCK + threadIdx.x; i < total; i += stride) {
        const int64_t g = i % gv;
        int64_t t = i / gv;
        int64_t d = t % Dg;
        t /= Dg;
        int w = (int)(t % W), h = (int)(t / W);
        if (flip & 1) h = H - 1 - h;
        if (flip & 2) w = W - 1 - w;
        if (flip & 4) d = Dg - 1 - d;
        out[(((int64_t)h * W + w) * Dg + d) * gv + g] = in[i];
    }
}

template <typename V>
static void flip_launch(const void* in, int H, int W, int64_t Dg, int64_t gbytes, int flip, void* out, hipStream_t s) {
    const int64_t gv = gbytes / (int64_t)sizeof(V);
    const int64_t total = (int64_t)H * W * Dg * gv;
    hipLaunchKernelGGL(flip_vec_kernel<V>, dim3(grid_for(total, NP_BLOCK, NP_GRID_CAP)), dim3(NP_BLOCK), 0, s,
                       static_cast<const V*>(in), H, W, Dg, gv, flip, total, static_cast<V*>(out));
}

__global__ void flip_boxes_kernel(const float* __restrict__ in, int64_t N, float H, float W, float D, int flip,
                                  float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float b[6];
    for (int k = 0; k < 6; ++k) b[k] = in[i * 6 + k];
    const float ext[3] = {H, W, D};
    for (int a = 0; a < 3; ++a)
        if (flip & (1 << a)) {
            const float lo = ext[a] - b[a + 3], hi = ext[a] - b[a];
            b[a] = lo;
            b[a + 3] = hi;
        }
    for (int k = 0; k < 6; ++k) out[i * 6 + k] = b[k];
}

}  // namespace m3d

using namespace m3d;

extern "C" size_t m3d_normalize_image_workspace_bytes(int64_t Z, int64_t Y, int64_t X, int32_t dtype) {
    if (Z <= 0 || Y <= 0 || X <= 0 || dtype < NP_U8 || dtype > NP_F32) return 0;
    return np_ws(nullptr).bytes;
}

extern "C" int m3d_normalize_image(const void* raw, int32_t dtype, int64_t Z, int64_t Y, int64_t X, int32_t transpose,
                                   float* out, double* stats, void* workspace, size_t ws_bytes, m3d_stream_t s) {
    if (int rc = np_check_volume("normalize_image", Z, Y, X, "Z, Y and X")) return rc;
    if (dtype < NP_U8 || dtype > NP_F32)
        return einval("normalize_image: dtype must be M3D_DTYPE_U8, M3D_DTYPE_U16 or M3D_DTYPE_F32");
    if (transpose != 0 && transpose != 1) return einval("normalize_image: transpose must be 0 or 1");
    if (raw == nullptr || out == nullptr || stats == nullptr) return einval("normalize_image: NULL pointer");
    if (raw == (const void*)out) return einval("normalize_image: raw and out must not be the same buffer");
    const size_t esz = dtype == NP_U8 ? 1 : (dtype == NP_U16 ? 2 : 4);
    if (reinterpret_cast<uintptr_t>(raw) % esz || reinterpret_cast<uintptr_t>(out) % 4 ||
        reinterpret_cast<uintptr_t>(stats) % 8)
        return einval("normalize_image: misaligned pointer");
    const NpWs need = np_ws(nullptr);
    if (workspace == nullptr || ws_bytes < need.bytes) return einval("normalize_image: workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return einval("normalize_image: misaligned workspace");
    const NpWs w = np_ws(workspace);
    if (dtype == NP_U8)
        return np_run<uint8_t, uint64_t>(static_cast<const uint8_t*>(raw), dtype, Z, Y, X, transpose, out, stats, w,
                                         st(s));
    if (dtype == NP_U16)
        return np_run<uint16_t, uint64_t>(static_cast<const uint16_t*>(raw), dtype, Z, Y, X, transpose, out, stats, w,
                                          st(s));
    return np_run<float, double>(static_cast<const float*>(raw), dtype, Z, Y, X, transpose, out, stats, w, st(s));
}

extern "C" size_t m3d_augment_image_workspace_bytes(int64_t H, int64_t W, int64_t D) {
    if (H <= 0 || W <= 0 || D <= 0) return 0;
    return sizeof(float) * (2 * NP_GRID_CAP + 2);
}

extern "C" int m3d_augment_image(const float* in, int64_t H, int64_t W, int64_t D, int32_t flip_mask,
                                 float brightness_delta, double noise_std, uint32_t seed_lo, uint32_t seed_hi,
                                 float* out, void* workspace, size_t ws_bytes, m3d_stream_t s) {
    if (int rc = np_check_volume("augment_image", H, W, D, "H, W and D")) return rc;
    if (flip_mask < 0 || flip_mask > 7) return einval("augment_image: flip_mask must be in [0, 7]");
    if (in == nullptr || out == nullptr) return einval("augment_image: NULL pointer");
    if (in == out) return einval("augment_image: in and out must not be the same buffer");
    const bool bright = brightness_delta > 0.f;
    float* ws = static_cast<float*>(workspace);
    if (bright && (workspace == nullptr || ws_bytes < m3d_augment_image_workspace_bytes(H, W, D)))
        return einval("augment_image: workspace too small");
    if (bright && reinterpret_cast<uintptr_t>(workspace) % 4) return einval("augment_image: misaligned workspace");
    const int64_t n = H * W * D;
    const unsigned grid = grid_for(n, NP_BLOCK, NP_GRID_CAP);
    float* mm = bright ? ws + 2 * NP_GRID_CAP : nullptr;
    if (bright) {                                   // the reduction pass only when the leg is on
        hipLaunchKernelGGL(aug_minmax_kernel, dim3(grid), dim3(NP_BLOCK), 0, st(s), in, n, ws);
        hipLaunchKernelGGL(aug_minmax_final_kernel, dim3(1), dim3(NP_BLOCK), 0, st(s), ws, (int)grid, mm);
        if (int rc = check_launch("aug_minmax_kernel")) return rc;
    }
    hipLaunchKernelGGL(aug_apply_kernel, dim3(grid), dim3(NP_BLOCK), 0, st(s), in, (int)H, (int)W, (int)D,
                       (int)flip_mask, bright ? brightness_delta : 0.f, noise_std > 0.0 ? noise_std : 0.0, seed_lo,
                       seed_hi, mm, out);
    return check_launch("aug_apply_kernel");
}

extern "C" int m3d_flip_masks_u8(const uint8_t* in, int64_t H, int64_t W, int64_t D, int64_t G, int32_t flip_mask,
                                 uint8_t* out, m3d_stream_t s) {
    if (int rc = np_check_volume("flip_masks_u8", H, W, D, "H, W and D")) return rc;
    if (G <= 0 || G > 0x7FFFFFFF) return einval("flip_masks_u8: G must be positive and below 2^31");
    if (flip_mask < 0 || flip_mask > 7) return einval("flip_masks_u8: flip_mask must be in [0, 7]");
    if (in == nullptr || out == nullptr) return einval("flip_masks_u8: NULL pointer");
    if (in == out) return einval("flip_masks_u8: in and out must not be the same buffer");
    // a z flip reverses G-byte groups; without it a row's D G bytes move as one group
    const int64_t Dg = (flip_mask & 4) ? D : 1;
    const int64_t gbytes = (flip_mask & 4) ? G : D * G;
    const uintptr_t al = reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | (uintptr_t)gbytes;
    if (al % 16 == 0) flip_launch<uint4>(in, (int)H, (int)W, Dg, gbytes, flip_mask, out, st(s));
    else if (al % 8 == 0) flip_launch<uint2>(in, (int)H, (int)W, Dg, gbytes, flip_mask, out, st(s));
    else if (al % 4 == 0) flip_launch<uint32_t>(in, (int)H, (int)W, Dg, gbytes, flip_mask, out, st(s));
    else if (al % 2 == 0) flip_launch<uint16_t>(in, (int)H, (int)W, Dg, gbytes, flip_mask, out, st(s));
    else flip_launch<uint8_t>(in, (int)H, (int)W, Dg, gbytes, flip_mask, out, st(s));
    return check_launch("flip_vec_kernel");
}

extern "C" int m3d_flip_boxes(const float* in, int64_t N, int64_t H, int64_t W, int64_t D, int32_t flip_mask,
                              float* out, m3d_stream_t s) {
    if (H <= 0 || W <= 0 || D <= 0) return einval("flip_boxes: H, W and D must be positive");
    if (H > (1 << 24) || W > (1 << 24) || D > (1 << 24)) return einval("flip_boxes: H, W and D must be exact floats");
    if (N < 0 || N > 0x7FFFFFFF / 6) return einval("flip_boxes: N must be in [0, 2^31 / 6]");
    if (flip_mask < 0 || flip_mask > 7) return einval("flip_boxes: flip_mask must be in [0, 7]");
    if (N == 0) return M3D_OK;
    if (in == nullptr || out == nullptr) return einval("flip_boxes: NULL pointer");
    if (in == out) return einval("flip_boxes: in and out must not be the same buffer");
    hipLaunchKernelGGL(flip_boxes_kernel, dim3(grid_for(N, 64)), dim3(64), 0, st(s), in, N, (float)H, (float)W,
                       (float)D, (int)flip_mask, out);
    return check_launch("flip_boxes_kernel");
}
