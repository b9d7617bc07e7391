// The stored head targets' narrow forms on the device (include/m3d.h, "Stored
// head targets"): float32 -> packed bits / float16 on the way to disk, and
// packed bits / float16 -> a gathered float32 batch on the way back, plus the
// per-row set-bit counts the generator filters on.  All five are streaming
// passes: no LDS staging, no atomics, every output element written once.
#include "common.h"

#include <hip/hip_fp16.h>

namespace m3d {
namespace {

constexpr int HS_BLOCK = 256;
constexpr int HS_UNROLL_LOG2 = 2;
constexpr int HS_UNROLL = 1 << HS_UNROLL_LOG2;          // independent 16-byte loads in flight per thread

__device__ __forceinline__ uint32_t gt_half_bits(const float4& v) {
    // first element in the highest bit (np.packbits' big-endian order); NaN > 0.5f is false
    return (v.x > 0.5f ? 8u : 0u) | (v.y > 0.5f ? 4u : 0u) | (v.z > 0.5f ? 2u : 0u) | (v.w > 0.5f ? 1u : 0u);
}

// One output byte per thread: lane l of a wave writes byte base + l, from the
// two 16-byte loads at x + 8 (base + l).  The thread that owns the last,
// partial byte reads its n % 8 elements one by one.
__global__ __launch_bounds__(HS_BLOCK) void pack_bits_kernel(const float* __restrict__ x, int64_t n,
                                                             uint8_t* __restrict__ bits) {
    const int64_t nfull = n >> 3;
    const int rem = (int)(n & 7);
    const int64_t base = (int64_t)blockIdx.x * (HS_BLOCK * HS_UNROLL) + threadIdx.x;
    float4 lo[HS_UNROLL], hi[HS_UNROLL];
#pragma unroll
    for (int j = 0; j < HS_UNROLL; ++j) {
        const int64_t g = base + (int64_t)j * HS_BLOCK;
        if (g < nfull) {
            const float4* p = reinterpret_cast<const float4*>(x + 8 * g);
            lo[j] = p[0];
            hi[j] = p[1];
        }
    }
#pragma unroll
    for (int j = 0; j < HS_UNROLL; ++j) {
        const int64_t g = base + (int64_t)j * HS_BLOCK;
        if (g < nfull) {
            bits[g] = (uint8_t)((gt_half_bits(lo[j]) << 4) | gt_half_bits(hi[j]));
        } else if (g == nfull && rem) {
            uint32_t b = 0;
            for (int e = 0; e < rem; ++e) b |= (x[8 * g + e] > 0.5f ? 0x80u : 0u) >> e;
            bits[g] = (uint8_t)b;
        }
    }
}

// Four elements per thread: one 16-byte load, one 8-byte store, both lane-contiguous.
__global__ __launch_bounds__(HS_BLOCK) void f32_to_f16_kernel(const float* __restrict__ x, int64_t n,
                                                              uint16_t* __restrict__ h) {
    const int64_t nfull = n >> 2;
    const int rem = (int)(n & 3);
    const int64_t base = (int64_t)blockIdx.x * (HS_BLOCK * HS_UNROLL) + threadIdx.x;
    float4 v[HS_UNROLL];
#pragma unroll
    for (int j = 0; j < HS_UNROLL; ++j) {
        const int64_t g = base + (int64_t)j * HS_BLOCK;
        if (g < nfull) v[j] = reinterpret_cast<const float4*>(x)[g];
    }
#pragma unroll
    for (int j = 0; j < HS_UNROLL; ++j) {
        const int64_t g = base + (int64_t)j * HS_BLOCK;
        if (g < nfull) {
            // v_cvt_f16_f32: round to nearest even, half subnormals kept, overflow to inf
            const uint32_t a = __half_as_ushort(__float2half_rn(v[j].x));
            const uint32_t b = __half_as_ushort(__float2half_rn(v[j].y));
            const uint32_t c = __half_as_ushort(__float2half_rn(v[j].z));
            const uint32_t d = __half_as_ushort(__float2half_rn(v[j].w));
            reinterpret_cast<uint2*>(h)[g] = make_uint2(a | (b << 16), c | (d << 16));
        } else if (g == nfull && rem) {
            for (int e = 0; e < rem; ++e) h[4 * g + e] = __half_as_ushort(__float2half_rn(x[4 * g + e]));
        }
    }
}

// One workgroup per row.  The row's bit range [r row_bits, (r + 1) row_bits) is
// walked in aligned 32-bit words of the stream; a byte-swapped word has stream
// bit k of the word at bit 31 - k, so the row's first and last word are masked
// by shifts.  The last word of the whole array may end past total_bytes: it is
// assembled from the bytes that exist.
__global__ __launch_bounds__(HS_BLOCK) void bits_row_counts_kernel(const uint8_t* __restrict__ bits, int64_t rows,
                                                                   int64_t row_bits, int64_t total_bytes,
                                                                   int32_t* __restrict__ counts) {
    const int64_t r = blockIdx.x;
    const int64_t b0 = r * row_bits, b1 = b0 + row_bits;
    const int64_t w0 = b0 >> 5, w1 = (b1 - 1) >> 5;
    int32_t acc = 0;
    for (int64_t w = w0 + threadIdx.x; w <= w1; w += HS_BLOCK) {
        uint32_t v;
        if (4 * w + 4 <= total_bytes) {
            v = __builtin_bswap32(reinterpret_cast<const uint32_t*>(bits)[w]);
        } else {
            v = 0;
            for (int e = 0; e < 4; ++e)
                if (4 * w + e < total_bytes) v |= (uint32_t)bits[4 * w + e] << (24 - 8 * e);
        }
        if (w == w0) v &= 0xFFFFFFFFu >> (int)(b0 & 31);
        if (w == w1) {
            const int end = (int)(b1 - (w1 << 5));          // 1..32 stream bits of this word belong to the row
            if (end < 32) v &= ~(0xFFFFFFFFu >> end);
        }
        acc += __popc(v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ int32_t part[HS_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t t = 0;
#pragma unroll
        for (int i = 0; i < HS_BLOCK / 64; ++i) t += part[i];
        counts[r] = t;
    }
}

struct GatherP {
    const void* src = nullptr;
    int64_t R = 0;
    int32_t S0 = 0, S1 = 0, S2 = 0, C = 0;
    const int32_t* sel = nullptr;
    const int32_t* i0 = nullptr;
    const int32_t* i1 = nullptr;
    const int32_t* i2 = nullptr;
    uint32_t Q = 0;          // T_out * M0 * M1 output rows of M2 * C floats
    uint32_t M0 = 0, M1 = 0;
    uint32_t I = 0;          // vectors per output row: M2 * (C / VEC)
    uint32_t CV = 0;         // vectors per position: C / VEC
    int32_t cvs = -1;        // log2(CV) where CV is a power of two (a shift for the division), else -1
    uint32_t rpb = 1;        // output rows per workgroup and step (1 when I >= HS_BLOCK; then blockIdx.y walks the row)
    uint32_t ujs = 0;        // log2 of a thread's steps along the row; its other HS_UNROLL >> ujs steps are further rows
    float* out = nullptr;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// out[t, a, b, c, k] = src[sel[t], i0[a], i1[b], i2[c], k] as float32, VEC
// consecutive k per thread and step (VEC = 4 needs C % 4 == 0: the four source
// elements are then one nibble of a byte, or one 8-byte group of halves).
// Lanes run along the output's innermost axes, so the stores of a wave are
// contiguous.  A thread makes HS_UNROLL steps: 1 << ujs of them HS_BLOCK vectors
// apart along the row (rows of at least HS_BLOCK vectors, rpb == 1), the others
// on further rows, rpb rows apart, in three passes -- table lookups, source loads, stores -- so that the
// dependent loads of its steps overlap: with one step per thread the pass ran
// at the latency of that chain, not at the memory's rate.
// WIDE (rpb == 1): a step's row is the same for the whole workgroup, so its
// decomposition into (t, a, b) and the three lookups that follow stay scalar.
template <bool BITS, int VEC, bool WIDE>
__global__ __launch_bounds__(HS_BLOCK) void unpack_gather_kernel(const GatherP p) {
    uint32_t rl = 0, j0 = threadIdx.x;
    if constexpr (!WIDE) {
        rl = threadIdx.x / p.I;
        j0 = threadIdx.x - rl * p.I;
    }
    // every load below is unconditional, from an index clamped into range, so that the
    // compiler can issue the steps' loads together; a dead step's results are dropped
    bool live[HS_UNROLL];
    int64_t o[HS_UNROLL];
    uint32_t kq[HS_UNROLL];
    int32_t r[HS_UNROLL], y[HS_UNROLL], x[HS_UNROLL], z[HS_UNROLL];
#pragma unroll
    for (int u = 0; u < HS_UNROLL; ++u) {
        uint32_t q, j;
        const uint32_t uj = u & ((1u << p.ujs) - 1u), uq = u >> p.ujs;       // the step's place along the row / in rows
        if constexpr (WIDE) {
            q = (blockIdx.x << (HS_UNROLL_LOG2 - p.ujs)) + uq;
            j = ((blockIdx.y << p.ujs) + uj) * HS_BLOCK + threadIdx.x;
        } else {
            q = (blockIdx.x * HS_UNROLL + u) * p.rpb + rl;
            j = j0;
        }
        live[u] = rl < p.rpb && j < p.I && q < p.Q;
        if (!live[u]) q = 0, j = 0;
        const uint32_t ta = q / p.M1, b = q - ta * p.M1;
        const uint32_t t = ta / p.M0, a = ta - t * p.M0;
        const uint32_t c = p.cvs >= 0 ? j >> p.cvs : j / p.CV;
        kq[u] = j - c * p.CV;
        o[u] = ((int64_t)q * p.I + j) * VEC;
        r[u] = p.sel[t];
        y[u] = p.i0[a];
        x[u] = p.i1[b];
        z[u] = p.i2[c];
    }
    int64_t e0[HS_UNROLL];
    uint2 raw[HS_UNROLL];
#pragma unroll
    for (int u = 0; u < HS_UNROLL; ++u) {
        const bool have = r[u] >= 0 && r[u] < p.R;          // a padding row (or a row past the source) reads row 0
        const int64_t row = have ? r[u] : 0;
        const int64_t e = (((row * p.S0 + clampi(y[u], p.S0 - 1)) * p.S1 + clampi(x[u], p.S1 - 1)) * p.S2 +
                           clampi(z[u], p.S2 - 1)) * p.C + (int64_t)kq[u] * VEC;
        e0[u] = have ? e : -1;
        raw[u] = make_uint2(0u, 0u);
        if constexpr (BITS) raw[u].x = reinterpret_cast<const uint8_t*>(p.src)[e >> 3];
        else if constexpr (VEC == 4) raw[u] = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(p.src) + e);
        else raw[u].x = reinterpret_cast<const uint16_t*>(p.src)[e];
    }
#pragma unroll
    for (int u = 0; u < HS_UNROLL; ++u) {
        if (!live[u]) continue;
        float v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = 0.f;
        if (e0[u] >= 0) {
            if constexpr (BITS) {
                const int sh = 8 - VEC - (int)(e0[u] & 7);          // VEC = 4: e0 % 4 == 0, the nibble at 4 or 0
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] = (float)((raw[u].x >> (sh + VEC - 1 - e)) & 1u);
            } else if constexpr (VEC == 4) {
                v[0] = __half2float(__ushort_as_half((unsigned short)(raw[u].x & 0xFFFFu)));
                v[1] = __half2float(__ushort_as_half((unsigned short)(raw[u].x >> 16)));
                v[2] = __half2float(__ushort_as_half((unsigned short)(raw[u].y & 0xFFFFu)));
                v[3] = __half2float(__ushort_as_half((unsigned short)(raw[u].y >> 16)));
            } else {
                v[0] = __half2float(__ushort_as_half((unsigned short)raw[u].x));
            }
        }
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(p.out + o[u]) = make_float4(v[0], v[1], v[2], v[3]);
        else p.out[o[u]] = v[0];
    }
}

int stream_check(const char* what, const void* x, int64_t n, const void* y, size_t x_align, size_t y_align,
                 char* msg, size_t msg_len) {
    if (n < 0) {
        snprintf(msg, msg_len, "%s: n must not be negative", what);
        return einval(msg);
    }
    if (n == 0) return M3D_OK;
    if (x == nullptr || y == nullptr) {
        snprintf(msg, msg_len, "%s: NULL pointer", what);
        return einval(msg);
    }
    if ((reinterpret_cast<uintptr_t>(x) % x_align) || (reinterpret_cast<uintptr_t>(y) % y_align)) {
        snprintf(msg, msg_len, "%s: the input must be %zu-byte aligned and the output %zu-byte aligned", what,
                 x_align, y_align);
        return einval(msg);
    }
    return M3D_OK;
}

template <bool BITS>
int unpack_gather(const char* what, const void* src, int64_t R, int64_t S0, int64_t S1, int64_t S2, int64_t C,
                  const int32_t* sel, int64_t T_out, const int32_t* i0, const int32_t* i1, const int32_t* i2,
                  int64_t M0, int64_t M1, int64_t M2, float* out, hipStream_t s) {
    char msg[160];
    auto bad = [&](const char* why) {
        snprintf(msg, sizeof msg, "%s: %s", what, why);
        return einval(msg);
    };
    if (R <= 0 || S0 <= 0 || S1 <= 0 || S2 <= 0 || C <= 0) return bad("R, S0, S1, S2 and C must be positive");
    if (T_out <= 0 || M0 <= 0 || M1 <= 0 || M2 <= 0) return bad("T_out, M0, M1 and M2 must be positive");
    const int64_t lim = 0x7FFFFFFF;
    if (S0 > lim || S1 > lim || S2 > lim || C > lim || M0 > lim || M1 > lim || M2 > lim || T_out > lim)
        return bad("every extent must be below 2^31");
    if (T_out * M0 > lim || T_out * M0 * M1 > lim) return bad("T_out * M0 * M1 must be below 2^31");
    if (M2 * C > lim) return bad("M2 * C must be below 2^31");
    if (R > (INT64_MAX / 8) / S0 / S1 / S2 / C) return bad("the source has too many elements");
    if (src == nullptr || sel == nullptr || i0 == nullptr || i1 == nullptr || i2 == nullptr || out == nullptr)
        return bad("NULL pointer");
    const bool vec = C % 4 == 0;
    if (reinterpret_cast<uintptr_t>(out) % (vec ? 16 : 4)) return bad("out must be 16-byte aligned (4 when C % 4 != 0)");
    if (!BITS && reinterpret_cast<uintptr_t>(src) % (vec ? 8 : 2))
        return bad("the float16 source must be 8-byte aligned (2 when C % 4 != 0)");
    GatherP p{};
    p.src = src;
    p.R = R;
    p.S0 = (int32_t)S0, p.S1 = (int32_t)S1, p.S2 = (int32_t)S2, p.C = (int32_t)C;
    p.sel = sel, p.i0 = i0, p.i1 = i1, p.i2 = i2;
    p.Q = (uint32_t)(T_out * M0 * M1);
    p.M0 = (uint32_t)M0, p.M1 = (uint32_t)M1;
    p.CV = (uint32_t)(vec ? C / 4 : C);
    p.I = (uint32_t)(M2 * p.CV);
    if ((p.CV & (p.CV - 1)) == 0) p.cvs = __builtin_ctz(p.CV);
    p.out = out;
    dim3 grid;
    if (p.I >= HS_BLOCK) {
        p.rpb = 1;
        const uint32_t chunks = (p.I + HS_BLOCK - 1) / HS_BLOCK;
        p.ujs = chunks >= 4 ? 2 : (chunks >= 2 ? 1 : 0);
        const uint32_t uq = HS_UNROLL >> p.ujs;
        grid = dim3((p.Q + uq - 1) / uq, (chunks + (1u << p.ujs) - 1) >> p.ujs);
        if (grid.y > 65535) return bad("M2 * C is too large for one launch");
    } else {
        p.rpb = HS_BLOCK / p.I;
        grid = dim3((p.Q + p.rpb * HS_UNROLL - 1) / (p.rpb * HS_UNROLL));
    }
    const bool wide = p.rpb == 1;
    if (vec && wide) hipLaunchKernelGGL((unpack_gather_kernel<BITS, 4, true>), grid, dim3(HS_BLOCK), 0, s, p);
    else if (vec) hipLaunchKernelGGL((unpack_gather_kernel<BITS, 4, false>), grid, dim3(HS_BLOCK), 0, s, p);
    else if (wide) hipLaunchKernelGGL((unpack_gather_kernel<BITS, 1, true>), grid, dim3(HS_BLOCK), 0, s, p);
    else hipLaunchKernelGGL((unpack_gather_kernel<BITS, 1, false>), grid, dim3(HS_BLOCK), 0, s, p);
    return check_launch("unpack_gather_kernel");
}

}  // namespace
}  // namespace m3d

using namespace m3d;

extern "C" int m3d_pack_bits_f32(const float* x, int64_t n, uint8_t* bits, m3d_stream_t s) {
    char msg[160];
    if (int rc = stream_check("pack_bits_f32", x, n, bits, 16, 1, msg, sizeof msg)) return rc;
    if (n == 0) return M3D_OK;
    const int64_t nbytes = (n + 7) / 8;
    const int64_t blocks = (nbytes + HS_BLOCK * HS_UNROLL - 1) / (HS_BLOCK * HS_UNROLL);
    if (blocks > 0x7FFFFFFF) return einval("pack_bits_f32: n is too large for one launch");
    hipLaunchKernelGGL(pack_bits_kernel, dim3((unsigned)blocks), dim3(HS_BLOCK), 0, st(s), x, n, bits);
    return check_launch("pack_bits_kernel");
}

extern "C" int m3d_f32_to_f16(const float* x, int64_t n, uint16_t* h, m3d_stream_t s) {
    char msg[160];
    if (int rc = stream_check("f32_to_f16", x, n, h, 16, 8, msg, sizeof msg)) return rc;
    if (n == 0) return M3D_OK;
    const int64_t nvec = (n + 3) / 4;
    const int64_t blocks = (nvec + HS_BLOCK * HS_UNROLL - 1) / (HS_BLOCK * HS_UNROLL);
    if (blocks > 0x7FFFFFFF) return einval("f32_to_f16: n is too large for one launch");
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3((unsigned)blocks), dim3(HS_BLOCK), 0, st(s), x, n, h);
    return check_launch("f32_to_f16_kernel");
}

extern "C" int m3d_bits_row_counts(const uint8_t* bits, int64_t rows, int64_t row_bits, int32_t* counts,
                                   m3d_stream_t s) {
    if (rows < 0) return einval("bits_row_counts: rows must not be negative");
    if (row_bits <= 0 || row_bits > 0x7FFFFFFF) return einval("bits_row_counts: row_bits must be in [1, 2^31)");
    if (rows > 0x7FFFFFFF) return einval("bits_row_counts: rows must be below 2^31");
    if (rows == 0) return M3D_OK;
    if (bits == nullptr || counts == nullptr) return einval("bits_row_counts: NULL pointer");
    if (reinterpret_cast<uintptr_t>(bits) % 4 || reinterpret_cast<uintptr_t>(counts) % 4)
        return einval("bits_row_counts: bits and counts must be 4-byte aligned");
    const int64_t total_bytes = (rows * row_bits + 7) / 8;
    hipLaunchKernelGGL(bits_row_counts_kernel, dim3((unsigned)rows), dim3(HS_BLOCK), 0, st(s), bits, rows, row_bits,
                       total_bytes, counts);
    return check_launch("bits_row_counts_kernel");
}

extern "C" int m3d_unpack_gather_bits(const uint8_t* bits, int64_t R, int64_t S0, int64_t S1, int64_t S2, int64_t C,
                                      const int32_t* sel, int64_t T_out, const int32_t* i0, const int32_t* i1,
                                      const int32_t* i2, int64_t M0, int64_t M1, int64_t M2, float* out,
                                      m3d_stream_t s) {
    return unpack_gather<true>("unpack_gather_bits", bits, R, S0, S1, S2, C, sel, T_out, i0, i1, i2, M0, M1, M2, out,
                               st(s));
}

extern "C" int m3d_unpack_gather_f16(const uint16_t* h, int64_t R, int64_t S0, int64_t S1, int64_t S2, int64_t C,
                                     const int32_t* sel, int64_t T_out, const int32_t* i0, const int32_t* i1,
                                     const int32_t* i2, int64_t M0, int64_t M1, int64_t M2, float* out,
                                     m3d_stream_t s) {
    return unpack_gather<false>("unpack_gather_f16", h, R, S0, S1, S2, C, sel, T_out, i0, i1, i2, M0, M1, M2, out,
                                st(s));
}
