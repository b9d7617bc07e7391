// The one-channel 7^3 stem conv (conv1, 1 -> 64 channels, strides (2,2,1)) on
// gfx950: stem_fwd_kernel and its weight gradient stem_wgrad_kernel, both also
// on a depth slab with halo planes (ConvP::halo).  No entry point lives here:
// the direct conv entries of conv3d.hip (m3d_conv3d_fwd*, m3d_conv3d_bwd_weight*)
// ask stem_ok and call launch_stem / launch_stem_wgrad (conv_types.h).
#include "conv_types.h"

namespace m3d {

typedef float floatx4 __attribute__((ext_vector_type(4)));

// ---- the one-channel 7^3 stem: conv1 (core/models.py:242, Conv3D(64, (7,7,7),
// strides (2,2,1)) after ZeroPadding3D(3)) -------------------------------------
// The implicit GEMM's scalar loader reaches 0.27 of the f32 MFMA peak here
// (K = 343 taps of ONE channel: no channel vector to load).  This kernel keeps
// the whole K operand on chip: the 343 x 64 weights live in LDS for the life
// of a workgroup that loops over many tiles (about 4 per CU), and every wave owns one
// output column (oy, ox) x 32 z x 64 channels with its own input window (the
// 49 (ky, kx) rows x 38 z voxels, + one zero row) in its own LDS region,
// refilled from registers prefetched during the previous tile's MFMAs.  No
// barrier after the weight load: the waves of a CU run out of phase.
// K order: the two MFMA k-slots (lane halves h) walk (ky, kx) rows R = rp and
// R = rp + 25 in step, 7 taps kz each -- so a lane's window offset is
// R * 38 + kz: one add per row, the 7 taps as ds_read immediates (a
// per-tap index walk cost more issue than the MFMAs).  Row R = 49 is the
// padding (zero weights, zero window row).  Epilogue: each 32-channel
// accumulator is staged in the wave's LDS region (row stride 40 floats:
// the lane halves, 4 rows apart, land 32 banks apart) and leaves as
// row-contiguous float4s in epi_store4's order of ops (bias, z, frozen BN,
// ReLU; conv3d.hip), written out in the kernel.
// Summation order: K in the (R pair, kz) order above -- an exact f32 FMA
// chain, a different order than the implicit GEMM (parity 1e-4).
constexpr int STEM_TZ = 32;
constexpr int STEM_WZ = STEM_TZ + 6;                             // 38
constexpr int STEM_WIN = 50 * STEM_WZ;                           // 49 rows + the zero row: 1900 floats
constexpr int STEM_RP = 25;                                      // row pairs (R, R + 25)
constexpr int STEM_NP = STEM_RP * 7;                             // 175 k pairs
constexpr int STEM_PER = (49 * STEM_WZ + 63) / 64;               // window values per lane (30)
constexpr int STEM_SLD = 40;                                     // epilogue staging row stride

__global__ __launch_bounds__(512) void stem_fwd_kernel(ConvP p, Epi e, int tz_n, int64_t ntiles) {
    __shared__ float wsh[STEM_NP * 128];          // [pair][h*32+l32][nb]  (89.6 KB)
    __shared__ float win[8][STEM_WIN];            // one window / staging region per wave (60.8 KB)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, h = lane >> 5;
    for (int i = tid; i < STEM_NP * 128; i += 512) {
        const int kp = i >> 7, r = i & 127, nb = r & 1, hl = r >> 1, hh = hl >> 5, ll = hl & 31;
        const int R = kp / 7 + STEM_RP * hh, kz = kp % 7;
        wsh[i] = R < 49 ? p.w[(R * 7 + kz) * 64 + nb * 32 + ll] : 0.0f;
    }
    float* ww = win[wave];
    if (lane < STEM_WZ) ww[49 * STEM_WZ + lane] = 0.0f;   // the padding row
    __syncthreads();                              // the only barrier: waves run free below
    const size_t plane = (size_t)(p.halo ? p.hdl : p.D), row = (size_t)p.W * plane, img = (size_t)p.H * row;
    auto decode = [&](int64_t t, int& b, int& oy, int& ox, int& tz) {
        tz = (int)(t % tz_n); t /= tz_n;
        ox = (int)(t % p.OW); t /= p.OW;
        oy = (int)(t % p.OH);
        b = (int)(t / p.OH);
    };
    auto fetch = [&](int64_t tile, float* v) {
        int b, oy, ox, tz;
        decode(tile, b, oy, ox, tz);
        const int gy0 = 2 * oy - p.py, gx0 = 2 * ox - p.px, gz0 = tz * STEM_TZ - p.pz;
        const float* xb = p.a + b * img;
#pragma unroll
        for (int q = 0; q < STEM_PER; ++q) {
            const int i = lane + 64 * q;
            float val = 0.0f;
            if (i < 49 * STEM_WZ) {
                const int R = i / STEM_WZ, iz = i - R * STEM_WZ;
                const int gy = gy0 + R / 7, gx = gx0 + R % 7, gz = gz0 + iz;
                if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W && gz >= 0 && gz < p.D) {
                    if (p.halo) {     // virtual z grid: slab planes from x, the others from the halo
                        const int zl = gz - p.hnlo;
                        if ((unsigned)zl < (unsigned)p.hdl)
                            val = xb[gy * row + gx * plane + zl];
                        else
                            val = p.halo[(((size_t)b * p.H + gy) * p.W + gx) * (2 * p.hr) +
                                         (zl < 0 ? zl + p.hr : p.hr + zl - p.hdl)];
                    } else {
                        val = xb[gy * row + gx * plane + gz];
                    }
                }
            }
            v[q] = val;
        }
    };
    const int64_t w0 = (int64_t)blockIdx.x * 8 + wave, wstride = (int64_t)gridDim.x * 8;
    float4 ebias[2], escale[2], eshift[2];
    for (int nb = 0; nb < 2; ++nb) {
        const int n = nb * 32 + 4 * (lane & 7);
        ebias[nb] = e.bias ? ld4(e.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        escale[nb] = e.scale ? ld4(e.scale + n) : make_float4(1.f, 1.f, 1.f, 1.f);
        eshift[nb] = e.scale ? ld4(e.shift + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float pre[STEM_PER];
    if (w0 < ntiles) fetch(w0, pre);
    for (int64_t tile = w0; tile < ntiles; tile += wstride) {
#pragma unroll
        for (int q = 0; q < STEM_PER; ++q)
            if (lane + 64 * q < 49 * STEM_WZ) ww[lane + 64 * q] = pre[q];
        __builtin_amdgcn_wave_barrier();
        if (tile + wstride < ntiles) fetch(tile + wstride, pre);      // next window in flight
        int b, oy, ox, tz;
        decode(tile, b, oy, ox, tz);
        floatx16 acc0 = {}, acc1 = {};
        const float* wa = ww + STEM_RP * STEM_WZ * h + l32;           // row R = rp + 25 h
        const float* wb = wsh + lane * 2;
        for (int rp = 0; rp < STEM_RP; ++rp) {
#pragma unroll
            for (int kz = 0; kz < 7; ++kz) {
                const float a = wa[kz];
                const float2 bv = *reinterpret_cast<const float2*>(wb + kz * 128);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv.y, acc1, 0, 0, 0);
            }
            wa += STEM_WZ;
            wb += 7 * 128;
        }
        __builtin_amdgcn_wave_barrier();          // window reads done before the staging writes
        const int64_t mbase = (((int64_t)b * p.OH + oy) * p.OW + ox) * p.OD;
        const int oz0 = tz * STEM_TZ;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const floatx16& acc = nb ? acc1 : acc0;
#pragma unroll
            for (int r = 0; r < 16; ++r) ww[((r & 3) + 8 * (r >> 2) + 4 * h) * STEM_SLD + l32] = acc[r];
            __builtin_amdgcn_wave_barrier();
            // a lane's 4 channels are the same in every row it stores (c4 = lane & 7):
            // the epilogue parameters are held in registers (epi_store4's order of ops)
            const int n = nb * 32 + 4 * (lane & 7);
            const float4 bb = ebias[nb], sc = escale[nb], sh = eshift[nb];
#pragma unroll
            for (int q = 0; q < 4; ++q) {                 // 32 rows x 8 float4 = 4 per lane
                const int rr = (lane >> 3) + 8 * q;
                float4 v = *reinterpret_cast<const float4*>(ww + rr * STEM_SLD + 4 * (lane & 7));
                if (oz0 + rr >= p.OD) continue;
                const int64_t m = mbase + oz0 + rr;
                if (e.bias) { v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w; }
                if (e.z) st4(e.z + m * 64 + n, v);
                if (e.scale) {
                    v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y;
                    v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                }
                if (e.relu) {
                    v.x = act(e.relu, v.x); v.y = act(e.relu, v.y); v.z = act(e.relu, v.z); v.w = act(e.relu, v.w);
                }
                st4(e.y + m * 64 + n, v);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}


bool stem_ok(int64_t Cin, int kh, int kw, int kd, int64_t Cout, int sy, int sx, int sz, int dly, int dlx,
             int dlz, int res_mode, int64_t split_n, int64_t ldy) {
    // the kernel's own epilogue covers bias / z / frozen BN / activation, plain
    // [M, 64] stores (no residual, split or accumulate)
    return Cin == 1 && kh == 7 && kw == 7 && kd == 7 && Cout == 64 && sy == 2 && sx == 2 && sz == 1 &&
           dly == 1 && dlx == 1 && dlz == 1 && res_mode == 0 && split_n <= 0 && (ldy <= 0 || ldy == 64);
}

// ---- the stem's weight gradient: dW[343][64] += sum_m window(m)[tap] dz[m][ch] ----
// The implicit-GEMM weight gradient reads the one-channel window through its
// scalar loader (0.27 of the f32 MFMA peak).  Here a workgroup (8 waves) loops
// over a contiguous range of m-tiles (one output column (oy, ox) x 32 z); per
// tile the 49 x 38 input window (the same fetch as stem_fwd_kernel, halo planes
// included) and the 32 x 64 dz rows are staged in LDS (double-buffered, one
// barrier per tile) and every wave accumulates its 11 of the 88 16 x 16 dW
// tiles (v_mfma_f32_16x16x4_f32: one n-tile of 16 channels x 11 k-tiles of 16
// taps) over the tile's 32 m in steps of 4.  A lane's window offset per k-tile
// is precomputed (tap -> R * 38 + kz), so every operand read is a ds_read_b32
// with an immediate offset.  Taps 343..351 read the zero row.  The partial dW
// leaves through wg_put (fp32 atomics, or the deterministic-mode partials).
constexpr int SWG_STR = 80;                                      // dz staging row stride (floats)
__global__ __launch_bounds__(512) void stem_wgrad_kernel(ConvP p, const float* __restrict__ dz,
                                                         float* __restrict__ dw, WgOut wo, int tz_n,
                                                         int64_t ntiles, int64_t per_block) {
    __shared__ float win[2][STEM_WIN];            // 49 rows x 38 z + the zero row
    __shared__ float dzs[2][STEM_TZ * SWG_STR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t_begin = (int64_t)blockIdx.x * per_block;
    const int64_t t_end = t_begin + per_block < ntiles ? t_begin + per_block : ntiles;
    if (t_begin >= t_end) return;
    float* const wp = wo.part ? wo.part + (int64_t)blockIdx.x * wo.pstride : nullptr;
    if (tid < STEM_WZ) { win[0][49 * STEM_WZ + tid] = 0.0f; win[1][49 * STEM_WZ + tid] = 0.0f; }
    const size_t plane = (size_t)(p.halo ? p.hdl : p.D), row = (size_t)p.W * plane, img = (size_t)p.H * row;
    // per tile: window values i = tid + 512 q (q < 4), dz float4 tid
    float wv[4];
    float4 dv;
    auto fetch = [&](int64_t tile) {
        int64_t t = tile;
        const int tz = (int)(t % tz_n); t /= tz_n;
        const int ox = (int)(t % p.OW); t /= p.OW;
        const int oy = (int)(t % p.OH);
        const int b = (int)(t / p.OH);
        const int gy0 = 2 * oy - p.py, gx0 = 2 * ox - p.px, gz0 = tz * STEM_TZ - p.pz;
        const float* xb = p.a + b * img;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 512 * q;
            float val = 0.0f;
            if (i < 49 * STEM_WZ) {
                const int R = i / STEM_WZ, iz = i - R * STEM_WZ;
                const int gy = gy0 + R / 7, gx = gx0 + R % 7, gz = gz0 + iz;
                if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W && gz >= 0 && gz < p.D) {
                    if (p.halo) {
                        const int zl = gz - p.hnlo;
                        if ((unsigned)zl < (unsigned)p.hdl)
                            val = xb[gy * row + gx * plane + zl];
                        else
                            val = p.halo[(((size_t)b * p.H + gy) * p.W + gx) * (2 * p.hr) +
                                         (zl < 0 ? zl + p.hr : p.hr + zl - p.hdl)];
                    } else {
                        val = xb[gy * row + gx * plane + gz];
                    }
                }
            }
            wv[q] = val;
        }
        const int zi = tid >> 4, c4 = tid & 15;          // 32 rows x 16 float4
        const int oz = tz * STEM_TZ + zi;
        dv = oz < p.OD ? *reinterpret_cast<const float4*>(
                             dz + ((((int64_t)b * p.OH + oy) * p.OW + ox) * p.OD + oz) * 64 + c4 * 4)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (tid + 512 * q < 49 * STEM_WZ) win[buf][tid + 512 * q] = wv[q];
        *reinterpret_cast<float4*>(&dzs[buf][(tid >> 4) * SWG_STR + (tid & 15) * 4]) = dv;
    };
    // this wave: n-tile nt (16 channels), k-tiles kt = kg + 2 j (j < 11) of 16 taps
    const int nt = wave & 3, kg = wave >> 2;
    const int l16 = lane & 15, lq = lane >> 4;
    int abase[11];
#pragma unroll
    for (int j = 0; j < 11; ++j) {
        const int tap = 16 * (kg + 2 * j) + l16;
        const int R = tap < 343 ? tap / 7 : 49, kz = tap < 343 ? tap % 7 : 0;
        abase[j] = R * STEM_WZ + kz + lq;
    }
    const int bbase = lq * SWG_STR + nt * 16 + l16;
    floatx4 acc[11];
#pragma unroll
    for (int j = 0; j < 11; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
    fetch(t_begin);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int64_t t = t_begin; t < t_end; ++t) {
        if (t + 1 < t_end) fetch(t + 1);
        const float* W = win[buf];
        const float* Z = dzs[buf];
#pragma unroll
        for (int s = 0; s < STEM_TZ / 4; ++s) {
            const float bv = Z[bbase + 4 * s * SWG_STR];
#pragma unroll
            for (int j = 0; j < 11; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(W[abase[j] + 4 * s], bv, acc[j], 0, 0, 0);
        }
        if (t + 1 < t_end) stage(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int j = 0; j < 11; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tap = 16 * (kg + 2 * j) + 4 * lq + r;
            if (tap < 343) wg_put(wo, dw, wp, (int64_t)tap * 64 + nt * 16 + l16, acc[j][r]);
        }
}


int launch_stem_wgrad(const ConvP& p, const float* dz, float* dw, hipStream_t s) {
    const int ncu = num_cus();
    const int tz_n = (p.OD + STEM_TZ - 1) / STEM_TZ;
    const int64_t ntiles = (int64_t)p.B * p.OH * p.OW * tz_n;
    // two workgroups per CU (LDS 2 x 23.4 KB each, 8 waves), >= 8 m-tiles each
    int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(2 * (int64_t)ncu, (ntiles + 7) / 8));
    const WgOut wo = wg_out(blocks, 1, 343, 64);
    const int64_t per = (ntiles + blocks - 1) / blocks;
    blocks = (ntiles + per - 1) / per;
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3((unsigned)blocks), dim3(512), 0, s, p, dz, dw, wo, tz_n, ntiles, per);
    wg_finish(wo, blocks, 1, 343, 64, 343 * 64, dw, s);
    return check_launch("stem_wgrad_kernel");
}

int launch_stem(const ConvP& p, const Epi& e, hipStream_t s) {
    const int ncu = num_cus();
    const int tz_n = (p.OD + STEM_TZ - 1) / STEM_TZ;
    const int64_t ntiles = (int64_t)p.B * p.OH * p.OW * tz_n;
    // about four workgroups per CU, not one persistent workgroup per CU: the
    // stem opens the step while the previous step's side-stream work (the
    // one-CU NMS reduce) may still hold a CU, and a persistent block waiting
    // for that CU would stall the whole launch (measured 1.5 ms in the step
    // vs 0.28 ms alone at 128^3); with 4 per CU the others absorb its share
    // M3D_STEM_X3=1 / 2: the bf16-split forms (measured slower than the f32 kernel: 2.65 / 2.24-2.5 vs
    // 2.2 ms at 256^3, DESIGN.md round-3 list); default the f32 MFMA kernel
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ntiles + 7) / 8, 4 * (int64_t)ncu));
    hipLaunchKernelGGL(stem_fwd_kernel, dim3(grid), dim3(512), 0, s, p, e, tz_n, ntiles);
    return check_launch("stem_fwd_kernel");
}

}  // namespace m3d
