// Internal header of the conv sources (gfx950 only).  conv3d.hip holds the
// convolution kernels and their entry points; two families that reach it only
// through host launchers have files of their own:
//   conv_rowsparse.hip  the row-sparse scan and data-gradient scatter (rs_*)
//   rpn_head_bwd.hip    the RPN head's compact backward (hc_*)
// A __global__ kernel is defined and launched in one file only (the build has
// no relocatable device code): a file that needs another's kernel calls the
// launcher declared here.  Beside those declarations the header holds only
// what both sides compile: kernel-argument structs, constants and
// force-inlined device helpers.
#pragma once
#include "common.h"

namespace m3d {

// the exact 3-way bf16 split of an fp32 value (conv3d.hip, "exact 3-way bf16 split", says why it is exact)
__device__ __forceinline__ uint32_t bf16_bits(float x) {
    return (uint32_t)__builtin_bit_cast(unsigned short, (__bf16)x);
}
__device__ __forceinline__ void split3(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
    h = bf16_bits(x);
    const float r = x - __uint_as_float(h << 16);
    m = bf16_bits(r);
    l = bf16_bits(r - __uint_as_float(m << 16));
}

// ---- row-sparse output gradients (conv_rowsparse.hip holds the description) ----
// the header's words, the scan's constants and the kernel-argument structs that
// the Winograd backward and the RPN head's compact backward fill in
constexpr int RS_CAP_MAX = 4096;        // most active rows the sparse path takes ...
constexpr int RS_CAP_DIV = 32;          // ... and at most rows / 32
constexpr int RS_PROBE_ROWS = 256;      // rows the probe reads
constexpr int RS_PROBE_DIV = 8;         // probe: DENSE when more than 1 / 8 of them are active
constexpr int RS_BLK = 64;              // rows per scan block
enum { RS_STATE = 0, RS_SKIP_DENSE = 1, RS_SKIP_SPARSE = 2, RS_N = 3, RS_PROBE = 4, RS_HDR_INTS = 64 };
enum { RS_UNDECIDED = 0, RS_DENSE = 1, RS_SPARSE = 2 };

// rs_mode, a per-call argument of m3d_conv3d_bwd_data_wino_rs / m3d_conv3d_bwd_weight_wino_ux (a test
// and A/B hook; the library holds no mode, every other entry point runs RS_AUTO): RS_AUTO attempts from
// RS_MIN_FLOP on, RS_OFF runs exactly the dense launches, ungated, RS_ALWAYS attempts at every size.
enum { RS_AUTO = 0, RS_OFF = 1, RS_ALWAYS = 2 };

struct RsHdr { int *h, *idx, *blk, *slot; };

struct RsPack {
    const float* dz = nullptr;
    int64_t rows = 0;
    int C = 0, cap = 0;
    int* h = nullptr;
    const int* blk = nullptr;
    int* slot = nullptr;
    int* idx = nullptr;
    float* dzc = nullptr;                  // [cap][C]
    const float* x = nullptr;              // weight gradient: x [B][H][W][D][Cx] -> xg [27][cap][Cx]
    float* xg = nullptr;
    int H = 0, W = 0, D = 0, OD = 0, pz = 0, Cx = 0;
    const float* w = nullptr;              // data gradient: w (nw elements) -> planes wp [3][nw]
    unsigned short* wp = nullptr;
    int64_t nw = 0;
    unsigned nb_idx = 0, nb_zero = 0;
};

// one wave copies (on) or zero-fills a row of C floats, C % 4 == 0 (the gathers of rs_pack_kernel and hc_*)
__device__ __forceinline__ void rs_copy_row(const float* __restrict__ s, float* __restrict__ d, int C, int lane,
                                            bool on) {
    for (int c = lane * 4; c < C; c += 256) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (on) v = *reinterpret_cast<const float4*>(s + c);
        *reinterpret_cast<float4*>(d + c) = v;
    }
}

// ---- host functions called across files (defined in the file named) ----------
// conv3d.hip: the point GEMMs M[xi] = U[xi] V[xi] on split planes (x3_gemm*_kernel), the bf16-split
// weight-gradient GEMM C[b] += A[b]^T B[b] (x3_wgrad*_kernel), split3_kernel
void launch_gemm_x3(const float* U, const float* V, float* Mo, int64_t T, int K, int N, int P, hipStream_t s,
                    bool af32 = false, const int* gate = nullptr, const int* mlim = nullptr);
int launch_wgrad_x3(const float* A, const float* Bm, float* C, int64_t M, int K, int N, int nbatch, int64_t bsa,
                    int64_t bsb, int64_t bsc, hipStream_t s, bool fresh = false, const int* gate = nullptr);
void launch_split3(const float* x, int64_t n, unsigned short* x3, hipStream_t s);
// conv_rowsparse.hip
size_t rs_al(size_t b);
size_t rs_hdr_bytes(int64_t rows);   // the header for dz of `rows` voxel rows
RsHdr rs_hdr(void* base, int64_t rows);
int rs_cap(int64_t rows);
bool rs_attempt(int mode, int64_t rows, int64_t Cin, int64_t Cout);
void rs_scan(const float* dz, int64_t rows, int C, int cap, const RsHdr& hd, RsPack q, hipStream_t s);
size_t rs_dgrad_bytes(int cap, int64_t Cin, int64_t Cout);
size_t rs_wgrad_bytes(int cap, int64_t Cin, int64_t Cout);
void rs_dgrad_launch(const float* dz, const float* w, int64_t B, int H, int W, int D, int OD, int pz, int Cin,
                     int Cout, float* dx, int accumulate, char* um, int cap, const RsHdr& hd, hipStream_t s);
// rs_dgrad_out_kernel over nvox voxels of dx
void launch_rs_dgrad_out(const float* ct, int64_t nvox, int H, int W, int D, int OD, int pz, int C, int accumulate,
                         const int* h, const int* slot, float* dx, hipStream_t s);

}  // namespace m3d
