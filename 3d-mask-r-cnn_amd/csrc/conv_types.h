// Internal header of the conv sources (gfx950 only).  conv3d.hip holds the
// convolution kernels and their entry points; three families that touch it only
// through host launchers have files of their own:
//   conv_stem.hip       the one-channel 7^3 stem and its weight gradient (stem_*)
//   conv_rowsparse.hip  the row-sparse scan and data-gradient scatter (rs_*)
//   rpn_head_bwd.hip    the RPN head's compact backward (hc_*)
// A kernel is defined and launched in one file only (the build has
// no relocatable device code): a file that needs another's kernel calls the
// launcher declared here.  Beside those declarations the header holds only
// what both sides compile: kernel-argument structs, constants and
// force-inlined device helpers.
#pragma once
#include "common.h"

namespace m3d {

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct ConvP {
    const float* a;   // A source (x or dz), channels-last [B,H,W,D,C]
    int B, H, W, D, C;
    int OH, OW, OD;   // M grid
    int kh, kw, kd;
    int sy, sx, sz;
    int py, px, pz;
    int64_t M;
    int K;            // taps * C
    const float* w;
    int N;
    int flip;         // bwd-data: use tap (taps-1-t)
    // batched GEMMs (Winograd points): blockIdx.z selects the batch; A, W and Y
    // advance by these element strides (0 for ordinary convs)
    int64_t bsa, bsw, bsy;
    int dly = 1, dlx = 1, dlz = 1;   // dilation (mrcnn_mask_conv3b: fwd, bwd-data on the flipped taps, bwd-weight)
    int nbatch = 1;                  // batches (PERSIST: looped inside the grid)
    // depth-slab halo planes beside the slab (the stem and the direct weight
    // gradient, m3d_conv3d_*_halo): the conv runs on the virtual z grid
    // [lower halo (hnlo planes) | slab (hdl) | upper halo], D = its depth; x (a)
    // holds the slab [B,H,W,hdl,C], halo [B,H,W,2*hr,C] the neighbours' planes
    // ([0,hr) from below, [hr,2hr) from above)
    const float* halo = nullptr;
    int hnlo = 0, hdl = 0, hr = 0;
};

struct Epi {
    const float* bias;
    const float* scale;
    const float* shift;
    const float* res;
    int res_mode;
    int relu;
    float* z;
    float* y;
    int64_t ldy;
    float* y2;
    int64_t ldy2;
    int split;
    int YH, YW, YD;
    int ysy, ysx, ysz;
    int accumulate;
    int simple;       // y row == m (same grid, unit store stride)
    // depth-slab halo (wino_output_kernel<.., HALO>): output z over the
    // halo-extended grid; planes [hlo, hlo + dl) go to y (depth dl), the halo
    // planes to yh [B][H][W][2][N] (plane 0 below, 1 above)
    float* yh;
    int hlo, dl;
    int deconv = 0;   // > 0: 2x2x2 stride-2 transposed conv, n = tap * deconv + o
    // fused BN-ReLU backward of the unit that produced this data gradient's
    // input (m3d_conv3d_bwd_data_bn): the stored value t (after accumulate) is
    // the unit's output gradient; written instead are dz = act'(t) * scale
    // (into y), dpre = act'(t) (into fdres, if set), and per-tile channel sums
    // of dpre, dpre * xhat, dz (rows of fpart, [3][rows][N]) -- the maths of
    // bn_act_bwd_kernel
    int fbn = 0, frelu = 0;
    const float* fy = nullptr;
    const float* fz = nullptr;
    const float* fscale = nullptr;
    const float* fmean = nullptr;
    const float* frstd = nullptr;
    float* fdres = nullptr;
    float* fpart = nullptr;
    int64_t fprows = 0;           // partial rows (stride of the three sum planes)
};

// activation codes (Epi::relu): 0 none, 1 ReLU, 2 sigmoid (mrcnn_mask)
__device__ __forceinline__ float act(int code, float v) {
    if (code == 1) return v > 0.0f ? v : 0.0f;
    if (code == 2) return 1.0f / (1.0f + expf(-v));
    return v;
}

// 16-byte loads / stores of four consecutive floats
__device__ __forceinline__ float4 ld4(const float* q) { return *reinterpret_cast<const float4*>(q); }
__device__ __forceinline__ void st4(float* q, const float4& v) { *reinterpret_cast<float4*>(q) = v; }

// -------------------------------------------------------------------------
// Weight-gradient epilogue target.  Default: fp32 atomics into C (the m-splits
// of a tile arrive in any order, so the last bits vary run to run).
// Deterministic mode (m3d_set_deterministic): each split stores its tile into
// part[split][batch][K][N] of the registered scratch and wg_reduce_kernel adds
// the splits to C in split order; with a single split (the scratch too small
// for two), the one writer of each element adds to C without an atomic.
// Store (either mode): the caller declared C uninitialised scratch (`fresh`,
// the Winograd-domain dW_hat) and the launcher settled on one split of a
// non-stream-K grid, so each (batch, k, n) has exactly one writer, which
// stores its sum: no zero-fill before the launch and no read of C
// (wg_settle).  Every other fresh launch is preceded by the fill.
// -------------------------------------------------------------------------
struct WgOut {
    float* part;
    int64_t pstride;      // floats per split (nbatch * K * N)
    int plain;
    int store;
    const int* gate;      // row-sparse gate (bwd_weight_wino): the workgroup returns when *gate != 0; NULL: ungated
};

__device__ __forceinline__ void wg_put(const WgOut& o, float* C, float* P, int64_t idx, float v) {
    if (P) P[idx] = v;
    else if (o.store) C[idx] = v;
    else if (o.plain) C[idx] += v;
    else unsafeAtomicAdd(C + idx, v);
}

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
// conv3d.hip: the chip's CU count, and the weight-gradient target of a launch (WgOut above; wg_finish
// runs wg_reduce_kernel)
int num_cus();
WgOut wg_out(int64_t& splits, int64_t nbatch, int64_t K, int64_t N);
void wg_finish(const WgOut& o, int64_t splits, int64_t nbatch, int64_t K, int64_t N, int64_t bsc, float* C,
               hipStream_t s);
// conv_stem.hip: stem_ok: the conv is the one-channel 7^3 stem with an epilogue the stem kernels cover
bool stem_ok(int64_t Cin, int kh, int kw, int kd, int64_t Cout, int sy, int sx, int sz, int dly, int dlx, int dlz,
             int res_mode, int64_t split_n, int64_t ldy);
int launch_stem(const ConvP& p, const Epi& e, hipStream_t s);
int launch_stem_wgrad(const ConvP& p, const float* dz, float* dw, hipStream_t s);
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
