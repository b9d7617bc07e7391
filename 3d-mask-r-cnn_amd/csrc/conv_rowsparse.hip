// ---- row-sparse output gradients --------------------------------------------
// The RPN loss leaves a gradient only on the sampled anchors, so the dz that
// reaches rpn_conv_shared1 has a few hundred non-zero voxel rows out of 10^5.
// bwd_data_wino / bwd_weight_wino scan dz on the device (a probe of evenly
// spaced rows first: a dense dz costs no pass over the tensor), and either run
// the Winograd launches (state DENSE) or a gather -> split GEMM -> scatter
// over the active rows only (state SPARSE).  Both sets of launches are always
// enqueued -- the step is replayed from a graph -- and every workgroup of the
// set that is not due returns on a gate word of the header below.
// Header (ints) behind the call's [WT][V][U][M] layout:
//   h[RS_STATE] 0 undecided (after the probe) / RS_DENSE / RS_SPARSE
//   h[RS_SKIP_DENSE] != 0: the dense kernels return; h[RS_SKIP_SPARSE] != 0: the sparse ones
//   h[RS_N] active rows (SPARSE);  h[RS_PROBE] != 0: the probe found dz dense (written by the probe
//   alone: the scan kernels read it, and never a word that one of them writes);
//   idx[RS_CAP_MAX] the active rows, ascending;
//   blk[rows / 64] active rows per 64-row group;  slot[rows] row -> compact slot or -1
#include "conv_types.h"

namespace m3d {

// RS_AUTO attempts the sparse path when the layer's direct-equivalent work 2 * 27 * rows * Cin * Cout reaches
// this.  A dense call pays 18-30 us for the attempt (probe, two scan launches that return, the gated sparse
// launches; DESIGN.md 5, scripts/rowsparse_overhead.py), which is to stay near 2 % of the call: 0.9 TFLOP
// admits rpn_conv_shared1 on P2 at 128^3 (0.93 TFLOP: 0.9-1.7 % / 1.6-2.4 % of its dense data / weight
// gradient) and leaves out fpn_p2 (0.46 TFLOP: 2.9 % / 3.2 %) and P3 (0.23 TFLOP).  The benchmark's P2
// sits 3 % above the threshold: a smaller volume runs dense (DESIGN.md 5 says what would lift that)
constexpr double RS_MIN_FLOP = 9e11;

size_t rs_al(size_t b) { return (b + 255) & ~(size_t)255; }
size_t rs_hdr_bytes(int64_t rows) {
    return rs_al(sizeof(int) * (RS_HDR_INTS + RS_CAP_MAX)) + rs_al(sizeof(int) * (size_t)((rows + RS_BLK - 1) / RS_BLK)) +
           rs_al(sizeof(int) * (size_t)rows);
}
RsHdr rs_hdr(void* base, int64_t rows) {
    RsHdr r{};
    char* p = static_cast<char*>(base);
    r.h = reinterpret_cast<int*>(p);
    r.idx = r.h + RS_HDR_INTS;
    p += rs_al(sizeof(int) * (RS_HDR_INTS + RS_CAP_MAX));
    r.blk = reinterpret_cast<int*>(p);
    p += rs_al(sizeof(int) * (size_t)((rows + RS_BLK - 1) / RS_BLK));
    r.slot = reinterpret_cast<int*>(p);
    return r;
}
int rs_cap(int64_t rows) {
    const int64_t c = rows / RS_CAP_DIV;
    return (int)(c > RS_CAP_MAX ? RS_CAP_MAX : c);
}
// whether this call scans dz at all (host side: shapes and the process mode only)
bool rs_attempt(int mode, int64_t rows, int64_t Cin, int64_t Cout) {
    if (mode == RS_OFF) return false;
    if (rs_cap(rows) < 1 || rows > 0x7FFFFFFF) return false;
    return mode == RS_ALWAYS || 2.0 * 27.0 * (double)rows * (double)Cin * (double)Cout >= RS_MIN_FLOP;
}

// this lane's part of "row has an element != 0" (-0.0f is not, a NaN is), C % 4 == 0
__device__ __forceinline__ bool rs_lane_active(const float* __restrict__ row, int C, int lane) {
    bool a = false;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(row + c);
        a |= (v.x != 0.0f) | (v.y != 0.0f) | (v.z != 0.0f) | (v.w != 0.0f);
    }
    return a;
}

// one workgroup of 16 waves: RS_PROBE_ROWS evenly spaced rows, 16 per wave
__global__ __launch_bounds__(1024) void rs_probe_kernel(const float* __restrict__ dz, int64_t rows, int C,
                                                        int* __restrict__ h) {
    __shared__ int cnt[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ns = rows < RS_PROBE_ROWS ? (int)rows : RS_PROBE_ROWS;
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < RS_PROBE_ROWS / 16; ++k) {
        const int i = wave * (RS_PROBE_ROWS / 16) + k;
        bool a = false;
        // evenly spaced, each sample 37 rows further along than the last: a plain stride is a multiple of
        // the depth at the step's shapes and would read one z plane and one x phase only
        if (i < ns) a = rs_lane_active(dz + (((int64_t)i * rows / ns + (int64_t)i * 37) % rows) * C, C, lane);
        m |= (a ? 1u : 0u) << k;
    }
    int c = 0;
#pragma unroll
    for (int k = 0; k < RS_PROBE_ROWS / 16; ++k) c += __ballot((m >> k) & 1u) != 0ull ? 1 : 0;
    if (lane == 0) cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int w = 0; w < 16; ++w) a += cnt[w];
        const bool dense = a * RS_PROBE_DIV > ns;
        h[RS_PROBE] = dense ? 1 : 0;
        h[RS_STATE] = dense ? RS_DENSE : RS_UNDECIDED;
        h[RS_SKIP_DENSE] = 0;
        h[RS_SKIP_SPARSE] = 1;
        h[RS_N] = 0;
    }
}

// slot[row] = row active (0 / 1), blk[block] = active rows of the block's RS_BLK rows
__global__ __launch_bounds__(256) void rs_flag_kernel(const float* __restrict__ dz, int64_t rows, int C,
                                                      const int* __restrict__ h, int* __restrict__ blk,
                                                      int* __restrict__ slot) {
    if (h[RS_PROBE]) return;
    __shared__ int cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * RS_BLK + wave * 16;
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        bool a = false;
        if (r0 + k < rows) a = rs_lane_active(dz + (r0 + k) * C, C, lane);
        m |= (a ? 1u : 0u) << k;
    }
    int c = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int act = __ballot((m >> k) & 1u) != 0ull ? 1 : 0;
        if (lane == 0 && r0 + k < rows) slot[r0 + k] = act;
        c += act;
    }
    if (lane == 0) cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// Everything between the scan's flags and the sparse GEMM, in one launch (each launch a dense call
// makes for nothing costs it about 3.5 us).  Every workgroup sums blk itself -- the count n, hence the
// state, and the count before its own rows -- so no launch stands between the flags and their prefix.
// Block ranges: [0, nb_idx) 256 rows each: slot[row] = compact slot or -1, idx[slot] = row (ascending:
// slots follow the row order), and the active rows gathered, dzc[slot] = dz[row] and, for the weight
// gradient, xg[tap][slot] = x at the tap's input voxel ('same' padding: zero outside);
// then nb_zero blocks zero rows n..cap of dzc / xg; then (data gradient) the three bf16 planes of w.
constexpr int RS_SPLIT_PER = 2048;         // elements of w per split block

__global__ __launch_bounds__(256) void rs_pack_kernel(RsPack p) {
    // the probe's verdict, in a word no launch of this kernel writes: the exit is the same for every wave
    // of every workgroup (block 0 publishes the final state below, in words this kernel never reads)
    if (p.h[RS_PROBE]) return;
    __shared__ int red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nblk = (p.rows + RS_BLK - 1) / RS_BLK;
    const bool ib = blockIdx.x < p.nb_idx;
    const int64_t g0 = ib ? (int64_t)blockIdx.x * 4 : 0;        // this block's first 64-row group
    int tot = 0, pre = 0;
    for (int64_t i = tid; i < nblk; i += 256) {
        const int c = p.blk[i];
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
    const bool sparse = n <= p.cap;
    if (blockIdx.x == 0 && tid == 0) {
        p.h[RS_STATE] = sparse ? RS_SPARSE : RS_DENSE;
        p.h[RS_SKIP_DENSE] = sparse ? 1 : 0;
        p.h[RS_SKIP_SPARSE] = sparse ? 0 : 1;
        p.h[RS_N] = sparse ? n : 0;
    }
    if (!sparse) return;
    if (ib) {
        const int64_t g = g0 + wave;
        if (g >= nblk) return;
        int base = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        for (int q = 0; q < wave; ++q) base += p.blk[g0 + q];
        const int64_t r = g * RS_BLK + lane;
        const bool act = r < p.rows && p.slot[r] != 0;
        unsigned long long m = __ballot(act);
        const int s = base + __popcll(m & ((1ull << lane) - 1ull));
        if (r < p.rows) p.slot[r] = act ? s : -1;
        if (act) p.idx[s] = (int)r;                    // s < n <= cap <= RS_CAP_MAX
        for (int k = 0; m; ++k) {                      // the group's active rows, one after the other
            const int j = __ffsll(m) - 1;
            m &= m - 1;
            const int64_t row = g * RS_BLK + j;
            const int sk = base + k;
            if (!p.dzc) break;                         // (the scan alone)
            rs_copy_row(p.dz + row * p.C, p.dzc + (int64_t)sk * p.C, p.C, lane, true);
            if (!p.xg) continue;
            int64_t t = row;
            const int zo = (int)(t % p.OD); t /= p.OD;
            const int xo = (int)(t % p.W); t /= p.W;
            const int yo = (int)(t % p.H);
            const int64_t b = t / p.H;
            // all 27 taps' loads of a 256-channel chunk in flight before the stores (one wave per row:
            // tap after tap the copies ran at one load latency each, 54 us of the 128^3 P2 call)
            for (int c = lane * 4; c < p.Cx; c += 256) {
                float4 v[27];
#pragma unroll
                for (int tap = 0; tap < 27; ++tap) {
                    const int yi = yo + tap / 9 - 1, xi = xo + (tap / 3) % 3 - 1, zi = zo + tap % 3 - p.pz;
                    const bool in = (unsigned)yi < (unsigned)p.H && (unsigned)xi < (unsigned)p.W &&
                                    (unsigned)zi < (unsigned)p.D;
                    v[tap] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (in)
                        v[tap] = *reinterpret_cast<const float4*>(
                            p.x + (((b * p.H + yi) * p.W + xi) * p.D + zi) * p.Cx + c);
                }
#pragma unroll
                for (int tap = 0; tap < 27; ++tap)
                    *reinterpret_cast<float4*>(p.xg + ((int64_t)tap * p.cap + sk) * p.Cx + c) = v[tap];
            }
        }
        return;
    }
    const unsigned bz = blockIdx.x - p.nb_idx;
    if (bz < p.nb_zero) {
        const int r = (int)bz * 4 + wave;
        if (r < n || r >= p.cap) return;
        rs_copy_row(p.dz, p.dzc + (int64_t)r * p.C, p.C, lane, false);
        if (p.xg)
            for (int tap = 0; tap < 27; ++tap)
                rs_copy_row(p.x, p.xg + ((int64_t)tap * p.cap + r) * p.Cx, p.Cx, lane, false);
        return;
    }
    const int64_t i0 = (int64_t)(bz - p.nb_zero) * RS_SPLIT_PER + tid;
#pragma unroll
    for (int k = 0; k < RS_SPLIT_PER / 256; ++k) {
        const int64_t i = i0 + k * 256;
        if (i >= p.nw) break;
        uint32_t hi, mi, lo;
        split3(p.w[i], hi, mi, lo);
        p.wp[i] = (unsigned short)hi;
        p.wp[p.nw + i] = (unsigned short)mi;
        p.wp[2 * p.nw + i] = (unsigned short)lo;
    }
}

// probe, flags, pack: q holds the pack's operands (x / xg or w / wp, dzc); the rest is filled in here
void rs_scan(const float* dz, int64_t rows, int C, int cap, const RsHdr& hd, RsPack q, hipStream_t s) {
    const int64_t nblk = (rows + RS_BLK - 1) / RS_BLK;
    q.dz = dz; q.rows = rows; q.C = C; q.cap = cap;
    q.h = hd.h; q.blk = hd.blk; q.slot = hd.slot; q.idx = hd.idx;
    q.nb_idx = (unsigned)((nblk + 3) / 4);
    q.nb_zero = q.dzc ? (unsigned)((cap + 3) / 4) : 0;
    const unsigned nb_split = (unsigned)((q.nw + RS_SPLIT_PER - 1) / RS_SPLIT_PER);
    hipLaunchKernelGGL(rs_probe_kernel, dim3(1), dim3(1024), 0, s, dz, rows, C, hd.h);
    hipLaunchKernelGGL(rs_flag_kernel, dim3((unsigned)nblk), dim3(256), 0, s, dz, rows, C, hd.h, hd.blk, hd.slot);
    hipLaunchKernelGGL(rs_pack_kernel, dim3(q.nb_idx + q.nb_zero + nb_split), dim3(256), 0, s, q);
}

// dx[v][:] (+)= sum over the 27 taps, in tap order, of ct[slot(dz row of the tap)][tap][:]
// where that row is inside dz and active: dx voxel (y, x, z) takes tap (ky, kx, kz)
// from dz (y - ky + 1, x - kx + 1, z - kz + pz).  A workgroup owns 8 consecutive
// voxels; a voxel without an active neighbour is zero-filled (left as it is
// under accumulate).
constexpr int RS_VOX = 8;
__global__ __launch_bounds__(256) void rs_dgrad_out_kernel(const float* __restrict__ ct, int64_t nvox, int H, int W,
                                                           int D, int OD, int pz, int C, int accumulate,
                                                           const int* __restrict__ h,
                                                           const int* __restrict__ slot, float* __restrict__ dx) {
    if (h[RS_SKIP_SPARSE]) return;
    __shared__ int ss[RS_VOX * 27];
    __shared__ int hit[RS_VOX];
    const int tid = threadIdx.x;
    const int64_t v0 = (int64_t)blockIdx.x * RS_VOX;
    if (tid < RS_VOX) hit[tid] = 0;
    __syncthreads();
    if (tid < RS_VOX * 27) {
        const int j = tid / 27, tap = tid % 27, ky = tap / 9, kx = (tap / 3) % 3, kz = tap % 3;
        int sl = -1;
        int64_t t = v0 + j;
        if (t < nvox) {
            const int z = (int)(t % D); t /= D;
            const int xx = (int)(t % W); t /= W;
            const int y = (int)(t % H);
            const int64_t b = t / H;
            const int yo = y - ky + 1, xo = xx - kx + 1, zo = z - kz + pz;
            if ((unsigned)yo < (unsigned)H && (unsigned)xo < (unsigned)W && (unsigned)zo < (unsigned)OD)
                sl = slot[((b * H + yo) * W + xo) * OD + zo];
        }
        ss[tid] = sl;
        if (sl >= 0) hit[j] = 1;
    }
    __syncthreads();
    const int L = C / 4;
    for (int q = tid; q < RS_VOX * L; q += 256) {
        const int j = q / L, c = (q % L) * 4;
        if (v0 + j >= nvox) break;
        float* o = dx + (v0 + j) * C + c;
        if (!hit[j]) {
            if (!accumulate) *reinterpret_cast<float4*>(o) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            continue;
        }
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (accumulate) a = *reinterpret_cast<const float4*>(o);
        for (int tap = 0; tap < 27; ++tap) {
            const int sl = ss[j * 27 + tap];
            if (sl < 0) continue;
            const float4 v = *reinterpret_cast<const float4*>(ct + ((int64_t)sl * 27 + tap) * C + c);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        *reinterpret_cast<float4*>(o) = a;
    }
}

// bytes the sparse paths lay out from the U region on (both regions belong to
// the path that runs): data gradient dzc [cap][Cout], w planes, ct [cap][27][Cin];
// weight gradient dzc [cap][Cout], xg [27][cap][Cin]
size_t rs_dgrad_bytes(int cap, int64_t Cin, int64_t Cout) {
    return rs_al(4 * (size_t)cap * Cout) + rs_al(6 * 27 * (size_t)Cin * Cout) + rs_al(4 * (size_t)cap * 27 * Cin);
}
size_t rs_wgrad_bytes(int cap, int64_t Cin, int64_t Cout) {
    return rs_al(4 * (size_t)cap * Cout) + rs_al(4 * 27 * (size_t)cap * Cin);
}

// the scan and the sparse data gradient's launches (gated on h[RS_SKIP_SPARSE]); um: the U region
void rs_dgrad_launch(const float* dz, const float* w, int64_t B, int H, int W, int D, int OD, int pz, int Cin,
                     int Cout, float* dx, int accumulate, char* um, int cap, const RsHdr& hd, hipStream_t s) {
    float* dzc = reinterpret_cast<float*>(um);
    unsigned short* wp = reinterpret_cast<unsigned short*>(um + rs_al(4 * (size_t)cap * Cout));
    float* ct = reinterpret_cast<float*>(um + rs_al(4 * (size_t)cap * Cout) + rs_al(6 * 27 * (size_t)Cin * Cout));
    RsPack q{};
    q.dzc = dzc; q.w = w; q.wp = wp; q.nw = (int64_t)27 * Cin * Cout;
    rs_scan(dz, B * H * W * OD, Cout, cap, hd, q, s);
    // ct[r][tap * Cin + c] = sum_n dzc[r][n] w[tap][c][n]: A = dzc (fp32), B = w as [27 Cin][Cout] planes
    launch_gemm_x3(dzc, reinterpret_cast<const float*>(wp), ct, cap, Cout, 27 * Cin, 1, s, true,
                   hd.h + RS_SKIP_SPARSE, hd.h + RS_N);
    launch_rs_dgrad_out(ct, B * H * W * D, H, W, D, OD, pz, Cin, accumulate, hd.h, hd.slot, dx, s);
}

void launch_rs_dgrad_out(const float* ct, int64_t nvox, int H, int W, int D, int OD, int pz, int C, int accumulate,
                         const int* h, const int* slot, float* dx, hipStream_t s) {
    hipLaunchKernelGGL(rs_dgrad_out_kernel, dim3((unsigned)((nvox + RS_VOX - 1) / RS_VOX)), dim3(256), 0, s, ct, nvox,
                       H, W, D, OD, pz, C, accumulate, h, slot, dx);
}

}  // namespace m3d

using namespace m3d;

// The scan alone (tests): ws receives the header of the layout above for `rows` rows.
extern "C" size_t m3d_conv3d_rowsparse_scan_bytes(int64_t rows) { return rows > 0 ? rs_hdr_bytes(rows) : 0; }
extern "C" int m3d_conv3d_rowsparse_scan(const float* dz, int64_t rows, int64_t C, int32_t cap, void* ws,
                                         size_t ws_bytes, m3d_stream_t s) {
    if (rows <= 0 || rows > 0x7FFFFFFF || C <= 0 || C % 4) return einval("rowsparse_scan: rows > 0 and C a positive multiple of 4");
    if (cap < 0 || cap > RS_CAP_MAX) return einval("rowsparse_scan: cap must be in [0, 4096]");
    if (!dz || !ws || ws_bytes < rs_hdr_bytes(rows)) return einval("rowsparse_scan: workspace missing or too small");
    rs_scan(dz, rows, (int)C, cap, rs_hdr(ws, rows), RsPack{}, st(s));
    return check_launch("rowsparse_scan");
}
