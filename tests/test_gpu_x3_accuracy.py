"""fp32-class accuracy of the bf16-split ("x3") GEMMs and the Winograd chain.

Every hot GEMM here runs fp32 arithmetic as six bf16 MFMAs on an exact 3-way
split (csrc/conv_types.h: split3; csrc/conv3d.hip: x3_mac, x3_mac_pair).  The other GPU tests hold
those kernels to 1e-4 .. 1e-5 of max|ref|, far above the ~1e-6 a lost
second-order term costs (a dropped or doubled MFMA, a wrong plane in a
hand-interleaved chain, a transform that leaves a lo plane zero).  Three bars
that such a fault cannot pass (tests/test_x3ref.py proves it on the host, with
the emulation and the mutations of tests/x3ref.py):

a. single-product probes: one operand has exactly one nonzero per output row
   (column), so every output element is one product a*b; |C - a*b| <=
   8 * 2^-24 |a*b| elementwise.  Derived, not measured: the three dropped terms
   (mid*lo, lo*mid, lo*lo) are below 2^-24 |a*b| in total, the six kept
   products are exact in the fp32 accumulator, at most six accumulator
   roundings cost at most 6.1 * 2^-24, and zero products / split partial sums
   add exact zeros.  (Healthy emulation 1.4 .. 1.7, any fault >= 118.)
b. dense GEMMs, both operands N(0,1): rms_rel <= 2 * e32, e32 the rms_rel of
   torch.bmm in CPU fp32 on the same operands (healthy emulation 0.5 .. 1.5,
   any fault >= 7).
c. the Winograd chain: rms_rel <= 4 * eW, eW the rms_rel of the staged fp32
   Winograd emulation at the kernel's tile (healthy emulation 1.0 .. 2.0, any
   fault >= 37).
d. the (2,2,1)-strided 1x1x1 weight gradient through m3d.nn, both forms
   (WGRAD1_STRIDED_X3 on: subsample + split GEMM, bar b; off: the f32 implicit
   GEMM, whose serial fp32 accumulation has the bar x3ref.STRIDED_F32_BAR).

Every case prints one "x3acc" line with its measured figures."""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import x3ref as R

pytestmark = pytest.mark.gpu

SPATIAL = {300: (5, 6, 10), 180: (6, 6, 5), 32: (4, 4, 2), 64: (4, 4, 4), 256: (8, 8, 4), 2048: (16, 16, 8)}


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def _planes(L, lib, t):
    """m3d_split3_f32 planes of a device tensor"""
    p = torch.empty(3 * t.numel(), dtype=torch.int16, device=t.device)
    lib.check(L.m3d_split3_f32(t.data_ptr(), t.numel(), p.data_ptr(), lib.stream()), "split3")
    return p


# ---- the entry points, each as C = A @ B (A [nb,M,K], B [nb,K,N] numpy fp32) ------
def _gemm_x3(cuda, A, B, af=False):
    from m3d import _lib
    L = _lib.load()
    nb, M, K = A.shape
    N = B.shape[2]
    Ad, Btd = _dev(cuda, A), _dev(cuda, B.transpose(0, 2, 1))
    B3 = _planes(L, _lib, Btd)
    C = torch.full((nb, M, N), float("nan"), device=cuda)
    if af:
        _lib.check(L.m3d_gemm_x3_af(Ad.data_ptr(), B3.data_ptr(), C.data_ptr(), nb, M, K, N, _lib.stream()), "x3_af")
    else:
        A3 = _planes(L, _lib, Ad)
        _lib.check(L.m3d_gemm_x3(A3.data_ptr(), B3.data_ptr(), C.data_ptr(), nb, M, K, N, _lib.stream()), "x3")
    return C.cpu().numpy()


def _gemm_x3_af(cuda, A, B):
    return _gemm_x3(cuda, A, B, af=True)


def _gemm_f32(cuda, A, B):
    from m3d import _lib
    L = _lib.load()
    nb, M, K = A.shape
    N = B.shape[2]
    Ad, Bd = _dev(cuda, A), _dev(cuda, B)
    C = torch.zeros((nb, M, N), device=cuda)
    _lib.check(L.m3d_gemm_f32(Ad.data_ptr(), Bd.data_ptr(), C.data_ptr(), nb, M, K, N, None, 0, 1, _lib.stream()),
               "gemm_f32")
    return C.cpu().numpy()


def _wgrad(cuda, A, B, det=False):
    """m3d_gemm_wgrad_f32: C [rows][N] += X^T B with X = A^T [red][rows] (the
    reduction runs over the operands' rows)"""
    from m3d import _lib
    L = _lib.load()
    nb, rows, red = A.shape
    N = B.shape[2]
    Xd, Bd = _dev(cuda, A.transpose(0, 2, 1)), _dev(cuda, B)
    C = torch.zeros((nb, rows, N), device=cuda)
    _lib.set_deterministic(det, scratch_bytes=64 << 20)
    try:
        _lib.check(L.m3d_gemm_wgrad_f32(Xd.data_ptr(), Bd.data_ptr(), C.data_ptr(), nb, red, rows, N, _lib.stream()),
                   "gemm_wgrad")
        torch.cuda.synchronize()
    finally:
        _lib.set_deterministic(False)
    return C.cpu().numpy()


def _wgrad_det(cuda, A, B):
    return _wgrad(cuda, A, B, det=True)


def _conv1_fwd(cuda, A, B, z=False):
    """m3d_conv3d_fwd_x3, plain (x3_gemm256_af_kernel<0>) or with z_out (<1>)"""
    from m3d import _lib
    L = _lib.load()
    _, M, Cin = A.shape
    Cout = B.shape[2]
    H, W, D = SPATIAL[M]
    x, w = _dev(cuda, A[0]), _dev(cuda, B[0])
    planes = torch.empty(3 * Cin * Cout, dtype=torch.int16, device=cuda)
    _lib.check(L.m3d_conv1_x3_planes(w.data_ptr(), Cin, Cout, 1, planes.data_ptr(), _lib.stream()), "planes")
    y = torch.full((M, Cout), float("nan"), device=cuda)
    zo = torch.full((M, Cout), float("nan"), device=cuda) if z else None
    _lib.check(L.m3d_conv3d_fwd_x3(x.data_ptr(), 1, H, W, D, Cin, planes.data_ptr(), Cout, None, None, None, None,
                                   0, 0, _lib.ptr(zo), y.data_ptr(), _lib.stream()), "fwd_x3")
    if z:       # no bias, BN, residual or activation: y is z, the GEMM value
        assert torch.equal(y, zo)
    return y.cpu().numpy()[None]


def _conv1_fwd_z(cuda, A, B):
    return _conv1_fwd(cuda, A, B, z=True)


def _conv1_dgrad(cuda, A, B, bn=False):
    """m3d_conv3d_bwd_data_x3: dx = dz w^T, dz = A [M][Cout], w = B^T [Cin][Cout];
    bn: m3d_conv3d_bwd_data_x3_bn with an identity descriptor (no ReLU, scale =
    rstd = 1, mean = 0, no z, no sums), whose dx is the GEMM value (<2> epilogue)"""
    from m3d import _lib
    L = _lib.load()
    _, M, Cout = A.shape
    Cin = B.shape[2]
    H, W, D = SPATIAL[M]
    dz, w = _dev(cuda, A[0]), _dev(cuda, B[0].T)
    planes = torch.empty(3 * Cin * Cout, dtype=torch.int16, device=cuda)
    _lib.check(L.m3d_conv1_x3_planes(w.data_ptr(), Cin, Cout, 0, planes.data_ptr(), _lib.stream()), "planes")
    dx = torch.full((M, Cin), float("nan"), device=cuda)
    if bn:
        one, zero = torch.ones(Cin, device=cuda), torch.zeros(Cin, device=cuda)
        d = _lib.BnBwd(None, None, one.data_ptr(), zero.data_ptr(), one.data_ptr(), 0, None, None, None, None)
        nbw = int(L.m3d_bn_bwd_fused_workspace_bytes(1, H, W, D, Cin))
        ws = torch.empty(nbw // 4 + 1, device=cuda)
        _lib.check(L.m3d_conv3d_bwd_data_x3_bn(dz.data_ptr(), planes.data_ptr(), 1, H, W, D, Cin, Cout, dx.data_ptr(),
                                               ctypes.addressof(d), ws.data_ptr(), nbw, _lib.stream()), "bwd_x3_bn")
        torch.cuda.synchronize()
    else:
        _lib.check(L.m3d_conv3d_bwd_data_x3(dz.data_ptr(), planes.data_ptr(), 1, H, W, D, Cin, Cout, dx.data_ptr(),
                                            _lib.stream()), "bwd_x3")
    return dx.cpu().numpy()[None]


def _conv1_dgrad_bn(cuda, A, B):
    return _conv1_dgrad(cuda, A, B, bn=True)


def _conv1_wgrad(cuda, A, B):
    """m3d_conv3d_bwd_weight of a 1x1x1 stride-1 conv: dw [Cin][Cout] += x^T dz,
    x = A^T [voxels][Cin], dz = B [voxels][Cout]"""
    from m3d import _lib
    L = _lib.load()
    _, Cin, M = A.shape
    Cout = B.shape[2]
    H, W, D = SPATIAL[M]
    x, dz = _dev(cuda, A[0].T), _dev(cuda, B[0])
    dw = torch.zeros((Cin, Cout), device=cuda)
    _lib.check(L.m3d_conv3d_bwd_weight(x.data_ptr(), dz.data_ptr(), 1, H, W, D, Cin, 1, 1, 1, Cout, H, W, D,
                                       1, 1, 1, 0, 0, 0, dw.data_ptr(), _lib.stream()), "bwd_weight")
    return dw.cpu().numpy()[None]


def _conv3_fwd(cuda, A, B):
    """m3d_conv3d_fwd, 3x3x3 'same' direct conv whose kernel has only its centre
    tap nonzero: y = x @ w[1,1,1], the other 26 taps add exact zeros"""
    from m3d import _lib
    L = _lib.load()
    _, M, Cin = A.shape
    Cout = B.shape[2]
    H, W, D = SPATIAL[M]
    x = _dev(cuda, A[0])
    wn = np.zeros((3, 3, 3, Cin, Cout), np.float32)
    wn[1, 1, 1] = B[0]
    w = _dev(cuda, wn)
    y = torch.full((M, Cout), float("nan"), device=cuda)
    _lib.check(L.m3d_conv3d_fwd(x.data_ptr(), 1, H, W, D, Cin, w.data_ptr(), 3, 3, 3, Cout, H, W, D, 1, 1, 1, 1, 1, 1,
                                None, None, None, None, 0, 0, None, y.data_ptr(), Cout, None, 0, 0, _lib.stream()),
               "conv3d_fwd")
    return y.cpu().numpy()[None]


def _conv3_dgrad(cuda, A, B):
    """m3d_conv3d_bwd_data of the same conv: dx = dz @ w[1,1,1]^T"""
    from m3d import _lib
    L = _lib.load()
    _, M, Cout = A.shape
    Cin = B.shape[2]
    H, W, D = SPATIAL[M]
    dz = _dev(cuda, A[0])
    wn = np.zeros((3, 3, 3, Cin, Cout), np.float32)
    wn[1, 1, 1] = B[0].T
    w = _dev(cuda, wn)
    dx = torch.full((M, Cin), float("nan"), device=cuda)
    _lib.check(L.m3d_conv3d_bwd_data(dz.data_ptr(), w.data_ptr(), 1, H, W, D, Cin, 3, 3, 3, Cout, H, W, D, 1, 1, 1,
                                     1, 1, 1, dx.data_ptr(), 0, _lib.stream()), "conv3d_bwd_data")
    return dx.cpu().numpy()[None]


ENTRY = {"gemm_x3": _gemm_x3, "gemm_x3_af": _gemm_x3_af, "gemm_f32": _gemm_f32, "gemm_wgrad": _wgrad,
         "gemm_wgrad_det": _wgrad_det, "conv1_fwd_x3": _conv1_fwd, "conv1_fwd_x3_z": _conv1_fwd_z,
         "conv1_dgrad_x3": _conv1_dgrad, "conv1_dgrad_x3_bn": _conv1_dgrad_bn, "conv1_wgrad": _conv1_wgrad,
         "conv3_fwd": _conv3_fwd, "conv3_dgrad": _conv3_dgrad}

# shapes (nb, M, K, N) of C [M][N] = A [M][K] @ B [K][N]; K is the reduction.  The
# weight gradients reduce over their operands' rows: m3d_gemm_wgrad_f32's
# (nb, M, K, N) is (nb, K, M, N) here.
PROBE = []
for _K in (32, 96):
    # x3_gemm_kernel 128x128 with ragged M / N tiles; its 128x64 tile; x3_gemm256(_af)_kernel<0>, ragged M
    PROBE += [(e, (2, 300, _K, n)) for e in ("gemm_x3", "gemm_x3_af") for n in (160, 64, 256)]
# conv_gemm_kernel (split in the LDS store): N = 32 / 64 / 96 tiles, the 128x128
# tiles (>= 512 blocks), K = 40: the non-BT loader
PROBE += [("gemm_f32", s) for s in ((2, 200, 64, 32), (2, 200, 64, 64), (2, 200, 64, 96), (52, 520, 32, 160),
                                    (2, 200, 40, 96))]
# x3_wgrad64_kernel, x3_wgrad_kernel, x3_wgrad_tr_kernel; deterministic and atomic partial sums
PROBE += [(e, s) for e in ("gemm_wgrad", "gemm_wgrad_det") for s in ((2, 64, 300, 96), (2, 128, 300, 160),
                                                                    (2, 192, 600, 192))]
PROBE += [(e, (1, 300, 64, 256)) for e in ("conv1_fwd_x3", "conv1_fwd_x3_z", "conv1_dgrad_x3", "conv1_dgrad_x3_bn")]
PROBE += [("conv1_wgrad", (1, ci, 300, co)) for ci, co in ((64, 96), (128, 160), (256, 256))]
PROBE += [("conv3_fwd", (1, 180, 32, 64)), ("conv3_dgrad", (1, 180, 64, 32))]
# the sparse role on either operand; once per entry point with A * 2^-40, B * 2^20
PROBE_CASES = [(e, s, role, False) for e, s in PROBE for role in ("a", "b")]
PROBE_CASES += [(e, next(s for e2, s in PROBE if e2 == e), "a", True) for e in ENTRY]

DENSE = []
for _K in (32, 64, 256):
    DENSE += [(e, (2, 300, _K, n)) for e in ("gemm_x3", "gemm_x3_af") for n in (160, 64, 256)]
    DENSE += [("gemm_f32", (2, 200, _K, n)) for n in (32, 64, 96)] + [("gemm_f32", (52, 520, _K, 160))]
    DENSE += [(e, (1, 300, _K, 256)) for e in ("conv1_fwd_x3", "conv1_fwd_x3_z", "conv1_dgrad_x3",
                                               "conv1_dgrad_x3_bn")]
    DENSE += [("conv3_fwd", (1, 180, _K, 64)), ("conv3_dgrad", (1, 180, _K, 32))]
DENSE += [("gemm_f32", (2, 200, 40, 96))]
for _M in (32, 64, 256, 2048):      # 2048 rows: the split / stream-K partial sums take part
    DENSE += [(e, (2, k, _M, n)) for e in ("gemm_wgrad", "gemm_wgrad_det") for k, n in ((64, 96), (128, 160),
                                                                                      (192, 192))]
    DENSE += [("conv1_wgrad", (1, ci, _M, co)) for ci, co in ((64, 96), (128, 160), (256, 256))]


def _id(c):
    if not isinstance(c, tuple):
        return str(c)
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)


@pytest.mark.parametrize("case", PROBE_CASES, ids=_id)
def test_single_product_probe(cuda, case):
    """|C - a*b| <= 8 * 2^-24 |a*b| elementwise (module docstring, a)"""
    entry, (nb, M, K, N), role, scaled = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    A, B, want = R.probe_operands(rng, nb, M, K, N, role, scaled)
    C = ENTRY[entry](cuda, A, B)
    assert C.shape == want.shape
    assert np.isfinite(C).all()
    excess = R.probe_excess(C, want)
    print(f"x3acc probe {entry} ({nb},{M},{K},{N}) sparse={role} scaled={int(scaled)}: "
          f"max |C - ab| / |ab| = {excess:.2f} x 2^-24 (bar 8)")
    assert np.all(np.abs(C.astype(np.float64) - want) <= R.PROBE_BOUND * np.abs(want)), excess


@pytest.mark.parametrize("case", DENSE, ids=_id)
def test_dense_gemm_accuracy(cuda, case):
    """rms_rel(kernel) <= 2 * e32 against float64 (module docstring, b)"""
    entry, (nb, M, K, N) = case
    rng = np.random.default_rng(zlib.crc32(repr(case[1]).encode()))
    A = rng.standard_normal((nb, M, K)).astype(np.float32)
    B = rng.standard_normal((nb, K, N)).astype(np.float32)
    ref = np.matmul(A.astype(np.float64), B.astype(np.float64))
    e32 = R.e32_bmm(A, B, ref)
    C = ENTRY[entry](cuda, A, B)
    assert C.shape == ref.shape
    err = R.rms_rel(C, ref)
    print(f"x3acc dense {entry} ({nb},{M},{K},{N}): rms_rel {err:.3e}, e32 {e32:.3e}, ratio {err / e32:.2f} "
          f"(bar {R.DENSE_BAR:g})")
    assert err <= R.DENSE_BAR * e32, (err, e32)


# ---- c. the Winograd chain -------------------------------------------------------
WINO_CASES = [((8, 8, 8), 64, 64), ((8, 8, 8), 64, 128), ((7, 5, 9), 128, 64), ((16, 16, 32), 256, 256)]


class _WinoCase:
    """Inputs and host references of one conv, each computed once on first use"""

    def __init__(self, sp, K, N):
        rng = np.random.default_rng(K * 7 + N + sp[2])
        self.sp, self.K, self.N = sp, K, N
        self.x = rng.standard_normal(sp + (K,)).astype(np.float32)
        self.w = (rng.standard_normal((3, 3, 3, K, N)) / np.sqrt(27 * K)).astype(np.float32)
        self.dy = rng.standard_normal(sp + (N,)).astype(np.float32)
        self._direct = {}
        self._emu = {}

    def direct(self, dtype):
        """(y, dx, dw) of torch's CPU conv3d in dtype"""
        if dtype not in self._direct:
            xr = torch.from_numpy(self.x).to(dtype).requires_grad_(True)
            wr = torch.from_numpy(self.w).to(dtype).requires_grad_(True)
            y = Fn.conv3d(xr.permute(3, 0, 1, 2)[None], wr.permute(4, 3, 0, 1, 2), padding=1)[0].permute(1, 2, 3, 0)
            (y * torch.from_numpy(self.dy).to(dtype)).sum().backward()
            self._direct[dtype] = {"fwd": y.detach().numpy(), "dgrad": xr.grad.numpy(), "wgrad": wr.grad.numpy()}
        return self._direct[dtype]

    def yardsticks(self, kind, tile):
        """(float64 reference, eW at this tile, rms_rel of the CPU fp32 direct conv)"""
        ref = self.direct(torch.float64)[kind]
        if (kind, tile) not in self._emu:
            emu = {"fwd": lambda: R.wino_fwd(self.x, self.w, tile),
                   "dgrad": lambda: R.wino_dgrad(self.dy, self.w, tile),
                   "wgrad": lambda: R.wino_wgrad(self.x, self.dy, tile)}[kind]()
            self._emu[kind, tile] = R.rms_rel(emu, ref)
        return ref, self._emu[kind, tile], R.rms_rel(self.direct(torch.float32)[kind], ref)


@pytest.fixture(scope="module", params=WINO_CASES, ids=_id)
def wino(request):
    return _WinoCase(*request.param)


@pytest.mark.parametrize("path", ["fwd", "fwd_keep+wgrad_u", "wgrad", "dgrad", "dgrad_vy4"])
def test_wino_chain_accuracy(cuda, wino, path):
    """rms_rel(kernel) <= 4 * eW against float64 (module docstring, c)"""
    from m3d import _lib
    L = _lib.load()
    p = _lib.ptr
    c = wino
    (H, W, D), K, N = c.sp, c.K, c.N
    x, w, dy = _dev(cuda, c.x), _dev(cuda, c.w), _dev(cuda, c.dy)
    nb = int(L.m3d_conv3d_wino_workspace_bytes(1, H, W, D, D, K, N))
    ws = torch.empty(nb // 4 + 1, device=cuda)
    st = _lib.stream()
    t_fwd = (int(L.m3d_conv3d_wino_tile_y()), int(L.m3d_conv3d_wino_tile_z()))
    t_wg = (int(L.m3d_conv3d_wino_tile_y()), int(L.m3d_conv3d_wino_wgrad_tile_z()))
    t_dg = (int(L.m3d_conv3d_wino_dgrad_tile_y()), int(L.m3d_conv3d_wino_dgrad_tile_z()))
    out = []                     # (label, kind, tile, result)
    if path == "fwd":
        y = torch.full(c.sp + (N,), float("nan"), device=cuda)
        _lib.check(L.m3d_conv3d_fwd_wino(p(x), 1, H, W, D, K, p(w), N, D, 1, None, None, None, None, 0, None, p(y),
                                         p(ws), nb, st), "fwd_wino")
        out.append(("fwd_wino", "fwd", t_fwd, y))
    elif path == "fwd_keep+wgrad_u":
        ub = int(L.m3d_conv3d_wino_u_bytes(1, H, W, D, K))
        assert ub > 0, "the forward keeps no transformed input in this build"
        u = torch.empty(ub // 4, device=cuda)
        y = torch.full(c.sp + (N,), float("nan"), device=cuda)
        _lib.check(L.m3d_conv3d_fwd_wino_keep(p(x), 1, H, W, D, K, p(w), N, D, 1, None, None, None, None, 0, None,
                                              p(y), p(u), p(ws), nb, st), "fwd_wino_keep")
        dw = torch.zeros((3, 3, 3, K, N), device=cuda)
        _lib.check(L.m3d_conv3d_bwd_weight_wino_u(p(u), p(dy), 1, H, W, D, K, N, D, 1, p(dw), p(ws), nb, st),
                   "bwd_weight_wino_u")
        out += [("fwd_wino_keep", "fwd", t_fwd, y), ("bwd_weight_wino_u", "wgrad", t_wg, dw)]
    elif path == "wgrad":
        dw = torch.zeros((3, 3, 3, K, N), device=cuda)
        _lib.check(L.m3d_conv3d_bwd_weight_wino(p(x), p(dy), 1, H, W, D, K, N, D, 1, p(dw), p(ws), nb, st),
                   "bwd_weight_wino")
        out.append(("bwd_weight_wino", "wgrad", t_wg, dw))
    elif path == "dgrad":
        dx = torch.full(c.sp + (K,), float("nan"), device=cuda)
        _lib.check(L.m3d_conv3d_bwd_data_wino(p(dy), p(w), 1, H, W, D, K, N, D, 1, p(dx), 0, p(ws), nb, st),
                   "bwd_data_wino")
        out.append(("bwd_data_wino", "dgrad", t_dg, dx))
    else:
        dx = torch.full(c.sp + (K,), float("nan"), device=cuda)
        _lib.check(L.m3d_conv3d_bwd_data_wino_vy(p(dy), p(w), 1, H, W, D, K, N, D, 1, p(dx), 0, p(ws), nb, 0, 4, st),
                   "bwd_data_wino_vy")
        out.append(("bwd_data_wino_vy(4)", "dgrad", (4, t_dg[1]), dx))
    torch.cuda.synchronize()
    failed = []
    for label, kind, tile, got in out:
        ref, eW, eD = c.yardsticks(kind, tile)
        err = R.rms_rel(got.cpu().numpy(), ref)
        print(f"x3acc wino {label} ({H},{W},{D}) {K}->{N} F({tile[0]}x2x{tile[1]}): rms_rel {err:.3e}, eW {eW:.3e}, "
              f"ratio {err / eW:.2f} (bar {R.WINO_BAR:g}); CPU fp32 direct conv {eD:.3e}, ratio {err / eD:.2f}")
        if not err <= R.WINO_BAR * eW:
            failed.append((label, err, eW))
    assert not failed, failed


# ---- d. the (2,2,1)-strided 1x1x1 weight gradient through m3d.nn --------------------
@pytest.mark.parametrize("strided_x3", [True, False], ids=["x3", "f32"])
@pytest.mark.parametrize("sp,cin,cout", R.STRIDED_CASES, ids=_id)
def test_strided_1x1_weight_gradient(cuda, sp, cin, cout, strided_x3, monkeypatch):
    """conv_bn_act at stride (2,2,1), B = 2, odd and even H / W: the kernel
    gradient within 2 * e32 (rms_rel; e32 from the same gradient by autograd in
    CPU fp32) on the split GEMM and within x3ref.STRIDED_F32_BAR * e32 on the f32
    implicit GEMM (its serial fp32 accumulation measured 2.18 x e32: see
    x3ref.STRIDED_F32_BAR), both within 1e-4 of the float64 gradient's scale;
    LAYER_LOG names the engine that ran it.  No BN or activation, so the output
    gradient reaches the weight-gradient kernel unchanged and the figure is
    that kernel's own."""
    import m3d.nn as mnn
    from oracle import model_ref as MR
    from test_gpu_conv import _Layer
    monkeypatch.setattr(mnn, "WGRAD1_STRIDED_X3", strided_x3)
    log = []
    monkeypatch.setattr(mnn, "LAYER_LOG", log)
    x, w, b, g = R.strided_case(sp, cin, cout)
    geo = mnn.conv_geom(sp, (1, 1, 1), (2, 2, 1), "valid")
    assert tuple(geo.out) == tuple(g.shape[1:4])
    layer = _Layer(w.to(cuda), b.to(cuda))
    xg = x.to(cuda).requires_grad_(True)
    y = mnn.conv_bn_act(xg, layer, geo, False)
    y.backward(g.to(cuda))
    mnn.join_wgrad()
    torch.cuda.synchronize()
    ref, e32 = R.strided_wgrad_refs(x, w, b, g)
    got = layer.kernel.grad.cpu().numpy()
    err = R.rms_rel(got, ref)
    mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    eng = [r[8] for r in log if r[0] == "conv1_wgrad"]
    bar = R.DENSE_BAR if strided_x3 else R.STRIDED_F32_BAR
    print(f"x3acc strided-1x1-wgrad {'x3' if strided_x3 else 'f32'} {sp} {cin}->{cout}: rms_rel {err:.3e}, "
          f"e32 {e32:.3e}, ratio {err / e32:.2f} (bar {bar:.3g}); max err / max|ref| {mx:.2e}; engine {eng}")
    assert eng == ["x3" if strided_x3 else "f32"], eng
    assert err <= bar * e32, (err, e32)
    assert mx <= 1e-4
    # the data gradient of the strided conv (zero at the skipped voxels) rides along
    xr = x.double().requires_grad_(True)
    MR.conv3d(xr, w.double(), b.double(), (2, 2, 1), "valid").backward(g.double())
    dx = xg.grad.double().cpu()
    assert float((dx - xr.grad).abs().max()) <= 1e-4 * float(xr.grad.abs().max())
