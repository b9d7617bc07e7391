"""Every reachable path of the implicit-GEMM half of csrc/conv3d.hip (forward,
data gradient, weight gradient, 2x2x2 deconv, plain / batched GEMM, split-K)
at the smallest shapes that cross its edges, through the C entries, against
the float64 references of tests/convref.py.

Acceptance, for every compared tensor, both of
1. max |got - ref| <= 1e-4 of the reference's largest magnitude (the project's
   criterion, close() of tests/test_gpu_conv.py);
2. element by element |got - ref| <= (6K + 16) 2^-24 sum|a||b| carried through
   the epilogue's own operations (convref's module docstring derives it; for a
   weight gradient K is the number of reduced rows and every split adds one
   rounding).  Nothing is taken from the kernels' output.
A ReLU is 1-Lipschitz, so bound 2 holds through it without choosing a branch;
tests/test_convref.py asserts that at most 0.1 % of any case's pre-activations
lie within the bound of zero and that both branches are taken.  The sigmoid
cases (the device's expf has no documented rounding here) are held to bound 2
at the pre-activation (z_out) and to criterion 1 after it; the sigmoid deconv
has no z_out, and the same tile is held to bound 2 by its act 0 / 1 twins.
Copied or scattered structure is exact: every destination sits between guard
bands and is pre-filled with NaN (or, where the call accumulates, with
non-zero random values), so an element never written, a write outside the
tensor, a touched column beyond Cout or a touched voxel that a strided scatter
does not cover all fail.

Which case reaches which instantiation (computed, not only claimed:
convref.all_paths, compared with the written-out list in tests/test_convref.py)

conv_gemm_kernel<BM x BN, A^T B ("nt": forward, GEMM, split-K forward) or
A B^T ("bt": data gradient, deconv), A loader, MFMA form, grid>:
* 128x32  nt avec f32 grid     test_fwd[t128x32-avec] [dil2-res3-bn-relu] [dil123] [aniso-k132]
                                [split-2-4-sigmoid] [split-5-8-sigmoid] [split-2-8-sigmoid], test_gemm[shared-ab] [grid-n32-bias]
* 128x32  nt avec f32 persist  test_gemm[persist-n32]
* 128x64  nt avec x3 grid      test_fwd[t128x64-bn-relu-z] [res2-relu] [ldy48-res1] [ldy38-res1-z]
                                [ldy38-res3-relu], test_gemm[grid-n64-bias], test_splitk_fwd[s2-res2, s4, s8]
* 128x64  nt avec x3 persist   test_gemm[persist-n64]
* 64x128  nt avec x3 grid      test_fwd[t64x128-res1-relu] (epi_store4_pre) [t64x128-plain] (epi_store4),
                                test_gemm[acc-bias-relu] (epi_store4_pre, accumulate), test_splitk_fwd[s2-res1-n512]
* 128x128 nt avec x3 grid      test_fwd[t128x128-big] (528 blocks, ragged last row tile), test_gemm[grid-n132-bias]
* 128x128 nt avec x3 persist   test_gemm[persist-n132] (5 rows x 132 columns a batch: ragged both ways)
* 128x32  nt scalar f32 grid   test_fwd[scalar-c48-k111] [scalar-stem-c32]
* 128x64  nt scalar f32 grid   test_fwd[scalar-c3-k333] [scalar-stem-s111], test_gemm[novec-k40-lda44]
* 64x128  nt scalar f32 grid   test_fwd[scalar-c6-n132]
* 128x128 nt scalar f32 grid   test_fwd[scalar-c4-big]
* 128x32  bt avec x3 persist   test_splitk_bwd_persist[bwd-s8-persist-c4]
* 128x64  bt avec x3 persist   test_splitk_bwd_persist[bwd-s64-persist-c36]
* 128x128 bt avec x3 persist   test_splitk_bwd_persist[bwd-s64-persist-wide] (5 rows, last column tile 4 wide)
* 128x32  bt avec x3 grid      test_bwd_data[flip-c4] [valid] [k133] [s221] [s222] [s112], test_deconv[n32-relu],
                                test_splitk_bwd[s8]
* 128x64  bt avec x3 grid      test_bwd_data[flip-c64], test_deconv[n64-none], test_splitk_bwd[s2-acc, s4-*]
* 64x128  bt avec x3 grid      test_bwd_data[flip-c132], test_deconv[n288-*]
* 128x128 bt avec x3 grid      test_deconv[n256-big-relu]
  epilogue: epi_store (scalar: split, ldy % 4) at the split and ldy38 cases; epi_store4 elsewhere;
  epi_store4_pre at res_mode 1 / accumulate with simple rows; the strided and deconv out_row at
  test_bwd_data[s*] and test_deconv; res_mode 2 at [res2-relu] and test_splitk_fwd[s2-res2-relu];
  res_mode 3 at [dil2-res3-bn-relu] [ldy38-res3-relu] and test_splitk_fwd[s4-res3-bn-relu].
splitk_epi_kernel: every test_splitk_fwd / test_splitk_bwd case.  splitk_reduce_kernel: test_splitk_reduce.
conv_wgrad_kernel<BI, BJ, A loader> (test_bwd_weight, every case in the modes atomic / det / det-small /
det-fit2 = fp32 atomics / scratch for all splits / scratch below two splits / scratch for exactly two):
* <64,64,vec>      [w64x64-m16] (M < 32) [x3-below-n64] (Cout 64, below M3D_TUNE_WGRAD1_X3_MIN_N = 65)
* <64,128,vec>     [w64x128-m1064] (384 + 384 + 296 rows; det-fit2: 544 + 520)
* <128,64,vec>     [w128x64-vec-m1024] (2 x 512)        * <128,64,scalar>  [w128x64-scalar]
* <128,128,vec>    [w128x128-vec] (K = 972, N = 132)     * <128,128,scalar> [w128x128-scalar]
x3_wgrad64_kernel<2> [x3-64-n68] [x3-64-m1064]; x3_wgrad_kernel<2> [x3-128-n68] [x3-128-m1064];
x3_wgrad_tr_kernel<0> [x3-tr-m420] and [x3-tr-m1064] in the det modes; x3_wgrad_tr_kernel<0, true>
(stream-K) [x3-tr-m1064-atomic].  Cout = 65 itself is no legal Cout (Cout % 4); 68 is the smallest at
or above the threshold and 64 the multiple of 4 below it.
wg_reduce_kernel: the det / det-fit2 modes of every case with M > 512; the "plain" single writer: every
det-small mode and the det modes of the single-split cases.

Not run here (tests/test_convref.py lists them with the reasons): the persistent 64x128 forms, which the
library holds and dispatch_gemm never picks (forms that no launch site names -- BK = 64, the non-split
forms of the vector loader at BT or BN >= 64 -- are not in the library); the fused-BN forms (tests/test_gpu_bnfuse.py); the HALO forms (tests/test_gpu_slab_halo.py); the stem
kernels.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import convref as R

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
EINVAL = -1


# --------------------------------------------------------------------------- helpers
def dev_in(a, dev):
    return torch.from_numpy(np.array(a, F, order="C")).to(dev)


class Dst:
    """rows x ld floats between two guard bands of four rows, 16-byte aligned,
    pre-filled with NaN or with `init`"""

    def __init__(self, rows, ld, dev, init=None):
        self.n, self.g = rows * ld, 4 * ld
        self.buf = torch.full((self.n + 2 * self.g,), NAN, dtype=torch.float32, device=dev)
        self.t = self.buf[self.g:self.g + self.n]
        if init is not None:
            self.t.copy_(dev_in(np.asarray(init).reshape(-1), dev))
        assert self.t.data_ptr() % 16 == 0
        self.rows, self.ld = rows, ld

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        """the tensor as numpy [rows, ld], after checking the guard bands"""
        torch.cuda.synchronize()
        guard = torch.cat([self.buf[:self.g], self.buf[self.g + self.n:]])
        assert bool(torch.isnan(guard).all()), "a write outside the destination"
        return self.t.cpu().numpy().reshape(self.rows, self.ld)

    def untouched(self):
        return bool(np.isnan(self.get()).all())


def compare(got, ref, err, what):
    """criterion 1, and bound 2 where `err` is given"""
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    assert np.isfinite(got).all(), what + ": an element was never written (NaN) or overflowed"
    d = np.abs(got - ref)
    scale = float(np.abs(ref).max())
    worst = float((d / (err + 1e-300)).max()) if err is not None else float("nan")
    print("%s: max err %.3e, 1e-4 of scale %.3e, largest err / bound %.3f" % (what, d.max(), 1e-4 * scale, worst))
    assert float(d.max()) <= 1e-4 * scale, what
    if err is not None:
        assert bool((d <= err + 1e-37).all()), what + ": past the rounding bound"


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def env(cuda):
    import m3d._lib as lib
    return lib.load(), lib, cuda


cached = functools.lru_cache(maxsize=None)      # small cases only: a reference is computed once and shared
_fwd_small = cached(lambda cid: R.fwd_data(next(c for c in R.FWD_CASES if c["id"] == cid)))


def fwd_data(cid):
    return (R.fwd_data(next(c for c in R.FWD_CASES if c["id"] == cid)) if cid.endswith("big") else _fwd_small(cid))


bwd_data = cached(lambda cid: R.bwd_data_data(next(c for c in R.BWD_DATA_CASES if c[0] == cid)))
wgrad_data = cached(lambda cid: R.wgrad_data(next(c for c in R.WGRAD_CASES if c[0] == cid)))
deconv_data = cached(lambda cid: R.deconv_data(next(c for c in R.DECONV_CASES if c[0] == cid)))


# --------------------------------------------------------------------------- forward
def run_fwd(env, c, d, splitk=None, ws_short=0, geom_override=None):
    """m3d_conv3d_fwd / _dil (or _fwd_splitk with splitk = splits) on case c; returns (rc, y, y2, z, ws)"""
    L, lib, dev = env
    B, (H, W, D), cin, cout, k = c["B"], c["sp"], c["cin"], c["cout"], c["k"]
    out, pad = geom_override or (d["out"], d["pad"])
    M = B * math.prod(out)
    C, cp = c["split"] or (0, 0)
    ldy = C or c["ldy"] or cout
    x, w = dev_in(d["x"], dev), dev_in(d["w"], dev)
    b, sc, sh = (None if d[n] is None else dev_in(d[n], dev) for n in ("bias", "scale", "shift"))
    res = None
    if c["res_mode"] in (1, 3):           # read with the output's row stride; the pad columns hold NaN
        r = np.full((M, ldy), NAN, F)
        r[:, :cout] = d["res"].reshape(M, cout)
        res = dev_in(r, dev)
    elif c["res_mode"] == 2:
        res = dev_in(d["res"], dev)
    y = Dst(M, ldy, dev)
    y2 = Dst(M, cp - C, dev) if C else None
    z = Dst(M, cout, dev) if c["z"] else None
    st = lib.stream()
    if splitk:
        ws = Dst(splitk * M, cout, dev)
        rc = L.m3d_conv3d_fwd_splitk(x.data_ptr(), B, H, W, D, cin, w.data_ptr(), cout, *out, *c["stride"], ptr(b),
                                     ptr(sc), ptr(sh), ptr(res), c["res_mode"], c["act"], z and z.ptr(), y.ptr(),
                                     splitk, ws.ptr(), ws.n * 4 - ws_short, st)
        return rc, y, y2, z, ws
    if c["dil"] == (1, 1, 1) and c["res_mode"] != 3:
        rc = L.m3d_conv3d_fwd(x.data_ptr(), B, H, W, D, cin, w.data_ptr(), *k, cout, *out, *c["stride"], *pad, ptr(b),
                              ptr(sc), ptr(sh), ptr(res), c["res_mode"], c["act"], z and z.ptr(), y.ptr(),
                              c["ldy"] if not C else C, y2 and y2.ptr(), cp - C, C, st)
    else:
        rc = L.m3d_conv3d_fwd_dil(x.data_ptr(), B, H, W, D, cin, w.data_ptr(), *k, cout, *out, *c["stride"], *pad,
                                  *c["dil"], ptr(b), ptr(sc), ptr(sh), ptr(res), c["res_mode"], c["act"],
                                  z and z.ptr(), y.ptr(), c["ldy"], None, 0, 0, st)
    return rc, y, y2, z, None


def check_fwd(c, d, y, y2, z):
    cid, cout = c["id"], c["cout"]
    C = c["split"][0] if c["split"] else 0
    got = y.get()
    n = C or cout
    compare(got[:, :n], d["y"].reshape(-1, n), None if d["yerr"] is None else d["yerr"].reshape(-1, n), cid + " y")
    assert np.isnan(got[:, n:]).all(), "columns beyond Cout touched"
    if C:
        compare(y2.get(), d["y2"].reshape(-1, cout - C), None, cid + " y2")
    if z is not None:
        compare(z.get(), d["z"].reshape(-1, cout), d["zerr"].reshape(-1, cout), cid + " z_out")


@pytest.mark.parametrize("cid", [c["id"] for c in R.FWD_CASES])
def test_fwd(env, cid):
    c = next(c for c in R.FWD_CASES if c["id"] == cid)
    d = fwd_data(cid)
    if cid.startswith("scalar-stem"):         # both must miss the stem kernel (Cout 32; stride 1)
        assert c["cin"] == 1 and c["k"] == R.K7 and (c["cout"] != 64 or c["stride"] != R.S221)
    rc, y, y2, z, _ = run_fwd(env, c, d)
    env[1].check(rc, cid)
    check_fwd(c, d, y, y2, z)
    if c["split"]:                            # y2 holds exactly the columns from split_n on, y the ones before
        assert y.ld == c["split"][0] and y2.ld == c["split"][1] - c["split"][0]


def test_fwd_rejections(env):
    L = env[0]
    c = dict(next(c for c in R.FWD_CASES if c["id"] == "res2-relu"))
    c["sp"] = (5, 6, 3)                       # OH odd: no (2,2,1)-upsampled residual
    d = dict(fwd_data("res2-relu"))
    d["x"] = np.zeros((2, 5, 6, 3, c["cin"]), F)
    rc, y, _, _, _ = run_fwd(env, c, d, geom_override=((5, 6, 3), (0, 0, 0)))
    assert rc == EINVAL and b"even OH/OW" in L.m3d_last_error() and y.untouched()
    c = dict(next(c for c in R.FWD_CASES if c["id"] == "t128x32-avec"), cout=22)
    rc, y, _, _, _ = run_fwd(env, c, fwd_data("t128x32-avec"))
    assert rc == EINVAL and b"multiple of 4" in L.m3d_last_error() and y.untouched()


# --------------------------------------------------------------------------- data gradient
def run_bwd_data(env, shape, cout, k, stride, pad, out, d, acc, splitk=None, ws_short=0):
    """m3d_conv3d_bwd_data (or _splitk); dx pre-filled as the contract says: an
    accumulated dx with values; an overwritten one with NaN where the conv
    covers it, and with the caller's zeros (include/m3d.h: "dx zeroed by the
    caller for strided ones", m3d/nn.py allocates it with torch.zeros) at the
    voxels a strided 1x1x1 conv never reads.  Deliberately so: the contract
    lets the kernel leave those voxels alone or write 0 to them, and a zero
    pre-fill accepts both; accumulate = 1 pins "left alone" bit for bit."""
    L, lib, dev = env
    B, H, W, D, cin = shape
    dz, w = dev_in(d["dz"], dev), dev_in(d["w"], dev)
    cov = np.broadcast_to(d["covered"][..., None], shape)
    init = d["dx0"] if acc else np.where(cov, F(NAN), F(0))
    dx = Dst(B * H * W * D, cin, dev, init)
    if splitk:
        ws = Dst(splitk * B * math.prod(out), cin, dev)
        rc = L.m3d_conv3d_bwd_data_splitk(dz.data_ptr(), w.data_ptr(), B, H, W, D, cin, cout, *out, *stride, dx.ptr(),
                                          acc, splitk, ws.ptr(), ws.n * 4 - ws_short, lib.stream())
        return rc, dx, ws
    rc = L.m3d_conv3d_bwd_data(dz.data_ptr(), w.data_ptr(), B, H, W, D, cin, *k, cout, *out, *stride, *pad, dx.ptr(),
                               acc, lib.stream())
    return rc, dx, None


def check_bwd_data(what, shape, d, acc, dx):
    got = dx.get().reshape(shape)
    cov = d["covered"]
    ref, err = d["dx"], d["err"]
    if acc:
        ref = ref + d["dx0"]
        err = R._round(ref, err)
        assert same_bits(got[~cov], d["dx0"][~cov]), "an uncovered voxel of an accumulated dx changed"
    else:
        assert same_bits(got[~cov], np.zeros_like(got[~cov])), "an uncovered voxel is not the caller's zero"
    compare(got[cov], ref[cov], err[cov], what)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("cid", [c[0] for c in R.BWD_DATA_CASES])
def test_bwd_data(env, cid, acc):
    _, cin, cout, k, stride, padding, sp = next(c for c in R.BWD_DATA_CASES if c[0] == cid)
    d = bwd_data(cid)
    shape = (R.BWD_B, *sp, cin)
    rc, dx, _ = run_bwd_data(env, shape, cout, k, stride, d["pad"], d["out"], d, acc)
    env[1].check(rc, cid)
    check_bwd_data("%s acc %d" % (cid, acc), shape, d, acc, dx)


@pytest.mark.parametrize("what,cin,cout,k,stride,pad,msg", [
    ("strided-k333", 8, 32, R.K3, (2, 2, 1), (1, 1, 1), b"1x1x1 kernels only"),
    ("padded-k111", 8, 32, R.K1, R.S1, (1, 0, 0), b"padding unsupported"),
    ("cout-36", 8, 36, R.K3, R.S1, (1, 1, 1), b"Cout must be a multiple of 32"),
    ("cin-6", 6, 32, R.K3, R.S1, (1, 1, 1), b"Cin must be a multiple of 4"),
])
def test_bwd_data_rejections(env, what, cin, cout, k, stride, pad, msg):
    L, lib, dev = env
    sp = (5, 4, 3)
    out = tuple(R.cdiv(n, s) for n, s in zip(sp, stride))
    dz = torch.zeros((2, *out, cout), device=dev)
    w = torch.zeros((*k, cin, cout), device=dev)
    dx = Dst(2 * math.prod(sp), cin, dev)
    rc = L.m3d_conv3d_bwd_data(dz.data_ptr(), w.data_ptr(), 2, *sp, cin, *k, cout, *out, *stride, *pad, dx.ptr(), 0,
                               lib.stream())
    assert rc == EINVAL and msg in L.m3d_last_error(), L.m3d_last_error()
    assert dx.untouched()                     # nothing was launched


# --------------------------------------------------------------------------- weight gradient
def run_bwd_weight(env, c, d, mode):
    """dw (pre-filled with dw0) and the deterministic scratch, both guarded"""
    L, lib, dev = env
    cid, cin, cout, k, stride, padding, sp = c
    x, dz = dev_in(d["x"], dev), dev_in(d["dz"], dev)
    dw = Dst(math.prod(k) * cin, cout, dev, d["dw0"])
    det, scratch = None, None
    if mode != "atomic":
        floats = R.wgrad_scratch_floats(c, mode)
        scratch = Dst(R.cdiv(floats, 256), 256, dev)
        det = lib.Det(1, scratch.ptr(), floats * 4)
    rc = L.m3d_conv3d_bwd_weight(x.data_ptr(), dz.data_ptr(), 2, *sp, cin, *k, cout, *d["out"], *stride, *d["pad"],
                                 dw.ptr(), ctypes.addressof(det) if det else None, lib.stream())
    lib.check(rc, cid)
    got = dw.get().reshape(d["dw"].shape)
    if scratch is not None:
        scratch.get()                         # its guard bands
    return got


@pytest.mark.parametrize("mode", R.WGRAD_MODES)
@pytest.mark.parametrize("cid", [c[0] for c in R.WGRAD_CASES])
def test_bwd_weight(env, cid, mode):
    c = next(c for c in R.WGRAD_CASES if c[0] == cid)
    d = wgrad_data(cid)
    _, target, splits, _ = R.wgrad_path_of(c, mode, torch.cuda.get_device_properties(env[2]).multi_processor_count)
    got = run_bwd_weight(env, c, d, mode)
    compare(got, d["dw"], R.wgrad_bound(d["M"], d["absprod"], d["dw0"], splits), "%s %s dw0 + dw" % (cid, mode))
    if mode != "atomic":                      # the ordered reduce and the single writer: the same bits again
        assert target in ("reduce", "plain")
        assert same_bits(run_bwd_weight(env, c, d, mode), got), "deterministic mode differs between two calls"


# --------------------------------------------------------------------------- deconv
@pytest.mark.parametrize("cid", [c[0] for c in R.DECONV_CASES])
def test_deconv(env, cid):
    L, lib, dev = env
    _, B, sp, cin, cout, act = next(c for c in R.DECONV_CASES if c[0] == cid)
    d = deconv_data(cid)
    x, w, b = dev_in(d["x"], dev), dev_in(d["w"], dev), dev_in(d["bias"], dev)
    y = Dst(8 * B * math.prod(sp), cout, dev)
    lib.check(L.m3d_deconv3d_k2s2(x.data_ptr(), B, *sp, cin, w.data_ptr(), cout, b.data_ptr(), act, y.ptr(),
                                  lib.stream()), cid)
    compare(y.get(), d["y"].reshape(-1, cout), None if d["yerr"] is None else d["yerr"].reshape(-1, cout), cid)


@pytest.mark.parametrize("cin,cout", [(48, 8), (32, 6)])
def test_deconv_rejections(env, cin, cout):
    L, lib, dev = env
    x = torch.zeros((1, 2, 2, 2, cin), device=dev)
    w = torch.zeros((2, 2, 2, cout, cin), device=dev)
    y = Dst(64, cout, dev)
    rc = L.m3d_deconv3d_k2s2(x.data_ptr(), 1, 2, 2, 2, cin, w.data_ptr(), cout, None, 0, y.ptr(), lib.stream())
    assert rc == EINVAL and b"Cout % 4 == 0 and Cin % 32 == 0" in L.m3d_last_error() and y.untouched()


# --------------------------------------------------------------------------- plain and batched GEMM
@pytest.mark.parametrize("cid", [c[0] for c in R.GEMM_CASES])
def test_gemm(env, cid):
    L, lib, dev = env
    c = next(c for c in R.GEMM_CASES if c[0] == cid)
    _, batch, M, K, N, lda, shared, bias, act, acc = c
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    d = R.gemm_data(c, ncu)
    batch = d["batch"]
    if c[1] is None:                          # the persistent size, and its twin with a bias on the grid form
        want = "grid" if bias else "persist"
        assert R.gemm_case_path(c, ncu)[6] == want and batch == R.persist_batch(ncu, M, N)
    A = np.array(d["A"])
    A[..., K:] = NAN                          # the rows' padding up to lda is no operand
    A, Bm = dev_in(A, dev), dev_in(d["B"], dev)
    b = dev_in(d["bias"], dev) if bias else None
    Cd = Dst(batch * M, N, dev, d["c0"])
    lib.check(L.m3d_gemm_f32_ex(A.data_ptr(), lda, 0 if shared else M * lda, Bm.data_ptr(), 0 if shared else K * N,
                                Cd.ptr(), M * N, batch, M, K, N, ptr(b), act, acc, lib.stream()), cid)
    compare(Cd.get(), d["y"].reshape(-1, N), d["yerr"].reshape(-1, N), cid)


def test_splitk_reduce(env):
    L, lib, dev = env
    rng = np.random.default_rng(17)
    splits, M, N = 3, 67, 20                  # 1340 elements: five full blocks and a ragged one
    ws = rng.normal(size=(splits, M, N)).astype(F)
    bias, sc, sh = R.relu_bias(ws.sum(0), rng), rng.uniform(0.5, 1.5, N).astype(F), rng.normal(0, 0.1, N).astype(F)
    r = R.epilogue(ws.astype(np.float64).sum(0), splits * R.U * np.abs(ws).astype(np.float64).sum(0), bias, sc, sh,
                   act=1)
    out = Dst(M, N, dev)
    wsd, bd, scd, shd = (dev_in(a, dev) for a in (ws, bias, sc, sh))
    lib.check(L.m3d_splitk_reduce(wsd.data_ptr(), splits, M, N, bd.data_ptr(), scd.data_ptr(), shd.data_ptr(), 1,
                                  out.ptr(), lib.stream()))
    compare(out.get(), r["y"], r["yerr"], "splitk_reduce")


# --------------------------------------------------------------------------- split-K entries
splitk_fwd_data = cached(lambda cid: R.splitk_fwd_data(next(c for c in R.SPLITK_FWD_CASES if c[0] == cid)))
splitk_bwd_data = cached(lambda cid: R.splitk_bwd_data(next(c for c in R.SPLITK_BWD_CASES if c[0] == cid)))


@pytest.mark.parametrize("cid", [c[0] for c in R.SPLITK_FWD_CASES])
def test_splitk_fwd(env, cid):
    c = next(c for c in R.SPLITK_FWD_CASES if c[0] == cid)
    fc, d = R.splitk_fwd_case(c), splitk_fwd_data(cid)
    rc, y, _, z, ws = run_fwd(env, fc, d, splitk=c[1])
    env[1].check(rc, cid)
    check_fwd(fc, d, y, None, z)
    part = ws.get()                           # every slice wrote its whole plane, and only that
    assert np.isfinite(part).all()


@pytest.mark.parametrize("cid", [c[0] for c in R.SPLITK_BWD_CASES])
def test_splitk_bwd(env, cid):
    _, splits, cin, cout, stride, acc = next(c for c in R.SPLITK_BWD_CASES if c[0] == cid)
    d = splitk_bwd_data(cid)
    shape = (1, *d["sp"], cin)
    rc, dx, ws = run_bwd_data(env, shape, cout, R.K1, stride, (0, 0, 0), R.SPLITK_OUT, d, acc, splitk=splits)
    env[1].check(rc, cid)
    check_bwd_data(cid, shape, d, acc, dx)
    assert np.isfinite(ws.get()).all()


@pytest.mark.parametrize("cid", [c[0] for c in R.SPLITK_PERSIST_CASES])
def test_splitk_bwd_persist(env, cid):
    """more K-slices than m3d_conv3d_splitk_count would give, on enough rows that the slices' plain
    partial GEMMs pass 6 * CUs tiles: the persistent tile loop of the B^T (data-gradient) forms"""
    ncu = torch.cuda.get_device_properties(env[2]).multi_processor_count
    c, out = R.splitk_persist_geom(next(c for c in R.SPLITK_PERSIST_CASES if c[0] == cid), ncu)
    cid, splits, cin, cout, stride, acc = c
    assert R.splitk_paths(c, False, ncu, out)[0][6] == "persist"
    d = R.splitk_bwd_data(c, out)
    shape = (1, *out, cin)
    rc, dx, ws = run_bwd_data(env, shape, cout, R.K1, stride, (0, 0, 0), out, d, acc, splitk=splits)
    env[1].check(rc, cid)
    check_bwd_data(cid, shape, d, acc, dx)
    assert np.isfinite(ws.get()).all()


def test_splitk_rejections(env):
    L = env[0]
    c = R.SPLITK_FWD_CASES[0]
    fc, d = R.splitk_fwd_case(c), splitk_fwd_data(c[0])
    rc, y, _, _, ws = run_fwd(env, fc, d, splitk=c[1], ws_short=4)
    assert rc == EINVAL and b"workspace smaller" in L.m3d_last_error() and y.untouched() and ws.untouched()
    rc, y, _, _, ws = run_fwd(env, fc, d, splitk=32)            # Cin 512 is no multiple of 32 * 32
    assert rc == EINVAL and b"multiple of 32 * splits" in L.m3d_last_error() and y.untouched() and ws.untouched()
    b = R.SPLITK_BWD_CASES[3]
    d = splitk_bwd_data(b[0])
    shape = (1, *d["sp"], b[2])
    rc, dx, ws = run_bwd_data(env, shape, b[3], R.K1, b[4], (0, 0, 0), R.SPLITK_OUT, d, 0, splitk=b[1], ws_short=4)
    assert rc == EINVAL and b"workspace smaller" in L.m3d_last_error() and dx.untouched() and ws.untouched()
    rc, dx, ws = run_bwd_data(env, shape, b[3], R.K1, b[4], (0, 0, 0), R.SPLITK_OUT, d, 0, splitk=32)
    assert rc == EINVAL and b"multiple of 32 * splits" in L.m3d_last_error() and dx.untouched() and ws.untouched()
