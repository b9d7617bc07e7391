"""The accuracy bars of tests/test_gpu_x3_accuracy.py, proven on the host before
any GPU is involved: for every probe and dense case (the GPU test's shapes, or
a subset of the same kernels' shapes) the emulated bf16-split arithmetic
(tests/x3ref.py) passes the bar, and every single fault -- one of the six MFMA
terms dropped or issued twice, one operand's lo plane zero -- misses it by at
least 2x.  The dense bars may therefore never exceed half the smallest mutated
ratio of their case (asserted here against x3ref.DENSE_BAR / WINO_BAR)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import x3ref as R

MUT = R.mutations()


def test_split3_exact_and_order():
    """hi + mid + lo == x in float64 for normal inputs (24 significand bits in
    3 x 8), each plane a bf16 value; the chain's order is the kernels' (x3_mac)"""
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * np.exp(rng.standard_normal(200000) * 8)).astype(np.float32)
    x = np.concatenate([x, np.float32([1.0, -1.0, 3.0e38, -3.0e38, 2.0 ** -100, 1 + 2.0 ** -23, 1 - 2.0 ** -24])])
    h, m, lo = R.split3(x)
    assert np.array_equal(h + m + lo, x.astype(np.float64))
    for p in (h, m, lo):
        assert np.array_equal(R.bf16(p), p)
    assert R.TERMS == ("lo,hi", "mid,mid", "hi,lo", "mid,hi", "hi,mid", "hi,hi")
    assert len(MUT) == 14


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("role", ["a", "b"])
@pytest.mark.parametrize("K", [32, 40, 64, 96, 256, 300])
def test_probe_bar_separates(K, role, scaled):
    """Single-product probes (one nonzero per row of the sparse operand): the
    healthy chain is within 8 * 2^-24 of a*b elementwise -- the derived bar:
    the dropped mid*lo, lo*mid, lo*lo below 2^-24, six exact products, at most
    six accumulator roundings -- and every mutation is at least 2x outside."""
    rng = np.random.default_rng(K + (7 if role == "b" else 0))
    A, B, want = R.probe_operands(rng, 2, 300, K, 160, role, scaled)
    nonzeros = (A != 0).sum(2) if role == "a" else (B != 0).sum(1)
    assert np.all(nonzeros == 1)          # one product per output element
    run = lambda **kw: R.gemm_x3(A, B, **kw)                                        # noqa: E731
    healthy = R.probe_excess(run(), want)
    assert healthy <= 8.0, healthy
    worst = {lab: R.probe_excess(run(**kw), want) for lab, kw in MUT}
    print(f"probe K={K} sparse={role} scaled={scaled}: healthy {healthy:.2f}, "
          f"mildest fault {min(worst.values()):.0f} ({min(worst, key=worst.get)}) x 2^-24")
    assert min(worst.values()) >= 16.0, worst


@pytest.mark.parametrize("nb,M,K,N", [(2, 300, 32, 160), (2, 300, 64, 64), (2, 300, 96, 256), (2, 200, 40, 96),
                                     (2, 300, 256, 256), (2, 96, 300, 160), (2, 64, 2048, 96)])
def test_dense_gemm_bar_separates(nb, M, K, N):
    """Dense N(0,1) GEMMs (reduction 32 .. 2048: the 1x1x1 / point GEMMs' K, the
    weight gradients' rows): healthy emulation <= DENSE_BAR * e32 (e32: torch.bmm
    in CPU fp32), every mutation >= 2 * DENSE_BAR * e32."""
    rng = np.random.default_rng(K * 1000 + N)
    A = rng.standard_normal((nb, M, K)).astype(np.float32)
    B = rng.standard_normal((nb, K, N)).astype(np.float32)
    ref = np.matmul(A.astype(np.float64), B.astype(np.float64))
    e32 = R.e32_bmm(A, B, ref)
    healthy = R.rms_rel(R.gemm_x3(A, B), ref) / e32
    worst = {lab: R.rms_rel(R.gemm_x3(A, B, **kw), ref) / e32 for lab, kw in MUT}
    print(f"dense gemm ({nb},{M},{K},{N}): e32 {e32:.2e}, healthy {healthy:.2f}, "
          f"mildest fault {min(worst.values()):.1f} ({min(worst, key=worst.get)})")
    assert healthy <= R.DENSE_BAR, healthy
    assert min(worst.values()) >= 2 * R.DENSE_BAR, worst


def _conv_ref(x, w, dy):
    """float64 'same' conv, data gradient and weight gradient ([H,W,D,C] layouts)"""
    xr = torch.from_numpy(x).double().requires_grad_(True)
    wr = torch.from_numpy(w).double().requires_grad_(True)
    y = Fn.conv3d(xr.permute(3, 0, 1, 2)[None], wr.permute(4, 3, 0, 1, 2), padding=1)[0].permute(1, 2, 3, 0)
    (y * torch.from_numpy(dy).double()).sum().backward()
    return y.detach().numpy(), xr.grad.numpy(), wr.grad.numpy()


WINO_CPU_CASES = [((8, 8, 8), 64, 64), ((8, 8, 8), 64, 128), ((7, 5, 9), 128, 64)]


@pytest.fixture(scope="module", params=WINO_CPU_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def wino_case(request):
    sp, K, N = request.param
    rng = np.random.default_rng(K + N + sp[2])
    x = rng.standard_normal(sp + (K,)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 3, K, N)) / np.sqrt(27 * K)).astype(np.float32)
    dy = rng.standard_normal(sp + (N,)).astype(np.float32)
    return x, w, dy, _conv_ref(x, w, dy)


@pytest.mark.parametrize("path", ["fwd", "dgrad2", "dgrad4", "wgrad"])
def test_wino_bar_separates(wino_case, path):
    """The Winograd chain at the kernels' tiles (forward and weight gradient
    F(4x2x4), data gradient F(2x2x4) and, tile_y = 4, F(4x2x4)): the emulated
    split point GEMM <= WINO_BAR * eW (eW: the staged fp32 Winograd), every
    mutation >= 2 * WINO_BAR * eW."""
    x, w, dy, (y, dx, dw) = wino_case
    run, ref = {
        "fwd": (lambda g: R.wino_fwd(x, w, (4, 4), g), y),
        "dgrad2": (lambda g: R.wino_dgrad(dy, w, (2, 4), g), dx),
        "dgrad4": (lambda g: R.wino_dgrad(dy, w, (4, 4), g), dx),
        "wgrad": (lambda g: R.wino_wgrad(x, dy, (4, 4), g), dw),
    }[path]
    eW = R.rms_rel(run(R.gemm_f32), ref)
    healthy = R.rms_rel(run(R.gemm_x3), ref) / eW
    worst = {lab: R.rms_rel(run(lambda A, B, kw=kw: R.gemm_x3(A, B, **kw)), ref) / eW for lab, kw in MUT}
    print(f"wino {path} {x.shape[:3]} {x.shape[3]}->{dy.shape[3]}: eW {eW:.2e}, healthy {healthy:.2f}, "
          f"mildest fault {min(worst.values()):.1f} ({min(worst, key=worst.get)})")
    assert healthy <= R.WINO_BAR, healthy
    assert min(worst.values()) >= 2 * R.WINO_BAR, worst


def test_wino_emulation_is_the_conv():
    """the staged emulation in float64-exact stages is the conv itself (tiling,
    padding, flips and transposes right): ragged grid, both tiles"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 3, 6, 8)).astype(np.float32)
    w = rng.standard_normal((3, 3, 3, 8, 12)).astype(np.float32)
    dy = rng.standard_normal((5, 3, 6, 12)).astype(np.float32)
    y, dx, dw = _conv_ref(x, w, dy)
    for tile in ((4, 4), (2, 4), (2, 2)):
        assert R.rms_rel(R.wino_fwd(x, w, tile), y) < 2e-6
        assert R.rms_rel(R.wino_dgrad(dy, w, tile), dx) < 2e-6
        assert R.rms_rel(R.wino_wgrad(x, dy, tile), dw) < 2e-6


@pytest.mark.parametrize("sp,cin,cout", R.STRIDED_CASES)
def test_strided_wgrad_bars_separate(sp, cin, cout):
    """The (2,2,1)-strided 1x1x1 weight gradient dW = x[:, ::2, ::2]^T g against
    its own e32 (autograd in CPU fp32): the split form's emulation <= DENSE_BAR;
    the f32 form as a serial fp32 FMA chain (one rounding per product, the
    v_mfma_f32_32x32x2_f32 accumulation) explains the ratio measured on the GPU
    and sits under STRIDED_F32_BAR; that bar stays under half the mildest
    mutated ratio, so neither form's bar lets a faulty split GEMM through."""
    x, w, b, g = R.strided_case(sp, cin, cout)
    ref, e32 = R.strided_wgrad_refs(x, w, b, g)
    ref = ref[0, 0, 0]
    A = x[:, ::2, ::2].reshape(-1, cin).numpy().T[None]
    B = g.reshape(-1, cout).numpy()[None]
    healthy = R.rms_rel(R.gemm_x3(A, B)[0], ref) / e32
    serial = R.rms_rel(R.gemm_f32(A, B, chunk=1)[0], ref) / e32
    worst = {lab: R.rms_rel(R.gemm_x3(A, B, **kw)[0], ref) / e32 for lab, kw in MUT}
    print(f"strided wgrad {sp} {cin}->{cout}: e32 {e32:.2e}, split emulation {healthy:.2f}, serial fp32 chain "
          f"{serial:.2f}, mildest fault {min(worst.values()):.1f} ({min(worst, key=worst.get)})")
    assert healthy <= R.DENSE_BAR, healthy
    assert serial <= R.STRIDED_F32_BAR, serial
    assert R.DENSE_BAR <= R.STRIDED_F32_BAR <= min(worst.values()) / 2, worst
