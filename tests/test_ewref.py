"""tests/ewref.py (the references of csrc/elementwise.hip's kernels) checked on
their own -- no GPU.  The pools against torch's max_pool3d on the -inf-padded
float64 input and the oracle's maxpool3d_same, the argmax and tie / NaN rules
against a scalar scan and a hand-computed case, the adjoints against autograd,
and the derived bound of the BN channel sums against a float32 replay of the
kernels' own summation order."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import ewref
from oracle import model_ref

F = np.float32
POOL_ALL = ewref.POOL_CASES + [ewref.POOL_MISALIGNED]
POOL_IDS = [c[0] for c in POOL_ALL]


def _finite(x):
    """the planted NaN / inf voxels replaced (torch's pool orders NaN differently)"""
    return np.where(np.isfinite(x), x, F(0.125)).astype(F)


def _torch_pool(xt, spatial, k, stride, pad, out):
    """max_pool3d of x [B,H,W,D,C] (a float64 tensor) padded with -inf: pad
    before as given, after as far as the last window reaches."""
    fp = []
    for n, kk, s, p, o in reversed(list(zip(spatial, k, stride, pad, out))):
        fp += [p, max((o - 1) * s + kk - n - p, 0)]
    y = TF.max_pool3d(TF.pad(xt.permute(0, 4, 1, 2, 3), fp, value=-math.inf), k, stride)
    return y.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("case", POOL_ALL, ids=POOL_IDS)
def test_maxpool_fwd_matches_torch(case):
    cid, C, k, stride, padding, spatial = case
    out, pad = ewref.pool_geometry(spatial, k, stride, padding)
    x = _finite(ewref.pool_input(cid, C, spatial))
    y, am = ewref.maxpool_fwd(x, k, stride, pad, out)
    assert y.dtype == F and am.dtype == np.uint8 and y.shape == (ewref.POOL_B, *out, C)
    xt = torch.from_numpy(x).double()
    want = _torch_pool(xt, spatial, k, stride, pad, out).numpy()
    assert want.shape == y.shape
    np.testing.assert_array_equal(y.astype(np.float64), want)
    if padding == "same":
        np.testing.assert_array_equal(y.astype(np.float64), model_ref.maxpool3d_same(xt, k, stride).numpy())
    # argmax by a scalar scan: it names an in-range tap holding the maximum, and no
    # earlier in-range tap holds a value as large (the first maximum wins)
    H, W, D = spatial
    for oy in range(out[0]):
        for ox in range(out[1]):
            for oz in range(out[2]):
                taps = []
                for ky in range(k[0]):
                    for kx in range(k[1]):
                        for kz in range(k[2]):
                            iy, ix, iz = (oy * stride[0] - pad[0] + ky, ox * stride[1] - pad[1] + kx,
                                          oz * stride[2] - pad[2] + kz)
                            if 0 <= iy < H and 0 <= ix < W and 0 <= iz < D:
                                taps.append(((ky * k[1] + kx) * k[2] + kz, x[:, iy, ix, iz, :]))
                ids = np.array([t[0] for t in taps])
                vals = np.stack([t[1] for t in taps])                    # [taps, B, C]
                first = ids[np.argmax(vals, axis=0)]                       # np.argmax: the first maximum
                np.testing.assert_array_equal(am[:, oy, ox, oz, :], first)


def test_maxpool_fwd_nan_inf_and_tie_rule():
    # hand-computed, window 3 along z with 'same' pad 1 on [1, nan, 2, -inf, -inf]
    x = np.array([1, np.nan, 2, -np.inf, -np.inf], F).reshape(1, 1, 1, 5, 1)
    y, am = ewref.maxpool_fwd(x, (1, 1, 3), (1, 1, 1), (0, 0, 1), (1, 1, 5))
    #   taps (pad, 1, nan): 1 initialises at kz = 1, nan > 1 is false
    #   (1, nan, 2): 2 replaces 1            (nan, 2, -inf): the first tap is NaN and stays
    #   (2, -inf, -inf): 2 at kz = 0         (-inf, -inf, pad): the first of the equal taps
    np.testing.assert_array_equal(y.reshape(-1), np.array([1, 2, np.nan, 2, -np.inf], F))
    np.testing.assert_array_equal(am.reshape(-1), [1, 2, 0, 0, 0])
    y, am = ewref.maxpool_fwd(np.array([np.inf, np.inf, 3, 3], F).reshape(1, 1, 1, 4, 1), (1, 1, 2), (1, 1, 2),
                              (0, 0, 0), (1, 1, 2))
    np.testing.assert_array_equal(y.reshape(-1), [np.inf, 3])
    np.testing.assert_array_equal(am.reshape(-1), [0, 0])


@pytest.mark.parametrize("cid", sorted(ewref.POOL_SPECIAL))
def test_planted_values_are_first_and_later_taps(cid):
    _, C, k, stride, padding, spatial = next(c for c in ewref.POOL_CASES if c[0] == cid)
    out, pad = ewref.pool_geometry(spatial, k, stride, padding)
    x = ewref.pool_input(cid, C, spatial)
    y, am = ewref.maxpool_fwd(x, k, stride, pad, out)
    for j, v in enumerate(ewref.SPECIAL_VALUES):
        vox = [s for s in ewref.special_voxels(cid) if s[5] is v or s[5] == v]
        assert len(vox) == 2
        hits = [h for s in vox for h in ewref.window_hits(s[1:4], spatial, k, stride, pad, out)]
        assert any(h[3] for h in hits) and any(not h[3] for h in hits), (cid, v)
    for b, iy, ix, iz, c, v in ewref.special_voxels(cid):
        assert x[b, iy, ix, iz, c] == v or (np.isnan(v) and np.isnan(x[b, iy, ix, iz, c]))
        for oy, ox, oz, first in ewref.window_hits((iy, ix, iz), spatial, k, stride, pad, out):
            got = y[b, oy, ox, oz, c]
            if np.isnan(v):          # a NaN wins exactly where it is the window's first tap
                assert np.isnan(got) == first
            elif v == np.inf:        # +inf wins unless a NaN came first
                assert got == np.inf or np.isnan(got)
            elif first:              # a leading -inf is replaced by any later finite tap
                assert got > -np.inf or np.isnan(got)
    assert np.isnan(y).any() and (y == np.inf).any()


@pytest.mark.parametrize("case", POOL_ALL, ids=POOL_IDS)
def test_maxpool_bwd_matches_autograd(case):
    cid, C, k, stride, padding, spatial = case
    out, pad = ewref.pool_geometry(spatial, k, stride, padding)
    rng = np.random.default_rng([7, C, *spatial])
    n = ewref.POOL_B * int(np.prod(spatial)) * C
    x = (rng.permutation(n).astype(np.float64) / n).astype(F).reshape(ewref.POOL_B, *spatial, C)   # no ties
    assert np.unique(x).size == n
    dy = (rng.integers(-16, 17, (ewref.POOL_B, *out, C)) / 8.0).astype(F)     # sums of <= 125 such are exact
    _, am = ewref.maxpool_fwd(x, k, stride, pad, out)
    dx = ewref.maxpool_bwd(dy, am, x.shape, k, stride, pad)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    _torch_pool(xt, spatial, k, stride, pad, out).backward(torch.from_numpy(dy).double())
    assert dx.dtype == F
    np.testing.assert_array_equal(dx.astype(np.float64), xt.grad.numpy())
    assert dx.astype(np.float64).sum() == dy.astype(np.float64).sum()


def test_maxpool_bwd_rejects_a_tap_outside_the_input():
    dy = np.ones((1, 1, 1, 2, 1), F)
    am = np.array([0, 0], np.uint8).reshape(1, 1, 1, 2, 1)      # output 0's tap kz = 0 is the 'same' pad
    with pytest.raises(ValueError):
        ewref.maxpool_bwd(dy, am, (1, 1, 1, 2, 1), (1, 1, 3), (1, 1, 1), (0, 0, 1))


def test_maxpool_bwd_summation_order():
    # one input voxel named by three outputs: ((1e8 + 1) - 1e8) in float32 is 0, any
    # other order gives 1 or 8
    dy = np.array([1e8, 1.0, -1e8], F).reshape(1, 1, 1, 3, 1)
    am = np.array([2, 1, 0], np.uint8).reshape(1, 1, 1, 3, 1)   # all three windows point at z = 1
    dx = ewref.maxpool_bwd(dy, am, (1, 1, 1, 3, 1), (1, 1, 3), (1, 1, 1), (0, 0, 1))
    np.testing.assert_array_equal(dx.reshape(-1), np.array([0, (F(1e8) + F(1)) + F(-1e8), 0], F))


@pytest.mark.parametrize("accumulate", [False, True])
def test_upsample221_bwd_matches_autograd(accumulate):
    rng = np.random.default_rng(11)
    shape = (2, 3, 5, 4, 8)
    d_up = (rng.integers(-64, 65, (2, 6, 10, 4, 8)) / 16.0).astype(F)
    d0 = (rng.integers(-64, 65, shape) / 16.0).astype(F) if accumulate else None
    src = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    up = model_ref.upsample221(src)
    assert tuple(up.shape) == d_up.shape
    up.backward(torch.from_numpy(d_up).double())
    want = src.grad.numpy() + (d0.astype(np.float64) if accumulate else 0.0)
    got = ewref.upsample221_bwd(d_up, d0)
    assert got.dtype == F
    np.testing.assert_array_equal(got.astype(np.float64), want)
    # the order: start value, then the taps (0,0), (0,1), (1,0), (1,1)
    t = np.array([[1.0, -1e8], [1e8, 1.0]], F).reshape(1, 2, 2, 1, 1)
    assert ewref.upsample221_bwd(t)[0, 0, 0, 0, 0] == ((F(0) + F(1)) + F(-1e8)) + F(1e8) + F(1)
    assert ewref.upsample221_bwd(t, np.full((1, 1, 1, 1, 1), 1e8, F))[0, 0, 0, 0, 0] == \
        (((F(1e8) + F(1)) + F(-1e8)) + F(1e8)) + F(1)


@pytest.mark.parametrize("hw", [(5, 4), (4, 5)])
def test_subsample221(hw):
    rng = np.random.default_rng([13, *hw])
    x = rng.normal(size=(2, *hw, 3, 8)).astype(F)
    y = ewref.subsample221_fwd(x)
    assert y.shape == (2, (hw[0] + 1) // 2, (hw[1] + 1) // 2, 3, 8)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    yt = xt[:, ::2, ::2]
    np.testing.assert_array_equal(y.astype(np.float64), yt.detach().numpy())
    dy = (rng.integers(-64, 65, y.shape) / 16.0).astype(F)
    dx0 = (rng.integers(-64, 65, x.shape) / 16.0).astype(F)
    yt.backward(torch.from_numpy(dy).double())
    got = ewref.subsample221_bwd(dy, dx0)
    np.testing.assert_array_equal(got.astype(np.float64), xt.grad.numpy() + dx0)
    keep = np.ones(x.shape, bool)
    keep[:, ::2, ::2] = False
    np.testing.assert_array_equal(got[keep], dx0[keep])


def test_bn_affine_formula():
    r, s, t = ewref.bn_affine([2.0, -1.0], [0.5, 0.25], [1.0, -3.0], [0.25, 3.75], 0.0)
    np.testing.assert_array_equal(r, [2.0, 1.0 / np.sqrt(3.75)])
    np.testing.assert_array_equal(s, [4.0, -1.0 / np.sqrt(3.75)])
    np.testing.assert_array_equal(t, [0.5 - 4.0, 0.25 - (-3.0) * (-1.0 / np.sqrt(3.75))])
    r, _, _ = ewref.bn_affine([1.0], [0.0], [0.0], [1.0], 1e-3)
    assert r[0] == 1.0 / np.sqrt(1.0 + float(F(1e-3)))


@pytest.mark.parametrize("relu,affine,acc", [(1, True, True), (0, False, False), (1, True, False), (0, True, True)])
def test_bn_act_bwd_matches_autograd(relu, affine, acc):
    M, C = 37, 12
    d = ewref.bn_case(M, C, relu, affine)
    g, dz, dres, sums, abs_sums = ewref.bn_act_bwd(d["dy"], d["y"], d["z"], relu, d["scale"], d["mean"], d["rstd"],
                                                    d["dres0"] if acc else None)
    assert g.dtype == F and dz.dtype == F and dres.dtype == F and sums.dtype == np.float64
    # y = act(z*scale + shift + res + bias) with scale = gamma*rstd, shift = beta - mean*scale;
    # the branch of the ReLU is the recorded y > 0, as in the kernel
    one = np.ones(C, F)
    rstd = torch.from_numpy(d["rstd"] if affine else one).double()
    mean = torch.from_numpy(d["mean"] if affine else 0 * one).double()
    gamma = (torch.from_numpy(d["scale"] if affine else one).double() / rstd).requires_grad_(True)
    beta = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    z = torch.from_numpy(d["z"]).double().requires_grad_(True)
    res = torch.zeros(M, C, dtype=torch.float64, requires_grad=True)
    pre = (z + bias) * (gamma * rstd) + (beta - mean * (gamma * rstd)) + res
    mask = torch.from_numpy(np.nan_to_num(d["y"], nan=-1.0) > 0).double() if relu else torch.ones(M, C).double()
    (pre * mask).backward(torch.from_numpy(d["dy"]).double())
    np.testing.assert_allclose(dz, z.grad.numpy(), rtol=2 ** -23, atol=0)
    np.testing.assert_allclose(dres, res.grad.numpy() + (d["dres0"] if acc else 0), rtol=2 ** -23, atol=0)
    tol = 1e-13 * abs_sums + 1e-300
    assert (np.abs(sums[0] - beta.grad.numpy()) <= tol[0]).all()
    assert (np.abs(sums[1] - gamma.grad.numpy()) <= 1e-13 * abs_sums[1] + 1e-13 * abs_sums[2]).all()
    # the bias enters through z: its gradient is sum dz
    assert (np.abs(sums[2] - bias.grad.numpy()) <= tol[2]).all()
    if relu:                        # y = 0.0, -0.0 and NaN pass nothing
        for i in range(3):
            assert g[i, i] == 0 and dz[i, i] == 0 and d["dy"][i, i] != 0
    assert (abs_sums >= np.abs(sums)).all()


def _gx(M, C):
    import m3d._lib as lib
    L = lib.load()
    nbytes = int(L.m3d_bn_act_bwd_workspace_bytes(M, C))
    assert nbytes % (12 * C) == 0
    return nbytes // (12 * C)


def test_bn_grid_shapes():
    """the cases reach what they are meant to reach"""
    geo = {(M, C): (*ewref.bn_grid(C), _gx(M, C)) for M, C, _, _ in ewref.BN_CASES}
    assert geo[(5, 4)] == (1, 256, 1, 1)
    assert geo[(300, 12)] == (4, 64, 1, 5)
    assert geo[(700, 1028)] == (256, 1, 2, 512)
    assert geo[(1100, 2048)] == (256, 1, 2, 512)
    assert geo[(40000, 64)] == (16, 16, 1, 1024)
    assert geo[(262444, 4)] == (1, 256, 1, 1024)
    passes = {k: -(-k[0] // (v[3] * v[1])) for k, v in geo.items()}
    assert passes == {(5, 4): 1, (300, 12): 1, (700, 1028): 2, (1100, 2048): 3, (40000, 64): 3, (262444, 4): 2}
    assert ewref._fold_serial_adds(1024) == 4 and ewref._fold_serial_adds(1) == 1
    assert ewref._fold_serial_adds(512) == 2 and ewref._fold_serial_adds(5) == 1


@pytest.mark.parametrize("M,C,relu,affine", ewref.BN_CASES)
def test_bn_sum_bound_holds_for_the_kernel_order(M, C, relu, affine):
    """The float32 replay of the kernels' summation order lies within the
    derived bound of the float64 sums, for every shape the GPU test uses and
    with non-zero destinations.  Largest error / bound ratio observed over the
    six cases: 0.035 (at (5, 4); 0.034 at (700, 1028), 0.031 at (1100, 2048),
    0.012 at (300, 12), below 0.003 at the two long ones)."""
    gx = _gx(M, C)
    d = ewref.bn_case(M, C, relu, affine)
    _, _, _, sums, abs_sums = ewref.bn_act_bwd(d["dy"], d["y"], d["z"], relu, d["scale"], d["mean"], d["rstd"])
    bound = ewref.bn_sum_bound(M, C, gx, abs_sums, d["dst0"])
    sim = ewref.bn_sums_simulated(d["dy"], d["y"], d["z"], relu, d["scale"], d["mean"], d["rstd"], gx, d["dst0"])
    err = np.abs(sim.astype(np.float64) - (sums + d["dst0"].astype(np.float64)))
    ratio = float((err / bound).max())
    print(f"bn_sums_simulated (M={M}, C={C}): depth {ewref.bn_sum_depth(M, C, gx)}, max err/bound {ratio:.4f}")
    assert (bound > 0).all()
    assert (err <= bound).all(), ratio
    assert ewref.bn_sum_depth(M, C, gx) * ewref.U <= 1e-5
    # without prior contents the replay equals a plain float32 column sum's value to the same bound
    sim0 = ewref.bn_sums_simulated(d["dy"], d["y"], d["z"], relu, d["scale"], d["mean"], d["rstd"], gx)
    assert (np.abs(sim0.astype(np.float64) - sums) <= ewref.bn_sum_bound(M, C, gx, abs_sums)).all()


def test_seg_sq_norm_and_bound():
    g = np.arange(-5, 6).astype(F)
    w = (2 * np.arange(11)).astype(F)
    assert ewref.seg_sq_norm(g, w, 0.5) == float(np.sum((np.arange(-5, 6) + np.arange(11)) ** 2))
    assert ewref.seg_sq_norm(g, w, 0.0) == 110.0
    rng = np.random.default_rng(17)
    g, w = rng.normal(size=40000).astype(F), rng.normal(size=40000).astype(F)
    l2 = F(0.01 / 40000)
    a = g + l2 * w
    for det in (False, True):
        assert ewref.norm_depth(40, 65, det) * ewref.U <= 1e-5
        # numpy's pairwise float32 sum is one more association the bound covers
        assert abs(float(np.sum(a * a)) - ewref.seg_sq_norm(g, w, l2)) <= ewref.norm_bound(g, w, l2, 65, det)
    assert ewref.norm_depth(40, 65, False) == 3 + 3 + 16 + 6 + 3 + 3 + 1
    assert ewref.norm_depth(40, 65, True) == 3 + 3 + 8 + 1 + 8
