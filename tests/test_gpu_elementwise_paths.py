"""Every kernel path of csrc/elementwise.hip at small shapes against
tests/ewref.py: the pools, the (2,2,1) resampling adjoints and the elementwise
outputs of the BN-ReLU backward bit for bit; the BN channel sums, the frozen-BN
affine and the optimizers' clip norms within bounds derived in ewref from the
kernels' rounding counts (never from their results); the optimizer updates
against oracle/optim_ref.py.

Which case reaches which path (the dispatch of m3d_maxpool3d_fwd / _bwd,
bn_grid, clip_norms):

* maxpool_fwd_kernel / maxpool_bwd_kernel (C % 4 != 0): test_maxpool[scalar-c6]
* the same by the alignment test (x, y, dy one float past a 16-byte boundary,
  the scalar case's geometry at C = 8, which aligned would take fwd333 /
  bwd333): test_maxpool_misaligned_falls_back_to_scalar
* maxpool_fwd333_kernel / maxpool_bwd333_kernel ((3,3,3)/(2,2,1) 'same',
  C % 4 == 0): test_maxpool[333-d1] (one plane), [333-d8] (one full run of 8),
  [333-d9] (a run of 8 and a run of 1; NaN / +inf / -inf planted), [333-d21]
  (a ragged third run); H and W odd and even, so both 'same' pads (1 and 0)
* maxpool_fwd4z_kernel<false> / maxpool_bwd4z_kernel<false> (sz == 1, not the
  stem's geometry): test_maxpool[4z-s111] (sy = sx = 1), [4z-k335] (kd = 5,
  pz = 2), [4z-valid] (no pad, OD = D - 2; NaN / +inf / -inf planted),
  [4z-k223] (even window, pad 0 before and 1 after), [4z-k111] (k = 1: must
  also equal subsample221)
* maxpool_fwd4_kernel<false> / maxpool_bwd4_kernel<false> (sz != 1):
  test_maxpool[4-k222-valid], [4-k222-same], [4-k333-s222]
* the Python padding arithmetic of nn.max_pool3d with autograd: every
  test_maxpool case ('valid' and sz = 2 among them)
* upsample221_bwd_kernel<uint32_t>, accumulate 0 and 1: test_upsample221_bwd.
  The int64-index instantiation needs >= 2^32 float4s (64 GiB): out of scope.
* subsample221_kernel, bwd 0 and 1: test_subsample221
* bn_affine_kernel: test_bn_affine (C = 1, 3, 257: a partial block, two blocks)
* bn_act_bwd_kernel + bn_sums_reduce_kernel: test_bn_act_bwd
  [5-4]        T = 1, R = 256 (251 rows idle), gx = 1, fold of one row
  [300-12]     T = 4 with an idle lane, R = 64, gx = 5; the 16-channel fold block
               has an idle quad; relu 0 with scale / mean / rstd NULL
  [700-1028]   two channel groups, the second with one quad; R = 1 (no LDS
               tree), gx = 512, two passes; 65 fold blocks, the last with one
               quad; dz NULL
  [1100-2048]  T = 256, R = 1, gx capped at 512, three passes (the last ragged)
  [40000-64]   gx = 1024 (the cap), three passes, four unrolled fold iterations
  [262444-4]   T = 1, a second pass of the 256-row blocks (rows 262144..262443)
  dres: accumulate_res 1 at [5-4] and [700-1028], 0 at [300-12] and
  [40000-64], NULL otherwise; every destination pre-filled.
* each sum alone, sums only (dz = dres = NULL, `part` set) and elementwise only
  (`part` NULL): test_bn_act_bwd_split_calls at (300, 12) and (700, 1028)
* sgd_norm_kernel with five blocks (a segment that starts at chunk 3 and ends
  in block 1, two whole segments inside block 1, a segment over three blocks),
  sgd_update_kernel, adaptive_update_kernel<0>, <1>, <2>:
  test_optimizer_steps[*-atomic]
* chunk_norm_kernel + seg_norm_kernel: test_optimizer_steps[*-deterministic]
* clipnorm = 0 (no norm pass, norms never read): test_optimizer_without_clipnorm
* the deterministic scratch check of clip_norms: test_deterministic_scratch_too_small

The halo forms of the pools are tied to these kernels by the equality tests of
test_gpu_slab_halo.py and are not repeated here.
"""
import functools

import numpy as np
import pytest
import torch

import ewref
from oracle import optim_ref as O

pytestmark = pytest.mark.gpu

F = np.float32
POOL_IDS = [c[0] for c in ewref.POOL_CASES]


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # a copy: the cached inputs are read-only


def _ro(a):
    a.setflags(write=False)
    return a


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def assert_bits(got, want, what=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


# --------------------------------------------------------------------------- max-pool
@functools.lru_cache(maxsize=None)
def _pool_ref(cid):
    _, C, k, stride, padding, spatial = next(c for c in ewref.POOL_CASES + [ewref.POOL_MISALIGNED] if c[0] == cid)
    out, pad = ewref.pool_geometry(spatial, k, stride, padding)
    x = ewref.pool_input(cid, C, spatial)
    y, am = ewref.maxpool_fwd(x, k, stride, pad, out)
    rng = np.random.default_rng([3, C, *spatial])
    dy = (rng.normal(size=y.shape) + 0.75).astype(F)         # both signs, and a sum far from 0
    dx = ewref.maxpool_bwd(dy, am, x.shape, k, stride, pad)
    return tuple(_ro(a) for a in (x, y, am, dy, dx)) + (out, pad)


def _offset_view(n, dev, fill, off):
    """n floats starting `off` floats into a 16-byte aligned buffer, guard floats either side"""
    buf = torch.full((n + 8,), fill, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:off + n]


def _pool_c_entry(dev, cid, k, stride, off):
    """(y, argmax, dx) of the C entries; off = 0: 16-byte aligned tensors, 1:
    x, y and dy one float past the boundary."""
    import m3d._lib as lib
    L = lib.load()
    x, y_ref, am_ref, dy, dx_ref, out, pad = _pool_ref(cid)
    shape = x.shape
    xb, xd = _offset_view(x.size, dev, 0.0, off)
    xd.copy_(T(x.reshape(-1), dev))
    yb, yd = _offset_view(y_ref.size, dev, float("nan"), off)
    am = torch.full(y_ref.shape, 255, dtype=torch.uint8, device=dev)
    assert xd.data_ptr() % 16 == 4 * off and yd.data_ptr() % 16 == 4 * off and am.data_ptr() % 4 == 0
    lib.check(L.m3d_maxpool3d_fwd(xd.data_ptr(), *shape, *k, *stride, *pad, *out, yd.data_ptr(), am.data_ptr(),
                                  lib.stream()), "maxpool3d_fwd")
    gb, gd = _offset_view(dy.size, dev, 0.0, off)
    gd.copy_(T(dy.reshape(-1), dev))
    dx = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    assert gd.data_ptr() % 16 == 4 * off and dx.data_ptr() % 16 == 0
    amd = T(am_ref, dev)
    lib.check(L.m3d_maxpool3d_bwd(gd.data_ptr(), amd.data_ptr(), *shape, *k, *stride, *pad, *out,
                                  dx.data_ptr(), lib.stream()), "maxpool3d_bwd")
    torch.cuda.synchronize()
    guard = torch.cat([yb[:off], yb[off + y_ref.size:]])
    assert bool(torch.isnan(guard).all()), "the pool wrote outside y"
    return yd.cpu().numpy().reshape(y_ref.shape), am.cpu().numpy(), dx.cpu().numpy()


def _check_pool(cid, y, am, dx):
    _, y_ref, am_ref, dy, dx_ref, _, _ = _pool_ref(cid)
    np.testing.assert_array_equal(y, y_ref)                  # NaNs compare equal
    np.testing.assert_array_equal(am, am_ref)
    assert_bits(dx, dx_ref, cid)
    # every output routes its gradient to exactly one in-range input
    sdy = dy.astype(np.float64).sum()
    assert abs(dx.astype(np.float64).sum() - sdy) <= 1e-6 * abs(sdy)


@pytest.mark.parametrize("case", ewref.POOL_CASES, ids=POOL_IDS)
def test_maxpool(cuda, case):
    from m3d import nn
    cid, C, k, stride, padding, spatial = case
    x, y_ref, am_ref, dy, dx_ref, out, pad = _pool_ref(cid)
    if cid in ewref.POOL_SPECIAL:
        assert np.isnan(y_ref).any() and np.isinf(y_ref).any()
    else:
        assert np.isfinite(x).all()
    _check_pool(cid, *_pool_c_entry(cuda, cid, k, stride, 0))
    # through nn.max_pool3d and autograd: the Python 'same' / 'valid' arithmetic
    xt = T(x, cuda).requires_grad_(True)
    yt = nn.max_pool3d(xt, k, stride, padding)
    assert tuple(yt.shape) == y_ref.shape
    yt.backward(T(dy, cuda))
    np.testing.assert_array_equal(yt.detach().cpu().numpy(), y_ref)
    assert_bits(xt.grad.cpu().numpy(), dx_ref, cid)
    if k == (1, 1, 1):                                       # P6's pool: the same as subsample221
        xs = T(x, cuda).requires_grad_(True)
        ys = nn.subsample221(xs)
        ys.backward(T(dy, cuda))
        assert_bits(ys.detach().cpu().numpy(), y_ref)
        assert_bits(xs.grad.cpu().numpy(), dx_ref)
        assert (am_ref == 0).all()


def test_maxpool_misaligned_falls_back_to_scalar(cuda):
    # the stem's geometry at C = 8 would take fwd333 / bwd333; one float past the
    # 16-byte boundary the float4 kernels must not run, and the results stay the same
    cid, C, k, stride, padding, spatial = ewref.POOL_MISALIGNED
    assert C == 8 and (k, stride, padding, spatial) == ewref.POOL_CASES[0][2:]
    _check_pool(cid, *_pool_c_entry(cuda, cid, k, stride, 1))


# --------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("accumulate", [0, 1])
def test_upsample221_bwd(cuda, accumulate):
    import m3d._lib as lib
    L = lib.load()
    B, H, W, D, C = 2, 3, 5, 4, 8
    rng = np.random.default_rng([21, accumulate])
    d_up = rng.normal(size=(B, 2 * H, 2 * W, D, C)).astype(F)
    d0 = rng.normal(size=(B, H, W, D, C)).astype(F) if accumulate else np.full((B, H, W, D, C), np.nan, F)
    dsrc, dupd = T(d0, cuda), T(d_up, cuda)
    lib.check(L.m3d_upsample221_bwd(dupd.data_ptr(), B, H, W, D, C, dsrc.data_ptr(), accumulate,
                                    lib.stream()), "upsample221_bwd")
    assert_bits(dsrc.cpu().numpy(), ewref.upsample221_bwd(d_up, d0 if accumulate else None))


@pytest.mark.parametrize("hw", [(5, 4), (4, 5)])
def test_subsample221(cuda, hw):
    import m3d._lib as lib
    L = lib.load()
    B, D, C = 2, 3, 8
    H, W = hw
    rng = np.random.default_rng([23, H, W])
    x = rng.normal(size=(B, H, W, D, C)).astype(F)
    want = ewref.subsample221_fwd(x)
    y = torch.full(want.shape, float("nan"), dtype=torch.float32, device=cuda)
    xd = T(x, cuda)
    lib.check(L.m3d_subsample221_fwd(xd.data_ptr(), B, H, W, D, C, y.data_ptr(), lib.stream()), "subsample221")
    assert_bits(y.cpu().numpy(), want)
    dy = rng.normal(size=want.shape).astype(F)
    dx0 = rng.normal(size=x.shape).astype(F)
    assert (dx0 != 0).all()
    dx, dyd = T(dx0, cuda), T(dy, cuda)
    lib.check(L.m3d_subsample221_bwd(dyd.data_ptr(), B, H, W, D, C, dx.data_ptr(), lib.stream()),
              "subsample221_bwd")
    got = dx.cpu().numpy()
    assert_bits(got, ewref.subsample221_bwd(dy, dx0))
    keep = np.ones(x.shape, bool)
    keep[:, ::2, ::2] = False
    assert_bits(got[keep], dx0[keep])                        # positions not sampled stay as they were
    assert (got[~keep] != dx0[~keep]).all()


# --------------------------------------------------------------------------- frozen-BN affine
@pytest.mark.parametrize("C,eps", [(1, 1e-3), (3, 0.0), (257, 1e-3)])
def test_bn_affine(cuda, C, eps):
    import m3d._lib as lib
    L = lib.load()
    rng = np.random.default_rng([29, C])
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F)
    beta, mean = rng.normal(size=C).astype(F), rng.normal(size=C).astype(F)
    var = rng.uniform(0.1, 4.0, C).astype(F)
    out = torch.full((3, C), float("nan"), dtype=torch.float32, device=cuda)
    dev = [T(a, cuda) for a in (gamma, beta, mean, var)]
    lib.check(L.m3d_bn_affine(*(t.data_ptr() for t in dev), float(eps), C, out[0].data_ptr(), out[1].data_ptr(),
                              out[2].data_ptr(), lib.stream()), "bn_affine")
    scale, shift, rstd = out.cpu().numpy().astype(np.float64)
    r64, s64, t64 = ewref.bn_affine(gamma, beta, mean, var, eps)
    u = ewref.U
    # IEEE float32 operations, each within u = 2^-24 relative of its exact result:
    # rstd  = 1 / sqrt(var + eps): add (u), sqrt (halves the error it is given: u/2, plus its own
    #         u), divide (u) -> 2.5 u to first order; asserted at 3 u
    # scale = gamma * rstd: one multiply more -> 3.5 u; asserted at 4 u
    # shift = beta - mean * scale: the product carries 3.5 u + u, the subtraction adds u of the
    #         result, which is at most |beta| + |mean * scale| -> 5.5 u of that; asserted at 6 u
    tsc = np.abs(beta.astype(np.float64)) + np.abs(mean * s64)
    print(f"m3d_bn_affine (C={C}): max err/bound rstd {(np.abs(rstd - r64) / (3 * u * np.abs(r64))).max():.3f}, "
          f"scale {(np.abs(scale - s64) / (4 * u * np.abs(s64))).max():.3f}, "
          f"shift {(np.abs(shift - t64) / (6 * u * tsc)).max():.3f}")
    assert (np.abs(rstd - r64) <= 3 * u * np.abs(r64)).all()
    assert (np.abs(scale - s64) <= 4 * u * np.abs(s64)).all()
    assert (np.abs(shift - t64) <= 6 * u * tsc).all()


# --------------------------------------------------------------------------- BN-ReLU backward
# (M, C) -> (dz written, dres: None (NULL) / "set" / "acc")
BN_OUT = {(5, 4): (True, "acc"), (300, 12): (True, "set"), (700, 1028): (False, "acc"), (1100, 2048): (True, None),
          (40000, 64): (True, "set"), (262444, 4): (True, None)}


def _gx(M, C):
    import m3d._lib as lib
    nbytes = int(lib.load().m3d_bn_act_bwd_workspace_bytes(M, C))
    assert nbytes % (12 * C) == 0
    return nbytes // (12 * C)


def _bn_run(dev, d, M, C, relu, want_dz, dres_mode, which):
    """m3d_bn_act_bwd through the C entry.  dz starts NaN-filled, dres with
    dres0, the requested sum destinations with dst0, the workspace NaN-filled.
    Returns (dz | None, dres | None, [sum | None] * 3) as numpy."""
    import m3d._lib as lib
    L = lib.load()
    opt = lambda a: None if a is None else T(a, dev)         # noqa: E731
    dy, y, z = T(d["dy"], dev), T(d["y"], dev), T(d["z"], dev)
    scale, mean, rstd = opt(d["scale"]), opt(d["mean"]), opt(d["rstd"])
    dz = torch.full((M, C), float("nan"), dtype=torch.float32, device=dev) if want_dz else None
    dres = T(d["dres0"], dev) if dres_mode else None
    sums = [T(d["dst0"][i], dev) if which[i] else None for i in range(3)]
    wsb = int(L.m3d_bn_act_bwd_workspace_bytes(M, C)) if any(which) else 0
    ws = torch.full((wsb // 4,), float("nan"), dtype=torch.float32, device=dev) if wsb else None
    lib.check(L.m3d_bn_act_bwd(dy.data_ptr(), y.data_ptr() if relu else None, z.data_ptr(), M, C, relu, lib.ptr(scale),
                               lib.ptr(mean), lib.ptr(rstd), lib.ptr(dz), lib.ptr(dres), 1 if dres_mode == "acc" else 0,
                               lib.ptr(sums[0]), lib.ptr(sums[1]), lib.ptr(sums[2]), lib.ptr(ws), wsb, lib.stream()),
              "bn_act_bwd")
    torch.cuda.synchronize()
    np_ = lambda t: None if t is None else t.cpu().numpy()    # noqa: E731
    return np_(dz), np_(dres), [np_(s) for s in sums]


@functools.lru_cache(maxsize=None)
def _bn_ref(M, C, relu, affine, acc):
    d = ewref.bn_case(M, C, relu, affine)
    g, dz, dres, sums, abs_sums = ewref.bn_act_bwd(d["dy"], d["y"], d["z"], relu, d["scale"], d["mean"], d["rstd"],
                                                    d["dres0"] if acc else None)
    return d, _ro(dz), _ro(dres), _ro(sums), _ro(abs_sums)


def _check_sums(M, C, d, sums, abs_sums, got, which):
    """The derived bound (ewref.bn_sum_depth) per channel, never looser than
    1e-5 of the summed magnitudes (test_gpu_bnfuse's figure); the destination's
    prior value counts as one of the terms.  Returns the largest err / bound."""
    gx = _gx(M, C)
    bound = ewref.bn_sum_bound(M, C, gx, abs_sums, d["dst0"])
    cap = 1e-5 * (abs_sums + np.abs(d["dst0"].astype(np.float64)))
    assert (bound <= cap).all()
    worst = 0.0
    for i in range(3):
        if not which[i]:
            assert got[i] is None
            continue
        err = np.abs(got[i].astype(np.float64) - (sums[i] + d["dst0"][i].astype(np.float64)))
        assert (err <= bound[i]).all(), (M, C, i, float((err / np.maximum(bound[i], 1e-300)).max()))
        pos = bound[i] > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bound[i][pos]).max()))
    return worst


@pytest.mark.parametrize("M,C,relu,affine", ewref.BN_CASES, ids=[f"{c[0]}-{c[1]}" for c in ewref.BN_CASES])
def test_bn_act_bwd(cuda, M, C, relu, affine):
    want_dz, dres_mode = BN_OUT[(M, C)]
    d, dz_ref, dres_ref, sums, abs_sums = _bn_ref(M, C, relu, affine, dres_mode == "acc")
    dz, dres, got = _bn_run(cuda, d, M, C, relu, want_dz, dres_mode, (1, 1, 1))
    if want_dz:
        assert_bits(dz, dz_ref, "dz")
    if dres_mode:
        assert_bits(dres, dres_ref, "dres")
    if relu:                                                 # y = 0.0, -0.0, NaN: zero gradient
        for i in range(3):
            assert d["dy"][i, i] != 0
            assert dz is None or dz[i, i] == 0
            assert dres is None or dres[i, i] == (d["dres0"][i, i] if dres_mode == "acc" else 0)
    ratio = _check_sums(M, C, d, sums, abs_sums, got, (1, 1, 1))
    print(f"m3d_bn_act_bwd (M={M}, C={C}): depth {ewref.bn_sum_depth(M, C, _gx(M, C))}, max err/bound {ratio:.4f}")


@pytest.mark.parametrize("M,C,relu,affine", [c for c in ewref.BN_CASES if (c[0], c[1]) in ((300, 12), (700, 1028))],
                         ids=["300-12", "700-1028"])
def test_bn_act_bwd_split_calls(cuda, M, C, relu, affine):
    """Each sum alone, the sums without the elementwise outputs and the
    elementwise outputs without the sums: the fused call's bits."""
    d, dz_ref, dres_ref, sums, abs_sums = _bn_ref(M, C, relu, affine, True)
    dz, dres, fused = _bn_run(cuda, d, M, C, relu, True, "acc", (1, 1, 1))
    assert_bits(dz, dz_ref)
    assert_bits(dres, dres_ref)
    _check_sums(M, C, d, sums, abs_sums, fused, (1, 1, 1))
    dz1, dres1, none = _bn_run(cuda, d, M, C, relu, True, "acc", (0, 0, 0))
    assert none == [None, None, None]
    assert_bits(dz1, dz)
    assert_bits(dres1, dres)
    dz2, dres2, only = _bn_run(cuda, d, M, C, relu, False, None, (1, 1, 1))
    assert dz2 is None and dres2 is None
    for i in range(3):
        assert_bits(only[i], fused[i], f"sums only, sum {i}")
        which = tuple(int(j == i) for j in range(3))
        _, _, alone = _bn_run(cuda, d, M, C, relu, False, None, which)
        _check_sums(M, C, d, sums, abs_sums, alone, which)
        assert_bits(alone[i], fused[i], f"sum {i} alone")


# --------------------------------------------------------------------------- optimizers
OPT_SIZES = [(3000, True), (20000, True), (5, False), (1024, False), (40000, True)]      # (elements, L2 term)
OPT_WD = 0.01
OPT_CASES = [
    ("SGD", {"learning_rate": 0.05, "momentum": 0.9, "clipnorm": 5.0, "decay": 0.01}),
    ("ADAM", {"learning_rate": 0.01, "beta1": 0.85, "beta2": 0.99, "clipnorm": 2.0, "decay": 0.05}),
    ("ADAM", {"lr": 0.003, "amsgrad": True, "clipnorm": 2.0}),
    ("ADADELTA", {"learning_rate": 1.0, "rho": 0.9, "clipnorm": 1.0, "decay": 0.02}),
]
OPT_IDS = ["sgd-momentum", "adam", "adam-amsgrad", "adadelta"]
OPT_SCALES = (3.0, 0.003, 3.0, 0.003)      # large: the big tensors clip; small: norms below clipnorm


@pytest.fixture
def det_mode():
    """sets m3d's deterministic mode for a test; always back to off afterwards"""
    import m3d._lib as lib
    try:
        yield lib.set_deterministic
    finally:
        lib.set_deterministic(False)


def _opt_store(dev, sizes=OPT_SIZES):
    from m3d.params import ParamStore
    st = ParamStore()
    ps = [st.add(f"t{i}/kernel:0", (n,), "ones" if n < 1024 else ("normal", 0.1), l2)
          for i, (n, l2) in enumerate(sizes)]
    st.finalize(dev, seed=3, weight_decay=OPT_WD)
    return st, ps


@functools.lru_cache(maxsize=None)
def _opt_grads():
    rng = np.random.default_rng(41)
    return tuple(tuple(_ro((rng.normal(size=n) * s).astype(F)) for n, _ in OPT_SIZES) for s in OPT_SCALES)


def _pad_mask(st, ps):
    pad = np.ones(st.total, bool)
    for p in ps:
        pad[p.offset:p.offset + p.numel] = False
    return pad


def _opt_run(dev, name, params):
    """Four steps on the GPU.  Returns per step the parameters before it, after
    it and st.norms, then the final flat buffer and every slot buffer."""
    from m3d.optim import KerasOptimizer
    st, ps = _opt_store(dev)
    seg = st.seg_of_chunk.cpu().numpy()
    assert st.n_chunks == 65 and np.array_equal(np.bincount(seg), [3, 20, 1, 1, 40])
    assert seg[3] == 1 and seg[22] == 1 and seg[23] == 2 and seg[24] == 3 and seg[25] == 4      # blocks of 16 chunks
    opt = KerasOptimizer({"name": name, "parameters": params})
    steps = []
    for it, grads in enumerate(_opt_grads()):
        before = [p.data.detach().cpu().numpy().copy() for p in ps]
        st.grad_flat.zero_()
        for p, g in zip(ps, grads):
            p.grad.copy_(torch.from_numpy(np.array(g)))
        opt.step(st)
        torch.cuda.synchronize()
        steps.append((before, [p.data.detach().cpu().numpy().copy() for p in ps], st.norms.cpu().numpy().copy()))
    slots = [s.cpu().numpy() for s in opt.state(st)]
    return st, ps, opt, steps, st.flat.detach().cpu().numpy(), slots


@functools.lru_cache(maxsize=None)
def _opt_ref(idx):
    """oracle/optim_ref.py over the same four steps: the parameters after each
    step and the float64 norm of every tensor's clipped quantity."""
    from m3d.optim import KerasOptimizer, keras_opt_params
    name, params = OPT_CASES[idx]
    opt = KerasOptimizer({"name": name, "parameters": params})
    hp = keras_opt_params(params)
    clip, decay, lr = hp.pop("clipnorm", 0.0), hp.pop("decay", 0.0), hp.pop("lr", opt.lr)
    st, ps = _opt_store(torch.device("cpu"))
    ref = [p.data.detach().numpy().copy() for p in ps]
    states = [{} for _ in ps]
    out = []
    for it, grads in enumerate(_opt_grads()):
        norms = []
        for i, (n, l2) in enumerate(OPT_SIZES):
            l2c = OPT_WD / n if l2 else 0.0
            norms.append(np.sqrt(ewref.seg_sq_norm(grads[i], ref[i], l2c)))
            ref[i] = O.step(opt.kind, ref[i], np.array(grads[i]), states[i], it, lr, decay=decay, clipnorm=clip,
                            l2coef=l2c, **hp)
        # large steps: every tensor of a whole chunk or more is clipped; small steps: some are not
        if OPT_SCALES[it] > 1:
            assert all(nv > clip for nv, (n, _) in zip(norms, OPT_SIZES) if n >= 1024), (it, norms)
        else:
            assert any(nv < clip for nv in norms), (it, norms)
        out.append([_ro(r.copy()) for r in ref])
    return clip, out


@pytest.mark.parametrize("mode", ["atomic", "deterministic"])
@pytest.mark.parametrize("idx", range(len(OPT_CASES)), ids=OPT_IDS)
def test_optimizer_steps(cuda, det_mode, idx, mode):
    name, params = OPT_CASES[idx]
    det = mode == "deterministic"
    if det:
        det_mode(True)
    clip, ref = _opt_ref(idx)
    st, ps, opt, steps, flat, slots = _opt_run(cuda, name, params)
    worst = 0.0
    for it, (before, after, norms) in enumerate(steps):
        for i, p in enumerate(ps):
            want = ref[it][i]
            err = np.abs(after[i].astype(np.float64) - want).max()
            assert err <= 1e-6 * (np.abs(want).max() + 1e-12), (name, mode, it, p.name, err)
            # the clip norm of this step, from the parameters the kernel read
            l2c = F(OPT_WD / p.numel) if p.l2 else F(0)
            g = _opt_grads()[it][i]
            n64 = ewref.seg_sq_norm(g, before[i], l2c)
            bound = ewref.norm_bound(g, before[i], l2c, st.n_chunks, det)
            assert bound <= 1e-5 * n64
            nerr = abs(float(norms[i]) - n64)
            assert nerr <= bound, (name, mode, it, p.name, nerr / bound)
            worst = max(worst, nerr / bound)
    print(f"clip norms ({OPT_IDS[idx]}, {mode}): max err/bound {worst:.4f}")
    pad = _pad_mask(st, ps)
    assert pad.sum() == st.total - sum(n for n, _ in OPT_SIZES)
    assert not flat[pad].any()
    assert len(slots) == {"SGD": 1, "ADADELTA": 2}.get(opt.kind, 3 if params.get("amsgrad") else 2)
    for s in slots:
        assert not s[pad].any() and s[~pad].any()
    if det:                                                  # bit-identical on a second run
        _, _, _, steps2, flat2, slots2 = _opt_run(cuda, name, params)
        assert_bits(flat2, flat)
        for a, b in zip(slots, slots2):
            assert_bits(b, a)
        for s1, s2 in zip(steps, steps2):
            assert_bits(s2[2], s1[2], "norms")


@pytest.mark.parametrize("idx", range(len(OPT_CASES)), ids=OPT_IDS)
def test_optimizer_without_clipnorm(cuda, idx):
    """clipnorm = 0: no norm pass; norms (NaN here) is neither written nor read."""
    from m3d.optim import KerasOptimizer, keras_opt_params
    name, params = OPT_CASES[idx]
    params = {k: v for k, v in params.items() if k != "clipnorm"}
    st, ps = _opt_store(cuda)
    st.norms.fill_(float("nan"))
    opt = KerasOptimizer({"name": name, "parameters": params})
    assert opt.clipnorm == 0.0
    hp = keras_opt_params(params)
    decay, lr = hp.pop("decay", 0.0), hp.pop("lr", opt.lr)
    ref = [p.data.detach().cpu().numpy().copy() for p in ps]
    states = [{} for _ in ps]
    for it in range(2):
        grads = _opt_grads()[it]
        st.grad_flat.zero_()
        for p, g in zip(ps, grads):
            p.grad.copy_(torch.from_numpy(np.array(g)))
        opt.step(st)
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            l2c = OPT_WD / p.numel if p.l2 else 0.0
            ref[i] = O.step(opt.kind, ref[i], np.array(grads[i]), states[i], it, lr, decay=decay, clipnorm=0.0,
                            l2coef=l2c, **hp)
            err = np.abs(p.data.detach().cpu().numpy().astype(np.float64) - ref[i]).max()
            assert err <= 1e-6 * (np.abs(ref[i]).max() + 1e-12), (name, it, p.name, err)
    assert bool(torch.isnan(st.norms).all())
    assert not st.flat.detach().cpu().numpy()[_pad_mask(st, ps)].any()


def test_sgd_entry_without_clipnorm_takes_null_norms(cuda):
    """m3d_sgd_keras called directly with clipnorm = 0 and norms = NULL."""
    import m3d._lib as lib
    L = lib.load()
    st, ps = _opt_store(cuda)
    grads = _opt_grads()[0]
    for p, g in zip(ps, grads):
        p.grad.copy_(torch.from_numpy(np.array(g)))
    ref = [p.data.detach().cpu().numpy().copy() for p in ps]
    lib.check(L.m3d_sgd_keras(st.flat.data_ptr(), st.grad_flat.data_ptr(), st.moments.data_ptr(), st.n_chunks,
                              st.seg_of_chunk.data_ptr(), st.l2_coef.data_ptr(), len(ps), 0.05, 0.9, 0.0, None,
                              lib.stream()), "sgd")
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        want = O.step("SGD", ref[i], np.array(grads[i]), {}, 0, 0.05, momentum=0.9,
                      l2coef=OPT_WD / p.numel if p.l2 else 0.0)
        err = np.abs(p.data.detach().cpu().numpy().astype(np.float64) - want).max()
        assert err <= 1e-6 * (np.abs(want).max() + 1e-12), (p.name, err)


def test_deterministic_scratch_too_small(cuda, det_mode):
    """1100 chunks need 1100 floats of deterministic scratch; with 4096 bytes the
    call is refused before any kernel runs."""
    from m3d.optim import KerasOptimizer
    st, ps = _opt_store(cuda, [(1100 * 1024, True)])
    assert st.n_chunks == 1100
    ps[0].grad.fill_(0.5)
    before = st.flat.detach().clone()
    moments = st.moments.clone()
    opt = KerasOptimizer({"name": "SGD", "parameters": {"learning_rate": 0.05, "momentum": 0.9, "clipnorm": 5.0}})
    det_mode(True, scratch_bytes=4096)
    with pytest.raises(ValueError, match="scratch smaller than n_chunks"):
        opt.step(st)
    torch.cuda.synchronize()
    assert torch.equal(st.flat.detach(), before) and torch.equal(st.moments, moments)
    assert opt.iterations == 0
    det_mode(True, scratch_bytes=4400)                        # exactly enough: the step runs
    opt.step(st)
    torch.cuda.synchronize()
    assert not torch.equal(st.flat.detach(), before)
