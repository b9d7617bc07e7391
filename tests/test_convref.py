"""tests/convref.py against torch-CPU float64 (F.conv3d with stride and
dilation, F.conv_transpose3d, autograd for both gradients) at the cases of
tests/test_gpu_conv_paths.py, and the coverage claim of that file: the union of
gemm_path / wgrad_path over the case tables equals the list of reachable
instantiations written out below.  No GPU.

Both sides are float64 here, so agreement is to 1e-12 of the result's scale.

Forms of conv_gemm_kernel<BM, BN, .., BT, AVEC, BK, NBUF, PERSIST, X3, FBN>
that no launch site names, so the library does not hold them
(test_library_holds_only_launchable_conv_kernels reads its kernel list):
* every BK = 64 form: dispatch_gemm passes BK = 32 only;
* X3 = false with AVEC and (BT or BN >= 64), with or without FBN: launch_gemm
  takes the bf16-split form wherever there is one;
* NBUF = 2 with AVEC: the vector loader always runs one LDS stage;
* scalar A with BT: every BT caller (data gradient, deconv, split-K) is vector.
In the library but never launched, and so run by no test:
* PERSIST at 64x128 (launch_gemm instantiates it with the other tiles): that
  tile is chosen below 512 blocks of 128 rows, which are at most 1022 tiles of
  64 rows, fewer than 6 * 256 CUs.
Reachable but left to other files: the fused-BN forms
(tests/test_gpu_bnfuse.py), the HALO forms of conv_wgrad_kernel
(tests/test_gpu_slab_halo.py) and the stem kernels (tests/test_gpu_conv.py,
test_gpu_slab_halo.py).  Every other reachable instantiation has a case.  The
large-M cases are small enough for torch float64 as they are; only the
persistent split-K cases are checked on a slice of their rows.
"""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import convref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def agree(got, ref, tol=TOL):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    scale = float(np.abs(ref).max()) + 1e-300
    assert float(np.abs(got - ref).max()) <= tol * scale


def t64(a):
    return torch.from_numpy(np.array(a, np.float64))


def torch_conv(x, w, stride, pad, dil, out):
    """F.conv3d on [B,H,W,D,C] / Keras kernels with pad-before `pad` and as much
    zero padding behind as `out` outputs need"""
    k = w.shape[:3]
    after = [max(0, (o - 1) * s + (kk - 1) * d + 1 - n - p)
             for o, s, kk, d, n, p in zip(out, stride, k, dil, x.shape[1:4], pad)]
    xp = TF.pad(x.permute(0, 4, 1, 2, 3), (pad[2], after[2], pad[1], after[1], pad[0], after[0]))
    y = TF.conv3d(xp, w.permute(4, 3, 0, 1, 2), stride=stride, dilation=dil)
    return y[:, :, :out[0], :out[1], :out[2]].permute(0, 2, 3, 4, 1)


def torch_epilogue(v, d, c):
    z = v = v + t64(d["bias"]) if d["bias"] is not None else v
    if d["scale"] is not None:
        v = v * t64(d["scale"]) + t64(d["shift"])
    if c["res_mode"] == 1:
        v = v + t64(d["res"])
    elif c["res_mode"] == 2:
        r = t64(d["res"]).permute(0, 4, 1, 2, 3)
        v = v + TF.interpolate(r, scale_factor=(2, 2, 1), mode="nearest").permute(0, 2, 3, 4, 1)
    v = torch.relu(v) if c["act"] == 1 else torch.sigmoid(v) if c["act"] == 2 else v
    if c["res_mode"] == 3:
        v = v + t64(d["res"])
    return z, v


@pytest.mark.parametrize("c", R.FWD_CASES + [R.splitk_fwd_case(c) for c in R.SPLITK_FWD_CASES],
                         ids=lambda c: c["id"])
def test_conv_fwd_and_epilogue(c):
    d = R.fwd_data(c)
    v = torch_conv(t64(d["x"]), t64(d["w"]), c["stride"], d["pad"], c["dil"], d["out"])
    z, y = torch_epilogue(v, d, c)
    agree(d["z"], z.numpy())
    full = np.concatenate([d["y"], d["y2"]], -1) if c["split"] else d["y"]
    agree(full, y.numpy())
    if c["split"]:
        assert d["y"].shape[-1] == c["split"][0] and d["y2"].shape[-1] == c["split"][1] - c["split"][0]
    ap = torch_conv(t64(d["x"]).abs(), t64(d["w"]).abs(), c["stride"], d["pad"], c["dil"], d["out"])
    agree(R.absprod_fwd(d["x"], d["w"], c["k"], c["stride"], d["pad"], c["dil"], d["out"]), ap.numpy())
    if c["act"] == 1:                    # the ReLU cap: the reference alone, perturbed by +- its bound
        assert R.relu_ambiguous(d["pre"], d["preerr"]) <= R.RELU_CAP * d["pre"].size
        assert 0.3 < float((d["pre"] > 0).mean()) < 0.7          # and both branches are taken


def test_epilogue_accumulate_and_bounds():
    rng = np.random.default_rng(5)
    acc, y0 = rng.normal(size=(3, 8)), rng.normal(size=(3, 8))
    err = np.full((3, 8), 1e-6)
    r = R.epilogue(acc, err, bias=np.ones(8), act=1, y0=y0)
    agree(r["y"], np.maximum(acc + 1, 0) + y0)
    assert (r["yerr"] > r["preerr"]).all() and (r["preerr"] >= r["zerr"]).all() and (r["zerr"] > err).all()
    s = R.epilogue(acc, err, scale=np.full(8, -3.0), shift=np.zeros(8))
    assert (s["yerr"] >= 3 * err).all()                      # the affine's Lipschitz factor
    assert R.epilogue(acc, err, act=2)["yerr"] is None       # the sigmoid is not bounded (module docstring)


def _grads(x, w, dz, stride, pad, out):
    xt, wt = t64(x).requires_grad_(True), t64(w).requires_grad_(True)
    torch_conv(xt, wt, stride, pad, (1, 1, 1), out).backward(t64(dz))
    return xt.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize("c", R.BWD_DATA_CASES, ids=lambda c: c[0])
def test_conv_bwd_data(c):
    cid, cin, cout, k, stride, padding, sp = c
    d = R.bwd_data_data(c)
    x = np.zeros((R.BWD_B, *sp, cin))
    dx, _ = _grads(x, d["w"], d["dz"], stride, d["pad"], d["out"])
    agree(d["dx"], dx)
    adx, _ = _grads(x, np.abs(d["w"]), np.abs(d["dz"]), stride, d["pad"], d["out"])
    agree(d["err"], R.sum_bound(math.prod(k) * cout, adx))
    # the voxels a strided 1x1x1 conv never reads
    want = np.zeros(sp, bool)
    want[::stride[0], ::stride[1], ::stride[2]] = True
    if k == R.K1:
        assert (d["covered"] == want).all() and (d["dx"][~d["covered"]] == 0).all()
        assert any(s > 1 for s in stride) and not d["covered"].all()
    else:
        assert d["covered"].all()


@pytest.mark.parametrize("c", R.SPLITK_BWD_CASES, ids=lambda c: c[0])
def test_splitk_bwd_data(c):
    cid, splits, cin, cout, stride, acc = c
    d = R.splitk_bwd_data(c)
    dx, _ = _grads(np.zeros((1, *d["sp"], cin)), d["w"], d["dz"], stride, (0, 0, 0), R.SPLITK_OUT)
    agree(d["dx"], dx)
    assert (d["dx"][~d["covered"]] == 0).all() and cout % (32 * splits) == 0


@pytest.mark.parametrize("c", R.SPLITK_PERSIST_CASES, ids=lambda c: c[0])
def test_splitk_persist_case(c):
    for ncu in (R.MIN_NCU, 64, R.NCU, 304):
        (_, splits, cin, cout, _, _), out = R.splitk_persist_geom(c, ncu)
        bn = 32 if cin <= 32 else 64 if cin <= 64 else 128
        M = math.prod(out)
        tiles = R.cdiv(M, 128) * R.cdiv(cin, bn) * splits
        # about 5 % past 6 * CUs at real CU counts (the 128x128 tile: or its 512 blocks)
        assert tiles > 6 * ncu and (ncu < 64 or tiles <= max(6 * ncu * 1.06, 512 * (bn == 128)) + splits)
        assert R.splitk_paths((0, splits, cin, cout), False, ncu, out)[0] == _gemm(128, bn, "bt", "avec", "x3",
                                                                                   "persist")
        assert ncu > R.NCU or max(M * cout, splits * M * cin, cin * cout) * 4 <= 35e6
        assert cout % (32 * splits) == 0 and splits <= 64 and cin % 4 == 0
    c, out = R.splitk_persist_geom(c, R.MIN_NCU)           # the same case at its smallest size,
    out = out if c[1] == 64 and c[2] > 64 else ((12, 16, 8) if c[1] == 8 else (17, 4, 2))   # or on a slice of rows
    d = R.splitk_bwd_data(c, out)
    dx, _ = _grads(np.zeros((1, *out, c[2])), d["w"], d["dz"], c[4], (0, 0, 0), out)
    agree(d["dx"], dx)


@pytest.mark.parametrize("c", R.WGRAD_CASES, ids=lambda c: c[0])
def test_conv_bwd_weight(c):
    cid, cin, cout, k, stride, padding, sp = c
    d = R.wgrad_data(c)
    _, dw = _grads(d["x"], np.zeros_like(d["dw0"]), d["dz"], stride, d["pad"], d["out"])
    agree(d["dw"], dw + d["dw0"])
    _, adw = _grads(np.abs(d["x"]), np.zeros_like(d["dw0"]), np.abs(d["dz"]), stride, d["pad"], d["out"])
    agree(d["absprod"], adw)
    assert float(np.abs(d["dw0"]).min()) > 0                 # a skipped += shows


@pytest.mark.parametrize("c", R.DECONV_CASES, ids=lambda c: c[0])
def test_deconv_k2s2(c):
    cid, B, sp, cin, cout, act = c
    d = R.deconv_data(c)
    xt = t64(d["x"]).permute(0, 4, 1, 2, 3)
    wt = t64(d["w"]).permute(4, 3, 0, 1, 2)                  # [Cin, Cout, 2, 2, 2]
    y = TF.conv_transpose3d(xt, wt, t64(d["bias"]), stride=2).permute(0, 2, 3, 4, 1)
    agree(d["pre"], y.numpy(), 1e-10)
    y = torch.relu(y) if act == 1 else torch.sigmoid(y) if act == 2 else y
    agree(d["y"], y.numpy(), 1e-10)
    ap = TF.conv_transpose3d(xt.abs(), wt.abs(), None, stride=2).permute(0, 2, 3, 4, 1)
    agree(R.absprod_deconv(d["x"], d["w"]), ap.numpy(), 1e-10)
    if act == 1:
        assert R.relu_ambiguous(d["pre"], d["preerr"]) <= R.RELU_CAP * d["pre"].size
        assert 0.3 < float((d["pre"] > 0).mean()) < 0.7


@pytest.mark.parametrize("c", R.GEMM_CASES, ids=lambda c: c[0])
def test_gemm(c):
    cid, batch, M, K, N, lda, shared, bias, act, acc = c
    d = R.gemm_data(c)
    A, Bm = t64(d["A"])[..., :K], t64(d["B"])
    v = torch.matmul(A, Bm).expand(d["batch"], M, N)
    if bias:
        v = v + t64(d["bias"])
    v = torch.relu(v) if act else v
    if acc:
        v = v + t64(d["c0"])
    agree(d["y"], v.numpy())
    if act == 1:
        assert R.relu_ambiguous(d["pre"], d["preerr"]) <= R.RELU_CAP * d["pre"].size
    if batch is None:                     # tiles pass 6 * CUs, by about 5 % at real CU counts
        per = R.cdiv(M, 128) * R.cdiv(N, 32 if N <= 32 else 64 if N <= 64 else 128)
        for ncu in (R.MIN_NCU, 64, R.NCU, 304):
            tiles = R.persist_batch(ncu, M, N) * per
            assert tiles > 6 * ncu and (ncu < 64 or tiles <= max(6 * ncu * 1.06, 512 * (N > 64)) + per)
            assert N <= 64 or tiles >= 512
        assert R.persist_batch(R.NCU, M, N) * M * lda * 4 <= 35e6           # A; the product is N / lda times that


# --------------------------------------------------------------------------- the path tables
def _gemm(bm, bn, t, a, f, g):
    return ("gemm", bm, bn, t, a, f, g, "")


TILES = [(128, 32), (128, 64), (64, 128), (128, 128)]
# every instantiation the default build can launch through the entries of
# tests/test_gpu_conv_paths.py
REACHABLE = (
    [_gemm(bm, bn, "nt", "avec", "x3" if bn >= 64 else "f32", "grid") for bm, bn in TILES] +
    [_gemm(bm, bn, "nt", "avec", "x3" if bn >= 64 else "f32", "persist") for bm, bn in TILES if bm == 128] +
    [_gemm(bm, bn, "nt", "scalar", "f32", "grid") for bm, bn in TILES] +
    [_gemm(bm, bn, "bt", "avec", "x3", "grid") for bm, bn in TILES] +
    [_gemm(bm, bn, "bt", "avec", "x3", "persist") for bm, bn in TILES if bm == 128] +
    [("wgrad", 64, 64, "vec"), ("wgrad", 64, 128, "vec"), ("wgrad", 128, 64, "vec"), ("wgrad", 128, 64, "scalar"),
     ("wgrad", 128, 128, "vec"), ("wgrad", 128, 128, "scalar"),
     ("x3_wgrad64",), ("x3_wgrad",), ("x3_wgrad_tr", "grid"), ("x3_wgrad_tr", "sk"),
     ("wg_reduce",), ("splitk_epi",)] +
    [("wg_target", fam, tgt) for fam in ("wgrad", "x3_wgrad64", "x3_wgrad", "x3_wgrad_tr")
     for tgt in ("atomic", "reduce", "plain")])


def test_tuning_constants_match_the_header():
    src = open(os.path.join(ROOT, "3d-mask-r-cnn_amd", "csrc", "common.h")).read()
    for name, v in R.TUNE.items():
        m = re.search(r"#ifndef %s\n#define %s (\d+)" % (name, name), src)
        assert m and int(m.group(1)) == v, name
    # the dispatch reads no other constant: the retired form switches are not defined any more
    for name in ("GEMM_X3", "X3W_TR", "X3W_SK", "WINO_NZ", "WINO_WGRAD_NZ", "WINO_NY"):
        assert not re.search(r"M3D_TUNE_%s\b" % name, src), name
    hip =open(os.path.join(ROOT, "3d-mask-r-cnn_amd", "csrc", "conv3d.hip")).read()
    assert "constexpr int W2_BK = %d;" % R.W2_BK in hip
    assert R.TUNE["M3D_TUNE_WGRAD1_X3_MIN_N"] == 65 and R.DET_SMALL_BYTES == 4096


# conv_gemm_kernel / conv_wgrad_kernel forms that other files run
FBN_FORMS = [("gemm", bm, bn, "bt", "avec", "x3", "grid", "fbn") for bm, bn in TILES]   # tests/test_gpu_bnfuse.py
HALO_FORMS = [("wgrad", 128, 64, "vec", "halo"), ("wgrad", 128, 64, "scalar", "halo"),  # tests/test_gpu_slab_halo.py
              ("wgrad", 128, 128, "vec", "halo"), ("wgrad", 128, 128, "scalar", "halo")]
# launch_gemm instantiates the persistent loop for every vector tile; dispatch_gemm never picks it at
# 64x128 (module docstring)
NEVER_CHOSEN_PERSIST_64X128 = [_gemm(64, 128, "nt", "avec", "x3", "persist"),
                               _gemm(64, 128, "bt", "avec", "x3", "persist")]
# the Winograd transforms and the bf16-split GEMMs, each with what launches it
WINO_X3_KERNELS = {
    # F(4,3) along z everywhere; the last argument of the transforms is the y tile
    "wino_input_kernel<4, false, false, 4>": "m3d_conv3d_fwd_wino*, m3d_conv3d_bwd_weight_wino, bwd_data_wino* tile_y 4",
    "wino_input_kernel<4, false, false, 2>": "m3d_conv3d_bwd_data_wino* (tile_y 2, the default)",
    "wino_input_kernel<4, false, true, 4>": "m3d_conv3d_fwd_wino_halo / _halo_phase, m3d_conv3d_bwd_weight_wino_halo",
    "wino_weight_kernel<4, true, 4>": "m3d_conv3d_fwd_wino*, m3d_conv3d_wino_weight_v, bwd_data_wino* tile_y 4",
    "wino_weight_kernel<4, true, 2>": "m3d_conv3d_bwd_data_wino*, m3d_conv3d_wino_weight_v (dgrad, tile_y 2)",
    "wino_output_kernel<4, 4>": "m3d_conv3d_fwd_wino*, bwd_data_wino_vy / _xv / _rs tile_y 4",
    "wino_output_kernel<4, 2>": "m3d_conv3d_bwd_data_wino* (tile_y 2)",
    "wino_output_bn_kernel<4, 4>": "m3d_conv3d_bwd_data_wino_bny / _xv tile_y 4",
    "wino_output_bn_kernel<4, 2>": "m3d_conv3d_bwd_data_wino_bn, _bny / _xv tile_y 2",
    "wino_output_halo_kernel<4, 2>": "m3d_conv3d_bwd_data_wino_halo",
    # the halo entry takes no tile_y: this one runs only in a build with M3D_TUNE_WINO_DGRAD_NY 0 or 4
    # (bwd_data_wino_launch<4> names the halo output beside the other two)
    "wino_output_halo_kernel<4, 4>": "m3d_conv3d_bwd_data_wino_halo where the library's data-gradient y tile is 4",
    "wino_grad_kernel<4>": "m3d_conv3d_bwd_weight_wino*",
    "wino_wgrad_out_kernel<4>": "m3d_conv3d_bwd_weight_wino*",
    "x3_gemm256_af_kernel<0>": "Winograd fwd / bwd-data point GEMMs (N % 256 == 0), m3d_gemm_x3_af, m3d_conv3d_fwd_x3",
    "x3_gemm256_af_kernel<1>": "m3d_conv3d_fwd_x3 with an epilogue",
    "x3_gemm256_af_kernel<2>": "m3d_conv3d_bwd_data_x3_bn / _bna",
    "x3_gemm256_kernel<0>": "m3d_gemm_x3 (N % 256 == 0)",
    "x3_gemm_kernel<32, false, 2, true, 128>": "Winograd fwd / bwd-data point GEMMs (other N), m3d_gemm_x3_af",
    "x3_gemm_kernel<32, false, 2, true, 64>": "Winograd fwd / bwd-data point GEMMs (N = 64), m3d_gemm_x3_af",
    "x3_gemm_kernel<32, false, 3, false, 128>": "m3d_gemm_x3",
    "x3_gemm_kernel<32, false, 3, false, 64>": "m3d_gemm_x3 (N = 64)",
    "x3_wgrad_tr_kernel<0, true>": "m3d_conv3d_bwd_weight_wino*, m3d_conv3d_bwd_weight (1x1x1), m3d_gemm_wgrad_f32: stream-K",
    "x3_wgrad_tr_kernel<0, false>": "the same, deterministic or below 32 steps: the split grid",
    "x3_wgrad_kernel<2>": "the same entries, K or N < 192",
    "x3_wgrad64_kernel<2>": "the same entries, K or N <= 64",
}


def _conv_kernels_of_the_library():
    """{kernel<template arguments>} of the conv kernels' host handles in libm3d.so (names only)"""
    import subprocess
    import m3d._lib as lib
    out = subprocess.run(["readelf", "-sW", "--demangle", lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    names = set()
    for line in out.splitlines():
        f = line.split()
        if len(f) < 8 or f[3] != "OBJECT" or f[6] == "UND":
            continue
        m = re.match(r"(?:void )?(?:m3d::)?((?:conv_gemm|conv_wgrad|wino_\w+|x3_gemm\w*|x3_wgrad\w*)_kernel<[^>]*>)\(",
                     " ".join(f[7:]))
        if m:
            names.add(m.group(1))
    return names


def _form(name):
    """a conv_gemm_kernel / conv_wgrad_kernel instantiation in the tuple form of REACHABLE"""
    kern, args = name[:-1].split("<")
    a = [{"true": True, "false": False}.get(v, v) for v in args.split(", ")]
    a = [v if isinstance(v, bool) else int(v) for v in a]
    if kern == "conv_wgrad_kernel":
        bi, bj, wi, wj, avec, halo = a
        assert (wi, wj) == (2, 2), name
        return ("wgrad", bi, bj, "vec" if avec else "scalar") + (("halo",) if halo else ())
    bm, bn, wm, wn, bt, avec, bk, nbuf, persist, x3, fbn = a
    assert (wm, wn) == ((4, 1) if bm == 128 and bn <= 64 else (2, 2)) and bk == 32 and nbuf == (1 if avec else 2), name
    return ("gemm", bm, bn, "bt" if bt else "nt", "avec" if avec else "scalar", "x3" if x3 else "f32",
            "persist" if persist else "grid", "fbn" if fbn else "")


def test_library_holds_only_launchable_conv_kernels():
    """The built library's conv kernels are the reachable instantiations and nothing else: a form that
    no entry point can launch (the losing side of a settled A/B) is not compiled in."""
    names = _conv_kernels_of_the_library()
    gemm = sorted(n for n in names if n.startswith(("conv_gemm_kernel<", "conv_wgrad_kernel<")))
    forms = [_form(n) for n in gemm]
    assert len(set(forms)) == len(forms) > 0
    want = [p for p in REACHABLE if p[0] in ("gemm", "wgrad")] + FBN_FORMS + HALO_FORMS + NEVER_CHOSEN_PERSIST_64X128
    assert len(set(want)) == len(want)
    assert set(forms) == set(want), (sorted(set(forms) - set(want)), sorted(set(want) - set(forms)))
    rest = names - set(gemm)
    assert rest == set(WINO_X3_KERNELS), (sorted(rest - set(WINO_X3_KERNELS)), sorted(set(WINO_X3_KERNELS) - rest))


@pytest.mark.parametrize("ncu", [R.NCU, R.MIN_NCU])
def test_every_reachable_instantiation_has_a_case(ncu):
    paths = R.all_paths(ncu)
    assert len(set(REACHABLE)) == len(REACHABLE)
    assert set(paths) == set(REACHABLE)
    assert R.all_paths(R.NCU).keys() == paths.keys()


def test_case_tables_reach_what_their_ids_say():
    p = {c["id"]: R.fwd_path(c) for c in R.FWD_CASES}
    assert p["t128x32-avec"] == _gemm(128, 32, "nt", "avec", "f32", "grid")
    assert p["t128x64-bn-relu-z"] == _gemm(128, 64, "nt", "avec", "x3", "grid")
    assert p["t64x128-res1-relu"] == p["t64x128-plain"] == _gemm(64, 128, "nt", "avec", "x3", "grid")
    assert p["t128x128-big"] == _gemm(128, 128, "nt", "avec", "x3", "grid")
    assert all(p[i][4] == "scalar" for i in p if i.startswith("scalar"))
    g = {c[0]: R.gemm_case_path(c) for c in R.GEMM_CASES}
    assert g["persist-n32"] == _gemm(128, 32, "nt", "avec", "f32", "persist")
    assert g["persist-n64"] == _gemm(128, 64, "nt", "avec", "x3", "persist")
    assert g["grid-n32-bias"] == _gemm(128, 32, "nt", "avec", "f32", "grid")
    assert g["grid-n64-bias"] == _gemm(128, 64, "nt", "avec", "x3", "grid")
    assert g["persist-n132"] == _gemm(128, 128, "nt", "avec", "x3", "persist")
    assert g["grid-n132-bias"] == _gemm(128, 128, "nt", "avec", "x3", "grid")
    w = {(c[0], m): R.wgrad_path_of(c, m) for c in R.WGRAD_CASES for m in R.WGRAD_MODES}
    assert w["w64x64-m16", "atomic"][2:] == (1, 32)                             # M < 32
    assert w["w64x128-m1064", "atomic"][1:] == ("atomic", 3, 384)               # 384 + 384 + 296
    assert w["w64x128-m1064", "det"][1:] == ("reduce", 3, 384)
    assert w["w64x128-m1064", "det-small"][1:] == ("plain", 1, 1088)            # fit < 2
    assert w["w64x128-m1064", "det-fit2"][1:] == ("reduce", 2, 544)             # splits lowered to what fits
    assert w["w128x64-vec-m1024", "atomic"][1:] == ("atomic", 2, 512)           # M = 2 * mper
    assert w["x3-below-n64", "atomic"][0] == ("wgrad", 64, 64, "vec")
    assert w["x3-64-n68", "atomic"][0] == ("x3_wgrad64",)
    assert w["x3-tr-m1064", "atomic"][0] == ("x3_wgrad_tr", "sk") and w["x3-tr-m1064", "det"][0][1] == "grid"
    for c in R.WGRAD_CASES:                       # the smallest scratch fits no case twice
        assert math.prod(c[3]) * c[1] * c[2] * 2 > R.DET_SMALL_BYTES // 4
