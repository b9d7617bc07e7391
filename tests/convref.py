"""Plain numpy float64 references of the implicit-GEMM half of csrc/conv3d.hip
(forward conv with its epilogue, data gradient, weight gradient, the 2x2x2
stride-2 transposed conv, plain GEMM) -- test infrastructure, no GPU.  Tensors
are channels-last [B, H, W, D, C]; kernels are Keras [kh, kw, kd, Cin, Cout].

The references are restatements of the definitions: one pass per kernel tap
over the output voxels that tap can reach, y[o] += x[o*s - p + k*d] @ w[k].
Nothing is gathered into an im2col matrix, nothing is tiled, so they share no
structure with conv_gemm_kernel / conv_wgrad_kernel.

Error bound (bound 2 of tests/test_gpu_conv_paths.py).  u = 2^-24.  A float32
sum in which no term passes through more than d rounded operations satisfies
|fl(sum) - sum| <= d * u * sum|term| to first order (tests/ewref.py has the
argument).  A sum of K products on the exact bf16 split is 6 bf16 MFMA
accumulations per product (6K roundings on the accumulator chain) and drops
three cross terms per product, each below u |a||b|; the plain f32 MFMA chain
needs only K.  So

    |got - ref| <= (6K + 16) * u * sum |a||b|                (sum_bound)

and the 16 leaves 13 roundings for a K split into slices that are added in
slice order (at most 7 more additions at 8 slices) and the second-order part.
Every operation of the epilogue on that value then adds one relative rounding
of its own result and carries the incoming bound through its Lipschitz factor
(|scale[n]| for the BN affine, 1 for the additions and the ReLU).  The sigmoid
is NOT bounded here: the rounding of the device's expf is not documented in
this repository, so sigmoid cases are compared under this bound at the
pre-activation (z_out) and under the 1e-4-of-scale criterion after it.

For a weight gradient the reduction length is the number of output rows M; each
m-split adds its partial tile to dW with one more rounding of the running
value (an fp32 atomic, or the ordered reduce and its final +=), bounded by
u (|dw0| + sum|a||b|) each: wgrad_bound.

gemm_path / wgrad_path restate the host dispatch of conv3d.hip, so the claim
"every reachable instantiation has a case" is computed (tests/test_convref.py)
and not only written down.
"""
import itertools
import math

import numpy as np

F = np.float32
U = 2.0 ** -24

# compile-time tuning defaults of csrc/common.h that the dispatch reads
# (tests/test_convref.py compares them with the header)
TUNE = {"M3D_TUNE_WGRAD_MINM": 512, "M3D_TUNE_X3W_TR_MINM": 256, "M3D_TUNE_X3W_SK_MIN_STEPS": 32,
        "M3D_TUNE_WGRAD1_X3_MIN_N": 65}
W2_BK = 16                      # conv3d.hip: rows per step of x3_wgrad_tr_kernel
NCU = 256                       # MI355X
# smallest CU count at which the persistent cases can be sized at all:
# launch_gemm's persistent grid is 3 * CUs rounded down to a multiple of 8
# workgroups, which below 3 CUs is a zero-sized launch (a latent host bug on a
# device no one has; out of scope here).  Every case takes the same path at 3
# CUs as at 256 (tests/test_convref.py).
MIN_NCU = 3


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------- geometry
def same_geom(n, k, s, d=1):
    """TF 'same': (output size, pad before)."""
    o = cdiv(n, s)
    return o, max((o - 1) * s + (k - 1) * d + 1 - n, 0) // 2


def valid_geom(n, k, s, d=1):
    return (n - (k - 1) * d - 1) // s + 1, 0


def geom(sp, k, stride, padding, dil=(1, 1, 1)):
    """(out, pad_before) of a conv on spatial size sp."""
    f = same_geom if padding == "same" else valid_geom
    g = [f(n, kk, s, d) for n, kk, s, d in zip(sp, k, stride, dil)]
    return tuple(o for o, _ in g), tuple(p for _, p in g)


def _taps(sp, out, k, stride, pad, dil):
    """(tap, output slices, input slices) of every tap that reaches the volume:
    the outputs o with 0 <= o*s - p + k*d < n, and the inputs they read."""
    for tap in itertools.product(*(range(kk) for kk in k)):
        osl, isl = [], []
        for n, o, kk, s, p, d in zip(sp, out, tap, stride, pad, dil):
            off = kk * d - p
            lo, hi = max(0, -(off // s)), min(o - 1, (n - 1 - off) // s)
            if hi < lo:
                break
            osl.append(slice(lo, hi + 1))
            isl.append(slice(lo * s + off, hi * s + off + 1, s))
        else:
            yield tap, (slice(None), *osl), (slice(None), *isl)


# --------------------------------------------------------------------------- the sums
def conv_fwd(x, w, k, stride, pad_before, dilation, out):
    """y [B, *out, Cout] = sum over taps and Cin; taps outside the volume read zero."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    assert tuple(w.shape[:3]) == tuple(k) and w.shape[3] == x.shape[4]
    y = np.zeros((x.shape[0], *out, w.shape[4]))
    for tap, o, i in _taps(x.shape[1:4], out, k, stride, pad_before, dilation):
        y[o] += x[i] @ w[tap]
    return y


def conv_bwd_data(dz, w, x_shape, k, stride, pad_before, out):
    """dx [x_shape] = the adjoint of conv_fwd in x (any stride: a strided 1x1x1
    conv scatters dz w^T to the voxels o*s and leaves the others zero)."""
    dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64)
    dx = np.zeros(x_shape)
    for tap, o, i in _taps(x_shape[1:4], out, k, stride, pad_before, (1, 1, 1)):
        dx[i] += dz[o] @ w[tap].T
    return dx


def conv_bwd_weight(x, dz, k, stride, pad_before, out, dw0):
    """dw0 + the adjoint of conv_fwd in w."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    dw = np.array(dw0, np.float64)
    for tap, o, i in _taps(x.shape[1:4], out, k, stride, pad_before, (1, 1, 1)):
        dw[tap] += np.tensordot(x[i], dz[o], axes=([0, 1, 2, 3], [0, 1, 2, 3]))
    return dw


def deconv_k2s2_sum(x, w):
    """KL.Conv3DTranspose(Cout, 2, strides=2) before bias and activation:
    y[b, 2i+a, 2j+b', 2k+c, o] = sum_cin x[b,i,j,k,cin] w[a,b',c,o,cin] (no overlap)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, D, _ = x.shape
    y = np.zeros((B, 2 * H, 2 * W, 2 * D, w.shape[3]))
    for a, b, c in itertools.product(range(2), repeat=3):
        y[:, a::2, b::2, c::2] = x @ w[a, b, c].T
    return y


def deconv_k2s2(x, w, bias, act):
    """(y, bound 2 of y or None for the sigmoid, pre-activation, its bound)"""
    r = epilogue(deconv_k2s2_sum(x, w), sum_bound(x.shape[4], absprod_deconv(x, w)), bias=bias, act=act)
    return r["y"], r["yerr"], r["pre"], r["preerr"]


def gemm(A, Bm):
    return np.asarray(A, np.float64) @ np.asarray(Bm, np.float64)


# the same sums over |a||b|
def absprod_fwd(x, w, k, stride, pad_before, dilation, out):
    return conv_fwd(np.abs(x), np.abs(w), k, stride, pad_before, dilation, out)


def absprod_bwd_data(dz, w, x_shape, k, stride, pad_before, out):
    return conv_bwd_data(np.abs(dz), np.abs(w), x_shape, k, stride, pad_before, out)


def absprod_bwd_weight(x, dz, k, stride, pad_before, out):
    return conv_bwd_weight(np.abs(x), np.abs(dz), k, stride, pad_before, out,
                           np.zeros((*k, x.shape[4], dz.shape[4])))


def absprod_deconv(x, w):
    return deconv_k2s2_sum(np.abs(x), np.abs(w))


def absprod_gemm(A, Bm):
    return gemm(np.abs(A), np.abs(Bm))


# --------------------------------------------------------------------------- bounds
def sum_bound(K, absprod):
    return (6 * K + 16) * U * absprod


def _round(v, err):
    """bound after one more float32 operation whose exact result is v"""
    return err + U * (np.abs(v) + err)


def wgrad_bound(M, absprod, dw0, splits):
    """splits partial tiles of at most M rows added to dw0 one after the other"""
    return sum_bound(M, absprod) + (splits + 1) * U * (np.abs(dw0) + absprod) * (1 + 1e-3)


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def upsample221(r):
    return np.repeat(np.repeat(r, 2, axis=1), 2, axis=2)


def epilogue(acc, err, bias=None, scale=None, shift=None, res=None, res_mode=0, act=0, split_n=0, y0=None):
    """epi_store of conv3d.hip on the exact sums `acc` [..., N] that the device
    holds within `err`: bias, z, scale / shift, residual 1 (same shape; the
    device reads it with the output's row stride ldy) or 2 ((2,2,1)-upsampled
    [B, OH/2, OW/2, OD, N]), activation 0 / 1 ReLU / 2 sigmoid, residual 3 (added
    after the activation), the split at split_n into (y, y2), accumulate onto y0.
    Returns z, pre (the activation's argument) and y with their bounds; yerr is
    None after a sigmoid."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)   # noqa: E731
    bias, scale, shift, res, y0 = f(bias), f(scale), f(shift), f(res), f(y0)
    v = np.asarray(acc, np.float64)
    err = np.asarray(err, np.float64)
    if bias is not None:
        v = v + bias
        err = _round(v, err)
    out = {"z": v, "zerr": err}
    if scale is not None:
        m = v * scale
        err = _round(m, err * np.abs(scale))
        v = m + shift
        err = _round(v, err)
    if res_mode == 1:
        v = v + res
        err = _round(v, err)
    elif res_mode == 2:
        v = v + upsample221(res)
        err = _round(v, err)
    out["pre"], out["preerr"] = v, err
    if act == 1:
        v = np.maximum(v, 0.0)                      # 1-Lipschitz, exact
    elif act == 2:
        v, err = sigmoid(v), None
    if res_mode == 3:
        v = v + res
        err = None if err is None else _round(v, err)
    if y0 is not None:
        assert not split_n
        v = v + y0
        err = None if err is None else _round(v, err)
    out["y"], out["yerr"] = v, err
    if split_n:
        out["y"], out["y2"] = v[..., :split_n], v[..., split_n:]
        if err is not None:
            out["yerr"], out["y2err"] = err[..., :split_n], err[..., split_n:]
        else:
            out["y2err"] = None
    return out


def relu_ambiguous(pre, preerr):
    """how many pre-activations lie within their bound of zero"""
    return int((np.abs(pre) <= preerr).sum())


RELU_CAP = 1e-3                 # of a tensor's elements


# --------------------------------------------------------------------------- dispatch
def gemm_path(M, N, K, nbatch, bt, avec, epi_flags, ncu=NCU):
    """The conv_gemm_kernel instantiation dispatch_gemm<BT, AVEC> /
    launch_gemm launch for a GEMM of M rows, N columns,
    nbatch batches: ("gemm", BM, BN, "bt" | "nt", "avec" | "scalar", "x3" | "f32",
    "persist" | "grid", "fbn" | "").  epi_flags: the names of whatever makes the
    epilogue not "plain" (launch_gemm: bias, scale, res, act, z, split,
    accumulate, deconv, fbn, ldy % 4); "fbn" selects the fused-BN form.  K does
    not steer the dispatch (BK = 32 everywhere; a BK = 64 form is never launched)."""
    if N <= 32:
        bm, bn = 128, 32
    elif N <= 64:
        bm, bn = 128, 64
    else:
        blocks128 = cdiv(M, 128) * cdiv(N, 128) * nbatch
        bm, bn = (64, 128) if blocks128 < 512 else (128, 128)
    t = "bt" if bt else "nt"
    if bt and "fbn" in epi_flags:
        return ("gemm", bm, bn, t, "avec" if avec else "scalar", "x3" if avec else "f32", "grid", "fbn")
    if not avec:
        return ("gemm", bm, bn, t, "scalar", "f32", "grid", "")       # NBUF = 2
    tiles = cdiv(M, bm) * cdiv(N, bn) * nbatch
    persist = nbatch > 1 and not epi_flags and tiles > 2 * (ncu * 3)
    x3 = bt or bn >= 64
    return ("gemm", bm, bn, t, "avec", "x3" if x3 else "f32", "persist" if persist else "grid", "")


def _wg_out(splits, per, det, scratch_floats):
    """wg_out: (splits, target)"""
    if not det:
        return splits, "atomic"
    fit = scratch_floats // per
    if splits <= 1 or fit < 2:
        return 1, "plain"
    return min(splits, fit), "reduce"


def _m_splits(M, tiles, minm, mround, det, scratch_floats, per, aim=1024):
    """the split arithmetic shared by launch_wgrad and
    launch_wgrad_x3: (splits, mper, target)"""
    splits = max(1, min(cdiv(aim, tiles), cdiv(M, minm)))
    splits, target = _wg_out(splits, per, det, scratch_floats)
    mper = cdiv(cdiv(M, splits), mround) * mround
    return cdiv(M, mper), mper, target


def wgrad_path(M, Cin, taps, Cout, unit_s1, det=False, scratch_floats=0, ncu=NCU):
    """The kernel m3d_conv3d_bwd_weight launches, with
    launch_wgrad, launch_wgrad_x3, launch_wgrad_tr
    and wg_out: (instantiation, target, splits, mper).  The
    instantiation names the kernel and its template arguments; target is where
    its partial tiles go ("atomic", "reduce" = wg_reduce_kernel, "plain").  splits
    is the number of additions one dW element receives (an upper bound on the
    stream-K path).  unit_s1: 1x1x1, stride 1, no padding, same grid."""
    K, N = taps * Cin, Cout
    vec = Cin % 4 == 0
    minm = TUNE["M3D_TUNE_WGRAD_MINM"]
    if vec and unit_s1 and Cout >= TUNE["M3D_TUNE_WGRAD1_X3_MIN_N"]:
        if K >= 192 and N >= 192:
            tiles = cdiv(K, 256) * cdiv(N, 256)
            trm = TUNE["M3D_TUNE_X3W_TR_MINM"]
            if not det and M >= TUNE["M3D_TUNE_X3W_SK_MIN_STEPS"] * W2_BK:
                nk, tn = cdiv(M, W2_BK), cdiv(N, 256)
                units = tiles * nk
                G = max(min(cdiv(units, cdiv(trm, W2_BK)), ncu) // tn * tn, tn)
                return ("x3_wgrad_tr", "sk"), "atomic", cdiv(nk, units // G) + 1, None
            splits = max(1, min(cdiv(ncu, tiles), cdiv(M, trm)))
            splits, target = _wg_out(splits, K * N, det, scratch_floats)
            mper = cdiv(cdiv(M, splits), W2_BK) * W2_BK
            return ("x3_wgrad_tr", "grid"), target, cdiv(M, mper), mper
        if K <= 64 or N <= 64:
            tiles = cdiv(K, 64) * cdiv(N, 64)
            s, mper, target = _m_splits(M, tiles, max(minm, 64), 64, det, scratch_floats, K * N)
            return ("x3_wgrad64",), target, s, mper
        tiles = cdiv(K, 128) * cdiv(N, 128)
        s, mper, target = _m_splits(M, tiles, max(minm, 32), 32, det, scratch_floats, K * N)
        return ("x3_wgrad",), target, s, mper
    if vec and K <= 64:
        bi, bj = (64, 64) if Cout <= 64 else (64, 128)
    elif Cout <= 64:
        bi, bj = 128, 64
    else:
        bi, bj = 128, 128
    tiles = cdiv(K, bi) * cdiv(N, bj)
    s, mper, target = _m_splits(M, tiles, max(minm, 32), 32, det, scratch_floats, K * N)
    return ("wgrad", bi, bj, "vec" if vec else "scalar"), target, s, mper


# --------------------------------------------------------------------------- cases
def _seed(*key):
    return np.random.default_rng([ord(c) for c in "".join(str(k) for k in key)])


def _ro(a):
    a.setflags(write=False)
    return a


def relu_bias(acc, rng):
    """A bias that keeps ReLU arguments away from zero without fixing their
    sign: +-3.5 standard deviations of the sums, alternating by channel (both
    branches are taken in every channel pair, and a small share of each
    channel crosses over).  Float32."""
    n = acc.shape[-1]
    s = 3.5 * float(acc.std())
    return ((np.where(np.arange(n) % 2 == 0, s, -s)) * rng.uniform(0.9, 1.1, n)).astype(F)


# Forward cases of m3d_conv3d_fwd / _dil.  Fields: B, sp (H, W, D), cin, cout,
# k, stride, padding ("same" | "valid" | (out, pad_before)), dil, and the
# epilogue: bias, bn, res_mode, act, z (z_out given), ldy (0: Cout), split
# (C, cp: Cout = cp, split_n = ldy = C, ldy2 = cp - C).
def _fc(cid, cin, cout, k, sp, stride=(1, 1, 1), padding="same", dil=(1, 1, 1), B=2, bias=True, bn=False,
        res_mode=0, act=0, z=False, ldy=0, split=None):
    return dict(id=cid, B=B, sp=sp, cin=cin, cout=cout, k=k, stride=stride, padding=padding, dil=dil, bias=bias,
                bn=bn, res_mode=res_mode, act=act, z=z, ldy=ldy, split=split)


K1, K3, K7, S1, S221 = (1, 1, 1), (3, 3, 3), (7, 7, 7), (1, 1, 1), (2, 2, 1)
FWD_CASES = [
    _fc("t128x32-avec", 32, 20, K3, (5, 4, 3)),                                     # M = 120: one ragged tile
    _fc("t128x64-bn-relu-z", 64, 52, K1, (6, 5, 3), stride=S221, padding="valid", bn=True, act=1, z=True),
    _fc("t64x128-res1-relu", 32, 132, K3, (5, 5, 5), res_mode=1, act=1),             # M = 250, epi_store4_pre
    _fc("t64x128-plain", 32, 132, K3, (5, 5, 5), bias=False),                       # epi_store4
    _fc("t128x128-big", 32, 256, K1, (33, 31, 33), B=1, act=1),                     # M = 33759: 528 blocks
    _fc("scalar-c3-k333", 3, 36, K3, (5, 4, 3)),                                    # K = 81
    _fc("scalar-c48-k111", 48, 20, K1, (5, 4, 3), act=1),
    _fc("scalar-stem-c32", 1, 32, K7, (9, 8, 7), stride=S221),                      # not stem_ok: Cout != 64
    _fc("scalar-stem-s111", 1, 64, K7, (9, 8, 7), bn=True, act=1),                  # not stem_ok: stride 1
    _fc("scalar-c6-n132", 6, 132, K3, (5, 4, 3)),                                   # 64x128 tile, scalar A
    _fc("dil2-res3-bn-relu", 32, 32, K3, (5, 4, 6), dil=(2, 2, 2), bn=True, act=1, res_mode=3),
    _fc("dil123", 32, 20, K3, (5, 6, 7), dil=(1, 2, 3)),
    _fc("res2-relu", 64, 36, K1, (4, 6, 3), padding="valid", res_mode=2, act=1),
    _fc("aniso-k132", 32, 20, (1, 3, 2), (4, 7, 5), stride=(1, 2, 1), padding=((4, 4, 5), (0, 1, 0))),
    _fc("split-2-4-sigmoid", 32, 4, K1, (1, 1, 300), B=1, padding="valid", act=2, z=True, split=(2, 4)),
    _fc("split-5-8-sigmoid", 32, 8, K1, (1, 1, 300), B=1, padding="valid", act=2, z=True, split=(5, 8)),
    # ldy < ldy2: a y2 stored with y's row stride lands inside y2, in the wrong rows
    _fc("split-2-8-sigmoid", 32, 8, K1, (1, 1, 300), B=1, padding="valid", act=2, z=True, split=(2, 8)),
    _fc("ldy48-res1", 32, 36, K1, (5, 4, 3), padding="valid", res_mode=1, ldy=48),
    _fc("ldy38-res1-z", 32, 36, K1, (5, 4, 3), padding="valid", res_mode=1, z=True, ldy=38),
    _fc("ldy38-res3-relu", 32, 36, K1, (5, 4, 3), padding="valid", res_mode=3, act=1, ldy=38),
]
# the scalar-A 128x128 tile needs 512 blocks of a Cin % 32 != 0 conv
FWD_CASES.append(_fc("scalar-c4-big", 4, 132, K1, (33, 31, 33), B=1, padding="valid"))   # 264 x 2 blocks, 18 MB


def fwd_geom(c):
    if isinstance(c["padding"], str):
        return geom(c["sp"], c["k"], c["stride"], c["padding"], c["dil"])
    return c["padding"]


def fwd_flags(c):
    fl = set()
    for name, on in (("bias", c["bias"]), ("scale", c["bn"]), ("res", c["res_mode"]), ("act", c["act"]),
                     ("z", c["z"]), ("split", c["split"]),
                     ("ldy", (c["split"][0] if c["split"] else c["ldy"] or c["cout"]) % 4)):
        if on:
            fl.add(name)
    return fl


def fwd_path(c, ncu=NCU):
    out, _ = fwd_geom(c)
    M = c["B"] * out[0] * out[1] * out[2]
    return gemm_path(M, c["cout"], math.prod(c["k"]) * c["cin"], 1, False, c["cin"] % 32 == 0, fwd_flags(c), ncu)


def fwd_data(c):
    """inputs (float32) and float64 results of a forward case: a dict with x, w,
    bias, scale, shift, res, and the epilogue()'s outputs"""
    rng = _seed("fwd", c["id"])
    out, pad = fwd_geom(c)
    B, cin, cout, k = c["B"], c["cin"], c["cout"], c["k"]
    K = math.prod(k) * cin
    x = rng.normal(size=(B, *c["sp"], cin)).astype(F)
    w = rng.normal(0, 1.0 / math.sqrt(K), (*k, cin, cout)).astype(F)
    acc = conv_fwd(x, w, k, c["stride"], pad, c["dil"], out)
    err = sum_bound(K, absprod_fwd(x, w, k, c["stride"], pad, c["dil"], out))
    bias = scale = shift = res = None
    if c["bias"]:
        bias = relu_bias(acc, rng) if c["act"] == 1 else rng.normal(0, 0.3, cout).astype(F)
    if c["bn"]:
        scale, shift = rng.uniform(0.5, 1.5, cout).astype(F), rng.normal(0, 0.1, cout).astype(F)
    if c["res_mode"] in (1, 3):
        res = rng.normal(0, 0.3, acc.shape).astype(F)
    elif c["res_mode"] == 2:
        res = rng.normal(0, 0.3, (B, out[0] // 2, out[1] // 2, out[2], cout)).astype(F)
    r = epilogue(acc, err, bias, scale, shift, res, c["res_mode"], c["act"], c["split"][0] if c["split"] else 0)
    r.update(x=x, w=w, bias=bias, scale=scale, shift=shift, res=res, out=out, pad=pad)
    return {key: _ro(v) if isinstance(v, np.ndarray) else v for key, v in r.items()}


# Data-gradient cases of m3d_conv3d_bwd_data (each run with accumulate 0 and 1):
# (id, cin, cout, k, stride, padding, sp)
BWD_DATA_CASES = [
    ("flip-c4", 4, 32, K3, S1, "same", (5, 4, 3)),            # N = 4: 128x32
    ("flip-c64", 64, 32, K3, S1, "same", (5, 4, 3)),          # 128x64
    ("flip-c132", 132, 32, K3, S1, "same", (5, 4, 3)),        # 64x128, second column tile 4 wide
    ("valid", 8, 32, K3, S1, "valid", (6, 5, 4)),             # pad' = 2
    ("k133", 8, 64, (1, 3, 3), S1, "same", (3, 5, 4)),        # pad' = (0, 1, 1)
    ("s221", 8, 32, K1, (2, 2, 1), "valid", (5, 7, 3)),
    ("s222", 8, 32, K1, (2, 2, 2), "valid", (5, 7, 3)),
    ("s112", 8, 32, K1, (1, 1, 2), "valid", (5, 7, 3)),
]
BWD_B = 2


def bwd_data_path(c, ncu=NCU):
    _, cin, cout, k, stride, padding, sp = c
    out, _ = geom(sp, k, stride, padding)
    grid = out if k == K1 else sp
    return gemm_path(BWD_B * math.prod(grid), cin, math.prod(k) * cout, 1, True, True, {"bwd"}, ncu)


def bwd_data_data(c):
    cid, cin, cout, k, stride, padding, sp = c
    rng = _seed("bwd", cid)
    out, pad = geom(sp, k, stride, padding)
    K = math.prod(k) * cout
    dz = rng.normal(size=(BWD_B, *out, cout)).astype(F)
    w = rng.normal(0, 1.0 / math.sqrt(K), (*k, cin, cout)).astype(F)
    dx0 = rng.normal(0, 0.5, (BWD_B, *sp, cin)).astype(F)
    shape = (BWD_B, *sp, cin)
    dx = conv_bwd_data(dz, w, shape, k, stride, pad, out)
    err = sum_bound(K, absprod_bwd_data(dz, w, shape, k, stride, pad, out))
    covered = conv_bwd_data(np.ones((BWD_B, *out, 1)), np.ones((*k, 1, 1)), (BWD_B, *sp, 1), k, stride, pad,
                            out)[..., 0] > 0
    return dict(dz=_ro(dz), w=_ro(w), dx0=_ro(dx0), dx=_ro(dx), err=_ro(err), covered=_ro(covered), out=out,
                pad=pad)


# Weight-gradient cases of m3d_conv3d_bwd_weight (each atomic, deterministic and
# deterministic with a scratch too small for two splits):
# (id, cin, cout, k, stride, padding, sp); B = 2
WGRAD_CASES = [
    ("w64x64-m16", 32, 24, K1, S221, "valid", (4, 3, 2)),             # M = 16 < 32
    ("w64x128-m1064", 64, 132, K1, (2, 2, 2), "valid", (13, 37, 7)),  # M = 2*512 + 40: 3 splits, the last ragged
    ("w128x64-vec-m1024", 8, 64, K3, S1, "same", (4, 8, 16)),         # M = 2 * mper
    ("w128x64-scalar", 3, 64, K3, S1, "same", (5, 4, 3)),
    ("w128x128-vec", 36, 132, K3, S1, "same", (5, 6, 7)),             # K = 972, N = 132: ragged both ways
    ("w128x128-scalar", 6, 68, K3, S1, "same", (5, 4, 3)),
    ("x3-below-n64", 32, 64, K1, S1, "valid", (5, 6, 7)),             # Cout 64 < 65: conv_wgrad_kernel<64,64>
    ("x3-64-n68", 32, 68, K1, S1, "valid", (5, 6, 7)),                # smallest Cout % 4 == 0 at or above 65
    ("x3-64-m1064", 64, 68, K1, S1, "valid", (7, 19, 4)),             # x3_wgrad64_kernel, 3 splits of 384
    ("x3-128-n68", 96, 68, K1, S1, "valid", (5, 6, 7)),               # x3_wgrad_kernel
    ("x3-128-m1064", 96, 132, K1, S1, "valid", (7, 19, 4)),
    ("x3-tr-m420", 192, 192, K1, S1, "valid", (5, 6, 7)),             # x3_wgrad_tr_kernel, split grid
    ("x3-tr-m1064", 192, 260, K1, S1, "valid", (7, 19, 4)),           # stream-K when atomic; 2 column tiles
]
WGRAD_MODES = ("atomic", "det", "det-small", "det-fit2")
DET_SMALL_BYTES = 4096          # the smallest legal scratch: fits no case's K*N twice


def wgrad_scratch_floats(c, mode):
    _, cin, cout, k, _, _, _ = c
    per = math.prod(k) * cin * cout
    return {"atomic": 0, "det": 8 * per, "det-small": DET_SMALL_BYTES // 4, "det-fit2": 2 * per}[mode]


def wgrad_path_of(c, mode, ncu=NCU):
    _, cin, cout, k, stride, padding, sp = c
    out, pad = geom(sp, k, stride, padding)
    unit_s1 = k == K1 and stride == S1 and out == tuple(sp)
    return wgrad_path(2 * math.prod(out), cin, math.prod(k), cout, unit_s1, mode != "atomic",
                      wgrad_scratch_floats(c, mode), ncu)


def wgrad_data(c):
    cid, cin, cout, k, stride, padding, sp = c
    rng = _seed("wgrad", cid)
    out, pad = geom(sp, k, stride, padding)
    x = rng.normal(size=(2, *sp, cin)).astype(F)
    dz = rng.normal(size=(2, *out, cout)).astype(F)
    dw0 = rng.normal(0, 3.0, (*k, cin, cout)).astype(F)
    dw = conv_bwd_weight(x, dz, k, stride, pad, out, dw0)
    ap = absprod_bwd_weight(x, dz, k, stride, pad, out)
    return dict(x=_ro(x), dz=_ro(dz), dw0=_ro(dw0), dw=_ro(dw), absprod=_ro(ap), out=out, pad=pad,
                M=2 * math.prod(out))


# m3d_deconv3d_k2s2: (id, B, sp, cin, cout, act)
DECONV_CASES = [
    ("n32-relu", 2, (3, 5, 7), 32, 4, 1),             # 128x32
    ("n64-none", 2, (3, 5, 7), 32, 8, 0),             # 128x64
    ("n288-none", 2, (3, 5, 7), 64, 36, 0),           # 64x128, third column tile 32 wide
    ("n288-relu", 2, (3, 5, 7), 64, 36, 1),
    ("n288-sigmoid", 2, (3, 5, 7), 64, 36, 2),
    ("n256-big-relu", 1, (33, 31, 33), 32, 32, 1),    # 128x128: 264 x 2 blocks
]


def deconv_path(c, ncu=NCU):
    _, B, sp, cin, cout, act = c
    return gemm_path(B * math.prod(sp), 8 * cout, cin, 1, True, True, {"deconv"}, ncu)


def deconv_data(c):
    cid, B, sp, cin, cout, act = c
    rng = _seed("deconv", cid)
    x = rng.normal(size=(B, *sp, cin)).astype(F)
    w = rng.normal(0, 1.0 / math.sqrt(cin), (2, 2, 2, cout, cin)).astype(F)
    bias = relu_bias(deconv_k2s2_sum(x, w), rng) if act == 1 else rng.normal(0, 0.3, cout).astype(F)
    y, yerr, pre, preerr = deconv_k2s2(x, w, bias, act)
    return dict(x=_ro(x), w=_ro(w), bias=_ro(bias), y=_ro(y), yerr=yerr, pre=pre, preerr=preerr)


# m3d_gemm_f32_ex: (id, batch, M, K, N, lda, shared operands, bias, act, accumulate); batch None: the
# persistent size, persist_batch(ncu, M, N)
PERSIST_M = 128 * 12 + 5
GEMM_CASES = [
    ("novec-k40-lda44", 2, 130, 40, 36, 44, False, True, 0, 0),
    ("shared-ab", 3, 70, 32, 20, 32, True, False, 0, 0),
    ("acc-bias-relu", 2, 200, 64, 132, 64, False, True, 1, 1),
    ("persist-n32", None, PERSIST_M, 32, 32, 32, False, False, 0, 0),
    ("persist-n64", None, PERSIST_M, 32, 64, 32, False, False, 0, 0),
    ("grid-n32-bias", None, PERSIST_M, 32, 32, 32, False, True, 0, 0),
    ("grid-n64-bias", None, PERSIST_M, 32, 64, 32, False, True, 0, 0),
    # the 128x128 persistent form: ragged tiles count in full, so 5 rows x 132 columns are two tiles per
    # batch (the second 4 columns wide) and the batches alone pass 512 blocks and 6 * CUs tiles
    ("persist-n132", None, 5, 32, 132, 32, False, False, 0, 0),
    ("grid-n132-bias", None, 5, 32, 132, 32, False, True, 0, 0),
]


def persist_batch(ncu, M, N):
    """batches of M x N products that pass 6 * CUs tiles by about 5 % (and, for N > 64, the 512 blocks
    of 128 rows from which dispatch_gemm takes the 128x128 tile)"""
    per = cdiv(M, 128) * cdiv(N, 32 if N <= 32 else 64 if N <= 64 else 128)
    batch = (6 * ncu * 105 // 100) // per + 1
    return batch if N <= 64 else max(batch, cdiv(512, per))


def gemm_case_path(c, ncu=NCU):
    _, batch, M, K, N, lda, shared, bias, act, acc = c
    batch = persist_batch(ncu, M, N) if batch is None else batch
    fl = {n for n, on in (("bias", bias), ("act", act), ("accumulate", acc)) if on}
    return gemm_path(M, N, K, batch, False, K % 32 == 0 and lda % 4 == 0, fl, ncu)


def gemm_data(c, ncu=NCU):
    cid, batch, M, K, N, lda, shared, bias, act, acc = c
    batch = persist_batch(ncu, M, N) if batch is None else batch
    rng = _seed("gemm", cid.replace("grid", "persist").replace("-bias", ""))     # the grid twin: same A, B
    nb = 1 if shared else batch
    A = rng.normal(size=(nb, M, lda)).astype(F)
    Bm = rng.normal(0, 1.0 / math.sqrt(K), (nb, K, N)).astype(F)
    prod = gemm(A[..., :K], Bm)
    err = sum_bound(K, absprod_gemm(A[..., :K], Bm))
    if shared:
        prod, err = np.repeat(prod, batch, 0), np.repeat(err, batch, 0)
    brng = _seed("gemm-bias", cid)
    b = None
    if bias:
        b = relu_bias(prod, brng) if act == 1 else brng.normal(0, 0.3, N).astype(F)
    c0 = brng.normal(0, 0.5, (batch, M, N)).astype(F) if acc else None
    r = epilogue(prod, err, bias=b, act=act, y0=c0)
    return dict(A=_ro(A), B=_ro(Bm), bias=b, c0=c0, y=r["y"], yerr=r["yerr"], pre=r["pre"], preerr=r["preerr"],
                batch=batch)


# Split-K entries on B, out = (1, (4, 4, 6)), M = 96:
# fwd: (id, splits, cin, cout, stride, bias, bn, res_mode, act, z)
SPLITK_OUT = (4, 4, 6)
SPLITK_FWD_CASES = [
    ("fwd-s2-res2-relu", 2, 512, 36, S1, True, False, 2, 1, False),
    ("fwd-s4-res3-bn-relu", 4, 512, 64, S1, True, True, 3, 1, True),
    ("fwd-s8-sigmoid", 8, 512, 36, S221, True, False, 0, 2, True),
    ("fwd-s2-res1-n512", 2, 64, 512, S1, False, False, 1, 0, False),
]
# bwd-data: (id, splits, cin, cout, stride, accumulate)
SPLITK_BWD_CASES = [
    ("bwd-s2-acc", 2, 36, 512, S1, 1),
    ("bwd-s4-s221", 4, 36, 512, S221, 0),
    ("bwd-s4-s221-acc", 4, 64, 512, S221, 1),
    ("bwd-s8", 8, 20, 512, S1, 0),
]


# The persistent B^T forms: data gradients in so many K-slices, on so many rows, that the slices' plain
# partial GEMMs pass 6 * CUs tiles (only a caller asking for more slices than m3d_conv3d_splitk_count
# gives gets here; the entry takes any count up to 64).  Cin picks the tile: 4 -> 128x32, 36 -> 128x64.
# The 128x128 tile would need a 52 MB workspace at full tiles, but ragged tiles count in full: the wide
# case has 5 rows (one row tile) and as many column tiles as it takes (Cin None: splitk_persist_geom;
# 3204 at 256 CUs, the last tile 4 wide).  At 64 slices of Cout 2048 a slice is one k-tile.
# At 256 CUs: dz 26 / 26 / 0.04 MB, workspace 3 / 30 / 4 MB, the wide case's kernel 26 MB.
SPLITK_PERSIST_CASES = [
    ("bwd-s8-persist-c4", 8, 4, 256, S1, 0),
    ("bwd-s64-persist-c36", 64, 36, 2048, S1, 0),
    ("bwd-s64-persist-wide", 64, None, 2048, S1, 0),
]


def splitk_persist_geom(c, ncu):
    """(the case with its Cin filled in, its output grid): tiles of 128 rows (c4, c36) or of 128
    columns (wide) that, times the slices, pass 6 * CUs by about 5 % (wide: and the 512 blocks of the
    128x128 tile); the last row tile of c36 holds 8 rows"""
    splits, cin = c[1], c[2]
    n = (6 * ncu * 105 // 100) // splits + 1
    if cin is None:
        n = max(n, cdiv(512, splits))
        return (c[0], splits, (n - 1) * 128 + 4, *c[3:]), (1, 5, 1)
    return c, ((n, 16, 8) if splits == 8 else ((n - 1) * 16 + 1, 4, 2))


def splitk_in_sp(stride, out=SPLITK_OUT):
    """an input volume with odd sizes where strided, whose strided 1x1x1 conv has the output `out`"""
    return tuple((o - 1) * s + 1 for o, s in zip(out, stride))


def splitk_paths(c, fwd, ncu=NCU, out=SPLITK_OUT):
    """(the partial GEMM's instantiation, the reduce kernel)"""
    splits, cin, cout = c[1], c[2], c[3]
    M = math.prod(out)
    if fwd:
        return gemm_path(M, cout, cin // splits, splits, False, True, set(), ncu), ("splitk_epi",)
    return gemm_path(M, cin, cout // splits, splits, True, True, set(), ncu), ("splitk_epi",)


def splitk_fwd_case(c):
    """a SPLITK_FWD_CASES entry as a forward case"""
    cid, splits, cin, cout, stride, bias, bn, res_mode, act, z = c
    return _fc(cid, cin, cout, K1, splitk_in_sp(stride), stride=stride, padding="valid", B=1, bias=bias, bn=bn,
               res_mode=res_mode, act=act, z=z)


def splitk_fwd_data(c):
    return fwd_data(splitk_fwd_case(c))


def splitk_bwd_data(c, out=SPLITK_OUT):
    cid, splits, cin, cout, stride, acc = c
    rng = _seed("splitk", cid)
    sp = splitk_in_sp(stride, out)
    dz = rng.normal(size=(1, *out, cout)).astype(F)
    w = rng.normal(0, 1.0 / math.sqrt(cout), (1, 1, 1, cin, cout)).astype(F)
    dx0 = rng.normal(0, 0.5, (1, *sp, cin)).astype(F)
    shape = (1, *sp, cin)
    dx = conv_bwd_data(dz, w, shape, K1, stride, (0, 0, 0), out)
    err = sum_bound(cout, absprod_bwd_data(dz, w, shape, K1, stride, (0, 0, 0), out))
    covered = np.zeros((1, *sp), bool)
    covered[:, ::stride[0], ::stride[1], ::stride[2]] = True
    return dict(dz=_ro(dz), w=_ro(w), dx0=_ro(dx0), dx=_ro(dx), err=_ro(err), covered=_ro(covered), sp=sp)


# --------------------------------------------------------------------------- coverage
def all_paths(ncu=NCU):
    """{instantiation: [case ids]} over every table above"""
    paths = {}

    def add(p, cid):
        paths.setdefault(p, []).append(cid)
    for c in FWD_CASES:
        add(fwd_path(c, ncu), "fwd:" + c["id"])
    for c in BWD_DATA_CASES:
        add(bwd_data_path(c, ncu), "bwd_data:" + c[0])
    for c in DECONV_CASES:
        add(deconv_path(c, ncu), "deconv:" + c[0])
    for c in GEMM_CASES:
        add(gemm_case_path(c, ncu), "gemm:" + c[0])
    for c in SPLITK_FWD_CASES:
        for p in splitk_paths(c, True, ncu):
            add(p, "splitk:" + c[0])
    for c in SPLITK_BWD_CASES:
        for p in splitk_paths(c, False, ncu):
            add(p, "splitk:" + c[0])
    for c in SPLITK_PERSIST_CASES:
        pc, out = splitk_persist_geom(c, ncu)
        for p in splitk_paths(pc, False, ncu, out):
            add(p, "splitk:" + c[0])
    for c in WGRAD_CASES:
        for mode in WGRAD_MODES:
            p, target, _, _ = wgrad_path_of(c, mode, ncu)
            add(p, "wgrad:%s-%s" % (c[0], mode))
            add(("wg_target", p[0], target), "wgrad:%s-%s" % (c[0], mode))
            if target == "reduce":
                add(("wg_reduce",), "wgrad:%s-%s" % (c[0], mode))
    return paths
