"""Plain numpy references of the kernels in csrc/elementwise.hip -- test
infrastructure, no GPU.  Written from the kernel comments and include/m3d.h.
Everything is channels-last [B, H, W, D, C]; the shapes the tests use are tiny,
so the pools vectorise over B and C and loop over window positions in Python.

What is exact and what is bounded
---------------------------------
* Max-pool forward / backward, the (2,2,1) resampling adjoints and the
  elementwise outputs of the BN-ReLU backward consist of comparisons and of
  single float32 operations in a stated order.  The references below perform
  the same float32 operations in the same order (the library is compiled
  without FMA contraction), so the GPU must match them bit for bit.
* The three channel sums of ``m3d_bn_act_bwd`` and the optimizers' clip norms
  are long float32 sums.  They are compared with float64 sums under a bound
  that is derived here from the addition depth of the kernels (``bn_sum_depth``
  and ``norm_depth``), never from what the kernels return.

The sum bound.  With u = 2^-24, a float32 sum in which no term passes through
more than d rounded operations (the roundings that form the term included)
satisfies, to first order in u and for any association,

    |fl(sum) - sum| <= d * u * sum |term|

(every rounding multiplies the partial sum it acts on by (1 + e), |e| <= u,
and a partial sum is bounded by the sum of the magnitudes of its terms).  The
second-order part, below d^2 u^2 / 2 * sum |term|, is covered by slack in
the count: every chain of additions starts from a zero accumulator, so its
first addition is exact but is counted (at least three such chains lie on
every path: per-thread rows, the fold accumulator, the destination's +=), and
d^2 u / 2 < 1 needs only d < 5792; the depths here stay below 100.
"""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24

# The cases of tests/test_gpu_elementwise_paths.py; tests/test_ewref.py checks
# the references at the same ones.
# (id, C, k, stride, padding, (H, W, D))
POOL_CASES = [
    ("scalar-c6", 6, (3, 3, 3), (2, 2, 1), "same", (7, 6, 9)),
    ("333-d1", 8, (3, 3, 3), (2, 2, 1), "same", (7, 6, 1)),
    ("333-d8", 8, (3, 3, 3), (2, 2, 1), "same", (6, 7, 8)),
    ("333-d9", 8, (3, 3, 3), (2, 2, 1), "same", (5, 5, 9)),
    ("333-d21", 8, (3, 3, 3), (2, 2, 1), "same", (4, 9, 21)),
    ("4z-s111", 8, (3, 3, 3), (1, 1, 1), "same", (5, 6, 9)),
    ("4z-k335", 8, (3, 3, 5), (2, 2, 1), "same", (6, 5, 10)),
    ("4z-valid", 8, (3, 3, 3), (2, 2, 1), "valid", (7, 8, 11)),
    ("4z-k223", 8, (2, 2, 3), (2, 2, 1), "same", (5, 5, 8)),
    ("4z-k111", 8, (1, 1, 1), (2, 2, 1), "valid", (5, 6, 3)),
    ("4-k222-valid", 4, (2, 2, 2), (2, 2, 2), "valid", (7, 7, 7)),
    ("4-k222-same", 4, (2, 2, 2), (2, 2, 2), "same", (7, 7, 7)),
    ("4-k333-s222", 8, (3, 3, 3), (2, 2, 2), "same", (6, 7, 9)),
]
# the scalar case's geometry at C = 8, run on tensors that are not 16-byte aligned
POOL_MISALIGNED = ("misaligned-c8", 8, (3, 3, 3), (2, 2, 1), "same", (7, 6, 9))
POOL_B = 2
# (M, C, relu, affine) of the m3d_bn_act_bwd cases (affine False: scale, mean
# and rstd NULL)
BN_CASES = [(5, 4, 1, True), (300, 12, 0, False), (700, 1028, 1, True), (1100, 2048, 1, True),
            (40000, 64, 1, True), (262444, 4, 0, True)]


# Cases with a NaN, a +inf and a -inf planted: ((y, x) of a voxel column that is
# the first tap (ky = kx = 0) of output (1, 1), (y, x) of one that is only ever
# a later tap (ky = kx = 1)).  The z stride is 1, so the first column's voxel at
# z is tap kz = 0 of one output and a later tap of its z neighbours.
POOL_SPECIAL = {"333-d9": ((1, 1), (2, 2)), "4z-valid": ((2, 2), (3, 3))}
SPECIAL_VALUES = (np.nan, np.inf, -np.inf)


def special_voxels(case_id):
    """[(b, y, x, z, c, value)] planted by pool_input."""
    (fy, fx), (ly, lx) = POOL_SPECIAL[case_id]
    out = []
    for j, v in enumerate(SPECIAL_VALUES):
        out.append((0, fy, fx, 2 + 2 * j, 0, v))
        out.append((1, ly, lx, 2 + 2 * j, 5, v))
    return out


def pool_input(case_id, C, spatial):
    """The pool cases' input [POOL_B, H, W, D, C]: values on a 0.25 grid in
    [-1, 1], so equal maxima inside a window are common; the POOL_SPECIAL cases
    with their non-finite voxels."""
    rng = np.random.default_rng([ord(ch) for ch in case_id] + [C, *spatial])
    x = (rng.integers(-4, 5, (POOL_B, *spatial, C)) * 0.25).astype(F)
    if case_id in POOL_SPECIAL:
        for b, iy, ix, iz, c, v in special_voxels(case_id):
            x[b, iy, ix, iz, c] = v
    return x


def window_hits(voxel, spatial, k, stride, pad, out):
    """[(oy, ox, oz, is_first)]: the outputs whose window holds the voxel (y, x,
    z), and whether it is the first in-range tap of that window."""
    H, W, D = spatial
    hits = []
    for oy in range(out[0]):
        for ox in range(out[1]):
            for oz in range(out[2]):
                lo = (oy * stride[0] - pad[0], ox * stride[1] - pad[1], oz * stride[2] - pad[2])
                if all(l <= v < l + kk for l, v, kk in zip(lo, voxel, k)):
                    first = tuple(max(l, 0) for l in lo)
                    hits.append((oy, ox, oz, first == tuple(voxel)))
    return hits


# --------------------------------------------------------------------------- max-pool
def same_out_pad(n, k, s):
    """TF 'SAME': (output size, pad before); the extra pad goes after."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2


def pool_geometry(spatial, k, stride, padding):
    """(out, pad) of KL.MaxPooling3D(k, stride, padding) on (H, W, D)."""
    if padding == "same":
        op = [same_out_pad(n, kk, s) for n, kk, s in zip(spatial, k, stride)]
        return tuple(o for o, _ in op), tuple(p for _, p in op)
    assert padding == "valid"
    return tuple((n - kk) // s + 1 for n, kk, s in zip(spatial, k, stride)), (0, 0, 0)


def maxpool_fwd(x, k, stride, pad, out):
    """x [B,H,W,D,C] float32 -> (y float32, argmax uint8), both [B,OH,OW,OD,C].

    The kernels' rule: the window is scanned in (ky, kx, kz) order over its
    in-range taps, the first in-range value initialises the maximum and a later
    one replaces it on strict '>'; argmax is (ky*kw + kx)*kd + kz.  Hence the
    first of equal maxima wins, a NaN at the first tap stays (nothing compares
    greater than it) and a NaN at a later tap is never taken; +-inf need no
    special case."""
    x = np.asarray(x, F)
    B, H, W, D, C = x.shape
    (kh, kw, kd), (sy, sx, sz), (py, px, pz), (OH, OW, OD) = k, stride, pad, out
    best = np.full((B, OH, OW, OD, C), -np.inf, F)
    arg = np.zeros((B, OH, OW, OD, C), np.uint8)
    seen = np.zeros((OH, OW, OD), bool)
    for ky in range(kh):
        iy = np.arange(OH) * sy - py + ky
        vy = (iy >= 0) & (iy < H)
        for kx in range(kw):
            ix = np.arange(OW) * sx - px + kx
            vx = (ix >= 0) & (ix < W)
            for kz in range(kd):
                iz = np.arange(OD) * sz - pz + kz
                vz = (iz >= 0) & (iz < D)
                v = x[:, np.clip(iy, 0, H - 1)][:, :, np.clip(ix, 0, W - 1)][:, :, :, np.clip(iz, 0, D - 1)]
                valid = vy[:, None, None] & vx[None, :, None] & vz[None, None, :]
                with np.errstate(invalid="ignore"):
                    gt = v > best
                take = valid[None, ..., None] & (~seen[None, ..., None] | gt)
                best = np.where(take, v, best)
                arg = np.where(take, np.uint8((ky * kw + kx) * kd + kz), arg)
                seen |= valid
    return best, arg


def maxpool_bwd(dy, argmax, in_shape, k, stride, pad):
    """dx [B,H,W,D,C] float32: per input voxel the sequential float32 sum,
    from 0, over the outputs (oy, ox, oz) ascending whose argmax byte names it
    (the kernels gather per input in exactly this order)."""
    dy = np.asarray(dy, F)
    argmax = np.asarray(argmax)
    B, H, W, D, C = in_shape
    (kh, kw, kd), (sy, sx, sz), (py, px, pz) = k, stride, pad
    _, OH, OW, OD, _ = dy.shape
    dx = np.zeros(in_shape, F)
    bi = np.broadcast_to(np.arange(B)[:, None], (B, C))
    ci = np.broadcast_to(np.arange(C)[None, :], (B, C))
    for oy in range(OH):
        for ox in range(OW):
            for oz in range(OD):
                a = argmax[:, oy, ox, oz, :].astype(np.int64)
                iy = oy * sy - py + a // (kw * kd)
                ix = ox * sx - px + (a // kd) % kw
                iz = oz * sz - pz + a % kd
                if not ((a < kh * kw * kd).all() and (iy >= 0).all() and (iy < H).all() and (ix >= 0).all()
                        and (ix < W).all() and (iz >= 0).all() and (iz < D).all()):
                    raise ValueError("maxpool_bwd: an argmax byte names a tap outside the input")
                # (b, c) pairs are distinct targets: a plain float32 add each
                dx[bi, iy, ix, iz, ci] = dx[bi, iy, ix, iz, ci] + dy[:, oy, ox, oz, :]
    return dx


# --------------------------------------------------------------------------- (2,2,1) resampling
def upsample221_bwd(d_up, d_src0=None):
    """Adjoint of UpSampling3D((2,2,1)): d_up [B,2H,2W,D,C] -> [B,H,W,D,C].
    float32 adds in the kernel's order: start value (d_src0, or 0 when not
    accumulating), then the taps (0,0), (0,1), (1,0), (1,1)."""
    d_up = np.asarray(d_up, F)
    B, H2, W2, D, C = d_up.shape
    acc = np.zeros((B, H2 // 2, W2 // 2, D, C), F) if d_src0 is None else np.array(d_src0, F)
    for a in range(2):
        for q in range(2):
            acc = acc + d_up[:, a::2, q::2]
    return acc


def subsample221_fwd(x):
    """P6 = MaxPooling3D((1,1,1), strides (2,2,1)): x[:, ::2, ::2]."""
    return np.ascontiguousarray(np.asarray(x, F)[:, ::2, ::2])


def subsample221_bwd(dy, dx0):
    """The adjoint accumulates: dx0 with dy added (float32) at [:, ::2, ::2]."""
    dx = np.array(dx0, F)
    dx[:, ::2, ::2] = dx[:, ::2, ::2] + np.asarray(dy, F)
    return dx


# --------------------------------------------------------------------------- frozen-BN affine
def bn_affine(gamma, beta, mean, var, eps):
    """(rstd, scale, shift) in float64 from the float32 inputs (eps as the
    float32 the C entry receives): rstd = 1/sqrt(var + eps), scale = gamma *
    rstd, shift = beta - mean * scale."""
    g, b, m, v = (np.asarray(a, F).astype(np.float64) for a in (gamma, beta, mean, var))
    rstd = 1.0 / np.sqrt(v + float(F(eps)))
    scale = g * rstd
    return rstd, scale, b - m * scale


# --------------------------------------------------------------------------- BN-ReLU backward
def bn_grid(C):
    """(T, R, groups) of bn_act_bwd_kernel: T threads (a power of two, at most
    256) cover T channel quads of a row, R = 256 / T rows per block pass,
    groups blocks along the channels."""
    quads = C // 4
    T = 1
    while T < quads and T < 256:
        T <<= 1
    return T, 256 // T, -(-quads // T)


def _chan(v, C, fill):
    return np.full(C, fill, F) if v is None else np.asarray(v, F)


def _dpre(dy, y, relu):
    dy = np.asarray(dy, F)
    if not relu:
        return dy
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(y, F) > 0, dy, F(0))       # y = 0, -0 or NaN: no gradient


def bn_act_bwd(dy, y, z, relu, scale, mean, rstd, dres0=None):
    """Backward of y = act(z*scale + shift [+ res]) on [M, C] float32 arrays
    (scale / mean / rstd None as the C entry's NULL: 1 / 0 / 1).

    Returns (g, dz, dres, sums, abs_sums):
    * g = dy masked by y > 0 (relu), dz = g * scale, dres = g (+ dres0 when
      accumulating) -- each one float32 operation, as the kernel forms them;
    * sums [3, C] float64: sum g, sum g*((z - mean)*rstd), sum g*scale, the
      terms exact in float64 from the float32 inputs, and abs_sums the same
      sums of the terms' magnitudes."""
    g = _dpre(dy, y, relu)
    M, C = g.shape
    sc, mu, rs = _chan(scale, C, 1), _chan(mean, C, 0), _chan(rstd, C, 1)
    dz = g * sc
    dres = g if dres0 is None else g + np.asarray(dres0, F)
    assert dz.dtype == F and dres.dtype == F
    g64 = g.astype(np.float64)
    zz = np.zeros((M, C)) if z is None else np.asarray(z, F).astype(np.float64)
    terms = np.stack([g64, g64 * ((zz - mu.astype(np.float64)) * rs.astype(np.float64)),
                      g64 * sc.astype(np.float64)])
    return g, dz, dres, terms.sum(1), np.abs(terms).sum(1)


def _fold_serial_adds(gx):
    """bn_sums_fold: the longest chain of serial additions into one of a
    thread's four accumulators (row group rg takes rows rg, rg + 64, ...: four
    per unrolled iteration while b + 192 < gx, then the tail into acc[0])."""
    worst = 0
    for rg in range(min(64, gx)):
        b, it = rg, 0
        while b + 192 < gx:
            b += 256
            it += 1
        tail = 0
        while b < gx:
            b += 64
            tail += 1
        worst = max(worst, it + tail)
    return worst


TERM_ROUNDINGS = 3          # g*((z - mean)*rstd): subtract, multiply, multiply (sum g: 0, sum g*scale: 1)


def bn_sum_depth(M, C, gx):
    """The largest number of float32 roundings any term of a channel sum of
    ``m3d_bn_act_bwd`` passes through, read off bn_act_bwd_kernel and
    bn_sums_fold (gx = the kernel's row blocks, i.e.
    m3d_bn_act_bwd_workspace_bytes(M, C) / (12 * C)):

    * forming the term: at most TERM_ROUNDINGS (3, for g*((z - mean)*rstd));
    * the thread's own rows r = bx*R + ty + i*gx*R < M, added one after the
      other: ceil(M / (gx*R)) additions;
    * the block's LDS tree over its R rows: log2 R additions (R = 1: none);
    * bn_sums_fold over the gx partial rows: the serial additions into one
      accumulator (_fold_serial_adds), 2 to combine the four accumulators as
      (a0 + a1) + (a2 + a3), 6 for the tree over the 64 row groups;
    * 1 for the += into the destination.

    The bound on a channel's sum is then bn_sum_depth * 2^-24 * (sum |term| +
    |destination's prior value|) -- the module docstring's inequality."""
    T, R, groups = bn_grid(C)
    rows = -(-M // (gx * R))
    return TERM_ROUNDINGS + rows + int(math.log2(R)) + _fold_serial_adds(gx) + 2 + 6 + 1


def bn_sum_bound(M, C, gx, abs_sums, dst0=None):
    """[3, C] float64 bound of the three channel sums (dst0: the [3, C] values
    the sums are added into)."""
    a = np.asarray(abs_sums, np.float64)
    if dst0 is not None:
        a = a + np.abs(np.asarray(dst0, np.float64))
    return bn_sum_depth(M, C, gx) * U * a


def bn_sums_simulated(dy, y, z, relu, scale, mean, rstd, gx, dst0=None):
    """The three channel sums [3, C] in float32 in the kernels' own order:
    per-thread rows, the LDS tree over the block's rows, bn_sums_fold (four
    accumulators per row group, their combine, the 64-group tree) and the +=
    into dst0 (zeros when None).  For the CPU self-test of bn_sum_bound."""
    g = _dpre(dy, y, relu)
    M, C = g.shape
    T, R, groups = bn_grid(C)
    sc, mu, rs = _chan(scale, C, 1), _chan(mean, C, 0), _chan(rstd, C, 1)
    zz = np.zeros((M, C), F) if z is None else np.asarray(z, F)
    terms = np.stack([g, g * ((zz - mu) * rs), g * sc])
    assert terms.dtype == F
    passes = -(-M // (gx * R))
    pad = np.zeros((3, passes * gx * R, C), F)       # rows past M add +0: exact
    pad[:, :M] = terms
    rows = pad.reshape(3, passes, gx, R, C)
    s = np.zeros((3, gx, R, C), F)
    for i in range(passes):
        s = s + rows[:, i]
    step = R // 2
    while step > 0:                                  # red[ty] += red[ty + step], ty < step
        s = np.concatenate([s[:, :, :step] + s[:, :, step:2 * step], s[:, :, step:]], axis=2)
        step //= 2
    part = s[:, :, 0]                                # [3, gx, C]
    red = np.zeros((3, 64, C), F)
    for rg in range(64):
        acc = np.zeros((4, 3, C), F)
        b = rg
        while b + 192 < gx:
            for u in range(4):
                acc[u] = acc[u] + part[:, b + 64 * u]
            b += 256
        while b < gx:
            acc[0] = acc[0] + part[:, b]
            b += 64
        red[:, rg] = (acc[0] + acc[1]) + (acc[2] + acc[3])
    step = 32
    while step > 0:
        red[:, :step] = red[:, :step] + red[:, step:2 * step]
        step //= 2
    dst = np.zeros((3, C), F) if dst0 is None else np.array(dst0, F)
    out = dst + red[:, 0]
    assert out.dtype == F
    return out


def bn_case(M, C, relu, affine):
    """Seeded inputs of one m3d_bn_act_bwd case: dy, y, z [M, C], scale / mean /
    rstd [C] (None when not affine), dres0 [M, C] and dst0 [3, C], the prior
    contents of dres and of the three sum destinations.  With relu, y holds an
    exact 0.0, a -0.0 and a NaN where dy is not zero (no gradient may pass)."""
    rng = np.random.default_rng([M, C, relu, int(affine)])
    d = {"dy": rng.normal(size=(M, C)).astype(F), "y": rng.normal(size=(M, C)).astype(F),
         "z": (rng.normal(size=(M, C)) * 2 + 0.5).astype(F),
         "dres0": rng.normal(size=(M, C)).astype(F), "dst0": rng.normal(size=(3, C)).astype(F),
         "scale": None, "mean": None, "rstd": None}
    if affine:
        d["scale"] = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F)
        d["mean"] = rng.normal(size=C).astype(F)
        d["rstd"] = rng.uniform(0.5, 2.0, C).astype(F)
    if relu:
        d["y"][0, 0], d["y"][1, 1], d["y"][2, 2] = 0.0, -0.0, np.nan
        d["dy"][0, 0], d["dy"][1, 1], d["dy"][2, 2] = 1.5, -2.5, 3.5
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


# --------------------------------------------------------------------------- optimizer clip norms
CHUNK = 1024                # floats per chunk of the flat parameter buffer
NORM_CHUNKS = 16            # chunks folded by one block of sgd_norm_kernel


def seg_sq_norm(g, w, l2):
    """float64 sum of (g + l2*w)^2 over one tensor (float32 g, w, l2)."""
    a = np.asarray(g, F).astype(np.float64) + float(F(l2)) * np.asarray(w, F).astype(np.float64)
    return float(np.sum(a * a))


def norm_depth(seg_chunks, n_chunks, deterministic):
    """Roundings a squared term passes through on its way into norms[seg].

    Both modes: 3 to form the term -- the multiply l2*w, the add to g, the
    square -- and 3 for the thread's a*a + b*b + c*c + d*d.
    Atomic mode (sgd_norm_kernel): at most NORM_CHUNKS additions of the
    thread's per-chunk values, 6 for the wave shuffle tree, 3 for red[0] +
    red[1] + red[2] + red[3], and one atomic per block that touches the
    segment, at most ceil(seg_chunks / NORM_CHUNKS) + 1, in any order.
    Deterministic mode (chunk_norm_kernel + seg_norm_kernel): 6 + 2 for the
    chunk's block sum, ceil(n_chunks / 256) serial additions per thread of
    seg_norm_kernel, 6 + 2 for its block sum.

    The terms are non-negative, so the bound depth * 2^-24 is relative to the
    norm itself, except for the rounding of a = g + l2*w, which is relative
    to |g| + |l2*w| rather than to |a|; ``norm_bound`` carries that part."""
    if deterministic:
        return 3 + 3 + (6 + 2) + -(-n_chunks // 256) + (6 + 2)
    return 3 + 3 + NORM_CHUNKS + 6 + 3 + -(-seg_chunks // NORM_CHUNKS) + 1


def norm_bound(g, w, l2, n_chunks, deterministic):
    """Absolute float64 bound on |norms[seg] - seg_sq_norm(g, w, l2)|:
    norm_depth * 2^-24 * sum a^2, plus the part of a's own rounding that is not
    relative to a: a_f32 = a(1 + e) + e'*|l2*w| gives a^2's error the extra
    2*|a|*|l2*w|*2^-24 per element."""
    g64 = np.asarray(g, F).astype(np.float64)
    lw = float(F(l2)) * np.asarray(w, F).astype(np.float64)
    a = g64 + lw
    seg_chunks = -(-g64.size // CHUNK)
    return U * (norm_depth(seg_chunks, n_chunks, deterministic) * float(np.sum(a * a)) +
                2.0 * float(np.sum(np.abs(a) * np.abs(lw))))
