"""Float64 NumPy restatement of the RPN head's backward (the contract of
m3d_rpn_head_compact_bwd_data / _bwd_weight, include/m3d.h).

The head, per pyramid level l (core/models.py:512-557, B = 1):
    s1 = relu(conv3x3x3(P_l, w1) + b1)        P_l [H][W][D][C0], s1 [..][C1]
    s2 = relu(s1 w2 + b2)                     [..][C2]
    z3 = s2 w24 + b24                         [..][8 apl] = [logits | bbox]
and its backward from dz3 = [dlogits | dbbox] over the level-concatenated rows:
    db24 = sum_r dz3               dw24 = s2^T dz3
    dz2  = (dz3 w24^T) [s2 > 0]    db2  = sum_r dz2      dw2 = s1^T dz2
    dz1  = (dz2 w2^T) [s1 > 0]     db1  = sum_r dz1
    dw1  = conv3x3x3's weight gradient of (P_l, dz1_l), summed over the levels
    dP_l = conv3x3x3's data gradient of dz1_l
written dense and independently of the compact form (no row list): the rows
whose dz3 is zero contribute exact zeros.  scan() restates the row rule.
"""
import numpy as np

import convref as R

K3, S1, PAD = (3, 3, 3), (1, 1, 1), (1, 1, 1)


def scan(dlogits, dbbox, cap, row0):
    """(n, idx, slot, level_first) of the device scan: a row is active if any
    element is != 0.0 (so -0.0 is not and a NaN is); idx ascending, slot[row] =
    compact slot or -1, both cut at cap; level_first[l] = first slot of level l
    (l = 0..nlevels), clamped to cap."""
    dl = np.asarray(dlogits).reshape(len(dlogits), -1)
    db = np.asarray(dbbox).reshape(len(dbbox), -1)
    act = (dl != 0.0).any(axis=1) | (db != 0.0).any(axis=1)
    rows = np.nonzero(act)[0]
    n = len(rows)
    idx = rows[:cap]
    slot = np.full(len(act), -1, np.int64)
    slot[idx] = np.arange(len(idx))
    before = np.concatenate([[0], np.cumsum(act)])              # active rows before row r
    first = [min(int(before[r]), cap) for r in row0]
    return n, idx, slot, first


def head_backward(dlogits, dbbox, s1, s2, P, w1, w2, w24, dP0=None):
    """dlogits [R][2 apl], dbbox [R][6 apl]; s1 / s2 / P: per-level lists
    ([H][W][D][C]); w1 [3][3][3][C0][C1], w2 [C1][C2], w24 [C2][8 apl].
    dP0: per-level values dP accumulates onto (None: zero).
    Returns dict(dP=[...], dw1, db1, dw2, db2, dw24, db24) in float64."""
    f = lambda a: np.asarray(a, np.float64)      # noqa: E731
    dz3 = np.concatenate([f(dlogits), f(dbbox)], axis=1)
    w1, w2, w24 = f(w1), f(w2), f(w24)
    a1 = np.concatenate([f(a).reshape(-1, a.shape[-1]) for a in s1])
    a2 = np.concatenate([f(a).reshape(-1, a.shape[-1]) for a in s2])
    out = {"db24": dz3.sum(0), "dw24": a2.T @ dz3}
    dz2 = (dz3 @ w24.T) * (a2 > 0)
    out["db2"], out["dw2"] = dz2.sum(0), a1.T @ dz2
    dz1 = (dz2 @ w2.T) * (a1 > 0)
    out["db1"] = dz1.sum(0)
    dw1 = np.zeros(w1.shape)
    dP, off = [], 0
    for l, p in enumerate(P):
        H, W, D, _ = p.shape
        d = dz1[off:off + H * W * D].reshape(1, H, W, D, -1)
        off += H * W * D
        dw1 = R.conv_bwd_weight(f(p)[None], d, K3, S1, PAD, (H, W, D), dw1)
        g = R.conv_bwd_data(d, w1, (1, H, W, D, p.shape[-1]), K3, S1, PAD, (H, W, D))[0]
        dP.append(g + (f(dP0[l]) if dP0 is not None else 0.0))
    out["dw1"], out["dP"] = dw1, dP
    return out

