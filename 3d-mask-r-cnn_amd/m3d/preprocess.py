"""Image normalisation on the GPU.

``normalize_image(raw)`` is ``ToyDataset.load_image``'s normalisation
(core/data_generators.py:1603-1630: transpose, ``np.percentile`` [1, 99],
clip, mean / std, ``tanh(0.5 x)``) through ``m3d_normalize_image``: the raw
stack stays in its file dtype (1 or 2 bytes per voxel for uint8 / uint16) and
the result is the float64 evaluation of the formula rounded once to float32.
``repeat=2`` is the reference's evaluation input, which normalises the
already normalised image once more (``MrcnnGenerator.get_input_prediction``,
1227-1242).
"""
from __future__ import annotations

import torch

from . import _lib, ops
from ._lib import check, ptr, stream

DTYPE_U8, DTYPE_U16, DTYPE_F32 = 0, 1, 2          # M3D_DTYPE_* (include/m3d.h)
_CODES = {torch.uint8: DTYPE_U8, torch.uint16: DTYPE_U16, torch.float32: DTYPE_F32}


def _normalize(L, raw, transpose):
    a, b, c = (int(v) for v in raw.shape)
    code = _CODES[raw.dtype]
    out = torch.empty((b, c, a) if transpose else (a, b, c), dtype=torch.float32, device=raw.device)
    stats = torch.empty(6, dtype=torch.float64, device=raw.device)
    wsb = int(L.m3d_normalize_image_workspace_bytes(a, b, c, code))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=raw.device)
    check(L.m3d_normalize_image(ptr(raw), code, a, b, c, 1 if transpose else 0, ptr(out), ptr(stats), ptr(ws), wsb,
                                stream()), "normalize_image")
    return out, stats


def normalize_image(raw, repeat=1, transpose=True, return_stats=False):
    """raw: a 3-D DEVICE tensor, (Z,Y,X) in file order (``transpose=True``) or
    already [H,W,D] (``transpose=False``); uint8, uint16 and float32 are read
    as they are, other dtypes are cast to float32 on the device first (the
    reference's ``astype(np.float32)``).  Returns [H,W,D,1] float32 on the
    same device; with ``return_stats`` also the device double[6] of the LAST
    pass (p1, p99, mean, std, non-finite inputs, 0).  A volume with non-finite
    voxels is counted there and its result is unspecified."""
    if not torch.is_tensor(raw):
        raise TypeError("normalize_image takes a device tensor")
    ops._dev(raw)
    if raw.dim() != 3:
        raise ValueError(f"normalize_image takes a 3-D volume, got shape {tuple(raw.shape)}")
    if int(repeat) < 1:
        raise ValueError("repeat must be >= 1")
    L = _lib.load()
    if raw.dtype not in _CODES:
        raw = raw.to(torch.float32)
    out, stats = _normalize(L, raw.contiguous(), transpose)
    for _ in range(int(repeat) - 1):
        out, stats = _normalize(L, out, False)
    out = out.unsqueeze(-1)
    return (out, stats) if return_stats else out
