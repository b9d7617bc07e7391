"""The stored head targets: the files TARGET_GENERATION leaves for HEAD_TRAINING.

``RPN.head_target_generation`` (core/models.py:3530-3796) runs the trained
trunk once per image and stores the sampled ROIs, their ROI-aligned features
and their targets; ``ToyHeadDataset`` / ``HeadGenerator`` (m3d.dataset,
m3d.generator) read them back.  The layout is the reference's ``_save_arrays``
(3604-3636), one ``np.savez_compressed`` file per array and image:

  ============================  =====================================
  ``rois/<name>.npz``             ``rois`` float32 [T,6]
  ``rois_aligned/<name>.npz``     ``rois_aligned`` float16 [T,P,P,P,C]
  ``mask_aligned/<name>.npz``     ``mask_bits`` uint8, ``mask_shape`` int32
  ``target_class_ids/<name>.npz`` ``tci`` int32 [T]
  ``target_bbox/<name>.npz``      ``bbox`` float32 [T,6]
  ``target_mask/<name>.npz``      ``tm_bits`` uint8, ``tm_shape`` int32
  ============================  =====================================

and one row per image in ``<output_dir>/datasets/<split>.csv`` under the
header ``rois,rois_aligned,mask_aligned,target_class_ids,target_bbox,target_mask``.
``*_bits`` is ``np.packbits(x > 0.5)`` of the flattened array, ``*_shape`` its
shape.

The narrowing runs on the device (csrc/headstore.hip): ``save_head_targets``
copies the float16 / packed forms to the host, 34 MB per image at
TRAIN_ROIS_PER_IMAGE = 128 instead of the 405 MB of the float32 features, and
``unpack_gather`` turns the uploaded narrow forms into a float32 batch.
"""
from __future__ import annotations

import csv
import os

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr, stream

COLUMNS = ("rois", "rois_aligned", "mask_aligned", "target_class_ids", "target_bbox", "target_mask")


# --------------------------------------------------------------------------- device passes
def _f32(x):
    if not torch.is_tensor(x):
        raise TypeError("a device tensor is required")
    ops._dev(x)
    return ops._c(x)


def pack_bits(x):
    """np.packbits(x > 0.5) of a float32 device tensor (flattened): uint8 [(n + 7) // 8]."""
    x = _f32(x)
    n = x.numel()
    bits = torch.empty((n + 7) // 8, dtype=torch.uint8, device=x.device)
    check(_lib.load().m3d_pack_bits_f32(ptr(x), n, ptr(bits), stream()), "pack_bits_f32")
    return bits


def to_half(x):
    """x.astype(np.float16) of a float32 device tensor: a float16 tensor of the same shape."""
    x = _f32(x)
    h = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    check(_lib.load().m3d_f32_to_f16(ptr(x), x.numel(), ptr(h), stream()), "f32_to_f16")
    return h


def bits_row_counts(bits, rows, row_bits):
    """Set bits per row of a packed [rows, row_bits] device array: int32 [rows]."""
    ops._dev(bits)
    rows, row_bits = int(rows), int(row_bits)
    if bits.dtype != torch.uint8 or not bits.is_contiguous():
        raise ValueError("bits_row_counts takes a contiguous uint8 tensor")
    if rows < 0 or row_bits <= 0 or bits.numel() < (rows * row_bits + 7) // 8:
        raise ValueError(f"bits_row_counts: {bits.numel()} bytes do not hold {rows} rows of {row_bits} bits")
    counts = torch.empty(rows, dtype=torch.int32, device=bits.device)
    check(_lib.load().m3d_bits_row_counts(ptr(bits), rows, row_bits, ptr(counts), stream()), "bits_row_counts")
    return counts


def index_table(stored, wanted):
    """_resize_spatial's index vector (core/data_generators.py:403-405):
    the identity for equal sizes, else np.linspace(0, S-1, M).astype(np.int64)."""
    stored, wanted = int(stored), int(wanted)
    if stored == wanted:
        return np.arange(stored, dtype=np.int64)
    return np.linspace(0, stored - 1, wanted).astype(np.int64)


def unpack_gather(src, shape, sel, out_spatial=None):
    """out[t,a,b,c,k] = src[sel[t], i0[a], i1[b], i2[c], k] as float32.

    src: a packed uint8 device tensor (bits of the logical array) or a float16
    device tensor; ``shape`` its logical [R,S0,S1,S2,C]; ``sel``: int sequence
    (or int32 device tensor) of rows, -1 for a zero row; ``out_spatial``
    (M0,M1,M2): the resized extent (default: the stored one).  Returns
    [len(sel),M0,M1,M2,C] float32."""
    ops._dev(src)
    R, S0, S1, S2, C = (int(v) for v in shape)
    M = (S0, S1, S2) if out_spatial is None else tuple(int(v) for v in out_spatial)
    dev = src.device
    if torch.is_tensor(sel):
        sel_host = sel.detach().cpu().numpy()
    else:
        sel_host = np.asarray(sel)
    sel_host = np.ascontiguousarray(sel_host.reshape(-1), dtype=np.int64)
    if sel_host.size == 0 or R == 0 or sel_host.max() < 0:          # nothing to read: all padding
        return torch.zeros((sel_host.size,) + M + (C,), dtype=torch.float32, device=dev)
    if sel_host.max() >= R:
        raise ValueError(f"unpack_gather: sel names row {int(sel_host.max())} of {R}")
    n = R * S0 * S1 * S2 * C
    if not src.is_contiguous():
        raise ValueError("unpack_gather takes a contiguous source")
    if src.dtype == torch.uint8:
        if src.numel() < (n + 7) // 8:
            raise ValueError(f"unpack_gather: {src.numel()} bytes do not hold {n} bits")
        fn = _lib.load().m3d_unpack_gather_bits
    elif src.dtype == torch.float16:
        if src.numel() != n:
            raise ValueError(f"unpack_gather: {src.numel()} halves, the shape says {n}")
        fn = _lib.load().m3d_unpack_gather_f16
    else:
        raise ValueError(f"unpack_gather takes packed uint8 or float16, got {src.dtype}")
    tables = np.concatenate([index_table(s, m) for s, m in zip((S0, S1, S2), M)]).astype(np.int32)
    host = torch.from_numpy(np.concatenate([sel_host.astype(np.int32), tables]))
    d = host.to(dev)
    T = sel_host.size
    out = torch.empty((T,) + M + (C,), dtype=torch.float32, device=dev)
    at = [d.data_ptr() + 4 * o for o in (0, T, T + M[0], T + M[0] + M[1])]
    check(fn(ptr(src), R, S0, S1, S2, C, at[0], T, at[1], at[2], at[3], M[0], M[1], M[2], ptr(out), stream()),
          "unpack_gather")
    return out


# --------------------------------------------------------------------------- the files
def save_head_target_arrays(output_dir, name, rois, rois_aligned, mask_bits, mask_shape, target_class_ids,
                            target_bbox, tm_bits, tm_shape):
    """Write one image's six files from host arrays already in their stored
    forms (``_save_arrays`` with use_npz, core/models.py:3604-3636) and return
    their paths in COLUMNS order."""
    arrays = (
        {"rois": np.asarray(rois).astype(np.float32, copy=False)},
        {"rois_aligned": np.asarray(rois_aligned).astype(np.float16, copy=False)},
        {"mask_bits": np.asarray(mask_bits, np.uint8), "mask_shape": np.asarray(mask_shape, np.int32)},
        {"tci": np.asarray(target_class_ids).astype(np.int32, copy=False)},
        {"bbox": np.asarray(target_bbox).astype(np.float32, copy=False)},
        {"tm_bits": np.asarray(tm_bits, np.uint8), "tm_shape": np.asarray(tm_shape, np.int32)},
    )
    paths = []
    for col, arrs in zip(COLUMNS, arrays):
        os.makedirs(os.path.join(output_dir, col), exist_ok=True)
        path = os.path.join(output_dir, col, f"{name}.npz")
        np.savez_compressed(path, **arrs)
        paths.append(path)
    return tuple(paths)


def save_head_targets(output_dir, name, rois, rois_aligned, mask_aligned, target_class_ids, target_bbox, target_mask):
    """One image's device tensors (batch axis stripped) to the six files:
    rois_aligned is narrowed to float16 and the two masks are bit-packed on the
    device; only those forms and the three small arrays cross to the host.
    Returns the paths in COLUMNS order."""
    ops._dev(rois, rois_aligned, mask_aligned, target_class_ids, target_bbox, target_mask)
    half = to_half(rois_aligned)
    mbits = pack_bits(mask_aligned)
    tbits = pack_bits(target_mask)
    return save_head_target_arrays(
        output_dir, name, rois.detach().cpu().numpy(), half.cpu().numpy(), mbits.cpu().numpy(),
        tuple(mask_aligned.shape), target_class_ids.cpu().numpy(), target_bbox.detach().cpu().numpy(),
        tbits.cpu().numpy(), tuple(target_mask.shape))


def write_csv_header(output_dir, split):
    """Start ``<output_dir>/datasets/<split>.csv`` with the header row; returns its path."""
    os.makedirs(os.path.join(output_dir, "datasets"), exist_ok=True)
    path = os.path.join(output_dir, "datasets", f"{split}.csv")
    with open(path, "w", newline="") as f:
        csv.writer(f).writerow(COLUMNS)
    return path


def append_csv_row(csv_path, paths):
    with open(csv_path, "a", newline="") as f:
        csv.writer(f).writerow(paths)
