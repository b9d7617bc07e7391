"""The reference's on-disk dataset format, read without scikit-image / pickle.

Mirrors ``utils.Dataset`` (core/utils.py:694-800) and ``ToyDataset``
(core/data_generators.py:1559-1716):

* ``<data_dir>/datasets/{train,test}.csv`` with (case-insensitive, substring
  matched) columns images / segs (optional) / cabs / masks holding file paths;
* images: Z-first TIFF stacks -> ``(Y, X, Z)``; clipped to the [1, 99]
  percentiles, z-scored, ``tanh(0.5 x)``; returned ``[H, W, D, 1]`` float32
  (core/data_generators.py:1603-1630);
* ``cabs`` (.dat): whitespace rows ``class z1 y1 x1 z2 y2 x2`` (exclusive
  ends), remapped to ``(y1, x1, z1, y2, x2, z2)`` and validated as the loader
  does (core/data_generators.py:1648-1668);
* masks: bz2-compressed pickles of a ``(Z, Y, X, N)`` array, transposed to
  ``(Y, X, Z, N)`` float32 (1679-1708).  The pickle is read with an
  allow-list unpickler that only reconstructs numpy arrays, so a data file
  cannot execute code.

The loaded volumes feed ``m3d.targets.build_rpn_targets`` /
``DetectionTargetLayer`` and the models as ``[1, H, W, D, 1]`` tensors.
"""
from __future__ import annotations

import bz2
import io
import os
import pickle

import numpy as np

from .tiff import imread


class _NumpyOnlyUnpickler(pickle.Unpickler):
    _ALLOWED = {
        ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
        ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"),
        ("numpy._core.multiarray", "scalar"), ("_codecs", "encode"),
    }

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refusing to load {module}.{name} from a mask file")


def load_mask_pickle(path) -> np.ndarray:
    """The bz2-pickled (Z, Y, X, N) mask array (numpy objects only)."""
    with bz2.BZ2File(path, "rb") as f:
        data = f.read()
    return np.asarray(_NumpyOnlyUnpickler(io.BytesIO(data), encoding="latin1").load())


def normalize_image(image_zyx: np.ndarray) -> np.ndarray:
    """ToyDataset.load_image normalisation: (Z,Y,X) -> [H,W,D,1] float32."""
    image = np.transpose(image_zyx, (1, 2, 0)).astype(np.float32)
    p1, p99 = np.percentile(image, [1, 99])
    image = np.clip(image, p1, p99)
    mean_val, std_val = np.mean(image), np.std(image)
    image = (image - mean_val) / std_val if std_val > 0 else image - mean_val
    image = np.tanh(image * 0.5)
    return image[..., np.newaxis].astype(np.float32, copy=False)


class Dataset:
    """utils.Dataset: class / image registries and id maps."""

    def __init__(self, class_map=None):
        self._image_ids = []
        self.image_info = []
        self.class_info = [{"source": "", "id": 0, "name": "BG"}]
        self.source_class_ids = {}

    def add_class(self, source, class_id, class_name):
        assert "." not in source, "Source name cannot contain a dot"
        for info in self.class_info:
            if info["source"] == source and info["id"] == class_id:
                return
        self.class_info.append({"source": source, "id": class_id, "name": class_name})

    def add_image(self, source, image_id, path, **kwargs):
        info = {"id": image_id, "source": source, "path": path}
        info.update(kwargs)
        self.image_info.append(info)

    def prepare(self, class_map=None):
        def clean_name(name):
            return ",".join(name.split(",")[:1])

        self.num_classes = len(self.class_info)
        self.class_ids = np.arange(self.num_classes)
        self.class_names = [clean_name(c["name"]) for c in self.class_info]
        self.num_images = len(self.image_info)
        self._image_ids = np.arange(self.num_images)
        self.class_from_source_map = {f"{i['source']}.{i['id']}": c for i, c in zip(self.class_info, self.class_ids)}
        self.image_from_source_map = {f"{i['source']}.{i['id']}": c for i, c in zip(self.image_info, self.image_ids)}
        self.sources = list({i["source"] for i in self.class_info})
        self.source_class_ids = {s: [i for i, info in enumerate(self.class_info) if i == 0 or s == info["source"]]
                                 for s in self.sources}

    def map_source_class_id(self, source_class_id):
        return self.class_from_source_map[source_class_id]

    def get_source_class_id(self, class_id, source):
        info = self.class_info[class_id]
        assert info["source"] == source
        return info["id"]

    @property
    def image_ids(self):
        return self._image_ids

    def source_image_link(self, image_id):
        return self.image_info[image_id]["path"]


class ToyDataset(Dataset):
    """core/data_generators.py:1559-1716."""

    def load_dataset(self, data_dir, is_train=True):
        import pandas as pd
        self.add_class("dataset", 1, "neuron")
        split = "train" if is_train else "test"
        td = pd.read_csv(os.path.join(data_dir, "datasets", f"{split}.csv"), sep=None, engine="python")
        cols = {c.lower(): c for c in td.columns}

        def pick(*cands, required=True):
            for c in cands:
                k = c.lower()
                if k in cols:
                    return cols[k]
                for lc, orig in cols.items():
                    if k in lc:
                        return orig
            if required:
                raise KeyError(f"[Dataset.load_dataset] none of columns {cands} found. "
                               f"Available: {list(td.columns)}")
            return None

        col_images = pick("images", "image", "img", "path", "image_path")
        col_segs = pick("segs", "seg", "seg_path", "labels", "label_path", required=False)
        col_cabs = pick("cabs", "cab", "boxes", "cab_path")
        col_masks = pick("masks", "mask", "masks_path", "mask_path")
        for i in range(len(td)):
            img, cab, msk = td.at[i, col_images], td.at[i, col_cabs], td.at[i, col_masks]
            seg = td.at[i, col_segs] if col_segs is not None else None
            for nm, v in (("images", img), ("cabs", cab), ("masks", msk)):
                if not isinstance(v, str):
                    raise ValueError(f"[load_dataset] bad '{nm}' at row {i}")
            self.add_image("dataset", image_id=i, path=img, seg_path=seg, cab_path=cab, m_path=msk)

    def load_image(self, image_id, z_slice=None, device=None, repeat=1):
        """The normalised [H,W,D,1] float32 volume.  ``device=None``: numpy, on
        the host.  With a device the raw stack is uploaded in its file dtype (1
        or 2 bytes per voxel for 8- / 16-bit TIFFs) and normalised there
        (m3d.preprocess.normalize_image; ``repeat=2`` is the reference's
        evaluation input); returns a device tensor."""
        raw = imread(self.image_info[image_id]["path"])
        if device is None:
            return normalize_image(raw)
        import torch
        from .preprocess import normalize_image as normalize_on_device
        if raw.dtype not in (np.uint8, np.uint16, np.float32):
            raw = raw.astype(np.float32)
        return normalize_on_device(torch.from_numpy(np.ascontiguousarray(raw)).to(device), repeat=repeat)

    def load_data(self, image_id, masks_needed=True):
        """-> boxes [N,6] int32 (y1,x1,z1,y2,x2,z2) px, class_ids [N] int32,
        masks [H,W,D,N] float32 (or None)."""
        info = self.image_info[image_id]
        cabs = np.loadtxt(info["cab_path"], ndmin=2, dtype=np.int32)
        if cabs.size:
            boxes = cabs[:, [2, 3, 1, 5, 6, 4]]
            class_ids = cabs[:, 0]
            valid = ((boxes[:, 3] > boxes[:, 0]) & (boxes[:, 4] > boxes[:, 1]) & (boxes[:, 5] > boxes[:, 2]) &
                     (boxes[:, 0] >= 0) & (boxes[:, 1] >= 0) & (boxes[:, 2] >= 0))
            boxes, class_ids = boxes[valid], class_ids[valid]
        else:
            boxes = np.zeros((0, 6), np.int32)
            class_ids = np.zeros((0,), np.int32)
        if not masks_needed:
            return boxes, class_ids, None
        if boxes.shape[0] == 0:
            img = imread(info["path"])
            return boxes, class_ids, np.zeros((img.shape[1], img.shape[2], img.shape[0], 0), np.float32)
        try:
            m = load_mask_pickle(info["m_path"])
            masks = np.transpose(m, (1, 2, 0, 3))
            if masks.dtype == np.bool_:
                masks = masks.astype(np.uint8)
            masks = masks.astype(np.float32, copy=False)
            if masks.shape[-1] != boxes.shape[0]:
                k = min(masks.shape[-1], boxes.shape[0])
                if k > 0:
                    masks, boxes, class_ids = masks[..., :k], boxes[:k], class_ids[:k]
                else:
                    masks = np.zeros((*masks.shape[:3], 0), np.float32)
                    boxes = np.zeros((0, 6), np.int32)
                    class_ids = np.zeros((0,), np.int32)
        except (OSError, EOFError, pickle.UnpicklingError, ValueError):
            img = imread(info["path"])
            masks = np.zeros((img.shape[1], img.shape[2], img.shape[0], 0), np.float32)
        return boxes, class_ids, masks


class ToyHeadDataset(Dataset):
    """The head dataset TARGET_GENERATION leaves (core/data_generators.py:
    1720-2023; written by m3d.headstore / MaskRCNN.head_target_generation):
    ``<data_dir>/datasets/{train,test}.csv`` with the columns rois,
    rois_aligned, mask_aligned, target_class_ids, target_bbox, target_mask
    (matched case-insensitively, by the reference's alternative names and by
    substring; the first, second and fourth are required), each cell the path
    of one image's ``.npz`` (or plain ``.npy``) file."""

    def __init__(self, config=None):
        super().__init__()
        self.config = config
        self.num_classes = int(getattr(config, "NUM_CLASSES", 2)) if config is not None else 2

    def load_dataset(self, data_dir, is_train=True):
        import csv
        self.add_class("dataset", 1, "neuron")
        split = "train" if is_train else "test"
        with open(os.path.join(data_dir, "datasets", f"{split}.csv"), newline="") as f:
            sample = f.read(4096)
            f.seek(0)
            try:
                dialect = csv.Sniffer().sniff(sample, delimiters=",;\t")
            except csv.Error:
                dialect = csv.excel
            rows = [r for r in csv.reader(f, dialect) if r]
        if not rows:
            raise ValueError(f"[ToyHeadDataset.load_dataset] {split}.csv is empty")
        header, rows = rows[0], rows[1:]
        cols = {c.strip().lower(): i for i, c in enumerate(header)}

        def pick(*cands, required=True):
            for c in cands:
                k = c.lower()
                if k in cols:
                    return cols[k]
                for lc, i in cols.items():
                    if k in lc:
                        return i
            if required:
                raise KeyError(f"[ToyHeadDataset.load_dataset] none of columns {cands} found. Available: {header}")
            return None

        col = {"rois": pick("rois", "rois_path", "r_path"),
               "ra_path": pick("rois_aligned", "ra_path", "aligned_rois", "roisAligned"),
               "ma_path": pick("mask_aligned", "ma_path", "aligned_mask", required=False),
               "tci_path": pick("target_class_ids", "tci_path", "tci"),
               "tb_path": pick("target_bbox", "tb_path", "bbox", required=False),
               "tm_path": pick("target_mask", "tm_path", "tm", required=False)}
        for i, row in enumerate(rows):
            info = {k: (row[c] if c is not None and c < len(row) and row[c] else None) for k, c in col.items()}
            for k, nm in (("rois", "rois"), ("ra_path", "rois_aligned"), ("tci_path", "target_class_ids")):
                if not info[k]:
                    raise ValueError(f"[ToyHeadDataset] bad '{nm}' at row {i}")
            self.add_image("dataset", image_id=i, path=os.path.basename(info["rois"]), **info)

    def prepare(self, class_map=None):
        super().prepare(class_map)
        self.num_classes = max(self.num_classes, len(self.class_info))

    @staticmethod
    def _load_any(path):
        """An .npz as a dict of its arrays, a plain .npy under "arr_0", None for no file."""
        if path is None:
            return None
        if str(path).endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                return {k: z[k] for k in z.files}
        return {"arr_0": np.load(path, allow_pickle=False)}

    @staticmethod
    def _pick(z, *keys):
        if z is None:
            return None
        for k in keys:
            if k in z:
                return z[k]
        return next(iter(z.values()))

    def filter_by_positive_count(self, min_positive=20):
        """Keep the images with at least ``min_positive`` positive target class
        ids (call after prepare()); returns the (name, count) pairs dropped."""
        keep, skipped = [], []
        for image_id in self.image_ids:
            info = self.image_info[int(image_id)]
            tci = self._pick(self._load_any(info["tci_path"]), "tci", "target_class_ids", "arr_0")
            n = int(np.sum(tci > 0))
            if n >= int(min_positive):
                keep.append(int(image_id))
            else:
                skipped.append((info["path"], n))
        self._image_ids = np.array(keep, dtype=np.int64)
        return skipped

    def _small(self, info):
        rois = self._pick(self._load_any(info["rois"]), "rois", "roi", "arr_0")
        tci = self._pick(self._load_any(info["tci_path"]), "tci", "target_class_ids", "arr_0")
        tb = self._pick(self._load_any(info["tb_path"]), "bbox", "target_bbox", "arr_0")
        rois = np.asarray(rois, np.float32)
        tci = np.asarray(tci, np.int32)
        tb = np.zeros((rois.shape[0], 6), np.float32) if tb is None else np.asarray(tb, np.float32)
        return rois, tci, tb

    def load_data(self, image_id):
        """-> rois [T,6] f32, rois_aligned [T,P,P,P,C] f32, mask_aligned
        [T,M,M,M,C] f32, target_class_ids [T] i32, target_bbox [T,6] f32,
        target_mask [T,m,m,m,1] f32, on the host (core/data_generators.py:
        1873-2023).  A missing mask_aligned / target_bbox / target_mask column is
        zeros of the configuration's shape."""
        info = self.image_info[image_id]
        rois, tci, tb = self._small(info)
        T = rois.shape[0]
        ra = np.asarray(self._pick(self._load_any(info["ra_path"]), "rois_aligned", "ra", "arr_0"), np.float32)

        def unbit(z, bits_key, shape_key, fallback):
            if z is None:
                return None
            if bits_key in z and shape_key in z:
                shape = tuple(int(v) for v in z[shape_key])
                flat = np.unpackbits(z[bits_key])
                need = int(np.prod(shape))
                if flat.shape[0] < need:
                    flat = np.pad(flat, (0, need - flat.shape[0]))
                x = flat[:need].reshape(shape)
            else:
                x = np.asarray(self._pick(z, fallback))
            if x.ndim == 4:
                x = x[..., np.newaxis]
            return x.astype(np.float32) if x.ndim == 5 else None

        ma = unbit(self._load_any(info["ma_path"]), "mask_bits", "mask_shape", "mask_aligned")
        tm = unbit(self._load_any(info["tm_path"]), "tm_bits", "tm_shape", "tm")
        cfg = self.config
        if ma is None:
            M, C = int(getattr(cfg, "MASK_POOL_SIZE", 14)), int(getattr(cfg, "TOP_DOWN_PYRAMID_SIZE", 256))
            ma = np.zeros((T, M, M, M, C), np.float32)
        if tm is None:
            m = int(cfg.MASK_SHAPE[0]) if cfg is not None and hasattr(cfg, "MASK_SHAPE") else 28
            tm = np.zeros((T, m, m, m, 1), np.float32)
        return rois, ra, ma, tci, tb, tm

    def load_packed(self, image_id, device):
        """The stored forms as they are, for m3d.headstore.unpack_gather: a dict
        with ``rois_aligned`` (float16 device tensor [T,P,P,P,C]), ``mask_bits``
        / ``tm_bits`` (packed uint8 device tensors) with their logical
        ``mask_shape`` / ``tm_shape`` (tuples), and ``rois`` / ``target_class_ids``
        / ``target_bbox`` on the host.  Only the .npz layout of
        m3d.headstore is read this way; use load_data for anything else."""
        import torch
        info = self.image_info[image_id]
        rois, tci, tb = self._small(info)
        ra = self._load_any(info["ra_path"])
        ma = self._load_any(info["ma_path"])
        tm = self._load_any(info["tm_path"])
        if (ra is None or "rois_aligned" not in ra or ra["rois_aligned"].dtype != np.float16 or ma is None
                or not {"mask_bits", "mask_shape"} <= set(ma) or tm is None
                or not {"tm_bits", "tm_shape"} <= set(tm)):
            raise ValueError(f"[ToyHeadDataset.load_packed] image {image_id} is not stored as float16 rois_aligned "
                             "and bit-packed mask_aligned / target_mask")

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(device)

        return {"rois": rois, "target_class_ids": tci, "target_bbox": tb,
                "rois_aligned": up(ra["rois_aligned"]),
                "mask_bits": up(ma["mask_bits"]), "mask_shape": tuple(int(v) for v in ma["mask_shape"]),
                "tm_bits": up(tm["tm_bits"]), "tm_shape": tuple(int(v) for v in tm["tm_shape"])}
