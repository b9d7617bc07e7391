"""The launch plan of the conv unit, pinned.

Every launch of the package goes through ``check(rc, "label")``.  For a set of
scenarios (the RPN training step under the routing switches, a no-grad forward,
one MaskRCNN.train_heads step and two single-layer calls) this test records the
ordered label list of every step plus nn.LAYER_LOG's roofline records, and
asserts both equal to tests/golden/launch_plan.json, which
scripts/record_launch_plan.py wrote from this same code.  A host-side
restructuring of m3d/nn.py or m3d/heads.py that moves, drops or reorders a
launch (or labels a log record with another engine than the one that ran)
fails here; a change that reroutes on purpose re-records the golden
("Where the routing lives").

The union of the recorded labels must hold every label the conv unit
(_ConvBNAct and its launch functions) and _RPNOut pass to ``check``, except the
depth-slab forms, which need more than one GPU (tests/test_gpu_slab_halo.py,
tests/test_slab.py)."""
import contextlib
import gc
import importlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan.json")

# every label literal of the conv unit and of _RPNOut
CONV_UNIT_LABELS = {
    "bn_affine", "conv3d_fwd_halo", "conv3d_fwd_wino_halo_phase1", "conv3d_fwd_wino_halo_phase2",
    "conv3d_fwd_wino_halo", "conv3d_fwd_wino_kv", "conv3d_fwd_wino_keep", "conv3d_fwd_wino", "conv3d_fwd_x3",
    "conv3d_fwd_splitk", "conv3d_fwd", "conv3d_bwd_weight_halo", "conv3d_bwd_weight",
    "conv3d_bwd_weight_wino_halo", "conv3d_bwd_weight_wino_u", "conv3d_bwd_weight_wino",
    "conv3d_bwd_data_wino_halo", "conv3d_bwd_data_wino_xv(bn)", "conv3d_bwd_data_wino_bn",
    "conv3d_bwd_data_wino_xv", "conv3d_bwd_data_wino", "subsample221", "conv3d_bwd_data_x3_bna",
    "conv3d_bwd_data_x3", "conv3d_bwd_data_splitk_bn", "conv3d_bwd_data_splitk", "conv3d_bwd_data_bn",
    "conv3d_bwd_data", "upsample221_bwd", "rpn_out_fwd", "rpn_out_wgrad", "rpn_out_dgrad_bn", "rpn_out_dgrad",
}
# the depth-slab forms: more than one GPU
SLAB_LABELS = {
    "conv3d_fwd_halo", "conv3d_fwd_wino_halo", "conv3d_fwd_wino_halo_phase1", "conv3d_fwd_wino_halo_phase2",
    "conv3d_bwd_weight_halo", "conv3d_bwd_weight_wino_halo", "conv3d_bwd_data_wino_halo",
}

# scenario -> the m3d.nn flags it sets
RPN_SCENARIOS = {
    "defaults": {},
    "bn_fuse_off": {"BN_FUSE": False},
    "x3_bn_fuse_off": {"X3_BN_FUSE": False},
    "winograd_off": {"WINOGRAD": False},
    "wino_v_prepass": {"WINO_V_PREPASS_MIN_VOXELS": 0},
    "wino_keep_none": {"WINO_KEEP_MAX_BYTES": 0},
    "conv1_x3_splitk_off": {"CONV1_X3": False, "SPLITK": False},
    "conv1_x3_small_tiles": {"CONV1_X3_FWD_TILES": 1, "CONV1_X3_DGRAD_TILES": 1, "CONV1_X3_DGRAD_MIN_K": 32,
                             "CONV1_X3_DGRAD_FUSED_MIN_K": 32},
    "wgrad_inline_first": {"WGRAD_STREAM": False, "WGRAD_LAST": False},
}
SCENARIOS = list(RPN_SCENARIOS) + ["no_grad_forward", "train_heads", "layer_wino_direct_wgrad", "layer_splitk"]


class Recorder:
    """Replaces ``check`` in m3d._lib and in every loaded m3d.* module that
    imported it by name with a wrapper that appends the label, then delegates."""

    def __init__(self):
        self.steps = [[]]

    def next_step(self):
        self.steps.append([])

    @contextlib.contextmanager
    def recording(self):
        import m3d
        from m3d import _lib
        # a module first imported while recording would keep this wrapper for good
        for f in sorted(os.listdir(os.path.dirname(m3d.__file__))):
            if f.endswith(".py") and f != "__init__.py":
                importlib.import_module("m3d." + f[:-3])
        orig = _lib.check

        def check(rc, what=""):
            self.steps[-1].append(what)
            return orig(rc, what)
        mods = [m for n, m in list(sys.modules.items())
                if (n == "m3d" or n.startswith("m3d.")) and m is not None and getattr(m, "check", None) is orig]
        for m in mods:
            m.check = check
        try:
            yield self
        finally:
            for m in mods:
                m.check = orig


def _rpn_steps(dev, rec, grad=True, after=None):
    """Two steps of a fresh RPN at the 64 x 64 x 16 synthetic config of
    tests/test_gpu_bnfuse.py::_step: the first registers kernels and transforms
    inline, the second takes the refreshed planes and pre-pass buffers.
    ``after(step, model, result)`` runs after each step (scripts/step_digest.py)."""
    from m3d.config import synthetic_rpn_config
    from m3d.model import RPN, RPNTargets, synthetic_rpn_targets, synthetic_volume
    cfg = synthetic_rpn_config(64, depth=16, PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=200)
    image = synthetic_volume(64, 16, seed=3).to(dev)
    model = RPN(cfg, device=dev, seed=7)
    match, bbox = synthetic_rpn_targets(model.anchors.shape[1], 256, seed=2)
    targets = RPNTargets(match, bbox, dev)
    for step in range(2):
        if step:
            rec.next_step()
        if grad:
            r = model.forward_backward(image, targets, proposals=False)
        else:
            with torch.no_grad():
                r = model.forward(image, proposals=False)
        if after is not None:
            after(step, model, r)


def _train_heads_steps(dev, rec, steps=1, after=None):
    """MaskRCNN.train_heads steps on both heads (the volume and config of
    tests/test_gpu_head_train.py::test_train_classifier_head_model_entry)."""
    import numpy as np
    from m3d.config import synthetic_mrcnn_config
    from m3d.heads import MaskRCNN
    from m3d.model import compose_image_meta, synthetic_volume
    from m3d.optim import KerasOptimizer
    cfg = synthetic_mrcnn_config(64, depth=8, PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=300,
                                 POST_NMS_ROIS_INFERENCE=64, TRAIN_ROIS_PER_IMAGE=12, ROI_POSITIVE_RATIO=0.5,
                                 RPN_POSITIVE_IOU=0.1, RPN_NEGATIVE_IOU=0.05, USE_MINI_MASK=False,
                                 MASK_SHAPE=[28, 28, 28], DETECTION_MAX_INSTANCES=8)
    meta = torch.from_numpy(compose_image_meta(0, [64, 64, 8, 1], [64, 64, 8, 1], [0, 0, 0, 64, 64, 8], 1.0,
                                               [1, 1])[None]).to(dev)
    boxes = np.array([[4, 4, 0, 32, 36, 8], [30, 8, 0, 60, 34, 8], [12, 36, 0, 40, 62, 8]], np.float32)
    masks = np.zeros((64, 64, 8, 3), bool)
    for g, (y1, x1, z1, y2, x2, z2) in enumerate(boxes.astype(int)):
        masks[y1:y2, x1:x2, z1:z2, g] = True
    model = MaskRCNN(cfg, device=dev, seed=2)
    args = (synthetic_volume(64, 8).to(dev), meta, torch.ones((1, 3), dtype=torch.int32, device=dev),
            torch.from_numpy(boxes[None]).to(dev), torch.from_numpy(masks[None]).to(dev))
    optimizer = KerasOptimizer({"name": "SGD", "parameters": {"learning_rate": 0.01, "momentum": 0.9}})
    for step in range(steps):
        if step:
            rec.next_step()
        r = model.train_heads(*args, optimizer, seed=5)
        if after is not None:
            after(step, model, r)


class _P:
    def __init__(self, data):
        self.data, self.grad = data, torch.zeros_like(data)


class _Layer:
    """Stand-in of params.ConvLayer over explicit tensors (no ParamStore: a BN
    of it has no batched affine, so the unit runs its own m3d_bn_affine)."""

    def __init__(self, k, cin, cout, dev, g):
        self.kernel = _P((torch.randn((k, k, k, cin, cout), generator=g) * 0.05).to(dev))
        self.bias = _P((torch.randn(cout, generator=g) * 0.1).to(dev))
        self.k = (k, k, k)
        self.name = f"layer{k}_{cin}_{cout}"

    def grad_dict(self, bn=None):
        g = {"kernel": self.kernel.grad, "bias": self.bias.grad}
        if bn is not None:
            g["gamma"], g["beta"] = bn.gamma.grad, bn.beta.grad
        return g


class _BN:
    def __init__(self, c, dev, g):
        self.gamma, self.beta = _P((torch.rand(c, generator=g) + 0.5).to(dev)), _P(torch.randn(c, generator=g).to(dev))
        self.moving_mean = torch.randn(c, generator=g).to(dev)
        self.moving_variance = (torch.rand(c, generator=g) + 0.5).to(dev)
        self.eps = 1e-3


def _layer_step(dev, k, cin, cout, sp):
    """conv_bn_act of one BN-ReLU layer, forward and backward."""
    from m3d import nn as mnn
    g = torch.Generator().manual_seed(5)
    layer, bn = _Layer(k, cin, cout, dev, g), _BN(cout, dev, g)
    x = torch.randn((1, *sp, cin), generator=g).to(dev).requires_grad_(True)
    geo = mnn.conv_geom(sp, (k, k, k), (1, 1, 1), "same")
    y = mnn.conv_bn_act(x, layer, geo, True, bn=bn)
    y.backward(torch.randn(y.shape, generator=g).to(dev))
    mnn.join_wgrad()


def record(name, dev):
    """Run scenario ``name``: {"steps": [[label, ...] per step], "log": [[kind,
    direct_flops, executed_flops, bytes, phase, name, engine], ...]}."""
    from m3d import nn as mnn
    flags = dict(RPN_SCENARIOS.get(name, {}))
    if name == "layer_wino_direct_wgrad":
        flags["WINO_MIN_C"] = 32      # a 32-channel Winograd conv: its weight gradient stays direct
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if mnn.FORK_EVENT != "torch":
        # the fork events' ring is created by the process's first fork: not part of any plan
        mnn.fork_event(idx, int(mnn.FORK_EVENT))
    mp = pytest.MonkeyPatch()
    rec = Recorder()
    log = []
    gc.collect()                      # the previous scenario's model
    try:
        # the per-forward registries start empty, whatever ran before in this process
        mp.setattr(mnn, "X3_PLANES", mnn.X3Planes())
        mp.setattr(mnn, "WINO_V", mnn.WinoVPrep())
        for k, v in flags.items():
            mp.setattr(mnn, k, v)
        mp.setattr(mnn, "LAYER_TIMING", False)
        mp.setattr(mnn, "LAYER_LOG", log)
        with rec.recording():
            if name in RPN_SCENARIOS:
                _rpn_steps(dev, rec)
            elif name == "no_grad_forward":
                _rpn_steps(dev, rec, grad=False)
            elif name == "train_heads":
                _train_heads_steps(dev, rec)
            elif name == "layer_wino_direct_wgrad":
                _layer_step(dev, 3, 32, 32, (6, 6, 8))
            elif name == "layer_splitk":
                _layer_step(dev, 1, 1024, 256, (4, 4, 8))
            else:
                raise KeyError(name)
        torch.cuda.synchronize()
    finally:
        mp.undo()
    return {"steps": [list(s) for s in rec.steps], "log": [[r[0], r[1], r[2], r[3], r[4], r[5], r[8]] for r in log]}


def encode(results):
    """The golden's form: each distinct label / log record once, the scenarios as index lists."""
    labels, records = [], []
    li, ri = {}, {}
    out = {}
    for name in SCENARIOS:
        r = results[name]
        steps = [[li.setdefault(s, len(li)) for s in step] for step in r["steps"]]
        logi = [ri.setdefault(json.dumps(x), len(ri)) for x in r["log"]]
        out[name] = {"steps": steps, "log": logi}
    labels = sorted(li, key=li.get)
    records = [json.loads(s) for s in sorted(ri, key=ri.get)]
    return {"labels": labels, "records": records, "scenarios": out}


def decode(gold):
    return {name: {"steps": [[gold["labels"][i] for i in step] for step in s["steps"]],
                   "log": [gold["records"][i] for i in s["log"]]}
            for name, s in gold["scenarios"].items()}


def dump(results, path):
    with open(path, "w") as f:
        json.dump(encode(results), f, separators=(",", ":"))
        f.write("\n")


_RESULTS = {}


def _result(name, dev):
    if name not in _RESULTS:
        _RESULTS[name] = record(name, dev)
    return _RESULTS[name]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return decode(json.load(f))


def _first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"first difference at {i}: {x!r} != {y!r} (after {a[max(0, i - 3):i]})"
    return f"lengths {len(a)} != {len(b)}"


@pytest.mark.parametrize("name", SCENARIOS)
def test_launch_plan(cuda, golden, name):
    got, want = _result(name, cuda), golden[name]
    assert len(got["steps"]) == len(want["steps"])
    for i, (a, b) in enumerate(zip(got["steps"], want["steps"])):
        assert a == b, f"{name} step {i}: " + _first_diff(a, b)
    glog = json.loads(json.dumps(got["log"]))
    assert glog == want["log"], f"{name} log: " + _first_diff(glog, want["log"])


def test_every_conv_unit_label_is_reached(cuda):
    seen = set()
    for name in SCENARIOS:
        for step in _result(name, cuda)["steps"]:
            seen.update(step)
    assert SLAB_LABELS <= CONV_UNIT_LABELS
    missing = CONV_UNIT_LABELS - SLAB_LABELS - seen
    assert not missing, sorted(missing)
