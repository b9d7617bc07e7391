"""The classifier head's training mode on the GPU (m3d.heads.ClassifierHead(
training=True), KerasOptimizer.step(chunks=...), optim.apply_max_norm,
MaskRCNN.train_classifier_head) against the float64 CPU evaluation of
tests/headtrain_ref.py (pinned by tests/test_headtrain_ref.py).

Cases (pool, C, fc, num_classes, B, N):
  small2 (3, 8, 32, 2, 2, 12) and small5 (3, 8, 32, 5, 2, 12): M = 24 ROIs, three
         of them all-zero rows (zero-padded ROIs count in the batch statistics);
         the logits kernel is scaled so that at least two rows have raw logits
         beyond +-10 (clip mask) while others stay inside.
  deep   (7, 256, 64, 2, 1, 8): K = 87808, the real conv1 depth: the split-K
         forward and both conv1 gradient GEMMs at their real reduction size.
The upstream gradients come from m3d.head_losses.mrcnn_losses (class + bbox).
Seeds are fixed below so that no float64 BN pre-activation lies within
1e-4 * rms of 0 and no raw logit within 1e-3 of +-10 (asserted on the checker's
values, in the five-step runs at every step): the float32 kernels and the
checker then take the same branches.

Bars.  Forward outputs: the project's 1e-4 of the output scale
(tests/test_gpu_heads.py).  Everything else: 10x the worst error of the
restatement evaluated in float32 on the CPU against float64 over these cases
(scripts/measure_headtrain_f32.py prints them); tensors relative to the
reference tensor's largest entry, losses relative to max(1, |ref|).  The conv1 /
conv2 bias gradients are true cancellations to about 0 under batch statistics:
their error is taken per column relative to that column's sum |dz|.

  quantity                      float32 CPU   bar       MI355X (measured)
  loss (one step)               3.14e-07      3.14e-06  8.5e-08
  parameter gradients           1.56e-06      1.56e-05  2.8e-06
  conv bias gradients           2.98e-07      2.98e-06  3.7e-07
  d_pooled                      2.36e-06      2.36e-05  1.3e-06
  five steps SGD:  losses       1.19e-07      1.19e-06  9.7e-08
                   parameters   7.80e-07      7.80e-06  6.0e-07
                   moving stats 1.06e-06      1.06e-05  7.1e-07
                   column norms 2.01e-07      2.01e-06  2.3e-07
  five steps Adam: losses       1.19e-07      1.19e-06  3.3e-07
                   parameters   2.72e-05      2.72e-04  8.0e-05
                   moving stats 2.24e-06      2.24e-05  5.9e-06
                   column norms 1.47e-07      1.47e-06  2.7e-07
(Adam divides by sqrt(v): parameters whose gradient is small move by the
rounding of that gradient, hence its larger float32 figure.)
"""
import functools
import math

import numpy as np
import pytest
import torch

import headtrain_ref as HT

pytestmark = pytest.mark.gpu

CASES = {"small2": (3, 8, 32, 2, 2, 12, 0), "small5": (3, 8, 32, 5, 2, 12, 1), "deep": (7, 256, 64, 2, 1, 8, 2)}
# worst float32-vs-float64 error of the restatement on the CPU (scripts/measure_headtrain_f32.py)
F32 = {"loss": 3.14e-07, "grad": 1.56e-06, "bias": 2.98e-07, "d_pooled": 2.36e-06}
F32_STEPS = {"sgd": {"s_loss": 1.19e-07, "s_param": 7.80e-07, "s_moving": 1.06e-06, "s_norm": 2.01e-07},
             "adam": {"s_loss": 1.19e-07, "s_param": 2.72e-05, "s_moving": 2.24e-06, "s_norm": 1.47e-07}}
BARS = {k: 10.0 * v for k, v in F32.items()}
BARS_STEPS = {o: {k: 10.0 * v for k, v in d.items()} for o, d in F32_STEPS.items()}
FWD_BAR = 1e-4
CONV_BIASES = ("mrcnn_class_conv1/bias:0", "mrcnn_class_conv2/bias:0")
STEPS = 5
STEPS_SEED = 8          # every step's smallest |pre-activation| / rms >= 2.6e-4 for both optimizers
OPTIMIZERS = {"sgd": ({"name": "SGD", "parameters": {"learning_rate": 0.05, "momentum": 0.9}},
                      ("SGD", 0.05, 0.9)),
              "adam": ({"name": "ADAM", "parameters": {"learning_rate": 0.01}},
                       ("ADAM", 0.01, 0.9, 0.999, 1e-7))}
WEIGHT_DECAY = 0.5


@functools.lru_cache(maxsize=None)
def case(name, bbox_scale=1.0, reseed=0):
    """float32 host parameters / inputs / targets of one case (torch, CPU)."""
    pool, C, fc, nc, B, N, seed = CASES[name]
    g = torch.Generator().manual_seed(100 + seed + 1000 * reseed)
    K = pool ** 3 * C

    def rn(*s, scale=1.0):
        return torch.randn(*s, generator=g) * scale
    p = {"mrcnn_class_conv1/kernel:0": rn(pool, pool, pool, C, fc, scale=1 / math.sqrt(K)),
         "mrcnn_class_conv1/bias:0": rn(fc, scale=0.1),
         "mrcnn_class_bn1/gamma:0": rn(fc, scale=0.2) + 1.0, "mrcnn_class_bn1/beta:0": rn(fc, scale=0.3),
         "mrcnn_class_conv2/kernel:0": rn(1, 1, 1, fc, fc, scale=1 / math.sqrt(fc)),
         "mrcnn_class_conv2/bias:0": rn(fc, scale=0.1),
         "mrcnn_class_bn2/gamma:0": rn(fc, scale=0.2) + 1.0, "mrcnn_class_bn2/beta:0": rn(fc, scale=0.3),
         # raw logits ~ N(0, ~6): some rows beyond +-10
         "mrcnn_class_logits/kernel:0": rn(fc, nc, scale=1.4), "mrcnn_class_logits/bias:0": rn(nc, scale=0.1),
         "mrcnn_bbox_fc/kernel:0": rn(fc, 6 * nc, scale=0.1 * bbox_scale),
         "mrcnn_bbox_fc/bias:0": rn(6 * nc, scale=0.1)}
    pooled = rn(B, N, pool, pool, pool, C)
    if N >= 12:
        pooled[0, N - 2:] = 0.0             # zero-padded ROIs
        pooled[1, N - 1] = 0.0
    ids = torch.randint(0, nc, (B, N), generator=g, dtype=torch.int32)
    ids[:, 0] = 1                           # at least one positive per image
    ids[:, 1] = 0
    tbox = rn(B, N, 6)
    active = torch.ones(B, nc)
    moving = {f"bn{i}": (rn(fc, scale=0.2), torch.rand(fc, generator=g) + 0.5) for i in (1, 2)}
    return dict(p=p, pooled=pooled, ids=ids, tbox=tbox, active=active, moving=moving, nc=nc, fc=fc)


def to64(c, dtype=torch.float64):
    f = lambda t: t.to(dtype)                                                   # noqa: E731
    return dict(p={k: f(v) for k, v in c["p"].items()}, pooled=f(c["pooled"]), ids=c["ids"].long(),
                tbox=f(c["tbox"]), active=f(c["active"]),
                moving={k: (f(a), f(b)) for k, (a, b) in c["moving"].items()}, nc=c["nc"], fc=c["fc"])


@functools.lru_cache(maxsize=None)
def reference(name):
    c = to64(case(name))
    total, lc, lb, grads, d_pooled, outs, aux = HT.loss_and_grads(c["p"], c["pooled"], c["ids"], c["tbox"],
                                                                  c["active"], c["nc"])
    return dict(total=total, lc=lc, lb=lb, grads=grads, d_pooled=d_pooled, outs=outs, aux=aux)


def margins(aux):
    """(smallest |BN pre-activation| / rms, smallest distance of a raw logit to +-10)."""
    m = min(float(aux[f"pre{i}"].detach().abs().min() / aux[f"pre{i}"].detach().pow(2).mean().sqrt()) for i in (1, 2))
    return m, float((aux["raw_logits"].detach().abs() - 10.0).abs().min())


def build(cuda, c, extra=False, weight_decay=0.0):
    """A ParamStore with the head (and, with ``extra``, a layer before and after
    it) holding the case's parameters."""
    from m3d.heads import ClassifierHead
    from m3d.params import BNLayer, ConvLayer, ParamStore
    pool, C = c["p"]["mrcnn_class_conv1/kernel:0"].shape[0], c["p"]["mrcnn_class_conv1/kernel:0"].shape[3]
    store = ParamStore()
    if extra:
        ConvLayer(store, "before", (1, 1, 1), 8, 8)
        BNLayer(store, "bn_before", 8)
    head = ClassifierHead(store, pool, c["nc"], c["fc"], C)
    if extra:
        ConvLayer(store, "after", (1, 1, 1), 8, 8)
    store.finalize(cuda, seed=3, weight_decay=weight_decay)
    with torch.no_grad():
        for k, v in c["p"].items():
            store.by_name[k].data.copy_(v)
        for i, bn in ((1, head.bn1), (2, head.bn2)):
            bn.moving_mean.copy_(c["moving"][f"bn{i}"][0])
            bn.moving_variance.copy_(c["moving"][f"bn{i}"][1])
    return store, head


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    return float((got - ref).abs().max()) / float(ref.abs().max())


def grad_errors(grads, ref):
    """(worst relative error of the ten non-cancelling gradients, worst conv
    bias gradient error relative to its column's sum |dz|)."""
    worst = max(rel(grads[k], ref["grads"][k]) for k in HT.PARAM_NAMES if k not in CONV_BIASES)
    bias = 0.0
    for i, k in enumerate(CONV_BIASES, 1):
        scale = ref["aux"][f"z{i}"].grad.abs().sum(0)
        bias = max(bias, float(((grads[k].detach().double().cpu() - ref["grads"][k]).abs() / scale).max()))
    return worst, bias


@pytest.mark.parametrize("name", list(CASES))
def test_cases_meet_their_preconditions(name):
    r = reference(name)
    m, clip = margins(r["aux"])
    assert m >= 1e-4 and clip >= 1e-3, (m, clip)
    raw = r["aux"]["raw_logits"].detach()
    beyond = (raw.abs() > 10.0).any(-1)
    if name != "deep":                       # the clip mask is checked at the small shapes
        assert int(beyond.sum()) >= 2 and int((~beyond).sum()) >= 2
    assert int((case(name)["ids"] > 0).sum()) >= 2


@pytest.mark.parametrize("name", list(CASES))
def test_head_forward_and_gradients_match_float64(cuda, name):
    from m3d.head_losses import mrcnn_losses
    c, r = case(name), reference(name)
    store, head = build(cuda, c)
    pooled = c["pooled"].to(cuda).requires_grad_(True)
    logits, probs, bbox = head(pooled, training=True)
    total, lc, lb, _ = mrcnn_losses(c["ids"].to(cuda), c["tbox"].to(cuda), None, logits, bbox, None,
                                    c["active"].to(cuda), (1.0, 1.0, 0.0))
    total.backward()
    for got, ref in zip((logits, probs, bbox), r["outs"]):
        assert rel(got, ref) < FWD_BAR
    grads = {k: store.by_name[k].grad for k in HT.PARAM_NAMES}
    g_err, b_err = grad_errors(grads, r)
    errs = {"loss": max(abs(float(a.detach()) - float(b)) / max(1.0, abs(float(b)))
                        for a, b in ((total, r["total"]), (lc, r["lc"]), (lb, r["lb"]))),
            "grad": g_err, "bias": b_err, "d_pooled": rel(pooled.grad, r["d_pooled"])}
    print(f"head_train {name} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= BARS[k], (k, v, BARS[k])
    assert pooled.grad.shape == pooled.shape
    # batch statistics went into the moving ones once (momentum 0.9)
    for i, bn in ((1, head.bn1), (2, head.bn2)):
        M = pooled.shape[0] * pooled.shape[1]
        mm, mv = HT.moving_update(*to64(c)["moving"][f"bn{i}"], r["aux"][f"mean{i}"].detach(),
                                  r["aux"][f"var{i}"].detach(), M, 0.9)
        assert rel(bn.moving_mean, mm) < FWD_BAR and rel(bn.moving_variance, mv) < FWD_BAR


def test_head_gradients_are_bit_reproducible_in_deterministic_mode(cuda):
    from m3d import _lib
    from m3d.head_losses import mrcnn_losses
    c = case("small5")
    _lib.set_deterministic(True, scratch_bytes=8 << 20, device=cuda)
    try:
        runs = []
        for _ in range(2):
            store, head = build(cuda, c)
            pooled = c["pooled"].to(cuda).requires_grad_(True)
            logits, _, bbox = head(pooled, training=True)
            mrcnn_losses(c["ids"].to(cuda), c["tbox"].to(cuda), None, logits, bbox, None, c["active"].to(cuda),
                         (1.0, 1.0, 0.0))[0].backward()
            runs.append((store.grad_flat.clone(), pooled.grad.clone()))
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][0].abs().max()) > 0


def test_frozen_path_is_unchanged_by_a_training_call(cuda):
    """training=False before and after a training-mode call: the same bits.  The
    training forward's one documented side effect, the moving statistics, is put
    back first (the frozen BN reads them)."""
    c = case("small2")
    store, head = build(cuda, c)
    pooled = c["pooled"].to(cuda)
    with torch.no_grad():
        first = [t.clone() for t in head(pooled)]
    saved = [(bn.moving_mean.clone(), bn.moving_variance.clone()) for bn in (head.bn1, head.bn2)]
    logits, _, bbox = head(pooled.clone().requires_grad_(True), training=True)
    (logits.sum() + bbox.sum()).backward()
    for bn, (mm, mv) in zip((head.bn1, head.bn2), saved):
        assert not torch.equal(bn.moving_mean, mm)
        bn.moving_mean.copy_(mm)
        bn.moving_variance.copy_(mv)
    with torch.no_grad():
        again = head(pooled)
        default = head(pooled, training=False)
    for a, b, d in zip(first, again, default):
        assert torch.equal(a, b) and torch.equal(a, d)


@functools.lru_cache(maxsize=None)
def steps_reference(opt):
    c = to64(case("small5", 10.0, STEPS_SEED))
    return HT.train_steps(c["p"], c["moving"], c["pooled"], c["ids"], c["tbox"], c["active"], c["nc"], STEPS,
                          OPTIMIZERS[opt][1], weight_decay=WEIGHT_DECAY)


@pytest.mark.parametrize("opt", list(OPTIMIZERS))
def test_five_step_reference_preconditions(opt):
    traj, q, _ = steps_reference(opt)
    assert float(traj[:, 3].min()) >= 1e-4
    p0 = case("small5", 10.0, STEPS_SEED)["p"]["mrcnn_bbox_fc/kernel:0"]
    assert float(p0.norm(dim=0).min()) > 1.0                       # the constraint engages on every column
    assert float(q["mrcnn_bbox_fc/kernel:0"].norm(dim=0).max()) <= 1.0


@pytest.mark.parametrize("opt", list(OPTIMIZERS))
def test_five_head_only_steps_match_float64(cuda, opt):
    from m3d.head_losses import mrcnn_losses
    from m3d.optim import KerasOptimizer, apply_max_norm
    from m3d.params import CHUNK
    c = case("small5", 10.0, STEPS_SEED)
    traj, q, moving = steps_reference(opt)
    store, head = build(cuda, c, extra=True, weight_decay=WEIGHT_DECAY)
    lo, hi = head.chunk_range()
    optimizer = KerasOptimizer(OPTIMIZERS[opt][0])
    state = optimizer.state(store)
    with torch.no_grad():
        store.grad_flat.fill_(0.25)                  # gradients and slots outside the head must not matter
        for s in state:
            s.fill_(0.125)
            s[lo * CHUNK:hi * CHUNK].zero_()
    flat0 = store.flat.detach().clone()
    state0 = [s.clone() for s in state]
    ids, tbox, active = c["ids"].to(cuda), c["tbox"].to(cuda), c["active"].to(cuda)
    pooled = c["pooled"].to(cuda)
    got = []
    for _ in range(STEPS):
        store.grad_flat[lo * CHUNK:hi * CHUNK].zero_()
        logits, _, bbox = head(pooled, training=True)
        total, lc, lb, _ = mrcnn_losses(ids, tbox, None, logits, bbox, None, active, (1.0, 1.0, 0.0))
        total.backward()
        optimizer.step(store, chunks=(lo, hi))
        apply_max_norm(store, head.max_norm_constraints)
        got.append((float(total.detach()), float(lc), float(lb)))
    got = np.array(got)
    errs = {"s_loss": float((np.abs(got - traj[:, :3]) / np.maximum(1.0, np.abs(traj[:, :3]))).max()),
            "s_param": max(rel(store.by_name[k].data, q[k]) for k in HT.PARAM_NAMES),
            "s_moving": max(max(rel(bn.moving_mean, moving[f"bn{i}"][0]), rel(bn.moving_variance, moving[f"bn{i}"][1]))
                            for i, bn in ((1, head.bn1), (2, head.bn2))),
            "s_norm": max(rel(store.by_name[k].data.norm(dim=0), q[k].norm(dim=0)) for k in HT.MAX_NORM)}
    print(f"head_train five steps {opt} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= BARS_STEPS[opt][k], (k, v, BARS_STEPS[opt][k])
    assert optimizer.iterations == STEPS
    # outside the head's chunk range: parameters and optimizer slots bit-identical
    flat = store.flat.detach()
    assert torch.equal(flat[:lo * CHUNK], flat0[:lo * CHUNK]) and torch.equal(flat[hi * CHUNK:], flat0[hi * CHUNK:])
    assert not torch.equal(flat[lo * CHUNK:hi * CHUNK], flat0[lo * CHUNK:hi * CHUNK])
    for s, s0 in zip(state, state0):
        assert torch.equal(s[:lo * CHUNK], s0[:lo * CHUNK]) and torch.equal(s[hi * CHUNK:], s0[hi * CHUNK:])
    assert float(store.by_name["mrcnn_bbox_fc/kernel:0"].data.detach().norm(dim=0).max()) <= 1.0 + 1e-6


def test_max_norm_kernel_known_answers(cuda):
    from m3d import _lib
    w = torch.tensor([[0.6, 3.0, 0.0], [0.8, 4.0, 0.0]], device=cuda)
    _lib.check(_lib.load().m3d_max_norm(w.data_ptr(), 2, 3, 2.0, _lib.stream()), "max_norm")
    want = HT.max_norm(torch.tensor([[0.6, 3.0, 0.0], [0.8, 4.0, 0.0]], dtype=torch.float64), 2.0)
    assert float((w.double().cpu() - want).abs().max()) < 4e-7
    assert torch.equal(w[:, 2], torch.zeros(2, device=cuda))
    big = torch.randn(700, 5, generator=torch.Generator().manual_seed(0)) * 0.1          # several rows per thread
    wb = big.to(cuda)
    _lib.check(_lib.load().m3d_max_norm(wb.data_ptr(), 700, 5, 1.0, _lib.stream()), "max_norm")
    assert rel(wb, HT.max_norm(big.double(), 1.0)) < 1e-6


def test_train_classifier_head_model_entry(cuda):
    """MaskRCNN.train_classifier_head at 64 x 64 x 8 (the volume, config and
    ground truth of tests/test_gpu_head_loss.py's end-to-end test)."""
    from m3d.config import synthetic_mrcnn_config
    from m3d.head_losses import LOSS_NAMES, active_class_ids_from_meta, mrcnn_losses
    from m3d.heads import MaskRCNN
    from m3d.model import compose_image_meta, synthetic_volume
    from m3d.optim import KerasOptimizer
    from m3d.params import CHUNK
    cfg = synthetic_mrcnn_config(64, depth=8, PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=300,
                                 POST_NMS_ROIS_INFERENCE=64, TRAIN_ROIS_PER_IMAGE=12, ROI_POSITIVE_RATIO=0.5,
                                 RPN_POSITIVE_IOU=0.1, RPN_NEGATIVE_IOU=0.05, USE_MINI_MASK=False,
                                 MASK_SHAPE=[28, 28, 28], DETECTION_MAX_INSTANCES=8)
    meta = torch.from_numpy(compose_image_meta(0, [64, 64, 8, 1], [64, 64, 8, 1], [0, 0, 0, 64, 64, 8], 1.0,
                                               [1, 1])[None]).to(cuda)
    boxes = np.array([[4, 4, 0, 32, 36, 8], [30, 8, 0, 60, 34, 8], [12, 36, 0, 40, 62, 8]], np.float32)
    masks = np.zeros((64, 64, 8, 3), bool)
    for g, (y1, x1, z1, y2, x2, z2) in enumerate(boxes.astype(int)):
        masks[y1:y2, x1:x2, z1:z2, g] = True
    args = (synthetic_volume(64, 8).to(cuda), meta, torch.ones((1, 3), dtype=torch.int32, device=cuda),
            torch.from_numpy(boxes[None]).to(cuda), torch.from_numpy(masks[None]).to(cuda))
    # the same losses from the pieces, on a second model of the same seed
    ref_model = MaskRCNN(cfg, device=cuda, seed=2)
    with torch.no_grad():
        _, rois, _, ids, tbox, _, maps = ref_model._head_targets(*args, 5)
        pooled = ref_model.roi_align_classifier([rois, meta] + maps)
        logits, _, bbox = ref_model.classifier(pooled, training=True)
        lw = getattr(cfg, "LOSS_WEIGHTS", {})
        want = mrcnn_losses(ids, tbox, None, logits, bbox, None, active_class_ids_from_meta(meta),
                            tuple(float(lw.get(n, 1.0)) for n in LOSS_NAMES))
    model = MaskRCNN(cfg, device=cuda, seed=2)
    lo, hi = model.classifier.chunk_range()
    flat0 = model.store.flat.detach().clone()
    bn0 = [(bn.moving_mean.clone(), bn.moving_variance.clone()) for bn in model.store.bns]
    out = model.train_classifier_head(*args, KerasOptimizer({"name": "SGD", "parameters": {
        "learning_rate": 0.01, "momentum": 0.9}}), seed=5)
    for k, w in (("loss", want[0]), ("mrcnn_class_loss", want[1]), ("mrcnn_bbox_loss", want[2])):
        assert bool(torch.isfinite(out[k]))
        assert abs(float(out[k]) - float(w)) <= 2e-6 * max(1.0, abs(float(w))), k
    assert float(out["mrcnn_class_loss"]) > 0 and int((out["target_class_ids"] > 0).sum()) > 0
    assert tuple(out["d_pooled"].shape) == tuple(pooled.shape) and float(out["d_pooled"].abs().max()) > 0
    flat = model.store.flat.detach()
    assert torch.equal(flat[:lo * CHUNK], flat0[:lo * CHUNK]) and torch.equal(flat[hi * CHUNK:], flat0[hi * CHUNK:])
    moved = [p.name for p in model.classifier.params()
             if not torch.equal(p.data, flat0[p.offset:p.offset + p.numel].view(p.shape))]
    # the conv biases' gradients cancel to rounding under batch statistics; every other tensor moves
    assert set(moved) >= {p.name for p in model.classifier.params()} - set(CONV_BIASES)
    head_bns = (model.classifier.bn1, model.classifier.bn2)
    for bn, (mm, mv) in zip(model.store.bns, bn0):
        same = torch.equal(bn.moving_mean, mm) and torch.equal(bn.moving_variance, mv)
        assert same != (bn in head_bns), bn.name
