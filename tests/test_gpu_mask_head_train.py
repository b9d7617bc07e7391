"""The mask head's training mode on the GPU (m3d.heads.MaskHead(training=True),
its kernels m3d_mask_out_bwd, m3d_conv3d_bwd_data_dil / _bwd_weight_dil,
m3d_deconv3d_k2s2_bwd_data / _bwd_weight, and MaskRCNN.train_heads) against the
float64 CPU evaluation of tests/maskhead_ref.py (pinned by
tests/test_maskhead_ref.py).

Cases (p, Cin, ch, C, B, N), parameters and inputs from maskhead_ref.case:
  tiny (3, 32, 32, 2, 2, 3)   one ROI all zero; at p = 3 the dilated taps reach only
                              0 <-> 2; 162 rows: the few-rows BN regime
  wino (6, 64, 64, 2, 1, 13)  2808 rows, above M3D_BN_TRAIN_FEW_ROWS_MAX; channels on
                              the Winograd path; 6 is 1.5 tiles
  c5   (4, 32, 32, 5, 1, 4)   the generic-C path of m3d_mask_out_bwd
  real (14, 64, 64, 2, 1, 2)  the real 14^3 -> 28^3 geometry
The upstream gradient comes from m3d.head_losses.mrcnn_mask_loss.

Branch agreement.  The float64 reference is evaluated on the GPU forward's own
ReLU sign patterns (return_activations): a pre-activation within float32
rounding of 0 otherwise flips a branch and moves every gradient upstream of it.
Separately the GPU's patterns may differ from float64's own only where the
float64 pre-activation is within 1e-4 rms of 0 and on at most 0.1 % of a layer
(tests/test_maskhead_ref.py asserts both of the float32 CPU restatement).

Bars.  Forward output: the project's 1e-4 of the output scale, and the same bar
against training=False on the batch's statistics.  Everything else: 10x the
worst error of the restatement evaluated in float32 on the CPU against float64
over these cases (scripts/measure_maskhead_f32.py prints them); tensors relative
to the reference tensor's largest entry, the loss relative to max(1, |ref|).
The five conv bias gradients are cancellations to about 0 under batch
statistics: their error is per column relative to that column's sum |dz|.

  quantity                      float32 CPU   bar       MI355X (measured)
  loss (one step)               2.64e-08      2.64e-07  3.9e-08
  parameter gradients           1.85e-06      1.85e-05  4.7e-06
  conv bias gradients           9.02e-08      9.02e-07  6.0e-08
  d_pooled                      5.02e-07      5.02e-06  2.7e-06
  moving statistics             8.00e-08      8.00e-07  7.9e-08
  five steps SGD:  losses       5.49e-08      5.49e-07  2.6e-08
                   parameters   1.12e-07      1.12e-06  1.1e-07
  forward output (bar 1e-4 of the output scale)             7.7e-06
  sign patterns differing from float64's own: at most 5.6e-06 of a layer, |pre| / rms <= 7.0e-06

m3d_mask_out_bwd alone, the dilated gradients and the deconv gradients are
compared with float64 under rounding bounds of their own sums (below), and
under tests/test_gpu_conv_paths.py's two criteria for the conv entries.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import convref as R
import maskhead_ref as MR

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
NAN = float("nan")
# worst float32-vs-float64 error of the restatement on the CPU (scripts/measure_maskhead_f32.py)
F32 = {"loss": 2.64e-08, "grad": 1.85e-06, "bias": 9.02e-08, "d_pooled": 5.02e-07, "moving": 8.00e-08,
       "s_loss": 5.49e-08, "s_param": 1.12e-07}
BARS = {k: 10.0 * v for k, v in F32.items()}
FWD_BAR = 1e-4
STEPS, LR, MOM = 5, 0.05, 0.9
DEV = "cuda:0"


def build(dev, c, extra=False):
    """A ParamStore with the mask head (and, with ``extra``, a layer before and
    after it) holding the case's parameters and moving statistics."""
    from m3d.heads import MaskHead
    from m3d.params import ConvLayer, ParamStore
    cin = c["p"]["mrcnn_mask_conv1/kernel:0"].shape[3]
    store = ParamStore()
    if extra:
        ConvLayer(store, "before", (1, 1, 1), 8, 8)
    head = MaskHead(store, c["C"], c["ch"], cin)
    if extra:
        ConvLayer(store, "after", (1, 1, 1), 8, 8)
    store.finalize(torch.device(dev), seed=3)
    with torch.no_grad():
        for k, v in c["p"].items():
            store.by_name[k].data.copy_(v)
        for name, (_, bn) in head.convs.items():
            bn.moving_mean.copy_(c["moving"]["bn" + name[4:]][0])
            bn.moving_variance.copy_(c["moving"]["bn" + name[4:]][1])
    return store, head


def one_step(dev, c):
    """forward + mask loss + backward on a fresh head: everything on the host."""
    from m3d.head_losses import mrcnn_mask_loss
    store, head = build(dev, c)
    pooled = c["pooled"].to(dev).requires_grad_(True)
    out, acts = head(pooled, training=True, return_activations=True)
    loss = mrcnn_mask_loss(c["tmask"].to(dev), c["ids"].to(dev), out)
    loss.backward()
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), masks={k: (v > 0).cpu() for k, v in acts.items()}, loss=float(loss.detach()),
                grads={k: store.by_name[k].grad.detach().cpu().clone() for k in MR.PARAM_NAMES},
                d_pooled=pooled.grad.cpu(), grad_flat=store.grad_flat.clone(),
                moving={"bn" + n[4:]: (bn.moving_mean.cpu().clone(), bn.moving_variance.cpu().clone())
                        for n, (_, bn) in head.convs.items()})


@functools.lru_cache(maxsize=None)
def gpu(name):
    return one_step(DEV, MR.case(name))


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 on the GPU forward's sign patterns."""
    return MR.reference_on(name, gpu(name)["masks"])


@functools.lru_cache(maxsize=None)
def own(name):
    return MR.reference_on(name, None)


@pytest.mark.parametrize("name", list(MR.CASES))
def test_gpu_branches_differ_from_float64_only_at_rounding(cuda, name):
    g = gpu(name)
    ps = MR.CASES[name][0]
    for k, m in g["masks"].items():
        side = 2 * ps if k == "deconv" else ps
        assert tuple(m.shape[1:4]) == (side,) * 3 and m.shape[-1] == MR.case(name)["ch"], k
    frac, margin = MR.branch_disagreement(g["masks"], own(name)["aux"])
    print(f"mask_head_train {name} branch flips: worst layer fraction {frac:.2e}, worst |pre|/rms {margin:.2e}")
    assert margin <= 1e-4 and frac <= 1e-3, (frac, margin)


@pytest.mark.parametrize("name", list(MR.CASES))
def test_forward_loss_and_gradients_match_float64(cuda, name):
    c, g, r = MR.case(name), gpu(name), reference(name)
    fwd = MR.rel(g["out"], r["out"])
    errs = MR.errors(g["loss"], g["grads"], g["d_pooled"], r)
    rows = c["pooled"].shape[0] * c["pooled"].shape[1] * MR.CASES[name][0] ** 3
    want = MR.moving_after(MR.to(c)["moving"], r["aux"], rows)
    errs["moving"] = max(max(MR.rel(a, b) for a, b in zip(g["moving"][k], want[k])) for k in want)
    print(f"mask_head_train {name} fwd={fwd:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert tuple(g["out"].shape) == tuple(r["out"].shape) and tuple(g["d_pooled"].shape) == tuple(c["pooled"].shape)
    assert fwd < FWD_BAR
    for k, v in errs.items():
        assert v <= BARS[k], (k, v, BARS[k])
    # the zero-padded ROI still receives a gradient (it is part of the batch statistics)
    assert float(g["d_pooled"][-1, -1].abs().max()) > 0


@pytest.mark.parametrize("name", ["tiny", "wino"])
def test_frozen_forward_on_the_batch_statistics_and_unchanged_inference(cuda, name):
    """training=False with the moving statistics set to the batch's equals the
    training forward to the forward bar; training=False gives the same bits
    before and after a training-mode call (its side effect, the moving
    statistics, put back first)."""
    c, g, r = MR.case(name), gpu(name), reference(name)
    store, head = build(cuda, c)
    pooled = c["pooled"].to(cuda)
    with torch.no_grad():
        first = head(pooled).clone()
    saved = [(bn.moving_mean.clone(), bn.moving_variance.clone()) for _, bn in head.convs.values()]
    out = head(pooled.clone().requires_grad_(True), training=True)
    out.sum().backward()
    for (_, bn), (mm, mv) in zip(head.convs.values(), saved):
        assert not torch.equal(bn.moving_mean, mm)
        bn.moving_mean.copy_(mm)
        bn.moving_variance.copy_(mv)
    with torch.no_grad():
        assert torch.equal(first, head(pooled)) and torch.equal(first, head(pooled, training=False))
        for n, (_, bn) in head.convs.items():
            bn.moving_mean.copy_(r["aux"]["mean_bn" + n[4:]].detach().float())
            bn.moving_variance.copy_(r["aux"]["var_bn" + n[4:]].detach().float())
        frozen = head(pooled)
    assert MR.rel(frozen, g["out"]) < FWD_BAR and MR.rel(frozen, r["out"]) < FWD_BAR


def test_five_sgd_steps_match_float64(cuda):
    from m3d.head_losses import mrcnn_mask_loss
    from m3d.optim import KerasOptimizer
    from m3d.params import CHUNK
    c = MR.case("tiny")
    c64 = MR.to(c)
    ref = MR.SGDSteps(c64["p"], c64["pooled"], c64["ids"], c64["tmask"], LR, MOM)
    store, head = build(cuda, c, extra=True)
    lo, hi = head.chunk_range()
    optimizer = KerasOptimizer({"name": "SGD", "parameters": {"learning_rate": LR, "momentum": MOM}})
    with torch.no_grad():
        store.grad_flat.fill_(0.25)                  # gradients outside the head must not matter
    flat0 = store.flat.detach().clone()
    ids, tmask, pooled = c["ids"].to(cuda), c["tmask"].to(cuda), c["pooled"].to(cuda)
    s_loss = 0.0
    for _ in range(STEPS):
        store.grad_flat[lo * CHUNK:hi * CHUNK].zero_()
        out, acts = head(pooled, training=True, return_activations=True)
        loss = mrcnn_mask_loss(tmask, ids, out)
        loss.backward()
        optimizer.step(store, chunks=(lo, hi))
        want, _ = ref.step({k: (v > 0).cpu() for k, v in acts.items()})
        s_loss = max(s_loss, abs(float(loss.detach()) - want) / max(1.0, abs(want)))
    s_param = max(MR.rel(store.by_name[k].data, torch.from_numpy(ref.cur[k])) for k in MR.PARAM_NAMES)
    print(f"mask_head_train five steps sgd s_loss={s_loss:.2e} s_param={s_param:.2e}")
    assert s_loss <= BARS["s_loss"] and s_param <= BARS["s_param"], (s_loss, s_param)
    assert optimizer.iterations == STEPS
    flat = store.flat.detach()
    assert torch.equal(flat[:lo * CHUNK], flat0[:lo * CHUNK]) and torch.equal(flat[hi * CHUNK:], flat0[hi * CHUNK:])
    assert not torch.equal(flat[lo * CHUNK:hi * CHUNK], flat0[lo * CHUNK:hi * CHUNK])


@pytest.mark.parametrize("name", ["tiny", "wino"])
def test_gradients_are_bit_reproducible_in_deterministic_mode(cuda, name):
    from m3d import _lib
    _lib.set_deterministic(True, scratch_bytes=64 << 20, device=cuda)
    try:
        runs = [one_step(cuda, MR.case(name)) for _ in range(2)]
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(runs[0]["grad_flat"], runs[1]["grad_flat"])
    assert torch.equal(runs[0]["d_pooled"], runs[1]["d_pooled"]) and torch.equal(runs[0]["out"], runs[1]["out"])
    assert float(runs[0]["grad_flat"].abs().max()) > 0


# --------------------------------------------------------------------------- m3d_mask_out_bwd alone
def same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def mask_out_inputs(V, ch, C, seed):
    rng = np.random.default_rng(seed)
    up = np.maximum(rng.normal(size=(V, ch)), 0).astype(F)              # post-ReLU: about half exactly 0
    w = rng.normal(0, 1 / math.sqrt(ch), (ch, C)).astype(F)
    out = R.sigmoid(rng.normal(0, 2, (V, C))).astype(F)
    g = rng.normal(size=(V, C)).astype(F)
    g[V // 3:V // 3 + 5] = 0                                            # all-zero g_mask rows
    init = [rng.normal(0, 0.5, s).astype(F) for s in ((ch, C), (C,), (ch,))]      # dW, db, d_deconv_bias: += targets
    return up, w, out, g, init


def mask_out_reference(up, w, out, g, init):
    """(g_up, dW, db, dbd) in float64 and their rounding bounds.  gl takes two
    rounded products, every term of a sum one more; a float32 sum of n terms in
    any grouping is within n u sum|term|, so (n + 8) u sum|term| covers a result
    and u (|init| + |sum|) more its += onto the initial value."""
    up, w, out, g = (np.asarray(a, np.float64) for a in (up, w, out, g))
    V, C = g.shape
    gl = g * out * (1 - out)
    s = gl @ w.T
    pos = up > 0
    g_up = s * pos
    e_gup = (C + 8) * U * (np.abs(gl) @ np.abs(w).T) * pos
    sums = [up.T @ gl, gl.sum(0), g_up.sum(0)]
    absd = [np.abs(up).T @ np.abs(gl), np.abs(gl).sum(0), (np.abs(gl) @ np.abs(w).T * pos).sum(0)]
    refs = [i.astype(np.float64) + t for i, t in zip(init, sums)]
    errs = [(V + 8 + C) * U * a + 2 * U * (np.abs(i) + a) for i, a in zip(init, absd)]
    return g_up, e_gup, refs, errs


def run_mask_out(dev, up, w, out, g, init, poison=True):
    from m3d import _lib
    L = _lib.load()
    V, ch = up.shape
    C = w.shape[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    d_up, d_w, d_out, d_g = t(up), t(w), t(out), t(g)
    dW, db, dbd = (t(i.copy()) for i in init)
    wsb = int(L.m3d_mask_out_bwd_workspace_bytes(V, ch, C))
    guard = 1024
    buf = torch.full((V * ch + 2 * guard,), NAN, dtype=torch.float32, device=dev)       # NaN-poisoned, guarded
    g_up = buf[guard:guard + V * ch]
    ws = torch.full((wsb // 4 + 2 * guard,), NAN if poison else 0.0, dtype=torch.float32, device=dev)
    _lib.check(L.m3d_mask_out_bwd(d_g.data_ptr(), d_out.data_ptr(), d_up.data_ptr(), d_w.data_ptr(), V, ch, C,
                                  g_up.data_ptr(), dW.data_ptr(), db.data_ptr(), dbd.data_ptr(),
                                  ws[guard:].data_ptr(), wsb, _lib.stream()), "mask_out_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + V * ch:]).all()), "g_up overrun"
    if poison:
        assert bool(torch.isnan(ws[:guard]).all()) and bool(torch.isnan(ws[guard + wsb // 4:]).all()), "ws overrun"
    return g_up.cpu().numpy().reshape(V, ch), [a.cpu().numpy() for a in (dW, db, dbd)]


# (V, ch, C): V not a multiple of the 256-row block; one wave per row (ch 256); idle lanes (ch 24: 6 of 8);
# the generic-C kernel (C != 2), C = 8 its widest; 2^18 rows and more: 1024 rows per workgroup
MASK_OUT_CASES = [(1000, 64, 2), (300, 256, 2), (77, 24, 3), (513, 32, 5), (256, 32, 8), (1, 4, 1),
                  ((1 << 18) + 77, 32, 2)]


@pytest.mark.parametrize("V,ch,C", MASK_OUT_CASES)
def test_mask_out_bwd_matches_float64(cuda, V, ch, C):
    up, w, out, g, init = mask_out_inputs(V, ch, C, 11 + ch + C)
    g_up, sums = run_mask_out(cuda, up, w, out, g, init)
    ref_gup, e_gup, refs, errs = mask_out_reference(up, w, out, g, init)
    assert np.isfinite(g_up).all(), "g_up not written whole (NaN left)"
    assert (g_up[up <= 0] == 0).all() and (g_up[V // 3:V // 3 + 5] == 0).all()
    d = np.abs(g_up - ref_gup)
    print(f"mask_out_bwd V={V} ch={ch} C={C}: g_up err/bound {float((d / (e_gup + 1e-300)).max()):.3f}, sums " +
          " ".join(f"{float((np.abs(a - b) / e).max()):.3f}" for a, b, e in zip(sums, refs, errs)))
    assert (d <= e_gup + 1e-37).all()
    for name, a, b, e in zip(("dW", "db", "d_deconv_bias"), sums, refs, errs):
        assert np.isfinite(a).all() and (np.abs(a - b) <= e).all(), name
    # no atomics: the same bits again, in normal mode, whatever the workspace held
    g_up2, sums2 = run_mask_out(cuda, up, w, out, g, init, poison=False)
    assert same_bits(g_up, g_up2) and all(same_bits(a, b) for a, b in zip(sums, sums2))


def test_mask_out_bwd_past_4gib(cuda):
    """up and g_up of 2^31 + 768 floats each (8 GiB): element offsets past 2^31.
    The float64 reference runs on the device in row chunks (test oracle only)."""
    from m3d import _lib
    L = _lib.load()
    ch, C = 256, 2
    V = (1 << 23) + 3
    gen = torch.Generator(device=cuda).manual_seed(3)
    up = torch.randn((V, ch), device=cuda, generator=gen).clamp_(min=0)
    w = torch.randn((ch, C), device=cuda, generator=gen) / 16
    out = torch.sigmoid(torch.randn((V, C), device=cuda, generator=gen))
    g = torch.randn((V, C), device=cuda, generator=gen)
    g_up = torch.full((V, ch), NAN, device=cuda)
    dW, db, dbd = (torch.zeros(s, device=cuda) for s in ((ch, C), (C,), (ch,)))
    wsb = int(L.m3d_mask_out_bwd_workspace_bytes(V, ch, C))
    ws = torch.empty(wsb // 4, device=cuda)
    _lib.check(L.m3d_mask_out_bwd(g.data_ptr(), out.data_ptr(), up.data_ptr(), w.data_ptr(), V, ch, C,
                                  g_up.data_ptr(), dW.data_ptr(), db.data_ptr(), dbd.data_ptr(), ws.data_ptr(), wsb,
                                  _lib.stream()), "mask_out_bwd")
    gl = (g * out * (1 - out)).double()
    rW = torch.zeros((ch, C), device=cuda, dtype=torch.float64)
    rbd = torch.zeros(ch, device=cuda, dtype=torch.float64)
    aW, abd = torch.zeros_like(rW), torch.zeros_like(rbd)
    worst = 0.0
    step = 1 << 20
    for v0 in range(0, V, step):
        u = up[v0:v0 + step].double()
        ref = (gl[v0:v0 + step] @ w.double().T) * (u > 0)
        worst = max(worst, float((g_up[v0:v0 + step].double() - ref).abs().max()))
        rW += u.T @ gl[v0:v0 + step]
        aW += u.T @ gl[v0:v0 + step].abs()
        rbd += ref.sum(0)
        abd += ref.abs().sum(0)
    assert bool(torch.isfinite(g_up[-4:]).all()) and worst <= 1e-6            # |g_up| ~ 0.03: a few float32 ulps
    # the longest chain of float32 additions behind one sum: a thread's 256 rows, 4 row groups, a fold
    # slice's workgroups, 16 slices (+ 8 for the terms' own roundings); each adds at most u sum|term|
    chain = 256 + 4 + -(-(-(-V // 1024)) // 16) + 16 + 8
    for got, ref, absd in ((dW, rW, aW), (db, gl.sum(0), gl.abs().sum(0)), (dbd, rbd, abd)):
        assert bool(((got.double() - ref).abs() <= chain * U * absd).all())


# --------------------------------------------------------------------------- dilated gradients
def dev_in(a, dev):
    return torch.from_numpy(np.array(a, F, order="C")).to(dev)


def compare(got, ref, err, what):
    """tests/test_gpu_conv_paths.py's criterion 1 (1e-4 of scale) and bound 2 (the rounding bound)"""
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    assert np.isfinite(got).all(), what + ": an element was never written (NaN) or overflowed"
    d = np.abs(got - ref)
    print("%s: max err %.3e, 1e-4 of scale %.3e, largest err / bound %.3f"
          % (what, d.max(), 1e-4 * np.abs(ref).max(), float((d / (err + 1e-300)).max())))
    assert float(d.max()) <= 1e-4 * float(np.abs(ref).max()), what
    assert bool((d <= err + 1e-37).all()), what + ": past the rounding bound"


# (id, B, sp, cin, cout, k, pad, dil): pad != dilation except in the last ('same' at dilation 2, several m-splits)
DIL_CASES = [("d2p1", 2, (7, 6, 9), 8, 32, (3, 3, 3), (1, 1, 1), (2, 2, 2)),
             ("d3p2", 2, (9, 7, 8), 8, 32, (3, 3, 3), (2, 2, 2), (3, 3, 3)),
             ("d231", 2, (7, 9, 8), 12, 64, (3, 3, 3), (1, 2, 0), (2, 3, 1)),
             ("d2same", 2, (12, 12, 12), 32, 32, (3, 3, 3), (2, 2, 2), (2, 2, 2))]


@functools.lru_cache(maxsize=None)
def dil_data(cid):
    _, B, sp, cin, cout, k, pad, dil = next(c for c in DIL_CASES if c[0] == cid)
    rng = np.random.default_rng(sum(map(ord, cid)))
    out = tuple(n + 2 * p - d * (kk - 1) for n, p, d, kk in zip(sp, pad, dil, k))
    K = math.prod(k) * cout
    x = rng.normal(size=(B, *sp, cin)).astype(F)
    dz = rng.normal(size=(B, *out, cout)).astype(F)
    w = rng.normal(0, 1 / math.sqrt(K), (*k, cin, cout)).astype(F)
    dx0 = rng.normal(0, 0.5, x.shape).astype(F)
    dw0 = rng.normal(0, 3.0, w.shape).astype(F)

    def adjoints(dzv, wv, xv):
        dx, dw = np.zeros(x.shape), np.zeros(w.shape)
        for tap, o, i in R._taps(sp, out, k, (1, 1, 1), pad, dil):
            dx[i] += dzv[o] @ wv[tap].T
            dw[tap] += np.tensordot(xv[i], dzv[o], axes=([0, 1, 2, 3], [0, 1, 2, 3]))
        return dx, dw
    dx, dw = adjoints(dz.astype(np.float64), w.astype(np.float64), x.astype(np.float64))
    adx, adw = adjoints(np.abs(dz).astype(np.float64), np.abs(w).astype(np.float64), np.abs(x).astype(np.float64))
    return dict(x=x, dz=dz, w=w, dx0=dx0, dw0=dw0, out=out, dx=dx, dw=dw, adx=adx, adw=adw, K=K,
                M=B * math.prod(out))


def run_dgrad(dev, cid, acc, dil=None, plain=False, d=None):
    from m3d import _lib
    L = _lib.load()
    _, B, sp, cin, cout, k, pad, dl = cid if isinstance(cid, tuple) else next(c for c in DIL_CASES if c[0] == cid)
    d = d or dil_data(cid)
    dz, w = dev_in(d["dz"], dev), dev_in(d["w"], dev)
    dx = dev_in(d["dx0"], dev) if acc else torch.full((B, *sp, cin), NAN, device=dev)
    if plain:
        rc = L.m3d_conv3d_bwd_data(dz.data_ptr(), w.data_ptr(), B, *sp, cin, *k, cout, *d["out"], 1, 1, 1, *pad,
                                   dx.data_ptr(), acc, _lib.stream())
    else:
        rc = L.m3d_conv3d_bwd_data_dil(dz.data_ptr(), w.data_ptr(), B, *sp, cin, *k, cout, *d["out"], 1, 1, 1, *pad,
                                       *(dil or dl), dx.data_ptr(), acc, _lib.stream())
    _lib.check(rc, cid)
    return dx.cpu().numpy()


def run_wgrad(dev, cid, det, dil=None, plain=False, d=None):
    from m3d import _lib
    L = _lib.load()
    _, B, sp, cin, cout, k, pad, dl = cid if isinstance(cid, tuple) else next(c for c in DIL_CASES if c[0] == cid)
    d = d or dil_data(cid)
    x, dz, dw = dev_in(d["x"], dev), dev_in(d["dz"], dev), dev_in(d["dw0"], dev)
    scratch = torch.empty(8 * dw.numel(), device=dev) if det else None
    dt = _lib.Det(1, scratch.data_ptr(), scratch.numel() * 4) if det else None
    dp = ctypes.addressof(dt) if det else None
    if plain:
        rc = L.m3d_conv3d_bwd_weight(x.data_ptr(), dz.data_ptr(), B, *sp, cin, *k, cout, *d["out"], 1, 1, 1, *pad,
                                     dw.data_ptr(), dp, _lib.stream())
    else:
        rc = L.m3d_conv3d_bwd_weight_dil(x.data_ptr(), dz.data_ptr(), B, *sp, cin, *k, cout, *d["out"], 1, 1, 1, *pad,
                                         *(dil or dl), dw.data_ptr(), dp, _lib.stream())
    _lib.check(rc, cid)
    return dw.cpu().numpy()


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("cid", [c[0] for c in DIL_CASES])
def test_bwd_data_dil_matches_float64(cuda, cid, acc):
    d = dil_data(cid)
    got = run_dgrad(cuda, cid, acc)
    ref, err = d["dx"], R.sum_bound(d["K"], d["adx"])
    if acc:
        ref = ref + d["dx0"]
        err = R._round(ref, err)
    compare(got, ref, err, "bwd_data_dil %s acc %d" % (cid, acc))


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("cid", [c[0] for c in DIL_CASES])
def test_bwd_weight_dil_matches_float64(cuda, cid, det):
    _, B, sp, cin, cout, k, pad, dl = next(c for c in DIL_CASES if c[0] == cid)
    d = dil_data(cid)
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    _, target, splits, _ = R.wgrad_path(d["M"], cin, math.prod(k), cout, False, det, 8 * d["dw0"].size, ncu)
    got = run_wgrad(cuda, cid, det)
    compare(got, d["dw"] + d["dw0"], R.wgrad_bound(d["M"], d["adw"], d["dw0"], splits),
            "bwd_weight_dil %s det %d (%d splits)" % (cid, det, splits))
    if det:
        assert same_bits(run_wgrad(cuda, cid, det), got), "deterministic mode differs between two calls"
    if cid == "d2same":
        assert splits > 1


def plain_case(case):
    """the case's tensors as a dilation-1 conv: 'same' 3^3 (pad 1), the output grid of the input's size"""
    _, B, sp, cin, cout, k, _, _ = case
    rng = np.random.default_rng(5)
    return dict(x=rng.normal(size=(B, *sp, cin)).astype(F), dz=rng.normal(size=(B, *sp, cout)).astype(F),
                w=rng.normal(0, 0.05, (*k, cin, cout)).astype(F), dx0=rng.normal(size=(B, *sp, cin)).astype(F),
                dw0=rng.normal(size=(*k, cin, cout)).astype(F), out=sp)


@pytest.mark.parametrize("cid", ["d2p1", "d2same"])
def test_dilation_one_is_the_plain_entry_bit_for_bit(cuda, cid):
    case = next(c for c in DIL_CASES if c[0] == cid)[:6] + ((1, 1, 1), (1, 1, 1))
    d = plain_case(case)
    for acc in (0, 1):
        assert same_bits(run_dgrad(cuda, case, acc, d=d), run_dgrad(cuda, case, acc, plain=True, d=d))
    # deterministic mode: the m-splits' partial tiles are added in order
    assert same_bits(run_wgrad(cuda, case, True, d=d), run_wgrad(cuda, case, True, plain=True, d=d))
    # atomic mode is reproducible with a single m-split only: one batch item of d2p1 is 378 <= 512 rows
    if cid == "d2p1":
        one = (cid, 1) + case[2:]
        assert math.prod(one[2]) <= 512
        d1 = plain_case(one)
        assert same_bits(run_wgrad(cuda, one, False, d=d1), run_wgrad(cuda, one, False, plain=True, d=d1))


# --------------------------------------------------------------------------- deconv backward
@pytest.mark.parametrize("cin,cout", [(36, 32), (32, 8)])
def test_deconv_k2s2_backward_matches_float64(cuda, cin, cout):
    """dx and dw of y[2i+t, o] = sum_c x[i,c] w[t,o,c] from g = dy: the vector
    loader (Cout % 32 == 0) and the scalar one; dw accumulates onto dw0; the
    deterministic mode twice gives the same bits."""
    from m3d import _lib
    L = _lib.load()
    rng = np.random.default_rng(cin + cout)
    B, sp = 2, (3, 5, 4)
    x = rng.normal(size=(B, *sp, cin)).astype(F)
    g = rng.normal(size=(B, *(2 * n for n in sp), cout)).astype(F)
    w = rng.normal(0, 1 / math.sqrt(8 * cout), (2, 2, 2, cout, cin)).astype(F)
    dw0 = rng.normal(size=w.shape).astype(F)

    def adjoints(gv, wv, xv):
        dx, dw = np.zeros(x.shape), np.zeros(w.shape)
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    gs = gv[:, a::2, b::2, c::2]
                    dx += gs @ wv[a, b, c]
                    dw[a, b, c] = np.tensordot(gs, xv, axes=([0, 1, 2, 3], [0, 1, 2, 3]))
        return dx, dw
    dx, dw = adjoints(g.astype(np.float64), w.astype(np.float64), x.astype(np.float64))
    adx, adw = adjoints(np.abs(g).astype(np.float64), np.abs(w).astype(np.float64), np.abs(x).astype(np.float64))
    d_x, d_g, d_w = dev_in(x, cuda), dev_in(g, cuda), dev_in(w, cuda)
    got = torch.full(x.shape, NAN, device=cuda)
    _lib.check(L.m3d_deconv3d_k2s2_bwd_data(d_g.data_ptr(), d_w.data_ptr(), B, *sp, cin, cout, got.data_ptr(),
                                            _lib.stream()), "deconv bwd_data")
    compare(got.cpu().numpy(), dx, R.sum_bound(8 * cout, adx), "deconv bwd_data %d->%d" % (cin, cout))
    M = B * math.prod(sp)
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    runs = []
    for det in (False, True, True):
        scratch = torch.empty(8 * w.size, device=cuda) if det else None
        dt = _lib.Det(1, scratch.data_ptr(), scratch.numel() * 4) if det else None
        dwt = dev_in(dw0, cuda)
        _lib.check(L.m3d_deconv3d_k2s2_bwd_weight(d_x.data_ptr(), d_g.data_ptr(), B, *sp, cin, cout, dwt.data_ptr(),
                                                  ctypes.addressof(dt) if det else None, _lib.stream()),
                   "deconv bwd_weight")
        _, _, splits, _ = R.wgrad_path(M, cout, 8, cin, False, det, 8 * w.size, ncu)
        runs.append(dwt.cpu().numpy())
        compare(runs[-1], dw + dw0, R.wgrad_bound(M, adw, dw0, splits),
                "deconv bwd_weight %d->%d det %d" % (cin, cout, det))
    assert same_bits(runs[1], runs[2])


# --------------------------------------------------------------------------- the model entry
def toy_args(cuda, depth):
    from m3d.model import compose_image_meta, synthetic_volume
    meta = torch.from_numpy(compose_image_meta(0, [64, 64, depth, 1], [64, 64, depth, 1], [0, 0, 0, 64, 64, depth],
                                               1.0, [1, 1])[None]).to(cuda)
    boxes = np.array([[4, 4, 0, 32, 36, depth], [30, 8, 0, 60, 34, depth], [12, 36, 0, 40, 62, depth]], np.float32)
    masks = np.zeros((64, 64, depth, 3), bool)
    for g, (y1, x1, z1, y2, x2, z2) in enumerate(boxes.astype(int)):
        masks[y1:y2, x1:x2, z1:z2, g] = True
    return (synthetic_volume(64, depth).to(cuda), meta, torch.ones((1, 3), dtype=torch.int32, device=cuda),
            torch.from_numpy(boxes[None]).to(cuda), torch.from_numpy(masks[None]).to(cuda))


def toy_config(depth, **kw):
    from m3d.config import synthetic_mrcnn_config
    d = dict(PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=300, POST_NMS_ROIS_INFERENCE=64, TRAIN_ROIS_PER_IMAGE=12,
             ROI_POSITIVE_RATIO=0.5, RPN_POSITIVE_IOU=0.1, RPN_NEGATIVE_IOU=0.05, USE_MINI_MASK=False,
             MASK_SHAPE=[28, 28, 28], DETECTION_MAX_INSTANCES=8)
    d.update(kw)
    return synthetic_mrcnn_config(64, depth=depth, **d)


SGD = {"name": "SGD", "parameters": {"learning_rate": 0.01, "momentum": 0.9}}


def test_train_heads_classifier_only_is_train_classifier_head(cuda):
    """heads=("classifier",) reproduces train_classifier_head bit for bit in
    deterministic mode (the volume and ground truth of tests/test_gpu_head_train.py)."""
    from m3d import _lib
    from m3d.heads import MaskRCNN
    from m3d.optim import KerasOptimizer
    cfg, args = toy_config(8), toy_args(cuda, 8)
    _lib.set_deterministic(True, scratch_bytes=64 << 20, device=cuda)
    try:
        a, b = MaskRCNN(cfg, device=cuda, seed=2), MaskRCNN(cfg, device=cuda, seed=2)
        ra = a.train_classifier_head(*args, KerasOptimizer(SGD), seed=5)
        rb = b.train_heads(*args, KerasOptimizer(SGD), seed=5, heads=("classifier",))
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(a.store.flat.detach(), b.store.flat.detach())
    assert torch.equal(a.store.moments, b.store.moments) and torch.equal(a.store.grad_flat, b.store.grad_flat)
    for k in ("loss", "mrcnn_class_loss", "mrcnn_bbox_loss", "d_pooled", "rois", "target_class_ids", "target_bbox"):
        assert torch.equal(ra[k], rb[k]), k
    for x, y in zip(a.store.bns, b.store.bns):
        assert torch.equal(x.moving_mean, y.moving_mean) and torch.equal(x.moving_variance, y.moving_variance)
    assert "mrcnn_mask_loss" not in rb and "d_mask_pooled" not in rb


def test_train_heads_both_heads_on_a_toy_volume(cuda):
    """One step of both heads at 64^3: finite losses that equal the pieces',
    only the two heads' chunks move, every trunk parameter and trunk BN statistic
    is bit-unchanged."""
    from m3d.head_losses import LOSS_NAMES, active_class_ids_from_meta, mrcnn_losses
    from m3d.heads import MaskRCNN
    from m3d.optim import KerasOptimizer
    from m3d.params import CHUNK
    # the untrained RPN's proposals are thin in z at depth 64: IoU thresholds that still give positives
    cfg = toy_config(64, HEAD_CONV_CHANNEL=64, RPN_POSITIVE_IOU=0.02, RPN_NEGATIVE_IOU=0.01)
    args = toy_args(cuda, 64)
    ref_model = MaskRCNN(cfg, device=cuda, seed=2)
    with torch.no_grad():
        _, rois, _, ids, tbox, tmask, maps = ref_model._head_targets(*args, 5)
        pooled = ref_model.roi_align_classifier([rois, args[1]] + maps)
        mpooled = ref_model.roi_align_mask([rois, args[1]] + maps)
        logits, _, bbox = ref_model.classifier(pooled, training=True)
        mask = ref_model.mask_head(mpooled, training=True)
        lw = getattr(cfg, "LOSS_WEIGHTS", {})
        want = mrcnn_losses(ids, tbox, tmask, logits, bbox, mask, active_class_ids_from_meta(args[1]),
                            tuple(float(lw.get(n, 1.0)) for n in LOSS_NAMES))
    model = MaskRCNN(cfg, device=cuda, seed=2)
    lo, hi = model.classifier.chunk_range()[0], model.mask_head.chunk_range()[1]
    assert model.classifier.chunk_range()[1] == model.mask_head.chunk_range()[0]
    flat0 = model.store.flat.detach().clone()
    bn0 = [(bn.moving_mean.clone(), bn.moving_variance.clone()) for bn in model.store.bns]
    optimizer = KerasOptimizer(SGD)
    out = model.train_heads(*args, optimizer, seed=5)
    assert optimizer.iterations == 1
    for k, w in zip(("loss", "mrcnn_class_loss", "mrcnn_bbox_loss", "mrcnn_mask_loss"), want):
        assert bool(torch.isfinite(out[k]))
        assert abs(float(out[k]) - float(w)) <= 2e-6 * max(1.0, abs(float(w))), k
    assert float(out["mrcnn_mask_loss"]) > 0 and int((out["target_class_ids"] > 0).sum()) > 0
    assert tuple(out["d_pooled"].shape) == tuple(pooled.shape) and float(out["d_pooled"].abs().max()) > 0
    assert tuple(out["d_mask_pooled"].shape) == tuple(mpooled.shape) and float(out["d_mask_pooled"].abs().max()) > 0
    assert bool(torch.isfinite(out["d_mask_pooled"]).all())
    flat = model.store.flat.detach()
    assert torch.equal(flat[:lo * CHUNK], flat0[:lo * CHUNK]) and torch.equal(flat[hi * CHUNK:], flat0[hi * CHUNK:])
    trunk = [p for p in model.store.params if not lo * CHUNK <= p.offset < hi * CHUNK]
    assert trunk and all(torch.equal(p.data, flat0[p.offset:p.offset + p.numel].view(p.shape)) for p in trunk)
    cancelling = set(MR.CONV_BIASES) | {"mrcnn_class_conv1/bias:0", "mrcnn_class_conv2/bias:0"}
    heads = model.classifier.params() + model.mask_head.params()
    moved = {p.name for p in heads if not torch.equal(p.data, flat0[p.offset:p.offset + p.numel].view(p.shape))}
    assert moved >= {p.name for p in heads} - cancelling
    head_bns = [model.classifier.bn1, model.classifier.bn2] + [bn for _, bn in model.mask_head.convs.values()]
    for bn, (mm, mv) in zip(model.store.bns, bn0):
        same = torch.equal(bn.moving_mean, mm) and torch.equal(bn.moving_variance, mv)
        assert same != any(bn is h for h in head_bns), bn.name
