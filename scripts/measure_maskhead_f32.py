"""float32-vs-float64 error of the mask head's training step on the CPU: the
figures the bars of tests/test_gpu_mask_head_train.py are 10x of.

For every case of tests/maskhead_ref.CASES the restatement runs in float32,
then in float64 on the float32 run's ReLU sign patterns (a pre-activation within
float32 rounding of 0 otherwise flips a branch and the comparison measures the
flip, not the arithmetic).  Printed: per case the errors of maskhead_ref.errors
and of the moving statistics after the step; then five SGD steps on the tiny
case (losses, parameters); then the worst of each over the cases.

    python scripts/measure_maskhead_f32.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import maskhead_ref as MR  # noqa: E402

STEPS, LR, MOM = 5, 0.05, 0.9


def one_step(name):
    c32 = MR.to(MR.case(name), torch.float32)
    loss, grads, d_pooled, out, aux = MR.loss_and_grads(c32["p"], c32["pooled"], c32["ids"], c32["tmask"])
    masks = MR.masks_of(aux)
    ref = MR.reference_on(name, masks)
    e = MR.errors(loss, grads, d_pooled, ref)
    e["fwd"] = MR.rel(out, ref["out"])
    rows = aux["z_conv1"].numel() // aux["z_conv1"].shape[-1]
    m32 = MR.moving_after(c32["moving"], aux, rows)
    m64 = MR.moving_after(MR.to(MR.case(name))["moving"], ref["aux"], rows)
    e["moving"] = max(max(MR.rel(a, b) for a, b in zip(m32[k], m64[k])) for k in m32)
    own = MR.reference_on(name, None)
    e["flip_frac"], e["flip_margin"] = MR.branch_disagreement(masks, own["aux"])
    return e


def five_steps():
    c32, c64 = MR.to(MR.case("tiny"), torch.float32), MR.to(MR.case("tiny"))
    a = MR.SGDSteps(c32["p"], c32["pooled"], c32["ids"], c32["tmask"], LR, MOM)
    b = MR.SGDSteps(c64["p"], c64["pooled"], c64["ids"], c64["tmask"], LR, MOM)
    s_loss = 0.0
    for _ in range(STEPS):
        la, aux = a.step()
        lb, _ = b.step(MR.masks_of(aux))
        s_loss = max(s_loss, abs(la - lb) / max(1.0, abs(lb)))
    s_param = max(float(np.abs(a.cur[k] - b.cur[k]).max() / np.abs(b.cur[k]).max()) for k in MR.PARAM_NAMES)
    return {"s_loss": s_loss, "s_param": s_param}


def main():
    worst = {}
    for name in MR.CASES:
        e = one_step(name)
        print(f"{name:5s} " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    s = five_steps()
    print("tiny five SGD steps " + " ".join(f"{k}={v:.2e}" for k, v in s.items()))
    worst.update(s)
    print("worst " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))


if __name__ == "__main__":
    main()
