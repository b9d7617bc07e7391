#!/usr/bin/env python
"""Bitwise digest of the training step, to compare two trees on one machine.

In deterministic mode (_lib.set_deterministic), for the "defaults",
"wino_v_prepass" and "conv1_x3_small_tiles" RPN scenarios and the train_heads
scenario of tests/test_gpu_launch_plan.py: the loss and a SHA-256 of
store.grad_flat after each of two steps, one line each.  Two trees that
compute the same bits print the same lines (the bits may differ between ROCm
versions: this is evidence for profiles/, not a golden).

  python scripts/step_digest.py > digest.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-mask-r-cnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import pytest
    import torch
    from m3d import _lib
    from m3d import nn as mnn
    from tests import test_gpu_launch_plan as T
    dev = torch.device("cuda:0")
    _lib.set_deterministic(True, device=dev)
    for name in ("defaults", "wino_v_prepass", "conv1_x3_small_tiles", "train_heads"):
        def after(step, model, r, name=name):
            torch.cuda.synchronize()
            h = hashlib.sha256(model.store.grad_flat.cpu().numpy().tobytes()).hexdigest()
            print(f"{name} step {step} loss {float(r['loss']).hex()} grad_flat {h}", flush=True)
        mp = pytest.MonkeyPatch()
        try:
            for k, v in T.RPN_SCENARIOS.get(name, {}).items():
                mp.setattr(mnn, k, v)
            if name == "train_heads":
                T._train_heads_steps(dev, T.Recorder(), steps=2, after=after)
            else:
                T._rpn_steps(dev, T.Recorder(), after=after)
        finally:
            mp.undo()
    _lib.set_deterministic(False)


if __name__ == "__main__":
    main()
