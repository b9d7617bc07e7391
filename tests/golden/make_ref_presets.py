"""Extract the anchor / RPN-geometry fields of the reference's 16 config
presets (configs/**/*.json of the reference tree, read as JSON data) into
tests/golden/ref_presets.json, and the key names of every preset (names only,
no values) into tests/golden/ref_preset_keys.json.  Only the keys that decide
the anchor pyramid and the RPN head's row count keep their values (derived
fixtures, not copies of the files).  Run from the repo root:
python tests/golden/make_ref_presets.py <reference tree>/configs"""
import glob
import json
import os
import sys

KEYS = ("MODE", "IMAGE_SIZE", "IMAGE_DEPTH", "IMAGE_CHANNEL_COUNT", "BACKBONE", "BACKBONE_STRIDES",
        "TOP_DOWN_PYRAMID_SIZE", "RPN_ANCHOR_SCALES", "RPN_ANCHOR_RATIOS", "RPN_ANCHOR_STRIDE")
ROOT = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))

out, names = {}, {}
for path in sorted(glob.glob(os.path.join(ROOT, "**", "*.json"), recursive=True)):
    with open(path) as f:
        d = json.load(f)
    out[os.path.relpath(path, ROOT)] = {k: d[k] for k in KEYS if k in d}
    names[os.path.relpath(path, ROOT)] = sorted(d)
with open(os.path.join(HERE, "ref_presets.json"), "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
with open(os.path.join(HERE, "ref_preset_keys.json"), "w") as f:
    json.dump(names, f, indent=1, sort_keys=True)
print(len(out), "presets")
