"""Generate tests/golden/tracker/decode_reference.npz by running the REAL reference's tracker post-processing (build container only).

    python -m oracle.make_decode_golden

The reference's own statements are extracted from its files and EXECUTED on seeded random inputs (nothing is copied into this
repository): `clip_box` (lib/utils/box_ops.py:117-126), the post-processing lines of UVLTrack.track (lib/test/tracker/uvltrack.py:116-125)
and its map_box_back (:167-173).  The tracker module itself cannot be imported, it needs cv2.  Stored: the inputs and the reference's
outputs, so that tests/test_oracle_golden.py pins oracle.clip_box / oracle.tracker_decode without the reference tree.
"""
from __future__ import annotations

import os
import re
import sys
import textwrap
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import as R                # noqa: E402
from oracle import uvl_oracle as O                # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tracker", "decode_reference.npz")
CLIP_CASES = 200
DECODE_SHAPES = ((16, 256), (24, 384))            # (feat_sz, search_size) of UVLTrack-B / -L
DECODE_TRIALS = 20


def reference_functions():
    import torch
    if not R.reference_available():
        raise SystemExit("reference tree not present at %s" % R.REF_ROOT)
    src = open(os.path.join(R.REF_ROOT, "lib", "test", "tracker", "uvltrack.py")).read()
    body = re.search(r"( +pred_boxes = out_dict\['bbox_map'\].*?\n +self\.state = clip_box\(.*?\n)", src, re.S)
    mbb = re.search(r"( +def map_box_back\(self, pred_box: list, resize_factor: float\):.*?\n +return \[.*?\]\n)", src, re.S)
    clip = re.search(r"def clip_box\(.*?\n    return \[x1, y1, w, h\]\n", open(os.path.join(R.REF_ROOT, "lib", "utils", "box_ops.py")).read(), re.S)
    assert body and mbb and clip, "reference statements not found"
    ns = {"torch": torch}
    exec(compile(clip.group(0), "ref_clip_box", "exec"), ns)
    exec(compile(textwrap.dedent(mbb.group(1)), "ref_map_box_back", "exec"), ns)
    return ns, compile(textwrap.dedent(body.group(1)), "ref_track_lines", "exec")


def main():
    import torch
    ns, code = reference_functions()
    d = {}
    rng = np.random.RandomState(0)
    boxes, hw, clipped = [], [], []
    for _ in range(CLIP_CASES):
        box = (rng.uniform(-50, 700, 2).tolist() + rng.uniform(1, 300, 2).tolist())
        H, W = rng.randint(100, 800, 2).tolist()
        boxes.append(box)
        hw.append([H, W])
        clipped.append(ns["clip_box"](list(box), H, W, margin=10))
    d["clip.box"], d["clip.hw"], d["clip.out"] = np.asarray(boxes, np.float64), np.asarray(hw, np.int64), np.asarray(clipped, np.float64)

    rng = np.random.RandomState(3)
    for F, search_size in DECODE_SHAPES:
        S = F * F
        window = O.hann_window(F)
        cols = {k: [] for k in ("cls", "cont", "bbox", "state", "rf", "hw", "out_state", "out_score", "out_net")}
        for _ in range(DECODE_TRIALS):
            cls = rng.uniform(0.05, 0.95, (1, F, F)).astype(np.float32)
            cont = rng.normal(0, 1.5, (1, S, 3)).astype(np.float32)
            bbox = rng.uniform(0.05, 0.95, (1, S, 4)).astype(np.float32)
            state = [float(rng.uniform(-20, 500)), float(rng.uniform(-20, 400)), float(rng.uniform(5, 200)), float(rng.uniform(5, 200))]
            rf = float(rng.uniform(0.5, 3.0))
            H, W = int(rng.randint(200, 800)), int(rng.randint(200, 1300))
            me = types.SimpleNamespace(state=list(state), has_cont=True, window=torch.from_numpy(window),
                                       params=types.SimpleNamespace(search_size=search_size))
            me.map_box_back = types.MethodType(ns["map_box_back"], me)
            loc = {"self": me, "out_dict": {"bbox_map": torch.from_numpy(bbox), "cls_score_test": torch.from_numpy(cls), "cont_score": torch.from_numpy(cont)},
                   "resize_factor": rf, "H": H, "W": W}
            exec(code, dict(ns), loc)
            for k, v in (("cls", cls[0]), ("cont", cont[0]), ("bbox", bbox[0]), ("state", state), ("rf", rf), ("hw", [H, W]),
                         ("out_state", [float(x) for x in me.state]), ("out_score", float(loc["score"])), ("out_net", loc["pred_box_net"].numpy().reshape(-1))):
                cols[k].append(v)
        for k, v in cols.items():
            dt = {"cls": np.float32, "cont": np.float32, "bbox": np.float32, "hw": np.int64, "out_net": np.float32}.get(k, np.float64)
            d["decode.f%d.%s" % (F, k)] = np.asarray(v, dt)
        d["decode.f%d.search_size" % F] = np.asarray(search_size, np.int64)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **d)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(d), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
