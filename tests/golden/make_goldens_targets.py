"""Golden training targets: runs the REFERENCE's own libs/dataset/openlane/transforms.py (read-only checkout at /root/reference,
loaded by path, unmodified) - Transforms.transform_annotation with its filter_lane and sample_lane - on the cases of
tests/target_cases.py and stores the inputs with the label rows it gives.
Build container only:  python tests/golden/make_goldens_targets.py   -> tests/golden/targets_tiny.json

Stand-ins (imgaug is not in this image and cannot be): `imgaug`, `imgaug.augmenters`, `imgaug.augmentables`,
`imgaug.augmentables.lines` and `libs.dataset.openlane.utils` are empty shells - transform_annotation, filter_lane and sample_lane
touch none of them; scipy and numpy are the real ones.  `Transforms.__init__` builds imgaug pipelines and is bypassed: the
instance gets a cfg with what options4OL.py:135-148 derives (max_lane_num, n_offsets, n_strips, strip_size, offsets_ys =
np.arange(height, -1, -strip_size), width).

Lanes are fed as lists of [x, y] Python floats whose values are float32-representable (multiples of 1/64) - the float64 path, not
the float32 one of the reference's loader (DESIGN.md "Training targets").  Cases marked reference = False (a non-finite
coordinate: the reference raises) are left out.  Label rows are stored without their trailing -1e5 entries."""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np

from tests import target_cases as C

REF_FILE = "/root/reference/libs/dataset/openlane/transforms.py"


def load_reference():
    shells = {"imgaug": {}, "imgaug.augmenters": {}, "imgaug.augmentables": {},
              "imgaug.augmentables.lines": dict(LineString=None, LineStringsOnImage=None),
              "libs": {}, "libs.dataset": {}, "libs.dataset.openlane": {}, "libs.dataset.openlane.utils": {}}
    saved = {k: sys.modules.get(k) for k in shells}
    for name, attrs in shells.items():
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        if name in ("imgaug", "imgaug.augmentables", "libs", "libs.dataset", "libs.dataset.openlane"):
            mod.__path__ = []
        sys.modules[name] = mod
    sys.modules["imgaug"].augmenters = sys.modules["imgaug.augmenters"]
    try:
        spec = importlib.util.spec_from_file_location("ref_transforms", REF_FILE)
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref


def trimmed(row):
    vals = [float(v) for v in row]
    while len(vals) > 2 and vals[-1] == C.INVALID:
        vals.pop()
    return vals


def main():
    ref = load_reference()
    out = {"invalid": C.INVALID, "geometries": {}}
    for name, H, W, S, R in C.GEOMETRIES:
        cfg = types.SimpleNamespace(max_lane_num=R, n_offsets=S, n_strips=S - 1, strip_size=H / (S - 1), height=H, width=W)
        cfg.offsets_ys = np.arange(cfg.height, -1, -cfg.strip_size)
        assert len(cfg.offsets_ys) == S, (name, len(cfg.offsets_ys))
        tr = object.__new__(ref.Transforms)
        tr.cfg = cfg
        recs = []
        for c in C.cases(name):
            if not c["reference"]:
                continue
            lanes = [[[float(x), float(y)] for x, y in lane] for lane in c["lanes"]]
            assert all(float(np.float32(v)) == v for lane in lanes for p in lane for v in p)
            label = tr.transform_annotation(H, W, lanes)["label"]
            assert label.dtype == np.float32 and label.shape == (R, 6 + S)
            recs.append(dict(name=c["name"], lanes=lanes, label=[trimmed(r) for r in label]))
            print(name, c["name"], "valid rows:", int(label[:, 1].sum()))
        out["geometries"][name] = dict(img_h=H, img_w=W, S=S, R=R, offsets_ys=[float(v) for v in cfg.offsets_ys], cases=recs)
    with open(os.path.join(HERE, "targets_tiny.json"), "w") as fh:
        fh.write('{"invalid": %r, "geometries": {\n' % C.INVALID)
        for gi, (name, g) in enumerate(out["geometries"].items()):
            head = {k: v for k, v in g.items() if k != "cases"}
            fh.write(' %s: {"head": %s, "cases": [\n' % (json.dumps(name), json.dumps(head)))
            fh.write(",\n".join("  " + json.dumps(r) for r in g["cases"]))
            fh.write("\n ]}%s\n" % ("," if gi + 1 < len(out["geometries"]) else ""))
        fh.write("}}\n")
    json.load(open(os.path.join(HERE, "targets_tiny.json")))


if __name__ == "__main__":
    main()
