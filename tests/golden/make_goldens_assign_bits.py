"""Records what the label-assignment kernels compute, bit for bit, into tests/golden/assign_parent_bits.npz.

Run on the GPU at the commit whose results are to be pinned (the parent of a change to csrc/assign_device.h / assign.hip):

    python tests/golden/make_goldens_assign_bits.py [--out FILE]

Only the public hip_ops.lane_assign(..., want_cost=True), lane_assign_tokens and lane_assign_one2many are used.  The inputs are
drawn on the host from numpy seeds (case_inputs below - the tests regenerate them from the recorded case list); the outputs are
kept as raw bits (floats as uint32).  tests/test_assign_bits_gpu.py holds a later build to these bits, tests/test_assign_bits_cpu.py
checks that the fixture is consistent in itself."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "assign_parent_bits.npz")
IMG_W, IMG_H = 800, 320

# N anchors, L label rows, S x-columns, E feature width, `valid` flag per label row; `off`: label columns outside [0, img_w)
# ("part": label 0 starts left of the image and ends right of it, "whole": additionally label 2 lies wholly outside, t_len = 0);
# `dup`: "pair" = anchors 5 and 6 identical, "all" = every anchor identical (ties go to the lowest index)
CASES = [
    dict(N=240, L=4, S=36, E=128, valid=[1, 1, 1, 1]),            # the workload shape with 4, 3, 1 and 0 valid labels
    dict(N=240, L=4, S=36, E=128, valid=[1, 1, 1, 0]),
    dict(N=240, L=4, S=36, E=128, valid=[0, 1, 0, 0]),
    dict(N=240, L=4, S=36, E=128, valid=[0, 0, 0, 0]),
    dict(N=1, L=1, S=1, E=16, valid=[1]),                         # odd row width: scalar path
    dict(N=3, L=4, S=3, E=32, valid=[1, 0, 1, 0]),                # fewer anchors than labels, interleaved validity
    dict(N=63, L=2, S=2, E=16, valid=[1, 1]),
    dict(N=64, L=3, S=16, E=256, valid=[1, 0, 1]),
    dict(N=65, L=3, S=18, E=32, valid=[1, 1, 1], off="part"),     # one full 16-column trip + remainder
    dict(N=256, L=4, S=72, E=256, valid=[1, 1, 1, 1]),
    dict(N=256, L=2, S=250, E=128, valid=[0, 1]),                 # the longest row
    dict(N=240, L=4, S=36, E=128, valid=[1, 1, 1, 1], off="whole"),
    dict(N=64, L=4, S=36, E=128, valid=[1, 1, 1, 1], dup="pair"),
    dict(N=65, L=4, S=16, E=32, valid=[1, 0, 1, 1], dup="all"),
    dict(N=240, L=1, S=36, E=128, valid=[1]),
]
for _i, _c in enumerate(CASES):
    _c.setdefault("off", None); _c.setdefault("dup", None); _c["seed"] = 7100 + _i


def case_inputs(c):
    """(pred [N,6+S], tgt [L,6+S], feat [N,E]) float32 of one case, from its seed alone."""
    r = np.random.default_rng(c["seed"])
    N, L, S, E = c["N"], c["L"], c["S"], c["E"]
    pred = (r.normal(size=(N, 6 + S)) * 0.3 + 0.4).astype(np.float32)
    tgt = np.zeros((L, 6 + S), np.float32)
    tgt[:, 1] = np.asarray(c["valid"], np.float32)
    tgt[:, 2:5] = r.uniform(0.05, 0.95, (L, 3)).astype(np.float32)
    tgt[:, 5] = S
    xs = r.uniform(150, 650, (L, 1)) + r.normal(0, 6, (L, S)).cumsum(1)
    tgt[:, 6:] = np.clip(xs, 1.0, IMG_W - 2.0).astype(np.float32)
    if c["off"] in ("part", "whole"):
        tgt[0, 6:6 + (S + 2) // 3] = -2.0
        tgt[0, 6 + S - (S + 3) // 4:] = float(IMG_W)             # x == img_w is outside
    if c["off"] == "whole":
        tgt[2, 6:] = -1e5
    if c["dup"] == "pair":
        pred[6] = pred[5]
    if c["dup"] == "all":
        pred[:] = pred[0]
    feat = r.normal(size=(N, E)).astype(np.float32)
    return pred, tgt, feat


def bits(t):
    """A device tensor as a host array of raw bits (floats as uint32)."""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_case(c, K, torch):
    """The three public calls on one case -> dict of raw-bit host arrays."""
    pred, tgt, feat = (torch.from_numpy(a).cuda() for a in case_inputs(c))
    L, E = c["L"], c["E"]
    rows_by_col, rows_sorted, n_valid, cost = K.lane_assign(pred, tgt, IMG_W, IMG_H, want_cost=True)
    tokens = torch.zeros((L + 1, E), dtype=torch.float32, device="cuda")
    valid = torch.zeros(L + 1, dtype=torch.bool, device="cuda")
    tok_sorted = K.lane_assign_tokens(pred, tgt, IMG_W, IMG_H, feat, (tokens, valid))
    m_rows, m_cols, m_n = K.lane_assign_one2many(pred, tgt, IMG_W, IMG_H)
    torch.cuda.synchronize()
    return dict(cost=bits(cost), rows_by_col=bits(rows_by_col), rows_sorted=bits(rows_sorted), n_valid=bits(n_valid).reshape(1),
                tok_rows_sorted=bits(tok_sorted), tokens=bits(tokens), valid=bits(valid).astype(np.uint8),
                many_rows=bits(m_rows), many_cols=bits(m_cols), many_n=bits(m_n).reshape(1))


def load(path=FIXTURE):
    """[(case dict, {name: array})] of the committed fixture."""
    z = np.load(path)
    cases = json.loads(str(z["cases"]))
    return [(c, {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}) for i, c in enumerate(cases)]


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    from phnet_amd import hip_ops as K
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    arrays = {"cases": np.asarray(json.dumps(CASES))}
    for i, c in enumerate(CASES):
        for k, v in run_case(c, K, torch).items():
            arrays[f"c{i}_{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(CASES)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
