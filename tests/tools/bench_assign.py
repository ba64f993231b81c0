"""GPU-box micro-benchmark of the label-assignment kernels at the workload shape (N = 240, L = 4, S = 36, E = 128): device time per
launch from a hipGraph of back-to-back launches (tests/tools/bench_conv.py `timeit`).

    python tests/tools/bench_assign.py                         one JSON line for the library in use
    python tests/tools/bench_assign.py --ab OTHER.so [--rounds 3] [--out FILE]
        the built library and OTHER.so (PHNET_LIB) alternated, one fresh process per run; medians and min-max per kernel"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
KERNELS = ("lane_assign", "lane_assign_tokens", "lane_assign_one2many")


def measure():
    import torch
    from phnet_amd import hip_ops as K
    from phnet_amd.synthetic import make_targets
    from tests.tools.bench_conv import timeit
    dev = "cuda"
    torch.manual_seed(0)
    pred = torch.randn(240, 42, device=dev) * 0.3 + 0.4
    tgt = make_targets(320, 800, 1).to(dev)[0]
    feat = torch.randn(240, 128, device=dev)
    L = tgt.shape[0]
    out = (torch.zeros(L + 1, 128, device=dev), torch.zeros(L + 1, dtype=torch.bool, device=dev))
    fns = {"lane_assign": lambda: K.lane_assign(pred, tgt, 800, 320),
           "lane_assign_tokens": lambda: K.lane_assign_tokens(pred, tgt, 800, 320, feat, out),
           "lane_assign_one2many": lambda: K.lane_assign_one2many(pred, tgt, 800, 320)}
    res = {}
    for name in KERNELS:
        runs = sorted(timeit(fns[name], iters=50) for _ in range(5))
        res[name] = round(runs[len(runs) // 2], 2)
    return res


def ab(other, rounds, out):
    runs = {"branch": [], "parent": []}
    for _ in range(rounds):
        for side in ("parent", "branch"):
            env = dict(os.environ)
            if side == "parent":
                env["PHNET_LIB"] = os.path.abspath(other)
            else:
                env.pop("PHNET_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{side} run ended with {p.returncode}")
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(side, runs[side][-1], flush=True)
    summary = {"shape": {"N": 240, "L": 4, "S": 36, "E": 128}, "unit": "us per launch (hipGraph of 50 back-to-back launches)",
               "rounds": rounds, "runs": runs}
    for side in runs:
        for k in KERNELS:
            v = sorted(r[k] for r in runs[side])
            summary.setdefault(side, {})[k] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
    print(json.dumps({s: summary[s] for s in ("parent", "branch")}))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    a = sys.argv
    if "--ab" in a:
        ab(a[a.index("--ab") + 1], int(a[a.index("--rounds") + 1]) if "--rounds" in a else 3, a[a.index("--out") + 1] if "--out" in a else None)
    else:
        print(json.dumps(measure()))
