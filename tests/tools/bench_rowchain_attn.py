"""GPU-box micro-benchmark of the row chain with the cross-attention stage (csrc/rowchain.hip: rowchain_attn_kernel) next to the
launches it replaces, at the workload shape (240 rows, E = 128, FF = 256, 8 heads, 40 keys, dropout 0.1): device time from a hipGraph
of back-to-back repetitions (tests/tools/bench_conv.py `timeit`), so a sequence of three launches pays its two launch boundaries
as it does in the step - except that everything is L2-warm here.

    python tests/tools/bench_rowchain_attn.py [--rounds 5] [--out FILE]

Forms the decoder reaches: "A+CA+B" = [out-projection .. q] -> cross-attention -> [out-projection .. next q|k|v] (layer 2),
"CA+B" = cross-attention -> [out-projection .. ] with q and t from the batched prefix (layer 1); each against its separate launches."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
R, E, FF, H, LK, P = 240, 128, 256, 8, 40, 0.1


def measure(rounds):
    import torch
    from phnet_amd import hip_ops as K
    from tests.tools.bench_conv import timeit
    dev = "cuda"
    torch.manual_seed(0)
    mat = lambda n, k: torch.randn(n, k, device=dev) / k ** 0.5           # noqa: E731
    vec = lambda n: torch.randn(n, device=dev) * 0.1                      # noqa: E731
    ln = lambda: (1 + 0.1 * torch.randn(E, device=dev), vec(E))           # noqa: E731
    x, resid, kv = torch.randn(R, E, device=dev), torch.randn(R, E, device=dev), torch.randn(LK, 2 * E, device=dev)
    valid = torch.ones(LK, dtype=torch.uint8, device=dev)
    state = torch.tensor([12345], dtype=torch.int64, device=dev)
    site = lambda i: (state, i, P, 3, 0)                                  # noqa: E731
    a = dict(wa=mat(E, E), ba=vec(E), ln1=ln(), wg=mat(E, E), bg=vec(E), rng_a=site(1))
    b = dict(wa=mat(E, E), ba=vec(E), ln1=ln(), ffn=(mat(FF, E), vec(FF), mat(E, FF), vec(E)), ln2=ln(), wg=mat(3 * E, E), bg=vec(3 * E),
             rng_a=site(3), rng_f=site(4), rng_3=site(5))
    t0, _, q0 = K.rowchain_fwd(x, resid=resid, **a)

    def three():
        t, _, q = K.rowchain_fwd(x, resid=resid, **a)
        o, _ = K.attention_fwd(q, kv[:, :E], kv[:, E:], H, valid, rng=site(2))
        return K.rowchain_fwd(o, resid=t, **b)

    def two():
        o, _ = K.attention_fwd(q0, kv[:, :E], kv[:, E:], H, valid, rng=site(2))
        return K.rowchain_fwd(o, resid=t0, **b)

    chain_a = (a["wa"], a["ba"], *a["ln1"], a["wg"], a["bg"])
    fns = {"A+CA+B: three launches": three,
           "A+CA+B: one launch": lambda: K.rowchain_attn_fwd(x, resid, kv[:, :E], kv[:, E:], H, key_valid=valid, chain_a=chain_a, rng_a0=site(1),
                                                             rng_c=site(2), **b),
           "CA+B: two launches": two,
           "CA+B: one launch": lambda: K.rowchain_attn_fwd(q0, t0, kv[:, :E], kv[:, E:], H, key_valid=valid, rng_c=site(2), **b),
           "rowchain A alone": lambda: K.rowchain_fwd(x, resid=resid, **a),
           "attention alone": lambda: K.attention_fwd(q0, kv[:, :E], kv[:, E:], H, valid, rng=site(2)),
           "rowchain B alone": lambda: K.rowchain_fwd(x, resid=t0, **b)}
    res = {}
    for name, fn in fns.items():
        runs = sorted(timeit(fn, iters=50) for _ in range(rounds))
        res[name] = {"median": round(runs[len(runs) // 2], 2), "min": round(runs[0], 2), "max": round(runs[-1], 2)}
    return {"shape": {"rows": R, "E": E, "FF": FF, "heads": H, "keys": LK, "dropout": P},
            "unit": "us per repetition (hipGraph of 50 back-to-back repetitions)", "rounds": rounds, "us": res}


if __name__ == "__main__":
    a = sys.argv
    out = measure(int(a[a.index("--rounds") + 1]) if "--rounds" in a else 5)
    print(json.dumps(out))
    if "--out" in a:
        path = a[a.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
