"""The library names the kernel it runs: the host-only phnet_*_kernel queries (answered by the decision functions the launches
call) against the symbols recorded before the Python copies of the heuristics were deleted, and every tuning switch against the
name it must change.  No GPU: nothing here launches."""
import ctypes
import json
import os
import re

import pytest

from phnet_amd import _lib

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = json.load(open(os.path.join(GOLD, "gemm_symbols_default.json")))
CONV_ARGS = ("N", "Hi", "Wi", "Ci", "Co", "R", "S", "stride", "pad")


@pytest.fixture(scope="module")
def lib():
    from phnet_amd import build
    build.build(verbose=False)
    handle = _lib.lib()
    assert handle.phnet_tune_reset() == 0
    yield handle
    assert handle.phnet_tune_reset() == 0


def query(lib, op, a):
    """(name, splits or None) the library reports for one fixture entry / one (op, args) pair."""
    name, sp = ctypes.create_string_buffer(96), ctypes.c_int32(-1)
    conv = [a[k] for k in CONV_ARGS] if "N" in a and "Hi" in a else None
    if op in ("fwd", "dgrad"):
        rc = lib.phnet_conv2d_kernel(int(op == "dgrad"), *conv, a["ws_bytes"], name, len(name), ctypes.byref(sp))
    elif op in ("wgrad", "wgrad_dbias"):
        rc = lib.phnet_conv2d_wgrad_kernel(*conv, int(op == "wgrad_dbias"), a["ws_bytes"], name, len(name), ctypes.byref(sp))
    elif op in ("conv3p_fwd", "conv3p_dgrad"):
        rc = lib.phnet_conv3p_kernel(a["M"], a["Ca"], a["Nn"], a["ws_bytes"], name, len(name), ctypes.byref(sp))
    else:
        assert op in ("linear_bwd", "linear_bwd_relu"), op
        rc = lib.phnet_linear_bwd_kernel(a["M"], a["K"], a["N"], int(op == "linear_bwd_relu"), name, len(name))
        sp = None
    assert rc == 0, (op, a, rc)
    return name.value.decode(), None if sp is None else sp.value


def test_fixture_covers_the_issue_shape_list():
    ops = {e["op"] for e in FIXTURE["default"]}
    assert ops == {"fwd", "dgrad", "wgrad", "wgrad_dbias", "conv3p_fwd", "conv3p_dgrad", "linear_bwd", "linear_bwd_relu"}
    assert sum(e["op"] == "fwd" for e in FIXTURE["default"]) == 2 * 17 + 6 + 6       # bench_conv rows at 1 and 8 clips, stage entries, FPN
    measured = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "BENCH_r03.json")).read()      # holds all_gemm_kernels
    assert "conv_igemm_kernel<64, 64, false, 16, true, 3, 4, true>" in measured
    assert not [e for e in FIXTURE["mirror_was_wrong"] if e["name"] in measured]


def test_names_unchanged_on_the_default_path(lib):
    wrong = []
    for e in FIXTURE["default"]:
        name, splits = query(lib, e["op"], e["args"])
        if name != e["name"] or (e["op"] in ("fwd", "dgrad", "conv3p_fwd", "conv3p_dgrad") and splits != e["splits"]):
            wrong.append((e, name, splits))
    assert not wrong, wrong[:5]


def tile_of(name):
    """(bm, bn, k_tile) a forward kernel name stands for."""
    m = re.fullmatch(r"conv_igemm_kernel<(\d+), (\d+), false, (\d+), .*>", name)
    rows = re.fullmatch(r"linrows_kernel<false, ([12])>", name)
    if rows:
        return (160 * int(rows.group(1)), 128, 16)                               # linrows_kernel<false, W>: 160 W x 128 tile, 16-deep steps
    assert m or name == "conv3x3s1_kernel<false>", name
    return tuple(int(v) for v in m.groups()) if m else (64, 64, 16)               # conv3x3s1_kernel: 64 x 64 tile, 16-deep units


def test_plan_and_kernel_query_agree(lib):
    """phnet_conv2d_plan takes M x Co x K alone: it describes the Linear layer ([M,1,1,K] image, 1x1 filter) of that GEMM, and must
    agree with the kernel query of exactly that launch - tall tiles of linrows_kernel included.  A convolution of the same GEMM
    runs that tile and split count too, except where its Linear view is a tall-tile pick: there it shares the split count only."""
    differ = []
    for e in FIXTURE["default"]:
        if e["op"] != "fwd":
            continue
        a = e["args"]
        ho, wo = (a["Hi"] + 2 * a["pad"] - a["R"]) // a["stride"] + 1, (a["Wi"] + 2 * a["pad"] - a["S"]) // a["stride"] + 1
        gemm = (a["N"] * ho * wo, a["Co"], a["R"] * a["S"] * a["Ci"])
        bm, bn, sp, kt = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        assert lib.phnet_conv2d_plan(*gemm, a["ws_bytes"], ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(sp), ctypes.byref(kt)) == 0
        plan = (bm.value, bn.value, kt.value, sp.value)
        name, splits = query(lib, "fwd", a)
        linear = dict(N=gemm[0], Hi=1, Wi=1, Ci=gemm[2], Co=gemm[1], R=1, S=1, stride=1, pad=0, ws_bytes=a["ws_bytes"])
        lin_name, lin_splits = query(lib, "fwd", linear)
        assert plan == tile_of(lin_name) + (lin_splits,), (a, lin_name)
        assert sp.value == splits, (a, name)
        if lin_name.startswith("linrows_kernel<") and linear != a:
            differ.append(gemm)
        else:
            assert plan == tile_of(name) + (splits,), (a, name)
    # layer4's 3x3 convolutions at one clip (stride 1 and the stride-2 entry): as Linear layers, 1250 rows x 4608 | 2304 -> 512 take tall tiles
    assert differ == [(1250, 512, 4608), (1250, 512, 2304)], differ


def test_workspace_rule_reproduces_the_fixture():
    """hip_ops.splitk_workspace_bytes is the one statement of the split-K scratch size: it gives every ws_bytes the fixture records."""
    from phnet_amd.hip_ops import splitk_workspace_bytes
    seen = 0
    for e in FIXTURE["default"]:
        a = e["args"]
        if e["op"] in ("conv3p_fwd", "conv3p_dgrad"):
            m, cols = a["M"], a["Nn"]
        elif e["op"] == "fwd":
            ho, wo = (a["Hi"] + 2 * a["pad"] - a["R"]) // a["stride"] + 1, (a["Wi"] + 2 * a["pad"] - a["S"]) // a["stride"] + 1
            m, cols = a["N"] * ho * wo, a["Co"]
        elif e["op"] == "dgrad":
            m, cols = a["N"] * a["Hi"] * a["Wi"], a["Ci"]
        else:
            continue
        assert splitk_workspace_bytes(m, cols) == a["ws_bytes"], e
        seen += 1
    assert seen >= 2 * (2 * 17 + 6 + 6)


L1 = dict(N=5, Hi=80, Wi=200, Ci=64, Co=64, R=3, S=3, stride=1, pad=1, ws_bytes=163840000)          # layer1 3x3
L2 = dict(N=5, Hi=40, Wi=100, Ci=128, Co=128, R=3, S=3, stride=1, pad=1, ws_bytes=1 << 30)          # layer2 3x3: 128 channels, 20000 pixels
CLIPB = dict(N=1200, Hi=1, Wi=1, Ci=8192, Co=1024, R=1, S=1, stride=1, pad=0, ws_bytes=1 << 30)     # 1200 x 8192 x 1024 Linear
HYPER1 = dict(N=1200, Hi=1, Wi=1, Ci=1024, Co=8192, R=1, S=1, stride=1, pad=0, ws_bytes=0)         # 1200 x 1024 -> 8192: no scratch (>= 2^23 outputs)
HYPER2 = dict(N=1200, Hi=1, Wi=1, Ci=4608, Co=1024, R=1, S=1, stride=1, pad=0, ws_bytes=39321600)  # 1200 x 4608 -> 1024
HYPER1_D = dict(N=1200, Hi=1, Wi=1, Ci=1024, Co=8192, R=1, S=1, stride=1, pad=0, ws_bytes=39321600)  # its data gradient: 1200 x 8192 -> 1024
HEAD = dict(N=240, Hi=1, Wi=1, Ci=1024, Co=8192, R=1, S=1, stride=1, pad=0, ws_bytes=62914560)      # 240-row hyper-net Linear
TOWER = dict(N=240, Hi=1, Wi=1, Ci=64, Co=64, R=1, S=1, stride=1, pad=0, ws_bytes=1 << 20)            # 240-row tower Linear

# (setter, arguments, op, shape, name in the default tuning, what the switch must make of it)
SWITCHES = [
    ("phnet_tune_force_k_tile", (-5,), "fwd", L1, "conv3x3s1_kernel<false>",
     lambda n, s: n == "conv_igemm_kernel<64, 64, false, 16, true, 3, 4, true>"),
    ("phnet_tune_force_k_tile", (-5,), "dgrad", L1, "conv3x3s1_kernel<true>", lambda n, s: "conv3x3s1_kernel" not in n),
    ("phnet_tune_force_k_tile", (-1,), "fwd", L1, "conv3x3s1_kernel<false>",
     lambda n, s: n == "conv_igemm_kernel<64, 64, false, 16, false, 3, 4, false>"),
    ("phnet_tune_force_k_tile", (-102,), "fwd", L1, "conv3x3s1_kernel<false>",
     lambda n, s: n == "conv_igemm_kernel<64, 64, false, 16, true, 3, 2, true>"),
    ("phnet_tune_force_k_tile", (-200,), "fwd", L1, "conv3x3s1_kernel<false>",
     lambda n, s: n == "conv_igemm_kernel<64, 64, false, 16, true, 3, 4, false>"),
    ("phnet_tune_force_k_tile", (32,), "fwd", HEAD, "conv_igemm_kernel<64, 64, false, 64, true, 3, 4, true>",
     lambda n, s: n == "conv_igemm_kernel<64, 64, false, 32, true, 3, 4, true>"),
    ("phnet_tune_force_k_tile", (-32,), "fwd", HEAD, "conv_igemm_kernel<64, 64, false, 64, true, 3, 4, true>",
     lambda n, s: n == "conv_igemm_kernel<64, 64, false, 32, true, 3, 4, true>"),
    ("phnet_tune_wgrad", (1 | 8, 768), "wgrad", L1, "wgrad3s_kernel<2>", lambda n, s: n == "conv_wgrad_kernel<64, 64, 3, 16, 4, true>"),
    ("phnet_tune_wgrad", (1 | 32, 768), "wgrad", L1, "wgrad3s_kernel<2>", lambda n, s: n == "conv_wgrad3x3_kernel<4, 16>"),
    ("phnet_tune_wgrad", (1 | 32 | 16, 768), "wgrad", L1, "wgrad3s_kernel<2>", lambda n, s: n == "conv_wgrad3x3_kernel<4, 32>"),
    ("phnet_tune_wgrad", (1 | 64, 768), "wgrad", CLIPB, "wgrad1s_kernel", lambda n, s: n.startswith("conv_wgrad_kernel<")),
    ("phnet_tune_wgrad", (1 | 8 | 4, 768), "wgrad", L1, "wgrad3s_kernel<2>", lambda n, s: n == "conv_wgrad_kernel<64, 64, 3, 32, 2, true>"),
    ("phnet_tune_wgrad", (8, 768), "wgrad", L2, "wgrad3s_kernel<2>", lambda n, s: n == "conv_wgrad_kernel<64, 64, 3, 16, 4, true>"),
    ("phnet_tune_wgrad", (1 | 2, 768), "wgrad", TOWER, "linear_wgrad_smallp_kernel<64, 64, 0>", lambda n, s: n.startswith("conv_wgrad_kernel<")),
    ("phnet_tune_wgrad", (1, -64), "wgrad", L1, "wgrad3s_kernel<2>", lambda n, s: n == "wgrad3s_kernel<2>" and s == 21),
    ("phnet_tune_mma", (0,), "fwd", L1, "conv3x3s1_kernel<false>", lambda n, s: n == "conv_igemm_kernel<64, 64, false, 16, true, 0, 1, false>"),
    ("phnet_tune_mma", (0,), "wgrad", L1, "wgrad3s_kernel<2>", lambda n, s: n == "conv_wgrad_kernel<64, 64, 0, 16, 1, false>"),
    ("phnet_tune_mma", (1,), "linear_bwd", dict(M=240, K=64, N=64), "linear_bwd_fused_kernel<true, false, 0>",
     lambda n, s: n == "linear_bwd_fused_kernel<true, false, 1>"),
    ("phnet_tune_force_k_tile", (-1,), "linear_bwd", dict(M=240, K=64, N=64), "linear_bwd_fused_kernel<true, false, 0>",
     lambda n, s: n == "linear_bwd_fused_kernel<false, false, 0>"),
    ("phnet_tune_force_conv_tile", (128, 128, 2), "fwd", L1, "conv3x3s1_kernel<false>",
     lambda n, s: n == "conv_igemm_kernel<128, 128, false, 16, false, 3, 4, false>" and s == 2),
    ("phnet_tune_force_k_tile", (-300,), "fwd", HYPER1, "linrows_kernel<false, 2>",
     lambda n, s: n == "conv_igemm_kernel<64, 64, false, 16, true, 3, 4, true>" and s == 1),
    ("phnet_tune_force_k_tile", (-300,), "dgrad", HYPER1_D, "linrows_kernel<true, 1>",
     lambda n, s: n == "conv_igemm_kernel<64, 64, true, 16, true, 3, 4, true>" and s == 4),
    ("phnet_conv3p_tune", (-1,), "conv3p_fwd", dict(M=20000, Ca=128, Nn=128, ws_bytes=81920000), "conv3p_kernel<2>",
     lambda n, s: n == "conv3p_kernel<1>"),
    ("phnet_conv3p_tune", (64,), "conv3p_fwd", dict(M=1250, Ca=512, Nn=512, ws_bytes=20480000), "conv3p_kernel<1>",
     lambda n, s: n == "conv3p_kernel<1>" and s == 1),
]


@pytest.mark.parametrize("case", SWITCHES, ids=[f"{c[0]}{c[1]}-{c[2]}" for c in SWITCHES])
def test_switch_reaches_the_name(lib, case):
    setter, args, op, shape, default_name, effect = case
    default = query(lib, op, shape)
    assert default[0] == default_name
    assert getattr(lib, setter)(*args) == 0
    try:
        assert effect(*query(lib, op, shape)), query(lib, op, shape)
    finally:
        assert lib.phnet_tune_reset() == 0
    assert query(lib, op, shape) == default


def test_reset_and_mode_getter(lib):
    assert lib.phnet_tune_mma_get() == 3
    assert lib.phnet_tune_mma(2) == 0 and lib.phnet_tune_mma_get() == 2
    assert lib.phnet_tune_gate_wave(0) == 0 and lib.phnet_tune_dyn_mfma(0) == 0 and lib.phnet_tune_force_k_tile(16) == 0
    assert lib.phnet_tune_reset() == 0 and lib.phnet_tune_mma_get() == 3
    assert query(lib, "fwd", HEAD)[0] == "conv_igemm_kernel<64, 64, false, 64, true, 3, 4, true>"
    name = ctypes.create_string_buffer(8)                                   # a buffer too short for the name is an argument error
    assert lib.phnet_conv3p_kernel(20000, 128, 128, 0, name, len(name), ctypes.byref(ctypes.c_int32())) == -1


# the hyper-network's three launches with the frames of a clip batched: (shape, op, tall-tile kernel, splits)
LINROWS_PRODUCTION = [(HYPER1, "fwd", "linrows_kernel<false, 2>", 1), (HYPER1_D, "dgrad", "linrows_kernel<true, 1>", 4),
                      (HYPER2, "fwd", "linrows_kernel<false, 1>", 4)]


def test_linrows_dispatch(lib, monkeypatch):
    """The default tuning names the tall-tile kernel (csrc/linrows.hip) for the three production shapes with their split counts 1, 4, 4,
    given the scratch hip_ops hands them, and not for few rows, a depth that is no multiple of 16, another arithmetic or the switch
    off; hip_ops.linear_fwd's timer symbol flips with the switch.  Host-side queries only: nothing launches."""
    from phnet_amd import hip_ops as ops
    import torch

    def linear(m, k, n):
        return dict(N=m, Hi=1, Wi=1, Ci=k, Co=n, R=1, S=1, stride=1, pad=0, ws_bytes=ops.splitk_workspace_bytes(m, n))

    generic = {"fwd": "conv_igemm_kernel<64, 64, false, 16, true, 3, 4, true>", "dgrad": "conv_igemm_kernel<64, 64, true, 16, true, 3, 4, true>"}
    for shape, op, name, splits in LINROWS_PRODUCTION:
        cols = shape["Ci"] if op == "dgrad" else shape["Co"]
        assert shape["ws_bytes"] == ops.splitk_workspace_bytes(shape["N"], cols)
        assert query(lib, op, shape) == (name, splits)
    for few_or_ragged in (linear(240, 1024, 8192), linear(256, 1024, 8192), linear(1200, 1000, 8192)):
        assert query(lib, "fwd", few_or_ragged)[0].startswith("conv_igemm_kernel<"), few_or_ragged
    try:
        assert lib.phnet_tune_mma(0) == 0
        assert all(query(lib, op, shape)[0].startswith("conv_igemm_kernel<") for shape, op, _, _ in LINROWS_PRODUCTION)
        assert lib.phnet_tune_reset() == 0
        assert lib.phnet_tune_force_k_tile(-300) == 0
        assert all(query(lib, op, shape) == (generic[op], splits) for shape, op, _, splits in LINROWS_PRODUCTION)
        # what hip_ops.linear_fwd records for the timer with the switch off / on (the symbol query on meta tensors, not a launch)
        seen = []
        monkeypatch.setattr(ops, "_timed_launch", lambda sym_fn, flops, launch, **kw: seen.append(sym_fn()))
        monkeypatch.setattr(ops, "workspace", lambda nbytes, device, slot=0: None)
        monkeypatch.setattr(ops, "_req", lambda t, *a, **k: t)
        x, w = torch.empty(1200, 1024, device="meta"), torch.empty(8192, 1024, device="meta")
        ops.linear_fwd(x, w, None)
        assert lib.phnet_tune_force_k_tile(-301) == 0
        ops.linear_fwd(x, w, None)
        assert seen == [("conv_igemm_kernel<64, 64, false, 16, true, 3, 4, true>", 1), ("linrows_kernel<false, 2>", 1)], seen
    finally:
        assert lib.phnet_tune_reset() == 0
