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


def test_plan_and_kernel_query_agree(lib):
    for e in FIXTURE["default"]:
        if e["op"] != "fwd":
            continue
        a = e["args"]
        ho, wo = (a["Hi"] + 2 * a["pad"] - a["R"]) // a["stride"] + 1, (a["Wi"] + 2 * a["pad"] - a["S"]) // a["stride"] + 1
        bm, bn, sp, kt = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        assert lib.phnet_conv2d_plan(a["N"] * ho * wo, a["Co"], a["R"] * a["S"] * a["Ci"], a["ws_bytes"], ctypes.byref(bm), ctypes.byref(bn),
                                     ctypes.byref(sp), ctypes.byref(kt)) == 0
        name, splits = query(lib, "fwd", a)
        m = re.fullmatch(r"conv_igemm_kernel<(\d+), (\d+), false, (\d+), .*>", name)
        tile = tuple(int(v) for v in m.groups()) if m else (64, 64, 16)           # conv3x3s1_kernel: 64 x 64 tile, 16-deep units
        assert m or name == "conv3x3s1_kernel<false>"
        assert (bm.value, bn.value, kt.value, sp.value) == tile + (splits,), (a, name)


L1 = dict(N=5, Hi=80, Wi=200, Ci=64, Co=64, R=3, S=3, stride=1, pad=1, ws_bytes=163840000)          # layer1 3x3
L2 = dict(N=5, Hi=40, Wi=100, Ci=128, Co=128, R=3, S=3, stride=1, pad=1, ws_bytes=1 << 30)          # layer2 3x3: 128 channels, 20000 pixels
CLIPB = dict(N=1200, Hi=1, Wi=1, Ci=8192, Co=1024, R=1, S=1, stride=1, pad=0, ws_bytes=1 << 30)     # 1200 x 8192 x 1024 Linear
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
