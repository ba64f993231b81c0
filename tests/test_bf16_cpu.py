"""The "bf16" inference arithmetic (phnet_tune_mma(4)) on the host: the numpy rounding the GPU tests' reference is built on, the
mode switch, what the host-only queries name in the mode and after it, and the size of the one-plane packed image.  No GPU: nothing
here launches.  (Without mode 4 in the library every library test below fails at `phnet_tune_mma(4) == 0`.)"""
import ctypes

import numpy as np
import pytest
import torch

from phnet_amd import _lib
from tests import bf16_cases as C

WS = 1 << 30                 # "there is a workspace": the plans then split K where they would in production


@pytest.fixture(scope="module")
def lib():
    from phnet_amd import build
    build.build(verbose=False)
    handle = _lib.lib()
    assert handle.phnet_tune_reset() == 0
    yield handle
    assert handle.phnet_tune_reset() == 0


def conv_name(lib, dgrad, shape):
    n, hi, wi, ci, co, r, stride, pad = shape
    name, sp = ctypes.create_string_buffer(96), ctypes.c_int32(-1)
    rc = lib.phnet_conv2d_kernel(int(dgrad), n, hi, wi, ci, co, r, r, stride, pad, WS, name, len(name), ctypes.byref(sp))
    return rc, name.value.decode(), sp.value


def p3_name(lib, shape):
    """The packed-weight kernel's answer for a 3x3 / stride-1 / pad-1 shape it takes, else None."""
    n, hi, wi, ci, co, r, stride, pad = shape
    if not (r == 3 and stride == 1 and pad == 1 and lib.phnet_conv3p_applies(n * hi * wi, ci, co)):
        return None
    name, sp = ctypes.create_string_buffer(96), ctypes.c_int32(-1)
    rc = lib.phnet_conv3p_kernel(n * hi * wi, ci, co, WS, name, len(name), ctypes.byref(sp))
    return rc, name.value.decode(), sp.value


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _torch_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def test_round_bf16_is_torch_s_conversion_bit_for_bit():
    rng = np.random.default_rng(0)
    normals = (rng.standard_normal(1 << 20) * np.exp(rng.uniform(-20, 20, 1 << 20))).astype(np.float32)
    patterns = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    hi16 = rng.integers(0, 1 << 16, 4096, dtype=np.uint32) << np.uint32(16)
    ties = np.concatenate([(hi16 | np.uint32(0x8000)), (hi16 | np.uint32(0x7FFF)), (hi16 | np.uint32(0x8001))]).view(np.float32)
    subnormals = rng.integers(0, 1 << 23, 4096, dtype=np.uint32)
    subnormals = np.concatenate([subnormals, subnormals | np.uint32(0x80000000)]).view(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max,
                        np.finfo(np.float32).tiny, 1.0, 1.00390625, 1.01171875], np.float32)
    for what, a in (("normals", normals), ("bit patterns", patterns), ("ties", ties), ("subnormals", subnormals), ("special", special)):
        got, want = C.round_bf16(a), _torch_round(a)
        nan = np.isnan(a)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan), what        # NaNs stay NaN
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what
        assert not (_bits(got)[~nan] & np.uint32(0xFFFF)).any(), what                                  # a bf16 value: 16 low zeros
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF80FFFF, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(np.float32)
    assert np.isnan(C.round_bf16(nans)).all()
    assert C.round_bf16(np.zeros((2, 3), np.float32)).shape == (2, 3)


def test_mode_switch(lib):
    assert lib.phnet_tune_reset() == 0 and lib.phnet_tune_mma_get() == 3
    assert lib.phnet_tune_mma(4) == 0
    assert lib.phnet_tune_mma(5) == -1 and lib.phnet_tune_mma(-1) == -1          # PHNET_ERR_ARG, and the mode stays
    assert lib.phnet_tune_mma_get() == 4
    assert lib.phnet_tune_reset() == 0 and lib.phnet_tune_mma_get() == 3


def test_mma_context_restores_the_mode_after_a_raise(lib):
    from phnet_amd import hip_ops as K
    assert K.mma_mode() == 3
    with pytest.raises(KeyError):
        with K.mma("bf16"):
            assert K.mma_mode() == 4
            raise KeyError("inside")
    assert K.mma_mode() == 3
    K.set_mma_mode("f32")
    try:
        with K.mma("bf16"):
            assert K.mma_mode() == 4
        assert K.mma_mode() == 0                                                 # the PREVIOUS mode, not the default
        with pytest.raises(ValueError):
            with K.mma("fp16"):
                pass
        assert K.mma_mode() == 0
        K.set_mma_mode("bf16")
        assert K.mma_mode() == 4
    finally:
        K.tune_reset()
    assert K.mma_mode() == 3


MODE4 = ("conv_igemm_kernel<", "linrows_bf16_kernel<", "conv3p_bf16_kernel<")


def _is_mode4(name):
    if name.startswith("conv_igemm_kernel<"):
        return name[len("conv_igemm_kernel<"):-1].split(", ")[5] == "4"          # <bm, bn, dgrad, k tile, uni, MMA, pf, buf>
    return name.startswith(MODE4[1:])


def test_queries_name_mode_4_forward_kernels_and_no_backward(lib):
    shapes = C.query_shapes()
    assert len(shapes) > 60
    assert lib.phnet_tune_reset() == 0
    before = [(conv_name(lib, 0, s), conv_name(lib, 1, s) if s[6] <= 2 else None, p3_name(lib, s)) for s in shapes]
    assert all(b[0][0] == 0 and not _is_mode4(b[0][1]) for b in before)
    assert any(b[0][1].startswith("linrows_kernel<") for b in before) and any(b[0][1] == "conv3x3s1_kernel<false>" for b in before)
    assert sum(b[2] is not None for b in before) >= 12

    assert lib.phnet_tune_mma(4) == 0
    try:
        families = set()
        for s, b in zip(shapes, before):
            rc, name, splits = conv_name(lib, 0, s)
            assert rc == 0 and _is_mode4(name), (s, rc, name)
            assert splits == 1, (s, name, splits)                                # never split on its own: batch-invariant results
            families.add(name.split("<")[0])
            rc_d, name_d, _ = conv_name(lib, 1, s)
            assert rc_d == -1 and name_d == "", (s, rc_d, name_d)                # the backward query: PHNET_ERR_ARG
            p3 = p3_name(lib, s)
            assert (p3 is None) == (b[2] is None), s
            if p3 is not None:
                assert p3[0] == 0 and p3[1] == b[2][1].replace("conv3p_kernel<", "conv3p_bf16_kernel<") and p3[2] == 1, (s, p3, b[2])
                families.add(p3[1].split("<")[0])
        assert families == {"conv_igemm_kernel", "linrows_bf16_kernel", "conv3p_bf16_kernel"}, families
        # phnet_tune_force_k_tile(-401): mode 3's split plan back, count for count (the A/B switch of tests/tools/bench_precision.py)
        assert lib.phnet_tune_force_k_tile(-401) == 0
        assert any(b[0][2] > 1 for b in before) and any(b[2] is not None and b[2][2] > 1 for b in before)
        for s, b in zip(shapes, before):
            rc, name, splits = conv_name(lib, 0, s)
            assert rc == 0 and _is_mode4(name) and splits == b[0][2], (s, name, splits, b[0])
            if b[2] is not None:
                assert p3_name(lib, s)[2] == b[2][2], s
        assert lib.phnet_tune_force_k_tile(-400) == 0
        # the other backward queries
        name, sp = ctypes.create_string_buffer(96), ctypes.c_int32(-1)
        assert lib.phnet_conv2d_wgrad_kernel(5, 80, 200, 64, 64, 3, 3, 1, 1, 0, WS, name, len(name), ctypes.byref(sp)) == -1
        assert lib.phnet_linear_bwd_kernel(240, 64, 64, 0, name, len(name)) == -1
        # the plan query answers for the mode from the same decision: the tall tile of the 1200-row hyper-net layer
        bm, bn, spl, kt = (ctypes.c_int32() for _ in range(4))
        assert lib.phnet_conv2d_plan(1200, 8192, 1024, 0, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(spl), ctypes.byref(kt)) == 0
        assert (bm.value, bn.value, spl.value, kt.value) == (320, 128, 1, 16)
        assert conv_name(lib, 0, (1200, 1, 1, 1024, 8192, 1, 1, 0))[1] == "linrows_bf16_kernel<2>"
    finally:
        assert lib.phnet_tune_reset() == 0
    # ---- and the default mode afterwards names what it named before ----
    after = [(conv_name(lib, 0, s), conv_name(lib, 1, s) if s[6] <= 2 else None, p3_name(lib, s)) for s in shapes]
    assert after == before
    assert lib.phnet_conv2d_wgrad_kernel(5, 80, 200, 64, 64, 3, 3, 1, 1, 0, WS, name, len(name), ctypes.byref(sp)) == 0
    assert lib.phnet_linear_bwd_kernel(240, 64, 64, 0, name, len(name)) == 0


def test_every_tuning_switch_keeps_mode_4_in_mode_4(lib):
    """No forward launch runs silently in another arithmetic: whatever the tile, K-tile, ring, operand-path and kernel-family
    switches say, the forward query of mode 4 names a mode-4 instantiation (one that conv_bf16.hip / linrows.hip / conv3p.hip build)."""
    l1 = (5, 80, 200, 64, 64, 3, 1, 1)
    head = (240, 1, 1, 1024, 8192, 1, 1, 0)
    hyper = (1200, 1, 1, 1024, 8192, 1, 1, 0)
    stem = (5, 320, 800, 4, 64, 7, 2, 3)
    switches = [("phnet_tune_force_k_tile", a) for a in ((16,), (32,), (64,), (-1,), (-5,), (-32,), (-101,), (-102,), (-200,), (-300,), (-302,), (-401,))]
    switches += [("phnet_tune_force_conv_tile", a) for a in ((64, 64, 3), (128, 128, 2), (128, 64, 1), (64, 128, 4))]
    try:
        for setter, args in switches:
            assert lib.phnet_tune_reset() == 0 and lib.phnet_tune_mma(4) == 0
            assert getattr(lib, setter)(*args) == 0
            for s in (l1, head, hyper, stem):
                rc, name, _ = conv_name(lib, 0, s)
                assert rc == 0 and _is_mode4(name), (setter, args, s, name)
                if name.startswith("conv_igemm_kernel<"):
                    bm, bn, dg, kt, uni, mma, pf, buf = name[len("conv_igemm_kernel<"):-1].split(", ")
                    assert (bm, bn) in {("64", "64"), ("128", "128"), ("128", "64"), ("64", "128")} and dg == "false"
                    assert kt in ("16", "32", "64") and pf in ("1", "2", "4")
                    assert uni == "false" or (bm, bn) == ("64", "64")            # the uniform-tap variant exists for the 64 x 64 tile
                    assert buf == "false" or uni == "true"                       # and buffer loads only on it
    finally:
        assert lib.phnet_tune_reset() == 0


@pytest.mark.parametrize("co,ci", [(64, 64), (128, 128), (512, 512)])
def test_one_plane_image_is_a_third(lib, co, ci):
    assert 3 * lib.phnet_conv3p_packed_bytes_bf16(co, ci) == lib.phnet_conv3p_packed_bytes(co, ci)
    assert lib.phnet_conv3p_packed_bytes_bf16(co, ci) == 9 * co * ci * 2
    from phnet_amd import hip_ops as K
    assert K.conv3p_packed_bytes(co, ci, planes=1) * 3 == K.conv3p_packed_bytes(co, ci, planes=3)


def test_precision_names():
    from phnet_amd import hip_ops as K
    assert K.precision_mode("fp32") == "bf16x3" and K.precision_mode("bf16") == "bf16"
    with pytest.raises(ValueError):
        K.precision_mode("fp16")
    with pytest.raises(RuntimeError, match="bf16"):
        K.precision_mode("bf16", training=True)
