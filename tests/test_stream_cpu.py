"""Streaming inference, the part that needs no GPU: the slot arithmetic of the token ring, the argument validation of the three
entry points of csrc/stream.hip, and the resources the compiler gives their kernels."""
import collections
import os
import re
import subprocess

import pytest

from phnet_amd import _lib
from phnet_amd import build as hip_build
from phnet_amd.stream import window_order

ERR_ARG = -1


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.SO_PATH):
        hip_build.build()
    return _lib.lib()


@pytest.mark.parametrize("W", [1, 2, 8])
def test_window_order_equals_a_bounded_deque(W):
    """Frame i is pushed to physical slot i % W; what a stream remembers after n pushes is the deque(maxlen=W) of its frames, oldest
    first - the order phnet_stream_window emits."""
    fifo = collections.deque(maxlen=W)
    for n in range(0, 3 * W + 2):
        assert window_order(n, W) == [i % W for i in fifo], (n, W)
        assert len(window_order(n, W)) == min(n, W)
        fifo.append(n)                                     # frame n goes to slot n % W
    with pytest.raises(ValueError):
        window_order(-1, W)
    with pytest.raises(ValueError):
        window_order(3, 0)


def test_stream_entry_points_validate_without_a_gpu(built):
    """Null pointers, non-positive sizes and L >= N are PHNET_ERR_ARG before any launch (no device is touched: this runs on a
    machine without one).  Non-null pointers are made-up addresses - a call that got past the checks would try to launch."""
    lib = built
    p = 0x1000                                              # never dereferenced on the host
    S, B, W, N, E, L = 3, 2, 8, 240, 128, 4

    def window(ptrs=(p,) * 7, s=S, b=B, w=W, e=E, l=L):
        return lib.phnet_stream_window(*ptrs, s, b, w, e, l, None)

    def push(ptrs=(p,) * 6, s=S, b=B, w=W, n=N, e=E, l=L):
        return lib.phnet_stream_push(*ptrs, s, b, w, n, e, l, None)

    def select(ptrs=(p,) * 3, b=B, n=N, e=E):
        return lib.phnet_stream_select(*ptrs, b, n, e, None)

    for i in range(7):
        assert window(tuple(None if j == i else p for j in range(7))) == ERR_ARG, i
    for i in range(6):
        assert push(tuple(None if j == i else p for j in range(6))) == ERR_ARG, i
    for i in range(3):
        assert select(tuple(None if j == i else p for j in range(3))) == ERR_ARG, i
    for bad in (0, -1):
        for key in ("s", "b", "w", "e", "l"):
            assert window(**{key: bad}) == ERR_ARG, (key, bad)
        for key in ("s", "b", "w", "n", "e", "l"):
            assert push(**{key: bad}) == ERR_ARG, (key, bad)
        for key in ("b", "n", "e"):
            assert select(**{key: bad}) == ERR_ARG, (key, bad)
    assert push(n=4, l=4) == ERR_ARG and push(n=4, l=5) == ERR_ARG           # L >= N: no anchor left for the mean token
    assert window(e=126) == ERR_ARG and select(e=126) == ERR_ARG             # 16-byte moves: E % 4 == 0
    assert push(e=2048) == ERR_ARG                                           # one workgroup holds 1024 / E groups of E threads


def test_stream_kernels_compile_without_scratch_or_spills(tmp_path):
    """hipcc --offload-arch=gfx950 on csrc/stream.hip: no scratch, no spilled registers (the three kernels are latency-bound
    data movement; at this commit: push 19 VGPRs, window 10, select 8, all at 8 waves per SIMD)."""
    src = os.path.join(hip_build.CSRC, "stream.hip")
    out = subprocess.run([hip_build._hipcc(), *hip_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", str(tmp_path / "stream.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    assert {n for n in names if "stream_" in n} and len([n for n in names if "stream_" in n]) == 3, names
    for key in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        vals = [int(v) for v in re.findall(key + r": (\d+)", out.stderr)]
        assert len(vals) == 3 and not any(vals), (key, vals)
    print("VGPRs:", dict(zip(names, re.findall(r" VGPRs: (\d+)", out.stderr))))


def test_long_eval_fixture_has_a_memory_that_changes():
    """The 11-frame eval golden that tests/test_stream_gpu.py feeds through a stream (W = 8: the ring wraps) keeps lanes on some
    frames and none on others, so its cross-frame memory holds positive tokens, then loses them again."""
    from tests import fixtures
    kept = [int((row >= 0).sum()) for row in fixtures.load("tiny_long_eval_r18_64x160.npz")["eval_keep"]]
    assert len(kept) == 11 and kept[0] > 0 and 0 in kept[1:8] and any(kept[1:8]), kept
