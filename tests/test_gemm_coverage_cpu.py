"""Census of the GEMM kernel tests, without a GPU: every kernel and split-K count tests/golden/gemm_symbols_default.json records
for production is launched by a shape some per-kernel test runs against fp64 - a row of tests/gemm_cases.py (run by
tests/test_gemm_coverage_gpu.py) or a shape of the lists of tests/test_kernels_gpu.py.  The picks are the library's own
host-only phnet_*_kernel queries in the default tuning; nothing here launches."""
import collections

import pytest

from phnet_amd import _lib
from tests import gemm_cases as G
from tests import test_kernels_gpu as KG
from tests.test_dispatch_cpu import FIXTURE, query

SPLIT_OPS = ("fwd", "dgrad", "conv3p_fwd", "conv3p_dgrad")           # the ops whose split count the fixture records


@pytest.fixture(scope="module")
def lib():
    from phnet_amd import build
    build.build(verbose=False)
    handle = _lib.lib()
    assert handle.phnet_tune_reset() == 0
    yield handle
    assert handle.phnet_tune_reset() == 0


def pick(lib, op, shape):
    return query(lib, op, G.query_args(lib, op, shape))


def existing_shapes():
    """(op, shape) of every launch the default-arithmetic per-kernel tests of tests/test_kernels_gpu.py make."""
    out = []
    for case in KG.CONV_CASES:                                       # test_conv_fwd_dgrad_wgrad_bf16x3
        out += [(op, case) for op in ("fwd", "dgrad", "wgrad", "wgrad_dbias")]
    for case in KG.CONV3P_CASES:                                     # test_packed_weight_3x3_kernel_vs_fp64
        out += [("conv3p_fwd", case), ("conv3p_dgrad", case), ("fwd", case + (3, 1, 1)), ("dgrad", case + (3, 1, 1))]
    for case in KG.WGRAD3_CASES:                                     # test_wgrad_three_taps_kernel_vs_fp64
        out += [("wgrad", case + (3, 1, 1)), ("wgrad_dbias", case + (3, 1, 1))]
    for p, ci, co in KG.WGRAD1S_CASES:                               # test_many_row_linear_weight_gradient_kernel_vs_fp64
        out += [("wgrad", (p, 1, 1, ci, co, 1, 1, 0)), ("wgrad_dbias", (p, 1, 1, ci, co, 1, 1, 0))]
    for case in KG.TAPS3_CASES:                                      # test_conv3x3_three_taps_forward_and_dgrad_vs_fp64
        out += [("fwd", case + (3, 1, 1)), ("dgrad", case + (3, 1, 1))]
    for case in KG.LINEAR_BWD_CASES:                                 # test_linear_backward_fused_launch
        out += [("linear_bwd", case), ("linear_bwd_relu", case)]
    return out


def reached(lib, rows=G.ROWS):
    """{(op, kernel): set of split counts} over the table rows and the existing lists."""
    got = collections.defaultdict(set)
    for op, shape in [(r.op, r.shape) for r in rows] + existing_shapes():
        name, splits = pick(lib, op, shape)
        got[(op, name)].add(splits)
    return got


def production(fixture=FIXTURE):
    want = collections.defaultdict(set)
    for e in fixture["default"]:
        want[(e["op"], e["name"])].add(e["splits"])
    return want


def missing(lib, rows=G.ROWS):
    """What production launches and no tested shape reaches: [(op, kernel)] and [(op, kernel, splits)]."""
    got, names, counts = reached(lib, rows), [], []
    for key, splits in sorted(production().items()):
        if key not in got:
            names.append(key)
        elif key[0] in SPLIT_OPS:
            counts += [key + (s,) for s in sorted(splits - got[key])]
    return names, counts


@pytest.mark.parametrize("row", G.ROWS, ids=G.row_id)
def test_row_gets_the_kernel_and_split_count_it_declares(lib, row):
    assert pick(lib, row.op, row.shape) == (row.kernel, row.splits)


def test_table_rows_are_distinct():
    assert len({(r.op, r.shape) for r in G.ROWS}) == len(G.ROWS)
    assert len({G.row_id(r) for r in G.ROWS}) == len(G.ROWS)


def test_every_production_kernel_and_split_count_is_reached(lib):
    names, counts = missing(lib)
    assert not names, names
    assert not counts, counts


def test_census_notices_a_lost_row(lib):
    """The table row that is the only cover of conv_igemm_kernel<128, 64, false, ...> (no list of test_kernels_gpu.py reaches a
    128-row tile in the default arithmetic), and the only one of 7 splits on the production 64x64 tile: without them the
    census must fail."""
    lost = [r for r in G.ROWS if r.kernel != G.T128X64]
    assert len(lost) == len(G.ROWS) - 1
    assert missing(lib, lost) == ([("fwd", G.T128X64)], [])
    lost = [r for r in G.ROWS if not (r.kernel == G.T64 and r.splits == 7)]
    assert len(lost) == len(G.ROWS) - 1
    assert missing(lib, lost) == ([], [("fwd", G.T64, 7)])


def test_table_holds_even_short_and_empty_last_splits():
    """Decided from the launch arithmetic, not from the row's label:
        launch_conv          ksteps = ceil(K / k_tile); a split takes k_per_split / k_tile = ceil(ksteps / splits) of them
        conv3x3s1 / conv3p   units = 3 * (channels / 16); a split takes units_per_split = ceil(units / splits)
        weight gradients     steps = ceil(P / pixels per step); a split takes ceil(steps / splits)
    and the last split gets what (splits - 1) full ones leave: as many (even), fewer (short) or none (empty)."""
    classes = collections.defaultdict(list)
    for row in G.ROWS:
        steps = G.reduction_steps(row)
        if steps is None or row.splits == 1:
            continue
        per_split = -(-steps // row.splits)
        begin_of_last = (row.splits - 1) * per_split
        kind = "empty" if begin_of_last >= steps else "short" if steps - begin_of_last < per_split else "even"
        assert kind == G.split_class(steps, row.splits)
        classes[kind].append(row)
        if row.reason in ("empty_split", "short_split"):                 # the label says what the arithmetic says
            assert row.reason == kind + "_split", (row, steps)
        else:
            assert kind != "empty", (row, steps)
    assert classes["even"] and classes["short"] and classes["empty"]
    # the issue's example: 240 x 1856 -> 2880 on 64-deep K tiles, 29 steps over 7 splits of 5: split 6 starts at k = 1920 > 1856
    head = next(r for r in G.ROWS if r.shape == (240, 1, 1, 1856, 2880, 1, 1, 0))
    assert G.reduction_steps(head) == 29 and head in classes["empty"] and 6 * 5 * 64 == 1920
    for op in ("fwd", "wgrad", "wgrad_dbias"):                           # an empty split in the forward plan and in the weight gradients
        assert any(r.op == op for r in classes["empty"]), op
    for kernel in G.WGRAD_PIXELS_PER_STEP:                               # every splitting weight-gradient kernel: a short or empty last split
        assert any(r.kernel == kernel for r in classes["short"] + classes["empty"]), kernel


def test_conv_cases_comments_name_the_kernels_they_reach(lib):
    """The case once commented '128x64 tile path' runs conv3x3s1_kernel since the picker changed; its comment says so now."""
    case = (1, 80, 200, 64, 64, 3, 1, 1)
    assert case in KG.CONV_CASES
    assert pick(lib, "fwd", case) == (G.TAPS3, 2) and pick(lib, "dgrad", case) == (G.TAPS3_D, 2)
    assert pick(lib, "wgrad", case) == (G.W3S, 85) and pick(lib, "wgrad_dbias", case) == (G.W3, 85)
