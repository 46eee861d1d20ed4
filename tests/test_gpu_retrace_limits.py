"""GPU: the Retrace kernel (K16, include/agx_retrace.h) at its launch edges, on special floats and against the papers' form, on
the scenarios of tests/batch_limit_cases.py (tests/test_batch_limits_cpu.py pins what each holds).  `edges`: B = 1, 63, 64, 65,
257 by L = 7, 8, 9, 15, 16, 17 - every length of the short last register set around 8 and 16 -, B = 4097 (65 workgroups, one lane
in the last) and L = AGX_SEQUENCE_LIMIT.  `special`: +-0, subnormals, +-3.4e38, +-inf and NaN at steps WITH a row, so that a
flushing or contracted build differs.  Both compare every element with tests/retrace_model.py EXACTLY (int32 patterns, a NaN as
a NaN) between guard regions.  `definition` holds what the device wrote against the sum of TD errors in float64 within the bound
derived in batch_limit_cases' docstring, no step left out."""
import numpy as np
import pytest
import torch

import batch_limit_cases as bl
import retrace_model as rm
from retrace_model import bits
from test_gpu_retrace import Rig, _passed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    torch.cuda.synchronize()
    r.pipe.close()


def _equal(got, want, has, what):
    assert rm.same(got[0], want[0]), what
    assert not bits(got[0])[~has].any(), what                        # +0.0 where there is no row
    assert got[1] is None or (rm.same(got[1], want[1]) and not bits(got[1])[~has].any()), what
    assert got[2] is None or np.array_equal(got[2], want[2]), what
    return sum(g.size for g in got if g is not None)


@pytest.mark.parametrize("B", sorted({B for B, _ in bl.EDGES}))
def test_retrace_by_workgroups_and_register_sets(rig, B):
    """Every L of `edges` at this B, both layouts, the optional buffers rotating as in tests/test_gpu_retrace.py; NaN and inf at
    steps with a row in every other shape."""
    compared = 0
    for L in [L for b, L in bl.EDGES if b == B]:
        k = bl.edge(B, L)
        opt = _passed(B, L)
        want = rm.retrace(**(k if opt["boot"] else dict(k, boot=None)))
        has = rm.has_row(k["length"], k["steps"])
        assert np.array_equal(want[2], has.astype(np.uint8))
        for time_major in (False, True):
            compared += _equal(rig.call(k, time_major, **opt), want, has, (B, L, time_major, opt))
    print(f"B = {B}: {compared} target / td / valid elements compared")


def test_retrace_special_floats(rig):
    """`special` with both boot forms and both layouts: the device's outputs are NaN exactly where the model's are and bit-equal
    elsewhere, and each of them holds NaN, infinite, subnormal and negative-zero results - counted on what the device wrote."""
    k = bl.special()
    has = rm.has_row(k["length"], k["steps"])
    for boot in (True, False):
        want = rm.retrace(**(k if boot else dict(k, boot=None)))
        for time_major in (False, True):
            got = rig.call(k, time_major, boot=boot)
            _equal(got, want, has, ("special", boot, time_major))
            found = bl.kinds(got[0]), bl.kinds(got[1])
            assert all(found[0].values()) and all(found[1].values()), found
    print(f"special {bl.SPECIAL_SHAPE}: target {found[0]}, td {found[1]}")


@pytest.mark.parametrize("B,L", bl.DEFINITION_SHAPES)
def test_device_output_against_the_sum_of_td_errors_in_float64(rig, B, L):
    """What the device wrote at (257, 17), (65, 256) and (4097, 9), in both layouts and both boot forms, against the papers' form
    within the derived bound; no step is left out."""
    k = bl.plain(B, L)
    for boot in (True, False):
        d = bl.definition(B, L, boot)
        assert not d["left_out"].any()
        for time_major in (False, True):
            target, td, valid = rig.call(k, time_major, boot=boot)
            assert np.array_equal(valid != 0, d["has"]) and np.isfinite(target).all() and np.isfinite(td).all()
            worst = bl.worst_ratio(target, td, d)
            print(f"({B}, {L}), boot {boot}, time-major {time_major}: {int(d['has'].sum())} steps, worst error / bound: target {worst[0]:.3f}, td {worst[1]:.3f}")
            assert worst[0] <= 1.0 and worst[1] <= 1.0, (boot, time_major, worst)
