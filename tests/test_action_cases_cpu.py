"""tests/action_cases.py checked on the CPU, before any GPU run: the definition (next_state) against the oracle classes wherever the
oracle is defined, the value tables and the batch layout, and the form list against tests/golden/geometry_cases.json.  Where the
oracle is not defined (NaN, +-inf through astype(int), a float or out-of-range fov_res, an action_type that is neither 0 nor 1,
an out-of-range stored state) the test names the include/agx.h sentence the definition follows, so the document and the
definition cannot drift apart.  No GPU involved."""
import math
import os
import re

import numpy as np
import pytest

import action_cases as ac
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGX_H = re.sub(r"\s*\n\s*\*\s*", " ", open(os.path.join(REPO, "include", "agx.h")).read())
OBS, FOV = (12, 12), (3, 5)
SAS = [ac.REL_SAS, (-3e9, 3e9), (-math.inf, math.inf)]


def _fixed(mode, sas):
    return O.FixedFovealOracle(obs_size=OBS, fov_size=FOV, fov_init_loc=(2, 3), sensory_action_mode=mode, resize_to_full=False,
                               sensory_action_space=sas)


def _flex(mode, sas):
    return O.FlexibleFovealOracle(obs_size=OBS, fov_size=FOV, fov_init_loc=(2, 3), sensory_action_mode=mode, resize_to_full=False,
                                  sensory_action_space=sas)


def _oracle_defined(v, mode, sas):
    """np.rint(np.clip(..)).astype(int) is defined where the clipped value is finite and inside int64."""
    x = float(v)
    if x != x:
        return False
    lo, hi = (0.0, float(max(OBS))) if mode == "absolute" else sas
    return abs(min(max(x, lo), hi)) < 2.0 ** 62


@pytest.mark.parametrize("dtype", ac.DTYPES)
def test_next_state_is_the_oracles_update_loc_wherever_that_is_defined(dtype):
    """FixedFovealOracle.update_loc (clip_to_valid_fov, clip_to_valid_sas) from several stored locations, absolute and relative at
    the three action spaces the GPU module uses.  With sas = +-3e9 the oracle's int64 sum lands ON the bound (finding 3)."""
    seen = 0
    for mode, sas in [("absolute", None)] + [("relative", s) for s in SAS]:
        for start in ((2, 3), (0, 0), (9, 7)):
            for bound in (9, 7):
                for name, v in ac.table(dtype, bound):
                    if not _oracle_defined(v, mode, sas):
                        continue
                    for pair in ((v, ac.NP_DTYPE[dtype](ac.ORDINARY)), (ac.NP_DTYPE[dtype](ac.ORDINARY), v)):
                        orc = _fixed(mode, sas)
                        orc.fov_loc = np.array(start)
                        orc.update_loc(np.array(pair, ac.NP_DTYPE[dtype]))
                        got = ac.next_state("fixed", mode, sas, OBS, FOV, start, None, pair, dtype, 0, False)
                        assert got == ((int(orc.fov_loc[0]), int(orc.fov_loc[1])), None), (mode, sas, start, name, got, orc.fov_loc)
                        seen += 1
    assert seen >= 100
    if dtype == "f64":
        got = ac.next_state("fixed", "relative", (-3e9, 3e9), OBS, FOV, (2, 3), None, (1e300, -1e300), dtype, 0, False)
        assert got == ((9, 0), None)


@pytest.mark.parametrize("dtype", ac.DTYPES)
def test_next_state_is_the_flexible_oracles_step_wherever_that_is_defined(dtype):
    """FlexibleFovealOracle.step: FOV_LOC at several resolutions, and FOV_RES for the values the reference can use (integers in
    [1, obs], stored unclipped and unrounded, fov_env.py:323)."""
    loc_seen = res_seen = 0
    for mode, sas in (("absolute", None), ("relative", ac.REL_SAS)):
        for res in ((3, 5), (1, 12), (12, 1), (7, 7)):
            for start in ((0, 0), (4, 2)):
                start = tuple(min(start[i], OBS[i] - res[i]) for i in (0, 1))
                for name, v in ac.table(dtype, 9):
                    for pair in ((v, ac.NP_DTYPE[dtype](ac.ORDINARY)), (ac.NP_DTYPE[dtype](ac.ORDINARY), v)):
                        arr = np.array(pair, ac.NP_DTYPE[dtype])
                        if _oracle_defined(v, mode, sas):
                            orc = _flex(mode, sas)
                            orc.fov_loc, orc.fov_res = np.array(start), np.array(res)
                            orc.step(np.zeros((1,) + OBS), arr, np.array([0]))
                            got = ac.next_state("flexible", mode, sas, OBS, FOV, start, res, pair, dtype, 0, False)
                            assert got == (tuple(map(int, orc.fov_loc)), res), (mode, res, start, name, got)
                            loc_seen += 1
                        x = float(v)
                        if x == x and x == np.floor(x) and 1 <= x <= 12:
                            orc = _flex(mode, sas)
                            orc.fov_loc, orc.fov_res = np.array(start), np.array(res)
                            orc.step(np.zeros((1,) + OBS), arr, np.array([1]))
                            got = ac.next_state("flexible", mode, sas, OBS, FOV, start, res, pair, dtype, 1, False)
                            assert got == (tuple(map(int, orc.fov_loc)), tuple(int(t) for t in orc.fov_res)), (mode, res, start, name, got)
                            res_seen += 1
    assert loc_seen >= 100 and res_seen >= 8


def test_where_the_oracle_is_undefined_the_definition_follows_agx_h():
    nan = float("nan")
    # NaN: the lower bound of the clip it meets
    assert "a NaN action element goes to the LOWER bound of the clip it meets (0 for an absolute location, sas_lo for a relative delta, 1 for a resolution)" in AGX_H
    assert ac.next_state("fixed", "absolute", None, OBS, FOV, (4, 4), None, (nan, 5.0), "f64", 0, False) == ((0, 5), None)
    assert ac.next_state("fixed", "relative", ac.REL_SAS, OBS, FOV, (8, 4), None, (nan, 1.0), "f64", 0, False) == ((1, 5), None)
    assert ac.next_state("fixed", "relative", (-math.inf, math.inf), OBS, FOV, (8, 4), None, (nan, math.inf), "f64", 0, False) == ((0, 7), None)
    assert ac.next_state("flexible", "absolute", None, OBS, FOV, (8, 4), (3, 5), (nan, 2.0), "f64", 1, False) == ((8, 4), (1, 2))
    # a float or out-of-range fov_res: rint, then [1, obs]
    assert "this ABI rints float input and clamps to [1, obs]" in AGX_H
    assert ac.next_state("flexible", "absolute", None, OBS, FOV, (8, 4), (3, 5), (2.5, 12.5), "f64", 1, False) == ((8, 0), (2, 12))
    assert ac.next_state("flexible", "absolute", None, OBS, FOV, (8, 4), (3, 5), (3.5, -math.inf), "f32", 1, False) == ((8, 4), (4, 1))
    # no 32-bit limit on the relative sum
    assert "the relative sum fov_loc + delta is formed in double, without a 32-bit limit" in AGX_H
    assert ac.next_state("fixed", "relative", (-3e9, 3e9), OBS, FOV, (2, 3), None, (2.0 ** 31, -2.0 ** 31), "f32", 0, False) == ((9, 0), None)
    # an action_type that is neither 0 nor 1
    assert "Any value that is not AGX_FOV_RES acts as AGX_FOV_LOC" in AGX_H
    for t in (2, -1, 1 << 20):
        assert ac.next_state("flexible", "absolute", None, OBS, FOV, (8, 4), (3, 5), (4, 20), "i32", t, False) == ((4, 7), (3, 5))
    # the stored state is clamped as it is read: res, then loc; a masked env keeps it raw
    assert "fov_res to [1, obs] (flexible kind; the other kinds use fov_size), then fov_loc to [0, obs - fov_res]" in AGX_H
    assert "An env the call's mask leaves out keeps its stored state as it is" in AGX_H
    assert ac.next_state("fixed", "absolute", None, OBS, FOV, (-5, 52), None, None, "f32", 0, False) == ((0, 7), None)
    assert ac.next_state("fixed", "relative", ac.REL_SAS, OBS, FOV, (12, -3), None, (-1, 2), "i32", 0, False) == ((8, 2), None)
    assert ac.next_state("flexible", "absolute", None, OBS, FOV, (5, 5), (0, 21), None, "f32", 0, False) == ((5, 0), (1, 12))
    assert ac.next_state("flexible", "absolute", None, OBS, FOV, (5, 5), (12, 12), (1, 1), "i32", 1, False) == ((0, 0), (1, 1))
    assert ac.next_state("flexible", "absolute", None, OBS, FOV, (-5, 52), (0, 21), (1, 1), "i32", 1, True) == ((-5, 52), (0, 21))
    assert ac.next_state("fixed", "absolute", None, OBS, FOV, (-5, 52), None, (1, 1), "i32", 0, True) == ((-5, 52), None)


# every class of value a table must hold: name -> predicate over (float value, exact int value or None, bound)
F_CLASSES = {
    "+0": lambda x, b: x == 0 and not np.signbit(x), "-0": lambda x, b: x == 0 and np.signbit(x),
    "a subnormal of f32": lambda x, b: 0 < abs(x) < 2.0 ** -126, "the smallest normal of f32": lambda x, b: abs(x) == 2.0 ** -126,
    "the largest f32 below 0.5": lambda x, b: x == float(np.nextafter(np.float32(0.5), np.float32(0))),
    "tie down 0.5": lambda x, b: x == 0.5, "tie up 1.5": lambda x, b: x == 1.5, "tie down 2.5": lambda x, b: x == 2.5,
    "bound - 0.5": lambda x, b: x == b - 0.5, "bound": lambda x, b: x == b, "bound + 0.5": lambda x, b: x == b + 0.5,
    "just past bound + 0.5": lambda x, b: b + 0.5 < x < b + 0.51,
    "2^24 + 2": lambda x, b: x == 2.0 ** 24 + 2, "+2^31": lambda x, b: x == 2.0 ** 31, "-2^31": lambda x, b: x == -2.0 ** 31,
    "+huge finite": lambda x, b: 3e38 < x < math.inf, "-huge finite": lambda x, b: -math.inf < x < -3e38,
    "+inf": lambda x, b: x == math.inf, "-inf": lambda x, b: x == -math.inf,
    "NaN, sign clear": lambda x, b: x != x and not np.signbit(x), "NaN, sign set": lambda x, b: x != x and np.signbit(x),
}
F64_CLASSES = {
    "a subnormal of f64": lambda x, b: 0 < abs(x) < 2.0 ** -1022, "beyond f32, finite": lambda x, b: 3.5e38 < abs(x) < math.inf,
    "12.5 in f32, rounds to 13": lambda x, b: 12.5 < x < 12.6 and float(np.float32(x)) == 12.5,
    "13.5 in f32, rounds to 13": lambda x, b: 13.4 < x < 13.5 and float(np.float32(x)) == 13.5,
    "0.5 in f32, rounds to 1": lambda x, b: 0.5 < x < 0.6 and float(np.float32(x)) == 0.5,
    "1.5 in f32, rounds to 1": lambda x, b: 1.4 < x < 1.5 and float(np.float32(x)) == 1.5,
    "2^53 + 2": lambda x, b: x == 2.0 ** 53 + 2, "the largest f64 below 0.5": lambda x, b: x == float(np.nextafter(0.5, 0.0)),
}
I_CLASSES = {"INT_MIN": lambda v, b: v == -2 ** 31, "-1": lambda v, b: v == -1, "0": lambda v, b: v == 0, "1": lambda v, b: v == 1,
             "bound": lambda v, b: v == b, "bound + 1": lambda v, b: v == b + 1, "INT_MAX": lambda v, b: v == 2 ** 31 - 1}
I64_CLASSES = {"low dword 0": lambda v, b: v == 2 ** 32, "low dword 5": lambda v, b: v == 2 ** 32 + 5,
               "negative, low dword 3": lambda v, b: v == -2 ** 32 + 3, "no double holds it": lambda v, b: v == 2 ** 53 + 1,
               "INT64_MIN": lambda v, b: v == -2 ** 63, "INT64_MAX": lambda v, b: v == 2 ** 63 - 1}


@pytest.mark.parametrize("bound", [1, 7, 54, 164])
@pytest.mark.parametrize("dtype", ac.DTYPES)
def test_every_value_class_is_in_every_table(dtype, bound):
    t = ac.table(dtype, bound)
    assert len({n for n, _ in t}) == len(t) and all(n in ac.WHY for n, _ in t)
    assert all(type(v) is ac.NP_DTYPE[dtype] for _, v in t), "a value of the wrong element type"
    if dtype in ("f32", "f64"):
        classes = dict(F_CLASSES, **(F64_CLASSES if dtype == "f64" else {}))
        vals = [float(v) for _, v in t]
    else:
        classes = dict(I_CLASSES, **(I64_CLASSES if dtype == "i64" else {}))
        vals = [int(v) for _, v in t]
    for name, pred in classes.items():
        assert any(pred(v, bound) for v in vals), (dtype, bound, name)
    if dtype in ("f32", "f64"):
        # a NaN with a payload: not the canonical quiet NaN of either sign
        u = np.array([v for _, v in t]).view(np.uint32 if dtype == "f32" else np.uint64)
        quiet = {0x7FC00000, 0xFFC00000} if dtype == "f32" else {0x7FF8000000000000, 0xFFF8000000000000}
        assert any(np.isnan(v) and int(b) not in quiet for (_, v), b in zip(t, u))
    assert len(t) == {"f32": 24, "f64": 34, "i32": 7, "i64": 13}[dtype]


@pytest.mark.parametrize("dtype", ac.DTYPES)
def test_batch_puts_every_value_once_in_each_element_next_to_an_ordinary_partner(dtype):
    br, bc = 9, 7
    a, mask, names = ac.batch(dtype, br, bc)
    tr, tc = ac.table(dtype, br), ac.table(dtype, bc)
    L = len(tr)
    assert a.dtype == ac.NP_DTYPE[dtype] and a.shape == (2 * L + ac.MASKED, 2) and len(names) == len(a) <= 72
    bits = a.view({4: np.uint32, 8: np.uint64}[a.itemsize])
    for k in range(L):
        assert bits[2 * k, 0] == np.array([tr[k][1]]).view(bits.dtype)[0] and a[2 * k, 1] == ac.ORDINARY, names[2 * k]
        assert bits[2 * k + 1, 1] == np.array([tc[k][1]]).view(bits.dtype)[0] and a[2 * k + 1, 0] == ac.ORDINARY, names[2 * k + 1]
    assert mask[:2 * L].all() and not mask[2 * L:].any() and ac.MASKED >= 2
    # the masked envs carry values that would move the state if they were read
    for m in range(2 * L, len(a)):
        assert ac.next_state("fixed", "absolute", None, OBS, FOV, (2, 3), None, a[m], dtype, 0, False) != ((2, 3), None), names[m]
    assert 0 <= ac.ORDINARY <= min(min(f.obs[i] - f.fov[i] for i in (0, 1)) for f in ac.FORMS)


def test_mixed_types_give_every_env_both_branches_and_hold_all_four_values():
    t0, t1 = ac.mixed_types(67, 0), ac.mixed_types(67, 1)
    assert set(t0.tolist()) | set(t1.tolist()) == {0, 1, 2, -1}
    assert ((t0 == 1) != (t1 == 1)).all()
    assert {2, -1} <= set(t0.tolist()) and {2, -1} <= set(t1.tolist())


def test_forms_reach_every_kernel_family_of_the_geometry_table():
    assert ac.form_families() == ac.table_families()
    assert ac.table_families() == {"fixed<GeomR>", "per3", "peripheral2", "generic:peripheral", "flex3", "raw3", "flexible2",
                                   "generic:flexible", "packed=raw3", "packed=offsets+flexible2", "packed=offsets+generic"}
    names = [f.name for f in ac.FORMS]
    assert len(set(names)) == len(names)
    # every family in each output mode the table builds for the chosen row, and the entry points the table cannot name
    by = {(f.entry, f.key, f.label.split(" ", 1)[0]) for f in ac.FORMS}
    for key in ("fixed_resize", "fixed_raw", "fixed_mask"):
        assert ("fovea", key, "fixed<GeomS>") in by and ("fovea", key, "fixed<GeomR>") in by
    for key, fam in (("flex_resize", "flex3"), ("flex_raw", "raw3"), ("flex_mask", "raw3")):
        assert ("fovea", key, fam) in by
    for key in ("flex_resize", "flex_raw", "flex_mask"):
        assert ("fovea", key, "flexible2") in by and ("fovea", key, "generic") in by
    assert {f.entry for f in ac.FORMS} == {"fovea", "fovea_packed", "step_fixed", "step_flexible_packed", "history_observe"}
    # agx_step_flexible_packed: one geometry with the band12 ingest plan (the scan rides in the ingest launch: square, obs % 12 == 0,
    # tests/golden/ingest_cases.json) and one without (three launches)
    ingest = {r["obs"]: r["plan"]["rgb"] for r in __import__("json").load(open(os.path.join(REPO, "tests", "golden", "ingest_cases.json")))}
    steps = [f for f in ac.FORMS if f.entry == "step_flexible_packed"]
    assert sorted(ingest[f.obs[0]].split()[0] for f in steps) == ["band12", "general"]
    assert all(f.obs[0] == f.obs[1] and "packed=raw3" in f.label for f in steps)


def test_the_smallest_row_per_family_is_chosen():
    """Per family the form's frame is the smallest (obs_h * obs_w * fs) the table offers for that family and key."""
    for f in ac.FORMS:
        if f.label == "fixed<GeomS>" or f.entry != "fovea":
            continue
        kind = ac.MODES[f.key][0]
        fam = ac.family(kind, f.label)
        sizes = [r["obs"][0] * r["obs"][1] * r["fs"] for r in ac.TABLE
                 if f.key in r["plan"] and not r["plan"][f.key].startswith("refused") and ac.family(kind, r["plan"][f.key]) == fam]
        assert f.obs[0] * f.obs[1] * f.fs == min(sizes), (f.name, min(sizes))
