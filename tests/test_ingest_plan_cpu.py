"""The case table of tests/test_gpu_ingest_geometry.py (tests/golden/ingest_cases.json) pinned to the K1 ingest form each
obs_size selects, per screen layout.  agx_create picks the K1 form from obs_size alone (build_k1,
active-gym_amd/csrc/agx_host_tables.h; plan_k1, agx_plan.h); `host_tables_harness k1plan` reports that plan from the very
functions agx_create calls, `k1tables` the tables it uploads.  If band_rows or the band12 condition is retuned, a label here goes red and the
table has to be chosen again - instead of the GPU cases silently moving to another kernel.  The coverage test says what the
table as a whole has to reach; the exhaustive tests hold the tables of all 256 legal sizes against the oracle's OpenCV
restatement and re-derive every claim the plan makes (affine rows, band12 read bound, packed row pairs) in Python.
No GPU involved: hipcc compiles the harness as a plain host program."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CASES = json.load(open(os.path.join(REPO, "tests", "golden", "ingest_cases.json")))
LAYOUTS = ("rgb", "gray", "rgb-compact", "gray-compact")
SIZES = list(range(4, 1025, 4))            # agx_create: 4 <= obs <= 1024, obs_w % 4 == 0; agx_ingest: square
RAW_H, RAW_W = 210, 160


def case_name(c):
    return "o{}_fs{}_n{}".format(c["obs"], c["fs"], c["n"])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("harness") / "host_tables_harness")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "host_tables_harness.cpp"),
                    "-o", out], check=True, capture_output=True, timeout=300)
    return out


def _lines(harness, cmd, obs, *knobs):
    r = subprocess.run([harness, cmd, str(obs), *knobs], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [line.split(" ") for line in r.stdout.strip().splitlines()]


def k1plan(harness, obs, *knobs):
    """({layout: label}, {key: int} of the `affine` and `flags` lines) of `harness k1plan obs`, with the knobs ("no_full=1") set."""
    labels, facts = {}, {}
    for words in _lines(harness, "k1plan", obs, *knobs):
        if words[0] in LAYOUTS:
            assert words[1].startswith("form=")
            labels[words[0]] = " ".join(words[1:])[len("form="):]
        else:
            facts.update({k: int(v) for k, v in (w.split("=") for w in words[1:])})
    assert set(labels) == set(LAYOUTS)
    return labels, facts


def k1tables(harness, obs):
    return {w[0]: np.array(w[1:], dtype=np.int64) for w in _lines(harness, "k1tables", obs)}


@pytest.fixture(scope="module")
def plans(harness):
    return {o: k1plan(harness, o) for o in SIZES}


@pytest.fixture(scope="module")
def tables(harness):
    return {o: k1tables(harness, o) for o in SIZES}


def _field(label, key):
    m = re.search(r"\b%s=(\d+)" % key, label)
    return int(m.group(1)) if m else None


def test_case_table_is_well_formed():
    names = [case_name(c) for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert c["obs"] in SIZES and 1 <= c["fs"] <= 16, c
        assert set(c["plan"]) == set(LAYOUTS), c
        assert c["n"] == 300 or c["n"] == (2 if c["obs"] >= 512 else 5), c


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_case_selects_the_form_the_table_says(harness, case):
    labels, _ = k1plan(harness, case["obs"])
    assert labels == case["plan"], case_name(case)


# What the table has to reach: name -> predicate over (case, layout, label).
def _general(v, **want):
    return v.startswith("general ") and all(_field(v, k) == x for k, x in want.items())


def _coverage():
    need = {}
    for o in (48, 60, 72, 84):
        for lay in LAYOUTS:
            need["band12 at %d, %s" % (o, lay)] = lambda c, k, v, o=o, lay=lay: c["obs"] == o and k == lay and v.startswith("band12 ")
    need["obs % 12 == 0 but not affine: general kernel, full bands"] = lambda c, k, v: c["obs"] in (12, 24, 36) and _general(v, affine=0, partial=0)
    need["not affine with a partial last band, below 40"] = lambda c, k, v: c["obs"] < 40 and k == "rgb" and _general(v, affine=0, partial=1)
    need["size 4: one band, one column quad"] = lambda c, k, v: c["obs"] == 4 and _general(v, bands=1, partial=1)
    need["size 8: one band, rows < band_rows"] = lambda c, k, v: c["obs"] == 8 and _general(v, bands=1, partial=1)
    for br in range(12, 0, -1):
        need["band_rows %d, full last band" % br] = lambda c, k, v, br=br: _general(v, br=br, partial=0)
        if br not in NO_PARTIAL:
            need["band_rows %d, partial last band" % br] = lambda c, k, v, br=br: _general(v, br=br, partial=1)
    need["band_rows < 12 on whole screens with affine rows"] = lambda c, k, v: k in ("rgb", "gray") and _general(v, affine=1) and _field(v, "br") < 12
    need["compact screens at a size whose whole screens are affine"] = lambda c, k, v: (
        k.endswith("-compact") and _general(v, affine=0) and _general(c["plan"]["rgb"], affine=1))
    need["first x-clamped size, 160"] = lambda c, k, v: c["obs"] == 160 and _general(v, xclamp=1, yclamp=0)
    need["last size without an x clamp, 156"] = lambda c, k, v: c["obs"] == 156 and _general(v, xclamp=0)
    need["last affine size, 208"] = lambda c, k, v: c["obs"] == 208 and k == "rgb" and _general(v, affine=1, yclamp=0)
    need["first non-affine up-scale, 212"] = lambda c, k, v: c["obs"] == 212 and k == "rgb" and _general(v, affine=0, yclamp=1, xclamp=1)
    for o in (256, 260, 512, 516, 1024):
        need["size %d" % o] = lambda c, k, v, o=o: c["obs"] == o and _general(v)
    need["frame_stack 1"] = lambda c, k, v: c["fs"] == 1
    need["frame_stack 16"] = lambda c, k, v: c["fs"] == 16
    need["frame_stack 16 at a size with affine rows"] = lambda c, k, v: c["fs"] == 16 and k == "rgb" and _general(v, affine=1)
    need["N = 300 at a non-band12, non-affine size"] = lambda c, k, v: c["n"] == 300 and k == "rgb" and _general(v, affine=0)
    return need


# band_rows = 256 / (obs / 4) for obs >= 88.  band_rows 4 holds for 208 .. 256 (all multiples of 4), 2 for 344 .. 512 (all
# even) and every size is a multiple of 1: no legal size has a partial last band there
# (test_no_size_has_a_partial_last_band_at_band_rows_4_2_1 confirms it from the harness over all 256 sizes).
NO_PARTIAL = (4, 2, 1)


def missing_forms(cases):
    entries = [(c, k, v) for c in cases for k, v in c["plan"].items()]
    return [name for name, pred in _coverage().items() if not any(pred(*e) for e in entries)]


def test_table_reaches_every_k1_form():
    assert missing_forms(CASES) == []


def test_coverage_condition_notices_a_lost_form():
    """The coverage condition is not vacuous: without the only case that carries a form, it names that form."""
    for lost, name in ((160, "first x-clamped size, 160"), (92, "band_rows 11, partial last band"), (72, "band12 at 72, gray-compact"),
                       (28, "N = 300 at a non-band12, non-affine size"), (516, "size 516")):
        rest = [c for c in CASES if c["obs"] != lost]
        assert len(rest) == len(CASES) - 1
        assert name in missing_forms(rest), (lost, name)


def test_no_size_has_a_partial_last_band_at_band_rows_4_2_1(plans):
    seen = {}
    for o in SIZES:
        v = plans[o][0]["rgb"]
        if v.startswith("general "):
            seen.setdefault(_field(v, "br"), set()).add(_field(v, "partial"))
    assert set(seen) == set(range(1, 13))
    for br in range(1, 13):
        assert seen[br] == ({0} if br in NO_PARTIAL else {0, 1}), (br, seen[br])


def test_every_class_of_the_256_sizes_has_a_case(plans):
    """A class = the four labels without the band count.  Every class some legal size falls in is run on the GPU."""
    def cls(labels):
        return tuple(re.sub(r" bands=\d+", "", labels[k]) for k in LAYOUTS)
    have = {cls(c["plan"]) for c in CASES}
    lost = {}
    for o in SIZES:
        if cls(plans[o][0]) not in have:
            lost.setdefault(cls(plans[o][0]), []).append(o)
    assert lost == {}


def test_tables_equal_the_oracles_for_all_256_sizes(tables):
    for o in SIZES:
        t = tables[o]
        for key, want in zip(("x0", "x1", "a0", "a1"), O.cv_tables_x(RAW_W, o)):
            assert np.array_equal(t[key], want), (o, key)
        ty = O.cv_tables_y(RAW_H, o)
        for key, want in zip(("y0", "y1", "b0", "b1"), ty):
            assert np.array_equal(t[key], want), (o, key)
        rows = np.unique(np.concatenate([ty[0], ty[1]]))
        assert np.array_equal(t["rows"], rows), (o, "rows")
        # compact screens: the packed index of a source row is its position in the row list
        assert np.array_equal(rows[t["py0"]], ty[0]) and np.array_equal(rows[t["py1"]], ty[1]), (o, "packed rows")


def test_plan_claims_hold_for_all_256_sizes(plans, tables):
    """Every claim a plan makes, re-derived from the oracle's tables: the labels' fields, the affine row form, and for the
    band12 forms the adjacent taps, the LDS read bound and the packed row pairs."""
    n_affine = n_band12 = 0
    for o in SIZES:
        labels, f = plans[o]
        x0, x1, _, _ = (np.asarray(v, np.int64) for v in O.cv_tables_x(RAW_W, o))
        y0, y1, _, _ = (np.asarray(v, np.int64) for v in O.cv_tables_y(RAW_H, o))
        # what the band kernel can hold, not the header's formula: phase 2 gives every column quad of every row of the band
        # one of the 256 threads, phase 1 has 6 loader groups x 4 iterations = 24 row jobs for 2 frames x br rows; the plan
        # must take the tallest band both allow
        fits = [r for r in range(1, 257) if r * (o // 4) <= 256 and 2 * r <= 24]
        br = max(fits)
        assert fits and (br + 1) not in fits
        for lay in LAYOUTS:
            v = labels[lay]
            assert _field(v, "br") == br and _field(v, "bands") == -(-o // br), (o, lay, v)
            if v.startswith("general "):
                assert _field(v, "partial") == int(o % br != 0), (o, lay)
                assert _field(v, "xclamp") == int((x0 == x1).any()) and _field(v, "yclamp") == int((y0 == y1).any()), (o, lay)
                assert _field(v, "affine") == (0 if lay.endswith("-compact") else f["ok"]), (o, lay)
            else:
                assert v.startswith("band12 ") and br == 12 and o % 12 == 0, (o, lay)
                assert f["compact12_ok" if lay.endswith("-compact") else "band12_ok"], (o, lay)
        if f["ok"]:
            n_affine += 1
            dy = np.arange(o, dtype=np.int64)
            z = (dy * f["mul"] + f["add"]) >> f["shift"]
            assert (z >= 0).all() and np.array_equal(z, y0) and np.array_equal(np.minimum(z + 1, RAW_H - 1), y1), (o, "affine")
            assert f["mul"] < 1 << 24 and o < 1 << 24          # the kernel multiplies with v_mul_u32_u24
        assert f["adjacent"] == int((x1 == x0 + 1).all()), o
        pairs = np.array_equal(np.searchsorted(np.unique(np.concatenate([y0, y1])), y0), 2 * np.arange(o)) and (y1 == y0 + 1).all()
        assert f["pairs"] == int(pairs), o
        assert f["rows"] == len(np.unique(np.concatenate([y0, y1]))), o
        if f["band12_ok"] or f["compact12_ok"]:
            n_band12 += 1
            assert f["band12_ok"] and f["ok"] and f["adjacent"] and o % 12 == 0 and (o // 4) * 12 <= 256, o
            # the band12 workgroup's LDS (band12_lds, agx_plan.h; layout in agx_k1_ingest.h): ytab12[12] int2 | xtab12[ow] int2 |
            # gray u16 [2 frames][12 rows][top, bottom][160] | 8 bytes of slack.  Phase 2 reads two aligned dwords at byte
            # (2 x0) & ~3 of a gray row; for the last row of the last frame that read has to end inside the allocation.
            tabs, row_b = 8 * (12 + o), 2 * RAW_W
            gray_b = 2 * 12 * 2 * row_b
            lds = tabs + gray_b + 8
            last_row = tabs + gray_b - row_b
            assert (last_row + ((2 * x0) & ~3) + 8 <= lds).all(), o
            assert lds <= 64 * 1024
            assert f["compact12_ok"] == int(pairs), o
    assert n_affine == len([o for o in SIZES if 40 <= o <= 208]) and n_band12 == 4


def test_no_full_knob_leaves_no_band12_at_the_tables_sizes(harness, plans):
    """AGX_INGEST_NO_FULL (agx_plan.h: Knobs::no_full): the general band kernel at every size of the case table, in every
    layout, with the band height and band count the plan has without the knob."""
    band12 = 0
    for o in sorted({c["obs"] for c in CASES}):
        labels, facts = k1plan(harness, o, "no_full=1")
        assert facts == plans[o][1], o
        for lay in LAYOUTS:
            assert labels[lay].startswith("general "), (o, lay, labels[lay])
            want = plans[o][0][lay]
            assert (_field(labels[lay], "br"), _field(labels[lay], "bands")) == (_field(want, "br"), _field(want, "bands")), (o, lay)
            band12 += want.startswith("band12 ")
    assert band12 == 16
