"""The case table of tests/test_gpu_geometry.py (tests/golden/geometry_cases.json) pinned to the kernel form each case
selects.  agx_create picks a kernel form from the geometry (and the context's fallback knobs) alone and the launch code
switches on the stored plan; `host_tables_harness plan` prints that plan on the CPU from the very functions agx_create calls
(active-gym_amd/csrc/agx_plan.h over the table builders of agx_host_tables.h) - nothing is restated.  If a bucket, a tap
bound or an LDS bound is retuned, or the library's dispatch drifts, a label here goes red and the table has to be chosen
again - instead of the GPU cases silently moving to another kernel.  The coverage test says which forms the table as a whole
has to reach; the knob tests pin what the fallback comparisons of tests/test_gpu_parity.py assume a knob selects.
No GPU involved: hipcc compiles the harness as a plain host program."""
import json
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CASES = json.load(open(os.path.join(REPO, "tests", "golden", "geometry_cases.json")))
MODES = {"fixed_resize": ("fixed", "resize"), "fixed_raw": ("fixed", "raw"), "fixed_mask": ("fixed", "mask"),
         "flex_resize": ("flexible", "resize"), "flex_raw": ("flexible", "raw"), "flex_mask": ("flexible", "mask"),
         "peripheral": ("peripheral", "resize")}


def case_name(c):
    return "o{}x{}_f{}x{}_p{}x{}_aa{}".format(*c["obs"], *c["fov"], *c["per"], c["aa"])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("harness") / "host_tables_harness")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "host_tables_harness.cpp"),
                    "-o", out], check=True, capture_output=True, timeout=300)
    return out


def plan(harness, c, mode, *knobs):
    """{kind: label} of `harness plan` for the case's geometry in output mode `mode`, with the knobs ("generic=1", ...) set."""
    r = subprocess.run([harness, "plan", *map(str, (*c["obs"], *c["fov"], *c["per"], c["aa"], mode)), *knobs],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.strip().splitlines():
        kind, label = line.split(" ", 1)
        assert label.startswith("form=")
        out[kind] = label[len("form="):]
    return out


def test_case_ids_are_unique():
    names = [case_name(c) for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert set(c["plan"]) <= set(MODES) and c["plan"], c
        assert set(c["big"]) <= set(c["plan"]), c
        assert c["fs"] in (1, 3, 4), c


@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_case_selects_the_form_the_table_says(harness, case):
    for key, want in case["plan"].items():
        kind, mode = MODES[key]
        assert plan(harness, case, mode)[kind] == want, (case_name(case), key)


def _entries():
    """(case, aa, key, label) of every kind-mode of every case of the table."""
    return [(c, c["aa"], k, v) for c in CASES for k, v in c["plan"].items()]


def _buckets(label, axis):
    m = re.search(r"\b%s=([\d,]+)" % axis, label)
    return set(map(int, m.group(1).split(","))) if m else set()


def _rstep(label):
    return int(re.search(r"rstep=(\d+)", label).group(1))


def _flex3(k, v):
    return k == "flex_resize" and v.startswith("flex3 ")


def _raw3(k, v):
    return k in ("flex_raw", "flex_mask") and v.startswith("raw3 ")


def _fixed(k, v):
    return k.startswith("fixed_") and v.startswith("fixed<GeomR>")


# What the table has to reach: name -> predicate over (case, aa, key, label).  A name ending in "@aa0" / "@aa1" asks for
# the form at that antialias value.  The squeeze tables have more than 4 taps only with antialias on (a plain bilinear
# row has two), so per3 MT 8 / 12 / 16, k_fovea_peripheral2 by taps and the H bucket 8 exist at aa = 1 alone.
def _coverage():
    need = {}
    for aa in (0, 1):
        t = "@aa%d" % aa
        need["per3 MT 4" + t] = lambda c, a, k, v, aa=aa: a == aa and k == "peripheral" and v.startswith("per3 mt=4 same=0")
        need["per3 same=1" + t] = lambda c, a, k, v, aa=aa: a == aa and k == "peripheral" and v.startswith("per3 ") and "same=1" in v
        need["flex3 W bucket 16" + t] = lambda c, a, k, v, aa=aa: a == aa and _flex3(k, v) and 16 in _buckets(v, "W")
        need["flex3 W buckets {4} or {4,8} only" + t] = lambda c, a, k, v, aa=aa: a == aa and _flex3(k, v) and _buckets(v, "W") in ({4}, {4, 8})
        need["flex3 rstep 1" + t] = lambda c, a, k, v, aa=aa: a == aa and _flex3(k, v) and _rstep(v) == 1
        need["flex3 rstep >= 5" + t] = lambda c, a, k, v, aa=aa: a == aa and _flex3(k, v) and _rstep(v) >= 5
        need["raw3" + t] = lambda c, a, k, v, aa=aa: a == aa and k == "flex_raw" and _raw3(k, v) and "packed=raw3" in v
        need["raw3 mask" + t] = lambda c, a, k, v, aa=aa: a == aa and k == "flex_mask" and _raw3(k, v)
        need["k_fovea_flexible2 by fov_h > 32" + t] = lambda c, a, k, v, aa=aa: a == aa and k == "flex_resize" and v.startswith("flexible2 why=fov_h>32")
        need["k_fovea_flexible2 by tap overflow" + t] = lambda c, a, k, v, aa=aa: a == aa and k == "flex_resize" and v.startswith("flexible2 why=taps")
        need["packed form outside the raw3 plan" + t] = lambda c, a, k, v, aa=aa: a == aa and k == "flex_raw" and "packed=offsets+flexible2" in v
        need["k_fovea_generic (peripheral) by geometry" + t] = lambda c, a, k, v, aa=aa: a == aa and k == "peripheral" and v.startswith("generic ")
        need["k_fovea_fixed<GeomR>" + t] = lambda c, a, k, v, aa=aa: a == aa and _fixed(k, v)
    need["flex3 rstep 2"] = lambda c, a, k, v: _flex3(k, v) and _rstep(v) == 2
    need["per3 MT 8"] = lambda c, a, k, v: k == "peripheral" and v.startswith("per3 mt=8 ")
    need["per3 MT 12"] = lambda c, a, k, v: k == "peripheral" and v.startswith("per3 mt=12 ")
    need["per3 MT 16"] = lambda c, a, k, v: k == "peripheral" and v.startswith("per3 mt=16 ")
    need["k_fovea_peripheral2 by geometry"] = lambda c, a, k, v: k == "peripheral" and v.startswith("peripheral2 ")
    need["flex3 H bucket 8"] = lambda c, a, k, v: _flex3(k, v) and 8 in _buckets(v, "H")
    need["raw3 W bucket 16"] = lambda c, a, k, v: _raw3(k, v) and 16 in _buckets(v, "W")
    need["k_fovea_generic (flexible) by geometry"] = lambda c, a, k, v: k == "flex_resize" and v.startswith("generic ")
    need["k_fovea_generic (flexible raw, packed) by geometry"] = lambda c, a, k, v: k == "flex_raw" and "packed=offsets+generic" in v
    need["flexible obs_w > 256"] = lambda c, a, k, v: k == "flex_resize" and "why=obs_w>256" in v
    need["raw3 accepted where flex3 is refused"] = lambda c, a, k, v: (
        k == "flex_raw" and _raw3(k, v) and not c["plan"].get("flex_resize", "flex3 ").startswith("flex3 "))
    need["raw3 narrower W buckets than flex3"] = lambda c, a, k, v: (
        k == "flex_raw" and _raw3(k, v) and 16 not in _buckets(v, "W") and 16 in _buckets(c["plan"].get("flex_resize", ""), "W"))
    need["GeomR non-square obs"] = lambda c, a, k, v: _fixed(k, v) and c["obs"][0] != c["obs"][1]
    need["GeomR non-square fov"] = lambda c, a, k, v: _fixed(k, v) and c["fov"][0] != c["fov"][1]
    need["GeomR fov_w not a multiple of 4"] = lambda c, a, k, v: _fixed(k, v) and c["fov"][1] % 4 != 0
    need["GeomR fov 1x1"] = lambda c, a, k, v: _fixed(k, v) and c["fov"] == [1, 1]
    need["GeomR fov = obs - 1"] = lambda c, a, k, v: _fixed(k, v) and c["fov"] == [c["obs"][0] - 1, c["obs"][1] - 1]
    need["agx_create refuses for LDS"] = lambda c, a, k, v: v.startswith("refused lds=")
    # the full-size (N = 1024) runs the GPU module makes
    need["N=1024 k_fovea_fixed<GeomR>"] = lambda c, a, k, v: k in c["big"] and _fixed(k, v)
    need["N=1024 per3 MT 8"] = lambda c, a, k, v: k in c["big"] and v.startswith("per3 mt=8 ")
    need["N=1024 per3 MT 16"] = lambda c, a, k, v: k in c["big"] and v.startswith("per3 mt=16 ")
    need["N=1024 k_fovea_peripheral2"] = lambda c, a, k, v: k in c["big"] and v.startswith("peripheral2 ")
    need["N=1024 k_fovea_flexible2"] = lambda c, a, k, v: k in c["big"] and k == "flex_resize" and v.startswith("flexible2 ")
    return need


def missing_forms(cases):
    entries = [(c, c["aa"], k, v) for c in cases for k, v in c["plan"].items()]
    return [name for name, pred in _coverage().items() if not any(pred(*e) for e in entries)]


def test_table_reaches_every_kernel_form():
    assert missing_forms(CASES) == []


def test_coverage_condition_notices_a_lost_form():
    """The coverage condition is not vacuous: without the only case that carries a form, it names that form."""
    for lost, name in (("o84x84_f30x30_p12x12_aa1", "N=1024 per3 MT 16"), ("o40x120_f12x50_p30x100_aa1", "flex3 rstep 2"),
                       ("o100x100_f30x20_p30x30_aa1", "raw3 accepted where flex3 is refused")):
        rest = [c for c in CASES if case_name(c) != lost]
        assert len(rest) == len(CASES) - 1
        assert name in missing_forms(rest), (lost, name)


def test_every_form_has_one_case_with_the_16_bit_and_colour_checks():
    """One case per selected kernel form carries "extras" (16-bit pair + colour context in the GPU module).  A form is a
    kernel instantiation: the bucket sets and rstep are run-time values of one kernel."""
    def form(k, v):
        v = re.sub(r" lds=\d+", "", v)
        return k.split("_")[0] + ":" + " ".join(t for t in v.split() if not t.startswith(("rstep=", "why=", "same=0", "W=", "H=")))
    forms = {form(k, v) for c, a, k, v in _entries() if not v.startswith("refused")}
    with_extras = {form(k, v) for c, a, k, v in _entries() if c["extras"] and not v.startswith("refused")}
    assert forms - with_extras == set()


# ---- the fallback knobs (agx_plan.h: Knobs; AGX_FOVEA_GENERIC, AGX_FLEX_V2, AGX_PER_V2 in the library)
def _form(label):
    return label.split(" ", 1)[0]


def _with_knob(harness, knob):
    """(key, kind, label without a knob, label with it) of every entry of the case table."""
    out = []
    for c in CASES:
        got = {mode: plan(harness, c, mode, knob) for mode in {MODES[k][1] for k in c["plan"]}}
        for key, want in c["plan"].items():
            kind, mode = MODES[key]
            out.append((key, kind, want, got[mode][kind]))
    return out


def test_generic_knob_sends_every_flexible_and_peripheral_entry_to_the_generic_kernel(harness):
    seen = 0
    for key, kind, want, got in _with_knob(harness, "generic=1"):
        if kind == "fixed":
            assert got == want, key
        elif not got.startswith("refused"):
            assert _form(got) == "generic", (key, got)
            assert "packed=" not in got or got.endswith("packed=offsets+generic"), (key, got)
            seen += 1
    assert seen >= 20


def test_flex_v2_knob_leaves_no_composed_flexible_form(harness):
    seen = 0
    for key, kind, want, got in _with_knob(harness, "flex_v2=1"):
        if kind == "flexible":
            assert _form(got) not in ("flex3", "raw3") and "packed=raw3" not in got, (key, got)
            seen += _form(want) in ("flex3", "raw3")
        else:
            assert got == want, key
    assert seen >= 10


def test_per_v2_knob_leaves_no_per3(harness):
    seen = 0
    for key, kind, want, got in _with_knob(harness, "per_v2=1"):
        if kind == "peripheral":
            assert _form(got) != "per3", (key, got)
            seen += _form(want) == "per3"
        else:
            assert got == want, key
    assert seen >= 5
