"""What tests/test_gpu_range_geometry.py runs (tests/range_cases.py), pinned on the two case tables and the seeds alone: the
cover reaches every kernel form and every awkward size a ranged launch has to be right at, and every run's partitions have
the ranges the run is about.  A table row or a seed that loses one of these fails here, on the CPU, instead of the GPU
module silently checking less."""
import re

import numpy as np

import range_cases as R


def _lds(label):
    return int(re.search(r"lds=(\d+)", label).group(1))


def _needs():
    """name -> predicate over a fovea cover entry."""
    need = {}

    def form(key, start):
        return lambda e: e["key"] in key and e["label"].startswith(start)
    flex = ("flex_resize",)
    raw = ("flex_raw", "flex_mask")
    for k in ("fixed_resize", "fixed_raw", "fixed_mask"):
        need["fixed<GeomR> " + k] = form((k,), "fixed<GeomR>")
    for why in ("fov_h>32", "taps", "obs_w>256"):
        need["flexible2 why=" + why] = form(flex, "flexible2 why=" + why)
        need["flexible2 (raw / mask) why=" + why] = form(raw, "flexible2 why=" + why)
    need["generic as flexible"] = form(flex, "generic ")
    need["generic as flexible raw / mask"] = form(raw, "generic ")
    need["generic as peripheral"] = form(("peripheral",), "generic ")
    for mt in (4, 8, 12, 16):
        need[f"per3 mt={mt}"] = form(("peripheral",), f"per3 mt={mt} same=0")
    need["per3 same=1"] = lambda e: e["key"] == "peripheral" and e["label"].startswith("per3 ") and "same=1" in e["label"]
    need["peripheral2"] = form(("peripheral",), "peripheral2 ")
    need["frame not a multiple of 16 B"] = lambda e: R.arith_class(e["case"], e["key"])[0]
    need["obs_h != obs_w"] = lambda e: R.arith_class(e["case"], e["key"])[1]
    need["obs_w > 256"] = lambda e: R.arith_class(e["case"], e["key"])[2]
    # every entry also runs a ranged float32 context (the twin of a 16-bit run), so an odd f32 row is reached in any type
    need["f32 observation row not a multiple of 16 B"] = lambda e: R.arith_class(e["case"], e["key"])[3]
    need["16-bit observation row not a multiple of 16 B, run in a 16-bit type"] = lambda e: (
        R.arith_class(e["case"], e["key"])[4] and e["dtype"] != "float32")
    need["3 x 5 raw crop in a 16-bit type"] = lambda e: e["key"] == "fixed_raw" and e["case"]["fov"] == [3, 5] and e["dtype"] != "float32"
    need["21 x 19 raw crop in a 16-bit type"] = lambda e: e["key"] == "fixed_raw" and e["case"]["fov"] == [21, 19] and e["dtype"] != "float32"
    need["10 x 12 (120 B frames)"] = lambda e: e["case"]["obs"] == [10, 12]
    for key in ("fixed_resize", "fixed_raw", "fixed_mask", "flex_resize", "flex_raw", "flex_mask", "peripheral"):
        need[key + " in float32"] = lambda e, key=key: e["key"] == key and e["dtype"] == "float32"
        need[key + " in a 16-bit type"] = lambda e, key=key: e["key"] == key and e["dtype"] != "float32"
    return need


def cover_problems(geom):
    cover = R.fovea_cover(geom)
    bad = [name for name, pred in _needs().items() if not any(pred(e) for e in cover)]
    for fam, keys in (("flex3", ("flex_resize",)), ("raw3", ("flex_raw", "flex_mask"))):
        rsteps = {re.search(r"rstep=(\d+)", e["label"]).group(1) for e in cover if e["key"] in keys and e["label"].startswith(fam + " ")}
        if len(rsteps) < 6:
            bad.append(f"{fam} at six rstep values")
    built = [(c, k, v) for c in geom for k, v in c["plan"].items() if not v.startswith("refused")]
    c, k, v = max(built, key=lambda t: _lds(t[2]))
    if not any(e["case"] is c and e["key"] == k for e in cover):
        bad.append("the largest LDS case that builds")
    return bad


def test_fovea_cover_is_the_label_rule_plus_the_arithmetic_classes():
    cover = R.fovea_cover()
    built = [(k, R.plain_label(v)) for c in R.GEOM for k, v in c["plan"].items() if not v.startswith("refused")]
    assert len(built) == 141
    by_label = [e for e in cover if e["why"] == "label"]
    assert len(by_label) == len(set(built)) == 54
    assert {(e["key"], e["label"]) for e in by_label} == set(built)
    # first in table order: no earlier row carries the same (key, label)
    for e in by_label:
        first = next(c for c in R.GEOM if R.plain_label(c["plan"].get(e["key"], "")) == e["label"])
        assert first is e["case"], e["id"]
    assert len(cover) == 66 and len({e["id"] for e in cover}) == 66
    # types alternate in table order, except where a row that is odd in both sizes would have run in float32
    for i, e in enumerate(cover):
        odd = all(R.arith_class(e["case"], e["key"])[3:])
        assert e["dtype"] == R.DTYPES[i % 3] or (odd and i % 3 == 0 and e["dtype"] != "float32"), e["id"]
    assert all(e["n"] == (2 if e["case"]["obs"] == [256, 256] else 11) for e in cover)


def test_fovea_cover_reaches_every_form_and_every_awkward_size():
    assert cover_problems(R.GEOM) == []


def test_cover_condition_notices_a_lost_row():
    """Not vacuous: without the rows that carry a property, the condition names it."""
    for lost, name in (([10, 12], "frame not a multiple of 16 B"), ([8, 264], "obs_w > 256"), ([128, 128], "the largest LDS case that builds"),
                       ([12, 12], "raw3 at six rstep values")):
        rest = [c for c in R.GEOM if c["obs"] != lost]
        assert len(rest) < len(R.GEOM)
        assert name in cover_problems(rest), (lost, name)
    rest = [c for c in R.GEOM if not (c["obs"] == [64, 64] and c["aa"] == 1)]
    assert "per3 mt=12" in cover_problems(rest)


def test_full_cover_is_every_obs_size_of_the_fovea_cover():
    full = R.full_cover()
    assert [f["obs"] for f in full] == list(dict.fromkeys(tuple(e["case"]["obs"]) for e in R.fovea_cover()))
    assert {f["dtype"] for f in full} == set(R.DTYPES)
    assert any(f["obs"] == (10, 12) for f in full) and any(f["obs"][1] > 256 for f in full)


def test_ingest_cover_reaches_every_k1_plan():
    cover = R.ingest_cover()
    assert len({e["id"] for e in cover}) == len(cover)
    for c in R.INGEST:                                             # every row, layouts cycling in table order
        assert any(e["row"] is c and e["form"] in R.LAYOUTS for e in cover), c["obs"]
    assert [e["form"] for e in cover[:len(R.INGEST)]] == [R.LAYOUTS[i % 4] for i in range(len(R.INGEST))]
    plans = {c["plan"][lay] for c in R.INGEST for lay in R.LAYOUTS if c["plan"][lay].startswith("general ")}
    reached = {e["row"]["plan"][e["form"]] for e in cover if e["form"] != "small"}
    general = {p for p in reached if p.startswith("general ")}
    assert {R._field(p, "br") for p in general} == set(range(1, 13)) == {R._field(p, "br") for p in plans}
    assert {R._field(p, "partial") for p in general} == {0, 1}
    # every distinct general plan of the rgb layout (a row's layouts differ in the affine flag alone)
    assert {c["plan"]["rgb"].replace("affine=1", "affine=0") for c in R.INGEST if c["plan"]["rgb"].startswith("general ")} \
        <= {p.replace("affine=1", "affine=0") for p in general}
    assert any("affine=1" in p for p in general) and any("affine=0" in p for p in general)

    def four(pred):
        rows = [c for c in R.INGEST if pred(c)]
        return any(all(any(e["row"] is c and e["form"] == lay for e in cover) for lay in R.LAYOUTS) for c in rows)
    assert four(lambda c: c["plan"]["rgb"].startswith("band12 "))
    assert four(lambda c: c["obs"] < 210 and R._field(c["plan"]["rgb"], "partial") == 1 and R._field(c["plan"]["rgb"], "bands") > 1)
    assert four(lambda c: c["obs"] > 210)
    assert sorted(e["row"]["obs"] for e in cover if e["form"] == "small") == [12, 84, 264]
    assert {e["n"] for e in cover} == {2, 5, 300} and all(e["n"] == e["row"]["n"] for e in cover)


def _runs():
    for e in R.fovea_cover():
        yield R.node(R.T_FOVEA, e), e["n"], R.STEPS, True
    for e in R.full_cover():
        yield R.node(R.T_FULL, e), e["n"], R.INGEST_STEPS, False
    for e in R.ingest_cover():
        yield R.node(R.T_INGEST, e), e["n"], R.INGEST_STEPS, False


def test_every_run_walks_the_ranges_it_is_about():
    """Stated again, not through plan_problems: a range of one env, a range with odd lo, the range that ends at N - 1, unequal
    ranges, one step walked from the top down, the single range strictly inside the batch."""
    count = 0
    for name, N, steps, masked in _runs():
        plan = R.run_plan(name, N, steps, masked)
        assert R.plan_problems(plan, N) == [], name
        a, b = plan["parts"]
        assert (len(a), len(b)) == (min(3, N), min(5, N)), name
        for part in (a, b):
            los = [lo for lo, n in part]
            assert los[0] == 0 and all(lo + n == nxt for (lo, n), nxt in zip(part, los[1:] + [N])), name
            assert len(part) == N or len({n for lo, n in part}) > 1, name
        both = a + b
        assert any(n == 1 for lo, n in both) and any(lo % 2 for lo, n in both) and any(lo + n - 1 == N - 1 for lo, n in both), name
        walks = [plan["walk"](s) for s in range(steps)]
        assert sum(w == plan["parts"][s % 2][::-1] and len(w) > 1 for s, w in enumerate(walks)) == 1, name
        assert all(w == plan["parts"][s % 2] for s, w in enumerate(walks) if s != plan["descending"]), name
        if N >= 3:
            lo, n = plan["single"]
            assert 0 < lo and n >= 1 and lo + n < N, name
        if masked:
            for lo, n in plan["walk"](R.MASKED_STEP):
                if n >= 2:
                    assert 0 < int(plan["mask"][lo:lo + n].sum()) < n, (name, lo, n)
            assert sorted(plan["walk"](R.RESET_STEP)) != sorted(plan["walk"](R.MASKED_STEP))
        assert R.run_plan(name, N, steps, masked)["parts"] == plan["parts"]       # a function of the id alone
        count += 1
    assert count == 66 + 11 + len(R.ingest_cover())


def test_plan_condition_notices_a_bad_plan():
    name, N = R.node(R.T_FOVEA, R.fovea_cover()[0]), 11
    plan = R.run_plan(name, N)
    lo, n = next(r for r in plan["walk"](R.MASKED_STEP) if r[1] >= 2)
    plan["mask"] = plan["mask"].copy()
    plan["mask"][lo:lo + n] = 1
    assert any("masked step" in p for p in R.plan_problems(plan, N))
    plan = R.run_plan(name, N)
    plan["parts"] = [[(0, 4), (4, 4), (8, 3)], [(0, 2), (2, 2), (4, 2), (6, 2), (8, 3)]]
    bad = R.plan_problems(plan, N)
    assert "no range of exactly one env" in bad and "no range with odd lo" in bad
    plan["single"] = (0, 3)
    assert "the single range touches an end of the batch" in R.plan_problems(plan, N)
    plan["parts"][0] = [(0, 4), (4, 4), (8, 2)]
    assert "a partition does not cover [0, N) once" in R.plan_problems(plan, N)
    assert np.array_equal(R.run_plan(name, N)["mask"], R.run_plan(name, N)["mask"])
