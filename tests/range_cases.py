"""The scenarios of tests/test_gpu_range_geometry.py, stated once: which geometries a ranged launch (agx_env_range) is run
at, in which observation type, and which partitions of [0, N) each run walks.  Everything here is a function of the two case
tables (tests/golden/geometry_cases.json, tests/golden/ingest_cases.json) and of the test ids, so a new table row extends the
cover and tests/test_range_cases_cpu.py can pin what the cover reaches without a device.  No torch, no GPU.

Fovea cover.  For every distinct (kind-mode key, plan label without " lds=N") that is not refused: the first case in table
order (54 runs).  A plan label does not see the arithmetic a ranged launch depends on - the fixed kinds have ONE label
(fixed<GeomR>) at every geometry - so the cover adds, per kind-mode key, the first case of every arithmetic class
(`arith_class`) the label rule has not reached (12 more runs: 10 x 12, whose frame is 120 B; the 3 x 5 raw crop at
frame_stack 3, 180 B / 90 B rows; 40 x 160 and 8 x 264 for the fixed kinds; ...).  `full` (agx_observe_full on a base
context) comes once per distinct obs size of that cover.  Observation types alternate float32 / bfloat16 / float16 over the
cover in table order; an entry whose rows are odd in both element sizes never takes float32 (every 16-bit run has a float32
twin, so its odd float32 rows are walked too).

Partitions.  A run's plan (`run_plan`) is drawn from a seed derived from the test id: two partitions of [0, N) with 3 and 5
ranges of unequal sizes, the step that is walked in descending order, the mask of the masked step, the subset fovea_reset
acts on, and one single range (lo, n) with 0 < lo and lo + n < N.  The draw is repeated until the conditions of
`plan_problems` hold, so they hold by construction; the CPU test states them once more over every id."""
import json
import os
import re
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GEOM = json.load(open(os.path.join(HERE, "golden", "geometry_cases.json")))
INGEST = json.load(open(os.path.join(HERE, "golden", "ingest_cases.json")))
DTYPES = ("float32", "bfloat16", "float16")
LAYOUTS = ("rgb", "gray", "rgb-compact", "gray-compact")
N_FOVEA = 11                       # envs of a fovea run
N_BIG_PLANE = 2                    # ... where one ring plane is 64 KiB or more (256 x 256)
STEPS = 4                          # fovea steps of a run; MASKED_STEP is the masked call, RESET_STEP starts with a ranged fovea_reset
MASKED_STEP, RESET_STEP = 2, 3
INGEST_STEPS = 2
# the test functions of tests/test_gpu_range_geometry.py: a run's seed is derived from "<function>[<param id>]"
T_FOVEA = "test_ranged_form_equals_whole_batch_and_oracle"
T_FULL = "test_ranged_observe_full"
T_INGEST = "test_ranged_ingest_equals_whole_batch_and_oracle"


def case_name(c):
    return "o{}x{}_f{}x{}_p{}x{}_aa{}".format(*c["obs"], *c["fov"], *c["per"], c["aa"])


def plain_label(v):
    """A plan label without its LDS bytes: the kernel form and what selects it."""
    return re.sub(r" lds=\d+", "", v)


def id_label(v):
    return re.sub(r"[^A-Za-z0-9.+]+", ".", plain_label(v).replace("<", "_").replace(">", "")).strip(".")


def obs_elems(c, key):
    """Elements of one env's observation row (agx_obs_shape): the fov-sized crop for a fixed fovea in raw mode, else full size."""
    (oh, ow), (fh, fw) = c["obs"], c["fov"]
    return c["fs"] * (fh * fw if key == "fixed_raw" else oh * ow)


def arith_class(c, key):
    """What the host arithmetic of a ranged launch depends on: (frame bytes % 16 != 0, obs_h != obs_w, obs_w > 256,
    f32 observation row bytes % 16 != 0, 16-bit observation row bytes % 16 != 0)."""
    oh, ow = c["obs"]
    el = obs_elems(c, key)
    return (oh * ow % 16 != 0, oh != ow, ow > 256, el * 4 % 16 != 0, el * 2 % 16 != 0)


def _built(geom):
    """(case index, key index, case, key, label) of every kind-mode of the table that builds, in table order."""
    return [(ci, ki, c, k, v) for ci, c in enumerate(geom) for ki, (k, v) in enumerate(c["plan"].items()) if not v.startswith("refused")]


def fovea_cover(geom=None):
    """The fovea runs, in table order: dicts of case, key, label, dtype, n, id, why ("label" | "arith")."""
    rows = _built(GEOM if geom is None else geom)
    picked, labels, classes = {}, set(), set()
    for ci, ki, c, k, v in rows:
        if (k, plain_label(v)) not in labels:
            labels.add((k, plain_label(v)))
            classes.add((k, arith_class(c, k)))
            picked[(ci, ki)] = "label"
    for ci, ki, c, k, v in rows:
        if (k, arith_class(c, k)) not in classes:
            classes.add((k, arith_class(c, k)))
            picked[(ci, ki)] = "arith"
    out = []
    for ci, ki, c, k, v in rows:
        if (ci, ki) in picked:
            dt = DTYPES[len(out) % 3]
            if dt == "float32" and all(arith_class(c, k)[3:]):
                dt = DTYPES[1 + len(out) % 2]      # rows that are odd in both element sizes run in a 16-bit type (and in f32 as its twin)
            n = N_BIG_PLANE if c["obs"][0] * c["obs"][1] >= 65536 else N_FOVEA
            out.append(dict(case=c, key=k, label=plain_label(v), plan=v, dtype=dt, n=n, why=picked[(ci, ki)],
                            id=f"{case_name(c)}-{k}-{id_label(v)}-{dt}"))
    return out


def full_cover(cover=None):
    """agx_observe_full on a base context: once per distinct obs size of the fovea cover, types cycling on."""
    cover = fovea_cover() if cover is None else cover
    out, seen = [], set()
    for e in cover:
        obs = tuple(e["case"]["obs"])
        if obs not in seen:
            seen.add(obs)
            dt = DTYPES[(len(cover) + len(out)) % 3]
            n = N_BIG_PLANE if obs[0] * obs[1] >= 65536 else N_FOVEA
            out.append(dict(obs=obs, fs=e["case"]["fs"], dtype=dt, n=n, id=f"o{obs[0]}x{obs[1]}_fs{e['case']['fs']}-full-{dt}"))
    return out


def _ingest_label(v):
    return re.sub(r"[^A-Za-z0-9]+", ".", v).strip(".")


def _field(label, name):
    m = re.search(r"\b%s=(\d+)" % name, label)
    return int(m.group(1)) if m else None


def ingest_cover(rows=None):
    """The ingest runs: every row of the table in one layout (cycling), all four layouts at the first band12 row, at the first
    down-scaling general row with several bands of which the last is partial, and at the first up-scaling row (obs > 210);
    agx_ingest_gray ("small") at 12, 84 and 264.  N is the row's own n."""
    rows = INGEST if rows is None else rows
    out, seen = [], set()

    def add(c, form):
        if (c["obs"], form) in seen:
            return
        seen.add((c["obs"], form))
        label = "small" if form == "small" else _ingest_label(c["plan"][form])
        out.append(dict(row=c, form=form, n=c["n"], id=f"o{c['obs']}_fs{c['fs']}_n{c['n']}-{form}-{label}"))

    for i, c in enumerate(rows):
        add(c, LAYOUTS[i % 4])
    band12 = next(c for c in rows if c["plan"]["rgb"].startswith("band12 "))
    partial = next(c for c in rows if c["plan"]["rgb"].startswith("general ") and c["obs"] < 210
                   and _field(c["plan"]["rgb"], "partial") == 1 and _field(c["plan"]["rgb"], "bands") > 1)
    up = next(c for c in rows if c["obs"] > 210)
    for c in (band12, partial, up):
        for lay in LAYOUTS:
            add(c, lay)
    for size in (12, 84, 264):
        add(next(c for c in rows if c["obs"] == size), "small")
    return out


# ---------------------------------------------------------------- partitions
def seed_of(node_name, *more):
    """The seed of a test from its id ("<function>[<param id>]"), as tests/test_gpu_geometry.py derives it."""
    return zlib.crc32("/".join([node_name, *map(str, more)]).encode())


def _partition(rng, N, parts):
    """`parts` ranges (lo, n) covering [0, N), ascending; their sizes are not all equal where that is possible."""
    parts = min(parts, N)
    while True:
        cuts = [0] + sorted(rng.choice(np.arange(1, N), parts - 1, replace=False).tolist()) + [N] if parts > 1 else [0, N]
        sizes = np.diff(cuts)
        if parts == N or parts == 1 or len(set(sizes.tolist())) > 1:
            return [(int(cuts[k]), int(sizes[k])) for k in range(parts)]


def plan_problems(plan, N):
    """What a plan lacks of the stated conditions (an empty list: nothing)."""
    bad = []
    ranges = plan["parts"][0] + plan["parts"][1]
    for part in plan["parts"]:
        if sorted(i for lo, n in part for i in range(lo, lo + n)) != list(range(N)):
            bad.append("a partition does not cover [0, N) once")
    if N > 1:
        if [len(p) for p in plan["parts"]] != [min(3, N), min(5, N)]:
            bad.append("not 3 and 5 ranges")
        for part in plan["parts"]:
            if 1 < len(part) < N and len({n for lo, n in part}) == 1:
                bad.append("equal ranges")
        if not any(n == 1 for lo, n in ranges):
            bad.append("no range of exactly one env")
        if not any(lo % 2 == 1 for lo, n in ranges):
            bad.append("no range with odd lo")
        if not any(lo + n == N and lo > 0 for lo, n in ranges):
            bad.append("no range that ends at N - 1")
    if not 0 <= plan["descending"] < plan["steps"]:
        bad.append("no step walked in descending order")
    if plan["mask"] is not None:
        for lo, n in plan["walk"](MASKED_STEP):
            if n >= 2 and len(set(plan["mask"][lo:lo + n].tolist())) != 2:
                bad.append(f"masked step: range ({lo}, {n}) is all masked or all unmasked")
    if plan["single"] is not None:
        lo, n = plan["single"]
        if not (0 < lo and n >= 1 and lo + n < N):
            bad.append("the single range touches an end of the batch")
    return bad


def run_plan(node_name, N, steps=STEPS, masked=True):
    """The plan of one run, drawn from the test id until `plan_problems` finds nothing.  parts: the two partitions; walk(step):
    the ranges of a step's walk in the order they are called (step s walks parts[s % 2]; step `descending` from the top
    down); mask: u8 [N] of the masked step (None without one); reset: u8 [N], the envs fovea_reset acts on, walked over
    parts[0]; single: (lo, n) of the single-range call (None where N < 3)."""
    rng = np.random.default_rng(seed_of(node_name, "plan"))
    for _ in range(100000):
        plan = dict(steps=steps, parts=[_partition(rng, N, 3), _partition(rng, N, 5)], descending=int(rng.integers(0, steps)),
                    mask=(rng.random(N) < 0.5).astype(np.uint8) if masked else None,
                    reset=(rng.random(N) < 0.4).astype(np.uint8), single=None)
        if N >= 3:
            lo = int(rng.integers(1, N - 1))
            plan["single"] = (lo, int(rng.integers(1, N - lo)))

        def walk(step, plan=plan):
            part = plan["parts"][step % 2]
            return part[::-1] if step == plan["descending"] else part
        plan["walk"] = walk
        if not plan_problems(plan, N):
            return plan
    raise AssertionError(f"{node_name}: no plan with the stated conditions at N = {N}")


def node(test, entry):
    return f"{test}[{entry['id']}]"
