"""The sweep of tests/test_gpu_history_geometry.py (tests/history_cases.py), checked on the table and the model alone - before any
GPU run: which code paths of the history readers the derived list reaches, that every case's seed gives the kinds of sample the
GPU module counts on, and - host_tables_harness carve - that the LDS regions k_history_memory (agx_k6_glimpse.h) touches end
inside what agx_plan.h's memory_lds sizes.  No GPU involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import history_cases as hc
from history_model import CLEAR, SKIP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIXED = [c for c in hc.SWEEP if c.kind == "fixed"]


def test_sweep_is_the_tables_fixed_rows_the_headline_geometry_and_full():
    ids = [hc.case_id(c) for c in hc.SWEEP]
    assert len(set(ids)) == len(ids)
    want = {(tuple(r["obs"]), tuple(r["fov"]), r["fs"], r["aa"], mode) for r in hc.TABLE for key, mode in hc.FIXED_KEYS.items()
            if key in r["plan"] and not r["plan"][key].startswith("refused")}
    want |= {hc.HEADLINE + (4, aa, mode) for aa in (0, 1) for mode in hc.FIXED_KEYS.values()}
    assert {(c.obs, c.fov, c.fs, c.aa, c.mode) for c in FIXED} == want and len(FIXED) == len(want)
    full = [c for c in hc.SWEEP if c.kind == "base"]
    assert sorted(c.obs for c in full) == sorted({c.obs for c in FIXED}) and all(c.mode == "full" for c in full)
    # the rows the history readers never read before: every one is in the sweep, in every mode the table builds
    for obs, fov, fs in (((64, 64), (21, 19), 3), ((96, 96), (50, 50), 1), ((128, 128), (31, 9), 1), ((120, 40), (30, 12), 3),
                         ((84, 84), (1, 1), 3), ((84, 84), (83, 83), 1), ((12, 12), (3, 5), 4)):
        assert {c.mode for c in FIXED if (c.obs, c.fov, c.fs) == (obs, fov, fs)} == {"resize", "raw", "mask"}, (obs, fov)
    assert {c.mode for c in FIXED if c.obs == (256, 256)} == {"raw", "mask"}


# what the sweep has to reach: name -> predicate over a fixed case
REACH = {
    "an odd fw (lds.raw + c is unaligned)": lambda c: c.fov[1] % 2 == 1,
    "fs = 1": lambda c: c.fs == 1,
    "fs >= 3": lambda c: c.fs >= 3,
    "ow > 256 (the striding phase C)": lambda c: c.obs[1] > hc.K_THREADS,
    "fh * ow / 4 > kWinRegs * 256 (window_tail runs)": lambda c: c.fov[0] * c.obs[1] // 4 > hc.K_WIN_REGS * hc.K_THREADS,
    "oh * ow % 16 != 0 (the dword push)": lambda c: c.obs[0] * c.obs[1] % 16 != 0,
    "oh - fh != ow - fw": lambda c: c.obs[0] - c.fov[0] != c.obs[1] - c.fov[1],
    "aa 0": lambda c: c.aa == 0,
    "aa 1": lambda c: c.aa == 1,
    "aa 0 at resize (the plain bilinear tap tables)": lambda c: c.aa == 0 and c.mode == "resize",
    "LDS >= 50 000 B": lambda c: hc.lds_bytes(c) >= 50000,
    "the compile-time geometry": lambda c: (c.obs, c.fov) == hc.HEADLINE and c.fs == 4,
}


@pytest.mark.parametrize("name", sorted(REACH))
def test_sweep_reaches(name):
    assert any(REACH[name](c) for c in FIXED), name


def test_reach_condition_notices_a_lost_row():
    """The condition is not vacuous: without the one geometry that carries a path, it fails."""
    for obs, name in (((8, 264), "ow > 256 (the striding phase C)"), ((10, 12), "oh * ow % 16 != 0 (the dword push)"),
                      ((256, 256), "LDS >= 50 000 B")):
        assert not any(REACH[name](c) for c in FIXED if c.obs != obs), name


@pytest.mark.parametrize("case", hc.SWEEP, ids=hc.case_id)
def test_seed_gives_every_kind_of_sample(case):
    """N = 3, T = fs + 2 (N = 2, T = fs + 3 at 256 x 256): at least 8 valid samples, a zero frame inside a valid stack (fs >= 2),
    an evicted sample, indices that wrap, CLEAR and SKIP."""
    seed = hc.seed_of(case)
    assert seed is not None, "no seed among the candidates satisfies the condition"
    N, T, steps = hc.shape_of_run(case)
    cmds = hc.commands(seed, N, steps)
    m, issued = hc.model_of(case, cmds)
    valid, zero, evicted = hc.kinds(case, m, issued)
    assert valid >= 8 and evicted >= 1 and int(m.count.min()) > T, (valid, evicted, m.count)
    assert zero >= 1 or case.fs == 1
    assert (cmds & SKIP).any() and (cmds & CLEAR).any()
    assert T == case.fs + (3 if N == 2 else 2) and N in (2, 3)


def test_replay_is_the_models_bookkeeping():
    """The NumPy re-derivation issues exactly the model's indices, and a zero-frame sample's stack starts with zero planes."""
    case = next(c for c in FIXED if c.fs == 4 and c.obs == (12, 12) and c.mode == "raw")
    seed = hc.seed_of(case)
    N, T, steps = hc.shape_of_run(case)
    m, issued = hc.model_of(case, hc.commands(seed, N, steps))
    seen = hc.replay(case, seed)
    assert sorted(seen) == sorted(issued)
    zero = [s for s in issued if m.valid(*s) and None in m.rows(*s)]
    assert zero
    for s in zero:
        stack, loc = seen[s]
        for j, row in enumerate(m.rows(*s)):
            assert (row is None) == (not stack[j].any())           # (a random 12 x 12 frame is not all zero)
        assert 0 <= loc[0] <= 12 - 3 and 0 <= loc[1] <= 12 - 5


def test_memory_lds_restatement_at_the_limit():
    """The numbers the GPU module's limit cases rest on: 256 / 200 mask-out fits at P = 3 and not at P = 4; 84 / 83 resize at P = 8."""
    big = next(c for c in FIXED if c.obs == (256, 256) and c.mode == "mask")
    assert hc.memory_lds(big, 3) == 128 + 3 * 51200 <= hc.K_MAX_LDS < hc.memory_lds(big, 4) == 128 + 4 * 51200
    wide = next(c for c in FIXED if c.fov == (83, 83) and c.mode == "resize")
    assert hc.memory_lds(wide, 8) == 128 + 8 * 6976 + 84 * 16 + 2 * 83 * 84 * 4 + 84 * 84 * 4 <= hc.K_MAX_LDS


# ---------------------------------------------------------------------------------------------- K6's carve, on the host
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("harness") / "host_tables_harness")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "host_tables_harness.cpp"),
                    "-o", out], check=True, capture_output=True, timeout=300)
    return out


@pytest.mark.parametrize("case", [c for c in FIXED if c.mode != "raw"], ids=hc.case_id)
def test_memory_lds_covers_the_carve_k6_touches(harness, case):
    """For P = 1, 3, 8: the end of the last region k_history_memory touches - from fixed_carve itself - is within memory_lds, every
    region the kernel reads as float4 / int4 starts on 16 bytes, and memory_lds is the restatement the GPU module decides by."""
    r = subprocess.run([harness, "carve", *map(str, (*case.obs, *case.fov)), case.mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert [ln.split()[0] for ln in lines] == ["P=1", "P=3", "P=8"], r.stdout
    for ln, P in zip(lines, (1, 3, 8)):
        f = dict(t.split("=") for t in ln.split())
        assert int(f["end"]) <= int(f["lds"]) and f["aligned"] == "1", ln
        assert int(f["lds"]) == hc.memory_lds(case, P), ln
        assert int(f["headline"]) == ((case.obs, case.fov) == hc.HEADLINE)
