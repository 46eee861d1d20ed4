"""CPU: include/agx_rollout.h (on-policy rollouts) <-> libagx.so's exports <-> active_gym/rollout.py; the refusals that need no
GPU; the rule and the GAE fold on hand-written cases (tests/rollout_model.py); the __host__ side of csrc/agx_rollout_math.h
(tests/rollout_harness.cpp), plain and under the host's sanitizers, against the model; and the seeds of the GPU cases on the
model alone."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rollout_model as rm
from steplog_model import F32, TERMINATED, TRUNCATED, bits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_rollout.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAMES = ["agx_rollout_gae", "agx_rollout_gather"]
CUT, BOOT = rm.CUT, rm.BOOT


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------------------------------------- surface
def test_header_declares_exactly_the_two_entry_points():
    src = open(HEADER).read()
    assert sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M))) == NAMES
    found = dict(re.findall(r"^#define\s+AGX_ROLLOUT_([A-Z_]+)\s+(\d+)\b", src, flags=re.M))
    assert found == {"LIMIT": "4096", "CUT": "4", "BOOT": "8"}
    from active_gym import rollout as ro
    assert ro.ROLLOUT_LIMIT == rm.ROLLOUT_LIMIT == 4096
    assert (ro.TERMINATED, ro.TRUNCATED, ro.CUT, ro.BOOT) == (TERMINATED, TRUNCATED, CUT, BOOT) == (1, 2, 4, 8)


def test_entry_points_are_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    for name in NAMES:
        assert hasattr(handle, name), name
    from active_gym import rollout as ro
    assert sorted(ro.SIGNATURES) == NAMES
    assert [len(ro.SIGNATURES[n][1]) for n in NAMES] == [12, 9]
    assert ro.SIGNATURES["agx_rollout_gae"][1][7:9] == [ctypes.c_float, ctypes.c_float]
    ro.lib()                                       # binds every signature: AttributeError if one is not exported
    import active_gym
    assert active_gym.Rollout is ro.Rollout


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_rollout.h") in deps
    for f in ("agx_k12_rollout.h", "agx_rollout_impl.h", "agx_rollout_math.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_headers_and_bindings_are_untouched():
    """Rollouts are additive: no older header names them, no older binding grew, the ABI version stays 2."""
    from active_gym import _native as nat
    from active_gym import sequence as sq
    from active_gym import steplog as sl
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):
        if hdr != "agx_rollout.h":
            assert "agx_rollout" not in open(os.path.join(REPO, "include", hdr)).read(), hdr
    assert [len(m.SIGNATURES) for m in (nat, sl, sq)] == [28, 6, 3]
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2


def test_a_null_handle_is_invalid_before_anything_else():
    """The handle is the first check of both entry points (N comes from it), so it is named whatever else is wrong."""
    from active_gym import _native as nat
    from active_gym import rollout as ro
    _build_mod().build()
    lib = ro.lib()
    buf = (ctypes.c_int64 * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for L, obs in ((4, ptr), (0, ptr), (4, None), (5000, None)):
        assert lib.agx_rollout_gather(None, L, None, obs, None, None, None, None, None) == nat.E_INVALID
        assert "agx_rollout_gather: null argument (log)" in nat.last_error(None)
        assert lib.agx_rollout_gae(None, L, ptr, ptr, ptr, ptr, None, 0.99, 0.95, obs, ptr, None) == nat.E_INVALID
        assert "agx_rollout_gae: null argument (h)" in nat.last_error(None)


def test_python_refusals_need_no_gpu():
    from active_gym import rollout as ro
    from active_gym.vector import AtariVecEnv
    assert ro.check_rollout_length(1) == 1 and ro.check_rollout_length(4096, 1024) == 4096
    for L in (0, 4097, -3):
        with pytest.raises(ValueError, match="L must be 1 .. 4096"):
            ro.check_rollout_length(L)
    with pytest.raises(ValueError, match="L \\* num_envs"):
        ro.check_rollout_length(4096, 1 << 20)
    assert ro.check_which("obs") == "obs" and ro.check_which("next") == "next"
    with pytest.raises(ValueError, match="which must be"):
        ro.check_which("prev")
    env = object.__new__(AtariVecEnv)              # (class defaults only: steplog is None)
    with pytest.raises(ValueError, match="rollout_batch needs a step log"):
        env.rollout_batch(8)
    with pytest.raises(ValueError, match="rollout_gae needs a step log"):
        env.rollout_gae({}, None, None)
    with pytest.raises(ValueError, match="L must be"):
        env.rollout_batch(0)

    class Closed:
        history, pipe, device, num_envs, payload_bytes = None, None, None, 4, 0

        def _live(self):
            raise RuntimeError("the step log or its history is closed")

    roll = ro.Rollout(Closed())
    with pytest.raises(RuntimeError, match="closed"):              # use after the log or its history is closed
        roll.gather(4)
    with pytest.raises(RuntimeError, match="closed"):
        roll.gae({}, None, None)
    with pytest.raises(ValueError, match="L must be"):
        roll.gather(0)                             # refused before anything is looked at
    with pytest.raises(ValueError, match="which must be"):
        roll.flat({}, "both")


# ---------------------------------------------------------------------------------------------- the rule, by hand
S, TE, TR, SI, SK, UN = rm.STEP, rm.TERM, rm.TRUNC, rm.SILENT, rm.SKIPPED, rm.UNREC
AUTORESET = [SI, S, S, TE, S, S]                   # rows 0 .. 6: 3 is the terminal observation, 4 the reset observation

# name: (kinds of one env, fs, T, the step the history is cleared in front of, L, the live slots newest first)
HAND = {
    "an autoreset step's two rows": (AUTORESET, 2, 8, None, 8, [(5, 6, BOOT), (4, 5, 0), (2, 3, TERMINATED), (1, 2, 0), (0, 1, 0)]),
    "L = 1": (AUTORESET, 2, 8, None, 1, [(5, 6, BOOT)]),
    "L > T": (AUTORESET, 2, 8, None, 20, [(5, 6, BOOT), (4, 5, 0), (2, 3, TERMINATED), (1, 2, 0), (0, 1, 0)]),
    "L cuts the rollout inside an episode": (AUTORESET, 2, 8, None, 3, [(5, 6, BOOT), (4, 5, 0), (2, 3, TERMINATED)]),
    "a double reset": ([SI, S, SI, SI, S], 2, 8, None, 8, [(3, 4, BOOT), (0, 1, CUT | BOOT)]),
    "an unrecorded row in the middle": ([SI, S, UN, S, S], 2, 8, None, 8, [(3, 4, BOOT), (2, 3, 0)]),
    # cnt = 12, T = 8: rows 4 .. 11 are retained, and observation 4 needs the evicted row 3
    "a wrapped history": ([SI] + [S] * 11, 2, 8, None, 8, [(10, 11, BOOT)] + [(j - 1, j, 0) for j in range(10, 5, -1)]),
    "a wrapped history, L below what is retained": ([SI] + [S] * 11, 2, 8, None, 4, [(10, 11, BOOT), (9, 10, 0), (8, 9, 0), (7, 8, 0)]),
    # after the clear the ages are unknown (255): observation 0's stack would reach in front of the history
    "a history after clear": ([SI, S, S, S, S, S, SI, S], 2, 8, 3, 8, [(3, 4, BOOT), (1, 2, CUT | BOOT)]),
    "a truncation with its reset": ([SI, S, TR, S], 2, 8, None, 8, [(3, 4, BOOT), (1, 2, TRUNCATED | BOOT), (0, 1, 0)]),
    "terminated at the newest slot": ([SI, S, TE], 2, 8, None, 8, [(1, 2, TERMINATED), (0, 1, 0)]),
    "a skipped env keeps its rows": ([SI, S, SK, SK, S], 2, 8, None, 8, [(1, 2, BOOT), (0, 1, 0)]),
    "nothing but a reset": ([SI], 2, 8, None, 4, []),
    "the newest row was never recorded": ([SI, S, S, UN], 2, 8, None, 4, []),
    # fs = 4, cnt = 9, T = 8: observation 3's stack reaches row 0, which is evicted, though observation 3 itself is retained
    "a deeper stack stops earlier": ([SI] + [S] * 8, 4, 8, None, 8, [(7, 8, BOOT), (6, 7, 0), (5, 6, 0), (4, 5, 0)]),
}


def _hand(name):
    kinds, fs, T, clear_at, L, want = HAND[name]
    hm, lm = rm.play(np.array(kinds, np.uint8)[:, None], fs, T, 4, 0, clear_at)
    return hm, lm, L, want


@pytest.mark.parametrize("name", sorted(HAND))
def test_rule_on_hand_written_cases(name):
    hm, lm, L, want = _hand(name)
    assert rm.rollout(lm, 0, L) == want
    out = rm.gather(lm, L)
    m = len(want)
    assert out["len"][0] == m
    assert out["obs_index"][:, 0].tolist() == [-1] * (L - m) + [s[0] for s in reversed(want)]
    assert out["next_index"][:, 0].tolist() == [-1] * (L - m) + [s[1] for s in reversed(want)]
    assert out["ends"][:, 0].tolist() == [0] * (L - m) + [s[2] for s in reversed(want)]
    assert not out["reward"][:L - m].any() and not out["payload"][:L - m].any()
    for t in range(L - m, L):                      # the row of next_index is the one the slot carries
        b = int(out["next_index"][t, 0])
        assert bits(out["reward"][t, 0]) == bits(lm.reward[b % hm.T, 0]) and np.array_equal(out["payload"][t, 0], lm.payload[b % hm.T, 0])


def test_the_hand_cases_hold_what_they_are_named_for():
    hm, lm, _, _ = _hand("an autoreset step's two rows")
    assert [int(hm.age[k, 0]) for k in range(7)] == [0, 1, 2, 3, 0, 1, 2] and int(lm.flags[3, 0]) == TERMINATED and int(lm.stamp[4, 0]) == -1
    hm, lm, _, _ = _hand("a wrapped history")
    assert int(hm.count[0]) == 12 > hm.T and hm.valid(0, 5) and not hm.valid(0, 4)
    hm, lm, _, _ = _hand("a history after clear")
    assert int(hm.count[0]) == 5 and [int(hm.age[k, 0]) for k in range(5)] == [255, 255, 255, 0, 1] and not hm.valid(0, 0) and hm.valid(0, 1)
    hm, lm, _, _ = _hand("an unrecorded row in the middle")
    assert lm.stamp[:5, 0].tolist() == [-1, 1, -1, 3, 4]


def test_chained_slots_share_their_observation():
    """Where a live slot t < L - 1 has none of the bits, next_index[t] == obs_index[t + 1] - over every case and L."""
    seen = 0
    for name in rm.CASES:
        _, hm, lm = rm.case_models(name)
        for L in rm.CASES[name][5]:
            out = rm.gather(lm, L)
            for n in range(hm.N):
                for t in range(L - int(out["len"][n]), L - 1):
                    if out["ends"][t, n] == 0:
                        assert out["next_index"][t, n] == out["obs_index"][t + 1, n], (name, L, n, t)
                        seen += 1
                    else:
                        assert out["ends"][t, n] & (TERMINATED | BOOT)
    assert seen > 100


# ---------------------------------------------------------------------------------------------- GAE, by hand
def _gae(ends, reward, value, boot, gamma, lam, length=None):
    col = lambda x, dt: np.asarray(x, dt)[:, None]
    L = len(ends)
    adv, ret = rm.gae(np.array([L if length is None else length], np.int32), col(reward, F32), col(ends, np.uint8), col(value, F32),
                      None if boot is None else col(boot, F32), gamma, lam)
    return adv[:, 0].tolist(), ret[:, 0].tolist()


R, V, B = [1.0, 2.0, 3.0], [0.5, 0.25, 0.125], [9.0, 9.0, 4.0]       # every figure below is exact in float32

# name: (ends, reward, value, boot, gamma, lambda, len, adv, ret)
GAE_HAND = {
    "lambda = 0": ([0, 0, BOOT], R, V, B, 0.5, 0.0, 3, [0.625, 1.8125, 4.875], [1.125, 2.0625, 5.0]),
    "lambda = 1, gamma = 1": ([0, 0, BOOT], R, V, B, 1.0, 1.0, 3, [9.5, 8.75, 6.875], [10.0, 9.0, 7.0]),
    "gamma = 1": ([0, 0, BOOT], R, V, B, 1.0, 0.5, 3, [0.75 + 0.5 * 5.3125, 1.875 + 0.5 * 6.875, 6.875], [0.75 + 0.5 * 5.3125 + 0.5, 5.5625, 7.0]),
    "terminated at the newest slot": ([0, 0, TERMINATED], R, V, B, 1.0, 1.0, 3, [5.5, 4.75, 2.875], [6.0, 5.0, 3.0]),
    # the value of slot 2 belongs to another episode: 1000 must not reach slot 1
    "truncated mid-rollout": ([0, TRUNCATED | BOOT, BOOT], R, [0.5, 0.25, 1000.0], [9.0, 2.0, 4.0], 1.0, 1.0, 3, [4.5, 3.75, -993.0], [5.0, 4.0, 7.0]),
    "cut mid-rollout": ([0, CUT | BOOT, BOOT], R, [0.5, 0.25, 1000.0], [9.0, 2.0, 4.0], 1.0, 1.0, 3, [4.5, 3.75, -993.0], [5.0, 4.0, 7.0]),
    "terminated mid-rollout": ([0, TERMINATED, BOOT], R, [0.5, 0.25, 1000.0], B, 1.0, 1.0, 3, [2.5, 1.75, -993.0], [3.0, 2.0, 7.0]),
    "padded slots are zero": ([0, 0, BOOT], R, V, B, 1.0, 1.0, 2, [0.0, 8.75, 6.875], [0.0, 9.0, 7.0]),
    "no boot buffer reads as zero": ([0, 0, TERMINATED], R, V, None, 1.0, 1.0, 3, [5.5, 4.75, 2.875], [6.0, 5.0, 3.0]),
}


@pytest.mark.parametrize("name", sorted(GAE_HAND))
def test_gae_on_hand_written_cases(name):
    ends, reward, value, boot, gamma, lam, length, adv, ret = GAE_HAND[name]
    assert _gae(ends, reward, value, boot, gamma, lam, length) == (adv, ret)


def test_gae_rounds_after_every_operation():
    """gamma * lambda, gamma * nv and gl * A are rounded to float32 before they are added: a fused or double-precision fold
    differs from the model on these figures."""
    gamma, lam = F32(0.99), F32(0.95)
    r, v, b = F32(0.1), F32(0.3), F32(0.7)
    adv, ret = _gae([0, BOOT], [r, r], [v, v], [b, b], gamma, lam)
    d1 = F32(F32(r + F32(gamma * b)) - v)
    d0 = F32(F32(r + F32(gamma * v)) - v)
    a0 = F32(d0 + F32(F32(gamma * lam) * d1))
    assert adv == [float(a0), float(d1)] and ret == [float(F32(a0 + v)), float(F32(d1 + v))]
    wide = float(r) + float(gamma) * float(v) - float(v) + float(gamma) * float(lam) * (float(r) + float(gamma) * float(b) - float(v))
    assert float(F32(wide)) != adv[0]              # the figures tell the two apart


# ---------------------------------------------------------------------------------------------- the harness
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "rollout_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "rollout_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "rollout_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


def _run(binary, tmp_path, tokens):
    path = tmp_path / "case.txt"
    path.write_text(" ".join(map(str, tokens)))
    r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]


def _harness_walk(binary, tmp_path, lm, L):
    """-> {n: [(obs_index, next_index, ends)] newest first}, with the slot numbers checked."""
    h = lm.h
    lines = _run(binary, tmp_path, [0, h.T, h.N, h.fs, L, *h.count.tolist(), *h.age.reshape(-1).tolist(), *lm.stamp.reshape(-1).tolist(),
                                    *lm.flags.reshape(-1).tolist()])
    out, at = {}, 0
    for n in range(h.N):
        assert lines[at][0] == n
        m = lines[at][1]
        rows = lines[at + 1:at + 1 + m]
        assert [r[0] for r in rows] == list(range(L - 1, L - 1 - m, -1))
        out[n] = [tuple(r[1:]) for r in rows]
        at += 1 + m
    assert at == len(lines)
    return out


def _harness_gae(binary, tmp_path, length, reward, ends, value, boot, gamma, lam):
    L, N = reward.shape
    tokens = [1, N, L, int(bits(gamma)), int(bits(lam)), int(boot is not None), *np.asarray(length).tolist(), *bits(reward).reshape(-1).tolist(),
              *ends.reshape(-1).tolist(), *bits(value).reshape(-1).tolist()]
    if boot is not None:
        tokens += bits(boot).reshape(-1).tolist()
    got = np.array(_run(binary, tmp_path, tokens), np.int64).astype(np.uint32).view(np.int32).reshape(L, N, 2)
    return got[..., 0], got[..., 1]


def _check_harness(binary, tmp_path):
    for name in sorted(HAND):
        hm, lm, L, want = _hand(name)
        assert _harness_walk(binary, tmp_path, lm, L) == {0: want}, name
    for name in sorted(GAE_HAND):
        ends, reward, value, boot, gamma, lam, length, adv, ret = GAE_HAND[name]
        col = lambda x, dt: np.asarray(x, dt)[:, None]
        ga, gr = _harness_gae(binary, tmp_path, [length], col(reward, F32), col(ends, np.uint8), col(value, F32),
                              None if boot is None else col(boot, F32), F32(gamma), F32(lam))
        assert ga[:, 0].tolist() == bits(adv).tolist() and gr[:, 0].tolist() == bits(ret).tolist(), name
    for name in sorted(rm.CASES):                  # the GPU cases, at every L they run and at the limit
        _, hm, lm = rm.case_models(name)
        for L in rm.CASES[name][5] + (4096,):
            assert _harness_walk(binary, tmp_path, lm, L) == {n: rm.rollout(lm, n, L) for n in range(hm.N)}, (name, L)
        for L in rm.CASES[name][5]:
            out = rm.gather(lm, L)
            value, boot = rm.gae_inputs(out, L)
            for gamma, lam in rm.GAMMA_LAMBDA:
                adv, ret = rm.gae(out["len"], out["reward"], out["ends"], value, boot, gamma, lam)
                ga, gr = _harness_gae(binary, tmp_path, out["len"], out["reward"], out["ends"], value, boot, F32(gamma), F32(lam))
                assert np.array_equal(ga, bits(adv)) and np.array_equal(gr, bits(ret)), (name, L, gamma, lam)
                assert np.isfinite(adv).all() and np.isfinite(ret).all()


def test_host_side_of_the_rule_and_the_fold(harness, tmp_path):
    _check_harness(harness, tmp_path)


def test_host_side_of_the_rule_and_the_fold_under_sanitizers(harness_san, tmp_path):
    _check_harness(harness_san, tmp_path)


# ---------------------------------------------------------------------------------------------- the GPU cases' seeds
def test_gpu_case_seeds_cover_every_kind_of_rollout():
    """On the model alone: over the cases of tests/test_gpu_rollout.py there is an env with len == L, one with 0 < len < L, one
    with len == 0, a skipped age-0 row between live slots, a CUT, a TRUNCATED, a TERMINATED, a BOOT at t < L - 1 and an env with
    cnt > T; the long case holds all but the empty env at each of its Ls above a wave, so that the chunked walk meets them."""
    seen = set()
    for name, case in rm.CASES.items():
        kind, hm, lm = rm.case_models(name)
        assert {rm.STEP, rm.TERM, rm.TRUNC, rm.SILENT, rm.SKIPPED, rm.UNREC} <= set(kind.reshape(-1).tolist()), name
        for L in case[5]:
            f = rm.features(lm, L)
            print(name, L, [len(rm.rollout(lm, n, L)) for n in range(hm.N)], sorted(f))
            seen |= f
            if name == "long" and L >= 64:
                assert f == rm.FEATURES - {"empty"}, (L, sorted(rm.FEATURES - f))
    assert seen == rm.FEATURES, sorted(rm.FEATURES - seen)
    assert rm.features(rm.case_models("small")[2], 5) == rm.FEATURES
    _, hm, lm = rm.case_models("cleared")
    assert hm.start_age == 254 and int(hm.count.max()) < hm.T and {"full", "partial", "empty"} <= rm.features(lm, 5)
    _, hm, lm = rm.case_models("long")
    lens = [len(rm.rollout(lm, n, 130)) for n in range(hm.N)]
    assert 130 in lens and any(64 < m < 130 for m in lens) and any(0 < m < 64 for m in lens)
