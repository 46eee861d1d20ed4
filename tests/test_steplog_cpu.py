"""CPU: include/agx_steplog.h (the step log) <-> libagx.so's exports <-> active_gym/steplog.py; the argument checks that come before
any HIP call; the rules the GPU tests use (tests/steplog_model.py) on a hand-written case; and the __host__ side of
csrc/agx_steplog_fold.h (tests/steplog_harness.cpp) against the model, bit for bit."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import replay_model as rm
import steplog_model as sm
from history_model import CLEAR, HistoryModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_steplog.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAMES = ["agx_steplog_bytes", "agx_steplog_clear", "agx_steplog_create", "agx_steplog_destroy", "agx_steplog_gather", "agx_steplog_record"]
GAMMA = 0.99


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------------------------------------- surface
def test_header_declares_exactly_the_six_entry_points_and_four_defines():
    src = open(HEADER).read()
    assert sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M))) == NAMES
    found = dict(re.findall(r"^#define\s+(AGX_STEP\w+)\s+(\d+)\b", src, flags=re.M))
    assert found == {"AGX_STEPLOG_PAYLOAD_LIMIT": "64", "AGX_STEPLOG_NSTEP_LIMIT": "64", "AGX_STEP_TERMINATED": "1", "AGX_STEP_TRUNCATED": "2"}
    from active_gym import steplog as sl
    assert (sl.PAYLOAD_LIMIT, sl.NSTEP_LIMIT, sl.TERMINATED, sl.TRUNCATED) == (64, 64, 1, 2)
    assert (sm.TERMINATED, sm.TRUNCATED) == (1, 2)
    assert "agx_history_clear" in src and "k >= cnt - T" in src          # the two things the header has to say


def test_entry_points_are_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    for name in NAMES:
        assert hasattr(handle, name), name
    from active_gym import steplog as sl
    assert sorted(sl.SIGNATURES) == NAMES
    assert [len(sl.SIGNATURES[n][1]) for n in NAMES] == [1, 2, 3, 1, 13, 6]
    assert sl.SIGNATURES["agx_steplog_bytes"][0] is ctypes.c_int64
    assert sl.SIGNATURES["agx_steplog_gather"][1][5] is ctypes.c_float
    sl.lib()                                       # binds every signature: AttributeError if one is not exported
    import active_gym
    assert active_gym.StepLog is sl.StepLog


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_steplog.h") in deps
    for f in ("agx_k8_steplog.h", "agx_steplog_impl.h", "agx_steplog_fold.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_headers_and_bindings_are_untouched():
    from active_gym import _native as nat
    from active_gym import glimpse as gl
    from active_gym import history as hi
    from active_gym import native_hostout as nh
    from active_gym import native_loop as nl
    from active_gym import replay as rp
    for hdr in ("agx.h", "agx_loop.h", "agx_hostout.h", "agx_history.h", "agx_glimpse.h", "agx_replay.h"):
        assert "agx_steplog" not in open(os.path.join(REPO, "include", hdr)).read(), hdr
    for mod in (nat, nl, nh, hi, gl, rp):
        assert not [k for k in mod.SIGNATURES if "steplog" in k]
    assert (len(nat.SIGNATURES), len(nl.SIGNATURES), len(hi.SIGNATURES), len(gl.SIGNATURES), len(rp.SIGNATURES)) == (28, 6, 8, 1, 5)
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2


def test_null_and_out_of_range_arguments_are_invalid_before_any_hip_call():
    from active_gym import _native as nat
    from active_gym import steplog as sl
    _build_mod().build()
    lib = sl.lib()
    s = ctypes.c_void_p()
    assert lib.agx_steplog_create(None, 4, ctypes.byref(s)) == nat.E_INVALID and not s.value
    assert "null argument (h)" in nat.last_error(None)
    for w in (-4, 3, 6, 68, 1 << 20):
        assert lib.agx_steplog_create(None, w, ctypes.byref(s)) == nat.E_INVALID and not s.value
        assert "payload_bytes must be" in nat.last_error(None), w
    assert lib.agx_steplog_destroy(None) == nat.OK
    assert lib.agx_steplog_bytes(None) == nat.E_INVALID
    assert lib.agx_steplog_clear(None, None) == nat.E_INVALID and "agx_steplog_clear: null argument (s)" in nat.last_error(None)
    assert lib.agx_steplog_record(None, None, None, None, None, None) == nat.E_INVALID
    assert "agx_steplog_record: null argument (s)" in nat.last_error(None)
    gather = lambda B, nstep: lib.agx_steplog_gather(None, None, None, B, nstep, 0.99, None, None, None, None, None, None, None)  # noqa: E731
    for nstep in (0, -1, 65):
        assert gather(4, nstep) == nat.E_INVALID and "nstep must be" in nat.last_error(None), nstep
    assert gather(-1, 1) == nat.E_INVALID and "B must be" in nat.last_error(None)
    assert gather(4, 1) == nat.E_INVALID and "agx_steplog_gather: null argument (s)" in nat.last_error(None)
    assert gather(0, 64) == nat.E_INVALID                      # B = 0 is AGX_OK only on a log


def test_python_refusals_need_no_gpu():
    from active_gym import AtariVecEnv
    from active_gym import steplog as sl
    for w in (-4, 2, 66, 68):
        with pytest.raises(ValueError, match="payload_bytes"):
            sl.StepLog(None, payload_bytes=w)        # refused before the history is looked at
    assert [sl.check_payload_bytes(w) for w in (0, 4, 12, 64)] == [0, 4, 12, 64]
    for nstep in (0, -1, 65):
        with pytest.raises(ValueError, match="nstep"):
            sl.check_nstep(nstep)
        with pytest.raises(ValueError, match="nstep"):
            sl.StepLog.gather(None, None, None, nstep=nstep)
        with pytest.raises(ValueError, match="nstep"):
            sl.StepLog.batch(None, None, 4, nstep=nstep)
    assert sl.check_nstep(1) == 1 and sl.check_nstep(64) == 64
    for extra in ({}, {"history_len": 0}):
        args = types.SimpleNamespace(obs_size=(84, 84), frame_stack=4, action_repeat=4, obs_dtype="float32", step_log=True, **extra)
        with pytest.raises(ValueError, match="step_log"):
            AtariVecEnv(args, 2, kind="fixed")
    assert sl.check_env_step_log(False, 0) is False and sl.check_env_step_log(True, 8) is True
    assert sl.check_env_step_log(False, 8, discrete_motor=False) is False
    with pytest.raises(ValueError, match="discrete motor action"):
        sl.check_env_step_log(True, 8, discrete_motor=False)


def test_dmc_vec_env_refuses_step_log_before_any_gpu_work():
    """DMCVecEnv's motor actions are float vectors, which the env's int32 payload would log wrong (action_dim = 1) or not at all:
    step_log is refused in the constructor's first lines, for both kinds the history serves."""
    from active_gym import DMCEnvArgs
    from active_gym.dmc_env import DMCVecEnv
    from active_gym.vector import AtariVecEnv
    assert AtariVecEnv._discrete_motor is True and DMCVecEnv._discrete_motor is False
    for kind in ("base", "fixed"):
        with pytest.raises(ValueError, match="discrete motor action"):
            DMCVecEnv(DMCEnvArgs("cartpole", "swingup", 0, (84, 84), history_len=8, step_log=True), 2, kind=kind)
    with pytest.raises(ValueError, match="history_len"):
        DMCVecEnv(DMCEnvArgs("cartpole", "swingup", 0, (84, 84), step_log=True), 2, kind="base")


# ---------------------------------------------------------------------------------------------- the rules, by hand
R = [None, 0.1, 0.7, None, 1.3, -2.9, 0.37, 5.1]          # the reward of the step that produced index k (None: a reset observation)


def _stage_a():
    """One env, fs = 2, T = 6.  Episode 1: indices 0 (reset) 1 2 (terminal); episode 2: 3 (reset) 4.  Recorded: 1, 2, 4."""
    h = HistoryModel(1, 2, 6)
    log = sm.StepLogModel(h, 4)
    for k in range(5):
        assert h.push([2 | (CLEAR if k in (0, 3) else 0)])[0] == k
        if R[k] is not None:
            log.record([k], [R[k]], [sm.TERMINATED if k == 2 else 0], np.full((1, 4), k, np.uint8))
    return h, log


def _stage_b(h, log):
    """... then 5 6 7 are appended (index 7 reuses the row of index 1; 0 and 1 are evicted) and 5, 6 recorded; 7 not yet."""
    for k in (5, 6, 7):
        assert h.push([2])[0] == k
    for k in (5, 6):
        log.record([k], [R[k]], [0], np.full((1, 4), k, np.uint8))


def _expect(got, steps, nxt, rewards=(), terminal=False, first=None):
    assert got[:2] == (steps, nxt), got
    if steps == 0:
        assert got[2:] == (None, None, None, None)
        return
    G, disc = sm.fold(rewards, GAMMA)
    assert len(rewards) == steps
    assert sm.bits(got[2]) == sm.bits(G) and sm.bits(got[3]) == sm.bits(0.0 if terminal else disc), got
    assert got[4] == (sm.TERMINATED if terminal else 0) and got[5].tolist() == [first] * 4


def test_hand_written_case():
    h, log = _stage_a()
    g = lambda k, nstep=3: log.gather(0, k, nstep, GAMMA)  # noqa: E731
    _expect(g(0), 2, 2, [R[1], R[2]], terminal=True, first=1)     # stops at a terminal row
    _expect(g(0, 1), 1, 1, [R[1]], first=1)
    _expect(g(1), 1, 2, [R[2]], terminal=True, first=2)
    _expect(g(2), 0, -1)                                          # stops at a reset row: 3 begins another episode
    _expect(g(3), 1, 4, [R[4]], first=4)                          # stops at the end of the history
    _expect(g(4), 0, -1)
    _expect(g(-1), 0, -1)
    _expect(g(5), 0, -1)
    assert log.gather(1, 0, 3, GAMMA)[0] == 0 and log.gather(-1, 0, 3, GAMMA)[0] == 0      # no such env
    _stage_b(h, log)
    assert int(log.stamp[7 % 6, 0]) == 1                          # the row 7 will use still carries index 1's data
    _expect(g(4), 2, 6, [R[5], R[6]], first=5)                    # stops at an unrecorded row
    _expect(g(6, 1), 0, -1)                                       # the row reused by 1 + T is not read as 7's
    _expect(g(3), 3, 6, [R[4], R[5], R[6]], first=4)
    _expect(g(0), 0, -1)                                          # evicted
    _expect(g(1), 0, -1)
    _expect(g(2), 0, -1)                                          # retained, and still before a reset
    log.record([7], [R[7]], [sm.TRUNCATED], np.full((1, 4), 7, np.uint8))
    got = g(4, 64)
    assert got[:2] == (3, 7) and got[4] == sm.TRUNCATED and sm.bits(got[3]) == sm.bits(sm.fold(R[5:8], GAMMA)[1])      # truncated: discount stays
    assert sm.bits(got[2]) == sm.bits(sm.fold(R[5:8], GAMMA)[0])
    # what record skips: -1, an evicted index, an index not yet issued
    before = log.stamp.copy()
    for k in (-1, 1, 8):
        log.record([k], [9.0], [0], np.zeros((1, 4), np.uint8))
    assert np.array_equal(log.stamp, before)
    log.clear()
    assert all(g(k)[0] == 0 for k in range(-1, 9))


# ---------------------------------------------------------------------------------------------- the host side of the fold
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "steplog_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "steplog_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "steplog_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


def _random_case():
    """N = 3, T = 8, fs = 2, 30 steps of commands(5, ..) incl. CLEAR / SKIP; rewards random float32 (not small integers: the
    order of the operations shows), random end flags, about a fifth of the rows left unrecorded."""
    N, T = 3, 8
    h = HistoryModel(N, 2, T)
    log = sm.StepLogModel(h)
    rng = np.random.default_rng(17)
    for cmd in rm.commands(5, N, 30):
        idx = h.push(cmd)
        idx[rng.random(N) < 0.2] = -1
        flags = (rng.random(N) < 0.15) * sm.TERMINATED + (rng.random(N) < 0.05) * sm.TRUNCATED
        log.record(idx, (rng.standard_normal(N) * 3).astype(np.float32), flags.astype(np.uint8))
    return h, log


def _tokens(h, log, nstep, samples):
    tok = [h.T, h.N, nstep, int(sm.bits(GAMMA))] + h.count.tolist() + h.age.ravel().tolist() + log.stamp.ravel().tolist()
    tok += log.reward.view(np.uint32).ravel().tolist() + log.flags.ravel().tolist()
    for n, k in samples:
        tok += [n, k]
    return [str(int(t)) for t in tok]


def _want(log, samples, nstep):
    out = []
    for n, k in samples:
        m, nxt, G, disc, last, _ = log.gather(n, k, nstep, GAMMA)
        out.append("0 -1 - - -" if m == 0 else f"{m} {nxt} {last} {int(sm.bits(G).view(np.uint32))} {int(sm.bits(disc).view(np.uint32))}")
    return out


def _check_harness(binary, tmp_path):
    h, log = _stage_a()
    _stage_b(h, log)
    cases = [(h, log)]
    h2, log2 = _random_case()
    cases.append((h2, log2))
    seen = set()
    for ci, (hh, ll) in enumerate(cases):
        samples = [(n, k) for n in range(-1, hh.N + 1) for k in range(-1, int(hh.count.max()) + 1)]
        for nstep in (1, 3, 64):
            tok = _tokens(hh, ll, nstep, samples)
            if ci == 0:
                r = subprocess.run([binary, *tok], capture_output=True, text=True, timeout=300)          # on the command line
            else:
                path = tmp_path / f"case_{nstep}.txt"
                path.write_text("\n".join(tok))
                r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)     # from a file
            assert r.returncode == 0, r.stdout + r.stderr
            want = _want(ll, samples, nstep)
            assert r.stdout.strip().splitlines() == want, (ci, nstep)
            if ci == 1:
                seen |= {int(w.split()[0]) for w in want}
    assert {0, 1, 2, 3} <= seen and max(seen) >= 4          # the random case folds long walks too
    r = subprocess.run([binary, "8", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


def test_host_side_of_the_fold_equals_the_model(harness, tmp_path):
    _check_harness(harness, tmp_path)


def test_host_side_of_the_fold_under_sanitizers(harness_san, tmp_path):
    _check_harness(harness_san, tmp_path)
