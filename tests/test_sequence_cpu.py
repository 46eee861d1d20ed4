"""CPU: include/agx_sequence.h (sequence replay) <-> libagx.so's exports <-> active_gym/sequence.py; the argument checks that come
before any HIP call; the Python refusals; the length rule on a hand-written case (tests/sequence_model.py); the __host__ side of
csrc/agx_sequence_math.h (tests/sequence_harness.cpp) against the model; and the seeds of the GPU cases on the model alone."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sequence_model as qm
from history_model import CLEAR, HistoryModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_sequence.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAMES = ["agx_sequence_gather", "agx_sequence_lengths", "agx_sequence_observe"]


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _declared(header):
    src = open(header).read()
    return sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M)))


# ---------------------------------------------------------------------------------------------- surface
def test_header_declares_exactly_the_three_entry_points():
    assert _declared(HEADER) == NAMES
    from active_gym import sequence as sq
    found = dict(re.findall(r"^#define\s+AGX_SEQUENCE_([A-Z_]+)\s+(\d+)\b", open(HEADER).read(), flags=re.M))
    assert found == {"LIMIT": "256"}
    assert sq.SEQUENCE_LIMIT == qm.SEQUENCE_LIMIT == 256


def test_entry_points_are_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    for name in NAMES:
        assert hasattr(handle, name), name
    from active_gym import sequence as sq
    assert sorted(sq.SIGNATURES) == NAMES
    assert [len(sq.SIGNATURES[n][1]) for n in NAMES] == [16, 7, 13]
    assert sq.SIGNATURES["agx_sequence_gather"][1][6] is ctypes.c_float
    sq.lib()                                       # binds every signature: AttributeError if one is not exported
    import active_gym
    assert active_gym.SequenceReplay is sq.SequenceReplay and active_gym.mixed_priority is sq.mixed_priority


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_sequence.h") in deps
    for f in ("agx_k11_sequence.h", "agx_sequence_impl.h", "agx_sequence_math.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_headers_and_bindings_are_untouched():
    """Sequence replay is additive: no older header names it, no older binding grew, the ABI version stays 2."""
    from active_gym import _native as nat
    from active_gym import augment as au
    from active_gym import glimpse as gl
    from active_gym import history as hi
    from active_gym import native_hostout as nh
    from active_gym import native_loop as nl
    from active_gym import priority as pr
    from active_gym import replay as rp
    from active_gym import steplog as sl
    for hdr in ("agx.h", "agx_loop.h", "agx_hostout.h", "agx_history.h", "agx_glimpse.h", "agx_replay.h", "agx_steplog.h", "agx_priority.h",
                "agx_augment.h"):
        assert "agx_sequence" not in open(os.path.join(REPO, "include", hdr)).read(), hdr
    for mod in (nat, nl, nh, hi, gl, rp, sl, pr, au):
        assert not [k for k in mod.SIGNATURES if "sequence" in k]
    assert [len(m.SIGNATURES) for m in (nat, nl, hi, gl, rp, sl, pr, au)] == [28, 6, 8, 1, 5, 6, 8, 5]
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2
    assert ctypes.sizeof(nat.AgxConfig) == 96


def test_null_and_out_of_range_arguments_are_invalid_before_any_hip_call():
    """Every AGX_E_INVALID names its argument.  The argument checks come before the handle is looked at, so none needs a GPU; the
    null handle comes after them."""
    from active_gym import _native as nat
    from active_gym import sequence as sq
    _build_mod().build()
    lib = sq.lib()
    buf = (ctypes.c_int64 * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    big = (1 << 31) // 8 + 1                       # big * 8 > INT32_MAX

    def lengths(env=ptr, index=ptr, B=4, L=8, out=ptr):
        return lib.agx_sequence_lengths(None, env, index, B, L, out, None)

    def gather(env=ptr, index=ptr, B=4, L=8, nstep=3, steps=ptr):
        return lib.agx_sequence_gather(None, env, index, B, L, nstep, 0.99, 0, None, steps, None, None, None, None, None, None)

    def observe(what=0, env=ptr, index=ptr, length=ptr, B=4, L=8, planes=1, obs=ptr):
        return lib.agx_sequence_observe(None, what, env, index, length, B, L, planes, 0, obs, None, None, None)

    cases = [
        (lengths, dict(L=0), "L must be 1 .. 256"), (lengths, dict(L=257), "L must be 1 .. 256"), (lengths, dict(B=-1), "B must be >= 0"),
        (lengths, dict(B=big), "B * L"), (lengths, dict(env=None), "null buffer (d_env)"), (lengths, dict(index=None), "null buffer (d_index)"),
        (lengths, dict(out=None), "null buffer (d_len)"), (lengths, dict(), "null argument (h)"),
        (lengths, dict(B=0, env=None, index=None, out=None), "null argument (h)"),
        (gather, dict(L=0), "L must be 1 .. 256"), (gather, dict(L=257), "L must be 1 .. 256"), (gather, dict(nstep=0), "nstep must be 1 .. 64"),
        (gather, dict(nstep=65), "nstep must be 1 .. 64"), (gather, dict(L=0, nstep=0), "L must be"), (gather, dict(B=-1), "B must be >= 0"),
        (gather, dict(B=big), "B * L"), (gather, dict(env=None), "null buffer (d_env)"), (gather, dict(index=None), "null buffer (d_index)"),
        (gather, dict(steps=None), "null buffer (d_steps)"), (gather, dict(), "null argument (log)"),
        (gather, dict(B=0, env=None, index=None, steps=None), "null argument (log)"),
        (observe, dict(L=0), "L must be 1 .. 256"), (observe, dict(L=257), "L must be 1 .. 256"), (observe, dict(what=2), "what must be"),
        (observe, dict(planes=0), "planes must be >= 1"), (observe, dict(B=-1), "B must be >= 0"), (observe, dict(B=big), "B * L"),
        (observe, dict(env=None), "null buffer (d_env)"), (observe, dict(index=None), "null buffer (d_index)"),
        (observe, dict(length=None), "null buffer (d_len)"), (observe, dict(obs=None), "null buffer (d_obs)"),
        (observe, dict(), "null argument (h)"), (observe, dict(B=0, env=None, index=None, length=None, obs=None), "null argument (h)"),
    ]
    for call, kw, named in cases:
        assert call(**kw) == nat.E_INVALID, (call.__name__, kw)
        assert named in nat.last_error(None), (call.__name__, kw, nat.last_error(None))
        assert "agx_sequence_" + call.__name__ in nat.last_error(None)


def test_python_refusals_need_no_gpu():
    import torch
    from active_gym import sequence as sq
    from active_gym.vector import AtariVecEnv
    assert sq.check_length(1) == 1 and sq.check_length(256) == 256
    for L in (0, 257, -3):
        with pytest.raises(ValueError, match="L must be 1 .. 256"):
            sq.check_length(L)
    assert sq.check_planes(None, 4) == 4 and sq.check_planes(1, 4) == 1
    for planes in (0, 5):
        with pytest.raises(ValueError, match="planes must be 1 .. frame_stack"):
            sq.check_planes(planes, 4)
    assert sq.check_sequence_draw(8) == 7 and sq.check_sequence_draw(80, 10) == 9 and sq.check_sequence_draw(65) == 64
    assert sq.check_sequence_draw(256, 65) == 64
    with pytest.raises(ValueError, match="min_length"):
        sq.check_sequence_draw(80)                 # forward = 79 exceeds AGX_REPLAY_SPAN_LIMIT: the message asks for min_length
    with pytest.raises(ValueError, match="min_length"):
        sq.check_sequence_draw(80, 66)
    with pytest.raises(ValueError, match="min_length must be 1 .. length"):
        sq.check_sequence_draw(8, 9)
    with pytest.raises(ValueError, match="L must be"):
        sq.check_sequence_draw(257, 4)
    env = object.__new__(AtariVecEnv)              # (class defaults only: steplog is None)
    with pytest.raises(ValueError, match="needs a step log"):
        env.sequence_batch(8, 8)
    with pytest.raises(ValueError, match="min_length"):
        env.sequence_batch(8, 80)
    with pytest.raises(ValueError, match="nstep"):
        env.sequence_batch(8, 8, nstep=0)
    with pytest.raises(ValueError, match="L must be"):
        env.sequence_batch(8, 0)

    class Closed:
        history, pipe, device = None, None, None

        def _live(self):
            raise RuntimeError("the step log or its history is closed")

    seq = sq.SequenceReplay(Closed())
    z = torch.zeros(1, dtype=torch.int32)
    for call in (lambda: seq.lengths(z, z, 4), lambda: seq.gather(z, z, 4), lambda: seq.observe(z, z, z, 4, what="full")):
        with pytest.raises(RuntimeError, match="closed"):          # use after the log or its history is closed
            call()
    with pytest.raises(ValueError, match="L must be"):
        seq.lengths(z, z, 0)                       # refused before anything is looked at
    with pytest.raises(ValueError, match="what must be"):
        seq.observe(z, z, z, 4, what="glimpse")


def test_mixed_priority_is_r2d2s():
    import torch
    from active_gym import mixed_priority
    td = torch.tensor([[1.0, 3.0, 9.0, 9.0], [2.0, 2.0, 2.0, 2.0], [5.0, 5.0, 5.0, 5.0]])
    live = torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0]], dtype=torch.uint8)
    got = mixed_priority(td, live, eta=0.9)
    want = torch.tensor([0.9 * 3.0 + 0.1 * 2.0, 0.9 * 2.0 + 0.1 * 2.0, 0.0])
    assert got.shape == (3,) and torch.allclose(got, want, rtol=1e-6, atol=0)
    assert torch.allclose(mixed_priority(td, live, eta=0.0), torch.tensor([2.0, 2.0, 0.0]), rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------- the length rule
def _hand_model():
    """One env, fs = 2, T = 8, two episodes: indices 0 .. 4 (ages 0 .. 4) and 5 .. 9 (ages 0 .. 4); 0 and 1 are evicted."""
    m = HistoryModel(1, 2, 8)
    for step in range(10):
        m.push(np.array([2 | (CLEAR if step in (0, 5) else 0)], np.uint8))
    assert int(m.count[0]) == 10 and [int(m.age[k % 8, 0]) for k in range(2, 10)] == [2, 3, 4, 0, 1, 2, 3, 4]
    return m


HAND = [  # (k, L, length, what ends it)
    (3, 4, 2, "episode"),          # 3, 4, then 5 is a reset row
    (4, 4, 1, "episode"),
    (5, 4, 4, "full"),             # the reset row itself starts a sequence
    (7, 4, 3, "end"),              # 7, 8, 9, then the end of the history
    (9, 4, 1, "end"),
    (9, 1, 1, "full"),
    (3, 1, 1, "full"),             # L = 1
    (5, 8, 5, "end"),              # L larger than what is left
    (5, 256, 5, "end"),
    (3, 256, 2, "episode"),
    (2, 4, 0, "zero"),             # retained, but its stack reaches the evicted row 1
    (1, 4, 0, "zero"),             # evicted
    (0, 1, 0, "zero"),
    (10, 4, 0, "zero"),            # not yet issued
    (-1, 4, 0, "zero"),
]


def test_length_rule_on_a_hand_written_case():
    m = _hand_model()
    for k, L, want, why in HAND:
        assert qm.length(m, 0, k, L) == want and qm.kind(m, 0, k, L) == why, (k, L)
    assert qm.length(m, 1, 5, 4) == 0 and qm.length(m, -1, 5, 4) == 0          # no such env
    import replay_model as rm
    for k in range(-1, 11):
        for L in (1, 2, 4, 8, 256):
            ahead = rm.inspect(m, 0, k)[1]
            assert qm.length(m, 0, k, L) == (0 if ahead < 0 else 1 + min(ahead, L - 1)), (k, L)


# ---------------------------------------------------------------------------------------------- the harness
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "sequence_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "sequence_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "sequence_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


def _harness_lengths(binary, tmp_path, m, L, samples):
    tokens = [m.T, m.N, m.fs, L, *m.count.tolist(), *m.age.reshape(-1).tolist()]
    for n, k in samples:
        tokens += [n, k]
    path = tmp_path / f"case_{L}.txt"
    path.write_text(" ".join(map(str, tokens)))
    r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [int(ln) for ln in r.stdout.split()]


def _check_harness(binary, tmp_path):
    m = _hand_model()
    for L in (1, 4, 8, 256):
        samples = [(0, k) for k in range(-1, 11)] + [(1, 5), (-1, 5)]
        assert _harness_lengths(binary, tmp_path, m, L, samples) == [qm.length(m, n, k, L) for n, k in samples], L
    got = {(k, L): v for (k, L, _, _), v in zip(HAND, [_harness_lengths(binary, tmp_path, m, L, [(0, k)])[0] for k, L, _, _ in HAND])}
    assert got == {(k, L): want for k, L, want, _ in HAND}
    # a random case: N = 7, fs = 4, T = 24, 60 steps with CLEAR and SKIP, every start and some outside the envs
    cmds = qm.commands(21, 7, 60)
    m = HistoryModel(7, 4, 24)
    for cmd in cmds:
        m.push(cmd)
    samples = qm.starts(m) + [(3, 1 << 40), (3, -(1 << 40)), (1 << 20, 2)]
    for L in (1, 3, 8, 64, 256):
        want = [qm.length(m, n, k, L) for n, k in samples]
        assert _harness_lengths(binary, tmp_path, m, L, samples) == want, L
        assert len(set(want)) >= min(L, 4)
    # the L > 64 case of the GPU tests
    m = HistoryModel(qm.LONG_N, qm.LONG_FS, qm.LONG_T)
    for cmd in qm.long_commands():
        m.push(cmd)
    samples = qm.starts(m)
    for L in qm.LONG_LS:
        assert _harness_lengths(binary, tmp_path, m, L, samples) == [qm.length(m, n, k, L) for n, k in samples], L


def test_host_side_of_the_length_rule(harness, tmp_path):
    _check_harness(harness, tmp_path)


def test_host_side_of_the_length_rule_under_sanitizers(harness_san, tmp_path):
    _check_harness(harness_san, tmp_path)


# ---------------------------------------------------------------------------------------------- the GPU cases' seeds
@pytest.mark.parametrize("name", sorted(qm.CASES))
def test_gpu_case_seeds_cover_every_kind_of_sequence(name):
    """On the model alone: at the case's largest L its starts give full-length, episode-cut, history-end-cut and zero-length
    sequences, and its command bytes hold CLEAR and SKIP."""
    cmds, m = qm.case_model(name)
    L = qm.CASES[name][5]
    k = qm.kinds(m, L)
    print(name, k)
    assert min(k.values()) >= 1, k
    assert (cmds & CLEAR).any() and (cmds & qm.SKIP).any()
    assert qm.kinds(m, 1)["full"] == sum(m.valid(n, kk) for n, kk in qm.starts(m))          # L = 1: every valid start is full


def test_long_case_holds_the_lengths_it_is_there_for():
    m = HistoryModel(qm.LONG_N, qm.LONG_FS, qm.LONG_T)
    for cmd in qm.long_commands():
        m.push(cmd)
    assert int(m.count.min()) == int(m.count.max()) == qm.LONG_STEPS < qm.LONG_T
    for (n, k), want in qm.LONG_WITNESS.items():
        assert qm.length(m, n, k, 256) == want, (n, k)
    at256 = {qm.length(m, n, k, 256) for n, k in qm.starts(m)}
    assert set(qm.LONG_LS) <= at256
    for L in qm.LONG_LS:                           # at each L: sequences that fill it exactly by a break, and ones it cuts
        got = [qm.length(m, n, k, L) for n, k in qm.starts(m)]
        assert L in got and 0 in got and any(0 < v < L for v in got), L
    k = qm.kinds(m, 70)
    assert min(k.values()) >= 1, k


def test_commands_are_test_gpu_historys():
    import test_gpu_history as th
    for seed, N, steps in [(3, 5, 25), (11, 4, 11)]:
        assert np.array_equal(qm.commands(seed, N, steps), th.commands(seed, N, steps))
