"""CPU: include/agx_augment.h (the random-shift augmentation) <-> libagx.so's exports <-> active_gym/augment.py; the argument
checks that come before any HIP call; the shift map on a hand-written table; the draw's distribution on the model
(tests/shift_model.py); and the __host__ side of csrc/agx_shift_math.h (tests/shift_harness.cpp) against the model."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import shift_model as sm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_augment.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAMES = ["agx_history_observe_shifted", "agx_shift_create", "agx_shift_destroy", "agx_shift_draw", "agx_shift_seed"]


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _declared(header):
    src = open(header).read()
    return sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M)))


# ---------------------------------------------------------------------------------------------- surface
def test_header_declares_exactly_the_five_entry_points():
    assert _declared(HEADER) == NAMES
    from active_gym import augment as au
    found = dict(re.findall(r"^#define\s+AGX_SHIFT_([A-Z_]+)\s+(\d+)\b", open(HEADER).read(), flags=re.M))
    assert found == {"PAD_LIMIT": "32"}
    assert au.PAD_LIMIT == sm.PAD_LIMIT == 32


def test_entry_points_are_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    for name in NAMES:
        assert hasattr(handle, name), name
    from active_gym import augment as au
    assert sorted(au.SIGNATURES) == NAMES
    assert au.SIGNATURES["agx_shift_seed"][1][1] is ctypes.c_uint64            # the seed travels by value, all 64 bits
    assert [len(au.SIGNATURES[n][1]) for n in NAMES] == [13, 3, 1, 4, 3]
    au.lib()                                       # binds every signature: AttributeError if one is not exported
    import active_gym
    assert active_gym.RandomShift is au.RandomShift


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_augment.h") in deps
    for f in ("agx_k10_augment.h", "agx_augment_impl.h", "agx_shift_math.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_headers_and_bindings_are_untouched():
    """The augmentation is additive: no older header names it, no older binding grew."""
    from active_gym import _native as nat
    from active_gym import glimpse as gl
    from active_gym import history as hi
    from active_gym import native_hostout as nh
    from active_gym import native_loop as nl
    from active_gym import priority as pr
    from active_gym import replay as rp
    from active_gym import steplog as sl
    for hdr in ("agx.h", "agx_loop.h", "agx_hostout.h", "agx_history.h", "agx_glimpse.h", "agx_replay.h", "agx_steplog.h", "agx_priority.h"):
        src = open(os.path.join(REPO, "include", hdr)).read()
        assert "agx_shift" not in src and "observe_shifted" not in src, hdr
    for mod in (nat, nl, nh, hi, gl, rp, sl, pr):
        assert not [k for k in mod.SIGNATURES if "shift" in k]
    assert [len(m.SIGNATURES) for m in (nat, nl, hi, gl, rp, sl)] == [28, 6, 8, 1, 5, 6] and len(pr.SIGNATURES) == 8
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2
    assert ctypes.sizeof(nat.AgxConfig) == 96


def test_null_and_out_of_range_arguments_are_invalid_before_any_hip_call():
    """Every AGX_E_INVALID names its argument.  The argument checks come before the handle is looked at, so none needs a GPU."""
    from active_gym import _native as nat
    from active_gym import augment as au
    _build_mod().build()
    lib = au.lib()
    s = ctypes.c_void_p()
    for pad in (-1, 33):
        assert lib.agx_shift_create(None, pad, ctypes.byref(s)) == nat.E_INVALID and not s.value
        assert "pad must be 0 .. 32" in nat.last_error(None)
    assert lib.agx_shift_create(None, 4, ctypes.byref(s)) == nat.E_INVALID and not s.value
    assert "null h" in nat.last_error(None)
    assert lib.agx_shift_create(None, 4, None) == nat.E_INVALID and "null out" in nat.last_error(None)
    assert lib.agx_shift_destroy(None) == nat.OK
    assert lib.agx_shift_seed(None, 7, None) == nat.E_INVALID and "null s" in nat.last_error(None)
    assert lib.agx_shift_draw(None, -1, None, None) == nat.E_INVALID and "B = -1" in nat.last_error(None)
    assert lib.agx_shift_draw(None, 4, None, None) == nat.E_INVALID and "null d_shift" in nat.last_error(None)
    buf = (ctypes.c_int64 * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.agx_shift_draw(None, 4, ptr, None) == nat.E_INVALID and "null s" in nat.last_error(None)
    assert lib.agx_shift_draw(None, 0, None, None) == nat.E_INVALID and "null s" in nat.last_error(None)

    def observe(what=0, env=ptr, index=ptr, B=4, action=None, dt=0, pad=4, shift=ptr, obs=ptr):
        return lib.agx_history_observe_shifted(None, what, env, index, B, action, dt, pad, shift, obs, None, None, None)

    for kw, named in [(dict(what=2), "what must be"), (dict(pad=-1), "pad must be 0 .. 32"), (dict(pad=33), "pad must be 0 .. 32"),
                      (dict(B=-1), "B = -1"), (dict(env=None), "null d_env"), (dict(index=None), "null d_index"),
                      (dict(shift=None), "null d_shift"), (dict(obs=None), "null d_obs"), (dict(action=ptr, dt=4), "action dtype 4"),
                      (dict(), "null h"), (dict(B=0, env=None, index=None, shift=None, obs=None), "null h")]:
        assert observe(**kw) == nat.E_INVALID, kw
        assert named in nat.last_error(None), (kw, nat.last_error(None))


def test_python_refusals_need_no_gpu():
    from active_gym import augment as au
    assert au.check_pad(0) == 0 and au.check_pad(32) == 32
    for pad in (-1, 33):
        with pytest.raises(ValueError, match="pad must be"):
            au.check_pad(pad)
        with pytest.raises(ValueError, match="pad must be"):
            au.RandomShift(None, pad=pad)          # refused before the history is looked at
    class Shift:
        history = object()
    au.check_no_glimpses(None)
    au.check_shift_read(None, 3, None)
    au.check_shift_read(Shift(), None, Shift.history)
    with pytest.raises(ValueError, match="the glimpse memory is not shifted"):
        au.check_no_glimpses(3)
    with pytest.raises(ValueError, match="the glimpse memory is not shifted"):
        au.check_shift_read(Shift(), 3, Shift.history)
    with pytest.raises(ValueError, match="another history"):
        au.check_shift_read(Shift(), None, object())


def test_replay_batch_refuses_shift_pad_with_glimpses_before_it_looks_at_the_env():
    """env.replay_batch checks its arguments first: no step log, no history and no GPU are needed to be refused."""
    from active_gym.vector import AtariVecEnv
    env = object.__new__(AtariVecEnv)              # (class defaults only: steplog is None)
    with pytest.raises(ValueError, match="the glimpse memory is not shifted"):
        env.replay_batch(8, glimpses=3, shift_pad=4)
    with pytest.raises(ValueError, match="pad must be"):
        env.replay_batch(8, shift_pad=33)
    with pytest.raises(ValueError, match="needs a step log"):
        env.replay_batch(8, shift_pad=4)
    with pytest.raises(ValueError, match="needs a frame history"):
        env.random_shift()


# ---------------------------------------------------------------------------------------------- the shift map
def test_shift_src_on_a_hand_written_table():
    assert [[sm.shift_src(i, d, 2, 5) for i in range(5)] for d in range(5)] == [
        [0, 0, 0, 1, 2],           # d = 0: two pixels of the top / left edge replicated
        [0, 0, 1, 2, 3],
        [0, 1, 2, 3, 4],           # d = pad: the identity
        [1, 2, 3, 4, 4],
        [2, 3, 4, 4, 4]]
    rows = [[sm.shift_src(i, d, 8, 3) for i in range(3)] for d in range(17)]          # the pad exceeds the plane: the clamp saturates
    assert rows[:7] == [[0, 0, 0]] * 7 and rows[7:10] == [[0, 0, 1], [0, 1, 2], [1, 2, 2]] and rows[10:] == [[2, 2, 2]] * 7
    assert [sm.shift_src(i, 0, 0, 4) for i in range(4)] == [0, 1, 2, 3]
    assert np.array_equal(sm.src_index([0, 2, 4, -3, 99], 2, 5),
                          np.array([[0, 0, 0, 1, 2], [0, 1, 2, 3, 4], [2, 3, 4, 4, 4], [0, 0, 0, 1, 2], [2, 3, 4, 4, 4]]))
    assert [sm.clamp(d, 4) for d in (-3, 0, 8, 99)] == [0, 0, 8, 8]


# ---------------------------------------------------------------------------------------------- the draw
DIST_SEED = 11


def test_draws_are_uniform_over_the_81_cells():
    """pad = 4, B = 81 * 2048, seed 11, call 0: each (dy, dx) cell's count lies within 4.5 binomial sigma of B / 81."""
    B = 81 * 2048
    d = sm.draw(DIST_SEED, 0, B, 4)
    assert d.min() == 0 and d.max() == 8
    counts = np.bincount(d[:, 0] * 9 + d[:, 1], minlength=81)
    p = 1.0 / 81
    sigma = np.sqrt(B * p * (1 - p))
    dev = np.abs(counts - B * p).max() / sigma
    print(f"81 cells, B = {B}: max deviation = {dev:.2f} sigma")
    assert counts.size == 81 and dev <= 4.5
    assert not np.array_equal(d[:1000], sm.draw(DIST_SEED, 1, 1000, 4))         # the next call differs
    assert not (d[:, 0] == d[:, 1]).all()                                       # the two halves of z are independent


def test_pad_zero_draws_zero():
    assert not sm.draw(5, 0, 100, 0).any()


# ---------------------------------------------------------------------------------------------- the harness
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "shift_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "shift_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "shift_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


def _run(binary, *args):
    r = subprocess.run([binary, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [list(map(int, ln.split())) for ln in r.stdout.strip().splitlines()]


def _check_harness(binary):
    B = 1000
    for pad in (0, 4, 32):
        for seed in (0, 1234567, (1 << 64) - 1):
            for call in range(4):
                got = np.array(_run(binary, "draw", seed, call, pad, B), np.int32)
                assert np.array_equal(got, sm.draw(seed, call, B, pad)), (pad, seed, call)
    for pad, n in [(2, 5), (8, 3), (0, 4), (32, 84)]:
        assert _run(binary, "src", pad, n) == [[sm.shift_src(i, d, pad, n) for i in range(n)] for d in range(2 * pad + 1)], (pad, n)
    assert _run(binary, "clamp", 4, -3, 0, 4, 8, 99, -2147483648, 2147483647) == [[0, 0, 4, 8, 8, 0, 8]]


def test_host_side_of_the_shift_math(harness):
    _check_harness(harness)


def test_host_side_of_the_shift_math_under_sanitizers(harness_san):
    _check_harness(harness_san)
