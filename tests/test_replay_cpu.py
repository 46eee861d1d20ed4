"""CPU: include/agx_replay.h (the replay sampler) <-> libagx.so's exports <-> active_gym/replay.py; the argument checks that come
before any HIP call; the rules the GPU tests use (tests/replay_model.py) on a hand-written case; uniformity of the draw on the
model; and the __host__ side of csrc/agx_replay_draw.h (tests/replay_harness.cpp) against the model beyond 2^32 candidates."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import replay_model as rm
from glimpse_model import taken_count
from history_model import CLEAR, SKIP, HistoryModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_replay.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAMES = ["agx_replay_create", "agx_replay_destroy", "agx_replay_inspect", "agx_replay_sample", "agx_replay_seed"]
CONFIGS = [(0, 0), (0, 1), (2, 1), (0, 3)]          # (back, forward)


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
    from active_gym import replay as rp
    src = open(HEADER).read()
    found = dict(re.findall(r"^#define\s+AGX_REPLAY_([A-Z_]+)\s+(\d+)\b", src, flags=re.M))
    assert found == {"SPAN_LIMIT": "64", "ATTEMPT_LIMIT": "64"}
    assert (rp.SPAN_LIMIT, rp.ATTEMPT_LIMIT) == (64, 64)


def test_entry_points_are_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    for name in NAMES:
        assert hasattr(handle, name), name
    from active_gym import replay as rp
    assert sorted(rp.SIGNATURES) == NAMES
    assert rp.SIGNATURES["agx_replay_seed"][1][1] is ctypes.c_uint64          # the seed travels by value, all 64 bits
    assert [len(rp.SIGNATURES[n][1]) for n in NAMES] == [5, 1, 7, 7, 3]
    rp.lib()                                       # binds every signature: AttributeError if one is not exported
    import active_gym
    assert active_gym.ReplaySampler is rp.ReplaySampler


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_replay.h") in deps
    for f in ("agx_k7_replay.h", "agx_replay_impl.h", "agx_replay_draw.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_headers_and_bindings_are_untouched():
    """The sampler is additive.  The token is agx_replay: agx_history.h's prose already speaks of a replay buffer."""
    from active_gym import _native as nat
    from active_gym import glimpse as gl
    from active_gym import history as hi
    from active_gym import native_hostout as nh
    from active_gym import native_loop as nl
    for hdr in ("agx.h", "agx_loop.h", "agx_hostout.h", "agx_history.h", "agx_glimpse.h"):
        assert "agx_replay" not in open(os.path.join(REPO, "include", hdr)).read(), hdr
    for mod in (nat, nl, nh, hi, gl):
        assert not [k for k in mod.SIGNATURES if "replay" in k]
    assert (len(nat.SIGNATURES), len(nl.SIGNATURES), len(hi.SIGNATURES), len(gl.SIGNATURES)) == (28, 6, 8, 1)
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2
    assert ctypes.sizeof(nat.AgxConfig) == 96


def test_null_and_out_of_range_arguments_are_invalid_before_any_hip_call():
    from active_gym import _native as nat
    from active_gym import replay as rp
    _build_mod().build()
    lib = rp.lib()
    r = ctypes.c_void_p()
    assert lib.agx_replay_create(None, 0, 1, 16, ctypes.byref(r)) == nat.E_INVALID and not r.value
    assert "null argument" in nat.last_error(None)
    for back, forward, attempts, what in [(-1, 1, 16, "back"), (65, 1, 16, "back"), (0, -1, 16, "forward"), (0, 65, 16, "forward"),
                                          (0, 1, -1, "attempts"), (0, 1, 65, "attempts")]:
        assert lib.agx_replay_create(None, back, forward, attempts, ctypes.byref(r)) == nat.E_INVALID and not r.value
        assert f"{what} must be" in nat.last_error(None), (back, forward, attempts)
    assert lib.agx_replay_destroy(None) == nat.OK
    assert lib.agx_replay_seed(None, 7, None) == nat.E_INVALID
    assert lib.agx_replay_sample(None, 4, None, None, None, None, None) == nat.E_INVALID
    assert lib.agx_replay_inspect(None, None, None, 4, None, None, None) == nat.E_INVALID


def test_python_refusals_need_no_gpu():
    from active_gym import replay as rp
    assert rp.check_replay_args(0, 1, 0) == (0, 1, 16) and rp.check_replay_args(64, 64, 64) == (64, 64, 64)
    for kw, what in [(dict(back=-1), "back"), (dict(back=65), "back"), (dict(forward=65), "forward"), (dict(forward=-1), "forward"),
                     (dict(attempts=65), "attempts"), (dict(attempts=-1), "attempts")]:
        with pytest.raises(ValueError, match=what):
            rp.ReplaySampler(None, **kw)           # refused before the history is looked at
    with pytest.raises(ValueError, match="forward >= 1"):
        rp.check_transitions(0, 0, None)
    with pytest.raises(ValueError, match="back >= 2"):
        rp.check_transitions(1, 1, 3)
    rp.check_transitions(2, 1, 3)
    rp.check_transitions(0, 1, None)
    rp.check_transitions(0, 1, 1)


# ---------------------------------------------------------------------------------------------- the draw function
def test_sm_is_splitmix64():
    want = [6457827717110365317, 3203168211198807973, 9817491932198370423]
    assert [rm.SM(1234567, i) for i in range(3)] == want
    assert rm.splitmix64(1234567, 3) == want                  # ... and the definition (a state that advances) gives the same
    for s in (0, 7, rm.M64, 1 << 63):
        assert [rm.SM(s, i) for i in range(5)] == rm.splitmix64(s, 5)


# ---------------------------------------------------------------------------------------------- the accepted set
def _hand_written():
    """T = 4, fs = 3, one env: append, append, CLEAR, SKIP, append (tests/test_history_cpu.py's case)."""
    m = HistoryModel(1, 3, 4)
    for c in (2, 2, 2 | CLEAR, SKIP, 2):
        m.push([c])
    return m


def test_hand_written_case():
    m = _hand_written()                       # indices 0 .. 3, ages 0 1 0 1, all retained and valid
    assert rm.accepted_set(m, 0, 0) == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert rm.accepted_set(m, 0, 1) == [(0, 0), (0, 2)]        # 1 -> 2 crosses the CLEAR; 3 has no successor yet
    assert rm.accepted_set(m, 1, 1) == [(0, 0), (0, 2)]        # back reaches no further than the episode's first append
    assert rm.candidates(m, 1) == ([0], [3], [0, 3])
    for _ in range(3):
        m.push([2])                           # indices 3 .. 6 retained, ages 1 2 3 4; 3 and 4 need the evicted row 2
    assert rm.accepted_set(m, 0, 0) == [(0, 5), (0, 6)]
    assert rm.accepted_set(m, 0, 1) == [(0, 5)]
    assert rm.accepted_set(m, 1, 1) == []                      # (0, 5) needs (0, 4) valid: it is not
    assert rm.candidates(m, 1) == ([3], [3], [0, 3])
    assert rm.inspect(m, 0, 5) == (3, 1) and rm.inspect(m, 0, 6) == (4, 0) and rm.inspect(m, 0, 4) == (-1, -1)


def test_inspect_on_the_hand_written_case():
    m = _hand_written()
    assert [rm.inspect(m, 0, k) for k in range(-1, 5)] == [(-1, -1), (0, 1), (1, 0), (0, 1), (1, 0), (-1, -1)]
    assert rm.inspect(m, 1, 0) == (-1, -1)


def _main_model(N=5, T=8, fs=4, seed=3, steps=13):
    m = HistoryModel(N, fs, T)
    for cmd in rm.commands(seed, N, steps):
        m.push(cmd)
    return m


@pytest.mark.parametrize("back, forward", CONFIGS)
def test_what_follows_from_acceptance(back, forward):
    """For every accepted (n, k): (n, k + f) is valid for f <= forward, and the glimpse memory of back + 1 glimpses is full at k
    and at k + forward."""
    for m in (_main_model(), _main_model(6, 16, 4, 5, 40)):
        V = rm.accepted_set(m, back, forward)
        assert V
        for n, k in V:
            assert all(m.valid(n, k + f) for f in range(forward + 1))
            for kk in (k, k + forward):
                assert taken_count(m, n, kk, back + 1) == min(back + 1, rm.age(m, n, kk) + 1)
            assert rm.inspect(m, n, k)[1] >= forward


# ---------------------------------------------------------------------------------------------- uniformity
@pytest.mark.parametrize("back, forward", CONFIGS)
def test_draws_are_uniform_over_the_accepted_set(back, forward):
    """N = 5, T = 8, fs = 4, commands(3, 5, 13), seed 7, call 0, B = 4096, attempts 16: every member of the accepted set is
    drawn, nothing outside it is, each member's count lies within 4.5 sigma of ok / |V|, and ok >= 0.99 B."""
    m = _main_model()
    B = 4096
    V = rm.accepted_set(m, back, forward)
    env, idx, ok, total = rm.draw(m, back, forward, 16, 7, 0, B)
    n_ok = int(ok.sum())
    assert total == rm.candidates(m, forward)[2][-1] > 0
    assert n_ok >= 0.99 * B
    assert ((env == -1) == (ok == 0)).all() and ((idx == -1) == (ok == 0)).all()
    drawn = {}
    for n, k, o in zip(env.tolist(), idx.tolist(), ok.tolist()):
        if o:
            drawn[(n, k)] = drawn.get((n, k), 0) + 1
    assert sorted(drawn) == V
    p = 1.0 / len(V)
    mean, sigma = n_ok * p, np.sqrt(n_ok * p * (1 - p))
    dev = max(abs(c - mean) for c in drawn.values()) / sigma
    print(f"(back, forward) = {(back, forward)}: |V| = {len(V)}, ok = {n_ok}, max deviation = {dev:.2f} sigma")
    assert dev <= 4.5
    if (back, forward) == (0, 3):
        assert n_ok < B                        # this config exercises the -1 path


# ---------------------------------------------------------------------------------------------- the 64-bit harness
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "replay_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "replay_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "replay_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


BIG_LO = [7, 0, 11, 5]
BIG_L = [3_000_000_000, 0, 5_000_000_000, 0]      # the total exceeds 2^32; a zero-length env inside and a zero-length last env
KEY, ATTEMPTS, DRAWS = rm.SM(7, 0), 16, 1000


def _check_big(binary):
    args = [str(KEY), str(ATTEMPTS), str(DRAWS)] + [str(v) for pair in zip(BIG_LO, BIG_L) for v in pair]
    r = subprocess.run([binary, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "sm 6457827717110365317 3203168211198807973 9817491932198370423"
    off = [0]
    for l in BIG_L:
        off.append(off[-1] + l)
    assert lines[1] == f"total {off[-1]}" and off[-1] > 1 << 32
    got = [tuple(map(int, ln.split())) for ln in lines[2:]]
    want = [rm.pick(KEY, b, ATTEMPTS, b % ATTEMPTS, BIG_LO, off) for b in range(DRAWS)]
    assert got == want
    assert {n for n, _ in got} == {0, 2}                         # zero-length envs are never found
    assert any(k - BIG_LO[2] > 1 << 32 for n, k in got if n == 2)
    for cnt, T, fwd in [(0, 8, 0), (0, 8, 1), (3, 8, 1), (3, 8, 5), (8, 8, 1), (13, 8, 3), (13, 8, 64), ((1 << 40) + 5, 1 << 20, 1)]:
        r = subprocess.run([binary, "len", str(cnt), str(T), str(fwd)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        lo = max(cnt - T, 0)
        assert tuple(map(int, r.stdout.split())) == (lo, max(cnt - fwd - lo, 0)), (cnt, T, fwd)


def test_host_side_of_the_draw_beyond_32_bits(harness):
    _check_big(harness)


def test_host_side_of_the_draw_under_sanitizers(harness_san):
    _check_big(harness_san)
