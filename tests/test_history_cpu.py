"""CPU: include/agx_history.h (the on-device frame history) <-> libagx.so's exports <-> active_gym/history.py; the argument
checks that come before any HIP call; the bookkeeping model the GPU tests use (tests/history_model.py) on a hand-written case."""
import ctypes
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from history_model import CLEAR, SKIP, HistoryModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_history.h")


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M)))


def test_header_surface_is_exported_and_bound():
    names = _declared()
    assert names == ["agx_history_bytes", "agx_history_clear", "agx_history_create", "agx_history_destroy", "agx_history_last_index",
                     "agx_history_observe", "agx_history_push", "agx_loop_set_history"]
    handle = ctypes.CDLL(_build_mod().build())
    for name in names:
        assert hasattr(handle, name), name
    from active_gym import history as hi
    assert sorted(hi.SIGNATURES) == names
    hi.lib()                                       # binds every signature: AttributeError if one is not exported


def test_binding_constants_mirror_the_header():
    from active_gym import history as hi
    src = open(HEADER).read()
    found = dict(re.findall(r"^#define\s+AGX_(HIST_[A-Z]+)\s+(\d+)\b", src, flags=re.M))
    assert sorted(found) == ["HIST_FOVEA", "HIST_FULL"]
    for name, val in found.items():
        assert getattr(hi, name) == int(val), name
    from active_gym import _native as nat
    assert (CLEAR, SKIP) == (nat.CMD_CLEAR, nat.CMD_SKIP)          # the model reads command bytes as the ingest does


def test_the_older_headers_and_bindings_are_untouched():
    """The history is additive: agx.h keeps its 28 entry points, agx_loop.h its six, and their bindings bind no history name."""
    from active_gym import _native as nat
    from active_gym import native_hostout as nh
    from active_gym import native_loop as nl
    for mod in (nat, nl, nh):
        assert not [k for k in mod.SIGNATURES if "history" in k]
    assert len(nat.SIGNATURES) == 28 and len(nl.SIGNATURES) == 6
    for hdr in ("agx.h", "agx_loop.h", "agx_hostout.h"):
        assert "history" not in open(os.path.join(REPO, "include", hdr)).read()


def test_source_hash_covers_the_new_files():
    m = _build_mod()
    deps = {os.path.relpath(d, REPO) for d in m.DEPS}
    assert os.path.join("include", "agx_history.h") in deps
    assert os.path.join("active-gym_amd", "csrc", "agx_history_impl.h") in deps
    assert os.path.join("active-gym_amd", "csrc", "agx_k5_history.h") in deps
    assert os.path.join("active-gym_amd", "csrc", "agx_resources.h") in deps      # where the history (and every handle) gets its storage


def test_null_arguments_are_invalid_before_any_hip_call():
    from active_gym import _native as nat
    from active_gym import history as hi
    _build_mod().build()
    lib = hi.lib()
    h = ctypes.c_void_p()
    assert lib.agx_history_create(None, 8, ctypes.byref(h)) == nat.E_INVALID and not h.value
    assert "null argument" in nat.last_error(None)
    assert lib.agx_history_destroy(None) == nat.OK
    assert lib.agx_history_clear(None, None) == nat.E_INVALID
    assert lib.agx_history_bytes(None) == nat.E_INVALID
    assert lib.agx_history_push(None, None, None, None) == nat.E_INVALID
    assert lib.agx_history_last_index(None, None, None) == nat.E_INVALID
    assert lib.agx_history_observe(None, hi.HIST_FOVEA, None, None, 0, None, 0, None, None, None, None) == nat.E_INVALID
    assert lib.agx_loop_set_history(None, None) == nat.E_INVALID


def test_model_on_the_hand_written_case():
    """T = 4, fs = 3, one env: append, append, CLEAR, SKIP, append x 4."""
    m = HistoryModel(1, 3, 4)
    got = [int(m.push([c])[0]) for c in (2, 2, 2 | CLEAR, SKIP, 2)]
    assert got == [0, 1, 2, -1, 3]
    # four appends so far, all retained (T = 4); ages 0, 1, 0 (CLEAR), 1
    assert [int(m.age[k % 4, 0]) for k in range(4)] == [0, 1, 0, 1]
    assert [m.valid(0, k) for k in range(-1, 5)] == [False, True, True, True, True, False]
    assert m.rows(0, 0) == [None, None, 0]          # a new history: zeros before the first append
    assert m.rows(0, 1) == [None, 0, 1]
    assert m.rows(0, 2) == [None, None, 2]          # the CLEAR zeroed the stack
    assert m.rows(0, 3) == [None, 2, 3]
    got = [int(m.push([2])[0]) for _ in range(3)]
    assert got == [4, 5, 6] and int(m.count[0]) == 7
    # indices 3 .. 6 are retained; their ages are 1, 2, 3, 4
    assert [int(m.age[k % 4, 0]) for k in range(3, 7)] == [1, 2, 3, 4]
    # 0 .. 2 are evicted; 3 needs row 2 and 4 needs rows 2, 3 - row 2 is evicted; 5 and 6 have their three rows; 7 was never issued
    assert [m.valid(0, k) for k in range(8)] == [False, False, False, False, False, True, True, False]
    assert m.rows(0, 5) == [3, 4, 5] and m.rows(0, 6) == [4, 5, 6]
    assert not m.valid(1, 5) and not m.valid(-1, 5)   # no such env
    # after clear(): nothing is valid, indices restart at 0, and the frames before an env's next append are unknown - its
    # first fs - 1 samples stay invalid until a CLEAR says the stack is zeros
    m.clear()
    assert not any(m.valid(0, k) for k in range(8))
    assert [int(m.push([2])[0]) for _ in range(3)] == [0, 1, 2]
    assert [m.valid(0, k) for k in range(3)] == [False, False, True] and m.rows(0, 2) == [0, 1, 2]
    assert int(m.push([1 | CLEAR])[0]) == 3 and m.valid(0, 3) and m.rows(0, 3) == [None, None, 3]


def test_age_saturates_at_255():
    m = HistoryModel(1, 2, 2)
    for _ in range(300):
        m.push([2])
    assert int(m.age[299 % 2, 0]) == 255 and m.valid(0, 299) and m.rows(0, 299) == [298, 299]


@pytest.mark.parametrize("kind, extra, match", [
    ("peripheral", {}, "kind"), ("flexible", {}, "kind"), ("flexible", {"ragged_obs": "packed"}, "kind"),
])
def test_vec_env_refuses_unsupported_history_before_any_gpu_work(kind, extra, match):
    """history_len > 0 with a kind the history does not serve: ValueError from the constructor's first lines (this runs
    without a GPU: nothing of the GPU path is reached)."""
    from active_gym import AtariVecEnv
    args = types.SimpleNamespace(obs_size=(84, 84), frame_stack=4, action_repeat=4, history_len=8, obs_dtype="float32", **extra)
    with pytest.raises(ValueError, match=match):
        AtariVecEnv(args, 2, kind=kind)


def test_check_env_history_rules():
    from active_gym.history import check_env_history
    assert check_env_history("peripheral", 0) == 0 and check_env_history("fixed", None) == 0
    assert check_env_history("fixed", 16) == 16 and check_env_history("base", 5) == 5
    with pytest.raises(ValueError, match="gray"):
        check_env_history("fixed", 4, channels=3)
    with pytest.raises(ValueError, match="packed"):
        check_env_history("fixed", 4, ragged_obs="packed")
    with pytest.raises(ValueError, match=">= 0"):
        check_env_history("fixed", -1)
