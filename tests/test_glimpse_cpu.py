"""CPU: include/agx_glimpse.h (the glimpse memory) <-> libagx.so's exports <-> active_gym/glimpse.py; the argument checks that
come before any HIP call; the rule the GPU tests use (tests/glimpse_model.py) on hand-written sequences."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from glimpse_model import sample_class, taken_count, taken_glimpses
from history_model import CLEAR, SKIP, HistoryModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_glimpse.h")


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _declared(header):
    src = open(header).read()
    return sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M)))


def test_header_declares_exactly_the_one_entry_point():
    assert _declared(HEADER) == ["agx_history_observe_memory"]
    from active_gym import glimpse as gl
    limit = re.search(r"^#define\s+AGX_GLIMPSE_LIMIT\s+(\d+)\b", open(HEADER).read(), flags=re.M)
    assert limit and int(limit.group(1)) == gl.GLIMPSE_LIMIT == 8


def test_entry_point_is_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    assert hasattr(handle, "agx_history_observe_memory")
    from active_gym import glimpse as gl
    assert sorted(gl.SIGNATURES) == _declared(HEADER)
    res, args = gl.SIGNATURES["agx_history_observe_memory"]
    # (h, glimpses, d_env, d_index, B, d_obs, d_fov_loc, d_taken, stream)
    assert res is ctypes.c_int and len(args) == 9 and args[1] is ctypes.c_int32 and args[4] is ctypes.c_int32
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (1, 4))
    gl.lib()                                       # binds the signature: AttributeError if it is not exported
    import active_gym
    assert active_gym.GlimpseMemory is gl.GlimpseMemory


def test_the_older_headers_and_bindings_are_untouched():
    from active_gym import _native as nat
    from active_gym import history as hi
    assert len(_declared(os.path.join(REPO, "include", "agx.h"))) == 28 and len(nat.SIGNATURES) == 28
    assert len(hi.SIGNATURES) == 8 and not [k for k in list(nat.SIGNATURES) + list(hi.SIGNATURES) if "memory" in k]
    for hdr in ("agx.h", "agx_loop.h", "agx_hostout.h", "agx_history.h"):
        assert "glimpse" not in open(os.path.join(REPO, "include", hdr)).read().lower()
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2
    assert ctypes.sizeof(nat.AgxConfig) == 96


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_glimpse.h") in deps
    assert os.path.join("active-gym_amd", "csrc", "agx_glimpse_impl.h") in deps
    assert os.path.join("active-gym_amd", "csrc", "agx_k6_glimpse.h") in deps


def test_null_history_is_invalid_before_any_hip_call():
    from active_gym import _native as nat
    from active_gym import glimpse as gl
    _build_mod().build()
    assert gl.lib().agx_history_observe_memory(None, 3, None, None, 1, None, None, None, None) == nat.E_INVALID


def test_python_refusals_need_no_gpu():
    from active_gym import _native as nat
    from active_gym import glimpse as gl
    with pytest.raises(ValueError, match="kind 'fixed'"):
        gl.check_glimpse_source("base", nat.OUT_RESIZE)
    with pytest.raises(ValueError, match="raw crops"):
        gl.check_glimpse_source("fixed", nat.OUT_RAW)
    gl.check_glimpse_source("fixed", nat.OUT_MASK)
    gl.check_glimpse_source("fixed", nat.OUT_RESIZE)


def _push(m, *cmds):
    for c in cmds:
        m.push(np.array([c], np.uint8))


def test_model_clear_one_and_two_appends_back():
    m = HistoryModel(1, 2, 8)
    _push(m, 2, 2, 2 | CLEAR, 2, 2)                       # indices 0 .. 4, ages 0 1 0 1 2
    assert taken_glimpses(m, 0, 2, 3) == [0] and sample_class(m, 0, 2, 3) == "clear"          # the CLEAR append itself
    assert taken_glimpses(m, 0, 3, 3) == [0, 1] and sample_class(m, 0, 3, 3) == "clear"       # a CLEAR one append back
    assert taken_glimpses(m, 0, 4, 3) == [0, 1, 2] and sample_class(m, 0, 4, 3) == "full"     # ... two back: all three
    assert taken_count(m, 0, 4, 8) == 3 and sample_class(m, 0, 4, 8) == "clear"
    assert taken_count(m, 0, 4, 1) == 1 and taken_count(m, 0, 1, 3) == 2
    assert taken_count(m, 0, 5, 3) == 0 and taken_count(m, 0, -1, 3) == 0 and sample_class(m, 0, 5, 3) == "invalid"


def test_model_skip_appends_nothing():
    m = HistoryModel(1, 2, 8)
    _push(m, 2, 2 | SKIP, 2, 2 | SKIP | CLEAR, 2)         # three appends, no CLEAR seen: the skipped ingest did not happen
    assert int(m.count[0]) == 3 and taken_glimpses(m, 0, 2, 3) == [0, 1, 2]


def test_model_eviction_of_the_oldest_glimpse_only():
    m = HistoryModel(1, 2, 3)
    _push(m, 2, 2, 2, 2, 2)                               # indices 2 .. 4 retained; the stack of index 2 needs index 1: gone
    assert m.valid(0, 4) and m.valid(0, 3) and not m.valid(0, 2)
    assert taken_glimpses(m, 0, 4, 3) == [0, 1] and sample_class(m, 0, 4, 3) == "evicted"
    assert taken_glimpses(m, 0, 4, 2) == [0, 1] and sample_class(m, 0, 4, 2) == "full"
    assert taken_count(m, 0, 2, 3) == 0                   # the sample itself is evicted: invalid, whatever its glimpses


def test_model_after_clear():
    m = HistoryModel(1, 3, 8)
    _push(m, 2, 2, 2)
    m.clear()
    _push(m, 2, 2, 2, 2)                                  # the frames before the clear are unknown: indices 0, 1 stay invalid
    assert [taken_count(m, 0, k, 3) for k in range(4)] == [0, 0, 1, 2]
    assert sample_class(m, 0, 3, 3) == "evicted"
    _push(m, 2 | CLEAR, 2)                                # a reset makes the episode's beginning known again
    assert taken_glimpses(m, 0, 4, 3) == [0] and taken_glimpses(m, 0, 5, 3) == [0, 1]


def test_model_age_saturated_at_255():
    m = HistoryModel(1, 2, 300)
    for _ in range(300):
        _push(m, 2)
    assert int(m.age[299, 0]) == 255 and int(m.age[256, 0]) == 255 and int(m.age[254, 0]) == 254
    assert taken_glimpses(m, 0, 299, 8) == list(range(8)) and taken_glimpses(m, 0, 256, 3) == [0, 1, 2]
    assert sample_class(m, 0, 299, 8) == "full"
