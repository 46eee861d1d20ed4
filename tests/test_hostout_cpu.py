"""CPU: include/agx_hostout.h (env-range launches, chunked host-output step) <-> libagx.so's exports <->
active_gym/native_hostout.py; argument checks that come before any HIP call; the chunk partition."""
import ctypes
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _declared():
    src = open(os.path.join(REPO, "include", "agx_hostout.h")).read()
    return sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M)))


def test_header_surface_is_exported_and_bound():
    names = _declared()
    assert names == ["agx_env_range", "agx_hostout_partition", "agx_loop_host_final", "agx_loop_host_prepare", "agx_loop_host_wait",
                     "agx_loop_step_host"]
    handle = ctypes.CDLL(_build_mod().build())
    for name in names:
        assert hasattr(handle, name), name
    from active_gym import native_hostout as nh
    assert sorted(nh.SIGNATURES) == names
    nh.lib()                                       # binds every signature: AttributeError if one is not exported
    hdr = open(os.path.join(REPO, "include", "agx_hostout.h")).read()
    assert int(re.search(r"#define\s+AGX_HOSTOUT_MAX_CHUNKS\s+(\d+)", hdr).group(1)) == nh.MAX_CHUNKS


def test_source_hash_covers_the_new_files():
    """agx_build_info() names the sources the library was built from: the new header and implementation are among them."""
    m = _build_mod()
    deps = {os.path.relpath(d, REPO) for d in m.DEPS}
    assert os.path.join("include", "agx_hostout.h") in deps
    assert os.path.join("active-gym_amd", "csrc", "agx_hostout_impl.h") in deps
    assert os.path.join("active-gym_amd", "csrc", "agx_range.h") in deps


def test_null_and_out_of_range_arguments_are_invalid_before_any_hip_call():
    from active_gym import _native as nat
    from active_gym import native_hostout as nh
    from active_gym import native_loop as nl
    _build_mod().build()
    lib = nh.lib()
    assert lib.agx_env_range(None, 0, 1) == nat.E_INVALID
    res = nl.AgxLoopResult()
    buf = (ctypes.c_int32 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.agx_loop_step_host(None, p, None, 0, None, p, p, p, ctypes.byref(res), None, p, p, p, 2) == nat.E_INVALID
    assert lib.agx_loop_host_wait(None) == nat.E_INVALID
    assert lib.agx_loop_host_prepare(None, 4) == nat.E_INVALID
    assert lib.agx_loop_host_final(None, None, None, None) == nat.E_INVALID
    lo, n = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    assert lib.agx_hostout_partition(0, 2, lo, n) == nat.E_INVALID
    assert lib.agx_hostout_partition(-3, 2, lo, n) == nat.E_INVALID
    assert lib.agx_hostout_partition(8, 0, lo, n) == nat.E_INVALID
    assert lib.agx_hostout_partition(8, -1, lo, n) == nat.E_INVALID
    assert lib.agx_hostout_partition(8, 2, None, n) == nat.E_INVALID
    assert lib.agx_hostout_partition(8, 2, lo, None) == nat.E_INVALID
    with pytest.raises(nat.AgxError):
        nh.partition(0, 3)


@pytest.mark.parametrize("N", [1, 5, 700, 1024])
@pytest.mark.parametrize("C", [1, 2, 4, 7])
def test_partition_covers_the_batch_exactly_in_ascending_order(N, C):
    """[0, N) exactly, ascending, no empty range, min(C, N) ranges (C > N: one env each), sizes within one env of each other.
    No alignment rule: agx_env_range takes any lo (include/agx_hostout.h)."""
    _build_mod().build()
    from active_gym import native_hostout as nh
    parts = nh.partition(N, C)
    assert len(parts) == min(C, N)
    at = 0
    for lo, n in parts:
        assert lo == at and n >= 1
        at += n
    assert at == N
    sizes = [n for _, n in parts]
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


def test_partition_clamps_to_the_chunk_limit():
    _build_mod().build()
    from active_gym import native_hostout as nh
    parts = nh.partition(1024, 1000)
    assert len(parts) == nh.MAX_CHUNKS and sum(n for _, n in parts) == 1024 and parts[0][0] == 0
