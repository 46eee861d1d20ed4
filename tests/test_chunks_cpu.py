"""CPU: include/agx_chunks.h (device-side minibatches of chunks on a rollout, for recurrent learners) <-> libagx.so's exports <->
active_gym/chunks.py; the refusals that need no GPU; the rule, the list, the take and its padding on tests/chunks_model.py alone;
and the __host__ side of csrc/agx_chunk_math.h (tests/chunks_harness.cpp), plain and under the host's sanitizers, against the
model."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import chunks_model as cm
import minibatch_model as mm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_chunks.h")
CSRC = os.path.join(REPO, "active-gym_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAMES = ["agx_chunks_create", "agx_chunks_destroy", "agx_chunks_select", "agx_chunks_take"]
SHAPES = ((1, 1), (3, 2), (5, 37), (64, 2), (65, 5), (130, 37), (3, 65))           # (N, L): tests/test_gpu_chunks.py's
LENGTHS = (1, 2, 5, 37, 64, None)                                                  # C; None: L


def chunk_lengths(L):
    return sorted({L if c is None else c for c in LENGTHS if (c or L) <= L})


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------------------------------------- surface
def test_header_declares_exactly_the_four_entry_points():
    src = open(HEADER).read()
    assert sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M))) == NAMES
    found = dict(re.findall(r"^#define\s+AGX_CHUNK_([A-Z_]+)\s+(\d+)\b", src, flags=re.M))
    assert found == {"LIMIT": "256", "L_LIMIT": "4096", "LIST": "2", "STREAMS": "8", "START_CHUNK": "1", "START_EPISODE": "2"}
    assert re.findall(r'^#include\s+(\S+)', src, flags=re.M) == ['"agx_history.h"']
    from active_gym import chunks as ch
    from active_gym import minibatch as mb
    from active_gym import rollout as ro
    assert (ch.CHUNK_LIMIT, ch.CHUNK_STREAMS, ch.START_CHUNK, ch.START_EPISODE) == (cm.LIMIT, mm.STREAMS, cm.START_CHUNK, cm.START_EPISODE) == (256, 8, 1, 2)
    assert cm.LIST == 2 > max(mb.MB_LIVE, mb.MB_BOOT) and ro.ROLLOUT_LIMIT == 4096
    assert ro.TERMINATED | ro.TRUNCATED | ro.CUT == cm.BREAK == 7 and ro.BOOT == 8         # the bits the header states as numbers


def test_the_header_respects_the_scans_of_the_older_tests():
    src = open(HEADER).read()
    for word in ("agx_minibatch", "agx_rollout", "agx_sequence", "agx_priority", "agx_steplog", "agx_replay", "agx_shift", "observe_shifted"):
        assert word not in src, word
    assert "retrace" not in src.lower()


def test_entry_points_are_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    for name in NAMES:
        assert hasattr(handle, name), name
    from active_gym import chunks as ch
    assert sorted(ch.SIGNATURES) == NAMES
    ch.lib()                                       # binds every signature: AttributeError if one is not exported
    import active_gym
    from active_gym.history import FrameHistory
    from active_gym.vector import AtariVecEnv
    assert active_gym.Chunker is ch.Chunker
    assert callable(active_gym.Rollout.chunker) and callable(FrameHistory.chunker) and callable(AtariVecEnv.rollout_chunks)


def _ctype(decl, ch):
    """The ctypes type of one parameter declaration of the header."""
    decl = re.sub(r"\s+", " ", decl.strip())
    kind = re.sub(r"\b\w+$", "", decl).strip() if not decl.endswith("*") else decl       # the declaration without the parameter's name
    table = {"uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "agx_chunks **": ctypes.POINTER(ctypes.c_void_p),
             "const agx_chunks_io *": ctypes.POINTER(ch.ChunkIo)}
    if kind in table:
        return table[kind]
    assert kind.endswith("*"), decl
    return ctypes.c_void_p


def test_every_prototype_matches_its_signature():
    from active_gym import chunks as ch
    src = open(HEADER).read()
    protos = dict(re.findall(r"^AGX_API int (agx_\w+)\(([^;]*?)\);", src, flags=re.M | re.S))
    assert sorted(protos) == NAMES
    for name in NAMES:
        res, args = ch.SIGNATURES[name]
        want = [_ctype(p, ch) for p in protos[name].split(",")]
        assert res is ctypes.c_int and args == want, (name, args, want)
    assert [len(ch.SIGNATURES[n][1]) for n in NAMES] == [3, 1, 6, 10]


def test_the_io_struct_is_the_headers(harness, tmp_path):
    """Field by field: the names and the order of agx_chunks_io; its size and two offsets as the C compiler lays them out."""
    from active_gym import chunks as ch
    body = re.search(r"typedef struct agx_chunks_io \{(.*?)\} agx_chunks_io;", open(HEADER).read(), flags=re.S).group(1)
    names = re.findall(r"\*?\b([a-z_0-9]+)(?:\[AGX_CHUNK_STREAMS\])?\s*[,;]", body)
    assert names == [f[0] for f in ch.ChunkIo._fields_]
    assert ctypes.sizeof(ch.ChunkIo) == 8 * 3 + 4 * 2 + 8 * 8 + 8 * 5 + 8 * 8 + 8 * 3 + 8 * 3 + 8 + 8
    (size, o_slot, o_valid), = _run(harness, tmp_path, [4])
    assert (size, o_slot, o_valid) == (ctypes.sizeof(ch.ChunkIo), ch.ChunkIo.d_slot.offset, ch.ChunkIo.d_valid.offset)


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_chunks.h") in deps
    for f in ("agx_k17_chunks.h", "agx_chunks_host.h", "agx_chunk_math.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_headers_and_bindings_are_untouched():
    """The chunker is additive: no older header names it, no older binding grew, the ABI version stays 2."""
    from active_gym import _native as nat
    from active_gym import minibatch as mb
    from active_gym import retrace as rt
    from active_gym import rollout as ro
    from active_gym import sequence as sq
    from active_gym import steplog as sl
    from active_gym import vtrace as vt
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):
        if hdr != "agx_chunks.h":
            assert "agx_chunk" not in open(os.path.join(REPO, "include", hdr)).read().lower(), hdr
    assert [len(m.SIGNATURES) for m in (nat, sl, sq, ro, vt, mb, rt)] == [28, 6, 3, 2, 1, 5, 1]
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2


def test_every_launching_entry_point_opens_a_device_guard():
    """tests/test_host_logic_cpu.py's audit of the *_impl.h files, on agx_chunks_host.h: every extern "C" entry point that
    launches, copies or acquires opens a DeviceGuard before its first device call."""
    src = open(os.path.join(CSRC, "agx_chunks_host.h")).read()
    assert '#include "agx_chunks_host.h"' in open(os.path.join(CSRC, "agx_api.hip")).read()
    entry = r"^(?:int|int64_t|const char \*)\s*(agx_\w+)\(([^\n]*\}\n|.*?^})"
    touch = (r"hipLaunchKernelGGL|AGX_LAUNCH|hipMemcpy|hipMemset|hipMalloc|hipFree|hipEventRecord|hipStream|hipDeviceSynchronize"
             r"|->own\.(?:device_mem|pinned|event|stream)\(|\b(?:ctx_build|loop_build|hist_block|hostout_make)\("
             r"|\bhist_chunks\(|\blaunch_hist_\w+\(|\bdelete \w+;|\bhostout_free\(")
    body = src[src.index('extern "C" {'):]
    seen = []
    for m in re.finditer(entry, body, flags=re.S | re.M):
        name, text = m.group(1), m.group(2)
        touches = re.search(touch, text)
        assert touches, name                        # all four launch, copy, acquire or give back
        assert 0 <= text.find("DeviceGuard g(") < touches.start(), name
        seen.append(name)
    assert sorted(seen) == NAMES
    assert not re.search(r"hipMalloc|hipFree|hipHostMalloc|hipHostFree", src) and "asm" not in src


def test_the_refusals_stand_in_the_headers_order():
    """The source order of the checks of select and take in agx_chunks_host.h: the handle, L, C, (S and first, C * S, io, n_f32,)
    d_len, (d_ends / d_slot,) the env range - and no launch before the last of them."""
    src = open(os.path.join(CSRC, "agx_chunks_host.h")).read()
    sel = src[src.index("int agx_chunks_select("):src.index("int agx_chunks_take(")]
    take = src[src.index("int agx_chunks_take("):]
    for text, marks in ((sel, ["null argument (c)", "chunks_bad_shape(", "null buffer (d_len)", "full_range(", "hipLaunchKernelGGL"]),
                        (take, ["null argument (c)", "chunks_bad_shape(", "first = %d, S = %d", "C * S", "null argument (io)", "n_f32 must be",
                                "null buffer (d_len)", '"d_ends" : "d_slot"', "full_range(", "S_ == 0", "hipLaunchKernelGGL"])):
        at = [text.index(m) for m in marks]
        assert at == sorted(at), marks
    shape = src[src.index("int chunks_bad_shape("):src.index("}  // namespace")]
    assert shape.index("rollout_bad_L(") < shape.index("C must be")


def test_a_null_handle_is_invalid_before_anything_else():
    from active_gym import _native as nat
    from active_gym import chunks as ch
    _build_mod().build()
    lib = ch.lib()
    buf = (ctypes.c_int64 * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    out = ctypes.c_void_p()
    assert lib.agx_chunks_create(None, 0, ctypes.byref(out)) == nat.E_INVALID and not out.value
    assert "agx_chunks_create: null argument" in nat.last_error(None)
    assert lib.agx_chunks_destroy(None) == nat.OK
    for L, C in ((4, 2), (0, 1), (5000, 1), (4, 0), (4, 5), (300, 257)):
        assert lib.agx_chunks_select(None, L, C, ptr, None, None) == nat.E_INVALID
        assert "agx_chunks_select: null argument (c)" in nat.last_error(None)
        assert lib.agx_chunks_take(None, 1, L, C, ptr, ptr, -1, -1, None, None) == nat.E_INVALID
        assert "agx_chunks_take: null argument (c)" in nat.last_error(None)


def test_python_refusals_need_no_gpu():
    from active_gym import chunks as ch
    from active_gym.vector import AtariVecEnv
    assert ch.check_chunk_length(1, 1) == 1 and ch.check_chunk_length(256, 4096) == 256 and ch.check_chunk_length(37, 37) == 37
    for C, L in ((0, 4), (-1, 4), (5, 4), (257, 4096), (257, 257)):
        with pytest.raises(ValueError, match="C must be 1 .. min"):
            ch.check_chunk_length(C, L)
    with pytest.raises(ValueError, match="C \\* S"):
        ch.check_rows(256, 2 ** 23)
    ch.check_rows(256, 2 ** 23 - 1)
    assert ch.check_streams(None) == {} and list(ch.check_streams(["adv"], {"adv": 1})) == ["adv"]
    with pytest.raises(ValueError, match="at most 8 streams"):
        ch.check_streams({f"s{k}": None for k in range(9)})
    for name in ("mask", "start", "state_index", "valid", "slot"):
        with pytest.raises(ValueError, match="outputs of every take"):
            ch.check_streams({name: None})
    env = object.__new__(AtariVecEnv)              # (class defaults only: steplog is None)
    with pytest.raises(ValueError, match="rollout_chunks needs a step log"):
        env.rollout_chunks({}, 4, 64)              # (raised by the call, not by the first next())

    class Closed:                                  # a Chunker whose handle is gone refuses before it looks at anything
        value = None

    c = object.__new__(ch.Chunker)
    c._handle = Closed()
    for call in (lambda: c.select({}, 4), lambda: c.take({}, 0, 4, 4)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    with pytest.raises(ValueError, match="S must be"):
        c.take({}, 0, -1, 4)
    with pytest.raises(ValueError, match="first must be"):
        c.take({}, -1, 4, 4)


# ---------------------------------------------------------------------------------------------- the model alone
def _take_all(model, a, L, C, permute=False, extra=0):
    total = int(model.off[-1])
    return model.take(permute, a["len"], a["ends"], L, C, 0, total + extra, a["obs_index"], a["next_index"], a["payload"], a["streams"][:2])


def test_hand_cases():
    """L = 5, C = 2 (G = 3, chunk 2 has one padded step at t = 5): len = 3 gives chunks 1 and 2; len = 4 starts inside chunk 0."""
    L, C = 5, 2
    a = cm.rollout_arrays(0, 1, L)
    a["ends"][:] = 0
    a["len"][:] = 3
    model = cm.Model(1, 0)
    assert model.select(a["len"], L, C) == 2
    got = _take_all(model, a, L, C)
    assert got["chunk"].tolist() == [1, 2] and got["first"].tolist() == [0, 0] and got["steps"].tolist() == [2, 1]
    assert got["slot"].T.tolist() == [[2, 3], [4, -1]] and got["mask"].T.tolist() == [[1, 1], [1, 0]]
    assert got["start"].T.tolist() == [[1, 0], [1, 0]] and got["env"].tolist() == [[0, 0], [0, 0]]
    assert got["state_index"].tolist() == [a["obs_index"][2, 0], a["obs_index"][4, 0]] and got["obs_index"][1, 1] == -1
    a["len"][:] = 4
    assert model.select(a["len"], L, C) == 3
    got = _take_all(model, a, L, C)
    assert got["chunk"].tolist() == [0, 1, 2] and got["first"].tolist() == [1, 0, 0] and got["steps"].tolist() == [1, 2, 1]
    assert got["slot"].T.tolist() == [[-1, 1], [2, 3], [4, -1]] and got["start"].T.tolist() == [[0, 1], [1, 0], [1, 0]]
    assert got["state_index"][0] == a["obs_index"][1, 0]
    a["ends"][1, 0], a["ends"][3, 0] = 2, 9          # an end at t0 and one at the last step of chunk 1
    got = _take_all(model, a, L, C)
    assert got["start"].T.tolist() == [[0, 1], [1 | 2, 0], [1 | 2, 0]] and got["ends"].T.tolist() == [[0, 2], [0, 9], [0, 0]]


@pytest.mark.parametrize("N,L", SHAPES)
def test_the_list_covers_every_live_slot_exactly_once(N, L):
    a = cm.rollout_arrays(100 + N * 131 + L, N, L)
    clamped = np.clip(a["len"], 0, L)
    live = np.arange(L)[:, None] >= L - clamped[None, :]
    tt, nn = np.nonzero(live)
    want = sorted((tt * N + nn).tolist())
    for C in chunk_lengths(L):
        G = -(-L // C)
        model = cm.Model(N, 7)
        total = model.select(a["len"], L, C)
        t0 = L - clamped
        count = np.where(clamped > 0, G - t0 // C, 0)                  # the header's closed form against the model's definition
        assert total == int(count.sum()) <= N * G and np.array_equal(np.diff(model.off), count)
        for permute in (False, True):
            got = _take_all(model, a, L, C, permute, extra=3)
            assert got["valid"].tolist() == [1] * total + [0] * 3
            masked = got["slot"][got["mask"] == 1]
            assert sorted(masked.tolist()) == want, "every live slot lies in exactly one (chunk, step)"
            assert int(got["steps"][:total].sum()) == int(clamped.sum()) and (got["steps"][:total] >= 1).all()
            assert ((got["slot"] >= 0) == (got["mask"] == 1))[:, :total].all()
            if total:
                assert (got["slot"][:, total:] == got["slot"][:, :3]).all() and not got["mask"][:, total:].any(), "positions past total wrap"
                assert (got["env"] == got["env"][0]).all() and (got["slot"][got["slot"] >= 0] % N == np.broadcast_to(got["env"], got["slot"].shape)[got["slot"] >= 0]).all()
                first = np.maximum(t0[got["env"][0]] - got["chunk"] * C, 0)            # the header's closed forms
                steps = np.minimum((got["chunk"] + 1) * C, L) - np.maximum(got["chunk"] * C, t0[got["env"][0]])
                assert np.array_equal(got["first"], first) and np.array_equal(got["steps"], steps)
            else:
                assert (got["slot"] == -1).all() and not got["env"].any() and (got["chunk"] == -1).all()
            # start & 2 exactly behind a slot with ends & 7, never at t0
            at = got["slot"] >= 0
            t, n = got["slot"][at] // N, got["slot"][at] % N
            behind = (t > t0[n]) & ((a["ends"][np.maximum(t - 1, 0), n] & 7) != 0)
            assert np.array_equal((got["start"][at] & 2) != 0, behind) and not got["start"][~at].any()
            assert np.array_equal((got["start"] & 1) != 0, at & (np.arange(C)[:, None] == got["first"][None, :]))
        order = _take_all(model, a, L, C)
        key = list(zip(order["env"][0].tolist(), order["chunk"].tolist()))
        assert key == sorted(key) and len(set(key)) == total, "the list is env-major, ascending g"


def test_len_outside_its_range_is_clamped():
    N, L, C = 5, 4, 3
    model = cm.Model(N, 0)
    assert model.select(np.array([-3, 9, 0, 4, 1], np.int32), L, C) == 0 + 2 + 0 + 2 + 1
    assert model.off.tolist() == [0, 0, 2, 2, 4, 5]


def test_the_epoch_is_a_bijection_of_its_own():
    """A bijection on [0, total); another order than a minibatcher's of the same seed; another order after another select."""
    N, L, C = 9, 8, 1                                                   # C = 1: the chunks are the live slots, list for list
    a = cm.rollout_arrays(5, N, L)
    model, mini = cm.Model(N, 3), mm.Model(N, 3)
    total = model.select(a["len"], L, C)
    assert total == mini.select(mm.LIVE, a["len"], a["ends"], L) > 16
    plain = _take_all(model, a, L, C)["slot"][0].tolist()
    assert plain == mini.take(mm.LIVE, False, a["len"], a["ends"], L, 0, total)["slot"].tolist()
    first = _take_all(model, a, L, C, True)["slot"][0].tolist()
    assert sorted(first) == sorted(plain) and len(set(first)) == total and first != plain
    assert first != mini.take(mm.LIVE, True, a["len"], a["ends"], L, 0, total)["slot"].tolist()
    assert model.base not in mini.base
    model.select(a["len"], L, C)
    second = _take_all(model, a, L, C, True)["slot"][0].tolist()
    assert sorted(second) == sorted(first) and second != first and model.calls == 2
    again = cm.Model(N, 3)
    again.select(a["len"], L, C)
    assert _take_all(again, a, L, C, True)["slot"][0].tolist() == first


def test_mismatched_arguments_are_invalid_rather_than_wrong():
    N, L, C = 6, 5, 2
    a = cm.rollout_arrays(11, N, L)
    a["len"][:] = [5, 3, 0, 5, 2, 4]
    model = cm.Model(N, 1)
    assert model.select(a["len"], L, C) == 3 + 2 + 0 + 3 + 2 + 3
    for L2, C2 in ((5, 1), (4, 2), (5, 5)):                             # another (L, C): null rows throughout
        got = model.take(False, a["len"], a["ends"][:L2], L2, C2, 0, 13)
        assert (got["slot"] == -1).all() and (got["chunk"] == -1).all() and not got["valid"].any() and not got["env"].any()
    got = model.take(False, np.array([1, 3, 0, 5, 0, 5], np.int32), a["ends"], L, C, 0, 13)
    # env 0 now has one chunk (its second and third are lost), env 4 none, env 5 three (others than before); env 1 and 3 unchanged
    lost = np.array([0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0], bool)
    assert np.array_equal(got["chunk"] == -1, lost) and np.array_equal(got["valid"] == 0, lost) and (got["slot"][:, lost] == -1).all()
    assert got["chunk"][0] == 2 and got["first"][0] == 0 and got["steps"][0] == 1


# ---------------------------------------------------------------------------------------------- the harness
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", CSRC, os.path.join(REPO, "tests", "chunks_harness.cpp"), "-o", out], check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "chunks_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "chunks_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


def _run(binary, tmp_path, tokens):
    path = tmp_path / "case.txt"
    path.write_text(" ".join(map(str, tokens)))
    r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]


def _u64(v):
    return [v >> 32, v & 0xFFFFFFFF]


def _check_harness(binary, tmp_path):
    for seed in (0, 3, mm.M64):                    # the keys
        for calls in (0, 1, 5):
            (bh, bl, kh, kl), = _run(binary, tmp_path, [3, *_u64(seed), calls])
            model = cm.Model(1, seed)
            assert (bh << 32) | bl == model.base and (kh << 32) | kl == mm.sm(model.base, calls)
    for N, L in SHAPES:                            # the counts and the takes: matched, another len, another (L, C)
        a = cm.rollout_arrays(100 + N * 131 + L, N, L)
        b = cm.rollout_arrays(900 + N * 131 + L, N, L)
        for C in chunk_lengths(L):
            counts = [r[0] for r in _run(binary, tmp_path, [1, N, L, C, *a["len"].tolist()])]
            model = cm.Model(N, 9)
            total = model.select(a["len"], L, C)
            assert counts == np.diff(model.off).tolist() and sum(counts) == total
            other = (L, C + 1) if C < L else (L, C - 1) if C > 1 else None
            for permute in (0, 1):
                for first, S in ((0, 1), (max(total - 300, 0), min(total, 300) + 3), (total + 1, 4)):
                    for arrays, seen in ((a, (L, C)), (b, (L, C)), (a, other)):
                        if seen is None:
                            continue
                        got = _run(binary, tmp_path, [2, permute, N, L, C, first, S, *seen, *_u64(model.key), *model.off.tolist(),
                                                      *arrays["len"].tolist(), *arrays["ends"].reshape(-1).tolist()])
                        model.seen = seen
                        want = model.take(bool(permute), arrays["len"], arrays["ends"], L, C, first, S)
                        model.seen = (L, C)
                        what = (N, L, C, permute, first, S, seen)
                        assert len(got) == S and all(len(r) == 5 + 4 * C for r in got), what
                        got = np.array(got, np.int64).reshape(S, -1)
                        for k, key in enumerate(("chunk", "first", "steps", "valid")):
                            assert got[:, k].tolist() == want[key].tolist(), (key, what)
                        assert got[:, 4].tolist() == want["env"][0].tolist(), what
                        for k, key in enumerate(("slot", "ends", "start", "mask")):
                            assert np.array_equal(got[:, 5 + k::4].T, want[key]), (key, what)


def test_host_side_of_the_chunk_math(harness, tmp_path):
    _check_harness(harness, tmp_path)


def test_host_side_of_the_chunk_math_under_sanitizers(harness_san, tmp_path):
    _check_harness(harness_san, tmp_path)
