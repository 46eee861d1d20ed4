"""CPU: include/agx_minibatch.h (device-side minibatches on a rollout) <-> libagx.so's exports <-> active_gym/minibatch.py; the
refusals that need no GPU; the rule, the lists and the permutation on tests/minibatch_model.py alone; and the __host__ side of
csrc/agx_minibatch_math.h (tests/minibatch_harness.cpp), plain and under the host's sanitizers, against the model."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import minibatch_model as mm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_minibatch.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAMES = ["agx_minibatch_create", "agx_minibatch_destroy", "agx_minibatch_scatter", "agx_minibatch_select", "agx_minibatch_take"]
TOTALS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 257, 1000, 4097, 20000)
KEYS = (0, 0x0123456789ABCDEF, mm.M64)
SHAPES = ((1, 1), (3, 2), (5, 37), (64, 2), (65, 1), (130, 37), (3, 65))          # (N, L): tests/test_gpu_minibatch.py's
SIGMA = 5.0


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------------------------------------- surface
def test_header_declares_exactly_the_five_entry_points():
    src = open(HEADER).read()
    assert sorted(set(re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M))) == NAMES
    found = dict(re.findall(r"^#define\s+AGX_MB_([A-Z_]+)\s+(\d+)\b", src, flags=re.M))
    assert found == {"LIMIT": "4096", "LIVE": "0", "BOOT": "1", "STREAMS": "8"}
    from active_gym import minibatch as mb
    from active_gym import rollout as ro
    assert (mb.MB_LIVE, mb.MB_BOOT, mb.MB_STREAMS) == (mm.LIVE, mm.BOOT, mm.STREAMS) == (0, 1, 8)
    assert ro.ROLLOUT_LIMIT == 4096 and ro.BOOT == mm.BOOT_BIT == 8


def test_entry_points_are_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    for name in NAMES:
        assert hasattr(handle, name), name
    from active_gym import minibatch as mb
    assert sorted(mb.SIGNATURES) == NAMES
    assert [len(mb.SIGNATURES[n][1]) for n in NAMES] == [3, 1, 8, 7, 10]
    mb.lib()                                       # binds every signature: AttributeError if one is not exported
    import active_gym
    assert active_gym.Minibatcher is mb.Minibatcher
    assert callable(active_gym.Rollout.minibatcher)


def test_the_io_struct_is_the_headers():
    """Field by field: the names and the order of agx_minibatch_io, pointers and two i32."""
    from active_gym import minibatch as mb
    body = re.search(r"typedef struct agx_minibatch_io \{(.*?)\} agx_minibatch_io;", open(HEADER).read(), flags=re.S).group(1)
    names = re.findall(r"\*?\b([a-z_0-9]+)(?:\[AGX_MB_STREAMS\])?\s*[,;]", body)
    assert names == [f[0] for f in mb.MinibatchIo._fields_]
    assert ctypes.sizeof(mb.MinibatchIo) == 8 * 3 + 4 * 2 + 8 * 8 + 8 * 5 + 8 * 8 + 8


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_minibatch.h") in deps
    for f in ("agx_k15_minibatch.h", "agx_minibatch_impl.h", "agx_minibatch_math.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_headers_and_bindings_are_untouched():
    """The minibatcher is additive: no older header names it, no older binding grew, the ABI version stays 2."""
    from active_gym import _native as nat
    from active_gym import rollout as ro
    from active_gym import vtrace as vt
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):
        if hdr != "agx_minibatch.h":
            assert "agx_minibatch" not in open(os.path.join(REPO, "include", hdr)).read(), hdr
    assert [len(m.SIGNATURES) for m in (nat, ro, vt)] == [28, 2, 1]
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2


def test_a_null_handle_is_invalid_before_anything_else():
    from active_gym import _native as nat
    from active_gym import minibatch as mb
    _build_mod().build()
    lib = mb.lib()
    buf = (ctypes.c_int64 * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    out = ctypes.c_void_p()
    assert lib.agx_minibatch_create(None, 0, ctypes.byref(out)) == nat.E_INVALID and not out.value
    assert "agx_minibatch_create: null argument" in nat.last_error(None)
    assert lib.agx_minibatch_destroy(None) == nat.OK
    for which, L in ((0, 4), (7, 4), (0, 0), (1, 5000)):
        assert lib.agx_minibatch_select(None, which, L, ptr, ptr, None, None) == nat.E_INVALID
        assert "agx_minibatch_select: null argument (mb)" in nat.last_error(None)
        assert lib.agx_minibatch_take(None, which, 1, L, ptr, ptr, -1, -1, None, None) == nat.E_INVALID
        assert "agx_minibatch_take: null argument (mb)" in nat.last_error(None)
        assert lib.agx_minibatch_scatter(None, -1, None, None, None, L, None, None) == nat.E_INVALID
        assert "agx_minibatch_scatter: null argument (mb)" in nat.last_error(None)


def test_python_refusals_need_no_gpu():
    from active_gym import minibatch as mb
    from active_gym.vector import AtariVecEnv
    assert mb.check_list("live") == 0 and mb.check_list("boot") == 1
    for bad in ("both", 0, None):
        with pytest.raises(ValueError, match="which must be"):
            mb.check_list(bad)
    assert mb.check_minibatch_size(0) == (0, 0) and mb.check_minibatch_size(4096, 2 ** 31 - 1 - 4096) == (2 ** 31 - 1 - 4096, 4096)
    with pytest.raises(ValueError, match="S must be >= 0"):
        mb.check_minibatch_size(-1)
    with pytest.raises(ValueError, match="first must be >= 0"):
        mb.check_minibatch_size(4, -1)
    with pytest.raises(ValueError, match="first \\+ S"):
        mb.check_minibatch_size(4096, 2 ** 31 - 4096)
    assert mb.check_streams(None) == {} and list(mb.check_streams(["adv"], {"adv": 1})) == ["adv"]
    with pytest.raises(ValueError, match="at most 8 streams"):
        mb.check_streams({f"s{k}": None for k in range(9)})
    with pytest.raises(ValueError, match="outputs of every take"):
        mb.check_streams({"valid": None})
    with pytest.raises(ValueError, match="not entries of the batch"):
        mb.check_streams(["adv"], {})
    for bad in (0, -4, 2 ** 31):
        with pytest.raises(ValueError, match="size must be"):
            mb.check_epoch_size(bad)
    env = object.__new__(AtariVecEnv)              # (class defaults only: steplog is None)
    with pytest.raises(ValueError, match="rollout_boot needs a step log"):
        env.rollout_boot({})
    with pytest.raises(ValueError, match="rollout_minibatches needs a step log"):
        env.rollout_minibatches({}, 64)            # (raised by the call, not by the first next())

    class Closed:                                  # a Minibatcher whose handle is gone refuses before it looks at anything
        value = None

    m = object.__new__(mb.Minibatcher)
    m._handle = Closed()
    for call in (lambda: m.select({}), lambda: m.take({}, 0, 4), lambda: m.scatter({}, None, None)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    with pytest.raises(ValueError, match="which must be"):
        m.select({}, "all")
    with pytest.raises(ValueError, match="S must be"):
        m.take({}, 0, -1)


# ---------------------------------------------------------------------------------------------- the model alone
@pytest.mark.parametrize("total", TOTALS)
def test_the_permutation_is_a_bijection(total):
    for ek in KEYS:
        assert sorted(mm.perm(ek, total, m) for m in range(total)) == list(range(total)), (total, ek)


def _cells(counts, n, p):
    """The largest distance of a cell from its expectation n * p, in binomial standard deviations."""
    sd = (n * p * (1 - p)) ** 0.5
    return max(abs(c - n * p) / sd for c in counts)


def _uniformity(perm_rows):
    """perm_rows(s, total, epochs, positions) -> int array [epochs, positions] under ek = SM(s, e).  The worst cell over the
    issue's four statistics and the seeds s = 0 .. 5."""
    worst = 0.0
    for s in range(6):
        for total, epochs in ((8, 4096), (5, 4000), (3, 3000)):
            got = perm_rows(s, total, epochs, 1)[:, 0]
            worst = max(worst, _cells(np.bincount(got, minlength=total), epochs, 1.0 / total))
        got = perm_rows(s, 4, 4800, 2)
        assert (got[:, 0] != got[:, 1]).all()
        pairs = np.bincount(got[:, 0] * 4 + got[:, 1], minlength=16)
        cells = [pairs[a * 4 + b] for a in range(4) for b in range(4) if a != b]
        assert len(cells) == 12 and sum(cells) == 4800
        worst = max(worst, _cells(cells, 4800, 1.0 / 12))
    return worst


def _model_rows(s, total, epochs, positions):
    return np.array([[mm.perm(mm.sm(s, e), total, m) for m in range(positions)] for e in range(epochs)], np.int64)


def test_the_permutation_is_uniform_over_epochs():
    """Position 0 of total = 8 / 5 / 3 and the ordered pair (perm(0), perm(1)) of total = 4, over the epochs of six seeds: no
    cell further than 5 binomial standard deviations from its expectation.  The seeds are fixed: the test is deterministic."""
    worst = _uniformity(_model_rows)
    print(f"worst cell: {worst:.2f} standard deviations")
    assert worst <= SIGMA


@pytest.mark.parametrize("N,L", SHAPES)
def test_an_epoch_hits_every_selected_slot_exactly_once(N, L):
    a = mm.rollout_arrays(100 + N * 131 + L, N, L)
    live = np.arange(L)[:, None] >= L - np.clip(a["len"], 0, L)[None, :]
    for which, want in ((mm.LIVE, live), (mm.BOOT, live & ((a["ends"] & 8) != 0))):
        model = mm.Model(N, 7)
        total = model.select(which, a["len"], a["ends"], L)
        assert total == int(want.sum())
        tt, nn = np.nonzero(want)
        for permute in (False, True):
            got = model.take(which, permute, a["len"], a["ends"], L, 0, total + 3)
            assert got["valid"].tolist() == [1] * total + [0] * 3
            assert sorted(got["slot"][:total].tolist()) == sorted((tt * N + nn).tolist())             # LIVE == nonzero(live) as a set
            if total:
                assert (got["slot"][total:] == got["slot"][:3]).all(), "positions past total wrap"
                assert (got["env"] == got["slot"] % N).all()
            else:
                assert (got["slot"] == -1).all() and not got["env"].any()
        order = model.take(which, False, a["len"], a["ends"], L, 0, total)["slot"]
        assert order.tolist() == sorted(order.tolist(), key=lambda e: (e % N, e // N)), "the list is env-major, ascending t"


def test_len_outside_its_range_is_clamped():
    N, L = 5, 4
    ends = np.full((L, N), 8, np.uint8)
    model = mm.Model(N, 0)
    assert model.select(mm.LIVE, np.array([-3, 9, 0, 4, 2], np.int32), ends, L) == 0 + 4 + 0 + 4 + 2
    assert model.off[mm.LIVE].tolist() == [0, 0, 4, 4, 8, 10]
    assert model.select(mm.BOOT, np.array([-3, 9, 0, 4, 2], np.int32), ends, L) == 10


def test_consecutive_selects_shuffle_anew_and_the_lists_have_keys_of_their_own():
    N, L = 9, 7
    a = mm.rollout_arrays(5, N, L)
    model = mm.Model(N, 3)
    orders = []
    for _ in range(3):
        total = model.select(mm.LIVE, a["len"], a["ends"], L)
        orders.append(tuple(model.take(mm.LIVE, True, a["len"], a["ends"], L, 0, total)["slot"].tolist()))
    assert len(set(orders)) == 3 and len({tuple(sorted(o)) for o in orders}) == 1
    assert model.calls == [3, 0] and model.base[0] != model.base[1]
    again = mm.Model(N, 3)                          # the same seed: the same epochs
    again.select(mm.LIVE, a["len"], a["ends"], L)
    assert tuple(again.take(mm.LIVE, True, a["len"], a["ends"], L, 0, len(orders[0]))["slot"].tolist()) == orders[0]
    other = mm.Model(N, 4)
    other.select(mm.LIVE, a["len"], a["ends"], L)
    assert tuple(other.take(mm.LIVE, True, a["len"], a["ends"], L, 0, len(orders[0]))["slot"].tolist()) != orders[0]


def test_mismatched_arrays_are_invalid_rather_than_wrong():
    """take with other len / ends than select saw: the rows whose r-th slot no longer exists are slot -1, env 0, valid 0."""
    N, L = 6, 5
    a = mm.rollout_arrays(11, N, L)
    a["len"][:] = [5, 3, 0, 5, 2, 4]
    for which in (mm.LIVE, mm.BOOT):
        model = mm.Model(N, 1)
        total = model.select(which, a["len"], np.full((L, N), 8, np.uint8), L)
        assert total == 19
        got = model.take(which, False, np.array([1, 3, 0, 5, 0, 4], np.int32), np.full((L, N), 8, np.uint8), L, 0, total)
        lost = np.array([0, 1, 1, 1, 1] + [0] * 3 + [0] * 5 + [1, 1] + [0] * 4, bool)
        assert ((got["slot"] == -1) == lost).all() and (got["valid"] == ~lost).all() and not got["env"][lost].any()
    model = mm.Model(N, 1)
    total = model.select(mm.BOOT, a["len"], np.full((L, N), 8, np.uint8), L)
    got = model.take(mm.BOOT, False, a["len"], np.zeros((L, N), np.uint8), L, 0, total)
    assert (got["slot"] == -1).all() and not got["valid"].any()


def test_scatter_skips_what_it_must():
    dst = np.full((3, 4), -7.5, np.float32)
    got = mm.scatter(np.array([0, -1, 12, 11, 5, 7], np.int32), np.array([1, 1, 1, 1, 0, 1], np.uint8), np.arange(6, dtype=np.float32) + 1, dst)
    want = dst.copy()
    want.reshape(-1)[[0, 11, 7]] = [1, 4, 6]
    assert np.array_equal(got, want) and (dst == -7.5).all()


# ---------------------------------------------------------------------------------------------- the harness
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "minibatch_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "minibatch_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "minibatch_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
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
    for total in TOTALS:                           # the permutation, every total and key of the bijection test
        for ek in KEYS:
            got = [r[0] for r in _run(binary, tmp_path, [0, *_u64(ek), total])]
            assert got == [mm.perm(ek, total, m) for m in range(total)], (total, ek)
    for seed in (0, 3, mm.M64):                    # the keys
        for which in (mm.LIVE, mm.BOOT):
            for calls in (0, 1, 5):
                (bh, bl, kh, kl), = _run(binary, tmp_path, [3, *_u64(seed), which, calls])
                model = mm.Model(1, seed)
                assert (bh << 32) | bl == model.base[which] and (kh << 32) | kl == mm.sm(model.base[which], calls)
    for N, L in SHAPES:                            # the counts and the takes, matched and mismatched
        a = mm.rollout_arrays(100 + N * 131 + L, N, L)
        b = mm.rollout_arrays(900 + N * 131 + L, N, L)
        for which in (mm.LIVE, mm.BOOT):
            counts = [r[0] for r in _run(binary, tmp_path, [1, which, N, L, *a["len"].tolist(), *a["ends"].reshape(-1).tolist()])]
            model = mm.Model(N, 9)
            total = model.select(which, a["len"], a["ends"], L)
            assert counts == np.diff(model.off[which]).tolist() and sum(counts) == total
            for permute in (0, 1):
                for first, S in ((0, 1), (max(total - 2, 0), 5), (0, 2 * total + 3), (total + 1, 4)):
                    for arrays in (a, b):
                        got = _run(binary, tmp_path, [2, which, permute, N, L, first, S, *_u64(model.key[which]), *model.off[which].tolist(),
                                                      *arrays["len"].tolist(), *arrays["ends"].reshape(-1).tolist()])
                        want = model.take(which, bool(permute), arrays["len"], arrays["ends"], L, first, S)
                        assert [r[0] for r in got] == want["slot"].tolist() and [r[1] for r in got] == want["env"].tolist()
                        assert [r[2] for r in got] == want["valid"].tolist(), (N, L, which, permute, first, S)

    def rows(s, total, epochs, positions):         # the uniformity statistic on the harness's own output
        got = np.array(_run(binary, tmp_path, [4, s, total, epochs, positions]), np.int64)
        assert got.shape == (epochs, positions)
        return got
    assert np.array_equal(rows(2, 4, 4800, 2), _model_rows(2, 4, 4800, 2))
    assert _uniformity(rows) <= SIGMA


def test_host_side_of_the_lists_and_the_permutation(harness, tmp_path):
    _check_harness(harness, tmp_path)


def test_host_side_of_the_lists_and_the_permutation_under_sanitizers(harness_san, tmp_path):
    _check_harness(harness_san, tmp_path)
