"""CPU: include/agx_vtrace.h (V-trace over a gathered rollout) <-> libagx.so's export <-> active_gym/vtrace.py; the refusals that
need no GPU; the fold on hand-written cases and its stated properties (tests/vtrace_model.py); the float32 model against the
paper's definition in float64 within a derived bound; the __host__ side of csrc/agx_vtrace_math.h (tests/vtrace_harness.cpp),
plain and under the host's sanitizers, against the model bit for bit; and BehaviourLog on CPU tensors."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import limit_cases as lc
import rollout_model as ro
import vtrace_model as vm
from steplog_model import F32, TERMINATED, TRUNCATED, bits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_vtrace.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAME = "agx_vtrace_returns"
CUT, BOOT = ro.CUT, ro.BOOT
ONE = (1.0, 1.0, 1.0)


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------------------------------------- surface
def test_header_declares_exactly_the_one_entry_point():
    src = open(HEADER).read()
    assert re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M) == [NAME]
    assert dict(re.findall(r"^#define\s+AGX_VTRACE_([A-Z_]+)\s+(\d+)\b", src, flags=re.M)) == {"LIMIT": "4096"}
    assert vm.BOOT == BOOT == 8 and vm.TERMINATED == TERMINATED == 1 and vm.BREAK == TERMINATED | TRUNCATED | CUT == 7
    # the fold is stated in full
    for line in ("td     = fadd(fadd(reward[t], fmul(gamma, nv)), -value[t])", "cc     = fmul(lambda, vmin(rho[t], c_bar))",
                 "A      = fadd(fmul(vmin(rho[t], rho_bar), td), fmul(fmul(gamma, cc), carry))", "vs[t]     = fadd(A, value[t])"):
        assert line in src, line


def test_header_stands_apart_from_the_rollout_header():
    """tests/test_rollout_cpu.py allows the lowercase name of the rollout entry points in one header only: this one includes
    agx_history.h alone and states the bits it reads as numbers."""
    src = open(HEADER).read()
    assert "agx_rollout" not in src
    assert re.findall(r'^#include\s+"([^"]+)"', src, flags=re.M) == ["agx_history.h"]
    assert "AGX_ROLLOUT_BOOT" in src and "AGX_STEP_TERMINATED" in src


def test_entry_point_is_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    assert hasattr(handle, NAME)
    from active_gym import vtrace as vt
    assert list(vt.SIGNATURES) == [NAME]
    res, args = vt.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 16 and args[1] is ctypes.c_int32 and args[8:13] == [ctypes.c_float] * 5
    assert all(a is ctypes.c_void_p for a in args[:1] + args[2:8] + args[13:])
    vt.lib()                                       # binds the signature: AttributeError if it is not exported
    import active_gym
    assert active_gym.VTrace is vt.VTrace and active_gym.BehaviourLog is vt.BehaviourLog


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_vtrace.h") in deps
    for f in ("agx_k13_vtrace.h", "agx_vtrace_impl.h", "agx_vtrace_math.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_bindings_are_untouched():
    """V-trace is additive: no older binding grew, the rollout binding is the two names it was, the ABI version stays 2."""
    from active_gym import _native as nat
    from active_gym import augment, glimpse, history, native_hostout, native_loop, priority, replay, rollout, sequence, steplog
    sizes = [len(m.SIGNATURES) for m in (nat, native_loop, history, glimpse, replay, steplog, priority, augment, sequence)]
    assert sizes == [28, 6, 8, 1, 5, 6, 8, 5, 3] and len(native_hostout.SIGNATURES) == 6
    assert sorted(rollout.SIGNATURES) == ["agx_rollout_gae", "agx_rollout_gather"]
    assert [len(rollout.SIGNATURES[n][1]) for n in sorted(rollout.SIGNATURES)] == [12, 9]
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2


def test_a_null_handle_is_invalid_before_anything_else():
    """The handle is the first check (N comes from it), so it is named whatever else is wrong."""
    from active_gym import _native as nat
    from active_gym import vtrace as vt
    _build_mod().build()
    lib = vt.lib()
    buf = (ctypes.c_int64 * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for L, out, bar in ((4, ptr, 1.0), (0, ptr, 1.0), (4, None, 1.0), (5000, None, -1.0), (4, ptr, float("nan"))):
        assert lib.agx_vtrace_returns(None, L, ptr, ptr, ptr, ptr, None, ptr, 0.99, 1.0, bar, bar, bar, out, ptr, None) == nat.E_INVALID
        assert "agx_vtrace_returns: null argument (h)" in nat.last_error(None)


def test_python_refusals_need_no_gpu():
    from active_gym import vtrace as vt
    from active_gym.vector import AtariVecEnv
    assert vt.check_bars(1.0, 0.5, float("inf")) == (1.0, 0.5, float("inf"))
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        for at, name in enumerate(("rho_bar", "c_bar", "pg_rho_bar")):
            bars = [1.0, 1.0, 1.0]
            bars[at] = bad
            with pytest.raises(ValueError, match=f"{name} must be > 0"):
                vt.check_bars(*bars)
    env = object.__new__(AtariVecEnv)              # (class defaults only: steplog and history are None)
    with pytest.raises(ValueError, match="rollout_vtrace needs a step log"):
        env.rollout_vtrace({}, None, None, None)
    with pytest.raises(ValueError, match="behaviour_log needs a frame history"):
        env.behaviour_log()

    class Closed:
        history, pipe, device, num_envs, payload_bytes = None, None, None, 4, 0

        def _live(self):
            raise RuntimeError("the step log or its history is closed")

    v = vt.VTrace(Closed())
    with pytest.raises(RuntimeError, match="closed"):              # use after the log or its history is closed
        v.returns({}, None, None, None)
    with pytest.raises(ValueError, match="c_bar must be > 0"):     # the levels are refused before anything is looked at
        v.returns({}, None, None, None, c_bar=0.0)
    with pytest.raises(ValueError, match="width must be"):
        vt.BehaviourLog(None, 0)


# ---------------------------------------------------------------------------------------------- the fold, by hand
def _col(x, dt):
    return np.asarray(x, dt)[:, None]


def _fold(ends, reward, value, boot, rho, gamma, lam, bars=ONE, length=None):
    L = len(ends)
    vs, pg = vm.vtrace(np.array([L if length is None else length], np.int32), _col(reward, F32), _col(ends, np.uint8), _col(value, F32),
                       None if boot is None else _col(boot, F32), _col(rho, F32), gamma, lam, bars)
    return vs[:, 0].tolist(), pg[:, 0].tolist()


R, V, B, H = [1.0, 2.0, 3.0], [0.5, 0.25, 1000.0], [9.0, 2.0, 4.0], [0.5, 0.5, 0.5]       # every figure below is exact in float32
NAN = float("nan")

# name: (ends, reward, value, boot, rho, gamma, lambda, bars, len, vs, pg_adv).  The value of slot 2 is 1000 and belongs to
# another episode wherever slot 1 ends one: it must not reach slot 1 or slot 0.
HAND = {
    "truncated mid-rollout": ([0, TRUNCATED | BOOT, BOOT], R, V, B, H, 1.0, 1.0, ONE, 3, [1.8125, 2.125, 503.5], [1.3125, 1.875, -496.5]),
    "cut mid-rollout": ([0, CUT | BOOT, BOOT], R, V, B, H, 1.0, 1.0, ONE, 3, [1.8125, 2.125, 503.5], [1.3125, 1.875, -496.5]),
    "terminated mid-rollout": ([0, TERMINATED, BOOT], R, V, [9.0, 9.0, 4.0], H, 1.0, 1.0, ONE, 3, [1.3125, 1.125, 503.5], [0.8125, 0.875, -496.5]),
    # inside one episode: slot 1 reads value[2] = 1000 and carries slot 2's A = 0.5 (3 + 4 - 1000)
    "one episode": ([0, 0, BOOT], R, V, B, H, 1.0, 1.0, ONE, 3,
                    [0.5 + 0.5 * 0.75 + 0.5 * 252.625, 0.25 + 252.625, 503.5], [0.5 * (1 + (0.25 + 252.625) - 0.5), 0.5 * (2 + (1000 - 496.5) - 0.25), -496.5]),
    "terminated at the newest slot": ([0, 0, TERMINATED], R, [0.5, 0.25, 0.125], B, H, 1.0, 1.0, ONE, 3,
                                      [0.5 + 0.375 + 0.5 * 1.65625, 0.25 + 1.65625, 1.5625], [0.5 * (1 + 1.90625 - 0.5), 0.5 * (2 + 1.5625 - 0.25), 1.4375]),
    "padded slots are zero": ([0, 0, BOOT], [NAN, 2.0, 3.0], [NAN, 0.25, 1000.0], B, [NAN, 0.5, 0.5], 1.0, 1.0, ONE, 2,
                              [0.0, 0.25 + 252.625, 503.5], [0.0, 0.5 * (2 + (1000 - 496.5) - 0.25), -496.5]),
    "no boot buffer reads as zero": ([0, TRUNCATED | BOOT, BOOT], R, V, None, H, 1.0, 1.0, ONE, 3,
                                     [0.5 + 0.375 + 0.5 * 0.875, 0.25 + 0.875, 1000 - 498.5], [0.5 * (1 + (0.25 + 0.875) - 0.5), 0.875, -498.5]),
    "L = 1": ([BOOT], [3.0], [1000.0], [4.0], [0.5], 1.0, 1.0, ONE, 1, [503.5], [-496.5]),
    "len = 0": ([0, 0, BOOT], R, V, B, H, 1.0, 1.0, ONE, 0, [0.0] * 3, [0.0] * 3),
    # the three levels act on their own ratio: rho = 4 is cut to 2 in td, to 0.5 in the trace and to 1 in the policy gradient
    "three levels": ([0, BOOT], [1.0, 2.0], [0.5, 0.25], [9.0, 4.0], [4.0, 4.0], 1.0, 1.0, (2.0, 0.5, 1.0), 2,
                     [0.5 + 2 * 0.75 + 0.5 * 11.5, 0.25 + 2 * 5.75], [1 + (0.25 + 11.5) - 0.5, 2 + 4 - 0.25]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_fold_on_hand_written_cases(name):
    ends, reward, value, boot, rho, gamma, lam, bars, length, vs, pg = HAND[name]
    assert _fold(ends, reward, value, boot, rho, gamma, lam, bars, length) == (vs, pg)


def test_fold_rounds_after_every_operation():
    """Every product and sum is rounded to float32 before the next: a fused or double-precision fold differs on these figures."""
    gamma, lam = F32(0.99), F32(0.95)
    r, v, b, w = F32(0.2), F32(0.4), F32(0.7), F32(0.6)
    vs, pg = _fold([0, BOOT], [r, r], [v, v], [b, b], [w, w], gamma, lam)
    td1 = F32(F32(r + F32(gamma * b)) - v)
    a1 = F32(w * td1)
    td0 = F32(F32(r + F32(gamma * v)) - v)
    a0 = F32(F32(w * td0) + F32(F32(gamma * F32(lam * w)) * a1))
    assert vs == [float(F32(a0 + v)), float(F32(a1 + v))]
    assert pg == [float(F32(w * F32(F32(r + F32(gamma * F32(v + a1))) - v))), float(F32(w * td1))]
    wide_a1 = float(w) * (float(r) + float(gamma) * float(b) - float(v))
    wide = float(v) + float(w) * (float(r) + float(gamma) * float(v) - float(v)) + float(gamma) * float(lam) * float(w) * wide_a1
    wide_pg = float(w) * (float(r) + float(gamma) * (float(v) + wide_a1) - float(v))
    assert float(F32(wide)) != vs[0] and float(F32(wide_pg)) != pg[0]               # the figures tell the two apart


# ---------------------------------------------------------------------------------------------- the stated properties
CASES = [(N, L, 1000 * N + L) for N in vm.NS for L in vm.LS]


def _live_finite(case):
    length, reward, ends, value, boot, rho, live = case
    return np.isfinite(reward[live]).all() and np.isfinite(value[live]).all() and np.isfinite(rho[live]).all() and np.isnan(rho[~live]).all()


def test_on_policy_is_gae_bit_for_bit():
    """rho = 1 with levels 1 (and above): A and vs are rollout_model's GAE adv and ret, as bits; rho = 3 under levels 1 is cut to 1
    and gives the same bits in all three outputs."""
    for N, L, seed in CASES:
        length, reward, ends, value, boot, rho, live = vm.case(N, L, seed)
        one = np.where(live, F32(1), F32(np.nan)).astype(F32)
        for gamma, lam in ro.GAMMA_LAMBDA + ((0.99, 1.0),):
            adv, ret = ro.gae_vec(length, reward, ends, value, boot, gamma, lam)
            for bars in (ONE, (1.0, 2.5, np.inf)):
                vs, pg, A = vm.vtrace(length, reward, ends, value, boot, one, gamma, lam, bars, with_A=True)
                assert np.array_equal(bits(A), bits(adv)) and np.array_equal(bits(vs), bits(ret)), (N, L, gamma, lam, bars)
            three = vm.vtrace(length, reward, ends, value, boot, (one * F32(3)).astype(F32), gamma, lam, ONE, with_A=True)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(three, (vs, pg, A))), (N, L, gamma, lam)


def test_rho_zero_gives_the_value_back():
    for N, L, seed in CASES:
        length, reward, ends, value, boot, rho, live = vm.case(N, L, seed)
        vs, pg = vm.vtrace(length, reward, ends, value, boot, np.zeros_like(rho), 0.99, 0.95, ONE)
        assert np.array_equal(bits(vs[live]), bits(value[live])) and not pg.any() and not vs[~live].any(), (N, L)


def test_lambda_zero_and_a_vanishing_c_bar_give_the_one_step_target():
    """lam = 0, and c_bar -> 0+ (the smallest subnormal): nothing is carried, vs = V + min(rho, rho_bar) td."""
    for N, L, seed in CASES:
        length, reward, ends, value, boot, rho, live = vm.case(N, L, seed)
        rho = np.where(live, np.maximum(rho, F32(0.25)), rho).astype(F32)
        nxt = np.concatenate([value[1:], np.zeros((1, N), F32)])
        nxt[L - 1] = 0
        nv = np.where(ends & BOOT, boot, np.where(ends & TERMINATED, F32(0), nxt)).astype(F32)
        for gamma, bars in ((0.99, ONE), (0.9, (2.0, 0.5, 1.0))):
            g = F32(gamma)
            with np.errstate(all="ignore"):
                td = ((reward + (g * nv).astype(F32)).astype(F32) - value).astype(F32)
                want = ((vm.vmin(rho, F32(bars[0])) * td).astype(F32) + value).astype(F32)
            for lam, c_bar in ((0.0, bars[1]), (0.95, 2.0 ** -149)):
                vs, _ = vm.vtrace(length, reward, ends, value, boot, rho, gamma, lam, (bars[0], c_bar, bars[2]))
                assert np.array_equal(bits(vs[live]), bits(want[live])), (N, L, gamma, lam, c_bar)


def test_no_nan_of_an_unused_input_reaches_an_output():
    """boot is NaN wherever BOOT is unset, reward / value / rho are NaN in every slot that is not live, len is wild (-3, L + 7, 0,
    L, 1): every output is finite and the slots that are not live are +0.0.  A NaN rho at a LIVE slot reads as the level."""
    holes = 0
    for N, L, seed in CASES:
        case = vm.case(N, L, seed)
        length, reward, ends, value, boot, rho, live = case
        assert _live_finite(case) and (np.isnan(boot).any() or (ends & BOOT).all())
        assert {-3, L + 7, 0, L, 1} <= set(length.tolist())
        for gamma, lam, bars in vm.PARAMS:
            vs, pg = vm.vtrace(length, reward, ends, value, boot, rho, gamma, lam, bars)
            assert np.isfinite(vs).all() and np.isfinite(pg).all(), (N, L, gamma, lam, bars)
            assert not bits(vs)[~live].any() and not bits(pg)[~live].any()
        bars = (2.0, 0.5, 1.0)
        hole = live & (np.random.default_rng(seed).random((L, N)) < 0.3)
        a = vm.vtrace(length, reward, ends, value, boot, np.where(hole, F32(np.nan), rho), 0.99, 0.5, bars)
        b = vm.vtrace(length, reward, ends, value, boot, np.where(hole, F32(7), rho), 0.99, 0.5, bars)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)), (N, L)
        holes += int(hole.sum())
    assert holes > 1000


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("gamma, lam, bars", vm.PARAMS)
def test_model_against_the_definition_in_float64(gamma, lam, bars):
    """vs_s = V_s + sum_k g^(k - s) (prod c_i) rho_k td_k as the explicit sum in float64 (vtrace_model.definition), against the
    float32 fold, for every live slot: |A32 - A| <= gamma_(5 c) S, |vs32 - vs| <= (1 + u) bA + u |vs| and the bound of pg_adv, all
    derived from the operation count in vtrace_model.bounds; the worst ratio of error to bound is printed.  No slot has a non-zero
    term below 2^-100, so the bounds, which do not model underflow, leave none out."""
    worst, checked, longest = [0.0, 0.0, 0.0], 0, 0
    for N, L, seed in ((70, 130, 3), (70, 33, 4), (5, 17, 5)):
        length, reward, ends, value, boot, rho, live = vm.case(N, L, seed)
        vs, pg, A = vm.vtrace(length, reward, ends, value, boot, rho, gamma, lam, bars, with_A=True)
        d = vm.definition(length, reward, ends, value, boot, rho, gamma, lam, bars)
        assert np.array_equal(d["live"], live) and not (d["smallest"][live] < lc.TINY).any()
        for at, (got, want, bound) in enumerate(zip((A, vs, pg), (d["A"], d["vs"], d["pg"]), vm.bounds(d))):
            err, bnd = np.abs(got.astype(np.float64) - want)[live], bound[live]
            assert (err <= bnd).all(), (N, L, at, float((err / np.maximum(bnd, 1e-300)).max()))
            nz = bnd > 0
            worst[at] = max(worst[at], float((err[nz] / bnd[nz]).max()))
        checked, longest = checked + int(live.sum()), max(longest, int(d["chain"][live].max()))
    print(f"gamma = {gamma}, lambda = {lam}, levels = {bars}: {checked} live slots, longest chain {longest}; worst error / bound "
          f"A {worst[0]:.3f}, vs {worst[1]:.3f}, pg_adv {worst[2]:.3f}")
    assert checked > 3000 and longest >= 8 and max(worst) < 1


# ---------------------------------------------------------------------------------------------- the harness
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "vtrace_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "vtrace_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "vtrace_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


def _harness(binary, tmp_path, length, reward, ends, value, boot, rho, gamma, lam, bars):
    L, N = reward.shape
    tokens = [N, L, *(int(bits(F32(x))) for x in (gamma, lam, *bars)), int(boot is not None), *np.asarray(length).tolist(),
              *bits(reward).reshape(-1).tolist(), *ends.reshape(-1).tolist(), *bits(value).reshape(-1).tolist(), *bits(rho).reshape(-1).tolist()]
    if boot is not None:
        tokens += bits(boot).reshape(-1).tolist()
    path = tmp_path / "case.txt"
    path.write_text(" ".join(map(str, tokens)))
    r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([[int(x) for x in ln.split()] for ln in r.stdout.splitlines()], np.int64).astype(np.uint32).view(np.int32).reshape(L, N, 2)
    return got[..., 0], got[..., 1]


def _same_but_nan(got, want):
    """Bit-equal, except that a NaN is any NaN (the hand cases put NaN into slots that are live for no one)."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got.view(np.float32)), nan) and np.array_equal(got[~nan], bits(want)[~nan])


def _check_harness(binary, tmp_path):
    for name in sorted(HAND):
        ends, reward, value, boot, rho, gamma, lam, bars, length, vs, pg = HAND[name]
        gv, gp = _harness(binary, tmp_path, [length], _col(reward, F32), _col(ends, np.uint8), _col(value, F32),
                          None if boot is None else _col(boot, F32), _col(rho, F32), gamma, lam, bars)
        assert gv[:, 0].tolist() == bits(vs).tolist() and gp[:, 0].tolist() == bits(pg).tolist(), name
    compared = 0
    for N, L, seed in CASES:                       # the GPU cases
        length, reward, ends, value, boot, rho, live = vm.case(N, L, seed)
        runs = [(g, la, bars, boot, ends) for g, la, bars in vm.PARAMS] + [(0.99, 0.5, (2.0, 0.5, 1.0), None, (ends & 7).astype(np.uint8))]
        for gamma, lam, bars, b, e in runs:
            vs, pg = vm.vtrace(length, reward, e, value, b, rho, gamma, lam, bars)
            gv, gp = _harness(binary, tmp_path, length, reward, e, value, b, rho, gamma, lam, bars)
            assert np.array_equal(gv, bits(vs)) and np.array_equal(gp, bits(pg)), (N, L, gamma, lam, bars, b is not None)
            compared += 2 * L * N
    # a NaN rho at live slots, through the very function the kernel runs
    length, reward, ends, value, boot, rho, live = vm.case(5, 17, 1)
    holed = np.where(live & (np.arange(17)[:, None] % 3 == 0), F32(np.nan), rho).astype(F32)
    vs, pg = vm.vtrace(length, reward, ends, value, boot, holed, 0.99, 0.5, (2.0, 0.5, 1.0))
    gv, gp = _harness(binary, tmp_path, length, reward, ends, value, boot, holed, 0.99, 0.5, (2.0, 0.5, 1.0))
    assert _same_but_nan(gv, vs) and _same_but_nan(gp, pg) and np.isfinite(vs).all()
    print(f"{compared} vs / pg_adv elements compared")


def test_host_side_of_the_fold(harness, tmp_path):
    _check_harness(harness, tmp_path)


def test_host_side_of_the_fold_under_sanitizers(harness_san, tmp_path):
    _check_harness(harness_san, tmp_path)


# ---------------------------------------------------------------------------------------------- BehaviourLog on CPU tensors
class _History:
    """What a BehaviourLog takes from its history."""
    capacity, num_envs, device = 4, 3, torch.device("cpu")
    closed = False

    def _live(self):
        if self.closed:
            raise RuntimeError("the history is closed")


def test_behaviour_log_rows_wrap_and_minus_one_is_skipped():
    from active_gym import BehaviourLog
    h = _History()
    mu = BehaviourLog(h, width=2)
    assert tuple(mu.values.shape) == (4, 3, 2) and mu.values.dtype == torch.float32 and not mu.values.any()
    val = lambda step: torch.tensor([[10.0 * n + step, -(10.0 * n + step)] for n in range(3)])
    index = torch.tensor([0, 0, 0])
    for step in range(1, 7):                       # env 1 sits out step 3 (index -1); indices run past T = 4: rows are reused
        idx = index.clone()
        if step == 3:
            idx[1] = -1
        mu.write(idx, val(step))
        index = index + (idx >= 0)
    assert index.tolist() == [6, 5, 6]
    # retained: the last four indices of each env
    obs_index = torch.tensor([[2, 1, 2], [3, 2, 3], [4, 3, 4], [5, 4, 5], [-1, -1, 5]])
    got = mu.read(obs_index)
    assert tuple(got.shape) == (5, 3, 2)
    step_of = {0: lambda k: k + 1, 1: lambda k: k + 1 if k < 2 else k + 2, 2: lambda k: k + 1}      # env 1's index 2 was written in step 4
    for t in range(5):
        for n in range(3):
            k = int(obs_index[t, n])
            want = [0.0, 0.0] if k < 0 else [10.0 * n + step_of[n](k), -(10.0 * n + step_of[n](k))]
            assert got[t, n].tolist() == want, (t, n, k)
    # the [B] form with env ids
    flat = mu.read(torch.tensor([5, 4, -1, 3]), torch.tensor([0, 1, 2, 2], dtype=torch.int32))
    assert flat.tolist() == [[6.0, -6.0], [16.0, -16.0], [0.0, 0.0], [24.0, -24.0]]
    with pytest.raises(TypeError, match="int64"):
        mu.write(torch.tensor([0, 0, 0], dtype=torch.int32), val(1))
    with pytest.raises(ValueError, match="values must be float32"):
        mu.write(torch.tensor([0, 0, 0]), torch.zeros(3, 1))
    with pytest.raises(ValueError, match="obs_index must be"):
        mu.read(torch.tensor([0, 0, 0]))
    h.closed = True
    with pytest.raises(RuntimeError, match="closed"):
        mu.write(torch.tensor([0, 0, 0]), val(1))
    with pytest.raises(RuntimeError, match="closed"):
        mu.read(obs_index)


def test_behaviour_log_skip_keeps_the_row():
    """An env whose index is -1 is skipped: row 0, which -1 would otherwise be folded onto, keeps its value."""
    from active_gym import BehaviourLog
    mu = BehaviourLog(_History())
    mu.write(torch.tensor([0, 4, 8]), torch.tensor([[1.0], [2.0], [3.0]]))           # all three land in row 0
    mu.write(torch.tensor([-1, 1, -1]), torch.tensor([[7.0], [8.0], [9.0]]))
    assert mu.values[0, :, 0].tolist() == [1.0, 2.0, 3.0] and mu.values[1, :, 0].tolist() == [0.0, 8.0, 0.0]
    assert mu.read(torch.tensor([[0, 4, 8], [-1, 1, -1]]))[..., 0].tolist() == [[1.0, 2.0, 3.0], [0.0, 8.0, 0.0]]
