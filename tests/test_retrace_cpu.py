"""CPU: include/agx_retrace.h (Retrace-family Q-returns over a sequence-replay batch) <-> libagx.so's export <->
active_gym/retrace.py; the refusals that need no GPU; the stated properties of the fold on tests/retrace_model.py; and the
__host__ side of csrc/agx_retrace_math.h (tests/retrace_harness.cpp, a stand-alone program run as its own process), plain and
under the host's sanitizers, against the model bit for bit at the shapes of the GPU cases."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import retrace_model as rm
from retrace_model import F32, bits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "agx_retrace.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAME = "agx_sequence_retrace"
C_TYPES = {"agx_history *": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "const int32_t *": ctypes.c_void_p,
           "const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "uint8_t *": ctypes.c_void_p, "void *": ctypes.c_void_p}


def _build_mod():
    spec = importlib.util.spec_from_file_location("agx_build", os.path.join(REPO, "active-gym_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------------------------------------- surface
def test_header_declares_exactly_the_one_entry_point_and_states_the_rule():
    src = open(HEADER).read()
    assert re.findall(r"^AGX_API[^;(]*?\b(agx_\w+)\s*\(", src, flags=re.M) == [NAME]
    assert not re.findall(r"^#define\s+AGX_(?!RETRACE_H\b)\w+", src, flags=re.M)           # the limit is the sequence header's
    assert re.findall(r'^#include\s+"([^"]+)"', src, flags=re.M) == ["agx_history.h", "agx_sequence.h"]
    for line in ("vnext = (l + 1 < len') ? v[l + 1] : boot[b]", "carry = has(l + 1) ? fmul(c[l + 1], fsub(T[l + 1], q[l + 1])) : 0",
                 "T[l]  = fadd(reward[l], fmul(discount[l], fadd(vnext, carry)))", "has(l) = l < len' and steps[l] == 1"):
        assert line in src, line
    assert rm.SEQUENCE_LIMIT == 256


def test_prototype_matches_the_binding():
    """Parameter by parameter: the C type of the header's prototype against the ctypes type of SIGNATURES."""
    from active_gym import retrace as rt
    proto = re.search(r"AGX_API int " + NAME + r"\((.*?)\);", open(HEADER).read(), flags=re.S).group(1)
    params = [" ".join(p.split()) for p in proto.split(",")]
    kinds = [re.match(r"(.*?)(\w+)$", p).group(1).strip() for p in params]
    names = [re.match(r"(.*?)(\w+)$", p).group(2) for p in params]
    assert names == ["h", "B", "L", "time_major", "d_len", "d_steps", "d_reward", "d_discount", "d_q", "d_v", "d_c", "d_boot", "d_target", "d_td",
                     "d_valid", "stream"]
    res, args = rt.SIGNATURES[NAME]
    assert res is ctypes.c_int and args == [C_TYPES[k] for k in kinds]


def test_entry_point_is_exported_and_bound():
    handle = ctypes.CDLL(_build_mod().build())
    assert hasattr(handle, NAME)
    from active_gym import retrace as rt
    assert list(rt.SIGNATURES) == [NAME]
    rt.lib()                                       # binds the signature: AttributeError if it is not exported
    import active_gym
    assert active_gym.Retrace is rt.Retrace and active_gym.coefficients is rt.coefficients
    assert callable(active_gym.AtariVecEnv.sequence_retrace)


def test_source_hash_covers_the_new_files():
    deps = {os.path.relpath(d, REPO) for d in _build_mod().DEPS}
    assert os.path.join("include", "agx_retrace.h") in deps
    for f in ("agx_k16_retrace.h", "agx_retrace_impl.h", "agx_retrace_math.h"):
        assert os.path.join("active-gym_amd", "csrc", f) in deps, f


def test_the_older_headers_and_bindings_are_untouched():
    """The fold is additive: no older header names it, no older binding grew, the ABI version stays 2."""
    from active_gym import _native as nat
    from active_gym import minibatch, rollout, sequence, steplog, vtrace
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):
        if hdr != "agx_retrace.h":
            src = open(os.path.join(REPO, "include", hdr)).read()
            assert "retrace" not in src.lower(), hdr
    assert [len(m.SIGNATURES) for m in (nat, steplog, sequence, rollout, vtrace, minibatch)] == [28, 6, 3, 2, 1, 5]
    for mod in (nat, steplog, sequence, rollout, vtrace, minibatch):
        assert not [k for k in mod.SIGNATURES if "retrace" in k]
    _build_mod().build()
    assert nat.lib().agx_abi_version() == nat.ABI_VERSION == 2
    assert ctypes.sizeof(nat.AgxConfig) == 96


def test_null_and_out_of_range_arguments_are_invalid_before_any_hip_call():
    """Every AGX_E_INVALID names its argument, in the header's order; the argument checks come before the handle is looked at, so
    none needs a GPU, and the null handle comes after them - also at B = 0."""
    from active_gym import _native as nat
    from active_gym import retrace as rt
    _build_mod().build()
    lib = rt.lib()
    buf = (ctypes.c_int64 * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    big = (1 << 31) // 8 + 1                       # big * 8 > INT32_MAX
    order = ["length", "steps", "reward", "discount", "q", "v", "c", "target"]

    def call(B=4, L=8, **kw):
        a = {k: ptr for k in order}
        a.update(kw)
        return lib.agx_sequence_retrace(None, B, L, 0, *[a[k] for k in order[:7]], None, a["target"], None, None, None)

    cases = [(dict(L=0), "L must be 1 .. 256"), (dict(L=257, B=-1), "L must be 1 .. 256"), (dict(B=-1, steps=None), "B must be >= 0"),
             (dict(B=big, q=None), "B * L"), (dict(), "null argument (h)"), (dict(B=0, **{k: None for k in order}), "null argument (h)")]
    cases += [({k: None}, f"null buffer (d_{'len' if k == 'length' else k})") for k in order]
    cases.append((dict(steps=None, target=None), "null buffer (d_steps)"))
    for kw, named in cases:
        assert call(**kw) == nat.E_INVALID, kw
        assert named in nat.last_error(None) and NAME in nat.last_error(None), (kw, nat.last_error(None))


def test_python_refusals_need_no_gpu():
    from active_gym import retrace as rt
    from active_gym.vector import AtariVecEnv
    assert [rt.check_kind(k) for k in rt.KINDS] == ["retrace", "qlambda", "tree"]
    for bad in ("vtrace", None, 0):
        with pytest.raises(ValueError, match="kind must be one of"):
            rt.check_kind(bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam must be 0 .. 1"):
            rt.check_lambda(bad)
    B, L = 3, 5
    good = dict(length=torch.zeros(B, dtype=torch.int32), steps=torch.zeros((B, L), dtype=torch.int32), ret=torch.zeros((B, L)), discount=torch.zeros((B, L)))
    assert rt.check_batch(good) == (B, L)
    assert rt.check_batch({k: (t.T.contiguous() if t.dim() == 2 else t) for k, t in good.items()}, time_major=True) == (B, L)
    bads = [({}, "no tensor 'length'"), (dict(good, steps=None), "no tensor 'steps'"), (dict(good, length=good["length"].long()), "length'\\] must be int32"),
            (dict(good, steps=good["steps"].long()), "steps'\\] must be int32"), (dict(good, steps=good["steps"][0]), "steps'\\] must be int32 \\[B, L\\]"),
            (dict(good, ret=good["ret"].double()), "'ret'\\] must be float32"), (dict(good, discount=good["discount"][:, :2]), "'discount'\\] must be float32"),
            (dict(good, steps=torch.zeros((B, 300), dtype=torch.int32)), "L must be 1 .. 256")]
    for batch, named in bads:
        with pytest.raises(ValueError, match=named):
            rt.check_batch(batch)
    with pytest.raises(ValueError, match="pass the time_major the batch was gathered with"):
        rt.check_batch(good, time_major=True)
    with pytest.raises(ValueError, match="out must be a dict"):
        rt.check_outputs({"target": None}, (B, L))
    with pytest.raises(ValueError, match="out\\['valid'\\] must be"):
        rt.check_outputs(dict(target=torch.zeros((B, L)), td=torch.zeros((B, L)), valid=torch.zeros((B, L))), (B, L))

    class Log:                                     # what a Retrace takes from its step log: nothing is looked at before the checks
        history, pipe, device = None, None, None

        def _live(self):
            raise RuntimeError("the step log or its history is closed")

    r = rt.Retrace(Log())
    z = torch.zeros((B, L))
    for args, named in (((z, z, z[:2]), "c must be float32"), ((z.double(), z, z), "q must be float32"), ((z, z.T, z), "v must be float32"),
                        ((z, z, z, torch.zeros(B + 1)), "boot must be float32")):
        with pytest.raises(ValueError, match=named):
            r.targets(good, *args)
    with pytest.raises(RuntimeError, match="closed"):                  # use after the log or its history is closed
        r.targets(good, z, z, z)
    env = object.__new__(AtariVecEnv)              # (class defaults only: steplog is None)
    with pytest.raises(ValueError, match="sequence_retrace needs a step log"):
        env.sequence_retrace({}, None, None, None)


def test_coefficients_are_the_three_families():
    from active_gym import coefficients
    lp, lm = torch.log(torch.tensor([[0.5, 0.25], [0.9, 0.1]])), torch.log(torch.tensor([[0.25, 0.5], [0.9, 0.4]]))
    assert torch.allclose(coefficients(lp, lm, 0.8), 0.8 * torch.tensor([[1.0, 0.5], [1.0, 0.25]]))
    assert torch.equal(coefficients(lp, None, 0.8, "qlambda"), torch.full((2, 2), 0.8))
    assert torch.allclose(coefficients(lp, lam=0.5, kind="tree"), 0.5 * torch.tensor([[0.5, 0.25], [0.9, 0.1]]))
    assert coefficients(lp.double(), lm.double()).dtype == torch.float32
    with pytest.raises(ValueError, match="needs logp_mu"):
        coefficients(lp)
    with pytest.raises(ValueError, match="needs logp_mu"):
        coefficients(lp, lm[:1])
    with pytest.raises(ValueError, match="kind must be one of"):
        coefficients(lp, lm, kind="sarsa")


# ---------------------------------------------------------------------------------------------- the fold, by hand
def _one(length, steps, reward, discount, q, v, c, boot=None):
    row = lambda x, dt: np.asarray(x, dt)[None, :]
    t, d, ok = rm.retrace(np.array([length], np.int32), row(steps, np.int32), row(reward, F32), row(discount, F32), row(q, F32), row(v, F32), row(c, F32),
                          None if boot is None else np.array([boot], F32))
    return t[0].tolist(), d[0].tolist(), ok[0].tolist()


def test_fold_on_hand_written_cases():
    """Every figure is exact in float32."""
    R, D, Q, V, C = [1.0, 2.0, 4.0], [0.5, 0.5, 0.5], [0.25, 0.5, 1.0], [8.0, 16.0, 32.0], [1.0, 0.5, 0.25]
    # a whole sequence: T2 = 4 + .5 * 64 = 36, td2 = 35; T1 = 2 + .5 (32 + .25 * 35) = 22.375; T0 = 1 + .5 (16 + .5 * 21.875) = 14.46875
    assert _one(3, [1, 1, 1], R, D, Q, V, C, 64.0) == ([14.46875, 22.375, 36.0], [14.21875, 21.875, 35.0], [1, 1, 1])
    # no boot buffer reads as 0
    assert _one(3, [1, 1, 1], R, D, Q, V, C)[0][2] == 4.0
    # len = 2: step 2 is padding, step 1 bootstraps from boot and not from v[2]
    assert _one(2, [1, 1, 1], R, D, Q, V, C, 64.0) == ([1 + .5 * (16 + .5 * 33.5), 34.0, 0.0], [1 + .5 * (16 + .5 * 33.5) - .25, 33.5, 0.0], [1, 1, 0])
    # a step without a row in the middle: it is invalid, step 0 reads its v but carries nothing over it
    assert _one(3, [1, 0, 1], R, D, Q, V, C, 64.0) == ([9.0, 0.0, 36.0], [8.75, 0.0, 35.0], [1, 0, 1])
    # steps == 2 (a batch gathered with nstep = 2) is no row either
    assert _one(3, [2, 2, 2], R, D, Q, V, C, 64.0) == ([0.0] * 3, [0.0] * 3, [0] * 3)
    # a terminated last step: discount 0 cuts the bootstrap
    assert _one(3, [1, 1, 1], R, [0.5, 0.5, 0.0], Q, V, C, 64.0)[0][2] == 4.0
    assert _one(0, [1, 1, 1], R, D, Q, V, C, 64.0) == ([0.0] * 3, [0.0] * 3, [0] * 3)


def test_fold_rounds_after_every_operation():
    """Every product and sum is rounded to float32 before the next: a fused or double-precision fold differs on these figures."""
    r, d, q, v, c, boot = F32(0.2), F32(0.99), F32(0.4), F32(0.7), F32(0.6), F32(0.3)
    t, e, ok = _one(2, [1, 1], [r, r], [d, d], [q, q], [v, v], [c, c], boot)
    T1 = F32(r + F32(d * F32(boot + F32(0))))
    td1 = F32(T1 - q)
    T0 = F32(r + F32(d * F32(v + F32(c * td1))))
    assert t == [float(T0), float(T1)] and e == [float(F32(T0 - q)), float(td1)] and ok == [1, 1]
    wide1 = float(r) + float(d) * float(boot)
    wide0 = float(r) + float(d) * (float(v) + float(c) * (wide1 - float(q)))
    assert float(F32(wide0)) != t[0]               # the figures tell the two apart


# ---------------------------------------------------------------------------------------------- the stated properties
SHAPES = [(B, L) for B in rm.BS for L in rm.LS]
SMALL = [(B, L) for B in (3, 65) for L in (1, 2, 37, 65)]


def test_zero_coefficients_give_the_one_step_target_to_the_bit():
    """c == 0: target = reward + discount * vnext at every step with a row, with vnext = v[l + 1] inside the sequence and boot behind it."""
    for B, L in SMALL:
        k = rm.case(B, L, 7 * B + L, c_mode="zero")
        target, td, valid = rm.retrace(**k)
        n = np.clip(k["length"], 0, L)
        nxt = np.concatenate([k["v"][:, 1:], np.zeros((B, 1), F32)], 1)
        vnext = np.where(np.arange(1, L + 1)[None, :] < n[:, None], nxt, k["boot"][:, None]).astype(F32)
        with np.errstate(all="ignore"):
            want = (k["reward"] + (k["discount"] * (vnext + F32(0)).astype(F32)).astype(F32)).astype(F32)
        has = rm.has_row(k["length"], k["steps"])
        assert has.any() and np.array_equal(valid, has.astype(np.uint8))
        with np.errstate(all="ignore"):
            want_td = (want - k["q"]).astype(F32)
        assert np.array_equal(bits(target)[has], bits(want)[has]) and np.array_equal(bits(td)[has], bits(want_td)[has])


def test_a_step_without_a_row_is_zero_whatever_its_inputs_hold():
    """The cases hold inf / NaN past the sequence's end and at rowless steps inside it: no output is anything but +0.0 there, every
    output is finite, and nothing changes when those inputs are replaced by other garbage."""
    specials = dict.fromkeys(("reward", "discount", "q", "c", "v"), 0)
    for B, L in SMALL:
        k = rm.case(B, L, 11 * B + L)
        has = rm.has_row(k["length"], k["steps"])
        inside = np.arange(L)[None, :] < np.clip(k["length"], 0, L)[:, None]
        for name in ("reward", "discount", "q", "c", "v"):
            specials[name] += int((~np.isfinite(k[name][~inside if name == "v" else ~has])).sum())
        out = rm.retrace(**k)
        assert all(np.isfinite(x).all() and not bits(x.astype(F32))[~has].any() for x in out)
        other = dict(k)
        for name in ("reward", "discount", "q", "c"):
            other[name] = np.where(has, k[name], F32(-7.5)).astype(F32)
        other["v"] = np.where(inside, k["v"], F32(1e30)).astype(F32)
        assert all(np.array_equal(bits(a.astype(F32)), bits(b.astype(F32))) for a, b in zip(out, rm.retrace(**other)))
    assert min(specials.values()) > 100            # the cases do hold inf / NaN in every input where no row reads it


def test_a_chain_never_crosses_a_step_without_a_row():
    """Whatever lies at and behind a rowless step l - but its v, which the rule lets step l - 1 read - cannot reach a step before
    it: the steps before l are those of the sequence cut to l + 1 steps that bootstraps from v[l]."""
    checked = 0
    for B, L in ((3, 37), (65, 65)):
        k = rm.case(B, L, 13 * B + L, c_mode="one")
        has = rm.has_row(k["length"], k["steps"])
        full = rm.retrace(**k)
        for b in range(B):
            holes = [l for l in range(1, int(np.clip(k["length"][b], 0, L))) if not has[b, l]]
            if not holes:
                continue
            l = holes[0]
            cut = {name: k[name][b:b + 1, :l] for name in rm.ARRAYS}
            part = rm.retrace(np.array([l], np.int32), boot=k["v"][b:b + 1, l], **cut)
            assert all(np.array_equal(bits(p[0].astype(F32)), bits(f[b, :l].astype(F32))) for p, f in zip(part, full)), (B, L, b, l)
            checked += 1
    assert checked > 20


def test_boot_is_read_iff_the_sequence_is_full_and_its_last_step_has_a_row():
    """On batches as the gather writes them: the last step of a sequence that stops short of L has no row (it is the terminal
    observation's own step, or the newest observation, whose step is not recorded yet), so nothing bootstraps behind it."""
    for B, L in SMALL:
        k = rm.case(B, L, 17 * B + L)
        n = np.clip(k["length"], 0, L)
        for b in range(B):
            if 0 < n[b] < L:
                k["steps"][b, n[b] - 1] = 0
        has = rm.has_row(k["length"], k["steps"])
        a, b = rm.retrace(**k), rm.retrace(**dict(k, boot=(k["boot"] + F32(1000)).astype(F32)))
        moved = np.array([not np.array_equal(bits(a[0][i]), bits(b[0][i])) for i in range(B)])
        reads = (np.clip(k["length"], 0, L) == L) & has[:, L - 1] & (k["discount"][:, L - 1] != 0)
        assert np.array_equal(moved, reads), (B, L)
        assert not moved[~((k["length"] >= L) & has[:, L - 1])].any()
    # NaN in boot shows only there, too
    k = rm.case(65, 37, 5)
    for b in range(65):
        if 0 < k["length"][b] < 37:
            k["steps"][b, k["length"][b] - 1] = 0
    t = rm.retrace(**dict(k, boot=np.full(65, np.nan, F32)))[0]
    full = (k["length"] >= 37) & (k["steps"][:, -1] == 1)
    assert np.isnan(t[full, -1]).all() and np.isfinite(t[~full]).all()


def test_steps_other_than_one_and_wild_lengths():
    for B, L in SMALL:
        k = rm.case(B, L, 19 * B + L)
        two = dict(k, steps=np.full((B, L), 2, np.int32))
        assert not any(x.any() for x in rm.retrace(**two))
        assert set(k["length"].tolist()) >= ({L, 0} if B == 3 else {L, 0, L + 7, -3})
        clamped = dict(k, length=np.clip(k["length"], 0, L).astype(np.int32))
        assert all(np.array_equal(bits(a.astype(F32)), bits(b.astype(F32))) for a, b in zip(rm.retrace(**k), rm.retrace(**clamped)))


# ---------------------------------------------------------------------------------------------- the harness
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "retrace_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "retrace_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "retrace_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


def _harness(binary, tmp_path, k, time_major=False, boot=True, td=True, valid=True):
    B, L = k["steps"].shape
    k = rm.transposed(k) if time_major else k
    tokens = [B, L, int(time_major), int(boot), int(td), int(valid), *k["length"].tolist(), *k["steps"].reshape(-1).tolist()]
    for name in ("reward", "discount", "q", "v", "c"):
        tokens += bits(k[name]).reshape(-1).tolist()
    if boot:
        tokens += bits(k["boot"]).tolist()
    path = tmp_path / "case.txt"
    path.write_text(" ".join(map(str, tokens)))
    r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array(r.stdout.split(), np.int64).reshape((L, B, 3) if time_major else (B, L, 3))
    got = got.transpose(1, 0, 2) if time_major else got
    return got[..., 0].astype(np.uint32).view(np.int32).view(F32), got[..., 1].astype(np.uint32).view(np.int32).view(F32), got[..., 2].astype(np.uint8)


def _check_harness(binary, tmp_path):
    compared = 0
    for B, L in SHAPES:                            # the GPU cases' shapes
        k = rm.case(B, L, 1000 * B + L, live_specials=(B + L) % 2 == 0)
        tm, boot = (B + L) % 3 == 0, (B * L) % 5 != 0
        target, td, valid = rm.retrace(**(k if boot else dict(k, boot=None)))
        gt, gd, gv = _harness(binary, tmp_path, k, tm, boot)
        assert rm.same(gt, target) and rm.same(gd, td) and np.array_equal(gv, valid), (B, L, tm, boot)
        compared += 3 * B * L
    k = rm.case(65, 37, 3)                         # the outputs that may be left out keep their sentinel
    gt, gd, gv = _harness(binary, tmp_path, k, False, True, td=False, valid=False)
    assert rm.same(gt, rm.retrace(**k)[0]) and (bits(gd) == -1).all() and (gv == 255).all()
    print(f"{compared} target / td / valid elements compared")


def test_host_side_of_the_fold(harness, tmp_path):
    _check_harness(harness, tmp_path)


def test_host_side_of_the_fold_under_sanitizers(harness_san, tmp_path):
    _check_harness(harness_san, tmp_path)
