"""CPU: what the scenarios of tests/vtrace_limit_cases.py are there for, pinned on the models alone - so that a seed that drifts
fails here and not silently on the device (tests/test_gpu_vtrace_limits.py) - the float32 model against the paper's definition in
float64 at L = AGX_VTRACE_LIMIT, and the __host__ side of csrc/agx_vtrace_math.h (tests/vtrace_harness.cpp) on the special floats
and at the limit, plain and under the host's sanitizers, against the model bit for bit."""
import os

import numpy as np
import pytest

import limit_cases as lc
import vtrace_limit_cases as vl
import vtrace_model as vm
from steplog_model import bits
from test_vtrace_cpu import HIPCC, _compile, _harness

F32 = np.float32


# ---------------------------------------------------------------------------------------------- the scenarios
def test_the_names_the_existing_tests_use_are_unchanged():
    assert vm.NS == (5, 70) and vm.LS == (1, 5, 8, 9, 16, 17, 33, 130) and len(vm.PARAMS) == 4
    assert vm.PARAMS[3] == (0.99, 0.5, (2.0, 0.5, 1.0))


def test_launch_geometry_reaches_every_edge():
    """N: below, at and above one block of 64 and several blocks; L: every remainder class of a short set at depth 8 and 16 next to
    the full ones; the many-block case has one lane in its last block; the limit is the header's."""
    assert vl.LIMIT_NS == (1, 63, 64, 65, 257) and vl.LIMIT_LS == (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48)
    for depth in (8, 16):
        assert {L % depth for L in vl.LIMIT_LS} >= {0, 1, depth - 1} and min(vl.LIMIT_LS) < depth < max(vl.LIMIT_LS) // 2
    N, Ls = vl.MANY_BLOCKS
    assert (N + 63) // 64 == 65 and N % 64 == 1 and Ls == (9, 17)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "agx_vtrace.h")).read()
    assert f"#define AGX_VTRACE_LIMIT {vl.LIMIT_L}" in " ".join(header.split())
    n, L, _ = vl.LIMIT_CASE
    assert L == vl.LIMIT_L and (L - 1) * n + n - 1 == 266_239 and L // 8 == 512
    for N in vl.LIMIT_NS + (vl.MANY_BLOCKS[0],):          # the last lane of the last block folds every slot
        for L in (1, 9, 48):
            length = vl.case(N, L, vl.limit_seed(N, L))[0]
            assert N <= 6 or length[-1] == L


def test_limit_cases_hold_the_wild_lengths_and_unused_nan():
    for N, L in ((65, 33), (257, 48), (4097, 17), vl.LIMIT_CASE[:2]):
        length, reward, ends, value, boot, rho, live = vl.case(N, L, vl.LIMIT_CASE[2] if L == vl.LIMIT_L else vl.limit_seed(N, L))
        assert length[:5].tolist() == [-3, L + 7, 0, L, 1]
        assert np.isnan(reward[~live]).all() and np.isnan(value[~live]).all() and np.isnan(rho[~live]).all() and np.isnan(boot[(ends & vm.BOOT) == 0]).all()
        assert np.isfinite(reward[live]).all() and np.isfinite(value[live]).all() and np.isfinite(rho[live]).all()
        assert (~live).sum() > 0.2 * L * N and live.sum() > 0.2 * L * N
        assert set(np.unique(ends)) == {0, 1, 8, 10, 12}


def test_special_case_inputs():
    """len holds -3, L + 7, 0, L and 1; rho's live slots hold each of SPECIAL_RHO - -0.0, subnormal, 3.4e38, +inf, NaN - next to
    ordinary ratios; reward, value and boot hold each of limit_cases.SPECIAL at live slots; what must not be read is NaN."""
    N, L = vl.SPECIAL_NL
    length, reward, ends, value, boot, rho, live = vl.case(N, L, vl.SPECIAL_SEED, True)
    assert length[:5].tolist() == [-3, L + 7, 0, L, 1]
    assert np.isnan(rho[~live]).all() and np.isnan(reward[~live]).all() and np.isnan(value[~live]).all() and np.isnan(boot[(ends & vm.BOOT) == 0]).all()
    w = rho[live]
    special = np.isin(bits(w), bits(vl.SPECIAL_RHO[:-1])) | np.isnan(w)
    assert 0.2 < special.mean() < 0.4
    for x in vl.SPECIAL_RHO[:-1]:
        assert (bits(w) == bits(x)).sum() >= 10, float(x)
    assert np.isnan(w).sum() >= 10 and ((w > 0) & (w < 4) & ~special).sum() > 500
    for name, x in (("reward", reward[live]), ("value", value[live]), ("boot", boot[live & ((ends & vm.BOOT) != 0)])):
        for s in lc.SPECIAL[:-1]:
            assert (bits(x) == bits(s)).any(), (name, float(s))
        assert np.isnan(x).any(), name


@pytest.mark.parametrize("params", vl.SPECIAL_PARAMS, ids=[f"set{i}" for i in range(len(vl.SPECIAL_PARAMS))])
def test_special_case_outputs_hold_every_kind(params):
    """For each special parameter set, with and without a boot buffer, each of vs and pg_adv holds at least one NaN, one
    infinity, one subnormal and one -0.0 - the reference alone shows that every kind is present - and every slot that is not live is
    +0.0 as bits, whatever was folded through it."""
    N, L = vl.SPECIAL_NL
    live = vl.case(N, L, vl.SPECIAL_SEED, True)[6]
    for boot in (True, False):
        vs, pg, _ = vl.model(N, L, vl.SPECIAL_SEED, *params, boot, True)
        for name, x in (("vs", vs), ("pg_adv", pg)):
            seen = vl.kinds(x)
            print(f"{params}, boot buffer {boot}, {name}: {seen}")
            assert all(v >= 1 for v in seen.values()), (name, boot, seen)
            assert not bits(x)[~live].any(), (name, boot)


def test_the_levels_of_the_special_sets():
    """No clipping at all under a gamma whose powers go subnormal; every level 1, undiscounted; ordinary levels; a level above every
    finite ratio next to a subnormal and a tiny one."""
    assert vl.SPECIAL_PARAMS[0] == (2.0 ** -3, 1.0, (np.inf,) * 3) and vl.SPECIAL_PARAMS[1] == (1.0, 1.0, (1.0, 1.0, 1.0))
    assert vl.SPECIAL_PARAMS[2] == (0.99, 0.95, (2.0, 0.5, 1.0))
    g, la, (rb, cb, pb) = vl.SPECIAL_PARAMS[3]
    assert (g, la) == (0.99, 1.0) and np.isfinite(F32(rb)) and F32(rb) > F32(3.39e38) and F32(cb) == F32(2.0 ** -149) and F32(pb) == F32(2.0 ** -126)


# ---------------------------------------------------------------------------------------------- the definition at the limit
@pytest.mark.parametrize("gamma, lam, bars", vm.PARAMS)
def test_model_against_the_definition_at_the_limit(gamma, lam, bars):
    """vtrace_model.definition - the explicit sum in float64 - against the float32 model at (N, L) = (65, 48), (257, 33) and
    (65, 4096), for every live slot, within vtrace_model.bounds (derived from the operation count, not measured).  No live slot has
    a non-zero term below 2^-100: the bounds do not model underflow, and nothing is left out.  More than 100,000 live slots, chains of
    10 slots and more.  The worst error / bound is printed."""
    worst, checked, longest = [0.0, 0.0, 0.0], 0, 0
    for N, L, seed in vl.DEFINITION_CASES:
        live = vl.case(N, L, seed)[6]
        vs, pg, A = vl.model(N, L, seed, gamma, lam, bars)
        d, bnd = vl.defined(N, L, seed, gamma, lam, bars)
        assert np.array_equal(d["live"], live) and not (d["smallest"][live] < lc.TINY).any(), (N, L)
        for at, (got, want, bound) in enumerate(zip((A, vs, pg), (d["A"], d["vs"], d["pg"]), bnd)):
            ok, ratio = vl.ratios(got, want, bound, live)
            assert ok, (N, L, at, ratio)
            worst[at] = max(worst[at], ratio)
        checked, longest = checked + int(live.sum()), max(longest, int(d["chain"][live].max()))
    print(f"gamma = {gamma}, lambda = {lam}, levels = {bars}: {checked} live slots, none left out, longest chain {longest}; worst error / "
          f"bound A {worst[0]:.3f}, vs {worst[1]:.3f}, pg_adv {worst[2]:.3f}")
    assert checked > 100_000 and longest >= 10 and max(worst) < 1


# ---------------------------------------------------------------------------------------------- the host side of the same fold
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


def _check_harness(binary, tmp_path):
    """vtrace_fold - the loop over the function the kernel folds every step with - on the special case under the four special
    parameter sets, with and without a boot buffer, and at L = 4096: bit-equal to the model, a NaN being any NaN."""
    N, L = vl.SPECIAL_NL
    runs = [(N, L, vl.SPECIAL_SEED, p, boot, True) for p in vl.SPECIAL_PARAMS for boot in (True, False)]
    runs += [(*vl.LIMIT_CASE, vm.PARAMS[3], True, False), (*vl.LIMIT_CASE, vm.PARAMS[1], False, False)]
    compared, seen = 0, dict(nan=0, inf=0, subnormal=0, negzero=0)
    for N, L, seed, (gamma, lam, bars), boot, special in runs:
        length, reward, ends, value, b, rho, live = vl.case(N, L, seed, special)
        vs, pg, _ = vl.model(N, L, seed, gamma, lam, bars, boot, special)
        gv, gp = _harness(binary, tmp_path, length, reward, ends if boot else vl.no_boot(ends), value, b if boot else None, rho, gamma, lam, bars)
        for got, want, name in ((gv, vs, "vs"), (gp, pg, "pg_adv")):
            assert vl.same_but_nan(got.view(F32), want), (name, N, L, gamma, lam, bars, boot)
            assert not got[~live].any(), name
            for k, v in vl.kinds(want).items():
                seen[k] += v
        compared += 2 * L * N
    print(f"{compared} vs / pg_adv elements compared; {seen}")
    assert all(v >= 8 for v in seen.values())


def test_host_side_of_the_fold_at_the_limits(harness, tmp_path):
    _check_harness(harness, tmp_path)


def test_host_side_of_the_fold_at_the_limits_under_sanitizers(harness_san, tmp_path):
    _check_harness(harness_san, tmp_path)
