"""The scenarios of the tests that hold the V-trace kernel (K13, include/agx_vtrace.h) at the limits its header states and on
special floats - tests/test_gpu_vtrace_limits.py - and what the CPU check (tests/test_vtrace_limits_cpu.py) shares with it: the
launch geometries, the special case and its parameter sets, the cases of the float64 check, and the references, each computed once
per process and handed out read-only.  The fold and the definition are tests/vtrace_model.py's, the value set and the GAE inputs
tests/limit_cases.py's.  Every seed is chosen on the models alone; the CPU test pins what each scenario is there for.  Pure
NumPy, no GPU."""
import functools

import numpy as np

import limit_cases as lc
import vtrace_model as vm
from limit_cases import F32

# ---------------------------------------------------------------------------------------------- launch geometry
LIMIT_NS = (1, 63, 64, 65, 257)       # one lane, a wave short of one, a full block, a block and one lane, four blocks and one lane
# the set edges at the built depth 8 and at the measured depth 16: a short first set, one set, a set and one slot, ...
LIMIT_LS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48)
MANY_BLOCKS = (4097, (9, 17))         # 65 blocks, one lane in the last
LIMIT_L = 4096                        # AGX_VTRACE_LIMIT: 512 register sets at depth 8, element numbers up to 266,239 at N = 65
LIMIT_CASE = (65, LIMIT_L, 11)        # (N, L, seed)
# (N, L, seed) of the float64 check: more than 100,000 live slots, chains of 10 slots and more
DEFINITION_CASES = ((65, 48, 3), (257, 33, 4), LIMIT_CASE)
GUARD = 4096                          # the sentinel elements in front of and behind every output on the device


def limit_seed(N, L):
    return 1000 * N + L


# ---------------------------------------------------------------------------------------------- special floats
SPECIAL_NL, SPECIAL_SEED = (65, 33), 3
# (gamma, lambda, (rho_bar, c_bar, pg_rho_bar)): no clipping under a gamma whose powers go subnormal; every level 1 undiscounted
# (two rewards of 3.4e38 overflow); ordinary levels; a huge level next to a subnormal and a tiny one
SPECIAL_PARAMS = ((2.0 ** -3, 1.0, (np.inf, np.inf, np.inf)), (1.0, 1.0, (1.0, 1.0, 1.0)), (0.99, 0.95, (2.0, 0.5, 1.0)),
                  (0.99, 1.0, (3.4e38, 2.0 ** -149, 2.0 ** -126)))
SPECIAL_RHO = np.array([0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 1.0, 4.0, 3.4e38, np.inf, np.nan], F32)
# rho's generator is seeded seed + SPECIAL_RHO_SEED.  A vs of -0.0 is rare - both products of A must be -0.0 (a ratio of -0.0 over
# a positive td and a positive carry, or an underflow) at a value of -0.0 - so the offset was chosen, on the model alone, as
# one at which every parameter set holds at least three of each kind in each output, with and without a boot buffer
SPECIAL_RHO_SEED = 5266


def special_case(N, L, seed):
    """limit_cases.gae_case(special = True) - reward, value and boot from special_values (+-0, +-2^-149, +-2^-126, +-3.4e38, +-inf,
    NaN and normals), boot NaN where BOOT is unset, reward and value NaN where the slot is not live - plus rho: uniform in [0, 4],
    about 30 % of the live slots from SPECIAL_RHO, NaN in every slot that is not live.
    -> (len, reward, ends, value, boot, rho, live)."""
    length, reward, ends, value, boot, live = lc.gae_case(N, L, seed, special=True)
    rng = np.random.default_rng(seed + SPECIAL_RHO_SEED)
    rho = rng.uniform(0.0, 4.0, (L, N)).astype(F32)
    pick = SPECIAL_RHO[rng.integers(0, len(SPECIAL_RHO), (L, N))]
    rho = np.where(rng.random((L, N)) < 0.3, pick, rho).astype(F32)
    rho[~live] = np.nan
    return length, reward, ends, value, boot, rho, live


def kinds(x):
    """How many NaN, infinite, subnormal and negative-zero elements a float32 array holds."""
    x = np.asarray(x, F32)
    return dict(nan=int(np.isnan(x).sum()), inf=int(np.isinf(x).sum()), subnormal=int(((x != 0) & (np.abs(x) < F32(2.0 ** -126))).sum()),
                negzero=int((x.view(np.int32) == np.int32(-2 ** 31)).sum()))


def same_but_nan(got, want):
    """float32 arrays: NaN exactly where `want` is NaN (any payload), bit-equal everywhere else."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


# ---------------------------------------------------------------------------------------------- references, computed once
def _frozen(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(N, L, seed, special=False):
    """vtrace_model.case, or special_case, once per process and read-only."""
    return _frozen((special_case if special else vm.case)(N, L, seed))


def no_boot(ends):
    """The ends bytes of a call without a boot buffer: the BOOT bit taken out."""
    return (ends & 7).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def model(N, L, seed, gamma, lam, bars, boot=True, special=False):
    """The float32 model's (vs, pg_adv, A) of case(N, L, seed, special) - boot = False: without a boot buffer, on no_boot(ends)."""
    length, reward, ends, value, b, rho, live = case(N, L, seed, special)
    return _frozen(vm.vtrace(length, reward, ends if boot else no_boot(ends), value, b if boot else None, rho, gamma, lam, bars, with_A=True))


def zero_value(live):
    """value = 0 on the live slots and NaN elsewhere: there vs = fadd(A, 0) is A itself."""
    return np.where(live, F32(0), F32(np.nan)).astype(F32)


@functools.lru_cache(maxsize=None)
def defined(N, L, seed, gamma, lam, bars, at_zero_value=False):
    """vtrace_model.definition of case(N, L, seed) in float64 with its bounds -> (d, (bA, bvs, bpg)); at_zero_value: of the same
    case with zero_value(live) as its value."""
    length, reward, ends, value, boot, rho, live = case(N, L, seed)
    d = vm.definition(length, reward, ends, zero_value(live) if at_zero_value else value, boot, rho, gamma, lam, bars)
    _frozen(list(d.values()))
    return d, _frozen(vm.bounds(d))


def ratios(got, want, bound, live):
    """(whether every live error is within its bound, the worst error / bound over the live slots whose bound is not 0)."""
    err, bnd = np.abs(np.asarray(got, np.float64) - want)[live], bound[live]
    nz = bnd > 0
    return bool((err <= bnd).all()), float((err[nz] / bnd[nz]).max()) if nz.any() else 0.0
