"""The definition tests/test_gpu_action_state.py holds the fovea state update to (no tests in here; tests/test_action_cases_cpu.py
checks this file on the CPU, so a table that drifts fails there and not silently on the device).

Every live fovea kernel opens with the same small computation - the sensory action becomes fov_loc (and fov_res for the flexible
kind).  :func:`next_state` says what that computation is, in Python ints and float64, written from oracle.oracle
(clip_to_valid_fov, clip_to_valid_sas, update_loc, FlexibleFovealOracle.step) and the normalisations include/agx.h documents:

* NaN goes to the LOWER bound of whichever clip it meets (the clip is fmin(fmax(x, lo), hi));
* a FOV_RES action is rint, then a clamp to [1, obs];
* a relative delta is added without any 32-bit limit;
* the state that is read is clamped first: res to [1, obs], then loc to [0, obs - res] (clamp on read, agx_set_fov_state);
* an action_type other than 0 / 1 acts as FOV_LOC;
* a masked-out env keeps its stored state as it is.

The value tables hold, per dtype, the values a kernel's arithmetic can get wrong; each is there to catch one named mistake
(WHY).  :func:`batch` lays a table out so that every value stands once in the row element and once in the column element, each
time next to an ordinary partner, and marks a few more envs as masked.  FORMS is the list of kernel forms the GPU module walks,
each reached by geometry alone from rows of tests/golden/geometry_cases.json."""
import collections
import json
import math
import os

import numpy as np

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_cases.json")))
HEADLINE = ((84, 84), (30, 30))          # agx_plan.h: headline_fixed, the compile-time k_fovea_fixed<GeomS>
REL_SAS = (-7.0, 9.0)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
DTYPES = ("f32", "f64", "i32", "i64")
NP_DTYPE = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "i64": np.int64}
FOV_LOC, FOV_RES = 0, 1


# ------------------------------------------------------------------------------------------------------- the definition
def _clip(x, lo, hi):
    """fmin(fmax(x, lo), hi) on a Python int or float: NaN goes to lo.  Ints stay ints (exact beyond 2^53)."""
    if isinstance(x, float) and x != x:
        return lo
    return min(max(x, lo), hi)


def _rint(x):
    """Round half to even; +-inf stays."""
    if isinstance(x, float):
        return x if math.isinf(x) else round(x)
    return x


def _clamp(x, lo, hi):
    return min(max(int(x), lo), hi)


def value_of(x, dtype):
    """The element as the kernel is given it: a Python float (f32 / f64 widen to double exactly) or a Python int."""
    return float(x) if dtype in ("f32", "f64") else int(x)


def next_state(kind, mode, sas, obs, fov, loc, res, action, dtype, type, masked):
    """(loc, res) after one call.  kind "fixed" | "peripheral" | "flexible"; mode "absolute" | "relative"; sas (lo, hi) of the
    relative delta; obs, fov (h, w); loc, res the STORED state (any int32; res ignored unless flexible); action None or a pair of
    elements of `dtype`; type the env's sensory_action_type (flexible; any int32); masked: the env is left out by the mask."""
    loc = (int(loc[0]), int(loc[1]))
    res = (int(res[0]), int(res[1])) if kind == "flexible" else None
    if masked:
        return loc, res
    rr = tuple(_clamp(res[i], 1, obs[i]) for i in (0, 1)) if kind == "flexible" else (int(fov[0]), int(fov[1]))
    lr = tuple(_clamp(loc[i], 0, obs[i] - rr[i]) for i in (0, 1))
    if action is None:
        return lr, (rr if kind == "flexible" else None)
    a = [value_of(action[i], dtype) for i in (0, 1)]
    if kind == "flexible" and type == FOV_RES:
        rn = tuple(int(_rint(_clip(a[i], 1, obs[i]))) for i in (0, 1))
        return tuple(min(lr[i], obs[i] - rn[i]) for i in (0, 1)), rn
    out = []
    for i in (0, 1):
        bound = obs[i] - rr[i]
        if mode == "absolute":
            out.append(int(_rint(_clip(a[i], 0, bound))))
        else:
            d = _rint(_clip(a[i], sas[0], sas[1]))
            out.append(int(_rint(_clip(lr[i] + d, 0, bound))))
    return tuple(out), (rr if kind == "flexible" else None)


# ------------------------------------------------------------------------------------------------------- the value tables
def _f32_bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def _f64_bits(u):
    return np.array([u], np.uint64).view(np.float64)[0]


# name -> the mistake the value catches
WHY = collections.OrderedDict([
    ("+0", "a sign test instead of a compare"), ("-0", "rint(-0) = -0 must store integer 0"),
    ("+denorm_min", "flush-to-zero or a subnormal widened wrongly"), ("-denorm_min", "the same, below zero"),
    ("+min_normal", "the smallest normal, next to the subnormal path"), ("-min_normal", "the same, below zero"),
    ("just_below_half", "0.49999997 + 0.5 rounds to 1 in f32: floor(x + 0.5) instead of rint"),
    ("0.5", "tie to even, down"), ("1.5", "tie to even, up"), ("2.5", "tie to even, down again: round-half-up gives 3"),
    ("bound-0.5", "a tie at the last cell: rint after the clip, not before"), ("bound", "the bound itself"),
    ("bound+0.5", "rint before the clip gives bound or bound + 1"), ("bound+0.50001", "the first value that rounds past the bound"),
    ("2^24+2", "an f32 integer beyond the mantissa of a half-precision or int24 detour"),
    ("+2^31", "(int) before the clip: out of int32 by one"), ("-2^31", "INT_MIN as a float"),
    ("+3.4e38", "the largest finite f32 range"), ("-3.4e38", "the same, below zero"),
    ("+inf", "inf through fmin / fmax and rint"), ("-inf", "the same, below zero"),
    ("+nan", "NaN goes to the lower bound"), ("-nan", "a sign-bit test on a NaN"), ("nan_payload", "a NaN that is not the canonical quiet one"),
    # f64 only
    ("+4.9e-324", "the f64 subnormal: zero once narrowed to f32"), ("-4.9e-324", "the same, below zero"),
    ("+1e300", "inf once narrowed to f32, UB once converted to int"), ("-1e300", "the same, below zero"),
    ("12.5+2^-40", "12.5 once narrowed to f32 (rounds to 12); in f64 it rounds to 13"),
    ("13.5-2^-40", "13.5 once narrowed to f32 (rounds to 14); in f64 it rounds to 13"),
    ("0.5+2^-40", "the same narrowing inside every geometry's range (the smallest bound is 1, a relative delta's 9): 0.5 in f32, rounds to 0"),
    ("1.5-2^-40", "1.5 in f32 (rounds to 2); in f64 it rounds to 1"),
    ("2^53+2", "an f64 integer beyond 2^53"), ("0.5-2^-54", "0.5 once 0.5 is added in f64: floor(x + 0.5) gives 1"),
    # integers
    ("INT_MIN", "negation or abs of INT_MIN"), ("-1", "the first value below the clip"), ("0", "the lower bound"), ("1", "an ordinary cell"),
    ("bound+1", "the first integer past the bound"), ("INT_MAX", "INT_MAX + loc wraps in 32 bits"),
    ("2^32", "an i64 read by its low dword alone is 0"), ("2^32+5", "an i64 read by its low dword alone is 5"),
    ("-2^32+3", "an i64 read by its low dword alone is 3"), ("2^53+1", "an i64 that no double holds"),
    ("INT64_MIN", "the most negative i64"), ("INT64_MAX", "the largest i64: rounds to 2^63 as a double"),
])


def table(dtype, bound):
    """[(name, value)] of `dtype` for a clip whose upper bound is `bound` (an int >= 0); values are NumPy scalars of the dtype."""
    b = int(bound)
    if dtype in ("f32", "f64"):
        f = NP_DTYPE[dtype]
        t = [("+0", f(0.0)), ("-0", f(-0.0)), ("+denorm_min", f(2.0 ** -149)), ("-denorm_min", f(-2.0 ** -149)),
             ("+min_normal", f(2.0 ** -126)), ("-min_normal", f(-2.0 ** -126)), ("just_below_half", f(np.float32(0.49999997))),
             ("0.5", f(0.5)), ("1.5", f(1.5)), ("2.5", f(2.5)),
             ("bound-0.5", f(b - 0.5)), ("bound", f(b)), ("bound+0.5", f(b + 0.5)), ("bound+0.50001", f(np.float32(b + 0.50001))),
             ("2^24+2", f(2.0 ** 24 + 2)), ("+2^31", f(2.0 ** 31)), ("-2^31", f(-2.0 ** 31)),
             ("+3.4e38", f(np.float32(3.4e38))), ("-3.4e38", f(np.float32(-3.4e38))), ("+inf", f(np.inf)), ("-inf", f(-np.inf))]
        if dtype == "f32":
            t += [("+nan", _f32_bits(0x7FC00000)), ("-nan", _f32_bits(0xFFC00000)), ("nan_payload", _f32_bits(0x7FA5A5A5))]
        else:
            t += [("+nan", _f64_bits(0x7FF8000000000000)), ("-nan", _f64_bits(0xFFF8000000000000)),
                  ("nan_payload", _f64_bits(0x7FF4A5A5A5A5A5A5)),
                  ("+4.9e-324", f(4.9e-324)), ("-4.9e-324", f(-4.9e-324)), ("+1e300", f(1e300)), ("-1e300", f(-1e300)),
                  ("12.5+2^-40", f(12.5 + 2.0 ** -40)), ("13.5-2^-40", f(13.5 - 2.0 ** -40)),
                  ("0.5+2^-40", f(0.5 + 2.0 ** -40)), ("1.5-2^-40", f(1.5 - 2.0 ** -40)),
                  ("2^53+2", f(2.0 ** 53 + 2)), ("0.5-2^-54", f(0.5 - 2.0 ** -54))]
        return t
    i = NP_DTYPE[dtype]
    t = [("INT_MIN", i(INT32_MIN)), ("-1", i(-1)), ("0", i(0)), ("1", i(1)), ("bound", i(b)), ("bound+1", i(b + 1)), ("INT_MAX", i(INT32_MAX))]
    if dtype == "i64":
        t += [("2^32", i(2 ** 32)), ("2^32+5", i(2 ** 32 + 5)), ("-2^32+3", i(-2 ** 32 + 3)), ("2^53+1", i(2 ** 53 + 1)),
              ("INT64_MIN", i(INT64_MIN)), ("INT64_MAX", i(INT64_MAX))]
    return t


ORDINARY = 1          # the partner element: in range at every geometry of FORMS (the smallest bound is 1), and a small delta
MASKED = 3            # envs the mask leaves out, appended behind the table's envs


def batch(dtype, bound_r, bound_c):
    """(actions [N, 2] of the dtype, mask u8 [N], names [N]): env 2 k holds value k of table(dtype, bound_r) in the ROW element, env
    2 k + 1 value k of table(dtype, bound_c) in the COLUMN element, the other element ORDINARY; then MASKED envs whose mask byte is 0
    and whose actions are the table's last values (which must leave no trace)."""
    tr, tc = table(dtype, bound_r), table(dtype, bound_c)
    L = len(tr)
    a = np.full((2 * L + MASKED, 2), ORDINARY, NP_DTYPE[dtype])
    names = []
    for k in range(L):
        a[2 * k, 0] = tr[k][1]
        a[2 * k + 1, 1] = tc[k][1]
        names += [tr[k][0] + "/row", tc[k][0] + "/col"]
    for m in range(MASKED):
        a[2 * L + m] = (tr[L - 1 - m][1], tc[L - 2 - m][1])
        names.append("masked:" + tr[L - 1 - m][0])
    mask = np.ones(2 * L + MASKED, np.uint8)
    mask[2 * L:] = 0
    return a, mask, names


_TYPES = ((0, 1, 1, 0, 2, 1, 1, -1), (1, 2, -1, 1, 1, 0, 0, 1))


def mixed_types(n, which):
    """sensory_action_type of the flexible kind's mixed calls: 0, 1, 2 and -1 over the envs.  which = 0, 1: the two patterns are
    complementary - an env that is FOV_RES in one is FOV_LOC-like (0, 2 or -1) in the other - so over the two calls every value
    of the table meets both branches in both elements."""
    return np.array([_TYPES[which][e % 8] for e in range(n)], np.int32)


# ------------------------------------------------------------------------------------------------------- the forms
Form = collections.namedtuple("Form", "name entry obs fov per aa fs key label")
MODES = {"fixed_resize": ("fixed", "resize"), "fixed_raw": ("fixed", "raw"), "fixed_mask": ("fixed", "mask"),
         "flex_resize": ("flexible", "resize"), "flex_raw": ("flexible", "raw"), "flex_mask": ("flexible", "mask"),
         "peripheral": ("peripheral", "resize")}


def _row(obs, fov, per, aa):
    for r in TABLE:
        if (tuple(r["obs"]), tuple(r["fov"]), tuple(r["per"]), r["aa"]) == (obs, fov, per, aa):
            return r
    raise KeyError((obs, fov, per, aa))


def _forms():
    """The smallest row of the table per kernel family, `fs` as the table gives it, in each output mode; then the packed forms,
    the one-call steps and the history's read-time action.  entry: the Python entry point the GPU module calls."""
    out = []

    def add(entry, obs, fov, per, aa, keys, headline=False):
        for key in keys:
            if headline:
                fs, label = 4, "fixed<GeomS>"
            else:
                r = _row(obs, fov, per, aa)
                fs, label = r["fs"], r["plan"][key]
            fam = label.split(" ", 1)[0]
            if entry in ("fovea_packed", "step_flexible_packed"):
                fam = label.rsplit("packed=", 1)[1]
            name = "{}-{}-o{}x{}_f{}x{}_aa{}-{}".format(entry, key, *obs, *fov, aa, fam.replace("<", "_").replace(">", ""))
            out.append(Form(name, entry, obs, fov, per, aa, fs, key, label))

    fixed = ("fixed_resize", "fixed_raw", "fixed_mask")
    flex = ("flex_resize", "flex_raw", "flex_mask")
    add("fovea", *HEADLINE, (40, 40), 1, fixed, headline=True)                       # compile-time fixed
    add("fovea", (10, 12), (3, 5), (4, 4), 1, fixed)                                  # run-time fixed<GeomR>
    add("fovea", (12, 12), (3, 5), (4, 4), 0, ("peripheral",))                        # per3
    add("fovea", (84, 84), (30, 30), (5, 5), 1, ("peripheral",))                      # peripheral2
    add("fovea", (8, 264), (4, 100), (4, 260), 0, ("peripheral",))                    # generic peripheral
    add("fovea", (12, 12), (3, 5), (4, 4), 0, flex)                                   # flex3, raw3, raw3 mask
    add("fovea", (8, 264), (4, 100), (4, 260), 0, flex)                               # flexible2
    add("fovea", (128, 128), (127, 127), (16, 16), 1, flex)                           # generic flexible
    add("fovea_packed", (12, 12), (3, 5), (4, 4), 0, ("flex_raw",))                   # scan + raw3 packed
    add("fovea_packed", (8, 264), (4, 100), (4, 260), 0, ("flex_raw",))               # scan + offsets + flexible2
    add("fovea_packed", (128, 128), (127, 127), (16, 16), 1, ("flex_raw",))           # scan + offsets + generic
    add("step_fixed", *HEADLINE, (40, 40), 1, ("fixed_resize",), headline=True)
    add("step_fixed", (12, 12), (3, 5), (4, 4), 0, ("fixed_raw",))
    add("step_flexible_packed", (84, 84), (1, 1), (1, 1), 0, ("flex_raw",))           # band12 ingest: the scan rides in the ingest launch
    add("step_flexible_packed", (12, 12), (3, 5), (4, 4), 0, ("flex_raw",))           # general ingest: three launches
    add("history_observe", *HEADLINE, (40, 40), 1, ("fixed_raw",), headline=True)
    add("history_observe", (12, 12), (3, 5), (4, 4), 0, ("fixed_resize",))
    return out


FORMS = _forms()


def family(kind, label):
    """The kernel family of a plan label of the table: the kernel's name, with the kind where one kernel serves two."""
    fam = label.split(" ", 1)[0]
    return fam + ":" + kind if fam == "generic" else fam


def table_families():
    """Every distinct kernel family tests/golden/geometry_cases.json names, the packed forms included."""
    out = set()
    for r in TABLE:
        for key, label in r["plan"].items():
            if label.startswith("refused"):
                continue
            out.add(family(MODES[key][0], label))
            if "packed=" in label:
                out.add("packed=" + label.rsplit("packed=", 1)[1])
    return out


def form_families():
    out = set()
    for f in FORMS:
        if f.label == "fixed<GeomS>":
            continue
        if f.entry in ("fovea_packed", "step_flexible_packed"):
            out.add("packed=" + f.label.rsplit("packed=", 1)[1])
        elif f.entry == "fovea":
            out.add(family(MODES[f.key][0], f.label))
    return out
