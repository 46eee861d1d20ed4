"""CPU: the colour (AGX_FRAME_RGB) constants of the C ABI and their binding twins, and the Python-side refusals that need no GPU."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defines():
    src = open(os.path.join(REPO, "include", "agx.h")).read()
    return {k: int(v, 0) for k, v in re.findall(r"^#define\s+AGX_([A-Z0-9_]+)\s+(-?(?:0x[0-9A-Fa-f]+|\d+))\b", src, flags=re.M)}


def test_colour_constants_and_binding_twins():
    from active_gym import _native as nat
    d = _defines()
    assert d["FRAME_RGB"] == 0x100 and nat.FRAME_RGB == 0x100
    assert d["GRAY_NONE"] == 2 and nat.GRAY_NONE == 2
    # the flag shares out_mode with the mode and the element type bits without overlapping them
    assert nat.FRAME_RGB & (nat.OBS_TYPE_MASK | nat.OUT_RAW | nat.OUT_RESIZE | nat.OUT_MASK) == 0
    assert nat.GRAY_NONE not in (nat.GRAY_CV15, nat.GRAY_CV14)
    # additive only: no entry point, no config field, same ABI version
    assert d["ABI_VERSION"] == 2 and nat.ABI_VERSION == 2


def test_pipeline_rejects_bad_channel_count():
    import pytest
    from active_gym import ObsPipeline
    with pytest.raises(ValueError):
        ObsPipeline(num_envs=1, kind="base", channels=2)


# ---------------------------------------------------------------------------------------------------------- colour goldens
import glob

import numpy as np
import pytest

GOLD = os.path.join(REPO, "tests", "golden")
RGB_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "colour_dmc_*.npz")))


def test_colour_goldens_exist_and_load_without_pickle():
    assert len(RGB_GOLDENS) >= 13
    for p in RGB_GOLDENS:
        g = np.load(p, allow_pickle=False)
        for k in g.files:
            assert g[k].dtype != object, (p, k)
        assert os.path.getsize(p) < 1 << 20


def golden_outputs(g):
    """the reference's observations of a colour golden as float64 [K, fs, 3, ...]"""
    if "out_u8" in g.files:
        return (g["out_u8"].astype(np.float32) / np.float32(255)).astype(np.float64)
    return g["out"].astype(np.float64)


@pytest.mark.parametrize("path", RGB_GOLDENS, ids=lambda p: os.path.basename(p)[11:-4])
def test_colour_golden_channels_equal_the_oracle_on_that_channel(path):
    """Each channel of the reference's colour run equals oracle/'s gray restatement of fov_env.py applied to that channel."""
    from oracle import oracle as O
    g = np.load(path, allow_pickle=False)
    kind = str(g["kind"])
    states = (g["states_u8"].astype(np.float32) / np.float32(255)).astype(np.float64)
    out = golden_outputs(g)
    obs, fov = tuple(int(v) for v in g["obs_size"]), tuple(int(v) for v in g["fov_size"])
    assert out.shape[:3] == (len(states), int(g["frame_stack"]), 3)
    tol = 0.0 if bool(g["exact"]) else 1e-5          # resampled: the reference resizes float32 states in float32
    for c in range(3):
        common = dict(obs_size=obs, fov_size=fov, fov_init_loc=tuple(g["fov_init_loc"]), sensory_action_mode=str(g["mode"]),
                      sensory_action_space=tuple(g["sensory_action_space"]), antialias=bool(g["antialias"]))
        if kind == "fixed":
            orc = O.FixedFovealOracle(resize_to_full=bool(g["resize_to_full"]), mask_out=bool(g["mask_out"]), **common)
        elif kind == "flexible":
            orc = O.FlexibleFovealOracle(resize_to_full=bool(g["resize_to_full"]), mask_out=bool(g["mask_out"]), **common)
        elif kind == "peripheral":
            orc = O.PeripheralOracle(peripheral_res=tuple(int(v) for v in g["peripheral_res"]), **common)
        t = 0
        for k in range(len(states)):
            s = states[k][:, c]
            if kind == "base":
                want = s
            elif bool(g["is_reset"][k]):
                want = orc.reset(s)
            else:
                a = g["sens"][t]
                want = orc.step(s, a, int(g["sens_type"][t])) if kind == "flexible" else orc.step(s, a)
            if not bool(g["is_reset"][k]):
                t += 1
            got = out[k][:, c]
            assert got.shape == np.shape(want), (k, c)
            assert np.max(np.abs(got - want), initial=0.0) <= tol, (k, c)
            if kind != "base":
                assert np.array_equal(np.asarray(orc.fov_loc, dtype=np.int64), g["fov_loc"][k]), (k, c)
    assert t == len(g["sens"])
