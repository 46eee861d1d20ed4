"""CPU: the observation element type (AGX_OBS_* bits of agx_config.out_mode, obs_dtype in Python) - validation in agx_create,
the binding's constants and the Python errors that are raised before any GPU work."""
import ctypes

import numpy as np
import pytest
import torch

from active_gym import _native as nat
from active_gym.atari_env import AtariEnvArgs
from active_gym.dmc_env import DMCEnvArgs


def _cfg(kind=nat.KIND_FIXED, out_mode=nat.OUT_RESIZE):
    cfg = nat.AgxConfig()
    cfg.struct_size = ctypes.sizeof(nat.AgxConfig)
    cfg.num_envs = 2
    cfg.kind = kind
    cfg.raw_h, cfg.raw_w = nat.RAW_H, nat.RAW_W
    cfg.obs_h = cfg.obs_w = 84
    cfg.frame_stack = 4
    cfg.fov_h = cfg.fov_w = 30
    cfg.per_h = cfg.per_w = 20
    cfg.out_mode = out_mode
    cfg.action_mode = nat.MODE_ABSOLUTE
    cfg.antialias = 1
    return cfg


def _create(cfg):
    lib = nat.lib()
    ctx = ctypes.c_void_p()
    rc = lib.agx_create(ctypes.byref(cfg), ctypes.byref(ctx))
    if rc == nat.OK:                      # a machine with a GPU: the config was valid
        lib.agx_destroy(ctx)
    return rc, nat.last_error(None)


def test_constants():
    assert (nat.OBS_F32, nat.OBS_BF16, nat.OBS_F16, nat.OBS_TYPE_MASK) == (0x00, 0x10, 0x20, 0x30)
    assert nat.OBS_TYPE_MASK & (nat.OUT_RAW | nat.OUT_RESIZE | nat.OUT_MASK) == 0


@pytest.mark.parametrize("kind", [nat.KIND_FIXED, nat.KIND_FLEXIBLE, nat.KIND_PERIPHERAL])
@pytest.mark.parametrize("mode", [nat.OUT_RAW, nat.OUT_RESIZE, nat.OUT_MASK])
@pytest.mark.parametrize("bits", [nat.OBS_F32, nat.OBS_BF16, nat.OBS_F16])
def test_valid_combinations_pass_validation(kind, mode, bits):
    # without a GPU the first failure is the device query (E_HIP), i.e. every config check before it passed
    rc, msg = _create(_cfg(kind, mode | bits))
    assert rc in (nat.OK, nat.E_HIP), (rc, msg)


@pytest.mark.parametrize("bits", [nat.OBS_F32, nat.OBS_BF16, nat.OBS_F16])
def test_base_kind_reads_only_the_type_bits(bits):
    for low in (0, 1, 2, 7):            # the low bits are ignored for AGX_KIND_BASE, as before
        rc, msg = _create(_cfg(nat.KIND_BASE, low | bits))
        assert rc in (nat.OK, nat.E_HIP), (low, bits, rc, msg)


@pytest.mark.parametrize("kind", [nat.KIND_FIXED, nat.KIND_FLEXIBLE, nat.KIND_PERIPHERAL])
@pytest.mark.parametrize("out_mode", [0x30, 0x31, 0x40, 0x41, 0x80 | nat.OBS_BF16, 5 | nat.OBS_BF16, 5])
def test_bad_out_mode_bits_are_rejected(kind, out_mode):
    rc, msg = _create(_cfg(kind, out_mode))
    assert rc == nat.E_INVALID, (hex(out_mode), rc, msg)
    assert "out_mode" in msg


def test_base_kind_rejects_both_type_bits():
    rc, msg = _create(_cfg(nat.KIND_BASE, nat.OBS_TYPE_MASK))
    assert rc == nat.E_INVALID and "out_mode" in msg


def test_resolve_obs_dtype():
    from active_gym.pipeline import obs_dtype_bits, resolve_obs_dtype
    assert resolve_obs_dtype("float32") is torch.float32
    assert resolve_obs_dtype(torch.bfloat16) is torch.bfloat16
    assert resolve_obs_dtype("float16") is torch.float16
    assert obs_dtype_bits("bfloat16") == nat.OBS_BF16 and obs_dtype_bits(torch.float16) == nat.OBS_F16
    assert obs_dtype_bits(torch.float32) == nat.OBS_F32
    for bad in ("float64", "bf16", torch.float64, torch.int8, np.float16, None):
        with pytest.raises(ValueError, match="obs_dtype"):
            resolve_obs_dtype(bad)


def test_pipeline_rejects_unknown_obs_dtype_first():
    from active_gym import ObsPipeline
    with pytest.raises(ValueError, match="obs_dtype"):
        ObsPipeline(num_envs=1, kind="base", obs_dtype="float64")


def _atari_args(**kw):
    base = dict(fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute", resize_to_full=True,
                frame_source="synthetic")
    base.update(kw)
    return AtariEnvArgs(game="breakout", seed=0, obs_size=(84, 84), **base)


def test_args_default_to_float32():
    assert AtariEnvArgs(game="breakout", seed=0, obs_size=(84, 84)).obs_dtype == "float32"
    assert DMCEnvArgs("cartpole", "swingup", 0, (84, 84)).obs_dtype == "float32"


@pytest.mark.parametrize("kw, what", [
    (dict(obs_dtype="float64"), "obs_dtype"),
    (dict(obs_dtype=torch.int32), "obs_dtype"),
    (dict(obs_dtype="bfloat16"), "NumPy"),                                           # host outputs (device=None)
    (dict(obs_dtype=torch.bfloat16), "NumPy"),
    (dict(obs_dtype="float16", ragged_obs="packed"), "packed"),
    (dict(obs_dtype="bfloat16", device="cuda", ragged_obs="packed"), "packed"),
    (dict(obs_dtype="float16", record=True), "record"),
    (dict(obs_dtype="bfloat16", device="cuda", record=True), "record"),
])
@pytest.mark.parametrize("kind", ["base", "fixed", "flexible"])
def test_env_errors_before_the_pipeline(kw, what, kind):
    from active_gym.vector import AtariVecEnv
    with pytest.raises(ValueError, match=what):
        AtariVecEnv(_atari_args(**kw), 2, kind=kind)


def test_dmc_env_errors_before_the_pipeline():
    from active_gym.dmc_env import DMCVecEnv
    with pytest.raises(ValueError, match="NumPy"):
        DMCVecEnv(DMCEnvArgs("cartpole", "swingup", 0, (84, 84), obs_dtype="bfloat16"), 2, kind="base")
    with pytest.raises(ValueError, match="record"):
        DMCVecEnv(DMCEnvArgs("cartpole", "swingup", 0, (84, 84), obs_dtype="float16", record=True), 2, kind="base")


def test_observation_space_dtypes():
    from active_gym.spaces import Box
    from active_gym.vector import obs_space_dtype
    assert obs_space_dtype(torch.float32) is np.float32
    assert obs_space_dtype(torch.float16) is np.float16
    assert obs_space_dtype(torch.bfloat16) is np.float32            # no NumPy bfloat16: the Box stays float32
    assert Box(low=-1., high=1., shape=(4, 84, 84), dtype=obs_space_dtype(torch.float16)).dtype == np.float16
