#!/usr/bin/env python3
"""Generate the colour DMC goldens (tests/golden/colour_dmc_*.npz) by EXECUTING the reference's own ``active_gym/dmc_env.py`` and
``active_gym/fov_env.py`` (read from the reference checkout, never copied) over ``tests/fake_dmc.ScriptedDMC``, with the
stand-ins of make_golden.py (imported, not edited).

The reference cannot run ``grey=False`` as written: ``_get_obs`` returns the ``(H, W, 3)`` render / 255 and
``_reset_buffer`` pushes ``(H, W)`` zeros, so the first ``np.stack`` raises.  ``_ColourDMCEnv`` below overrides exactly those two
methods to what the reference's declared ``(frame_stack, 3, H, W)`` observation space says: ``_get_obs`` transposes the render to
CHW, ``_reset_buffer`` pushes ``(3, H, W)`` zeros.  Everything else - action conversion, action repeat, the stack, RecordWrapper,
and the fovea wrappers' crop / paste / Resize on ``[..., H, W]`` - is the reference's code as it stands.  The Resize stand-in here
flattens all leading axes into the batch (torchvision's tensor ``resize`` accepts ``[..., H, W]``; make_golden.py's form is 3-D
only).

Only data is written (inputs, actions and the reference's outputs); run from the repo root:
    python tests/golden/make_golden_dmc_rgb.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))


def _load_make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


MG = _load_make_golden()


class _FlatResize(torch.nn.Module):
    """torchvision.transforms.Resize(size) on a tensor [..., H, W]: every leading axis goes into the batch, each plane is
    interpolated on its own (bilinear, align_corners=False, antialias per MG._STATE), same-size input returned as is."""

    def __init__(self, size):
        super().__init__()
        self.size = tuple(int(s) for s in size)

    def forward(self, img):
        if tuple(img.shape[-2:]) == self.size:
            return img
        lead = tuple(img.shape[:-2])
        x = img.reshape((-1, 1) + tuple(img.shape[-2:]))
        out = torch.nn.functional.interpolate(x, size=self.size, mode="bilinear", align_corners=False,
                                              antialias=MG._STATE["antialias"])
        return out.reshape(lead + self.size)


def _reference():
    if not os.path.isdir(MG.REF):
        raise SystemExit(f"reference checkout not found at {MG.REF}; goldens are generated in the build container only")
    MG._install_standins()
    sys.modules["torchvision.transforms"].Resize = _FlatResize      # before fov_env.py binds the name
    fov_env, _, dmc_env = MG._load_reference()

    class _ColourDMCEnv(dmc_env.DMCEnv):
        """The reference's DMCEnv with its two grey=False lines made to match its declared (fs, 3, H, W) space."""

        def _get_obs(self, time_step):
            return super()._get_obs(time_step).transpose(2, 0, 1)         # (H, W, 3) -> (3, H, W)

        def _reset_buffer(self):
            for _ in range(self.frame_stack):
                self.state_buffer.append(np.zeros((3,) + tuple(self.obs_size)))

    return fov_env, dmc_env, _ColourDMCEnv


GEOM = dict(obs=(20, 24), fov=(6, 8), per=(7, 9))


def _case(fov_env, dmc_env, Colour, name, kind, seed, mode="absolute", resize_to_full=False, mask_out=False, antialias=True,
          fs=3, ar=2, steps=12, episode_len=9):
    import fake_dmc
    obs, fov = GEOM["obs"], GEOM["fov"]
    MG._STATE["next_dmc"] = lambda kw: fake_dmc.ScriptedDMC(seed, episode_len=episode_len)
    MG._STATE["antialias"] = antialias
    kw = dict(frame_stack=fs, action_repeat=ar, grey=False, record=True, fov_size=fov, fov_init_loc=(1.4, 2.5),
              sensory_action_mode=mode, sensory_action_space=(-3.0, 4.0), resize_to_full=resize_to_full, mask_out=mask_out,
              peripheral_res=GEOM["per"])
    args = dmc_env.DMCEnvArgs(domain_name="scripted", task_name="t", seed=seed, obs_size=tuple(obs), **kw)
    core = Colour(args)
    assert core.observation_space.shape == (fs, 3) + tuple(obs)
    rec_env = fov_env.RecordWrapper(core, args)                          # DMCBaseEnv (dmc_env.py:255-258)
    env = {"base": lambda: rec_env, "fixed": lambda: fov_env.FixedFovealEnv(rec_env, args),
           "flexible": lambda: fov_env.FlexibleFovealEnv(rec_env, args),
           "peripheral": lambda: fov_env.FixedFovealPeripheralEnv(rec_env, args)}[kind]()
    rng = np.random.default_rng(seed + 1)
    motor = rng.uniform(-1, 1, size=(steps, 2)).astype(np.float32)
    sens = np.zeros((steps, 2))
    stype = np.zeros(steps, np.int64)
    hi = np.array(obs) - np.array(fov)
    for t in range(steps):
        if kind == "flexible" and rng.random() < 0.5:
            stype[t] = 1
            sens[t] = (rng.integers(2, obs[0] + 1), rng.integers(2, obs[1] + 1))
            if t == 1:
                sens[t] = (fov[0] + 5, max(2, fov[1] - 3))                # rows > fov rows: the squeeze path
        elif mode == "absolute":
            sens[t] = rng.uniform(-3.0, max(hi) + 3.0, size=2)
        else:
            sens[t] = rng.uniform(-5.0, 6.0, size=2)
    states, outs, locs, ress, dones, is_reset = [], [], [], [], [], []

    def push(o, info, d, rs):
        states.append(np.stack(core.state_buffer).astype(np.float64))
        outs.append(np.asarray(o, dtype=np.float64))
        locs.append(np.asarray(info.get("fov_loc", np.zeros(2)), dtype=np.int64))
        ress.append(np.asarray(info.get("fov_res", fov), dtype=np.int64))
        dones.append(bool(d))
        is_reset.append(rs)

    o, info = env.reset()
    push(o, info, False, True)
    for t in range(steps):
        if kind == "base":
            act = motor[t]
        else:
            # FOV_RES: integer resolutions, as the reference needs them (it slices with fov_res unconverted, fov_env.py:284)
            act = {"motor_action": motor[t], "sensory_action": sens[t].astype(np.int64) if stype[t] else sens[t]}
            if kind == "flexible":
                act["sensory_action_type"] = np.array((int(stype[t]),))
        o, r, d, tr, info = env.step(act)
        push(o, info, d, False)
        if d:
            o, info = env.reset()
            push(o, info, False, True)
    assert any(dones), "the script must cross an episode end"
    states = np.stack(states)
    u8 = np.rint(states * 255.0).astype(np.uint8)
    assert np.array_equal((u8.astype(np.float32) / np.float32(255.0)).astype(np.float64), states)
    rs = np.stack([np.asarray(s, dtype=np.float64) for s in rec_env.record_buffer["state"]])
    rs_u8 = np.rint(rs * 255.0).astype(np.uint8)
    assert np.array_equal((rs_u8.astype(np.float32) / np.float32(255.0)).astype(np.float64), rs)
    out = np.stack(outs)
    exact = kind == "base" or (kind == "fixed" and (mask_out or not resize_to_full))   # crops / pastes of u8 / 255 values
    rec = dict(kind=kind, mode=mode, resize_to_full=resize_to_full, mask_out=mask_out, antialias=antialias, seed=seed,
               obs_size=np.array(obs), fov_size=np.array(fov), peripheral_res=np.array(GEOM["per"]), fov_init_loc=np.array((1.4, 2.5)),
               sensory_action_space=np.array((-3.0, 4.0)), frame_stack=fs, action_repeat=ar, episode_len=episode_len,
               motor=motor, sens=sens, sens_type=stype, dones=np.array(dones), is_reset=np.array(is_reset),
               states_u8=u8, fov_loc=np.stack(locs), fov_res=np.stack(ress), record_states_u8=rs_u8, exact=exact,
               obs_space_shape=np.array(env.observation_space.shape))
    if exact:
        ou8 = np.rint(out * 255.0).astype(np.uint8)
        assert np.array_equal((ou8.astype(np.float32) / np.float32(255.0)).astype(np.float64), out)
        rec["out_u8"] = ou8
    else:
        rec["out"] = out.astype(np.float32)
    path = os.path.join(HERE, f"colour_dmc_{name}.npz")
    np.savez_compressed(path, **rec)
    return path


def main():
    fov_env, dmc_env, Colour = _reference()
    c = lambda *a, **k: _case(fov_env, dmc_env, Colour, *a, **k)      # noqa: E731
    paths = [c("base", "base", 31),
             c("fixed_raw_abs", "fixed", 32),
             c("fixed_mask_abs", "fixed", 33, mask_out=True),
             c("fixed_resize_abs", "fixed", 34, resize_to_full=True),
             c("fixed_raw_rel", "fixed", 35, mode="relative"),
             c("fixed_mask_rel", "fixed", 36, mode="relative", mask_out=True),
             c("fixed_resize_rel", "fixed", 37, mode="relative", resize_to_full=True)]
    for aa in (False, True):
        paths += [c(f"flex_mask_aa{int(aa)}", "flexible", 40 + aa, mask_out=True, antialias=aa),
                  c(f"flex_resize_aa{int(aa)}", "flexible", 42 + aa, resize_to_full=True, antialias=aa),
                  c(f"per_aa{int(aa)}", "peripheral", 44 + aa, antialias=aa)]
    total = 0
    for p in paths:
        sz = os.path.getsize(p)
        total += sz
        print(f"{os.path.relpath(p, REPO):50s} {sz / 1024:8.1f} KiB")
    print(f"total {total / 1e6:.2f} MB in {len(paths)} files")


if __name__ == "__main__":
    main()
