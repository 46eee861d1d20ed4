"""The ``infos`` dictionaries of the vector envs (SyncVectorEnv conventions, gymnasium<1.0): pure functions of arrays and
tensors, shared by reset(), reset_envs() and both step loops of :class:`~active_gym.vector.AtariVecEnv`."""
from __future__ import annotations

import numpy as np
import torch


def with_masks(info, n):
    """Every key with its ``_key`` mask (all True: every env reports every key)."""
    out = {}
    for k, v in info.items():
        out[k] = v
        out["_" + k] = np.ones(n, bool)
    return out


def fov_entries(loc, res, numpy_out: bool, h_loc=None, h_res=None):
    """The ``fov_loc`` / ``fov_res`` entries from the i32 [*, 2] device tensors (None: no such key); host rows a chunked step
    already brought home (``h_loc`` / ``h_res``) take their place.  Host outputs: NumPy int64 like the reference's
    info["fov_loc"].  Device outputs (args.device set): int64 DEVICE tensors - no device-to-host copy, hence no synchronisation
    inside step(): the next step's emulation then overlaps this step's last H2D chunk and kernels."""
    out = {}
    for key, dev, host in (("fov_loc", loc, h_loc), ("fov_res", res, h_res)):
        v = dev if host is None else host
        if v is not None:
            if numpy_out and isinstance(v, torch.Tensor):
                v = v.cpu().numpy()
            out[key] = v.astype(np.int64) if numpy_out else v.to(torch.int64)
    return out


def terminal_rows(n, idx, obs_rows, info, gathered, hist_index=None):
    """``final_observation`` / ``final_info``: object arrays [n], filled for the envs in ``idx``.  ``obs_rows[j]`` is the
    terminal observation of env ``idx[j]``; its final_info copies row ``idx[j]`` of every per-env array in ``info``, takes
    row ``j`` of the entries in ``gathered`` (rows already gathered for ``idx``, handed out as views), and - where given -
    ``hist_index[idx[j]]`` as its ``history_index``."""
    final_obs = np.empty(n, dtype=object)
    final_info = np.empty(n, dtype=object)
    for j, i in enumerate(idx):
        final_obs[i] = obs_rows[j]
        fi = {key: (gathered[key][j] if key in gathered else (val[i].copy() if isinstance(val[i], np.ndarray) else val[i]))
              for key, val in info.items()}
        fi.update((key, val[j]) for key, val in gathered.items() if key not in info)
        if hist_index is not None:
            fi["history_index"] = hist_index[i]
        final_info[i] = fi
    return final_obs, final_info


def attach_final(infos, done, final_obs, final_info):
    """The four ``final_*`` keys of a step in which envs were reset."""
    infos["final_observation"] = final_obs
    infos["_final_observation"] = done.copy()
    infos["final_info"] = final_info
    infos["_final_info"] = done.copy()
    return infos
