"""CPU: the functions that build the vector envs' infos (active_gym/infos.py) on NumPy inputs - what reset(), reset_envs()
and both step loops of AtariVecEnv share: key masks, fov entries, terminal rows, final keys."""
import numpy as np
import pytest
import torch

from active_gym.infos import attach_final, fov_entries, terminal_rows, with_masks

N, DONE = 4, [1, 3]


def _info():
    return {"ep_len": np.array([5, 6, 7, 8], np.int64),                                  # 1-D
            "fov_loc": np.arange(8, dtype=np.int64).reshape(N, 2),                       # 2-D
            "discount": np.array([None, 0.0, 1.0, 0.5], dtype=object)}                   # object dtype (DMC)


def test_terminal_rows_exist_exactly_for_the_done_envs_and_are_copies():
    info = _info()
    obs_rows = [np.full((2, 3), 10.0), np.full((2, 3), 30.0)]                            # row j belongs to env DONE[j]
    final_obs, final_info = terminal_rows(N, DONE, obs_rows, info, {})
    assert final_obs.dtype == object and final_info.dtype == object and final_obs.shape == final_info.shape == (N,)
    for i in range(N):
        assert (final_info[i] is not None) == (i in DONE) and (final_obs[i] is not None) == (i in DONE)
    assert final_obs[1] is obs_rows[0] and final_obs[3] is obs_rows[1]
    for i in DONE:
        fi = final_info[i]
        assert list(fi) == ["ep_len", "fov_loc", "discount"] and "history_index" not in fi
        assert fi["ep_len"] == 5 + i and fi["fov_loc"].tolist() == [2 * i, 2 * i + 1]
    assert final_info[1]["discount"] == 0.0 and final_info[3]["discount"] == 0.5
    # copies: the env zeroes the counters of the reset envs and overwrites the fov rows right after
    info["ep_len"][:] = 0
    info["fov_loc"][:] = -1
    info["discount"][:] = None
    assert final_info[1]["ep_len"] == 6 and final_info[3]["ep_len"] == 8
    assert final_info[3]["fov_loc"].tolist() == [6, 7] and final_info[1]["discount"] == 0.0


def test_gathered_rows_are_taken_by_position_not_by_env_index():
    info = _info()
    gathered = {"fov_loc": np.array([[100, 101], [300, 301]]),                          # replaces the per-env entry, in place
                "fov_res": np.array([[11, 12], [31, 32]])}                               # a key the per-env info does not have
    _, final_info = terminal_rows(N, DONE, [0.0, 1.0], info, gathered)
    assert list(final_info[1]) == ["ep_len", "fov_loc", "discount", "fov_res"]
    assert final_info[1]["fov_loc"].tolist() == [100, 101] and final_info[3]["fov_loc"].tolist() == [300, 301]
    assert final_info[1]["fov_res"].tolist() == [11, 12] and final_info[3]["fov_res"].tolist() == [31, 32]
    assert final_info[0] is None and final_info[2] is None


def test_terminal_history_index_is_the_one_passed_in():
    hist = np.array([40, 41, 42, 43], np.int64)
    _, final_info = terminal_rows(N, DONE, [0.0, 1.0], {"ep_len": np.arange(N)}, {}, hist)
    assert final_info[1]["history_index"] == 41 and final_info[3]["history_index"] == 43
    # ... also where the per-env info carries one of its own (the native loop's: the reset observation's index)
    _, final_info = terminal_rows(N, DONE, [0.0, 1.0], {"history_index": hist + 1}, {}, hist)
    assert final_info[1]["history_index"] == 41 and final_info[3]["history_index"] == 43


def test_final_keys_carry_their_own_copies_of_done():
    done = np.array([False, True, False, True])
    fo, fi = terminal_rows(N, DONE, [0.0, 1.0], _info(), {})
    infos = attach_final(with_masks(_info(), N), done, fo, fi)
    assert infos["final_observation"] is fo and infos["final_info"] is fi
    for key in ("_final_observation", "_final_info"):
        assert np.array_equal(infos[key], done) and infos[key] is not done
    assert infos["_final_observation"] is not infos["_final_info"]
    done[:] = False
    assert infos["_final_info"].tolist() == [False, True, False, True]
    for key in _info():
        assert infos["_" + key].dtype == bool and infos["_" + key].all() and infos["_" + key].shape == (N,)


@pytest.mark.parametrize("flexible", [False, True])
def test_fov_entries_are_int64_and_host_rows_win(flexible):
    loc = torch.arange(8, dtype=torch.int32).reshape(N, 2)                               # (CPU tensors stand in for the device's)
    res = torch.full((N, 2), 30, dtype=torch.int32) if flexible else None
    keys = ["fov_loc", "fov_res"] if flexible else ["fov_loc"]
    host = fov_entries(loc, res, True)
    assert list(host) == keys and all(isinstance(v, np.ndarray) and v.dtype == np.int64 for v in host.values())
    assert np.array_equal(host["fov_loc"], loc.numpy())
    dev = fov_entries(loc, res, False)
    assert list(dev) == keys and all(isinstance(v, torch.Tensor) and v.dtype == torch.int64 for v in dev.values())
    assert torch.equal(dev["fov_loc"], loc.long())
    # rows the chunked step already brought home take the device tensors' place
    h_loc = np.full((N, 2), 7, np.int32)
    h_res = np.full((N, 2), 9, np.int32) if flexible else None
    won = fov_entries(loc, res, True, h_loc, h_res)
    assert list(won) == keys and won["fov_loc"].dtype == np.int64 and np.array_equal(won["fov_loc"], h_loc)
    if flexible:
        assert won["fov_res"].dtype == np.int64 and np.array_equal(won["fov_res"], h_res)
    assert fov_entries(None, None, True) == {} and fov_entries(None, None, False) == {}
