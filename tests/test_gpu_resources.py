"""GPU: what the handles of libagx hold and give back (csrc/agx_resources.h).  Public API only: the device bytes the frame
history, the step log and the prioritized sampler report are their section formulas, create / close cycles of every handle kind
leave the device's free memory where it was, and a native step loop with host outputs is made, stepped and closed repeatedly.
The failure paths (the k-th allocation of a create refused) are tests/resources_harness.cpp's, against a mocked runtime."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _al(b):
    return (b + 255) & ~255           # every section of a handle's block is padded to 256 bytes


def _handles(pipe, capacity, payload=12):
    """One handle of each kind on a new history of `pipe`; everything is the pipeline's to close (active_gym/lifetime.py)."""
    from active_gym.augment import RandomShift
    from active_gym.history import FrameHistory
    from active_gym.minibatch import Minibatcher
    from active_gym.priority import PrioritizedSampler
    from active_gym.replay import ReplaySampler
    from active_gym.rollout import Rollout
    from active_gym.steplog import StepLog
    hist = FrameHistory(pipe, capacity)
    log = StepLog(hist, payload)
    made = dict(hist=hist, replay=ReplaySampler(hist), log=log, prio=PrioritizedSampler(hist, back=1, forward=1), shift=RandomShift(hist),
                mb=Minibatcher(Rollout(log)))
    return made


def _pipe(kind, N, fs=4):
    from active_gym import ObsPipeline
    kw = dict(fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute", resize_to_full=True) if kind == "fixed" else {}
    return ObsPipeline(num_envs=N, kind=kind, obs_size=(84, 84), frame_stack=fs, device=torch.device(DEV), **kw)


def test_reported_bytes_are_the_section_formulas():
    """N = 3, 84 x 84, capacity 5, payload 12, back = forward = 1: frames | loc | count | age, stamp | reward | flags | payload and
    stamp | incl | csum | envsum | envacc | off | state | weight | cacc | wmax, each section padded to 256 bytes.  Twice in one
    process, on a fixed-fovea and on a base context, closed through the pipeline (children first)."""
    N, T, W, px = 3, 5, 12, 84 * 84
    rows, chunks = T * N, N * ((T + 63) // 64)               # a chunk of the prioritized sampler is 64 rows of one env
    want_hist = _al(T * N * px) + _al(T * N * 2 * 4) + _al(N * 8) + _al(T * N)
    want_log = _al(rows * 8) + _al(rows * 4) + _al(rows) + _al(rows * W)
    want_prio = (2 * _al(rows * 8) + _al(chunks * 8) + 2 * _al(N * 8) + _al((N + 1) * 8) + _al(3 * 8) + _al(rows * 4) + _al(chunks * 4)
                 + _al(4))
    assert (want_hist, want_log, want_prio) == (106752, 1024, 2560)
    for kind in ("fixed", "base", "fixed", "base"):
        pipe = _pipe(kind, N)
        h = _handles(pipe, T, W)
        assert h["hist"].nbytes == want_hist
        assert h["log"].bytes() == want_log
        assert h["prio"].bytes() == want_prio
        pipe.close()
        assert not any(v.alive for v in h.values()) and not pipe.alive
    torch.cuda.synchronize()


def test_create_close_cycles_leave_free_memory_where_it_was():
    """A base context of 16 envs with a 512-step history (one block of about 58 MB) and one handle of each other kind, made and
    closed 20 times: the device's free memory after cycle 20 is not below that after cycle 1 by more than half a history block (a
    block leaked per cycle would cost 19 of them)."""
    N, T = 16, 512
    free, nbytes = [], 0
    for _ in range(20):
        pipe = _pipe("base", N)
        h = _handles(pipe, T)
        nbytes = h["hist"].nbytes
        pipe.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(torch.device(DEV))[0])
    assert nbytes == _al(T * N * 84 * 84) + _al(T * N * 8) + _al(N * 8) + _al(T * N) and nbytes > 57_000_000
    print(f"free after cycle 1: {free[0]}, after cycle 20: {free[-1]}, one history block: {nbytes}")
    assert free[-1] >= free[0] - nbytes // 2, (free[0], free[-1], nbytes)


def test_native_loop_with_host_outputs_cycles():
    """The native step loop with its host-output side prepared (host_obs_chunks = 3), made, stepped once and closed, four times."""
    from active_gym import AtariEnvArgs, AtariVecEnv
    N = 12
    for _ in range(4):
        env = AtariVecEnv(AtariEnvArgs(game="g", seed=2, obs_size=(84, 84), fov_size=(30, 30), fov_init_loc=(0, 0), sensory_action_mode="absolute",
                                       resize_to_full=True, frame_source="native", frame_format="gray", num_workers=2, scripted_lives=2,
                                       scripted_p_life=100, scripted_p_over=30, host_obs_chunks=3), N, kind="fixed")
        assert env._loop is not None and env._host_step is not None
        env.reset()
        obs, *_ = env.step({"motor_action": np.zeros(N, np.int64), "sensory_action": np.full((N, 2), 20, np.int64)})
        assert isinstance(obs, np.ndarray) and obs.shape[0] == N and env._host_step.steps == 1
        loop = env._loop
        env.close()
        assert not loop.alive and not env.pipe.alive
