"""CPU: bench.py's options and the --dump-outputs writer (what is sampled, in which types, within the size limit)."""
import os

import numpy as np
import torch

import bench

OBS_ROW = 4 * 84 * 84 * 4              # one env's f32 observation stack at the headline configuration


def test_plain_run_is_the_default_and_steps_are_taken_as_given():
    a = bench.parse(["--steps", "37", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 37 and a.warmup == 3
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_selection_whole_when_it_fits_else_a_fixed_seeded_sample():
    assert bench.dump_selection({"obs": (64, OBS_ROW), "fov_loc": (64, 16)}) == {"obs": None, "fov_loc": None}
    sizes = {"obs": (1024, OBS_ROW), "fov_loc": (1024, 16)}
    s = bench.dump_selection(sizes)
    assert s["fov_loc"] is None                                  # small outputs stay whole
    rows = s["obs"]
    assert 0 < len(rows) < 1024 and np.all(np.diff(rows) > 0) and rows[-1] < 1024
    assert len(rows) * (OBS_ROW + 8) + 1024 * 16 <= bench.DUMP_BUDGET
    assert np.array_equal(bench.dump_selection(sizes)["obs"], rows)        # same arguments, same rows


def test_dump_outputs_types_and_size_limit(tmp_path):
    g = torch.Generator().manual_seed(0)
    outs = {"obs": torch.rand((1024, 4, 84, 84), generator=g), "fov_loc": torch.randint(0, 55, (1024, 2), dtype=torch.int32, generator=g),
            "offsets": torch.arange(1025, dtype=torch.int64) * 3600}
    bench.dump_outputs(str(tmp_path), outs)
    files = sorted(os.listdir(tmp_path))
    assert files == ["fov_loc.npy", "obs.npy", "obs_rows.npy", "offsets.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64_000_000
    got = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert got["obs"].dtype == np.float32 and got["fov_loc"].dtype == np.float64 and got["offsets"].dtype == np.float64
    rows = got["obs_rows"].astype(np.int64)
    assert np.array_equal(got["obs"], outs["obs"].numpy()[rows])
    assert np.array_equal(got["fov_loc"], outs["fov_loc"].numpy().astype(np.float64))
    assert np.array_equal(got["offsets"], outs["offsets"].numpy().astype(np.float64))
