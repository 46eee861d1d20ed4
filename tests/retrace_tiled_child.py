"""Child process of tests/test_gpu_retrace.py::test_tiled_form_of_the_experiments_build_equals_the_model: runs with AGX_LIB =
libagx_exp.so and AGX_RETRACE_TILED = 1, so that a batch-major call takes the LDS-tiled kernel
(active-gym_amd/csrc/experiments/agx_retrace_tiled.h), and holds every element of every output of every batch-major case of
the parent's shapes against tests/retrace_model.py.  Prints "TILED_OK <elements>"."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "active-gym_amd"))

import retrace_model as rm  # noqa: E402
import test_gpu_retrace as tg  # noqa: E402


def main():
    from active_gym import _native as nat
    assert os.environ.get("AGX_RETRACE_TILED") == "1" and "libagx_exp" in os.environ.get("AGX_LIB", "")
    rig, compared = tg.Rig(), 0
    assert "libagx_exp" in open("/proc/self/maps").read(), nat.build_info()
    for B in rm.BS:
        for L in rm.LS:
            k = rm.case(B, L, 1000 * B + L, live_specials=(B + L) % 2 == 0)
            opt = tg._passed(B, L)
            want = rm.retrace(**(k if opt["boot"] else dict(k, boot=None)))
            got = rig.call(k, False, **opt)
            assert rm.same(got[0], want[0]), (B, L)
            assert got[1] is None or rm.same(got[1], want[1]), (B, L)
            assert got[2] is None or np.array_equal(got[2], want[2]), (B, L)
            compared += sum(B * L for g in got if g is not None)
    rig.pipe.close()
    print(f"TILED_OK {compared}")


if __name__ == "__main__":
    main()
