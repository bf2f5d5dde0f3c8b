"""Inputs of the device layout sampler's scale tests (tests/test_layout_scale_cases_cpu.py pins them without a GPU,
tests/test_gpu_layout_scale.py and tests/test_gpu_route_solver.py run them): counts beyond one grid of the
sampling kernels, and a config the device sampler gives up on more often than its failure list holds."""
import numpy as np

MAX_GRID = 8192                  # kMaxGrid of csrc/zenv_layout.cpp: one wave per block, grid = min(count, kMaxGrid)
PASSES3 = 2 * MAX_GRID + 1       # block 0 makes three trips of the grid-stride loop, every other block two
HOST_ATTEMPTS = 10000            # the host sampler's attempts: what a seed it cannot finish counts as

_restarts = {}


def tight_config(Z, keepout=1.589):
    """TIGHT: one zone, the robot fixed in the middle.  The zone fits only in the corners of the box, so most seeds
    need hundreds of restarts and some thousands; with keepout 1.590 the host gives up on seed 1078."""
    return Z.default_config(0, 1, zones_keepout=keepout, robot_locations=[(0.0, 0.0)])


def host_restarts(Z, keepout, seed_first, seed_last):
    """int64 [seed_last - seed_first + 1]: the host sampler's restarts for tight_config(keepout) at the seeds
    seed_first .. seed_last; HOST_ATTEMPTS where it fails.  Computed once per range."""
    key = (keepout, seed_first, seed_last)
    if key not in _restarts:
        cfg = tight_config(Z, keepout)
        out = np.zeros(seed_last - seed_first + 1, np.int64)
        for i, seed in enumerate(range(seed_first, seed_last + 1)):
            try:
                out[i] = Z.sample_layout(cfg, seed)[3]
            except Z.ZenvError as e:
                if e.code != Z.E_LAYOUT:
                    raise
                out[i] = HOST_ATTEMPTS
        out.setflags(write=False)
        _restarts[key] = out
    return _restarts[key]
