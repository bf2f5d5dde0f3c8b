"""CPU: the inputs of the device sampler's scale tests (tests/layout_scale_cases.py) are what the GPU tests need them to
be -- the grid cap and the failure list's size the counts were chosen for, a config whose seeds give up on the device more
often than the list holds while the host finishes every one, and a neighbour the host fails on at a known seed -- and the
shared sampler's host instantiation follows the host sampler thousands of restarts deep on that config."""
import os

import numpy as np

from tests.layout_scale_cases import HOST_ATTEMPTS, MAX_GRID, PASSES3, host_restarts, tight_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_the_counts_were_chosen_for(zenv_mod):
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import build
    layout = open(os.path.join(build.CSRC, "zenv_layout.cpp")).read()
    header = open(os.path.join(ROOT, "include", "zenv.h")).read()
    assert "constexpr int kMaxGrid = 256 * 32;" in layout and MAX_GRID == 256 * 32 and PASSES3 == 2 * MAX_GRID + 1
    assert "#define ZENV_SAMPLE_STATUS_CAP 1024" in header and Z.SAMPLE_STATUS_CAP == 1024
    assert "#define ZENV_DEVICE_RESTARTS 256" in header and Z.DEVICE_RESTARTS == 256
    assert HOST_ATTEMPTS == 10000 and "kSamplerHostAttempts = 10000;" in open(
        os.path.join(build.CSRC, "layout_sampler.hpp")).read()


def test_tight_gives_up_on_the_device_more_often_than_the_list_holds(zenv_mod):
    Z = zenv_mod
    cfg = tight_config(Z)
    assert (cfg.num_zones, cfg.n_robot_locations, cfg.zones_keepout) == (1, 1, 1.589)
    assert (cfg.robot_location[0], cfg.robot_location[1]) == (0.0, 0.0)
    r = host_restarts(Z, 1.589, 1, 2001)
    cap = Z.SAMPLE_STATUS_CAP
    assert r.max() < HOST_ATTEMPTS                            # no host failure
    hard = r > Z.DEVICE_RESTARTS
    for window in (hard[:2000], hard[1:]):                    # seeds 1..2000 (the build) and 2..2001 (the ring's refill)
        assert cap < window.sum() < 2 * cap                   # a second pass of the repair loop names the rest
        assert not window.all()


def test_the_neighbour_the_host_cannot_finish(zenv_mod):
    Z = zenv_mod
    r = host_restarts(Z, 1.590, 1, 2000)
    assert np.flatnonzero(r >= HOST_ATTEMPTS)[0] + 1 == 1078
    assert (r > Z.DEVICE_RESTARTS).sum() > Z.SAMPLE_STATUS_CAP


def test_shared_sampler_follows_the_host_sampler_on_tight(zenv_mod):
    Z = zenv_mod
    cfg = tight_config(Z)
    r = host_restarts(Z, 1.589, 1, 2001)
    bad = []
    for seed in range(1, 2002):
        want, got = Z.sample_layout(cfg, seed), Z.sample_layout_shared(cfg, seed)
        if not (all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(want[:3], got[:3]))
                and want[3] == got[3] == r[seed - 1]):
            bad.append(seed)
    assert bad == []
    assert r.max() > 1000                                     # thousands of restarts deep
