"""CPU: the layout sampler written once for host and device (csrc/layout_sampler.hpp), through its host instantiation
zenv_sample_layout_shared -- it must give what the host sampler (zenv_sample_layout, pinned to numpy by
tests/golden/reset_vectors.npz) gives, bit for bit, restarts included; the threshold that replaces the keepout test's
square root must decide as the square root does; and the C boundary of the device-sampling calls is complete."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reset_vectors.npz"))

# name -> (config maker, seeds)
CASES = {
    "PointTSP-v0": (lambda Z: Z.config_for_id("PointTSP-v0"), range(1, 3001)),
    "ColourMatch-v0": (lambda Z: Z.config_for_id("ColourMatch-v0"), range(1, 3001)),
    "z25k40": (lambda Z: Z.default_config(0, 25, zones_keepout=0.40), range(1, 3001)),
    "z32k35": (lambda Z: Z.default_config(0, 32, zones_keepout=0.35), range(1, 201)),
    "z1": (lambda Z: Z.default_config(0, 1), range(1, 201)),
    "PointTSP-v4": (lambda Z: Z.config_for_id("PointTSP-v4"), range(1, 201)),
    "PointTSP-v5": (lambda Z: Z.config_for_id("PointTSP-v5"), range(1, 201)),
    "seed-range-ends": (lambda Z: Z.config_for_id("PointTSP-v0"), (2 ** 32 - 2, 0)),
    "seed-range-ends-colours": (lambda Z: Z.config_for_id("ColourMatch-v0"), (2 ** 32 - 2, 0)),
}


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_sampler_equals_the_host_sampler(zenv_mod, name):
    Z = zenv_mod
    make, seeds = CASES[name]
    cfg = make(Z)
    restarts = {}
    for s in seeds:
        want, got = Z.sample_layout(cfg, s), Z.sample_layout_shared(cfg, s)
        assert _same(want, got), (name, s, want, got)
        restarts[s] = want[3]
    # the cases are what they are meant to be: deep restarts (and with them a second twist) are in
    if name == "PointTSP-v0":
        assert restarts[188] == 15 == max(restarts.values())
        assert sum(r > 0 for r in restarts.values()) > 1500
    if name == "z25k40":
        assert restarts[1859] == 4 == max(restarts.values())
    if name == "ColourMatch-v0":
        assert max(restarts.values()) == 0


@pytest.mark.parametrize("tag,task,zones,keepout", [("z15", 0, 15, 0.55), ("z6", 2, 6, 0.55), ("z5", 0, 5, 0.55),
                                                    ("z25k40", 0, 25, 0.40)])
def test_shared_sampler_matches_golden(zenv_mod, tag, task, zones, keepout):
    Zm = zenv_mod
    cfg = Zm.default_config(task, zones, zones_keepout=keepout)
    for i, s in enumerate(GOLD["seeds"]):
        robot, zxy, aux, restarts = Zm.sample_layout_shared(cfg, int(s))
        assert np.array_equal(robot, GOLD[f"robot_{tag}"][i])
        assert np.array_equal(zxy, GOLD[f"zones_{tag}"][i])
        assert restarts == GOLD[f"restarts_{tag}"][i]
        if tag == "z6":
            assert np.array_equal(aux, GOLD["colours_z6"][i])


def test_shared_sampler_errors(zenv_mod):
    Z = zenv_mod
    with pytest.raises(Z.ZenvError) as ei:
        Z.sample_layout_shared(Z.default_config(0, 25), 1)          # 0.55 keepout cannot hold 25 zones
    assert ei.value.code == Z.E_LAYOUT
    for seed in (2 ** 32 - 1, -1):
        with pytest.raises(Z.ZenvError) as ei:
            Z.sample_layout_shared(Z.config_for_id("PointTSP-v0"), seed)
        assert ei.value.code == Z.E_ARG and "2**32 - 1" in str(ei.value)
    with pytest.raises(Z.ZenvError) as ei:                           # deadlines need the host libm's log
        Z.sample_layout_shared(Z.config_for_id("PointTTSP-v0"), 1)
    assert ei.value.code == Z.E_ARG and "TimedTSP" in str(ei.value)
    # the restart count of the failure is the reference's limit
    cfg = Z.default_config(0, 25)
    r = C.c_int32(-1)
    assert Z._native.lib().zenv_sample_layout_shared(C.byref(cfg), 1, None, None, None, C.byref(r)) == Z.E_LAYOUT
    assert r.value == 10000


@pytest.mark.parametrize("name", sorted(n for n in CASES if not n.startswith("seed-range")))
def test_threshold_decides_as_the_square_root(zenv_mod, name):
    """sqrt(s) < A  <=>  s < T: at T, at its two neighbours and at 10^5 random s around A^2, for both right-hand sides."""
    Z = zenv_mod
    cfg = CASES[name][0](Z)
    rhs, thr = Z.layout_thresholds(cfg)
    assert rhs[0] == (cfg.robot_keepout + cfg.placements_margin) + cfg.zones_keepout
    assert rhs[1] == (cfg.zones_keepout + cfg.placements_margin) + cfg.zones_keepout
    rng = np.random.default_rng(12345)
    for A, T in zip(rhs.tolist(), thr.tolist()):
        assert A > 0 and T > 0
        below, above = math.nextafter(T, 0.0), math.nextafter(T, math.inf)
        assert math.sqrt(below) < A <= math.sqrt(T) <= math.sqrt(above)      # T is the boundary itself
        near = np.array([below, T, above])
        # a few thousand ulps either side of A^2 (where rounding decides) and a wide band around it
        ulps = A * A + np.spacing(A * A) * rng.integers(-4000, 4001, 50000)
        wide = A * A * rng.uniform(0.5, 1.5, 50000)
        for s in (near, ulps, wide):
            assert np.array_equal(np.sqrt(s) < A, s < T)


def test_names_abi_and_ctypes_table(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    text = open(os.path.join(ROOT, "include", "zenv.h")).read()
    names = ("zenv_sample_layout_shared", "zenv_layout_thresholds", "zenv_bank_build_device",
             "zenv_bank_build_seeds_device", "zenv_bank_update_device", "zenv_ring_stream", "zenv_ring_refill",
             "zenv_sample_status", "zenv_bank_read")
    for name in names:
        assert f"int {name}(" in text and hasattr(nat.lib(), name) and name in nat.exported_symbols()
    assert "int zenv_bank_build_device(zenv_t *h, int64_t seed_first, int count);" in text
    assert "int zenv_bank_build_seeds_device(zenv_t *h, const int64_t *seeds, int count);" in text
    assert "int zenv_bank_update_device(zenv_t *h, const int32_t *slots, const int64_t *seeds, int count);" in text
    assert "int zenv_ring_stream(zenv_t *h, const int64_t *seed0, int32_t depth);" in text
    assert "int zenv_ring_refill(zenv_t *h);" in text
    assert ("int zenv_sample_status(zenv_t *h, int32_t *slots, int64_t *seeds, int32_t *codes, int cap, int32_t *n_failed,\n"
            "                       int64_t *n_sampled_total);") in text
    assert ("int zenv_bank_read(zenv_t *h, int slot_first, int count, double *robot4, double *zone_xy, int32_t *aux,\n"
            "                   int64_t *seeds, float *first12);") in text
    assert "#define ZENV_DEVICE_RESTARTS 256\n" in text and "#define ZENV_SAMPLE_STATUS_CAP 1024\n" in text
    assert "ZENV_SAMPLE_UNFINISHED = 1, ZENV_SAMPLE_SEED_RANGE = 2" in text
    assert (nat.DEVICE_RESTARTS, nat.SAMPLE_STATUS_CAP, nat.SAMPLE_UNFINISHED, nat.SAMPLE_SEED_RANGE) == (256, 1024, 1, 2)
    assert (Z.DEVICE_RESTARTS, Z.SAMPLE_UNFINISHED, Z.SAMPLE_SEED_RANGE) == (256, 1, 2)
    # the sampler has the host sampler's signature
    assert nat._PROTOTYPES["zenv_sample_layout_shared"] == nat._PROTOTYPES["zenv_sample_layout"]
    lib = nat.lib()
    # null handles / arguments answer E_ARG before anything touches a device
    for call in (lambda: lib.zenv_bank_build_device(None, 1, 1), lambda: lib.zenv_bank_build_seeds_device(None, None, 1),
                 lambda: lib.zenv_bank_update_device(None, None, None, 1), lambda: lib.zenv_ring_stream(None, None, 1),
                 lambda: lib.zenv_ring_refill(None), lambda: lib.zenv_sample_status(None, None, None, None, 0, None, None),
                 lambda: lib.zenv_bank_read(None, 0, 0, None, None, None, None, None),
                 lambda: lib.zenv_sample_layout_shared(None, 1, None, None, None, None),
                 lambda: lib.zenv_layout_thresholds(None, None, None)):
        assert call() == Z.E_ARG and b"null" in lib.zenv_last_error()


def test_python_surface_and_build_sources(zenv_mod):
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import build
    from combinatorial_rl_tasks_amd.penv import ParallelEnv
    for src in ("layout_sample.hip", "zenv_layout.cpp"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src))
    assert os.path.exists(os.path.join(build.CSRC, "layout_sampler.hpp"))
    want = {"build_bank_device": ["seed_first", "count"], "build_bank_seeds_device": ["seeds"],
            "update_bank_device": ["slots", "seeds"], "ring_stream": ["seed0", "depth"], "ring_refill": [],
            "sample_status": [], "read_bank": ["first", "count"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(Z.ZoneVecEnv, name)).parameters)[1:] == params, name
    sig = inspect.signature(ParallelEnv.__init__)
    assert sig.parameters["device_layouts"].default is False
    assert list(sig.parameters)[1:] == ["envs", "device", "episodes_per_env", "device_layouts"]
    assert "--fresh-layouts" in open(os.path.join(ROOT, "examples", "ppo_torch.py")).read()
    assert os.path.exists(os.path.join(ROOT, "scripts", "layout_sample_time.py"))
