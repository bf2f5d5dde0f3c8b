"""DIAYN's device learner at the edges of its shapes (zenv_diayn_*): the head's width S, the hidden size around a tile of
32 and at its limit, one and two zones, minibatch counts around a row tile, zone rows around a chunk of 256 and 17 chunks
(the split reduce), a smaller minibatch after a larger one on NaN observations, and the compaction around its block
(kInvBlock = 1024 sample indexes per block of 256 threads x 4) and across a tile of its scan (kInvScan = 64 block
counts, so more than 65 536 sample indexes).  The rule is ppo_update_ref.check_rule."""
import numpy as np
import pytest
import torch

from tests import diayn_update_dev as D
from tests import diayn_update_ref as R

pytestmark = pytest.mark.gpu

INV_BLOCK, INV_SCAN = 1024, 64        # csrc/ppo_update.hpp: kInvBlock, kInvScan
_SETUPS = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _SETUPS.values():
        s["env"].set_stream(None)
        s["env"].close()
    D.print_worst(REPORT, "diayn shapes", 44)


def _setup(Z, env_id="PointTSP-v0", h=32, N=16, S=5, T=12, L=4, zones=None, steps=10):
    key = (env_id, h, N, S, T, L, zones, steps)
    if key not in _SETUPS:
        over = dict(num_steps=steps)
        if zones is not None:
            over["num_zones"] = zones
        _SETUPS[key] = D.dy_setup(Z, Z.config_for_id(env_id, **over), h, N, S, seed=len(_SETUPS), T=T, L=L)
    return _SETUPS[key]


@pytest.mark.parametrize("S", [1, 2, 31, 32])
def test_head_widths(zenv_mod, S):
    s = _setup(zenv_mod, S=S)
    idx = D.dy_indexes(s, "all", 0)
    stats, grads = D.dy_check_minibatch(zenv_mod, s, s["sd"], idx, f"S{S}", REPORT)
    if S == 1:                        # one skill: the probability is exactly 1
        assert stats[0] == 0.0 and stats[5] == 0.0
        assert all(np.all(g == 0) for g in grads.values())
    else:
        assert len(set(R.batch(s["lo"], idx, torch.float64)["skill"].tolist())) > S // 2


@pytest.mark.parametrize("env_id,h", [("PointTSP-v0", 31), ("ColourMatch-v0", 32), ("PointTSP-v0", 33),
                                      ("ColourMatch-v0", 191)])
def test_hidden_sizes(zenv_mod, env_id, h):
    s = _setup(zenv_mod, env_id=env_id, h=h, S=32 if h == 191 else 5)
    D.dy_check_minibatch(zenv_mod, s, s["sd"], D.dy_indexes(s, 40, 1), f"h{h}", REPORT)


@pytest.mark.parametrize("zones", [1, 2])
def test_one_and_two_zones(zenv_mod, zones):
    s = _setup(zenv_mod, zones=zones, N=32, steps=50)
    assert s["Z"] == zones
    D.dy_check_minibatch(zenv_mod, s, s["sd"], D.dy_indexes(s, 40, 2), f"Z{zones}", REPORT)


@pytest.mark.parametrize("count", [1, 31, 32, 33])
def test_minibatch_counts_around_a_row_tile(zenv_mod, count):
    s = _setup(zenv_mod)
    D.dy_check_minibatch(zenv_mod, s, s["sd"], D.dy_indexes(s, count, 3), f"count{count}", REPORT)


@pytest.mark.parametrize("rows", [255, 256, 257])
def test_zone_rows_around_a_chunk(zenv_mod, rows):
    s = _setup(zenv_mod, zones=1, N=32, steps=50)          # one zone: a zone row per sample
    assert len(s["kept"]) >= 257
    D.dy_check_minibatch(zenv_mod, s, s["sd"], D.dy_indexes(s, rows, 4), f"rows{rows}", REPORT)


def test_seventeen_chunks_take_the_split_reduce(zenv_mod):
    s = _setup(zenv_mod, N=32, steps=50)                   # 15 zones
    count = 274
    assert s["Z"] == 15 and len(s["kept"]) >= count and (count * 15 + 255) // 256 == 17
    D.dy_check_minibatch(zenv_mod, s, s["sd"], D.dy_indexes(s, count, 5), "chunks17", REPORT)


def test_a_smaller_minibatch_after_a_larger_one_on_nan_observations(zenv_mod):
    """Every workspace row a minibatch reads is written by it: what a NaN minibatch of 64 left behind does not reach a
    minibatch of 5."""
    Z = zenv_mod
    s = _setup(Z)
    env, obs = s["env"], s["lo_t"]["obs"]
    small = D.dy_indexes(s, 5, 6).astype(np.int32)
    large = np.setdiff1d(s["kept"], small)[:64].astype(np.int32)
    assert len(large) == 64
    D.dy_init(s)
    env.diayn_minibatch(small)
    clean = (env.diayn_stats()[0].copy(), D.grad_arena(s))
    saved = obs.clone()
    try:
        T1 = s["T"] - 1
        for i in large:
            obs[int(i) // T1, int(i) % T1 + 1] = float("nan")
        torch.cuda.synchronize()
        env.diayn_minibatch(large)
        assert np.isnan(env.diayn_stats()[0][0])
        env.diayn_minibatch(small)
        np.testing.assert_array_equal(env.diayn_stats()[0], clean[0])
        np.testing.assert_array_equal(D.grad_arena(s), clean[1])
    finally:
        obs.copy_(saved)
        torch.cuda.synchronize()


@pytest.mark.parametrize("N,T,L", [(33, 32, 4), (32, 33, 3), (25, 42, 6), (64, 1026, 27)])
def test_compaction_around_a_block_and_across_a_scan_tile(zenv_mod, N, T, L):
    Z = zenv_mod
    total = N * (T - 1)
    assert total in (INV_BLOCK - 1, INV_BLOCK, INV_BLOCK + 1) or total > INV_BLOCK * INV_SCAN
    s = _setup(Z, h=16, N=N, T=T, L=L, steps=10)
    env, mask = s["env"], s["lo_t"]["mask"]
    np.testing.assert_array_equal(env.diayn_samples(), s["kept"])         # as collected
    rng = np.random.default_rng(total)
    saved = mask.clone()
    try:
        for p in (0.5, 0.02, 1.0):
            m = (rng.random((N, T)) < p).astype(np.float32)
            m[-1, -1] = 1.0                                               # the last sample index is kept
            mask.copy_(torch.as_tensor(m, device=mask.device))
            D.refresh(s)
            got = env.diayn_samples()
            np.testing.assert_array_equal(got, s["kept"])
            assert got[-1] == total - 1 and len(got) == int((m[:, 1:] != 0).sum())
    finally:
        mask.copy_(saved)
        D.refresh(s)
