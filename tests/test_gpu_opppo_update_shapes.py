"""The Options agent's two PPO updates on the device (zenv_opppo_*) at the smallest shapes at which a width can go wrong:
the skill one-hot's widths (K15's) under the three-component head.  Every comparison of two floating-point results
follows ppo_update_ref.check_rule, as test_gpu_opppo_update.py's do.  T = 13 frames: 12 low-level frames per env, 96
samples at N = 8; M, the closed transitions, is what the collection gave (tests/opppo_update_dev.py: at least 8, no
multiple of 32).

  S = 1, 2, 5, 24, 25, 32 on 7-feature zone rows (ColourMatch-v0): XD = 8 + S is 32 and 33 at S = 24 and 25, zone_net_.0's
      gathered input W1C is 24, 24, 24, 40, 48, 48 columns, and the high level's logit buffer is full at S = 32
  h = 31, 32, 33: either side of a 32-feature tile
  h = 191 with S = 32 on PointTTSP-v0 (F 7): KC = 232 columns -- combine_net_'s product taken in two -- and the widest
      partial; a minibatch of 33 samples
  Z = 1 and 2 zones
  255 / 256 / 257 zone rows (one zone, so as many samples): either side of a 256-row chunk
  more than 16 chunks: 288 samples x 15 zones = 4320 zone rows, 17 chunks, k_ppo_reduce_split
  an M that is no multiple of 32: every high-level case
Then a workspace a larger minibatch has left full of NaN, at both levels.  In every low-level case the three rows of
actor.mu_ / actor.std_ and the seven head-bias sums are compared: with the head image back at two rows per head, or the
entropy's divisor back at 2, each of them fails."""
import numpy as np
import pytest
import torch

from tests import ppo_update_shapes as SH
from tests import opppo_update_dev as D
from tests import opppo_update_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
LEVELS = D.LEVELS
HYPER = {"lo": R.LO_HYPER, "hi": R.HI_HYPER}
TTSP = ("id", "PointTTSP-v0")
T = 13
TL = T - 1                  # low-level frames per env
# name -> config, h, N, S
CASES = {
    "s1": (SH.CM, 16, 8, 1), "s2": (SH.CM, 16, 8, 2), "s5": (SH.CM, 16, 8, 5), "s24": (SH.CM, 16, 8, 24),
    "s25": (SH.CM, 16, 8, 25), "s32": (SH.CM, 16, 8, 32),
    "h31": (SH.CM, 31, 8, 5), "h32": (SH.CM, 32, 8, 5), "h33": (SH.CM, 33, 8, 5),
    "wide": (TTSP, 191, 8, 32),
    "z1": (SH.zones(1), 16, 8, 5), "z2": (SH.zones(2), 16, 8, 5),
    "rows": (SH.zones(1), 16, 22, 5),          # 22 x 12 = 264 samples
    "chunks": (SH.TSP, 16, 24, 5),
    "cm64": (SH.CM, 64, 8, 5),
}
BOTH = [c for c in CASES if c not in ("rows", "chunks", "cm64")]
_SETUPS = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _SETUPS.values():
        s["env"].set_stream(None)
        s["env"].close()
    D.print_worst(REPORT, "opppo update shapes", 44)


def _setup(Z, case):
    if case not in _SETUPS:
        spec, h, N, S = CASES[case]
        _SETUPS[case] = D.op_setup(Z, SH.make_cfg(Z, spec, num_steps=12), h, N, S, seed=list(CASES).index(case), T=T)
    return _SETUPS[case]


def widths(s):
    """(XD, W1C, HP, KC) as csrc/zenv_train.cpp lays the low level out."""
    XD = 8 + s["S"]
    HP = (s["h"] + 32) // 32 * 32
    return XD, (XD + s["F"] + 1 + 7) // 8 * 8, HP, HP + (XD + 7) // 8 * 8


@pytest.mark.parametrize("level", ["lo", "hi"])
@pytest.mark.parametrize("case", BOTH)
def test_both_levels_at_the_width_edges(zenv_mod, case, level):
    s = _setup(zenv_mod, case)
    spec, h, N, S = CASES[case]
    M = s["M"]
    assert M >= D.PLANTED and M % 32 != 0 and s["total"]["lo"] == 96 and (s["h"], s["S"]) == (h, S)
    XD, W1C, HP, KC = widths(s)
    if case.startswith("s"):
        assert s["F"] == 7 and (XD, W1C) == {1: (9, 24), 2: (10, 24), 5: (13, 24), 24: (32, 40), 25: (33, 48),
                                             32: (40, 48)}[S]
        assert KC - HP == {1: 16, 2: 16, 5: 16, 24: 32, 25: 40, 32: 40}[S]
    if case.startswith("h"):
        assert HP == {31: 32, 32: 64, 33: 64}[h]
    if case == "wide":
        assert s["F"] == 7 and (HP, KC, W1C) == (192, 232, 48) and (KC + 31) // 32 == 8
    if case.startswith("z"):
        assert s["Z"] == int(case[1:])
    if level == "lo":
        idx = np.arange(96 - 33, 96) if case == "wide" else np.arange(96)
        D.assert_every_skill(s, idx)
    else:
        idx = np.arange(M)
        D.assert_planted_branches(s)
    stats, s64, s32 = D.op_check_minibatch(zenv_mod, s, level, s["sd"][level], idx, HYPER[level], f"edge-{case}", REPORT)
    assert stats[2] == 0.0
    if level == "lo":                                       # the third component's rows are there
        g = D.op_by_key(s["env"], "lo", zenv_mod._native.PPO_GRAD)
        for key in ("actor.mu_.weight", "actor.std_.weight", "actor.mu_.bias", "actor.std_.bias"):
            assert g[key].shape[0] == 3 and float(np.abs(g[key][2]).max()) > 0, key
    if level == "hi" and S == 1:                            # one skill: no entropy, and no gradient through the logits
        g = D.op_by_key(s["env"], "hi", zenv_mod._native.PPO_GRAD)
        assert stats[0] == 0.0
        for key in ("actor.discrete_.0.weight", "actor.discrete_.0.bias", "actor.enc_.0.0.weight", "actor.enc_.0.0.bias"):
            assert np.all(g[key] == 0), key


@pytest.mark.parametrize("batch", [255, 256, 257])
def test_low_level_either_side_of_a_row_chunk(zenv_mod, batch):
    s = _setup(zenv_mod, "rows")
    assert s["Z"] == 1 and s["total"]["lo"] == 264
    idx = np.arange(264 - batch, 264)
    rows, row_chunks, sample_chunks, split = SH.edge_of(batch, s["Z"])
    assert rows == batch and row_chunks == sample_chunks == (2 if batch == 257 else 1) and not split
    D.assert_every_skill(s, idx)
    D.op_check_minibatch(zenv_mod, s, "lo", s["lo_sd"], idx, R.LO_HYPER, f"rows-{batch}", REPORT)


def test_low_level_with_more_than_16_chunks(zenv_mod):
    s = _setup(zenv_mod, "chunks")
    assert s["Z"] == 15 and s["total"]["lo"] == 288
    idx = np.arange(288)
    rows, row_chunks, sample_chunks, split = SH.edge_of(288, s["Z"])
    assert rows == 4320 and row_chunks == 17 and sample_chunks == 2 and split
    D.assert_every_skill(s, idx)
    D.op_check_minibatch(zenv_mod, s, "lo", s["lo_sd"], idx, R.LO_HYPER, "chunks-288", REPORT)


@pytest.mark.parametrize("level", ["lo", "hi"])
def test_a_smaller_minibatch_reads_nothing_a_larger_one_left(zenv_mod, level):
    """A minibatch of every sample on NaN observations leaves NaN in the workspace's rows; minibatches of 5 and of 13
    samples on the same learner then give the bits a freshly initialised learner gives."""
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "cm64")
    env, tenv, lv, total, N = s["env"], s["tenv"], LEVELS[level], s["total"][level], s["N"]
    assert total > 13 + D.PLANTED
    D.op_init(s)                                            # max_batch = every sample
    with torch.cuda.device(tenv.device):
        obs = tenv._alias(nat.F_EXP_OBS, (T, N, 8), np.float32)[:TL] if level == "lo" else s["hi_t"]["obs"]
    assert obs.shape == ((TL, N, 8) if level == "lo" else (s["M"], 8))
    saved = obs.clone()
    try:
        obs.fill_(float("nan"))
        torch.cuda.synchronize()
        env.opppo_minibatch(lv, np.arange(total, dtype=np.int32))
        assert np.all(np.isnan(env.opppo_stats(lv)[0][[0, 1, 3, 4, 5]])) and np.any(np.isnan(D.grad_arena(s, lv)))
    finally:
        obs.copy_(saved)
        torch.cuda.synchronize()
    batches = [D.op_indexes(s, level, n, 9).astype(np.int32) for n in (5, 13)]
    stale = []
    for idx in batches:
        env.opppo_minibatch(lv, idx)
        stale.append((env.opppo_stats(lv).copy(), D.grad_arena(s, lv)))
    for idx, (stats, arena) in zip(batches, stale):
        D.op_init(s)
        env.opppo_minibatch(lv, idx)
        assert np.all(np.isfinite(stats)) and np.all(np.isfinite(arena)) and float(np.abs(arena).max()) > 0
        np.testing.assert_array_equal(stats, env.opppo_stats(lv))
        np.testing.assert_array_equal(arena, D.grad_arena(s, lv))
