"""The xy-goals agent's two PPO updates on the device (zenv_xyppo_*) at the edges the new code adds -- the products'
tile and chunk edges are covered for both input widths by test_gpu_ppo_update_shapes.py / test_gpu_hppo_update_shapes.py.
Every comparison of two floating-point results follows ppo_update_ref.check_rule, as test_gpu_xyppo_update.py's do.

Shapes: one env, one frame, skill_len 1 (M = 1 row, one low sample); one window per env (skill_len = T = 5, N 33:
M = 33, 165 low samples); M = 31 and 32 rows (with the 33 above: either side of the per-sample workspace's 32-row
padding); 1 zone and 32 zones at h 31, 32 and 33 (M = 8: the planted rows are every row).  Then a workspace a larger
minibatch has left full of NaN, at both levels."""
import numpy as np
import pytest
import torch

from tests import ppo_update_shapes as S
from tests import xyppo_update_dev as D
from tests import xyppo_update_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
LEVELS = D.LEVELS
HYPER = {"lo": R.LO_HYPER, "hi": R.HI_HYPER}
# name -> config, h, N, T, skill_len
CASES = {
    "one": (S.TSP, 16, 1, 1, 1),
    "w1": (S.CM, 33, 33, 5, 5),
    "m31": (S.CM, 32, 31, 2, 2),
    "m32": (S.CM, 32, 32, 2, 2),
    "z1h31": (S.zones(1), 31, 4, 8, 4),
    "z1h33": (S.zones(1), 33, 4, 8, 4),
    "z32h32": (S.zones(32, zones_keepout=0.30), 32, 4, 8, 4),
    "z32h33": (S.zones(32, zones_keepout=0.30), 33, 4, 8, 4),
    "cm64": (S.CM, 64, 20, 12, 4),
}
_SETUPS = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _SETUPS.values():
        s["env"].set_stream(None)
        s["env"].close()
    D.print_worst(REPORT, "xyppo update shapes", 44)


def _setup(Z, case):
    if case not in _SETUPS:
        spec, h, N, T, L = CASES[case]
        _SETUPS[case] = D.xy_setup(Z, S.make_cfg(Z, spec, num_steps=12), h, N, seed=list(CASES).index(case), T=T, L=L)
    return _SETUPS[case]


@pytest.mark.parametrize("level", ["lo", "hi"])
@pytest.mark.parametrize("case", [c for c in CASES if c != "cm64"])
def test_both_levels_at_the_shape_edges(zenv_mod, case, level):
    s = _setup(zenv_mod, case)
    spec, h, N, T, L = CASES[case]
    assert s["M"] == N * (T // L) and s["total"] == {"lo": N * T, "hi": s["M"]}
    if case == "one":
        assert s["M"] == 1 and s["total"]["lo"] == 1
    if case in ("w1", "m31", "m32"):
        assert s["M"] == {"w1": 33, "m31": 31, "m32": 32}[case] == N
        assert S.padded_rows(s["M"], s["Z"])[1] == (64 if case == "w1" else 32)
    if case.startswith("z"):
        assert s["Z"] == (1 if case.startswith("z1h") else 32)
    idx = np.arange(s["total"][level])
    planted = level == "hi" and s["M"] >= D.PLANTED
    if planted:
        D.assert_planted_branches(s)
    stats, s64, s32 = D.xy_check_minibatch(zenv_mod, s, level, s["sd"][level], idx, HYPER[level], f"edge-{case}", REPORT)
    if not planted:                                         # records as collected: ratio = 1
        adv = D.xy_batch(s, level, idx, F64)["advantage"]
        R.check_rule(f"edge-{case}/{level}.policy_loss_at_ratio_1", stats[3], -float(adv.mean()), s32["policy_loss"], REPORT)
    assert stats[2] == 0.0


@pytest.mark.parametrize("level", ["lo", "hi"])
def test_a_smaller_minibatch_reads_nothing_a_larger_one_left(zenv_mod, level):
    """A minibatch of every sample on NaN observations leaves NaN in the workspace's rows; minibatches of 5 and of 37
    samples on the same learner then give the bits a freshly initialised learner gives."""
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "cm64")
    env, tenv, lv, total, T = s["env"], s["tenv"], LEVELS[level], s["total"][level], s["T"]
    assert total > 37
    D.xy_init(s)                                            # max_batch = every sample
    with torch.cuda.device(tenv.device):
        obs = tenv._alias(nat.F_EXP_OBS, (T, s["N"], 8), np.float32) if level == "lo" else s["hi_t"]["obs"]
    assert obs.shape == ((T, s["N"], 8) if level == "lo" else (s["M"], 8))
    saved = obs.clone()
    try:
        obs.fill_(float("nan"))
        torch.cuda.synchronize()
        env.xyppo_minibatch(lv, np.arange(total, dtype=np.int32))
        assert np.all(np.isnan(env.xyppo_stats(lv)[0][[0, 1, 3, 4, 5]])) and np.any(np.isnan(D.grad_arena(s, lv)))
    finally:
        obs.copy_(saved)
        torch.cuda.synchronize()
    batches = [D.xy_indexes(s, level, n, 9).astype(np.int32) for n in (5, 37)]
    stale = []
    for idx in batches:
        env.xyppo_minibatch(lv, idx)
        stale.append((env.xyppo_stats(lv).copy(), D.grad_arena(s, lv)))
    for idx, (stats, arena) in zip(batches, stale):
        D.xy_init(s)
        env.xyppo_minibatch(lv, idx)
        assert np.all(np.isfinite(stats)) and np.all(np.isfinite(arena)) and float(np.abs(arena).max()) > 0
        np.testing.assert_array_equal(stats, env.xyppo_stats(lv))
        np.testing.assert_array_equal(arena, D.grad_arena(s, lv))
