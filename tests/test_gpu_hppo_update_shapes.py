"""The Zone-goals agent's two PPO updates on the device (zenv_hppo_*, ppo_update.hip) at a large M and at the edges of
their tiles, chunks and zone counts (the table of tests/ppo_update_shapes.py, checked on the CPU by
test_ppo_update_shapes_cpu.py), on the records of a real zenv_collect_hier.  Every comparison of two floating-point
results follows ppo_update_ref.check_rule, as test_gpu_hppo_update.py's do.

Handles as there: goal-enabled, episodes of 12 steps, T = 33 frames, rows 0-7 of the high level planted.  Shapes: 16
zones with N 160 (h 33; M >= 320: the high level on 255, 256 and 257 rows -- 16 chunks of zone rows, the last plain
reduce of a split learner, and 17, the first split with a one-chunk segment and empty ones -- and on all M rows, two
sample chunks; the low level on 256, 257 and 1000 samples), 2 zones (h 31, N 8), 32 zones (h 32, N 8), PointTSP-v0 at
h 128 (N 8).  Then a workspace a larger minibatch has left full of NaN, at both levels."""
import numpy as np
import pytest
import torch

from tests import hppo_update_ref as R
from tests import ppo_update_dev as D
from tests import ppo_update_shapes as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
T = D.HIER_T
LEVELS = D.LEVELS
HYPER = {"lo": R.LO_HYPER, "hi": R.HI_HYPER}
_SETUPS = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _SETUPS.values():
        s["env"].set_stream(None)
        s["env"].close()
    D.print_worst(REPORT, "hppo update shapes", 44)


def _setup(Z, case):
    """One handle per row of the table: fresh parameters in the acting agent, one collect_hier, rows 0-7 planted."""
    if case not in _SETUPS:
        row = S.HIER[case]
        s = D.hier_setup(Z, S.make_cfg(Z, row["cfg"], num_steps=12), row["h"], row["N"], row["seed"])
        assert (s["Z"], s["F"]) == (row["Z"], row["F"])
        _SETUPS[case] = s
    return _SETUPS[case]


EDGES = [(case, level, batch) for case in ("bigM", "z2", "z32", "h128") for level in ("hi", "lo")
         for batch in S.HIER[case][level]]


@pytest.mark.parametrize("case,level,batch", EDGES)
def test_both_levels_at_the_shape_edges(zenv_mod, case, level, batch):
    s = _setup(zenv_mod, case)
    idx = D.hier_indexes(s, level, batch, 2 if level == "hi" else 1)
    n = len(idx)
    assert s["total"][level] - 1 in idx and n == (s["total"][level] if batch == "all" else batch)
    rows, row_chunks, sample_chunks, split = S.edge_of(n, s["Z"])
    print(f"{case} {level}: {n} samples, {rows} zone rows in {row_chunks} chunks, {sample_chunks} sample chunks, M {s['M']}")
    if (case, level, n) in S.HIER_EDGES:
        assert (rows, row_chunks, split) == S.HIER_EDGES[case, level, n]
    if case == "bigM":
        assert s["M"] >= 320 and (batch == "all" or (case, level, n) in S.HIER_EDGES)
    if (case, batch) == ("bigM", "all"):
        # two chunks of samples (k_ppo_tn per sample, k_ppo_stats striding past its 256 threads), > 16 of zone rows
        assert n == s["M"] > S.CHUNK and sample_chunks >= 2 and row_chunks > S.SPLIT and split
    if level == "hi" and batch == "all":                    # the planted rows: every branch has a sample
        b = D.hier_batch(s, "hi", idx, F64)
        hi, lo, val = R.branches("hi", R.model_from("hi", s["hi_sd"], s["F"], F64), b, R.HI_HYPER["clip_eps"])
        assert bool(hi[2]) and bool(lo[5]) and bool(val[6]) and bool(val[7]) and not bool(hi[3]) and not bool(lo[4])
        n_avail = b["action_mask"].sum(dim=1)
        assert int(n_avail[0]) == 1 and int(n_avail[1]) == s["Z"]
    stats, s64, s32 = D.hier_check_minibatch(zenv_mod, s, level, s["sd"][level], idx, HYPER[level], f"edge-{case}", REPORT)
    if not (level == "hi" and batch == "all"):              # rows as collected: ratio = 1
        adv = D.hier_batch(s, level, idx, F64)["advantage"]
        R.check_rule(f"edge-{case}/{level}.policy_loss_at_ratio_1", stats[3], -float(adv.mean()), s32["policy_loss"], REPORT)
    assert stats[2] == 0.0


def _grad_arena(s, lv):
    from combinatorial_rl_tasks_amd import _native as nat
    tenv = s["tenv"]
    ptr, count = s["env"].hppo_tensor_ptr(lv, nat.PPO_GRAD, -1)
    with torch.cuda.device(tenv.device):
        return tenv._alias_ptr(ptr, (count,)).cpu().numpy().copy()


def test_the_split_reduce_gives_the_same_bytes_twice(zenv_mod):
    """All M rows of the high level twice from the same state: more than 16 chunks of zone rows, so the zone-row
    gradients are added by k_ppo_reduce_split, whose order is fixed."""
    s = _setup(zenv_mod, "bigM")
    env = s["env"]
    idx = np.arange(s["M"], dtype=np.int32)
    assert S.edge_of(s["M"], s["Z"])[3] and s["M"] > S.CHUNK
    D.hier_init(s)
    out = []
    for _ in range(2):
        env.hppo_minibatch(1, idx)
        out.append((env.hppo_stats(1).copy(), _grad_arena(s, 1)))
    assert np.all(np.isfinite(out[0][0])) and np.all(np.isfinite(out[0][1])) and float(np.abs(out[0][1]).max()) > 0
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("level", ["lo", "hi"])
def test_a_smaller_minibatch_reads_nothing_a_larger_one_left(zenv_mod, level):
    """A minibatch of every sample on NaN observations leaves NaN in the workspace's rows; minibatches of
    5 and of 37 samples on the same learner then give the bits a freshly initialised learner gives."""
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "cm64")
    env, tenv, lv, total = s["env"], s["tenv"], LEVELS[level], s["total"][level]
    assert total > 37
    D.hier_init(s)                                          # max_batch = every sample
    with torch.cuda.device(tenv.device):
        obs = tenv._alias(nat.F_EXP_OBS, (T, s["N"], 8), np.float32) if level == "lo" else s["hi_t"]["obs"]
    assert obs.shape == ((T, s["N"], 8) if level == "lo" else (s["M"], 8))
    saved = obs.clone()
    try:
        obs.fill_(float("nan"))
        torch.cuda.synchronize()
        env.hppo_minibatch(lv, np.arange(total, dtype=np.int32))
        assert np.all(np.isnan(env.hppo_stats(lv)[0][[0, 1, 3, 4, 5]])) and np.any(np.isnan(_grad_arena(s, lv)))
    finally:
        obs.copy_(saved)
        torch.cuda.synchronize()
    batches = [D.hier_indexes(s, level, n, 9).astype(np.int32) for n in (5, 37)]
    stale = []
    for idx in batches:
        env.hppo_minibatch(lv, idx)
        stale.append((env.hppo_stats(lv).copy(), _grad_arena(s, lv)))
    for idx, (stats, arena) in zip(batches, stale):
        D.hier_init(s)
        env.hppo_minibatch(lv, idx)
        assert np.all(np.isfinite(stats)) and np.all(np.isfinite(arena)) and float(np.abs(arena).max()) > 0
        np.testing.assert_array_equal(stats, env.hppo_stats(lv))
        np.testing.assert_array_equal(arena, _grad_arena(s, lv))
