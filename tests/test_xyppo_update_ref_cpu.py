"""The restatement the xy-goals device learners are tested against (tests/xyppo_update_ref.py), checked on the CPU: the
numpy derivatives of the high level's head -- the per-row formulas k_xyppo_hi_loss computes -- against float64 autograd
on every loss branch, the entropy statistic, and the low level's flat index order."""
import numpy as np
import torch

from tests import xy_ref
from tests import xyppo_update_ref as R
from tests.test_hppo_update_ref_cpu import _branch_rows, _rel, _returns

F64 = torch.float64
HYPER = dict(clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5)


def _rows(B, seed):
    rng = np.random.default_rng(seed)
    pre_mu, pre_std = rng.normal(size=(B, 2)), rng.normal(size=(B, 2))
    v = rng.normal(size=B)
    mu, sd = 2.0 * (1 / (1 + np.exp(-pre_mu)) - 0.5), 1 / (1 + np.exp(-pre_std)) + 1e-3
    goal = mu + sd * rng.normal(size=(B, 2))
    lp = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(sd)).log_prob(torch.as_tensor(goal)).numpy()
    d_old, adv, v_off = _branch_rows(B, rng)
    old_lp = lp.sum(axis=1) + d_old                         # ONE recorded log_prob per row
    old_v = v + v_off
    ret = _returns(v, old_v, rng)
    return pre_mu, pre_std, v, goal, lp, old_lp, old_v, adv, ret


def test_joint_gaussian_head_derivatives_match_autograd():
    B = 12
    pre_mu, pre_std, v, goal, lp, old_lp, old_v, adv, ret = _rows(B, 3)
    t = {k: torch.as_tensor(a, dtype=F64).requires_grad_() for k, a in dict(pm=pre_mu, ps=pre_std, v=v).items()}
    b = dict(goal=torch.as_tensor(goal), log_prob=torch.as_tensor(old_lp), value=torch.as_tensor(old_v),
             advantage=torch.as_tensor(adv), returnn=torch.as_tensor(ret))
    loss, entropy, _, _ = R.hi_head_loss(2.0 * (torch.sigmoid(t["pm"]) - 0.5), torch.sigmoid(t["ps"]) + 1e-3, t["v"], b,
                                         HYPER)
    loss.backward()
    # every branch is there: rows 0-1 above the range, 2-3 below it, 4-5 with the value a whole 1 away
    ratio = np.exp(lp.sum(axis=1) - old_lp)
    assert (ratio[:2] > 1.2).all() and (ratio[2:4] < 0.8).all() and (np.abs(ratio[4:] - 1) < 0.2).all()
    assert (np.abs(v - old_v)[4:6] > 0.2).all()
    d_mu, d_sd, d_v, ent = R.joint_gaussian_head_derivatives(pre_mu, pre_std, v, goal, old_lp, old_v, adv, ret, HYPER)
    assert _rel(d_mu, t["pm"].grad.numpy()) < 1e-10
    assert _rel(d_sd, t["ps"].grad.numpy()) < 1e-10
    assert _rel(d_v, t["v"].grad.numpy()) < 1e-10
    assert abs(ent - float(entropy.detach())) < 1e-12
    # clipped with the advantage on the clipping side (rows 0 and 3): no policy gradient, only the entropy's on std
    assert np.all(d_mu[0] == 0) and np.all(d_mu[3] == 0) and np.all(d_mu[1] != 0) and np.all(d_mu[2] != 0)
    sd = 1 / (1 + np.exp(-pre_std)) + 1e-3
    ssd = sd - 1e-3
    want = -HYPER["entropy_coef"] / (B * sd[0]) * ssd[0] * (1 - ssd[0])
    assert _rel(d_sd[0], want) < 1e-12
    assert d_v[4] != 0 and d_v[5] == 0 and t["v"].grad[5] == 0          # the value clip taken: no gradient


def test_the_flat_head_is_not_the_high_level_head():
    """The flat learner's loss on the same rows -- recorded log_prob split evenly over the two dimensions, so that the
    ratio is the same -- has half the entropy and half the entropy's derivative: what reusing k_ppo_loss would give."""
    from tests import hppo_update_ref as RH
    B = 12
    pre_mu, pre_std, v, goal, lp, old_lp, old_v, adv, ret = _rows(B, 5)
    d_mu, d_sd, d_v, ent = R.joint_gaussian_head_derivatives(pre_mu, pre_std, v, goal, old_lp, old_v, adv, ret, HYPER)
    split = np.repeat(old_lp[:, None] / 2.0, 2, axis=1)
    f_mu, f_sd, f_v = RH.gaussian_head_derivatives(pre_mu, pre_std, v, goal, split, old_v, adv, ret, HYPER)
    assert _rel(f_mu, d_mu) < 1e-10 and _rel(f_v, d_v) < 1e-12
    sd = 1 / (1 + np.exp(-pre_std)) + 1e-3
    ssd = sd - 1e-3
    half = 0.5 * HYPER["entropy_coef"] / (B * sd) * ssd * (1 - ssd)
    assert _rel(f_sd - half, d_sd) < 1e-10 and _rel(f_sd, d_sd) > 1e-4


def test_entropy_statistic_is_sum_then_mean():
    std = torch.rand((7, 2), dtype=F64, generator=torch.Generator().manual_seed(1)) + 0.05
    dist = torch.distributions.Normal(torch.zeros_like(std), std)
    want = dist.entropy().sum(-1).mean()
    assert abs(float(R.hi_entropy(std)) - float(want)) < 1e-14
    assert abs(float(want) - 2.0 * float(dist.entropy().mean())) < 1e-12
    # and through the restated loss of a model
    hi_sd, _ = xy_ref.random_state_dicts(6, h=8, seed=2)
    g = torch.Generator().manual_seed(4)
    b = dict(obs=torch.randn((5, 8), generator=g, dtype=F64), zone_obs=torch.rand((5, 3, 6), generator=g, dtype=F64),
             goal=torch.randn((5, 2), generator=g, dtype=F64), log_prob=torch.randn((5,), generator=g, dtype=F64),
             value=torch.randn((5,), generator=g, dtype=F64), advantage=torch.randn((5,), generator=g, dtype=F64),
             returnn=torch.randn((5,), generator=g, dtype=F64))
    model = R.model_from("hi", hi_sd, 6, F64)
    _, stats = R.loss_and_stats("hi", model, b, R.HI_HYPER)
    mu, std, v = model(b["obs"], b["zone_obs"])
    assert abs(stats["entropy"] - float(torch.distributions.Normal(mu, std).entropy().sum(-1).mean().detach())) < 1e-14
    grads, stats = R.gradients("hi", model, b, R.HI_HYPER)
    assert len(grads) == 18 and all(float(x.abs().max()) > 0 for x in grads.values())


def test_low_level_index_map_is_the_transposed_flattening():
    """The reference stores [T][N] and flattens transpose(0, 1).reshape(-1): flat index i is env i // T, frame i % T,
    and every frame is there, the last one included."""
    T, N = 3, 2
    tm = np.arange(T * N).reshape(T, N) * 10                # time-major: value = 10 (t N + n)
    flat = torch.as_tensor(tm).transpose(0, 1).reshape(-1).numpy()
    env, frame = R.lo_index(np.arange(N * T), T)
    np.testing.assert_array_equal(flat, tm[frame, env])
    np.testing.assert_array_equal(env, [0, 0, 0, 1, 1, 1])
    np.testing.assert_array_equal(frame, [0, 1, 2, 0, 1, 2])
    assert set(frame.tolist()) == set(range(T))             # frame T-1 is among them
    # lo_batch on the [N, T, ...] views the collectors hand out picks the same elements
    lo = {k: np.ascontiguousarray(tm.T).astype(np.float32).reshape((N, T) + s) * np.ones((N, T) + s, np.float32)
          for k, s in (("obs", (1,)), ("zone_obs", (1, 1)), ("goal", (1,)), ("action", (1,)), ("log_prob", (1,)),
                       ("value", ()), ("advantage", ()), ("returnn", ()))}
    b = R.lo_batch(lo, np.arange(N * T), F64)
    np.testing.assert_array_equal(b["value"].numpy(), flat)
