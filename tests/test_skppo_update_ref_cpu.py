"""The restatement the fixed-length-skills device learners are tested against (tests/skppo_update_ref.py), checked on the
CPU: the numpy derivatives of both heads -- the per-row formulas k_ppo_loss and k_skppo_hi_loss compute -- against float64
autograd on every loss branch (unclipped, clipped above, clipped below, value clipped), with one skill (every derivative
exactly 0), with a recorded skill of probability 1e-6, at float32, and the restated modules against tests/skill_ref.py."""
import numpy as np
import pytest
import torch

from tests import skill_ref
from tests import skppo_update_ref as R
from tests.test_hppo_update_ref_cpu import _branch_rows, _rel, _returns

F64 = torch.float64
HYPER = dict(clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5)


def _hi_rows(B, S, seed, rare=False):
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(B, S)) * 1.5
    v = rng.normal(size=B)
    action = rng.integers(0, S, B)
    if rare:                                                # row 6: the recorded skill has probability about 1e-6
        logits[6] = rng.normal(size=S) * 0.1
        logits[6, action[6]] -= np.log(1e6 / (S - 1))
    lp = torch.log_softmax(torch.as_tensor(logits), dim=1).numpy()[np.arange(B), action]
    d_old, adv, v_off = _branch_rows(B, rng)
    old_v = v + v_off
    return logits, v, action, lp, lp + d_old, old_v, adv, _returns(v, old_v, rng)


def _hi_autograd(logits, v, action, old_lp, old_v, adv, ret):
    t = {k: torch.as_tensor(a, dtype=F64).requires_grad_() for k, a in dict(lg=logits, v=v).items()}
    b = dict(action=torch.as_tensor(action), log_prob=torch.as_tensor(old_lp), value=torch.as_tensor(old_v),
             advantage=torch.as_tensor(adv), returnn=torch.as_tensor(ret))
    loss, entropy, _, _ = R.hi_head_loss(t["lg"], t["v"], b, HYPER)
    loss.backward()
    return t["lg"].grad.numpy(), t["v"].grad.numpy(), float(entropy.detach())


@pytest.mark.parametrize("S", [2, 5, 32])
def test_skill_head_derivatives_match_autograd_on_every_branch(S):
    B = 12
    logits, v, action, lp, old_lp, old_v, adv, ret = _hi_rows(B, S, 3 + S, rare=S > 2)
    ratio = np.exp(lp - old_lp)
    # every branch is there: rows 0-1 above the range, 2-3 below it, 4-5 with the value a whole 1 away, the rest inside
    assert (ratio[:2] > 1.2).all() and (ratio[2:4] < 0.8).all() and (np.abs(ratio[4:] - 1) < 0.2).all()
    assert (np.abs(v - old_v)[4:6] > 0.2).all()
    if S > 2:
        assert 0.5e-6 < np.exp(lp[6]) < 2e-6
    g_lg, g_v, entropy = _hi_autograd(logits, v, action, old_lp, old_v, adv, ret)
    d, d_v, ent = R.skill_head_derivatives(logits, action, old_lp, v, old_v, adv, ret, HYPER)
    assert _rel(d, g_lg) < 1e-10 and _rel(d_v, g_v) < 1e-10 and abs(ent - entropy) < 1e-12
    if S > 2:
        assert _rel(d[6], g_lg[6]) < 1e-9                   # the rare skill's row on its own scale
    # clipped with the advantage on the clipping side (rows 0 and 3): only the entropy's part is left
    m = logits.max(axis=1, keepdims=True)
    lps = logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))
    p = np.exp(lps)
    H = -(p * lps).sum(axis=1)
    for row in (0, 3):
        assert _rel(d[row], HYPER["entropy_coef"] / B * p[row] * (lps[row] + H[row])) < 1e-12
    for row in (1, 2):
        assert abs(d[row, action[row]]) > 1e-3
    assert d_v[4] != 0 and d_v[5] == 0 and g_v[5] == 0      # the value clip taken: no gradient
    # a row's derivatives sum to zero: a shift common to its logits changes nothing
    assert np.abs(d.sum(axis=1)).max() < 1e-15


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_skill_gives_exactly_zero(dtype):
    """S = 1: the one probability is 1, log p = 0 and H = 0 -- float64 autograd gives exactly 0 for every logit, and so
    do the stated formulas at either precision."""
    B = 12
    logits, v, action, lp, old_lp, old_v, adv, ret = _hi_rows(B, 1, 9)
    assert np.all(action == 0) and np.all(lp == 0)
    g_lg, g_v, entropy = _hi_autograd(logits, v, action, old_lp, old_v, adv, ret)
    assert np.all(g_lg == 0) and entropy == 0
    cast = [a.astype(dtype) for a in (logits, old_lp, v, old_v, adv, ret)]
    d, d_v, ent = R.skill_head_derivatives(cast[0], action, cast[1], cast[2], cast[3], cast[4], cast[5], HYPER)
    assert d.dtype == dtype and np.all(d == 0) and ent == 0
    assert _rel(d_v, g_v) < (1e-10 if dtype == np.float64 else 1e-5)


def test_skill_head_derivatives_at_float32():
    B, S = 12, 5
    logits, v, action, lp, old_lp, old_v, adv, ret = _hi_rows(B, S, 8, rare=True)
    d64, dv64, e64 = R.skill_head_derivatives(logits, action, old_lp, v, old_v, adv, ret, HYPER)
    cast = [a.astype(np.float32) for a in (logits, old_lp, v, old_v, adv, ret)]
    d32, dv32, e32 = R.skill_head_derivatives(cast[0], action, cast[1], cast[2], cast[3], cast[4], cast[5], HYPER)
    assert d32.dtype == np.float32 and _rel(d32, d64) < 1e-5 and _rel(dv32, dv64) < 1e-5 and abs(e32 - e64) < 1e-5


def test_low_level_head_derivatives_match_autograd():
    """The low level's loss is the flat one: a recorded log_prob per component, the entropy's mean over B x 2."""
    B = 12
    rng = np.random.default_rng(4)
    pre_mu, pre_std, v = rng.normal(size=(B, 2)), rng.normal(size=(B, 2)), rng.normal(size=B)
    mu, sd = 2.0 * (1 / (1 + np.exp(-pre_mu)) - 0.5), 1 / (1 + np.exp(-pre_std)) + 1e-3
    action = mu + sd * rng.normal(size=(B, 2))
    lp = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(sd)).log_prob(torch.as_tensor(action)).numpy()
    d_old, adv, v_off = _branch_rows(B, rng)
    old_lp = lp + d_old[:, None] / 2.0                      # per component
    old_v = v + v_off
    ret = _returns(v, old_v, rng)
    ratio = np.exp((lp - old_lp).sum(axis=1))
    assert (ratio[:2] > 1.2).all() and (ratio[2:4] < 0.8).all() and (np.abs(ratio[4:] - 1) < 0.2).all()
    t = {k: torch.as_tensor(a, dtype=F64).requires_grad_() for k, a in dict(pm=pre_mu, ps=pre_std, v=v).items()}
    b = dict(action=torch.as_tensor(action), log_prob=torch.as_tensor(old_lp.sum(axis=1)), value=torch.as_tensor(old_v),
             advantage=torch.as_tensor(adv), returnn=torch.as_tensor(ret))
    loss, entropy, _, _ = R.lo_head_loss(2.0 * (torch.sigmoid(t["pm"]) - 0.5), torch.sigmoid(t["ps"]) + 1e-3, t["v"], b,
                                         HYPER)
    loss.backward()
    d_mu, d_sd, d_v = R.gaussian_head_derivatives(pre_mu, pre_std, v, action, old_lp, old_v, adv, ret, HYPER)
    assert _rel(d_mu, t["pm"].grad.numpy()) < 1e-10 and _rel(d_sd, t["ps"].grad.numpy()) < 1e-10
    assert _rel(d_v, t["v"].grad.numpy()) < 1e-10
    assert np.all(d_mu[0] == 0) and np.all(d_mu[3] == 0) and np.all(d_mu[1] != 0) and np.all(d_mu[2] != 0)
    assert d_v[4] != 0 and d_v[5] == 0
    dist = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(sd))
    assert abs(float(entropy.detach()) - float(dist.entropy().sum() / (2 * B))) < 1e-12


@pytest.mark.parametrize("S", [1, 5, 32])
def test_restated_modules_are_skill_ref_networks(S):
    """The modules the gradients come from compute what tests/skill_ref.py computes, and their parameters() order is the
    arenas' order."""
    from combinatorial_rl_tasks_amd import agents
    F, h, B, Zn = 6, 9, 7, 4
    hi_sd, lo_sd = skill_ref.random_state_dicts(F, S, h=h, seed=3)
    rng = np.random.default_rng(2)
    obs, zo = rng.normal(size=(B, 8)).astype(np.float32), rng.uniform(-1, 1, (B, Zn, F)).astype(np.float32)
    skill = rng.integers(0, S, B)
    hi, lo = R.model_from("hi", hi_sd, F, F64), R.model_from("lo", lo_sd, F, F64)
    assert R.sizes(hi_sd, "hi") == (h, S) == R.sizes(lo_sd, "lo")
    with torch.no_grad():
        logits, hv = hi(torch.as_tensor(obs, dtype=F64), torch.as_tensor(zo, dtype=F64))
        mu, std, lv = lo(torch.as_tensor(obs, dtype=F64), torch.as_tensor(zo, dtype=F64), torch.as_tensor(skill))
    want_hi, want_lo = skill_ref.high(hi_sd, obs, zo, F64), skill_ref.low(lo_sd, obs, zo, skill, S, F64)
    np.testing.assert_allclose(torch.log_softmax(logits, dim=1).numpy(), want_hi[0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(hv.numpy(), want_hi[1], rtol=0, atol=1e-13)
    for got, want in zip((mu, std, lv), want_lo):
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-13)
    hi_keys, lo_keys = agents.skppo_state_dict_keys()
    assert list(hi_keys.values()) == [k for k, _ in hi.named_parameters()] and len(hi_keys) == 16
    assert list(lo_keys.values()) == [k for k, _ in lo.named_parameters()] and len(lo_keys) == 18


def test_gradients_of_both_levels_and_the_index_map():
    F, S, h, N, T, Zn = 6, 3, 8, 2, 3, 4
    hi_sd, lo_sd = skill_ref.random_state_dicts(F, S, h=h, seed=5)
    g = torch.Generator().manual_seed(4)
    n = N * T
    lo = dict(obs=torch.randn((n, 8), generator=g), zone_obs=torch.rand((n, Zn, F), generator=g),
              action=torch.randn((n, 2), generator=g), log_prob=torch.randn((n, 2), generator=g) * 0.1 - 1.0,
              value=torch.randn((n,), generator=g), advantage=torch.randn((n,), generator=g),
              returnn=torch.randn((n,), generator=g))
    lo = {k: v.numpy().reshape((N, T) + tuple(v.shape[1:])) for k, v in lo.items()}
    lo["skill"] = (np.arange(n, dtype=np.int32) % S).reshape(N, T)
    lo["value"] = (np.arange(n, dtype=np.float32) * 10).reshape(N, T)          # value = 10 (env T + frame)
    b = R.lo_batch(lo, np.arange(n), F64)
    env, frame = R.lo_index(np.arange(n), T)
    np.testing.assert_array_equal(b["value"].numpy(), 10.0 * (env * T + frame))
    assert set(frame.tolist()) == set(range(T)) and b["skill"].dtype == torch.int64
    grads, stats = R.gradients("lo", R.model_from("lo", lo_sd, F, F64), b, R.LO_HYPER)
    assert len(grads) == 18 and all(float(x.abs().max()) > 0 for x in grads.values())
    hi = dict(obs=lo["obs"].reshape(n, 8), zone_obs=lo["zone_obs"].reshape(n, Zn, F), action=lo["skill"].reshape(n),
              value=lo["value"].reshape(n) / 50, log_prob=np.full(n, -1.0, np.float32),
              advantage=lo["advantage"].reshape(n), returnn=lo["returnn"].reshape(n))
    grads, stats = R.gradients("hi", R.model_from("hi", hi_sd, F, F64), R.hi_batch(hi, np.arange(n), F64), R.HI_HYPER)
    assert len(grads) == 16 and all(float(x.abs().max()) > 0 for x in grads.values())
    assert stats["value_std"] == 0.0 and 0 < stats["entropy"] <= np.log(S) + 1e-12
