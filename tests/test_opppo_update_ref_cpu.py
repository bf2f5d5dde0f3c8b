"""The restatement the Options agent's device learners are tested against (tests/opppo_update_ref.py), checked on the CPU:
the numpy derivatives of the three-component head -- the seven columns k_skppo_lo_loss<3> computes -- against float64
autograd on every loss branch, the entropy's divisor 3 B, the third component's recorded log_prob alone taking the ratio
out of the clip range, float32, and the restated modules against tests/option_ref.py."""
import numpy as np
import pytest
import torch

from tests import option_ref
from tests import opppo_update_ref as R
from tests.test_hppo_update_ref_cpu import _branch_rows, _rel, _returns

F64 = torch.float64
HYPER = dict(clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5)


def _lo_rows(B, seed, d_old=None):
    """Pre-activations, an action drawn from their Normal, the current log_probs [B, 3] and the branch plan."""
    rng = np.random.default_rng(seed)
    pre_mu, pre_std, v = rng.normal(size=(B, 3)), rng.normal(size=(B, 3)), rng.normal(size=B)
    mu, sd = 2.0 * (1 / (1 + np.exp(-pre_mu)) - 0.5), 1 / (1 + np.exp(-pre_std)) + 1e-3
    action = mu + sd * rng.normal(size=(B, 3))
    lp = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(sd)).log_prob(torch.as_tensor(action)).numpy()
    plan, adv, v_off = _branch_rows(B, rng)
    old_v = v + v_off
    return dict(pre_mu=pre_mu, pre_std=pre_std, v=v, mu=mu, sd=sd, action=action, lp=lp, plan=plan, adv=adv, old_v=old_v,
                ret=_returns(v, old_v, rng))


def _autograd(r, old_lp, hyper=HYPER):
    t = {k: torch.as_tensor(r[k], dtype=F64).requires_grad_() for k in ("pre_mu", "pre_std", "v")}
    b = dict(action=torch.as_tensor(r["action"]), log_prob=torch.as_tensor(old_lp.sum(axis=1)),
             value=torch.as_tensor(r["old_v"]), advantage=torch.as_tensor(r["adv"]), returnn=torch.as_tensor(r["ret"]))
    loss, entropy, _, _ = R.lo_head_loss(2.0 * (torch.sigmoid(t["pre_mu"]) - 0.5), torch.sigmoid(t["pre_std"]) + 1e-3,
                                         t["v"], b, hyper)
    loss.backward()
    return t["pre_mu"].grad.numpy(), t["pre_std"].grad.numpy(), t["v"].grad.numpy(), float(entropy.detach())


def _numpy(r, old_lp, hyper=HYPER, dtype=np.float64):
    c = lambda a: np.asarray(a).astype(dtype)                                                         # noqa: E731
    return R.option_head_derivatives(c(r["pre_mu"]), c(r["pre_std"]), c(r["v"]), c(r["action"]), c(old_lp), c(r["old_v"]),
                                     c(r["adv"]), c(r["ret"]), hyper)


def test_seven_head_columns_match_autograd_on_every_branch():
    B = 12
    r = _lo_rows(B, 4)
    old_lp = r["lp"] + r["plan"][:, None] / 3.0              # the offset spread over the three components
    ratio = np.exp((r["lp"] - old_lp).sum(axis=1))
    assert (ratio[:2] > 1.2).all() and (ratio[2:4] < 0.8).all() and (np.abs(ratio[4:] - 1) < 0.2).all()
    g_mu, g_sd, g_v, _ = _autograd(r, old_lp)
    d_mu, d_sd, d_v = _numpy(r, old_lp)
    assert d_mu.shape == (B, 3) and d_sd.shape == (B, 3) and d_v.shape == (B,)
    assert _rel(d_mu, g_mu) < 1e-10 and _rel(d_sd, g_sd) < 1e-10 and _rel(d_v, g_v) < 1e-10
    for col in range(3):                                     # each of the seven columns on its own scale
        assert _rel(d_mu[:, col], g_mu[:, col]) < 1e-10 and _rel(d_sd[:, col], g_sd[:, col]) < 1e-10
    assert np.all(d_mu[0] == 0) and np.all(d_mu[3] == 0) and np.all(d_mu[1] != 0) and np.all(d_mu[2] != 0)
    assert d_v[4] != 0 and d_v[5] == 0


def test_the_entropy_is_a_mean_over_3B():
    B = 12
    r = _lo_rows(B, 5)
    _, _, _, entropy = _autograd(r, r["lp"])
    dist = torch.distributions.Normal(torch.as_tensor(r["mu"]), torch.as_tensor(r["sd"]))
    assert abs(entropy - float(dist.entropy().sum()) / (3 * B)) < 1e-12
    assert abs(entropy - float(dist.entropy().sum()) / (2 * B)) > 1e-3
    # on a clipped row nothing but the entropy's term is left in the std's derivative: -(c / (3 B)) / sd times sigmoid'
    old_lp = r["lp"] + r["plan"][:, None] / 3.0
    _, d_sd, _ = _numpy(r, old_lp)
    _, g_sd, _, _ = _autograd(r, old_lp)
    ssd = r["sd"] - 1e-3
    want = -HYPER["entropy_coef"] / (3 * B) / r["sd"] * ssd * (1 - ssd)
    for row in (0, 3):
        assert _rel(d_sd[row], want[row]) < 1e-12 and _rel(g_sd[row], want[row]) < 1e-10
    assert _rel(d_sd[0], want[0] * 1.5) > 0.1                # and not 1 / (2 B)


@pytest.mark.parametrize("shift,adv_sign", [(-0.5, 1.0), (0.5, -1.0)])
def test_the_third_recorded_log_prob_alone_takes_the_ratio_out_of_the_range(shift, adv_sign):
    """Components 0-1 at ratio 1; the third component's recorded log_prob moved by -0.5 / +0.5 and nothing else: the
    ratio is e^0.5 / e^-0.5, and with the advantage on the clipping side the mu / std derivatives of ALL three
    components are zero but for the entropy's term.  Unmoved, the third component's derivatives are not zero."""
    B = 12
    r = _lo_rows(B, 6)
    r["adv"] = adv_sign * (np.abs(r["adv"]) + 0.1)
    hyper = dict(HYPER, entropy_coef=0.0)
    d_mu0, d_sd0, _ = _numpy(r, r["lp"], hyper)
    assert np.all(d_mu0[:, 2] != 0) and np.all(d_sd0[:, 2] != 0)
    old_lp = r["lp"].copy()
    old_lp[:, 2] += shift
    ratio = np.exp((r["lp"] - old_lp).sum(axis=1))
    np.testing.assert_allclose(ratio, np.exp(-shift), rtol=1e-12)
    assert np.all((ratio > 1.2) if shift < 0 else (ratio < 0.8))
    g_mu, g_sd, _, _ = _autograd(r, old_lp, hyper)
    d_mu, d_sd, _ = _numpy(r, old_lp, hyper)
    assert np.all(g_mu == 0) and np.all(g_sd == 0) and np.all(d_mu == 0) and np.all(d_sd == 0)
    # the advantage on the other side: the unclipped branch wins, and the gradient carries the moved ratio
    r["adv"] = -r["adv"]
    g_mu, g_sd, _, _ = _autograd(r, old_lp, hyper)
    d_mu, d_sd, _ = _numpy(r, old_lp, hyper)
    assert _rel(d_mu, g_mu) < 1e-10 and _rel(d_sd, g_sd) < 1e-10
    assert _rel(d_mu, -d_mu0 * np.exp(-shift)) < 1e-10


def test_head_derivatives_at_float32():
    B = 12
    r = _lo_rows(B, 8)
    old_lp = r["lp"] + r["plan"][:, None] / 3.0
    d64 = _numpy(r, old_lp)
    d32 = _numpy(r, old_lp, dtype=np.float32)
    for a, b in zip(d32, d64):
        assert a.dtype == np.float32 and _rel(a, b) < 2e-5


def test_the_modules_are_the_restated_networks():
    """LoModelRef / HiModelRef at float64 against tests/option_ref.py's functions on the same state_dicts."""
    F, S, h, B, Zn = 6, 5, 16, 9, 4
    hi_sd, lo_sd = option_ref.random_state_dicts(F, S, h=h, seed=2)
    rng = np.random.default_rng(0)
    obs, zone_obs = rng.normal(size=(B, 8)).astype(np.float32), rng.normal(size=(B, Zn, F)).astype(np.float32)
    skill = rng.integers(0, S, B)
    with torch.no_grad():
        mu, std, v = R.model_from("lo", lo_sd, F, F64)(torch.as_tensor(obs, dtype=F64), torch.as_tensor(zone_obs, dtype=F64),
                                                       torch.as_tensor(skill))
        logits, hv = R.model_from("hi", hi_sd, F, F64)(torch.as_tensor(obs, dtype=F64), torch.as_tensor(zone_obs, dtype=F64))
    want = option_ref.low(lo_sd, obs, zone_obs, skill, S, F64)
    assert mu.shape == (B, 3) and std.shape == (B, 3)
    for got, ref in zip((mu, std, v), want):
        np.testing.assert_allclose(got.numpy(), np.asarray(ref), rtol=1e-12, atol=1e-13)
    want_hi = option_ref.high(hi_sd, obs, zone_obs, F64)
    np.testing.assert_allclose(torch.log_softmax(logits, dim=1).numpy(), np.asarray(want_hi[0]), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(hv.numpy(), np.asarray(want_hi[1]), rtol=1e-12, atol=1e-13)
    assert R.sizes(lo_sd, "lo") == (h, S) and R.sizes(hi_sd, "hi") == (h, S)
    assert list(dict(R.model_from("lo", lo_sd, F, F64).named_parameters())) == list(lo_sd)


def test_lo_batch_takes_either_layout_and_skips_frame_T_minus_1():
    N, T = 3, 5
    rng = np.random.default_rng(1)
    lo = dict(obs=rng.normal(size=(N, T - 1, 8)), zone_obs=rng.normal(size=(N, T - 1, 2, 6)),
              action=rng.normal(size=(N, T - 1, 3)), log_prob=rng.normal(size=(N, T - 1, 3)),
              value=rng.normal(size=(N, T - 1)), advantage=rng.normal(size=(N, T - 1)), returnn=rng.normal(size=(N, T - 1)),
              skill=rng.integers(0, 4, (N, T - 1)))
    apart = dict(lo, action=lo["action"][..., :2], log_prob=lo["log_prob"][..., :2], term_action=lo["action"][..., 2],
                 term_log_prob=lo["log_prob"][..., 2])
    idx = np.array([0, 5, N * (T - 1) - 1])
    a, b = R.lo_batch(lo, idx, F64), R.lo_batch(apart, idx, F64)
    for k in a:
        assert torch.equal(a[k], b[k])
    env, frame = R.lo_index(idx, T)
    assert list(env) == [0, 1, 2] and list(frame) == [0, 1, T - 2]
    assert torch.equal(a["action"][1], torch.as_tensor(lo["action"][1, 1]))
