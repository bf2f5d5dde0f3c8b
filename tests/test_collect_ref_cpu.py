"""The float64 restatements of tests/collect_ref.py without a device: the GAE against hand-computed short rollouts and
against the float32 recursion of test_collect_experiences, the log_prob against torch.distributions.Normal, the float32
action draw against the float64 one, and the float64 variants of the network restatements against their float32
defaults."""
import numpy as np
import pytest
import torch

from tests import collect_ref


@pytest.mark.parametrize("case", [
    # T = 1: only the bootstrap; cur_mask 0 cuts it
    dict(r=[[1.0]], v=[[0.5]], m=[[1.0]], cur=[1.0], nv=[2.0], g=0.9, lam=0.8, adv=[[2.3]]),
    dict(r=[[1.0]], v=[[0.5]], m=[[0.0]], cur=[0.0], nv=[2.0], g=0.9, lam=0.8, adv=[[0.5]]),
    # T = 2: frame 0 ended its episode (mask[1] = 0), then the same without the end
    dict(r=[[1.0], [2.0]], v=[[0.5], [1.5]], m=[[1.0], [0.0]], cur=[1.0], nv=[3.0], g=0.9, lam=0.8, adv=[[0.5], [3.2]]),
    dict(r=[[1.0], [2.0]], v=[[0.5], [1.5]], m=[[1.0], [1.0]], cur=[1.0], nv=[3.0], g=0.9, lam=0.8,
         adv=[[1.85 + 0.72 * 3.2], [3.2]]),
    # T = 3, discount = lambda = 1: the advantage is the sum of the rewards to the end minus the value; mask[0] unused
    dict(r=[[0.0], [0.0], [1.0]], v=[[0.2], [0.4], [0.6]], m=[[0.0], [1.0], [1.0]], cur=[0.0], nv=[10.0], g=1.0,
         lam=1.0, adv=[[0.8], [0.6], [0.4]]),
    # discount 0: r - v; lambda 0: the one-step TD error
    dict(r=[[0.0], [0.0], [1.0]], v=[[0.2], [0.4], [0.6]], m=[[1.0], [1.0], [1.0]], cur=[1.0], nv=[10.0], g=0.0,
         lam=0.95, adv=[[-0.2], [-0.4], [0.4]]),
    dict(r=[[0.0], [0.0], [1.0]], v=[[0.2], [0.4], [0.6]], m=[[1.0], [1.0], [0.0]], cur=[1.0], nv=[10.0], g=1.0,
         lam=0.0, adv=[[0.2], [-0.4], [10.4]]),
])
def test_gae_by_hand(case):
    adv, ret, mag = collect_ref.gae(case["r"], case["v"], case["m"], case["cur"], case["nv"], case["g"], case["lam"])
    assert np.allclose(adv, case["adv"], rtol=0, atol=1e-12), adv
    assert np.allclose(ret, np.asarray(case["v"]) + np.asarray(case["adv"]), rtol=0, atol=1e-12)
    assert (mag >= np.abs(adv) - 1e-12).all()


def _f32_recursion(reward, value, mask, cur_mask, next_value, discount, gae_lambda):
    """The float32 loop of test_collect_experiences (tests/test_gpu_mlp.py), on time-major records."""
    f = np.float32
    nv, nm, na = np.asarray(next_value, f), np.asarray(cur_mask, f), np.zeros(reward.shape[1], f)
    adv = np.zeros(reward.shape, f)
    for k in reversed(range(reward.shape[0])):
        delta = reward[k] + f(discount) * nv * nm - value[k]
        adv[k] = delta + f(discount) * f(gae_lambda) * na * nm
        nv, nm, na = value[k], mask[k], adv[k]
    return adv


@pytest.mark.parametrize("g,lam", [(0.99, 0.95), (1.0, 1.0), (1.0, 0.0), (0.0, 0.95)])
def test_gae_against_the_float32_recursion(g, lam):
    rs = np.random.RandomState(3)
    T, N = 64, 300
    reward = np.where(rs.rand(T, N) < 0.2, rs.randn(T, N), 0).astype(np.float32)
    value = rs.randn(T, N).astype(np.float32)
    mask = (rs.rand(T, N) > 0.05).astype(np.float32)
    cur, nv = (rs.rand(N) > 0.05).astype(np.float32), rs.randn(N).astype(np.float32)
    g32, lam32 = float(np.float32(g)), float(np.float32(lam))
    adv64, ret64, mag = collect_ref.gae(reward, value, mask, cur, nv, g32, lam32)
    adv32 = _f32_recursion(reward, value, mask, cur, nv, g, lam)
    err = np.abs(adv32 - adv64) / (mag * 2.0 ** -24)
    assert err.max() <= 8, err.max()                     # the bound test_gpu_collect_paths holds the device to
    assert np.abs(adv64).max() > 1 and (mask == 0).any()
    assert np.array_equal(ret64, value.astype(np.float64) + adv64)


def test_log_prob_against_torch_normal():
    rs = np.random.RandomState(5)
    mu = rs.uniform(-1, 1, (500, 2))
    std = rs.uniform(1e-3, 1.001, (500, 2))
    a = mu + std * rs.randn(500, 2) * 3
    lp, mag = collect_ref.normal_log_prob(a, mu, std)
    want = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(std)).log_prob(torch.as_tensor(a)).numpy()
    assert lp.dtype == np.float64 and np.abs(lp - want).max() <= 1e-12 * np.abs(want).max()
    assert (mag >= np.abs(lp) - 1e-12).all()


def test_action_draw_float32_against_float64():
    rs = np.random.RandomState(7)
    n = 4000
    mu = rs.uniform(-1, 1, (n, 2)).astype(np.float32)
    std = rs.uniform(1e-3, 1.001, (n, 2)).astype(np.float32)
    for seed, index0, step in ((1, 0, 0), (0xABCDEF0123, 4242, 77), (3, 2 ** 40, 2 ** 32 - 1)):
        a = collect_ref.action_draw(mu, std, seed, index0, step)
        assert a.dtype == np.float32
        assert collect_ref.action_draw_ulps(a, mu, std, seed, index0, step).max() <= 4
        other = collect_ref.action_draw(mu, std, seed, index0 + 1, step)     # env_index0 shifts the stream
        assert collect_ref.action_draw_ulps(other, mu, std, seed, index0, step).max() > 1e3


def test_float64_network_restatements():
    """forward_fp32 / inverse_log_softmax with dtype=float64 agree with their float32 defaults to float32 rounding, and
    the defaults still return float32."""
    from oracle import policy_ref as P
    from tests.skill_collect_ref import inverse_log_softmax, random_inverse_state_dict
    rs = np.random.RandomState(2)
    obs = rs.uniform(-1, 1, (40, 8)).astype(np.float32)
    zo = rs.uniform(-1, 1, (40, 5, 6)).astype(np.float32)
    t = P.random_tensors(6, h=33, seed=1, distributional=True)
    r32, r64 = P.forward_fp32(t, obs, zo), P.forward_fp32(t, obs, zo, dtype=torch.float64)
    for a, b in zip(r32, r64):
        assert a.dtype == np.float32 and b.dtype == np.float64 and np.abs(a - b).max() < 1e-5
    sd = random_inverse_state_dict(6, 4, h=33, seed=2)
    l32, l64 = inverse_log_softmax(sd, obs, zo), inverse_log_softmax(sd, obs, zo, dtype=torch.float64)
    assert l32.dtype == np.float32 and l64.dtype == np.float64 and np.abs(l32 - l64).max() < 1e-5
