"""tests/xy_ref.py against an independent assembly: the xy-goals high level built from torch.nn modules that load the
state_dict by its keys, and the goal draw's Philox stream against the other streams.  No device."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import philox_ref, xy_ref


class _EnvModel(nn.Module):
    """ZoneEnvModel: zone_net_ on [obs, zone row], the mean over the zones, combine_net_ on [obs, zone_emb]."""

    def __init__(self, F, h):
        super().__init__()
        self.zone_net_ = nn.Sequential(nn.Linear(8 + F, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h))
        self.combine_net_ = nn.Linear(8 + h, h)

    def forward(self, obs, zone_obs):
        n_zones = zone_obs.shape[1]
        rows = torch.cat([obs.unsqueeze(1).repeat(1, n_zones, 1), zone_obs], dim=2)
        return self.combine_net_(torch.cat([obs, self.zone_net_(rows).mean(dim=1)], dim=1))


class _Actor(nn.Module):
    """PolicyNetwork on a Box(-1, 1, (2,)) with hiddens=[h]."""

    def __init__(self, h):
        super().__init__()
        self.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h, h), nn.ReLU()))
        self.mu_ = nn.Linear(h, 2)
        self.std_ = nn.Linear(h, 2)

    def forward(self, emb):
        x = self.enc_(emb)
        return 2 * (torch.sigmoid(self.mu_(x)) - 0.5), torch.sigmoid(self.std_(x)) + 1e-3


class _High(nn.Module):
    def __init__(self, F, h, critic):
        super().__init__()
        self.env_model = _EnvModel(F, h)
        self.actor = _Actor(h)
        if critic:
            self.critic = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))

    def forward(self, obs, zone_obs):
        emb = self.env_model(obs, zone_obs)
        mu, std = self.actor(emb)
        return mu, std, self.critic(emb).squeeze(1) if hasattr(self, "critic") else torch.zeros(len(obs))


@pytest.mark.parametrize("F,h,Z,critics", [(6, 16, 1, True), (7, 128, 25, True), (6, 191, 15, False)])
def test_high_matches_the_modules(F, h, Z, critics):
    hi, lo = xy_ref.random_state_dicts(F, h, 3 + h, critics)
    net = _High(F, h, critics)
    assert sorted(net.state_dict()) == sorted(hi)               # the checkpoint's keys, no more and no fewer
    net.load_state_dict(hi)
    rs = np.random.RandomState(h)
    obs = rs.uniform(-1, 1, (37, 8)).astype(np.float32)
    zo = rs.uniform(-1, 1, (37, Z, F)).astype(np.float32)
    with torch.no_grad():
        want = net(torch.as_tensor(obs), torch.as_tensor(zo))
    got = xy_ref.high(hi, obs, zo)
    for g, w in zip(got, want):
        w = w.numpy()
        assert g.shape == w.shape and g.dtype == np.float32
        assert np.all(np.abs(g - w) <= 1e-6 * np.maximum(1.0, np.abs(w))), float(np.abs(g - w).max())
    assert (np.abs(got[0]) < 1).all() and (got[1] > 1e-3).all() and (got[1] < 1.001).all()
    assert got[2].any() == critics
    # the low level's keys are the Zone-goals low level's: hier_ref.low takes them
    mu, std, v = xy_ref.low(lo, obs, zo, rs.uniform(-2, 2, (37, 2)).astype(np.float32))
    assert mu.shape == std.shape == (37, 2) and v.shape == (37,) and v.any() == critics


def test_the_goal_stream_is_its_own_and_keyed_by_the_global_env():
    n, seed, step = 64, 0xDEADBEEF12345, 17
    g = xy_ref.goal_noise(n, seed, 0, step)
    assert g.shape == (n, 2) and g.dtype == np.float64 and np.isfinite(g).all()
    assert not np.array_equal(g, philox_ref.action_noise(n, seed, 0, step))
    words = philox_ref._draw(n, seed, 0, step, xy_ref.TAG_XY_GOAL)
    for tag in (philox_ref.TAG_ACTION, philox_ref.TAG_GOAL, philox_ref.TAG_SKILL):
        assert tag != xy_ref.TAG_XY_GOAL
        other = philox_ref._draw(n, seed, 0, step, tag)
        assert not any(np.array_equal(a, b) for a, b in zip(words, other))
    # global env index: env i at offset 5 draws what env i + 5 draws at offset 0, also beyond 2^32
    assert np.array_equal(xy_ref.goal_noise(n - 5, seed, 5, step), g[5:])
    big = xy_ref.goal_noise(n, seed, 2 ** 40, step)
    assert np.array_equal(xy_ref.goal_noise(n - 1, seed, 2 ** 40 + 1, step), big[1:])
    assert not np.array_equal(big, g)
    # another seed or step: other draws
    assert not np.array_equal(xy_ref.goal_noise(n, seed + 1, 0, step), g)
    assert not np.array_equal(xy_ref.goal_noise(n, seed, 0, step + 1), g)
    # the arithmetic is action_noise's: the same words give the same pair
    u1 = philox_ref.uniform(words[0]).astype(np.float64)
    ang = (np.float32(6.283185307179586) * philox_ref.uniform(words[1])).astype(np.float64)
    assert np.array_equal(g[:, 0], np.sqrt(-2.0 * np.log(u1)) * np.cos(ang))
