"""TEST INFRASTRUCTURE -- float32 torch restatement of the xy-goals agent's high level and its goal draw (checker only).

Restated from their description, op for op:
* ``HighPolicyValueModel``  xy-goals/src/hier_policy_value_models.py:19-43: emb = ZoneEnvModel(obs, zone_obs);
  x = relu(actor.enc_.0.0(emb)); goal_mu = 2 (sigmoid(actor.mu_(x)) - 0.5), goal_std = sigmoid(actor.std_(x)) + 1e-3;
  value = critic.2(relu(critic.0(emb)))
* ``LoPolicyValueModel``    :45-72 is the Zone-goals low level on [obs, goal, zone row]: ``hier_ref.low`` as it stands,
  the goal being the high level's sample instead of a zone centre / 3
* the goal draw: Philox stream 0x585947, the Box-Muller pair of the action draw (``philox_ref.action_noise``)
"""
import numpy as np
import torch

from tests import hier_ref, philox_ref

TAG_XY_GOAL = 0x585947


def random_state_dicts(F, h=128, seed=0, critics=True, bias_scale=0.1, weight_scale=1.0):
    """(hi_state_dict, lo_state_dict) with the reference's key names, float32 torch tensors: rows of N(0, 1) normalised
    to unit norm, biases of scale 0.1 (so that the bias path is exercised).  weight_scale multiplies every weight row,
    as in hier_ref.random_state_dicts: larger activations, for the precision sweeps."""
    g = torch.Generator().manual_seed(seed)

    def lin(n_out, n_in):
        return hier_ref._lin(g, n_out, n_in, bias_scale, weight_scale)

    hi, lo = {}, {}
    for sd, x in ((hi, 8), (lo, 10)):
        for name, n_in in (("zone_net_.0", x + F), ("zone_net_.2", h), ("zone_net_.4", h)):
            sd[f"env_model.{name}.weight"], sd[f"env_model.{name}.bias"] = lin(h, n_in)
        sd["env_model.combine_net_.weight"], sd["env_model.combine_net_.bias"] = lin(h, x + h)
        sd["actor.enc_.0.0.weight"], sd["actor.enc_.0.0.bias"] = lin(h, h)
        sd["actor.mu_.weight"], sd["actor.mu_.bias"] = lin(2, h)
        sd["actor.std_.weight"], sd["actor.std_.bias"] = lin(2, h)
        if critics:
            sd["critic.0.weight"], sd["critic.0.bias"] = lin(h, h)
            sd["critic.2.weight"], sd["critic.2.bias"] = lin(1, h)
    return hi, lo


def high(hi_sd, obs, zone_obs, dtype=torch.float32):
    """-> goal_mu [B,2], goal_std [B,2], value [B]; numpy arrays of `dtype` (float32: the reference's modules; float64:
    the same operations on the same float32 inputs)."""
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in hi_sd.items()}
    obs = torch.as_tensor(np.asarray(obs, np.float32)).to(dtype)
    zo = torch.as_tensor(np.asarray(zone_obs, np.float32)).to(dtype)
    emb = hier_ref._encoder(sd, obs, zo)
    x = torch.relu(emb @ sd["actor.enc_.0.0.weight"].T + sd["actor.enc_.0.0.bias"])
    mu = 2 * (torch.sigmoid(x @ sd["actor.mu_.weight"].T + sd["actor.mu_.bias"]) - 0.5)
    std = torch.sigmoid(x @ sd["actor.std_.weight"].T + sd["actor.std_.bias"]) + 1e-3
    return mu.numpy(), std.numpy(), hier_ref._critic(sd, emb).numpy()


low = hier_ref.low


def scale_head_rows(sd, a, names=("actor.mu_", "actor.std_")):
    """Keeps the sigmoid heads `names` of state dict `sd` out of saturation on a batch, in place.  a: float64 [B, h], the
    heads' input (relu(actor.enc_.0.0(.)) of the batch).  Every head weight row w is divided by max(1, max_b |w . a_b| /
    3) (float64, rounded to float32 once); the biases stay.  -> float64 [B, rows]: the pre-activations w . a_b + bias of
    the rows of all `names` with the weights as they are afterwards.  With B = 0 nothing changes."""
    a = torch.as_tensor(np.asarray(a, np.float64))
    out = []
    for name in names:
        w = sd[f"{name}.weight"].to(torch.float64)
        if a.shape[0]:
            div = torch.clamp((a @ w.T).abs().max(dim=0).values / 3.0, min=1.0)
            sd[f"{name}.weight"] = (w / div[:, None]).to(torch.float32)
        out.append(a @ sd[f"{name}.weight"].to(torch.float64).T + sd[f"{name}.bias"].to(torch.float64))
    return torch.cat(out, dim=1).numpy()


def _head_input(sd, x, zone_obs):
    """float64 relu(actor.enc_.0.0(emb)) of the per-env input x (obs, or [obs, goal]): what mu_ / std_ are applied to."""
    sd = {k: torch.as_tensor(np.asarray(v)).to(torch.float64) for k, v in sd.items()}
    x = torch.as_tensor(np.asarray(x, np.float32)).to(torch.float64)
    zo = torch.as_tensor(np.asarray(zone_obs, np.float32)).to(torch.float64)
    if not len(x):
        return torch.zeros(0, sd["actor.enc_.0.0.bias"].shape[0], dtype=torch.float64)
    emb = hier_ref._encoder(sd, x, zo)
    return torch.relu(emb @ sd["actor.enc_.0.0.weight"].T + sd["actor.enc_.0.0.bias"])


def normalise_heads(hi_sd, lo_sd, obs, zone_obs, goal, has_goal):
    """scale_head_rows on both levels for one batch: the high level's goal_mu / goal_std rows on every env, the low
    level's mu / std rows on the envs with has_goal under their goal [B, 2].  In place.  -> (hi, lo) float64
    pre-activations [B, 4] and [has_goal.sum(), 4] of the rescaled heads."""
    has = np.asarray(has_goal, bool)
    obs, zone_obs = np.asarray(obs, np.float32), np.asarray(zone_obs, np.float32)
    pre_hi = scale_head_rows(hi_sd, _head_input(hi_sd, obs, zone_obs))
    x = np.concatenate([obs, np.asarray(goal, np.float32)], axis=1)[has]
    pre_lo = scale_head_rows(lo_sd, _head_input(lo_sd, x, zone_obs[has]))
    return pre_hi, pre_lo


def goal_noise(n, seed, env_index0, step):
    """float64 [n, 2]: the standard normal pair of the goal draw of envs 0 .. n-1 -- ``philox_ref.action_noise``'s
    arithmetic (float64 Box-Muller on the two float32 uniforms, the angle formed in float32) on the goal stream."""
    c = philox_ref._draw(n, seed, env_index0, step, TAG_XY_GOAL)
    u1 = philox_ref.uniform(c[0]).astype(np.float64)
    ang = (np.float32(6.283185307179586) * philox_ref.uniform(c[1])).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
