"""TEST INFRASTRUCTURE -- float32 torch restatement of the Zone-goals agent's two networks (checker only).

Restated from their description, op for op:
* ``HighPolicyValueModel``  zone-goals/src/hier_policy_value_models.py:19-56: emb = ZoneEnvModel(obs, zone_obs);
  logit_z = actor.2(relu(actor.0([emb, zone_obs[z]]))); value = critic.2(relu(critic.0(emb)))
* ``LoPolicyValueModel``    :58-86: emb = ZoneEnvGoalModel(obs, goal, zone_obs) (env_model.py:82-116), PolicyNetwork
  (policy_network.py:40-53, Box branch) and the same critic
* ``init_params``           :11-17: rows of N(0, 1) normalised to unit norm, zero biases (small random ones here, so
  that the bias path is exercised)
"""
import numpy as np
import torch


def _lin(g, n_out, n_in, bias_scale, weight_scale=1.0):
    w = torch.randn(n_out, n_in, generator=g)
    w = w / torch.sqrt(w.pow(2).sum(1, keepdim=True))
    if weight_scale != 1.0:
        w = w * weight_scale
    return w, bias_scale * torch.randn(n_out, generator=g)


def random_state_dicts(F, h=128, seed=0, bias_scale=0.1, critics=True, weight_scale=1.0):
    """(hi_state_dict, lo_state_dict) with the reference's key names, float32 torch tensors.  weight_scale multiplies
    every weight row (unit norm by default): larger activations, for the precision sweeps."""
    g = torch.Generator().manual_seed(seed)

    def lin(g, n_out, n_in, bias_scale):
        return _lin(g, n_out, n_in, bias_scale, weight_scale)

    hi, lo = {}, {}
    for sd, x in ((hi, 8), (lo, 10)):
        for name, n_in in (("zone_net_.0", x + F), ("zone_net_.2", h), ("zone_net_.4", h)):
            sd[f"env_model.{name}.weight"], sd[f"env_model.{name}.bias"] = lin(g, h, n_in, bias_scale)
        sd["env_model.combine_net_.weight"], sd["env_model.combine_net_.bias"] = lin(g, h, x + h, bias_scale)
    hi["actor.0.weight"], hi["actor.0.bias"] = lin(g, h, h + F, bias_scale)
    hi["actor.2.weight"], hi["actor.2.bias"] = lin(g, 1, h, bias_scale)
    lo["actor.enc_.0.0.weight"], lo["actor.enc_.0.0.bias"] = lin(g, h, h, bias_scale)
    lo["actor.mu_.weight"], lo["actor.mu_.bias"] = lin(g, 2, h, bias_scale)
    lo["actor.std_.weight"], lo["actor.std_.bias"] = lin(g, 2, h, bias_scale)
    if critics:
        for sd in (hi, lo):
            sd["critic.0.weight"], sd["critic.0.bias"] = lin(g, h, h, bias_scale)
            sd["critic.2.weight"], sd["critic.2.bias"] = lin(g, 1, h, bias_scale)
    return hi, lo


def _encoder(sd, x, zo):
    """ZoneEnvModel / ZoneEnvGoalModel: x = obs [B,8] or [obs, goal] [B,10], zo [B,Z,F] -> emb [B,h]."""
    bs, n_zones = zo.shape[0], zo.shape[1]
    rows = torch.cat([x.view(bs, 1, -1).expand(bs, n_zones, x.shape[1]), zo], dim=-1)
    y = torch.relu(rows @ sd["env_model.zone_net_.0.weight"].T + sd["env_model.zone_net_.0.bias"])
    y = torch.relu(y @ sd["env_model.zone_net_.2.weight"].T + sd["env_model.zone_net_.2.bias"])
    y = y @ sd["env_model.zone_net_.4.weight"].T + sd["env_model.zone_net_.4.bias"]
    zone_emb = y.sum(dim=1) / n_zones
    return torch.cat([x, zone_emb], dim=-1) @ sd["env_model.combine_net_.weight"].T + sd["env_model.combine_net_.bias"]


def _critic(sd, emb):
    if "critic.0.weight" not in sd:
        return torch.zeros(emb.shape[0], dtype=emb.dtype)
    v = torch.relu(emb @ sd["critic.0.weight"].T + sd["critic.0.bias"])
    return (v @ sd["critic.2.weight"].T + sd["critic.2.bias"]).squeeze(1)


def high(hi_sd, obs, zone_obs, available, dtype=torch.float32):
    """-> masked logits [B,Z] (-inf where bit z of available[b] is clear), value [B]; numpy arrays of `dtype`
    (float32: the reference's modules; float64: the same operations on the same float32 inputs, as a precise yardstick)."""
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in hi_sd.items()}
    obs = torch.as_tensor(np.asarray(obs, np.float32)).to(dtype)
    zo = torch.as_tensor(np.asarray(zone_obs, np.float32)).to(dtype)
    emb = _encoder(sd, obs, zo)
    bs, n_zones = zo.shape[0], zo.shape[1]
    x = torch.cat([emb.view(bs, 1, -1).expand(bs, n_zones, emb.shape[1]), zo], dim=-1)
    x = torch.relu(x @ sd["actor.0.weight"].T + sd["actor.0.bias"])
    logits = (x @ sd["actor.2.weight"].T + sd["actor.2.bias"]).squeeze(-1)
    bits = (np.asarray(available, np.uint32)[:, None] >> np.arange(n_zones, dtype=np.uint32)) & 1
    logits[torch.as_tensor(bits == 0)] = float("-inf")
    return logits.numpy(), _critic(sd, emb).numpy()


def low(lo_sd, obs, zone_obs, goal_xy, dtype=torch.float32):
    """goal_xy [B,2] = the goal zone's centre / 3 (float32) -> mu [B,2], std [B,2], value [B]; numpy arrays of `dtype`."""
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in lo_sd.items()}
    obs = torch.as_tensor(np.asarray(obs, np.float32)).to(dtype)
    zo = torch.as_tensor(np.asarray(zone_obs, np.float32)).to(dtype)
    goal = torch.as_tensor(np.asarray(goal_xy, np.float32)).to(dtype)
    emb = _encoder(sd, torch.cat([obs, goal], dim=-1), zo)
    a = torch.relu(emb @ sd["actor.enc_.0.0.weight"].T + sd["actor.enc_.0.0.bias"])
    mu = 2 * (torch.sigmoid(a @ sd["actor.mu_.weight"].T + sd["actor.mu_.bias"]) - 0.5)
    std = torch.sigmoid(a @ sd["actor.std_.weight"].T + sd["actor.std_.bias"]) + 1e-3
    return mu.numpy(), std.numpy(), _critic(sd, emb).numpy()
