"""TEST INFRASTRUCTURE -- float32 torch restatement of the fixed-length-skills agent's two networks (checker only).

Restated from their description, op for op:
* ``HighPolicyValueModel``  main/src/hier_policy_value_models.py:19-43: emb = ZoneEnvModel(obs, zone_obs);
  x = actor.discrete_.0(relu(actor.enc_.0.0(emb))), Categorical(logits=log_softmax(x)); value = critic.2(relu(critic.0(emb)))
* ``LoPolicyValueModel``    :45-76: onehot = one_hot(skill, S); emb = ZoneEnvSkillModel(obs, onehot, zone_obs)
  (env_model.py:81-117: zone_net_ on [obs, onehot, zone row], combine_net_ on [obs, onehot, zone_emb]); x = [emb, onehot];
  PolicyNetwork(x) (policy_network.py, Box branch) and critic.2(relu(critic.0(x)))
"""
import numpy as np
import torch


def _lin(g, n_out, n_in, bias_scale, weight_scale=1.0):
    w = torch.randn(n_out, n_in, generator=g)
    w = w / torch.sqrt(w.pow(2).sum(1, keepdim=True))
    if weight_scale != 1.0:
        w = w * weight_scale
    return w, bias_scale * torch.randn(n_out, generator=g)


def random_state_dicts(F, S, h=128, seed=0, bias_scale=0.1, critics=True, weight_scale=1.0):
    """(hi_state_dict, lo_state_dict) with the reference's key names, float32 torch tensors.  The skill columns get
    a larger scale so that the skill visibly changes the low level's output.  weight_scale multiplies every weight row
    (unit norm by default): larger activations, for the precision sweeps."""
    g = torch.Generator().manual_seed(seed)

    def lin(g, n_out, n_in, bias_scale):
        return _lin(g, n_out, n_in, bias_scale, weight_scale)

    hi, lo = {}, {}
    for sd, x in ((hi, 8), (lo, 8 + S)):
        for name, n_in in (("zone_net_.0", x + F), ("zone_net_.2", h), ("zone_net_.4", h)):
            sd[f"env_model.{name}.weight"], sd[f"env_model.{name}.bias"] = lin(g, h, n_in, bias_scale)
        sd["env_model.combine_net_.weight"], sd["env_model.combine_net_.bias"] = lin(g, h, x + h, bias_scale)
    hi["actor.enc_.0.0.weight"], hi["actor.enc_.0.0.bias"] = lin(g, h, h, bias_scale)
    hi["actor.discrete_.0.weight"], hi["actor.discrete_.0.bias"] = lin(g, S, h, bias_scale)
    lo["actor.enc_.0.0.weight"], lo["actor.enc_.0.0.bias"] = lin(g, h, h + S, bias_scale)
    lo["actor.mu_.weight"], lo["actor.mu_.bias"] = lin(g, 2, h, bias_scale)
    lo["actor.std_.weight"], lo["actor.std_.bias"] = lin(g, 2, h, bias_scale)
    if critics:
        hi["critic.0.weight"], hi["critic.0.bias"] = lin(g, h, h, bias_scale)
        lo["critic.0.weight"], lo["critic.0.bias"] = lin(g, h, h + S, bias_scale)
        for sd in (hi, lo):
            sd["critic.2.weight"], sd["critic.2.bias"] = lin(g, 1, h, bias_scale)
    for key, lo_col in (("env_model.zone_net_.0.weight", 8), ("env_model.combine_net_.weight", 8),
                        ("actor.enc_.0.0.weight", h), ("critic.0.weight", h)):
        if key in lo:
            lo[key][:, lo_col:lo_col + S] *= 3.0
    return hi, lo


def _t(sd, dtype=torch.float32):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}


def _x(a, dtype):
    return torch.as_tensor(np.asarray(a, np.float32)).to(dtype)


def _encoder(sd, x, zo):
    """ZoneEnvModel on a per-env input x [B,X] (obs, or [obs, onehot]) and zone rows zo [B,Z,F] -> emb [B,h]."""
    bs, n_zones = zo.shape[0], zo.shape[1]
    rows = torch.cat([x.view(bs, 1, -1).expand(bs, n_zones, x.shape[1]), zo], dim=-1)
    y = torch.relu(rows @ sd["env_model.zone_net_.0.weight"].T + sd["env_model.zone_net_.0.bias"])
    y = torch.relu(y @ sd["env_model.zone_net_.2.weight"].T + sd["env_model.zone_net_.2.bias"])
    y = y @ sd["env_model.zone_net_.4.weight"].T + sd["env_model.zone_net_.4.bias"]
    zone_emb = y.sum(dim=1) / n_zones
    return torch.cat([x, zone_emb], dim=-1) @ sd["env_model.combine_net_.weight"].T + sd["env_model.combine_net_.bias"]


def _critic(sd, x):
    if "critic.0.weight" not in sd:
        return torch.zeros(x.shape[0], dtype=x.dtype)
    v = torch.relu(x @ sd["critic.0.weight"].T + sd["critic.0.bias"])
    return (v @ sd["critic.2.weight"].T + sd["critic.2.bias"]).squeeze(1)


def high(hi_sd, obs, zone_obs, dtype=torch.float32):
    """-> log-softmax logits [B,S], value [B]; numpy arrays of `dtype` (float32: the reference's modules; float64: the
    same operations on the same float32 inputs, as a precise yardstick)."""
    sd = _t(hi_sd, dtype)
    emb = _encoder(sd, _x(obs, dtype), _x(zone_obs, dtype))
    a = torch.relu(emb @ sd["actor.enc_.0.0.weight"].T + sd["actor.enc_.0.0.bias"])
    x = a @ sd["actor.discrete_.0.weight"].T + sd["actor.discrete_.0.bias"]
    return torch.log_softmax(x, dim=1).numpy(), _critic(sd, emb).numpy()


def low(lo_sd, obs, zone_obs, skill, S, dtype=torch.float32):
    """skill [B] in 0 .. S-1 -> mu [B,2], std [B,2], value [B]; numpy arrays of `dtype`."""
    sd = _t(lo_sd, dtype)
    onehot = torch.nn.functional.one_hot(torch.as_tensor(np.asarray(skill), dtype=torch.int64), S).to(dtype)
    obs = _x(obs, dtype)
    emb = _encoder(sd, torch.cat([obs, onehot], dim=-1), _x(zone_obs, dtype))
    x = torch.cat([emb, onehot], dim=-1)
    a = torch.relu(x @ sd["actor.enc_.0.0.weight"].T + sd["actor.enc_.0.0.bias"])
    mu = 2 * (torch.sigmoid(a @ sd["actor.mu_.weight"].T + sd["actor.mu_.bias"]) - 0.5)
    std = torch.sigmoid(a @ sd["actor.std_.weight"].T + sd["actor.std_.bias"]) + 1e-3
    return mu.numpy(), std.numpy(), _critic(sd, x).numpy()
