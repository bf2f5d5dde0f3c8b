"""TEST INFRASTRUCTURE -- float32 torch restatement of the variable-length Options agent (checker only).

Restated from their description: the two networks are the fixed-length-skills agent's (tests/skill_ref.py) except that
the low level's PolicyNetwork has a Box of action_dim + 1 = 3 outputs (options/src/hier_policy_value_models.py:46-74),
so actor.mu_ / actor.std_ are [3, h].  Per step (options/scripts/evaluate_hier.py:63-75) the first two components of
the sample are the action and termination_prob = sigmoid(4 * sample[2] - 3).

The host draws: the third normal comes from words 2 and 3 of the action draw's Philox block (tag 0x4D4C50), the
termination uniform from word 0 of a block with the tag 0x4F5054 (tests/philox_ref.py for the keying)."""
import numpy as np
import torch

from tests import philox_ref, skill_ref, xy_ref

TAG_OPTION_TERM = 0x4F5054


def random_state_dicts(F, S, h=128, seed=0, critics=True, term_bias=None, **kw):
    """skill_ref.random_state_dicts with the low level's two heads widened to three rows (a generator of their own;
    weight_scale multiplies them like every other weight row).
    term_bias: the third row of actor.mu_ becomes weight 0, bias term_bias, and the third row of actor.std_ weight 0,
    bias -100 -- mu_2 = 2 (sigmoid(term_bias) - 0.5) for every input, std_2 at its floor of 1e-3."""
    hi, lo = skill_ref.random_state_dicts(F, S, h=h, seed=seed, critics=critics, **kw)
    g = torch.Generator().manual_seed(seed + 7919)
    for name in ("actor.mu_", "actor.std_"):
        w = torch.randn(1, h, generator=g)
        w = w / torch.sqrt(w.pow(2).sum(1, keepdim=True)) * kw.get("weight_scale", 1.0)
        b = 0.1 * torch.randn(1, generator=g)
        lo[f"{name}.weight"] = torch.cat([lo[f"{name}.weight"], w], dim=0)
        lo[f"{name}.bias"] = torch.cat([lo[f"{name}.bias"], b], dim=0)
    if term_bias is not None:
        lo["actor.mu_.weight"][2] = 0.0
        lo["actor.mu_.bias"][2] = float(term_bias)
        lo["actor.std_.weight"][2] = 0.0
        lo["actor.std_.bias"][2] = -100.0
    return hi, lo


def skill_planner_part(lo_sd):
    """The low level's state dict without the third rows: what a skill planner of the same weights would hold."""
    out = dict(lo_sd)
    for k in ("actor.mu_.weight", "actor.mu_.bias", "actor.std_.weight", "actor.std_.bias"):
        out[k] = lo_sd[k][:2].clone()
    return out


high = skill_ref.high


def low(lo_sd, obs, zone_obs, skill, S, dtype=torch.float32):
    """skill [B] in 0 .. S-1 -> mu [B,3], std [B,3], value [B]; numpy arrays of `dtype`.  skill_ref.low is written for
    any number of head rows."""
    return skill_ref.low(lo_sd, obs, zone_obs, skill, S, dtype)


def normalise_heads(lo_sd, obs, zone_obs, skill, S):
    """xy_ref.scale_head_rows on the low level's three mu_ and three std_ rows for one batch: the envs with skill >= 0,
    under their skill.  In place.  -> float64 pre-activations [(skill >= 0).sum(), 6] of the rescaled heads."""
    has = np.asarray(skill) >= 0
    if not has.any():
        return xy_ref.scale_head_rows(lo_sd, np.zeros((0, lo_sd["actor.mu_.weight"].shape[1])))
    sd = skill_ref._t(lo_sd, torch.float64)
    onehot = torch.nn.functional.one_hot(torch.as_tensor(np.asarray(skill)[has], dtype=torch.int64), S).to(torch.float64)
    obs = skill_ref._x(np.asarray(obs, np.float32)[has], torch.float64)
    zo = skill_ref._x(np.asarray(zone_obs, np.float32)[has], torch.float64)
    emb = skill_ref._encoder(sd, torch.cat([obs, onehot], dim=-1), zo)
    a = torch.relu(torch.cat([emb, onehot], dim=-1) @ sd["actor.enc_.0.0.weight"].T + sd["actor.enc_.0.0.bias"])
    return xy_ref.scale_head_rows(lo_sd, a.numpy())


def term_prob(a2):
    """sigmoid(4 a - 3) in float64."""
    return 1.0 / (1.0 + np.exp(-(4.0 * np.asarray(a2, np.float64) - 3.0)))


def term_noise(n, seed, env_index0, step_index):
    """float64 [n]: the standard normal of the third component -- Box-Muller's cosine branch in float64 on the float32
    uniforms of words 2 and 3, the angle formed as the device forms it (philox_ref.action_noise)."""
    c = philox_ref._draw(n, seed, env_index0, step_index, philox_ref.TAG_ACTION)
    u1 = philox_ref.uniform(c[2]).astype(np.float64)
    ang = (np.float32(6.283185307179586) * philox_ref.uniform(c[3])).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(ang)


def term_uniform(n, seed, env_index0, step_index):
    """float32 [n]: the uniform of the termination draw of envs 0 .. n-1."""
    return philox_ref.uniform(philox_ref._draw(n, seed, env_index0, step_index, TAG_OPTION_TERM)[0])
