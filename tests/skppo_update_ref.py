"""The fixed-length-skills agent's two PPO updates restated for the tests of the device learners (zenv_skppo_*): this
project's own code, written from the reference's behaviour, no text of it.

  networks  HighPolicyValueModel / LoPolicyValueModel (main/src/hier_policy_value_models.py:19-76) as torch modules of
            any dtype under the reference's state_dict names -- the operations of tests/skill_ref.py on the modules'
            own parameters; gradients come from torch autograd
  losses    the sub-batch bodies of update_lo_parameters / update_hi_parameters (main/src/torch_ac/algos/
            _hier_policy_opt.py:265-419).  The low level's is the flat one: the joint ratio of the two action
            components against a recorded log_prob per component, the entropy's mean over B x 2.  The high level's takes
            Categorical(logits = log_softmax(logits)) over the S skills, unmasked: one recorded log_prob per row, the
            entropy's mean over rows
  samples   lo_exps hold every one of the T frames of an env: flat index i is env i // T, frame i % T
  norm      the gradient norm, taken and not clipped with
  heads     the derivative of either loss with respect to the head pre-activations, per row, in numpy at float64 or
            float32: the formulas k_ppo_loss and k_skppo_hi_loss (csrc/ppo_update.hip) compute

The float64 run of this code is the truth, the float32 run of the same code on the CPU the ruler for rounding
(``check_rule`` of tests/ppo_update_ref.py).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from tests import skill_ref as SK
from tests.hppo_update_ref import (_clipped, _np_clipped_policy, _np_clipped_value, gaussian_head_derivatives,  # noqa: F401
                                   lo_head_loss)
from tests.ppo_update_ref import STATS, adam_step, check_rule, perturbed, total_norm  # noqa: F401  (re-exported)

LO_HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.003, value_loss_coef=0.5, max_grad_norm=math.inf)
HI_HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=math.inf)


def _env_model(x_dim, F, h):
    env = nn.Module()
    env.zone_net_ = nn.Sequential(nn.Linear(x_dim + F, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h))
    env.combine_net_ = nn.Linear(x_dim + h, h)
    return env


class HiModelRef(nn.Module):
    """forward -> (raw logits [B, S], value [B])."""

    def __init__(self, F, S, h, dtype=torch.float64):
        super().__init__()
        self.env_model = _env_model(8, F, h)
        actor = nn.Module()
        actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h, h), nn.ReLU()))
        actor.discrete_ = nn.Sequential(nn.Linear(h, S))
        self.actor = actor
        self.critic = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))
        self.to(dtype)

    def forward(self, obs, zone_obs):
        p = dict(self.named_parameters())
        emb = SK._encoder(p, obs, zone_obs)
        return self.actor.discrete_(self.actor.enc_(emb)), SK._critic(p, emb)


class LoModelRef(nn.Module):
    """forward -> (mu [B, 2], std [B, 2], value [B]); skill: int64 [B] in 0 .. S-1."""

    def __init__(self, F, S, h, dtype=torch.float64):
        super().__init__()
        self.S = S
        self.env_model = _env_model(8 + S, F, h)
        actor = nn.Module()
        actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h + S, h), nn.ReLU()))
        actor.mu_ = nn.Linear(h, 2)
        actor.std_ = nn.Linear(h, 2)
        self.actor = actor
        self.critic = nn.Sequential(nn.Linear(h + S, h), nn.ReLU(), nn.Linear(h, 1))
        self.to(dtype)

    def forward(self, obs, zone_obs, skill):
        p = dict(self.named_parameters())
        onehot = nn.functional.one_hot(skill, self.S).to(obs.dtype)
        x = torch.cat([SK._encoder(p, torch.cat([obs, onehot], dim=-1), zone_obs), onehot], dim=-1)
        a = self.actor.enc_(x)
        mu = 2.0 * (torch.sigmoid(self.actor.mu_(a)) - 0.5)
        std = torch.sigmoid(self.actor.std_(a)) + 1e-3
        return mu, std, SK._critic(p, x)


def sizes(hi_or_lo_sd, level):
    """(h, S) from a level's state_dict."""
    h = int(hi_or_lo_sd["env_model.zone_net_.0.bias"].shape[0])
    if level == "hi":
        return h, int(hi_or_lo_sd["actor.discrete_.0.bias"].shape[0])
    return h, int(hi_or_lo_sd["actor.enc_.0.0.weight"].shape[1]) - h


def model_from(level, state_dict, F, dtype):
    """level: "hi" or "lo"."""
    h, S = sizes(state_dict, level)
    model = (HiModelRef if level == "hi" else LoModelRef)(F, S, h, dtype)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state_dict.items()})
    return model


def hi_head_loss(logits, value, b, hyper):
    """The high level's sub-batch body from the model's raw logits: Categorical(logits = log_softmax(logits)).
    b["action"] int64 [B]: the recorded skill; b["log_prob"] [B]."""
    dist = torch.distributions.Categorical(logits=torch.log_softmax(logits, dim=1))
    entropy = dist.entropy().mean()
    policy_loss, value_loss = _clipped(dist.log_prob(b["action"]), value, b, hyper["clip_eps"])
    loss = policy_loss - hyper["entropy_coef"] * entropy + hyper["value_loss_coef"] * value_loss
    return loss, entropy, policy_loss, value_loss


def loss_and_stats(level, model, b, hyper):
    if level == "hi":
        logits, v = model(b["obs"], b["zone_obs"])
        loss, entropy, policy_loss, value_loss = hi_head_loss(logits, v, b, hyper)
    else:
        mu, std, v = model(b["obs"], b["zone_obs"], b["skill"])
        lo_b = dict(b, log_prob=b["log_prob"].sum(dim=1))
        loss, entropy, policy_loss, value_loss = lo_head_loss(mu, std, v, lo_b, hyper)
    stats = {"entropy": entropy.item(), "value": v.mean().item(), "value_std": 0.0, "policy_loss": policy_loss.item(),
             "value_loss": value_loss.item()}
    return loss, stats


def gradients(level, model, b, hyper):
    """state_dict key -> gradient of the loss, and the statistics with the gradient norm."""
    model.zero_grad()
    loss, stats = loss_and_stats(level, model, b, hyper)
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    stats["grad_norm"] = total_norm(grads.values())
    return grads, stats


def branches(level, model, b, clip_eps):
    """Which samples take a clipped branch: (policy, ratio above the range), (policy, below), (value)."""
    with torch.no_grad():
        if level == "hi":
            logits, v = model(b["obs"], b["zone_obs"])
            lp = torch.log_softmax(logits, dim=1).gather(1, b["action"].view(-1, 1)).squeeze(1)
            old = b["log_prob"]
        else:
            mu, std, v = model(b["obs"], b["zone_obs"], b["skill"])
            lp = torch.distributions.Normal(mu, std).log_prob(b["action"]).sum(dim=1)
            old = b["log_prob"].sum(dim=1)
        ratio = torch.exp(lp - old)
        hi = (ratio > 1.0 + clip_eps) & (b["advantage"] > 0)
        lo = (ratio < 1.0 - clip_eps) & (b["advantage"] < 0)
        dv = v - b["value"]
        vc = b["value"] + dv.clamp(-clip_eps, clip_eps)
        val = (dv.abs() > clip_eps) & ((vc - b["returnn"]).pow(2) > (v - b["returnn"]).pow(2))
    return hi, lo, val


class RefLearner:
    """One level's inner loop in a dtype: autograd gradients, the norm, torch's own Adam; the clip only when
    max_grad_norm is finite (the reference has none)."""

    def __init__(self, level, state_dict, F, dtype, hyper):
        self.level, self.hyper = level, hyper
        self.model = model_from(level, state_dict, F, dtype)
        self.opt = torch.optim.Adam(self.model.parameters(), hyper["lr"], eps=hyper["adam_eps"], foreach=False)

    def minibatch(self, batch):
        grads, stats = gradients(self.level, self.model, batch, self.hyper)
        if math.isfinite(self.hyper["max_grad_norm"]):
            nn.utils.clip_grad_norm_(self.model.parameters(), self.hyper["max_grad_norm"], foreach=False)
        self.opt.step()
        return [stats[k] for k in STATS]


_LO_FIELDS = ("obs", "zone_obs", "action", "log_prob", "value", "advantage", "returnn")
_HI_FIELDS = ("obs", "zone_obs", "value", "log_prob", "advantage", "returnn")


def lo_index(i, T):
    """Flat low-level sample index -> (env, frame): lo_exps flatten [N][T], every frame kept."""
    i = np.asarray(i)
    return i // T, i % T


def lo_batch(lo, idx, dtype):
    """lo: name -> array [N, T, ...] (ZoneVecEnv.collect_skills); idx: flat [N][T] sample indexes."""
    idx = np.asarray(idx, np.int64)
    out = {}
    for k in _LO_FIELDS + ("skill",):
        a = np.asarray(lo[k])
        flat = torch.as_tensor(a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])[idx])
        out[k] = flat.to(torch.int64) if k == "skill" else flat.to(dtype)
    return out


def hi_batch(hi, idx, dtype):
    """hi: name -> array [M, ...]; idx: row indexes."""
    idx = np.asarray(idx, np.int64)
    out = {k: torch.as_tensor(np.asarray(hi[k])[idx]).to(dtype) for k in _HI_FIELDS}
    out["action"] = torch.as_tensor(np.asarray(hi["action"])[idx].astype(np.int64))
    return out


# ---- the high level's head derivatives as the kernel forms them, per row, in numpy (any float dtype)
def skill_head_derivatives(logits, action, old_log_prob, v, old_value, adv, ret, hyper):
    """k_skppo_hi_loss.  logits [B, S] raw, action [B].  With p the softmax, H the row's entropy and g_lp = -adv / B
    through ratio: d logit_s = g_lp (1[s = a] - p_s) + (entropy_coef / B) p_s (log p_s + H).
    -> (d logits [B, S], d v [B], entropy statistic)."""
    B, S = logits.shape
    inv_b = logits.dtype.type(1.0) / logits.dtype.type(B)
    m = logits.max(axis=1, keepdims=True)
    lp = logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))
    p = np.exp(lp)
    H = -(p * lp).sum(axis=1)
    a = np.asarray(action, np.int64)
    _, g_lp = _np_clipped_policy(lp[np.arange(B), a] - old_log_prob, adv, hyper["clip_eps"], inv_b)
    onehot = (np.arange(S)[None, :] == a[:, None]).astype(logits.dtype)
    g_lp = g_lp.astype(logits.dtype)                        # np.where's constants are float64
    d = g_lp[:, None] * (onehot - p) + logits.dtype.type(hyper["entropy_coef"]) * inv_b * p * (lp + H[:, None])
    _, d_v = _np_clipped_value(v, old_value, ret, hyper["clip_eps"], hyper["value_loss_coef"], inv_b)
    return d, d_v.astype(logits.dtype), H.sum() * inv_b
