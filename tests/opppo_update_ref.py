"""The Options agent's two PPO updates restated for the tests of the device learners (zenv_opppo_*): this project's own
code, written from the reference's behaviour, no text of it.

  networks  HighPolicyValueModel / LoPolicyValueModel (options/src/hier_policy_value_models.py) as torch modules of any
            dtype under the reference's state_dict names.  The high level is the skill planner's (HiModelRef of
            tests/skppo_update_ref.py, the same class); the low level is the skill planner's with three rows in
            actor.mu_ / actor.std_ -- the action's two components and a_2, whose sample ends the option
  losses    the sub-batch bodies of update_lo_parameters / update_hi_parameters (options/src/torch_ac/algos/
            _hier_policy_opt.py:208-381).  The low level's: the joint ratio of the THREE components against a recorded
            log_prob per component, the entropy's mean over B x 3.  a_2 is a third action dimension and nothing more:
            sigmoid(4 a_2 - 3) and the termination draw play no part.  The high level's takes Categorical(logits =
            log_softmax(logits)) over the S skills, unmasked: one recorded log_prob per row, the entropy's mean over rows
  samples   lo_exps hold frames 0 .. T-2 of an env: flat index i is env i // (T - 1), frame i % (T - 1)
  norm      the gradient norm, taken and not clipped with
  heads     the derivative of either loss with respect to the head pre-activations, per row, in numpy at float64 or
            float32: the formulas k_skppo_lo_loss<3> (seven columns: three of actor.mu_, three of actor.std_, the value)
            and k_skppo_hi_loss (csrc/ppo_update.hip) compute

The float64 run of this code is the truth, the float32 run of the same code on the CPU the ruler for rounding
(``check_rule`` of tests/ppo_update_ref.py).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from tests import skill_ref as SK
from tests.hppo_update_ref import (HALF_LOG_2PI, _clipped, _np_clipped_policy, _np_clipped_value, _np_sigmoid,  # noqa: F401
                                   lo_head_loss)
from tests.ppo_update_ref import STATS, adam_step, check_rule, perturbed, total_norm  # noqa: F401  (re-exported)
from tests.skppo_update_ref import (HiModelRef, _env_model, hi_batch, hi_head_loss, skill_head_derivatives)  # noqa: F401

LO_HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.003, value_loss_coef=0.5, max_grad_norm=math.inf)
HI_HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=math.inf)
NA = 3                      # the low level's action components


class LoModelRef(nn.Module):
    """forward -> (mu [B, 3], std [B, 3], value [B]); skill: int64 [B] in 0 .. S-1."""

    def __init__(self, F, S, h, dtype=torch.float64):
        super().__init__()
        self.S = S
        self.env_model = _env_model(8 + S, F, h)
        actor = nn.Module()
        actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h + S, h), nn.ReLU()))
        actor.mu_ = nn.Linear(h, NA)
        actor.std_ = nn.Linear(h, NA)
        self.actor = actor
        self.critic = nn.Sequential(nn.Linear(h + S, h), nn.ReLU(), nn.Linear(h, 1))
        self.to(dtype)

    def pre_activations(self, obs, zone_obs, skill):
        """(actor.mu_'s output [B, 3], actor.std_'s [B, 3], value [B]) before the sigmoids."""
        p = dict(self.named_parameters())
        onehot = nn.functional.one_hot(skill, self.S).to(obs.dtype)
        x = torch.cat([SK._encoder(p, torch.cat([obs, onehot], dim=-1), zone_obs), onehot], dim=-1)
        a = self.actor.enc_(x)
        return self.actor.mu_(a), self.actor.std_(a), SK._critic(p, x)

    def forward(self, obs, zone_obs, skill):
        pre_mu, pre_std, v = self.pre_activations(obs, zone_obs, skill)
        return 2.0 * (torch.sigmoid(pre_mu) - 0.5), torch.sigmoid(pre_std) + 1e-3, v


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


def loss_and_stats(level, model, b, hyper):
    if level == "hi":
        logits, v = model(b["obs"], b["zone_obs"])
        loss, entropy, policy_loss, value_loss = hi_head_loss(logits, v, b, hyper)
    else:
        mu, std, v = model(b["obs"], b["zone_obs"], b["skill"])
        lo_b = dict(b, log_prob=b["log_prob"].sum(dim=1))           # the three recorded log_probs
        loss, entropy, policy_loss, value_loss = lo_head_loss(mu, std, v, lo_b, hyper)   # entropy().mean(): B x 3
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


def lo_index(i, T):
    """Flat low-level sample index -> (env, frame): lo_exps flatten [N][T - 1]; frame T - 1 is not among them."""
    i = np.asarray(i)
    return i // (T - 1), i % (T - 1)


def lo_batch(lo, idx, dtype):
    """lo: name -> array [N, T - 1, ...] with action / log_prob [.., 3] (ZoneVecEnv.collect_options), or with the
    third component apart in term_action / term_log_prob [N, T - 1] (TorchZoneEnv's); idx: flat [N][T - 1] indexes."""
    idx = np.asarray(idx, np.int64)
    lo = dict(lo)
    if "term_action" in lo:
        lo["action"] = np.concatenate([np.asarray(lo["action"]), np.asarray(lo["term_action"])[..., None]], axis=-1)
        lo["log_prob"] = np.concatenate([np.asarray(lo["log_prob"]), np.asarray(lo["term_log_prob"])[..., None]], axis=-1)
    out = {}
    for k in _LO_FIELDS + ("skill",):
        a = np.asarray(lo[k])
        flat = torch.as_tensor(a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])[idx])
        out[k] = flat.to(torch.int64) if k == "skill" else flat.to(dtype)
    assert out["action"].shape[1] == NA and out["log_prob"].shape[1] == NA
    return out


# ---- the low level's head derivatives as the kernel forms them, per sample, in numpy (any float dtype)
def option_head_derivatives(pre_mu, pre_std, v, action, old_log_prob, old_value, adv, ret, hyper):
    """k_skppo_lo_loss<3>.  pre_mu, pre_std [B, 3]: the outputs of actor.mu_ / actor.std_ before the sigmoid; action
    and old_log_prob [B, 3] per component.  The ratio is over all three components; the entropy's mean is over B x 3,
    so its term in the std's derivative carries 1 / (3 B).  -> (d pre_mu [B, 3], d pre_std [B, 3], d v [B]): the seven
    columns of the head's delta."""
    B, A = pre_mu.shape
    one = pre_mu.dtype.type
    inv_b = one(1.0) / one(B)
    smu, ssd = _np_sigmoid(pre_mu), _np_sigmoid(pre_std)
    mu, sd = one(2.0) * (smu - one(0.5)), ssd + one(1e-3)
    diff = action - mu
    lp = -(diff * diff) / (one(2.0) * (sd * sd)) - np.log(sd) - one(HALF_LOG_2PI)
    _, g_lp = _np_clipped_policy((lp - old_log_prob).sum(axis=1), adv, hyper["clip_eps"], inv_b)
    g_lp = g_lp.astype(pre_mu.dtype)
    var = sd * sd
    g_mu = g_lp[:, None] * (diff / var)
    g_sd = g_lp[:, None] * ((diff * diff) / (var * sd) - one(1.0) / sd) - one(hyper["entropy_coef"]) * (inv_b / one(A)) / sd
    _, d_v = _np_clipped_value(v, old_value, ret, hyper["clip_eps"], hyper["value_loss_coef"], inv_b)
    return g_mu * one(2.0) * smu * (one(1.0) - smu), g_sd * ssd * (one(1.0) - ssd), d_v.astype(pre_mu.dtype)
