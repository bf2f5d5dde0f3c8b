"""The xy-goals agent's two PPO updates restated for the tests of the device learners (zenv_xyppo_*): this project's
own code, written from the reference's behaviour, no text of it.

  networks  HighPolicyValueModel / LoPolicyValueModel (xy-goals/src/hier_policy_value_models.py:19-72): the high level
            is the flat actor-critic's network with the plain critic (``ppo_update_ref.ACModelRef``), the low level the
            Zone-goals low level on [obs, goal] (``hppo_update_ref.LoModelRef``); both carry the reference's state_dict
            names, gradients come from torch autograd
  losses    the sub-batch bodies of update_hi_parameters / update_lo_parameters (xy-goals/src/torch_ac/algos/
            _hier_policy_opt.py:209-363).  The low level's is the Zone-goals low level's.  The high level's takes the
            Normal of the goal: the joint log_prob (summed over the two dimensions) against ONE recorded log_prob per
            row, and the entropy summed over the two dimensions before the mean over rows
  samples   lo_exps hold every one of the T frames of an env (:147-158): flat index i is env i // T, frame i % T
  norm      the gradient norm, taken and not clipped with
  heads     the derivative of the high level's loss with respect to the head pre-activations, per row, in numpy: the
            formulas k_xyppo_hi_loss (csrc/ppo_update.hip) computes

The float64 run of this code is the truth, the float32 run of the same code on the CPU the ruler for rounding
(``check_rule`` of tests/ppo_update_ref.py).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from tests import hppo_update_ref as RH
from tests import ppo_update_ref as RF
from tests.hppo_update_ref import (HALF_LOG_2PI, _clipped, _np_clipped_policy, _np_clipped_value, _np_sigmoid,
                                   lo_batch, lo_head_loss)
from tests.ppo_update_ref import STATS, adam_step, check_rule, perturbed, total_norm  # noqa: F401  (re-exported)

LO_HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.003, value_loss_coef=0.5, max_grad_norm=math.inf)
HI_HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=math.inf)


class HiModelRef(RF.ACModelRef):
    """forward -> (goal_mu [B, 2], goal_std [B, 2], value [B])."""

    def __init__(self, F, h, dtype=torch.float64):
        super().__init__(F, h, False, dtype)

    def forward(self, obs, zone_obs):
        mu, std, v, _ = super().forward(obs, zone_obs)
        return mu, std, v


LoModelRef = RH.LoModelRef


def model_from(level, state_dict, F, dtype):
    """level: "hi" or "lo"."""
    h = state_dict["env_model.zone_net_.0.bias"].shape[0]
    model = (HiModelRef if level == "hi" else LoModelRef)(F, h, dtype)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state_dict.items()})
    return model


def hi_entropy(std):
    """The high level's entropy statistic: per row the sum over the goal's two dimensions, then the mean over rows."""
    return torch.distributions.Normal(torch.zeros_like(std), std).entropy().sum(dim=-1).mean()


def hi_head_loss(mu, std, value, b, hyper):
    """The high level's sub-batch body from the actor's Normal and the critic's value.  b["goal"] [B, 2];
    b["log_prob"] [B]: the recorded one, already summed over the two dimensions."""
    dist = torch.distributions.Normal(mu, std)
    entropy = dist.entropy().sum(dim=-1).mean()
    policy_loss, value_loss = _clipped(dist.log_prob(b["goal"]).sum(dim=-1), value, b, hyper["clip_eps"])
    loss = policy_loss - hyper["entropy_coef"] * entropy + hyper["value_loss_coef"] * value_loss
    return loss, entropy, policy_loss, value_loss


def loss_and_stats(level, model, b, hyper):
    if level == "hi":
        mu, std, v = model(b["obs"], b["zone_obs"])
        loss, entropy, policy_loss, value_loss = hi_head_loss(mu, std, v, b, hyper)
    else:
        mu, std, v = model(b["obs"], b["zone_obs"], b["goal"])
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
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    stats["grad_norm"] = total_norm(grads.values())
    return grads, stats


def branches(level, model, b, clip_eps):
    """Which samples take a clipped branch: (policy, ratio above the range), (policy, below), (value)."""
    with torch.no_grad():
        if level == "hi":
            mu, std, v = model(b["obs"], b["zone_obs"])
            lp = torch.distributions.Normal(mu, std).log_prob(b["goal"]).sum(dim=1)
            old = b["log_prob"]
        else:
            mu, std, v = model(b["obs"], b["zone_obs"], b["goal"])
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


_HI_FIELDS = ("obs", "zone_obs", "goal", "value", "log_prob", "advantage", "returnn")


def lo_index(i, T):
    """Flat low-level sample index -> (env, frame): lo_exps flatten [N][T], every frame kept."""
    i = np.asarray(i)
    return i // T, i % T


def hi_batch(hi, idx, dtype):
    """hi: name -> array [M, ...]; idx: row indexes."""
    idx = np.asarray(idx, np.int64)
    return {k: torch.as_tensor(np.asarray(hi[k])[idx]).to(dtype) for k in _HI_FIELDS}


# lo_batch is hppo_update_ref's, here on arrays [N, T, ...]: it flattens the two leading axes whatever the second one is


# ---- the high level's head derivatives as the kernel forms them, per row, in numpy (any float dtype)
def joint_gaussian_head_derivatives(pre_mu, pre_std, v, goal, old_log_prob, old_value, adv, ret, hyper):
    """k_xyppo_hi_loss.  pre_mu, pre_std [B, 2]: the outputs of actor.mu_ / actor.std_ before the sigmoid; old_log_prob
    [B]: one per row, the recorded joint log_prob.  -> (d pre_mu [B, 2], d pre_std [B, 2], d v [B], entropy statistic)
    of the minibatch loss.  The entropy's part of d std is entropy_coef / (B std): twice the flat loss's, whose mean
    runs over 2 B terms."""
    inv_b = 1.0 / pre_mu.shape[0]
    smu, ssd = _np_sigmoid(pre_mu), _np_sigmoid(pre_std)
    mu, sd = 2.0 * (smu - 0.5), ssd + 1e-3
    diff = goal - mu
    lp = -(diff * diff) / (2.0 * (sd * sd)) - np.log(sd) - HALF_LOG_2PI
    _, g_lp = _np_clipped_policy((lp[:, 0] + lp[:, 1]) - old_log_prob, adv, hyper["clip_eps"], inv_b)
    var = sd * sd
    g_mu = g_lp[:, None] * (diff / var)
    g_sd = g_lp[:, None] * ((diff * diff) / (var * sd) - 1.0 / sd) - hyper["entropy_coef"] * inv_b / sd
    _, d_v = _np_clipped_value(v, old_value, ret, hyper["clip_eps"], hyper["value_loss_coef"], inv_b)
    entropy = (0.5 + HALF_LOG_2PI + np.log(sd)).sum(axis=1).sum() * inv_b
    return g_mu * 2.0 * smu * (1.0 - smu), g_sd * ssd * (1.0 - ssd), d_v, entropy
