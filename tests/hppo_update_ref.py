"""The Zone-goals agent's two PPO updates restated for the tests of the device learners (zenv_hppo_*): this project's
own code, written from the reference's behaviour, no text of it.

  networks  HighPolicyValueModel / LoPolicyValueModel (zone-goals/src/hier_policy_value_models.py:19-86) as torch
            modules of any dtype under the reference's state_dict names; the arithmetic of the encoder and the critic
            is tests/hier_ref.py's, called on the modules' parameters; gradients come from torch autograd
  losses    the sub-batch bodies of update_lo_parameters / update_hi_parameters (zone-goals/src/torch_ac/algos/
            _hier_policy_opt.py:235-258, :312-334)
  norm      the gradient norm of :271 / :348 (taken, not clipped with: the reference's clip is commented out)
  Adam      torch.optim.Adam (betas 0.9 / 0.999, no weight decay, no amsgrad)
  heads     the derivatives of both loss bodies with respect to the head pre-activations, per sample, in numpy: the
            formulas k_ppo_loss and k_hppo_loss (csrc/ppo_update.hip) compute

The float64 run of this code is the truth, the float32 run of the same code on the CPU the ruler for rounding
(``check_rule`` of tests/ppo_update_ref.py).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from tests import hier_ref as H
from tests.ppo_update_ref import STATS, adam_step, check_rule, perturbed, total_norm  # noqa: F401  (re-exported)

LO_HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.003, value_loss_coef=0.5, max_grad_norm=math.inf)
HI_HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=math.inf)
HALF_LOG_2PI = 0.9189385332046727


def _env_model(x_dim, F, h):
    env = nn.Module()
    env.zone_net_ = nn.Sequential(nn.Linear(x_dim + F, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h))
    env.combine_net_ = nn.Linear(x_dim + h, h)
    return env


def _critic(h):
    return nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))


class HiModelRef(nn.Module):
    """forward -> (raw logits [B, Z], value [B])."""

    def __init__(self, F, h, dtype=torch.float64):
        super().__init__()
        self.env_model = _env_model(8, F, h)
        self.actor = nn.Sequential(nn.Linear(h + F, h), nn.ReLU(), nn.Linear(h, 1))
        self.critic = _critic(h)
        self.to(dtype)

    def forward(self, obs, zone_obs):
        p = dict(self.named_parameters())
        emb = H._encoder(p, obs, zone_obs)
        bs, Z = zone_obs.shape[0], zone_obs.shape[1]
        x = torch.cat([emb.view(bs, 1, -1).expand(bs, Z, emb.shape[1]), zone_obs], dim=-1)
        return self.actor(x).squeeze(-1), H._critic(p, emb)


class LoModelRef(nn.Module):
    """forward -> (mu [B, 2], std [B, 2], value [B])."""

    def __init__(self, F, h, dtype=torch.float64):
        super().__init__()
        self.env_model = _env_model(10, F, h)
        actor = nn.Module()
        actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h, h), nn.ReLU()))
        actor.mu_ = nn.Linear(h, 2)
        actor.std_ = nn.Linear(h, 2)
        self.actor = actor
        self.critic = _critic(h)
        self.to(dtype)

    def forward(self, obs, zone_obs, goal):
        p = dict(self.named_parameters())
        emb = H._encoder(p, torch.cat([obs, goal], dim=-1), zone_obs)
        a = self.actor.enc_(emb)
        mu = 2.0 * (torch.sigmoid(self.actor.mu_(a)) - 0.5)
        std = torch.sigmoid(self.actor.std_(a)) + 1e-3
        return mu, std, H._critic(p, emb)


def model_from(level, state_dict, F, dtype):
    """level: "hi" or "lo"."""
    h = state_dict["env_model.zone_net_.0.bias"].shape[0]
    model = (HiModelRef if level == "hi" else LoModelRef)(F, h, dtype)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state_dict.items()})
    return model


def _clipped(log_prob, value, b, eps):
    """The ratio, the clipped surrogate and the clipped value loss both bodies share."""
    ratio = torch.exp(log_prob - b["log_prob"])
    surr1 = ratio * b["advantage"]
    surr2 = torch.clamp(ratio, 1.0 - eps, 1.0 + eps) * b["advantage"]
    policy_loss = -torch.min(surr1, surr2).mean()
    clipped = b["value"] + torch.clamp(value - b["value"], -eps, eps)
    value_loss = torch.max((value - b["returnn"]).pow(2), (clipped - b["returnn"]).pow(2)).mean()
    return policy_loss, value_loss


def lo_head_loss(mu, std, value, b, hyper):
    """:238-257 from the actor's Normal and the critic's value.  b["log_prob"]: the recorded one, summed over the two
    action components."""
    dist = torch.distributions.Normal(mu, std)
    entropy = dist.entropy().mean()
    policy_loss, value_loss = _clipped(dist.log_prob(b["action"]).sum(dim=1), value, b, hyper["clip_eps"])
    loss = policy_loss - hyper["entropy_coef"] * entropy + hyper["value_loss_coef"] * value_loss
    return loss, entropy, policy_loss, value_loss


def hi_head_loss(logits, value, b, hyper):
    """:315-334 from the model's raw logits: the model hands out Categorical(logits), the update masks that
    distribution's (normalised) logits with -inf and builds a second Categorical."""
    lg = torch.distributions.Categorical(logits=logits).logits.clone()
    lg[~b["action_mask"]] = float("-inf")
    dist = torch.distributions.Categorical(logits=lg)
    entropy = dist.entropy().mean()
    policy_loss, value_loss = _clipped(dist.log_prob(b["action"]), value, b, hyper["clip_eps"])
    loss = policy_loss - hyper["entropy_coef"] * entropy + hyper["value_loss_coef"] * value_loss
    return loss, entropy, policy_loss, value_loss


def hi_head_loss_independent(logits, value, b, hyper):
    """The same loss stated another way: per row, torch.log_softmax over the available columns only."""
    lps, ents = [], []
    for i in range(logits.shape[0]):
        cols = torch.nonzero(b["action_mask"][i]).flatten()
        lp = torch.log_softmax(logits[i, cols], dim=0)
        ents.append(-(lp.exp() * lp).sum())
        lps.append(lp[(cols == b["action"][i]).nonzero().flatten()[0]])
    entropy = torch.stack(ents).mean()
    policy_loss, value_loss = _clipped(torch.stack(lps), value, b, hyper["clip_eps"])
    loss = policy_loss - hyper["entropy_coef"] * entropy + hyper["value_loss_coef"] * value_loss
    return loss, entropy, policy_loss, value_loss


def loss_and_stats(level, model, b, hyper):
    if level == "hi":
        logits, v = model(b["obs"], b["zone_obs"])
        loss, entropy, policy_loss, value_loss = hi_head_loss(logits, v, b, hyper)
    else:
        mu, std, v = model(b["obs"], b["zone_obs"], b["goal"])
        lo_b = dict(b, log_prob=b["log_prob"].sum(dim=1))
        loss, entropy, policy_loss, value_loss = lo_head_loss(mu, std, v, lo_b, hyper)
    stats = {"entropy": entropy.item(), "value": v.mean().item(), "value_std": 0.0, "policy_loss": policy_loss.item(),
             "value_loss": value_loss.item()}
    return loss, stats


def gradients(level, model, b, hyper):
    """state_dict key -> gradient of the loss, and the statistics with the norm of :271 / :348."""
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
            logits, v = model(b["obs"], b["zone_obs"])
            lg = logits.masked_fill(~b["action_mask"], float("-inf"))
            lp = torch.log_softmax(lg, dim=1).gather(1, b["action"].view(-1, 1)).squeeze(1)
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


_LO_FIELDS = ("obs", "zone_obs", "goal", "action", "log_prob", "value", "advantage", "returnn")
_HI_FIELDS = ("obs", "zone_obs", "value", "log_prob", "advantage", "returnn")


def lo_batch(lo, idx, dtype):
    """lo: name -> array [N, T-1, ...] (ZoneVecEnv.collect_hier); idx: flat [N][T-1] sample indexes."""
    out = {}
    for k in _LO_FIELDS:
        a = np.asarray(lo[k])
        out[k] = torch.as_tensor(a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])[np.asarray(idx, np.int64)]).to(dtype)
    return out


def hi_batch(hi, idx, dtype):
    """hi: name -> array [M, ...]; idx: row indexes."""
    idx = np.asarray(idx, np.int64)
    out = {k: torch.as_tensor(np.asarray(hi[k])[idx]).to(dtype) for k in _HI_FIELDS}
    out["action"] = torch.as_tensor(np.asarray(hi["action"])[idx].astype(np.int64))
    out["action_mask"] = torch.as_tensor(np.asarray(hi["action_mask"])[idx].astype(bool))
    return out


def synthetic_hier_experience(hi_sd, lo_sd, F, Z, N, T, M, seed=0):
    """(lo, hi) as a collect_hier would leave them, float32, from random observations: lo [N, T-1, ...], hi [M, ...]
    with 1 to Z available goals per row.  Actions, log_probs and values are the float64 networks' own at the given
    state_dicts, the advantages unit normal, returnn = value + advantage."""
    g = torch.Generator().manual_seed(3000 + seed)
    f64 = torch.float64
    n = N * (T - 1)
    obs = torch.randn((n, 8), generator=g, dtype=f64)
    zo = torch.rand((n, Z, F), generator=g, dtype=f64) * 2.0 - 1.0
    goal = torch.rand((n, 2), generator=g, dtype=f64) * 2.0 - 1.0
    with torch.no_grad():
        mu, std, v = model_from("lo", lo_sd, F, f64)(obs, zo, goal)
        action = mu + std * torch.randn(mu.shape, generator=g, dtype=f64)
        log_prob = torch.distributions.Normal(mu, std).log_prob(action)
    adv = torch.randn((n,), generator=g, dtype=f64)
    flat = dict(obs=obs, zone_obs=zo, goal=goal, action=action, log_prob=log_prob, value=v, advantage=adv,
                returnn=v + adv)
    lo = {k: a.to(torch.float32).numpy().reshape((N, T - 1) + tuple(a.shape[1:])) for k, a in flat.items()}
    obs = torch.randn((M, 8), generator=g, dtype=f64)
    zo = torch.rand((M, Z, F), generator=g, dtype=f64) * 2.0 - 1.0
    n_avail = torch.randint(1, Z + 1, (M,), generator=g)
    mask = torch.zeros((M, Z), dtype=torch.bool)
    for i in range(M):
        mask[i, torch.randperm(Z, generator=g)[:int(n_avail[i])]] = True
    with torch.no_grad():
        logits, v = model_from("hi", hi_sd, F, f64)(obs, zo)
        dist = torch.distributions.Categorical(logits=logits.masked_fill(~mask, float("-inf")))
        u = torch.rand((M,), generator=g, dtype=f64)
        a = (dist.probs.cumsum(dim=1) < u.view(-1, 1)).sum(dim=1).clamp(max=Z - 1)
        a = torch.where(mask.gather(1, a.view(-1, 1)).squeeze(1), a, mask.to(torch.int64).argmax(dim=1))
        log_prob = dist.log_prob(a)
    adv = torch.randn((M,), generator=g, dtype=f64)
    hi = dict(obs=obs.float().numpy(), zone_obs=zo.float().numpy(), action=a.to(torch.int32).numpy(),
              action_mask=mask.numpy(), value=v.float().numpy(), log_prob=log_prob.float().numpy(),
              advantage=adv.float().numpy(), returnn=(v + adv).float().numpy())
    return lo, hi


# ---- the head derivatives as the kernels form them, per sample, in numpy (any float dtype)
def _np_clipped_policy(dlp, adv, eps, inv_b):
    """-> (-min(surr1, surr2), d loss / d log_prob): clipped_policy of ppo_update.hip."""
    ratio = np.exp(dlp)
    lo, hi = 1.0 - eps, 1.0 + eps
    surr1, surr2 = ratio * adv, np.clip(ratio, lo, hi) * adv
    through = np.where(surr1 <= surr2, 1.0, np.where((ratio >= lo) & (ratio <= hi), 1.0, 0.0))
    return -np.minimum(surr1, surr2), -adv * inv_b * through * ratio


def _np_clipped_value(v, old, ret, eps, coef, inv_b):
    """-> (max(s1, s2), d loss / d v): clipped_value of ppo_update.hip."""
    dv = v - old
    vc = old + np.clip(dv, -eps, eps)
    s1, s2 = (v - ret) ** 2, (vc - ret) ** 2
    inside = (dv >= -eps) & (dv <= eps)
    dl = np.where(s1 >= s2, 2.0 * (v - ret), np.where(inside, 2.0 * (vc - ret), 0.0))
    return np.maximum(s1, s2), coef * inv_b * dl


def _np_sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gaussian_head_derivatives(pre_mu, pre_std, v, action, old_log_prob, old_value, adv, ret, hyper):
    """k_ppo_loss without the distributional critic.  pre_mu, pre_std [B, 2]: the outputs of actor.mu_ / actor.std_
    before the sigmoid; old_log_prob [B, 2] per component.  -> (d pre_mu [B, 2], d pre_std [B, 2], d v [B]) of the
    minibatch loss."""
    inv_b = 1.0 / pre_mu.shape[0]
    smu, ssd = _np_sigmoid(pre_mu), _np_sigmoid(pre_std)
    mu, sd = 2.0 * (smu - 0.5), ssd + 1e-3
    diff = action - mu
    lp = -(diff * diff) / (2.0 * (sd * sd)) - np.log(sd) - HALF_LOG_2PI
    _, g_lp = _np_clipped_policy((lp - old_log_prob).sum(axis=1), adv, hyper["clip_eps"], inv_b)
    var = sd * sd
    g_mu = g_lp[:, None] * (diff / var)
    g_sd = g_lp[:, None] * ((diff * diff) / (var * sd) - 1.0 / sd) - hyper["entropy_coef"] * (0.5 * inv_b) / sd
    _, d_v = _np_clipped_value(v, old_value, ret, hyper["clip_eps"], hyper["value_loss_coef"], inv_b)
    return g_mu * 2.0 * smu * (1.0 - smu), g_sd * ssd * (1.0 - ssd), d_v


def categorical_head_derivatives(logits, mask, action, old_log_prob, v, old_value, adv, ret, hyper):
    """k_hppo_loss.  logits [B, Z] raw, mask [B, Z] bool, action [B].  With p the masked softmax and H the row's
    entropy: d logit_z = g_lp (1[z = a] - p_z) + (entropy_coef / B) p_z (log p_z + H), 0 where z is unavailable.
    -> (d logits [B, Z], d v [B])."""
    B = logits.shape[0]
    inv_b = 1.0 / B
    d = np.zeros_like(logits)
    dlp = np.zeros(B, logits.dtype)
    rows = []
    for i in range(B):
        z = np.nonzero(mask[i])[0]
        lg = logits[i, z]
        m = lg.max()
        lp = lg - (m + np.log(np.exp(lg - m).sum()))
        rows.append((z, lp, -(np.exp(lp) * lp).sum()))
        dlp[i] = lp[list(z).index(int(action[i]))] - old_log_prob[i]
    _, g_lp = _np_clipped_policy(dlp, adv, hyper["clip_eps"], inv_b)
    for i, (z, lp, ent) in enumerate(rows):
        p = np.exp(lp)
        d[i, z] = g_lp[i] * ((z == int(action[i])) - p) + hyper["entropy_coef"] * inv_b * p * (lp + ent)
    _, d_v = _np_clipped_value(v, old_value, ret, hyper["clip_eps"], hyper["value_loss_coef"], inv_b)
    return d, d_v
