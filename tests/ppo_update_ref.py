"""The flat actor-critic's PPO update restated for the tests of the device learner (zenv_ppo_*): this project's own
code, written from the reference's behaviour, no text of it.

  network   ACModel (main/src/flat_model.py:21-68) = ZoneEnvModel (main/src/env_model.py:48-79) + PolicyNetwork's Box
            branch (main/src/policy_network.py:39-52) + the plain or the distributional critic, as torch modules of any
            dtype under the reference's state_dict names; gradients come from torch autograd
  loss      update_parameters' sub-batch body for recurrence 1 (main/src/torch_ac/algos/ppo.py:68-100)
  clip      the norm of ppo.py:121 and clip_grad_norm_ (:122), as arithmetic
  Adam      torch.optim.Adam's step (:27, :123: betas 0.9 / 0.999, no weight decay, no amsgrad), as arithmetic
  indexes   _get_batches_starting_indexes (:157-183) for recurrence 1

The float64 run of this code is the truth; the float32 run of the same code on the CPU is the ruler for rounding
(``check_rule``): a device result may deviate from the truth by 8 times what float32 torch does, or by 8 ulp at the
tensor's scale, whichever is larger.
"""
import math

import numpy as np
import torch
import torch.nn as nn

HYPER = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=0.5)
STATS = ("entropy", "value", "value_std", "policy_loss", "value_loss", "grad_norm")
# the clipped-branch condition (test_ppo_update_ref_cpu.py): parameters theta + SCALE * N(0, 1) * |theta| from this seed
PERTURB_SEED, PERTURB_SCALE = 11, 0.05
PERTURB_CLIP_EPS = 0.02


class ACModelRef(nn.Module):
    def __init__(self, F, h, distributional=False, dtype=torch.float64):
        super().__init__()
        self.distributional = distributional
        env = nn.Module()
        env.zone_net_ = nn.Sequential(nn.Linear(8 + F, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h))
        env.combine_net_ = nn.Linear(8 + h, h)
        self.env_model = env
        actor = nn.Module()
        actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h, h), nn.ReLU()))
        actor.mu_ = nn.Linear(h, 2)
        actor.std_ = nn.Linear(h, 2)
        self.actor = actor
        if distributional:                                   # flat_model.py:34-40
            self.critic = nn.Sequential(nn.Linear(h, h), nn.ReLU())
            self.critic_mu = nn.Linear(h, 1)
            self.critic_sigma = nn.Linear(h, 1)
        else:                                                # :43-47
            self.critic = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))
        self.to(dtype)

    def forward(self, obs, zone_obs):
        Z = zone_obs.shape[1]
        x = torch.cat([obs.unsqueeze(1).expand(-1, Z, -1), zone_obs], dim=-1)
        zone_emb = self.env_model.zone_net_(x).sum(dim=1) / Z                  # env_model.py:77
        emb = self.env_model.combine_net_(torch.cat([obs, zone_emb], dim=-1))
        a = self.actor.enc_(emb)
        mu = 2.0 * (torch.sigmoid(self.actor.mu_(a)) - 0.5)                     # policy_network.py:46-48
        std = torch.sigmoid(self.actor.std_(a)) + 1e-3
        if self.distributional:
            c = self.critic(emb)
            v = self.critic_mu(c).squeeze(1)
            sigma = nn.functional.softplus(self.critic_sigma(c), beta=0.3).squeeze(1) + 1e-3
            return mu, std, v, sigma
        return mu, std, self.critic(emb).squeeze(1), None


def random_state_dict(F, h, distributional=False, seed=0):
    """A float32 state_dict as init_params leaves the weights (unit-norm rows, flat_model.py:12-18), with small random
    biases so that no bias gradient is tested at a special point."""
    g = torch.Generator().manual_seed(1000 + seed)
    model = ACModelRef(F, h, distributional, torch.float32)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g))
                m.weight.div_(m.weight.pow(2).sum(1, keepdim=True).sqrt())
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return {k: v.clone() for k, v in model.state_dict().items()}


def perturbed(state_dict, seed=PERTURB_SEED, scale=PERTURB_SCALE):
    g = torch.Generator().manual_seed(seed)
    return {k: (v + scale * torch.randn(v.shape, generator=g) * v.abs()).to(v.dtype) for k, v in state_dict.items()}


def model_from(state_dict, F, dtype):
    h = state_dict["env_model.zone_net_.0.bias"].shape[0]
    model = ACModelRef(F, h, "critic_sigma.weight" in state_dict, dtype)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state_dict.items()})
    return model


def as_batch(exps, idx, dtype):
    """exps: name -> array [N, T, ...] (ZoneVecEnv.collect); idx: flat [N][T] sample indexes (base.py:212-227)."""
    out = {}
    for k in ("obs", "zone_obs", "action", "log_prob", "value", "advantage", "returnn"):
        a = np.asarray(exps[k])
        flat = a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])
        out[k] = torch.as_tensor(flat[np.asarray(idx, np.int64)]).to(dtype)
    return out


def branches(model, b, clip_eps):
    """Which samples take a clipped branch: (policy, ratio above the range), (policy, below), (value)."""
    with torch.no_grad():
        mu, std, v, sigma = model(b["obs"], b["zone_obs"])
        ratio = torch.exp((torch.distributions.Normal(mu, std).log_prob(b["action"]) - b["log_prob"]).sum(dim=1))
        hi = (ratio > 1.0 + clip_eps) & (b["advantage"] > 0)
        lo = (ratio < 1.0 - clip_eps) & (b["advantage"] < 0)
        dv = v - b["value"]
        vc = b["value"] + dv.clamp(-clip_eps, clip_eps)
        val = (dv.abs() > clip_eps) & ((vc - b["returnn"]).pow(2) > (v - b["returnn"]).pow(2))
    return hi, lo, val


def loss_and_stats(model, b, hyper):
    """ppo.py:68-100 for one sub-batch: the loss (a tensor) and the five logged means."""
    mu, std, v, sigma = model(b["obs"], b["zone_obs"])
    dist = torch.distributions.Normal(mu, std)
    entropy = dist.entropy().mean()
    ratio = torch.exp((dist.log_prob(b["action"]) - b["log_prob"]).sum(dim=1))
    eps = hyper["clip_eps"]
    surr1 = ratio * b["advantage"]
    surr2 = torch.clamp(ratio, 1.0 - eps, 1.0 + eps) * b["advantage"]
    policy_loss = -torch.min(surr1, surr2).mean()
    if model.distributional:
        value_loss = -torch.distributions.Normal(v, sigma).log_prob(b["returnn"]).mean()
    else:
        clipped = b["value"] + torch.clamp(v - b["value"], -eps, eps)
        value_loss = torch.max((v - b["returnn"]).pow(2), (clipped - b["returnn"]).pow(2)).mean()
    loss = policy_loss - hyper["entropy_coef"] * entropy + hyper["value_loss_coef"] * value_loss
    stats = {"entropy": entropy.item(), "value": v.mean().item(),
             "value_std": sigma.mean().item() if model.distributional else 0.0,
             "policy_loss": policy_loss.item(), "value_loss": value_loss.item()}
    outputs = {"mu": mu.detach(), "std": std.detach(), "value": v.detach()}
    return loss, stats, outputs


def gradients(model, b, hyper):
    """state_dict key -> gradient of the loss, and the statistics with the norm of ppo.py:121."""
    model.zero_grad()
    loss, stats, _ = loss_and_stats(model, b, hyper)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    stats["grad_norm"] = total_norm(grads.values())
    return grads, stats


def total_norm(grads):
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))


def clip_coef(norm, max_norm):
    """clip_grad_norm_: every gradient is multiplied by min(1, max_norm / (norm + 1e-6))."""
    return min(1.0, max_norm / (norm + 1e-6))


def adam_step(p, g, m, v, step, lr, eps, beta1=0.9, beta2=0.999):
    """One step of torch.optim.Adam on float64 arrays, in place; step counts from 1."""
    m *= beta1
    m += (1.0 - beta1) * g
    v *= beta2
    v += (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p -= (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)


def batch_indexes(num_frames, frames_per_proc, batch_num, rng):
    """The index order of one epoch for recurrence 1: a permutation of all frames; on an odd batch_num the frames at
    the end of a rollout ((i + 1) % T == 0) are dropped, and the shift recurrence // 2 is 0."""
    idx = rng.permutation(np.arange(num_frames))
    if batch_num % 2:
        idx = idx[(idx + 1) % frames_per_proc != 0]
    return idx.astype(np.int32)


class RefLearner:
    """update_parameters' inner loop in a dtype: autograd gradients, the clip, torch's own Adam."""

    def __init__(self, state_dict, F, dtype, hyper):
        self.model = model_from(state_dict, F, dtype)
        self.hyper = hyper
        self.opt = torch.optim.Adam(self.model.parameters(), hyper["lr"], eps=hyper["adam_eps"], foreach=False)

    def minibatch(self, batch):
        grads, stats = gradients(self.model, batch, self.hyper)
        nn.utils.clip_grad_norm_(self.model.parameters(), self.hyper["max_grad_norm"], foreach=False)
        self.opt.step()
        return [stats[k] for k in STATS]


def check_rule(name, dev, ref64, ref32, report=None):
    """The tolerance rule: e_dev <= 8 max(e32, 2^-24 max|ref|) in the max norm.  Returns e_dev / that bound's base."""
    ref64 = np.asarray(ref64, np.float64)
    e32 = float(np.max(np.abs(np.asarray(ref32, np.float64) - ref64))) if ref64.size else 0.0
    e_dev = float(np.max(np.abs(np.asarray(dev, np.float64) - ref64))) if ref64.size else 0.0
    base = max(e32, 2.0 ** -24 * (float(np.max(np.abs(ref64))) if ref64.size else 0.0))
    ratio = e_dev / base if base > 0 else (0.0 if e_dev == 0 else math.inf)
    if report is not None:
        report.append((name, e_dev, e32, ratio))
    print(f"rule {name}: e_dev {e_dev:.3e} e32 {e32:.3e} ratio {ratio:.2f}")
    assert np.all(np.isfinite(np.asarray(dev))), name
    assert e_dev <= 8.0 * base, f"{name}: e_dev {e_dev:.3e} > 8 x max(e32 {e32:.3e}, ulp) = {8.0 * base:.3e}"
    return ratio


def synthetic_experience(state_dict, F, Z, N, T, seed=0):
    """exps.* as a collect would leave them ([N, T, ...] float32), from random observations: the actions, log_probs and
    values are the float64 network's own at `state_dict`, the advantages unit normal, returnn = value + advantage."""
    g = torch.Generator().manual_seed(2000 + seed)
    obs = torch.randn((N * T, 8), generator=g, dtype=torch.float64)
    zone_obs = torch.rand((N * T, Z, F), generator=g, dtype=torch.float64) * 2.0 - 1.0
    with torch.no_grad():
        mu, std, v, _ = model_from(state_dict, F, torch.float64)(obs, zone_obs)
        action = mu + std * torch.randn(mu.shape, generator=g, dtype=torch.float64)
        log_prob = torch.distributions.Normal(mu, std).log_prob(action)
    adv = torch.randn((N * T,), generator=g, dtype=torch.float64)
    flat = dict(obs=obs, zone_obs=zone_obs, action=action, log_prob=log_prob, value=v, advantage=adv, returnn=v + adv)
    return {k: a.to(torch.float32).numpy().reshape((N, T) + tuple(a.shape[1:])) for k, a in flat.items()}
