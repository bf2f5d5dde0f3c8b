"""Options training on the device env: experience collection by ``zenv_collect_option`` (the skill picks, the low level's
action with its termination component, the env step, the semi-Markov high-level transitions and both GAE recursions in
HIP kernels), the two PPO updates in plain PyTorch on the same device and stream.

This is the loop of the reference's Options agent (options/src/torch_ac/algos/hrl_policy_planner.py with
_hier_policy_opt.py: collect_experiences, update_lo_parameters, update_hi_parameters) with ``ParallelEnv`` and the host
loop replaced by ``TorchZoneEnv.collect_options``.  The modules carry the reference's parameter names
(options/src/hier_policy_value_models.py; restated in tests/option_ref.py), so their state_dicts are the checkpoint's;
after every update the device agent is reloaded from them.  Reloading drops the transitions the last collection left
open: an option that is still running when a collection ends is not trained on, its skill is picked again.

    python examples/options_ppo_torch.py --env PointTSP-v0 --procs 4096 --frames-per-proc 100

``--device-update`` runs both levels' updates in the library as well (``TorchZoneEnv.opppo_init`` / ``opppo_update`` /
``opppo_publish``: zenv_opppo_*, csrc/ppo_update.hip).  ``opppo_publish`` reloads the device agent as the torch path's
reload does, open transitions dropped alike.  Off by default, the torch path is what it was.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Categorical, Normal

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import combinatorial_rl_tasks_amd as Z  # noqa: E402
from combinatorial_rl_tasks_amd.agents import episode_log_history  # noqa: E402
from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv  # noqa: E402


class _ZoneEncoder(nn.Module):
    """ZoneEnvModel (x = obs) / ZoneEnvSkillModel (x = [obs, onehot]): shared MLP over [x, zone row], mean, combine."""

    def __init__(self, x_dim, zone_feat, h):
        super().__init__()
        self.zone_net_ = nn.Sequential(nn.Linear(x_dim + zone_feat, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(),
                                       nn.Linear(h, h))
        self.combine_net_ = nn.Linear(x_dim + h, h)

    def forward(self, x, zone_obs):
        n_zones = zone_obs.shape[1]
        rows = torch.cat([x.unsqueeze(1).expand(-1, n_zones, -1), zone_obs], dim=-1)
        return self.combine_net_(torch.cat([x, self.zone_net_(rows).mean(dim=1)], dim=-1))


def _init_params(module):               # unit-norm rows, zero bias (hier_policy_value_models.py init_params)
    for m in module.modules():
        if isinstance(m, nn.Linear):
            with torch.no_grad():
                m.weight.normal_(0, 1)
                m.weight /= m.weight.pow(2).sum(1, keepdim=True).sqrt()
                m.bias.zero_()


class HighPolicyValueModel(nn.Module):
    """The high level: Categorical over the S skills and the value, from ZoneEnvModel's embedding."""

    def __init__(self, zone_feat, n_skills, h=128):
        super().__init__()
        self.env_model = _ZoneEncoder(8, zone_feat, h)
        self.actor = nn.Module()
        self.actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h, h), nn.ReLU()))
        self.actor.discrete_ = nn.Sequential(nn.Linear(h, n_skills))
        self.critic = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))
        _init_params(self)

    def forward(self, obs, zone_obs):
        emb = self.env_model(obs, zone_obs)
        logits = self.actor.discrete_(self.actor.enc_(emb))
        return Categorical(logits=F.log_softmax(logits, dim=1)), self.critic(emb).squeeze(1)


class LoPolicyValueModel(nn.Module):
    """The low level: Normal(mu, std) over three components -- the action's two and the one whose sample a_2 ends the
    option with probability sigmoid(4 a_2 - 3) -- and the value, from [obs, onehot(skill)] and the zone rows."""

    def __init__(self, zone_feat, n_skills, h=128):
        super().__init__()
        self.n_skills = n_skills
        self.env_model = _ZoneEncoder(8 + n_skills, zone_feat, h)
        self.actor = nn.Module()
        self.actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h + n_skills, h), nn.ReLU()))
        self.actor.mu_ = nn.Linear(h, 3)
        self.actor.std_ = nn.Linear(h, 3)
        self.critic = nn.Sequential(nn.Linear(h + n_skills, h), nn.ReLU(), nn.Linear(h, 1))
        _init_params(self)

    def forward(self, obs, zone_obs, skill):
        onehot = F.one_hot(skill.long(), self.n_skills).to(obs.dtype)
        x = torch.cat([self.env_model(torch.cat([obs, onehot], dim=-1), zone_obs), onehot], dim=-1)
        a = self.actor.enc_(x)
        dist = Normal(2.0 * (torch.sigmoid(self.actor.mu_(a)) - 0.5), torch.sigmoid(self.actor.std_(a)) + 1e-3)
        return dist, self.critic(x).squeeze(1)


def _ppo_loss(log_prob, old_log_prob, value, sb, clip_eps):
    ratio = torch.exp(log_prob - old_log_prob)
    adv = sb["advantage"]
    policy_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_eps, 1.0 + clip_eps) * adv).mean()
    v_clip = sb["value"] + torch.clamp(value - sb["value"], -clip_eps, clip_eps)
    value_loss = torch.max((value - sb["returnn"]).pow(2), (v_clip - sb["returnn"]).pow(2)).mean()
    return policy_loss, value_loss


class OptionsPPO:
    """One iteration of the Options agent: collect_experiences on the device, then the two updates of
    _hier_policy_opt.py:227-381 in torch -- the high level's PPO on the closed transitions, the low level's on the
    T - 1 frames of every env, its ratio over all three components of the action.  With device_update both run in the
    library (``opppo_init`` once; then ``collect_options``, ``opppo_update``, ``opppo_publish`` per iteration, and the
    modules get the learners' parameters back after every update)."""

    def __init__(self, tenv, n_skills=5, h=128, frames_per_proc=100, epochs=4, batch_size=16384, hi_epochs=4,
                 hi_batch_size=4096, lr=3e-4, hi_lr=3e-4, discount=0.99, gae_lambda=0.95, clip_eps=0.2,
                 entropy_coef=0.003, hi_entropy_coef=0.01, value_loss_coef=0.5, hi_value_coef=0.5, seed=1,
                 device_update=False):
        self.tenv, self.S, self.T = tenv, n_skills, frames_per_proc
        dev, F_ = tenv.device, tenv.env.zone_feat
        self.hi_net = HighPolicyValueModel(F_, n_skills, h).to(dev)
        self.lo_net = LoPolicyValueModel(F_, n_skills, h).to(dev)
        self.epochs, self.batch_size, self.hi_epochs, self.hi_batch_size = epochs, batch_size, hi_epochs, hi_batch_size
        self.discount, self.gae_lambda, self.clip_eps = discount, gae_lambda, clip_eps
        self.entropy_coef, self.hi_entropy_coef = entropy_coef, hi_entropy_coef
        self.value_loss_coef, self.hi_value_coef = value_loss_coef, hi_value_coef
        self.lo_optimizer = torch.optim.Adam(self.lo_net.parameters(), lr, eps=1e-8)
        self.hi_optimizer = torch.optim.Adam(self.hi_net.parameters(), hi_lr, eps=1e-8)
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self.seed, self.it = seed, 0
        self.device_update = device_update
        if device_update:
            self.rng = np.random.default_rng(seed)
            tenv.opppo_init(self.hi_net.state_dict(), self.lo_net.state_dict(),
                            lo=dict(lr=lr, clip_eps=clip_eps, entropy_coef=entropy_coef, value_loss_coef=value_loss_coef,
                                    max_batch=batch_size),
                            hi=dict(lr=hi_lr, clip_eps=clip_eps, entropy_coef=hi_entropy_coef,
                                    value_loss_coef=hi_value_coef, max_batch=hi_batch_size))
            tenv.opppo_publish()

    def _batches(self, total, size):
        order = torch.randperm(total, device=self.tenv.device, generator=self.gen)
        return [order[i:i + size] for i in range(0, total, size)]

    def collect(self):
        """Reload the device agent from the modules (device_update: opppo_publish has), collect; (lo, hi,
        termination_rate) of TorchZoneEnv."""
        if not self.device_update:
            self.tenv.load_options(self.hi_net.state_dict(), self.lo_net.state_dict())
        out = self.tenv.collect_options(self.T, policy_seed=self.seed * 1000003 + self.it, discount=self.discount,
                                        gae_lambda=self.gae_lambda)
        self.it += 1
        return out

    def update_lo_parameters(self, lo):
        flat = {k: v.reshape((-1,) + tuple(v.shape[2:])) for k, v in lo.items()}
        action = torch.cat([flat["action"], flat["term_action"].unsqueeze(1)], dim=1)           # the reference's _action
        old_log_prob = torch.cat([flat["log_prob"], flat["term_log_prob"].unsqueeze(1)], dim=1).sum(1)
        stats = {}
        for _ in range(self.epochs):
            for idx in self._batches(action.shape[0], self.batch_size):
                sb = {k: flat[k][idx] for k in ("obs", "zone_obs", "skill", "value", "advantage", "returnn")}
                dist, value = self.lo_net(sb["obs"], sb["zone_obs"], sb["skill"])
                entropy = dist.entropy().mean()
                policy_loss, value_loss = _ppo_loss(dist.log_prob(action[idx]).sum(1), old_log_prob[idx], value, sb,
                                                    self.clip_eps)
                loss = policy_loss - self.entropy_coef * entropy + self.value_loss_coef * value_loss
                self.lo_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self.lo_optimizer.step()
                stats = {"policy_loss": policy_loss, "value_loss": value_loss, "entropy": entropy}
        return {k: float(v.detach()) for k, v in stats.items()}

    def update_hi_parameters(self, hi):
        stats = {}
        action = hi["action"].long()
        for _ in range(self.hi_epochs):
            for idx in self._batches(action.shape[0], self.hi_batch_size):
                sb = {k: hi[k][idx] for k in ("obs", "zone_obs", "value", "advantage", "returnn", "log_prob")}
                dist, value = self.hi_net(sb["obs"], sb["zone_obs"])
                entropy = dist.entropy().mean()
                policy_loss, value_loss = _ppo_loss(dist.log_prob(action[idx]), sb["log_prob"], value, sb,
                                                    self.clip_eps)
                loss = policy_loss - self.hi_entropy_coef * entropy + self.hi_value_coef * value_loss
                self.hi_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self.hi_optimizer.step()
                stats = {"policy_loss": policy_loss, "value_loss": value_loss, "entropy": entropy}
        return {k: float(v.detach()) for k, v in stats.items()}

    def update(self, lo, hi):
        """Both updates on one collection (before the next collect overwrites its buffers); the high level's only when
        some transition closed."""
        if self.device_update:
            logs = self.tenv.opppo_update(self.epochs, self.batch_size, self.hi_epochs, self.hi_batch_size, self.rng)
            self.tenv.opppo_publish()
            hi_sd, lo_sd = self.tenv.opppo_state_dicts()  # the modules follow the learners
            self.hi_net.load_state_dict(hi_sd)
            self.lo_net.load_state_dict(lo_sd)
            return logs
        logs = {}
        if hi["action"].shape[0]:
            logs.update({"hi_" + k: v for k, v in self.update_hi_parameters(hi).items()})
        logs.update({"lo_" + k: v for k, v in self.update_lo_parameters(lo).items()})
        return logs

    def iteration(self):
        lo, hi, rate = self.collect()
        logs = {"num_frames_hi": int(hi["action"].shape[0]), "termination_rate": float(rate),
                "reward_per_frame": float(lo["env_reward"].mean())}
        num_frames = self.tenv.episode_logs()["num_frames"]      # logs of collect_experiences, synthesized
        logs.update(episode_log_history(self.tenv.episode_log_stats(), num_frames))
        logs.update(self.update(lo, hi))
        return logs


def train(env_id="PointTSP-v0", procs=4096, frames_per_proc=100, updates=10, n_skills=5, hidden=128, seed=1, log=print,
          device_update=False, **kw):
    torch.manual_seed(seed)
    env = Z.ZoneVecEnv(env_id, procs)
    env.build_bank(seed, 4 * procs)
    env.schedule_sequential(stride=procs)
    tenv = TorchZoneEnv(env)
    tenv.reset()
    algo = OptionsPPO(tenv, n_skills, hidden, frames_per_proc, seed=seed, device_update=device_update, **kw)
    for u in range(updates):
        t0 = time.perf_counter()
        logs = algo.iteration()
        torch.cuda.synchronize()
        logs.update(update=u, seconds=round(time.perf_counter() - t0, 3))
        log({k: (round(v, 4) if isinstance(v, float) else v) for k, v in logs.items()})
    env.close()
    return algo


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="PointTSP-v0")
    ap.add_argument("--procs", type=int, default=4096)
    ap.add_argument("--frames-per-proc", type=int, default=100)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--n-skills", type=int, default=5)
    ap.add_argument("--hidden-size", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device-update", action="store_true",
                    help="run both levels' PPO updates in the library (zenv_opppo_*) instead of torch")
    a = ap.parse_args()
    train(a.env, a.procs, a.frames_per_proc, a.updates, a.n_skills, a.hidden_size, a.seed, device_update=a.device_update)
