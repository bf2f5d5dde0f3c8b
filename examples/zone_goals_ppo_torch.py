"""Zone-goals training on the device env: experience collection by ``zenv_collect_hier`` (the high level's goal pick,
the low level's action, the env step, the semi-Markov bookkeeping and both GAE recursions in HIP kernels), the two PPO
updates in plain PyTorch on the same device and stream.

This is the loop of the reference's HierPolicyAlgo (zone-goals/src/torch_ac/algos/hrl_policy_planner.py with
_hier_policy_opt.py: collect_experiences, update_lo_parameters, update_hi_parameters) with ``ParallelEnv`` and the host
loop replaced by ``TorchZoneEnv.collect_hier``.  ``HighPolicyValueModel`` / ``LoPolicyValueModel`` carry the reference's
parameter names (zone-goals/src/hier_policy_value_models.py, restated in tests/hier_ref.py), so their state_dicts are
the checkpoint's hi_model_state / lo_model_state; after every update the device agent is reloaded from them.

    python examples/zone_goals_ppo_torch.py --env PointTSP-v0 --procs 4096 --frames-per-proc 128 --updates 10

``--device-update`` runs the two updates in the library as well (``TorchZoneEnv.hppo_init`` / ``hppo_update`` /
``hppo_publish``: zenv_hppo_*, csrc/ppo_update.hip); off by default, the torch path is what it was.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Categorical

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import combinatorial_rl_tasks_amd as Z  # noqa: E402
from combinatorial_rl_tasks_amd.agents import episode_log_history  # noqa: E402
from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv  # noqa: E402


class _ZoneEncoder(nn.Module):
    """ZoneEnvModel (x = obs) / ZoneEnvGoalModel (x = [obs, goal]): shared MLP over [x, zone row], mean, combine."""

    def __init__(self, x_dim, zone_feat, h):
        super().__init__()
        self.zone_net_ = nn.Sequential(nn.Linear(x_dim + zone_feat, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(),
                                       nn.Linear(h, h))
        self.combine_net_ = nn.Linear(x_dim + h, h)

    def forward(self, x, zone_obs):
        n_zones = zone_obs.shape[1]
        rows = torch.cat([x.unsqueeze(1).expand(-1, n_zones, -1), zone_obs], dim=-1)
        return self.combine_net_(torch.cat([x, self.zone_net_(rows).mean(dim=1)], dim=-1))


def _init_params(module):               # hier_policy_value_models.py init_params: unit-norm rows, zero bias
    for m in module.modules():
        if isinstance(m, nn.Linear):
            with torch.no_grad():
                m.weight.normal_(0, 1)
                m.weight /= m.weight.pow(2).sum(1, keepdim=True).sqrt()
                m.bias.zero_()


class HighPolicyValueModel(nn.Module):
    """The high level: one logit per zone from [emb, zone row], and the value of emb."""

    def __init__(self, zone_feat, h=128):
        super().__init__()
        self.env_model = _ZoneEncoder(8, zone_feat, h)
        self.actor = nn.Sequential(nn.Linear(h + zone_feat, h), nn.ReLU(), nn.Linear(h, 1))
        self.critic = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))
        _init_params(self)

    def forward(self, obs, zone_obs):
        emb = self.env_model(obs, zone_obs)
        n_zones = zone_obs.shape[1]
        logits = self.actor(torch.cat([emb.unsqueeze(1).expand(-1, n_zones, -1), zone_obs], dim=-1)).squeeze(-1)
        return logits, self.critic(emb).squeeze(1)


class LoPolicyValueModel(nn.Module):
    """The low level: Normal(mu, std) over the action and the value, from [obs, goal] and the zone rows."""

    def __init__(self, zone_feat, h=128):
        super().__init__()
        self.env_model = _ZoneEncoder(10, zone_feat, h)
        self.actor = nn.Module()
        self.actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h, h), nn.ReLU()))
        self.actor.mu_ = nn.Linear(h, 2)
        self.actor.std_ = nn.Linear(h, 2)
        self.critic = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))
        _init_params(self)

    def forward(self, obs, zone_obs, goal):
        emb = self.env_model(torch.cat([obs, goal], dim=-1), zone_obs)
        a = self.actor.enc_(emb)
        dist = torch.distributions.Normal(2.0 * (torch.sigmoid(self.actor.mu_(a)) - 0.5),
                                          torch.sigmoid(self.actor.std_(a)) + 1e-3)
        return dist, self.critic(emb).squeeze(1)


def _ppo_loss(log_prob, old_log_prob, value, sb, clip_eps):
    ratio = torch.exp(log_prob - old_log_prob)
    adv = sb["advantage"]
    policy_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_eps, 1.0 + clip_eps) * adv).mean()
    v_clip = sb["value"] + torch.clamp(value - sb["value"], -clip_eps, clip_eps)
    value_loss = torch.max((value - sb["returnn"]).pow(2), (v_clip - sb["returnn"]).pow(2)).mean()
    return policy_loss, value_loss


class HierPPO:
    """HierPolicyAlgo's iteration: collect_experiences on the device, then update_hi_parameters and
    update_lo_parameters (_hier_policy_opt.py:196-330) in torch -- or, with device_update, both updates in the library
    too (``hppo_init`` once; then ``collect_hier``, ``hppo_update``, ``hppo_publish`` per iteration; hi_net / lo_net get
    the learners' parameters back when ``train`` ends)."""

    def __init__(self, tenv, hi_net, lo_net, frames_per_proc=128, epochs=4, batch_size=16384, hi_epochs=4,
                 hi_batch_size=4096, lr=3e-4, hi_lr=3e-4, discount=0.99, gae_lambda=0.95, clip_eps=0.2,
                 entropy_coef=0.003, hi_entropy_coef=0.01, value_loss_coef=0.5, hi_value_coef=0.5, seed=1,
                 device_update=False):
        self.tenv, self.hi_net, self.lo_net = tenv, hi_net, lo_net
        self.T, self.epochs, self.batch_size = frames_per_proc, epochs, batch_size
        self.hi_epochs, self.hi_batch_size = hi_epochs, hi_batch_size
        self.discount, self.gae_lambda, self.clip_eps = discount, gae_lambda, clip_eps
        self.entropy_coef, self.hi_entropy_coef = entropy_coef, hi_entropy_coef
        self.value_loss_coef, self.hi_value_coef = value_loss_coef, hi_value_coef
        self.lo_optimizer = torch.optim.Adam(lo_net.parameters(), lr, eps=1e-8)
        self.hi_optimizer = torch.optim.Adam(hi_net.parameters(), hi_lr, eps=1e-8)
        self.gen = torch.Generator(device=tenv.device).manual_seed(seed)
        self.seed, self.it = seed, 0
        self.device_update = device_update
        if device_update:
            self.rng = np.random.default_rng(seed)
            tenv.hppo_init(hi_net.state_dict(), lo_net.state_dict(),
                           lo=dict(lr=lr, clip_eps=clip_eps, entropy_coef=entropy_coef, value_loss_coef=value_loss_coef,
                                   max_batch=batch_size),
                           hi=dict(lr=hi_lr, clip_eps=clip_eps, entropy_coef=hi_entropy_coef,
                                   value_loss_coef=hi_value_coef, max_batch=hi_batch_size))
            tenv.hppo_publish()

    def _batches(self, total, size):
        order = torch.randperm(total, device=self.tenv.device, generator=self.gen)
        return [order[i:i + size] for i in range(0, total, size)]

    def update_lo_parameters(self, lo):
        flat = {k: v.reshape((-1,) + tuple(v.shape[2:])) for k, v in lo.items()}
        stats = {}
        for _ in range(self.epochs):
            for idx in self._batches(flat["obs"].shape[0], self.batch_size):
                sb = {k: v[idx] for k, v in flat.items()}
                dist, value = self.lo_net(sb["obs"], sb["zone_obs"], sb["goal"])
                entropy = dist.entropy().mean()
                policy_loss, value_loss = _ppo_loss(dist.log_prob(sb["action"]).sum(1), sb["log_prob"].sum(1), value,
                                                    sb, self.clip_eps)
                loss = policy_loss - self.entropy_coef * entropy + self.value_loss_coef * value_loss
                self.lo_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self.lo_optimizer.step()
                stats = {"policy_loss": policy_loss, "value_loss": value_loss, "entropy": entropy}
        return {k: float(v.detach()) for k, v in stats.items()}

    def update_hi_parameters(self, hi):
        stats = {}
        total = hi["action"].shape[0]
        if total == 0:
            return {"policy_loss": 0.0, "value_loss": 0.0, "entropy": 0.0}
        action = hi["action"].long()
        for _ in range(self.hi_epochs):
            for idx in self._batches(total, self.hi_batch_size):
                sb = {k: v[idx] for k, v in hi.items() if k != "count"}
                logits, value = self.hi_net(sb["obs"], sb["zone_obs"])
                logits = logits.masked_fill(~sb["action_mask"], float("-inf"))    # dist.logits[~action_mask] = -inf
                dist = Categorical(logits=logits)
                entropy = dist.entropy().mean()
                policy_loss, value_loss = _ppo_loss(dist.log_prob(action[idx]), sb["log_prob"], value, sb,
                                                    self.clip_eps)
                loss = policy_loss - self.hi_entropy_coef * entropy + self.hi_value_coef * value_loss
                self.hi_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self.hi_optimizer.step()
                stats = {"policy_loss": policy_loss, "value_loss": value_loss, "entropy": entropy}
        return {k: float(v.detach()) for k, v in stats.items()}

    def iteration(self):
        """Reload the device agent, collect, update both levels; returns the logs (lo_* / hi_*)."""
        if not self.device_update:
            self.tenv.load_hier(self.hi_net.state_dict(), self.lo_net.state_dict())
        lo, hi = self.tenv.collect_hier(self.T, policy_seed=self.seed * 1000003 + self.it, discount=self.discount,
                                        gae_lambda=self.gae_lambda)
        self.it += 1
        logs = {"frames": lo["obs"].shape[0] * lo["obs"].shape[1], "hi_frames": int(hi["action"].shape[0]),
                "reward_per_frame": float(lo["env_reward"].mean())}
        num_frames = self.tenv.episode_logs()["num_frames"]      # logs of collect_experiences, synthesized
        logs.update(episode_log_history(self.tenv.episode_log_stats(), num_frames))
        if self.device_update:
            logs.update(self.tenv.hppo_update(self.epochs, self.batch_size, self.hi_epochs, self.hi_batch_size, self.rng))
            self.tenv.hppo_publish()
            return logs
        logs.update({"hi_" + k: v for k, v in self.update_hi_parameters(hi).items()})
        logs.update({"lo_" + k: v for k, v in self.update_lo_parameters(lo).items()})
        return logs


def train(env_id="PointTSP-v0", procs=4096, frames_per_proc=128, updates=10, hidden=128, seed=1, log=print, **kw):
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    env = Z.ZoneVecEnv(env_id, procs)
    env.build_bank(seed, 4 * procs)
    env.schedule_sequential(stride=procs)
    env.enable_goals()
    tenv = TorchZoneEnv(env)
    tenv.reset()
    hi_net = HighPolicyValueModel(env.zone_feat, hidden).to(dev)
    lo_net = LoPolicyValueModel(env.zone_feat, hidden).to(dev)
    algo = HierPPO(tenv, hi_net, lo_net, frames_per_proc=frames_per_proc, seed=seed, **kw)
    for u in range(updates):
        t0 = time.perf_counter()
        logs = algo.iteration()
        torch.cuda.synchronize()
        logs.update(update=u, seconds=round(time.perf_counter() - t0, 3))
        log({k: (round(v, 4) if isinstance(v, float) else v) for k, v in logs.items()})
    if algo.device_update:
        hi_sd, lo_sd = tenv.hppo_state_dicts()
        hi_net.load_state_dict(hi_sd)
        lo_net.load_state_dict(lo_sd)
    env.close()
    return hi_net, lo_net


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="PointTSP-v0")
    ap.add_argument("--procs", type=int, default=4096)
    ap.add_argument("--frames-per-proc", type=int, default=128)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--hidden-size", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device-update", action="store_true",
                    help="run both PPO updates in the library (zenv_hppo_*) instead of torch")
    a = ap.parse_args()
    train(a.env, a.procs, a.frames_per_proc, a.updates, a.hidden_size, a.seed, device_update=a.device_update)
