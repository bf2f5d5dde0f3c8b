"""xy-goals training on the device env: experience collection by ``zenv_collect_xy`` (the goal picks, the low level's
action, the env step with the idle no-op, the distance-to-goal reward and both GAE recursions in HIP kernels), the two
updates in plain PyTorch on the same device and stream.

This is the loop of the reference's xy-goals agent (xy-goals/src/torch_ac/algos/hrl_policy_planner.py with
_hier_policy_opt.py: collect_experiences, update_hi_parameters, update_lo_parameters) with ``ParallelEnv`` and the host
loop replaced by ``TorchZoneEnv.collect_xy``.  The modules carry the reference's parameter names
(xy-goals/src/hier_policy_value_models.py; restated in tests/xy_ref.py), so their state_dicts are the checkpoint's;
after every update the device agent is reloaded from them.

    python examples/xy_goals_ppo_torch.py --env PointTSP-v0 --procs 4096 --skill-len 20 --frames-per-proc 100

``--device-update`` runs the two updates in the library as well (``TorchZoneEnv.xyppo_init`` / ``xyppo_update`` /
``xyppo_publish``: zenv_xyppo_*, csrc/ppo_update.hip); off by default, the torch path is what it was.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Normal

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


def _init_params(module):               # unit-norm rows, zero bias (hier_policy_value_models.py init_params)
    for m in module.modules():
        if isinstance(m, nn.Linear):
            with torch.no_grad():
                m.weight.normal_(0, 1)
                m.weight /= m.weight.pow(2).sum(1, keepdim=True).sqrt()
                m.bias.zero_()


class _PolicyValueModel(nn.Module):
    """Both levels: Normal(mu, std) over two dimensions (the goal, the action) and the value from the encoder's
    embedding -- the high level on obs, the low level on [obs, goal]."""

    def __init__(self, x_dim, zone_feat, h=128):
        super().__init__()
        self.env_model = _ZoneEncoder(x_dim, zone_feat, h)
        self.actor = nn.Module()
        self.actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h, h), nn.ReLU()))
        self.actor.mu_ = nn.Linear(h, 2)
        self.actor.std_ = nn.Linear(h, 2)
        self.critic = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))
        _init_params(self)

    def forward(self, x, zone_obs):
        emb = self.env_model(x, zone_obs)
        a = self.actor.enc_(emb)
        dist = Normal(2.0 * (torch.sigmoid(self.actor.mu_(a)) - 0.5), torch.sigmoid(self.actor.std_(a)) + 1e-3)
        return dist, self.critic(emb).squeeze(1)


class HighPolicyValueModel(_PolicyValueModel):
    def __init__(self, zone_feat, h=128):
        super().__init__(8, zone_feat, h)


class LoPolicyValueModel(_PolicyValueModel):
    def __init__(self, zone_feat, h=128):
        super().__init__(10, zone_feat, h)

    def forward(self, obs, zone_obs, goal):
        return super().forward(torch.cat([obs, goal], dim=-1), zone_obs)


def _ppo_loss(log_prob, old_log_prob, value, sb, clip_eps):
    ratio = torch.exp(log_prob - old_log_prob)
    adv = sb["advantage"]
    policy_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_eps, 1.0 + clip_eps) * adv).mean()
    v_clip = sb["value"] + torch.clamp(value - sb["value"], -clip_eps, clip_eps)
    value_loss = torch.max((value - sb["returnn"]).pow(2), (v_clip - sb["returnn"]).pow(2)).mean()
    return policy_loss, value_loss


class XyGoalsPPO:
    """One iteration of the xy-goals agent: collect_experiences on the device, then the two updates of
    _hier_policy_opt.py:195-363 in torch -- hi PPO on the windows (batches of batch_size // skill_len rows), lo PPO on
    the frames.  With device_update both updates run in the library too (``xyppo_init`` once; then ``collect_xy``,
    ``xyppo_update``, ``xyppo_publish`` per iteration; the modules get the learners' parameters back when ``train``
    ends)."""

    def __init__(self, tenv, h=128, skill_len=20, frames_per_proc=100, epochs=4, batch_size=16384, hi_epochs=4, lr=3e-4,
                 hi_lr=3e-4, discount=0.99, gae_lambda=0.95, clip_eps=0.2, entropy_coef=0.003, hi_entropy_coef=0.01,
                 value_loss_coef=0.5, hi_value_coef=0.5, seed=1, device_update=False):
        self.tenv, self.L, self.T = tenv, skill_len, frames_per_proc
        dev, F_ = tenv.device, tenv.env.zone_feat
        self.hi = HighPolicyValueModel(F_, h).to(dev)
        self.lo = LoPolicyValueModel(F_, h).to(dev)
        self.epochs, self.batch_size, self.hi_epochs = epochs, batch_size, hi_epochs
        self.hi_batch_size = max(1, batch_size // skill_len)
        self.discount, self.gae_lambda, self.clip_eps = discount, gae_lambda, clip_eps
        self.entropy_coef, self.hi_entropy_coef = entropy_coef, hi_entropy_coef
        self.value_loss_coef, self.hi_value_coef = value_loss_coef, hi_value_coef
        self.lo_optimizer = torch.optim.Adam(self.lo.parameters(), lr, eps=1e-8)
        self.hi_optimizer = torch.optim.Adam(self.hi.parameters(), hi_lr, eps=1e-8)
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self.seed, self.it = seed, 0
        self.device_update = device_update
        if device_update:
            self.rng = np.random.default_rng(seed)
            tenv.xyppo_init(self.hi.state_dict(), self.lo.state_dict(),
                            lo=dict(lr=lr, clip_eps=clip_eps, entropy_coef=entropy_coef, value_loss_coef=value_loss_coef,
                                    max_batch=batch_size),
                            hi=dict(lr=hi_lr, clip_eps=clip_eps, entropy_coef=hi_entropy_coef,
                                    value_loss_coef=hi_value_coef, max_batch=self.hi_batch_size))
            tenv.env.configure_skills(skill_len)          # the period xyppo_publish hands on
            tenv.xyppo_publish()

    def _batches(self, total, size):
        order = torch.randperm(total, device=self.tenv.device, generator=self.gen)
        return [order[i:i + size] for i in range(0, total, size)]

    def collect(self):
        """Reload the device agent from the modules (device_update: xyppo_publish has), collect; (lo, hi, num_frames)
        of TorchZoneEnv.collect_xy."""
        if not self.device_update:
            self.tenv.load_xy(self.hi.state_dict(), self.lo.state_dict(), skill_len=self.L)
        out = self.tenv.collect_xy(self.T, policy_seed=self.seed * 1000003 + self.it, discount=self.discount,
                                   gae_lambda=self.gae_lambda)
        self.it += 1
        return out

    def update_hi_parameters(self, hi):
        stats = {}
        for _ in range(self.hi_epochs):
            for idx in self._batches(hi["goal"].shape[0], self.hi_batch_size):
                sb = {k: v[idx] for k, v in hi.items()}
                dist, value = self.hi(sb["obs"], sb["zone_obs"])
                entropy = dist.entropy().sum(dim=-1).mean()
                policy_loss, value_loss = _ppo_loss(dist.log_prob(sb["goal"]).sum(dim=-1), sb["log_prob"], value, sb,
                                                    self.clip_eps)
                loss = policy_loss - self.hi_entropy_coef * entropy + self.hi_value_coef * value_loss
                self.hi_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self.hi_optimizer.step()
                stats = {"policy_loss": policy_loss, "value_loss": value_loss, "entropy": entropy}
        return {k: float(v.detach()) for k, v in stats.items()}

    def update_lo_parameters(self, lo):
        flat = {k: v.reshape((-1,) + tuple(v.shape[2:])) for k, v in lo.items()}
        stats = {}
        for _ in range(self.epochs):
            for idx in self._batches(flat["obs"].shape[0], self.batch_size):
                sb = {k: v[idx] for k, v in flat.items()}
                dist, value = self.lo(sb["obs"], sb["zone_obs"], sb["goal"])
                entropy = dist.entropy().mean()
                delta = (dist.log_prob(sb["action"]) - sb["log_prob"]).sum(dim=1)      # per dimension, then summed
                policy_loss, value_loss = _ppo_loss(delta, 0.0, value, sb, self.clip_eps)
                loss = policy_loss - self.entropy_coef * entropy + self.value_loss_coef * value_loss
                self.lo_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self.lo_optimizer.step()
                stats = {"policy_loss": policy_loss, "value_loss": value_loss, "entropy": entropy}
        return {k: float(v.detach()) for k, v in stats.items()}

    def update(self, lo, hi):
        """The two updates on one collection (before the next collect overwrites its buffers), high level first."""
        logs = {"hi_" + k: v for k, v in self.update_hi_parameters(hi).items()}
        logs.update({"lo_" + k: v for k, v in self.update_lo_parameters(lo).items()})
        return logs

    def iteration(self):
        lo, hi, num_frames = self.collect()
        logs = {"num_frames": num_frames, "reward_per_frame": float(lo["env_reward"].mean()),
                "lo_reward_per_frame": float(lo["reward"].mean())}
        assert self.tenv.episode_logs()["num_frames"] == num_frames     # logs of collect_experiences, synthesized
        logs.update(episode_log_history(self.tenv.episode_log_stats(), num_frames))
        if self.device_update:
            logs.update(self.tenv.xyppo_update(self.epochs, self.batch_size, self.hi_epochs, self.hi_batch_size, self.rng))
            self.tenv.xyppo_publish()
            return logs
        logs.update(self.update(lo, hi))
        return logs


def train(env_id="PointTSP-v0", procs=4096, skill_len=20, frames_per_proc=100, updates=10, hidden=128, seed=1,
          log=print, **kw):
    torch.manual_seed(seed)
    env = Z.ZoneVecEnv(env_id, procs)
    env.build_bank(seed, 4 * procs)
    env.schedule_sequential(stride=procs)
    tenv = TorchZoneEnv(env)
    tenv.reset()
    algo = XyGoalsPPO(tenv, hidden, skill_len, frames_per_proc, seed=seed, **kw)
    for u in range(updates):
        t0 = time.perf_counter()
        logs = algo.iteration()
        torch.cuda.synchronize()
        logs.update(update=u, seconds=round(time.perf_counter() - t0, 3))
        log({k: (round(v, 4) if isinstance(v, float) else v) for k, v in logs.items()})
    if algo.device_update:
        hi_sd, lo_sd = tenv.xyppo_state_dicts()
        algo.hi.load_state_dict(hi_sd)
        algo.lo.load_state_dict(lo_sd)
    env.close()
    return algo


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="PointTSP-v0")
    ap.add_argument("--procs", type=int, default=4096)
    ap.add_argument("--skill-len", type=int, default=20)
    ap.add_argument("--frames-per-proc", type=int, default=100)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--hidden-size", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device-update", action="store_true",
                    help="run both PPO updates in the library (zenv_xyppo_*) instead of torch")
    a = ap.parse_args()
    train(a.env, a.procs, a.skill_len, a.frames_per_proc, a.updates, a.hidden_size, a.seed,
          device_update=a.device_update)
