"""Fixed-length-skills / DIAYN training on the device env: experience collection by ``zenv_collect_skill`` (the skill
picks, the low level's action, the env step with the idle no-op, the inverse model's diversity reward and both GAE
recursions in HIP kernels), the four updates in plain PyTorch on the same device and stream.

This is the loop of the reference's skill planner (main/src/torch_ac/algos/hrl_policy_planner.py with
_hier_policy_opt.py: collect_experiences, update_lo_parameters, update_hi_parameters, update_inverse_parameters,
update_skill_prior) with ``ParallelEnv`` and the host loop replaced by ``TorchZoneEnv.collect_skills``.  The modules carry
the reference's parameter names (main/src/hier_policy_value_models.py, main/src/inverse_model.py; restated in
tests/skill_ref.py and tests/skill_collect_ref.py), so their state_dicts are the checkpoint's; after every update the
device agent is reloaded from them.

    python examples/skill_planner_ppo_torch.py --env PointTSP-v0 --procs 4096 --skill-len 20 --frames-per-proc 100

``--device-update`` runs all four updates in the library as well: the low and the high level's (``TorchZoneEnv.skppo_init``
/ ``skppo_update`` / ``skppo_publish``: zenv_skppo_*, csrc/ppo_update.hip) and the inverse model's and the skill prior's
(``diayn_init`` / ``diayn_update`` / ``diayn_prior_update`` / ``diayn_publish``: zenv_diayn_*).  Off by default, the
torch path is what it was.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Categorical

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
    """The low level: Normal(mu, std) over the action and the value, from [obs, onehot(skill)] and the zone rows."""

    def __init__(self, zone_feat, n_skills, h=128):
        super().__init__()
        self.n_skills = n_skills
        self.env_model = _ZoneEncoder(8 + n_skills, zone_feat, h)
        self.actor = nn.Module()
        self.actor.enc_ = nn.Sequential(nn.Sequential(nn.Linear(h + n_skills, h), nn.ReLU()))
        self.actor.mu_ = nn.Linear(h, 2)
        self.actor.std_ = nn.Linear(h, 2)
        self.critic = nn.Sequential(nn.Linear(h + n_skills, h), nn.ReLU(), nn.Linear(h, 1))
        _init_params(self)

    def forward(self, obs, zone_obs, skill):
        onehot = F.one_hot(skill.long(), self.n_skills).to(obs.dtype)
        x = torch.cat([self.env_model(torch.cat([obs, onehot], dim=-1), zone_obs), onehot], dim=-1)
        a = self.actor.enc_(x)
        dist = torch.distributions.Normal(2.0 * (torch.sigmoid(self.actor.mu_(a)) - 0.5),
                                          torch.sigmoid(self.actor.std_(a)) + 1e-3)
        return dist, self.critic(x).squeeze(1)


class InverseModel(nn.Module):
    """DIAYN's discriminator: the skill's logits from an observation (main/src/inverse_model.py)."""

    def __init__(self, zone_feat, n_skills, h=128):
        super().__init__()
        self.zone_net = nn.Sequential(nn.Linear(8 + zone_feat, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(),
                                      nn.Linear(h, h))
        self.combine_net = nn.Sequential(nn.Linear(8 + h, h), nn.ReLU(), nn.Linear(h, n_skills))

    def forward(self, obs, zone_obs):
        n_zones = zone_obs.shape[1]
        rows = torch.cat([obs.unsqueeze(1).expand(-1, n_zones, -1), zone_obs], dim=-1)
        return self.combine_net(torch.cat([obs, self.zone_net(rows).sum(dim=1) / n_zones], dim=-1))


def _ppo_loss(log_prob, old_log_prob, value, sb, clip_eps):
    ratio = torch.exp(log_prob - old_log_prob)
    adv = sb["advantage"]
    policy_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_eps, 1.0 + clip_eps) * adv).mean()
    v_clip = sb["value"] + torch.clamp(value - sb["value"], -clip_eps, clip_eps)
    value_loss = torch.max((value - sb["returnn"]).pow(2), (v_clip - sb["returnn"]).pow(2)).mean()
    return policy_loss, value_loss


class SkillPlannerPPO:
    """One iteration of the skill planner: collect_experiences on the device, then the four updates of
    _hier_policy_opt.py:265-466 in torch -- lo PPO, hi PPO, the inverse model's cross-entropy, the skill prior's.  With
    device_update the lo and hi PPO run in the library (``skppo_init`` once; then ``collect_skills``, ``skppo_update``,
    ``skppo_publish`` per iteration, and the modules get the learners' parameters back after every update), and so do
    the other two (``diayn_init`` once; ``diayn_update``, ``diayn_prior_update``, ``diayn_publish`` per iteration)."""

    def __init__(self, tenv, n_skills=5, h=128, skill_len=20, frames_per_proc=100, diversity_coef=0.1, train_hi=True,
                 epochs=4, batch_size=16384, hi_epochs=4, hi_batch_size=4096, inverse_epochs=4,
                 inverse_batch_size=16384, lr=3e-4, hi_lr=3e-4, inverse_lr=3e-4, discount=0.99, gae_lambda=0.95,
                 clip_eps=0.2, entropy_coef=0.003, hi_entropy_coef=0.01, value_loss_coef=0.5, hi_value_coef=0.5,
                 seed=1, device_update=False):
        self.tenv, self.S, self.L, self.T = tenv, n_skills, skill_len, frames_per_proc
        dev, F_ = tenv.device, tenv.env.zone_feat
        self.hi_net = HighPolicyValueModel(F_, n_skills, h).to(dev)
        self.lo_net = LoPolicyValueModel(F_, n_skills, h).to(dev)
        self.inverse = InverseModel(F_, n_skills, h).to(dev)
        self.skill_logits = torch.zeros(n_skills, device=dev, requires_grad=True)     # the learned skill prior
        self.diversity_coef, self.train_hi = diversity_coef, train_hi
        self.epochs, self.batch_size, self.hi_epochs, self.hi_batch_size = epochs, batch_size, hi_epochs, hi_batch_size
        self.inverse_epochs, self.inverse_batch_size = inverse_epochs, inverse_batch_size
        self.discount, self.gae_lambda, self.clip_eps = discount, gae_lambda, clip_eps
        self.entropy_coef, self.hi_entropy_coef = entropy_coef, hi_entropy_coef
        self.value_loss_coef, self.hi_value_coef = value_loss_coef, hi_value_coef
        self.lo_optimizer = torch.optim.Adam(self.lo_net.parameters(), lr, eps=1e-8)
        self.hi_optimizer = torch.optim.Adam(self.hi_net.parameters(), hi_lr, eps=1e-8)
        self.inverse_optimizer = torch.optim.Adam(self.inverse.parameters(), inverse_lr, eps=1e-8)
        self.skill_logit_optimizer = torch.optim.Adam([self.skill_logits], 1e-2, eps=1e-8)
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self.seed, self.it = seed, 0
        self.device_update = device_update
        if device_update:
            self.rng = np.random.default_rng(seed)
            tenv.skppo_init(self.hi_net.state_dict(), self.lo_net.state_dict(),
                            lo=dict(lr=lr, clip_eps=clip_eps, entropy_coef=entropy_coef, value_loss_coef=value_loss_coef,
                                    max_batch=batch_size),
                            hi=dict(lr=hi_lr, clip_eps=clip_eps, entropy_coef=hi_entropy_coef,
                                    value_loss_coef=hi_value_coef, max_batch=hi_batch_size))
            tenv.env.configure_skills(skill_len)          # the period skppo_publish hands on
            tenv.skppo_publish()
            tenv.diayn_init(self.inverse.state_dict(), n_skills, prior_logits=self.skill_logits.detach(),
                            lr=inverse_lr, max_batch=inverse_batch_size)
            tenv.diayn_publish()

    def _batches(self, total, size):
        order = torch.randperm(total, device=self.tenv.device, generator=self.gen)
        return [order[i:i + size] for i in range(0, total, size)]

    def collect(self):
        """Reload the device agent from the modules (device_update: skppo_publish has), collect; (lo, hi, inverse,
        num_frames) of TorchZoneEnv."""
        if not self.device_update:
            self.tenv.load_skills(self.hi_net.state_dict(), self.lo_net.state_dict(), skill_len=self.L)
            self.tenv.load_skill_inverse(self.inverse.state_dict(), self.S)
        prior = self.tenv.diayn_prior_logits() if self.device_update else self.skill_logits.detach()
        out = self.tenv.collect_skills(self.T, policy_seed=self.seed * 1000003 + self.it, discount=self.discount,
                                       gae_lambda=self.gae_lambda, diversity_coef=self.diversity_coef,
                                       skill_prior_logits=prior, sample_hi=self.train_hi)
        self.it += 1
        return out

    def update_lo_parameters(self, lo):
        flat = {k: v.reshape((-1,) + tuple(v.shape[2:])) for k, v in lo.items()}
        stats = {}
        for _ in range(self.epochs):
            for idx in self._batches(flat["obs"].shape[0], self.batch_size):
                sb = {k: v[idx] for k, v in flat.items()}
                dist, value = self.lo_net(sb["obs"], sb["zone_obs"], sb["skill"])
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
        action = hi["action"].long()
        for _ in range(self.hi_epochs):
            for idx in self._batches(action.shape[0], self.hi_batch_size):
                sb = {k: v[idx] for k, v in hi.items()}
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

    def update_inverse_parameters(self, inverse):
        losses = []
        total = inverse["skill"].shape[0]
        for _ in range(self.inverse_epochs):
            for idx in self._batches(total, self.inverse_batch_size):
                loss = F.cross_entropy(self.inverse(inverse["obs"][idx], inverse["zone_obs"][idx]),
                                       inverse["skill"][idx].long())
                self.inverse_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self.inverse_optimizer.step()
                losses.append(loss.detach())
        first = max(1, len(losses) // self.inverse_epochs)
        return {"loss": float(torch.stack(losses[:first]).mean()) if losses else 0.0}

    def update_skill_prior(self, hi):
        actions = hi["action"].long()
        loss = F.cross_entropy(self.skill_logits.expand(actions.shape[0], self.S), actions)
        self.skill_logit_optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.skill_logit_optimizer.step()
        return {"loss": float(loss.detach())}

    def update(self, lo, hi, inverse):
        """The four updates on one collection (before the next collect overwrites its buffers)."""
        if self.device_update:
            logs = self.tenv.skppo_update(self.epochs, self.batch_size, self.hi_epochs if self.train_hi else 0,
                                          self.hi_batch_size, self.rng)
            self.tenv.skppo_publish()
            hi_sd, lo_sd = self.tenv.skppo_state_dicts()  # the modules follow the learners
            self.hi_net.load_state_dict(hi_sd)
            self.lo_net.load_state_dict(lo_sd)
            logs.update({"inverse_" + k: v for k, v in
                         self.tenv.diayn_update(self.inverse_epochs, self.inverse_batch_size, self.gen).items()})
            new_logits = self.tenv.diayn_prior_update()
            self.tenv.diayn_publish()
            self.inverse.load_state_dict(self.tenv.diayn_state_dict())
            with torch.no_grad():
                self.skill_logits.copy_(torch.as_tensor(new_logits))
            probs = F.softmax(self.skill_logits.detach(), dim=0)
            logs.update({"prior_" + str(i): float(p) for i, p in enumerate(probs)})
            return logs
        logs = {"lo_" + k: v for k, v in self.update_lo_parameters(lo).items()}
        if self.train_hi:
            logs.update({"hi_" + k: v for k, v in self.update_hi_parameters(hi).items()})
        logs.update({"inverse_" + k: v for k, v in self.update_inverse_parameters(inverse).items()})
        logs.update({"prior_" + k: v for k, v in self.update_skill_prior(hi).items()})
        return logs

    def iteration(self):
        lo, hi, inverse, num_frames = self.collect()
        logs = {"num_frames": num_frames, "reward_per_frame": float(lo["env_reward"].mean()),
                "diversity_per_frame": float(lo["diversity"].mean())}
        # logs of collect_experiences, synthesized as train_skill_planner.py:233-250 does
        assert self.tenv.episode_logs()["num_frames"] == num_frames
        logs.update(episode_log_history(self.tenv.episode_log_stats(), num_frames,
                                        ("return_per_episode", "num_frames_per_episode", "diversity_per_episode")))
        logs.update(self.update(lo, hi, inverse))
        return logs


def train(env_id="PointTSP-v0", procs=4096, skill_len=20, frames_per_proc=100, updates=10, n_skills=5, hidden=128,
          diversity_coef=0.1, seed=1, log=print, device_update=False, **kw):
    torch.manual_seed(seed)
    env = Z.ZoneVecEnv(env_id, procs)
    env.build_bank(seed, 4 * procs)
    env.schedule_sequential(stride=procs)
    tenv = TorchZoneEnv(env)
    tenv.reset()
    algo = SkillPlannerPPO(tenv, n_skills, hidden, skill_len, frames_per_proc, diversity_coef, seed=seed,
                           device_update=device_update, **kw)
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
    ap.add_argument("--skill-len", type=int, default=20)
    ap.add_argument("--frames-per-proc", type=int, default=100)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--n-skills", type=int, default=5)
    ap.add_argument("--hidden-size", type=int, default=128)
    ap.add_argument("--diversity-coef", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device-update", action="store_true",
                    help="run the four updates in the library (zenv_skppo_*, zenv_diayn_*) instead of torch")
    a = ap.parse_args()
    train(a.env, a.procs, a.skill_len, a.frames_per_proc, a.updates, a.n_skills, a.hidden_size, a.diversity_coef,
          a.seed, device_update=a.device_update)
