"""The project's own restatement of DIAYN's two remaining updates -- the inverse model's cross-entropy update and the
learned skill prior's step (main/src/torch_ac/algos/_hier_policy_opt.py:193-199, 421-464) -- for the tests of the device
learner (zenv_diayn_*): InverseRef, a torch module of any dtype under InverseModel's state_dict names; the kept-sample
rule, the sub-batch loss and the per-row derivative of the logits in numpy; the prior's closed-form gradient and Adam step.
The tolerance rule, Adam and the norm are tests/ppo_update_ref.py's."""
import math

import numpy as np
import torch
import torch.nn as nn

from tests.ppo_update_ref import adam_step, check_rule, perturbed, total_norm  # noqa: F401  (re-exported)

STATS = ("loss", "grad_norm")                     # columns 0 and 5 of the statistics row; 1-4 are 0
HYPER = dict(lr=3e-4, adam_eps=1e-8)
PRIOR = dict(lr=1e-2, adam_eps=1e-8)


class InverseRef(nn.Module):
    """InverseModel: logits = combine_net.2(relu(combine_net.0([obs, mean over zones of zone_net([obs, zone row])])))."""

    def __init__(self, F, S, h, dtype):
        super().__init__()
        self.zone_net = nn.Sequential(nn.Linear(8 + F, h), nn.ReLU(), nn.Linear(h, h), nn.ReLU(), nn.Linear(h, h))
        self.combine_net = nn.Sequential(nn.Linear(8 + h, h), nn.ReLU(), nn.Linear(h, S))
        self.to(dtype)

    def forward(self, obs, zone_obs):
        n_zones = zone_obs.shape[1]
        rows = torch.cat([obs.unsqueeze(1).expand(-1, n_zones, -1), zone_obs], dim=-1)
        return self.combine_net(torch.cat([obs, self.zone_net(rows).sum(dim=1) / n_zones], dim=-1))


def model_from(state_dict, F, dtype):
    S, h = (int(v) for v in state_dict["combine_net.2.weight"].shape)
    model = InverseRef(F, S, h, dtype)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state_dict.items()})
    return model


def kept_samples(mask):
    """mask [N, T] -> the kept sample indexes, ascending: i = env (T - 1) + f where mask[env, f + 1] != 0."""
    keep = np.asarray(mask)[:, 1:] != 0
    return np.flatnonzero(keep.reshape(-1)).astype(np.int32)


def kept_samples_loops(mask):
    """The same list by the reference's own loops (:193-199): for j in procs, for i in range(T - 1) if masks[i+1][j]."""
    masks = np.asarray(mask).T                    # [T][procs], as the reference holds it
    T, P = masks.shape
    out = []
    for j in range(P):
        for i in range(T - 1):
            if masks[i + 1][j]:
                out.append(j * (T - 1) + i)
    return np.asarray(out, np.int32)


def batch(lo, idx, dtype):
    """lo: name -> array [N, T, ...] (collect_skills' lo); idx: sample indexes in [0, N (T - 1)).  The observation is
    frame f + 1's, the skill frame f's."""
    idx = np.asarray(idx, np.int64)
    T1 = lo["obs"].shape[1] - 1
    env, f = idx // T1, idx % T1
    return {"obs": torch.as_tensor(np.asarray(lo["obs"])[env, f + 1]).to(dtype),
            "zone_obs": torch.as_tensor(np.asarray(lo["zone_obs"])[env, f + 1]).to(dtype),
            "skill": torch.as_tensor(np.asarray(lo["skill"])[env, f].astype(np.int64))}


def loss_rows(logits, skill):
    """Per-row cross-entropy in numpy, in the logits' dtype."""
    logits = np.asarray(logits)
    m = logits.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(logits - m).sum(axis=1))
    return lse - logits[np.arange(len(skill)), np.asarray(skill)]


def dlogit(logits, skill):
    """d mean(CE) / d logits in numpy, in the logits' dtype: (softmax - onehot) / B."""
    logits = np.asarray(logits)
    m = logits.max(axis=1, keepdims=True)
    p = np.exp(logits - m)
    p = p / p.sum(axis=1, keepdims=True)
    p[np.arange(len(skill)), np.asarray(skill)] -= 1
    return p / logits.dtype.type(len(skill))


def gradients(model, b, scale=1.0):
    """state_dict key -> gradient of the mean cross-entropy (times scale), and the two statistics."""
    model.zero_grad()
    loss = nn.functional.cross_entropy(model(b["obs"], b["zone_obs"]), b["skill"]) * scale
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return grads, {"loss": loss.item(), "grad_norm": total_norm(grads.values())}


class RefLearner:
    """update_inverse_parameters' inner loop in a dtype: autograd gradients, torch's own Adam, no clip."""

    def __init__(self, state_dict, F, dtype, hyper=HYPER):
        self.model = model_from(state_dict, F, dtype)
        self.opt = torch.optim.Adam(self.model.parameters(), hyper["lr"], eps=hyper["adam_eps"], foreach=False)

    def minibatch(self, b):
        grads, stats = gradients(self.model, b)
        self.opt.step()
        return stats


def prior_gradient(logits, actions, S):
    """softmax(logits) - count / M in float64: the gradient of F.cross_entropy(logits.expand(M, S), actions)."""
    z = np.asarray(logits, np.float64)
    p = np.exp(z - z.max())
    p /= p.sum()
    return p - np.bincount(np.asarray(actions), minlength=S)[:S] / float(len(actions))


class PriorRef:
    """update_skill_prior in a dtype: torch's own Adam on skill_logits."""

    def __init__(self, logits, dtype, hyper=PRIOR):
        self.logits = torch.as_tensor(np.asarray(logits)).to(dtype).clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.logits], hyper["lr"], eps=hyper["adam_eps"], foreach=False)

    def step(self, actions):
        a = torch.as_tensor(np.asarray(actions, np.int64))
        loss = nn.functional.cross_entropy(self.logits.expand(a.shape[0], self.logits.shape[0]), a)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return self.logits.detach().numpy().copy()


def prior_step_numpy(logits, m, v, actions, step, hyper=PRIOR):
    """The same step from the closed-form gradient on float64 arrays, in place."""
    g = prior_gradient(logits, actions, len(logits))
    adam_step(logits, g, m, v, step, hyper["lr"], hyper["adam_eps"])
    return g


def isnan(x):
    return math.isnan(float(x))
