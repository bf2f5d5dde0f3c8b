"""The flat actor-critic's A2C update restated for the tests of the device learner (zenv_a2c_*): this project's own code,
written from the reference's behaviour, no text of it.

  network   ppo_update_ref.ACModelRef, the plain critic (A2CAlgo has no distributional branch)
  loss      update_parameters' body for recurrence 1 (main/src/torch_ac/algos/a2c.py:49-57):
              -mean(log_prob(a) advantage) - entropy_coef mean(entropy) + value_loss_coef mean((value - returnn)^2)
            with log_prob(a) summed over the action's two components -- ppo.py:73-76's reading; a2c.py:53 as written
            multiplies [B, 2] by [B] and raises for the Box policy -- and the entropy's mean over B x 2
  chunks    the loss of all `total` frames as a sum over chunks of at most max_batch frames, every chunk's sums divided by
            `total`; autograd adds each chunk's gradient onto ``.grad`` in the chunks' order, in the model's dtype
  clip      the norm of a2c.py:79 and clip_grad_norm_ (:80), as arithmetic
  RMSprop   torch.optim.RMSprop's step (:18, :81: momentum 0, not centered, no weight decay), as arithmetic: eps is added
            after the square root
  indexes   _get_starting_indexes (:95-110) for recurrence 1: 0 .. N T - 1

The float64 run is the truth, the float32 run of the same code on the CPU the ruler (ppo_update_ref.check_rule).
"""
import numpy as np
import torch
import torch.nn as nn

from tests import ppo_update_ref as R

HYPER = dict(lr=0.01, rmsprop_alpha=0.99, rmsprop_eps=1e-8, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=0.5)
STATS = ("entropy", "value", "policy_loss", "value_loss", "grad_norm")


def chunks_of(idx, max_batch):
    """The index list cut as zenv_a2c_update cuts it: consecutive pieces of max_batch, the last one short."""
    idx = np.asarray(idx)
    return [idx[lo:lo + max_batch] for lo in range(0, len(idx), max_batch)]


def chunk_terms(model, b, hyper, total):
    """One chunk's share of the update's loss (a tensor), and its sums of the four logged per-sample terms."""
    mu, std, v, _ = model(b["obs"], b["zone_obs"])
    dist = torch.distributions.Normal(mu, std)
    log_prob = dist.log_prob(b["action"]).sum(dim=1)
    entropy = dist.entropy()                                           # [B, 2]: the mean is over both
    policy = -(log_prob * b["advantage"]).sum()
    value = (v - b["returnn"]).pow(2).sum()
    loss = (policy - hyper["entropy_coef"] * entropy.sum() / 2.0 + hyper["value_loss_coef"] * value) / total
    sums = {"entropy": entropy.sum().item() / 2.0, "value": v.sum().item(), "policy_loss": policy.item(),
            "value_loss": value.item()}
    return loss, sums


def accumulate(model, exps, chunks, hyper):
    """The gradient of the loss over every frame the chunks name and the five statistics, chunk by chunk in order."""
    dtype = next(model.parameters()).dtype
    total = int(sum(len(c) for c in chunks))
    model.zero_grad()
    run = dict.fromkeys(STATS[:4], 0.0)
    for c in chunks:
        loss, sums = chunk_terms(model, R.as_batch(exps, c, dtype), hyper, total)
        loss.backward()                                                # .grad += the chunk's share
        for k in run:
            run[k] += sums[k]
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    stats = {k: run[k] / total for k in run}
    stats["grad_norm"] = R.total_norm(grads.values())
    return grads, stats


def rmsprop_step(p, g, sq, lr, alpha, eps):
    """One step of torch.optim.RMSprop on float64 arrays, in place."""
    sq *= alpha
    sq += (1.0 - alpha) * g * g
    p -= lr * g / (np.sqrt(sq) + eps)


class RefLearner:
    """update_parameters in a dtype: chunked autograd gradients, the clip, torch's own RMSprop."""

    def __init__(self, state_dict, F, dtype, hyper):
        self.model = R.model_from(state_dict, F, dtype)
        self.hyper = hyper
        self.opt = torch.optim.RMSprop(self.model.parameters(), hyper["lr"], alpha=hyper["rmsprop_alpha"],
                                       eps=hyper["rmsprop_eps"], foreach=False)

    def update(self, exps, chunks):
        grads, stats = accumulate(self.model, exps, chunks, self.hyper)
        self.apply()
        return stats

    def apply(self):
        """clip_grad_norm_ on a copy of the accumulated gradient -- it stays unclipped, as the device's arena does -- and
        the optimizer's step."""
        kept = [p.grad.detach().clone() for p in self.model.parameters()]
        nn.utils.clip_grad_norm_(self.model.parameters(), self.hyper["max_grad_norm"], foreach=False)
        self.opt.step()
        for p, g in zip(self.model.parameters(), kept):
            p.grad.copy_(g)

    def square_avg(self):
        return {k: self.opt.state[p]["square_avg"].detach().clone() for k, p in self.model.named_parameters()}


def golden_exps(g):
    """The recorded batch of tests/golden/agent_main_a2c_update.npz as ``as_batch`` reads one: name -> [N, T, ...]."""
    N, T = (int(v) for v in g["flat_a2c_update/shape/NT"])
    out = {}
    for k in ("obs", "zone_obs", "action", "log_prob", "value", "advantage", "returnn"):
        a = g[f"flat_a2c_update/exp/{k}"]
        out[k] = np.ascontiguousarray(a.reshape((N, T) + a.shape[1:]))
    return out, N, T


def golden_hyper(g):
    return {k: float(g[f"flat_a2c_update/hyper/{k}"]) for k in HYPER}
