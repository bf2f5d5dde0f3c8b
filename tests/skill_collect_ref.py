"""TEST INFRASTRUCTURE -- restatements for zenv_collect_skill (checker only), shared by tests/test_gpu_skill_collect.py
and tests/test_skill_collect_cpu.py:
* ``random_inverse_state_dict`` / ``inverse_log_softmax``: a float32 torch restatement of InverseModel
  (main/src/inverse_model.py): zone_net on [obs, zone row], the mean over the zones, combine_net = Linear, ReLU, Linear
* ``replay``: a second handle driven frame by frame with zenv_policy(SKILL_SAMPLE) + zenv_step, auto-reset only on a
  window's last frame -- what one collection sees
* ``bookkeeping``: numpy restatement of _hier_policy_opt.py:104-212 besides the networks (both GAEs, the window sums,
  next_mask, num_frames, the inverse-exps selection)
"""
import numpy as np
import torch

from tests.skill_ref import _lin

LAM, GAMMA = 0.95, 0.99


def random_inverse_state_dict(F, S, h=128, seed=0, bias_scale=0.1, weight_scale=1.0):
    """InverseModel.state_dict() with the reference's key names, float32 torch tensors.  weight_scale multiplies every
    weight row (unit norm by default): larger logits, for the edge sweeps."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, n_out, n_in in (("zone_net.0", h, 8 + F), ("zone_net.2", h, h), ("zone_net.4", h, h),
                              ("combine_net.0", h, 8 + h), ("combine_net.2", S, h)):
        w, b = _lin(g, n_out, n_in, bias_scale, weight_scale)
        sd[f"{name}.weight"], sd[f"{name}.bias"] = w * (3.0 if name == "combine_net.2" else 1.0), b
    return sd


def inverse_log_softmax(sd, obs, zone_obs, dtype=torch.float32):
    """log_softmax(InverseModel(obs)) [B, S], float32 numpy (InverseModel.forward, then F.log_softmax(dim=-1));
    dtype=torch.float64: the same operations on the same float32 weights and inputs in float64."""
    sd = {k: torch.as_tensor(np.asarray(v)).float().to(dtype) for k, v in sd.items()}
    o = torch.as_tensor(np.asarray(obs, np.float32)).to(dtype)
    zo = torch.as_tensor(np.asarray(zone_obs, np.float32)).to(dtype)
    bs, n_zones = zo.shape[0], zo.shape[1]
    x = torch.cat([o.view(bs, 1, 8).expand(bs, n_zones, 8), zo], dim=-1)
    y = torch.relu(x @ sd["zone_net.0.weight"].T + sd["zone_net.0.bias"])
    y = torch.relu(y @ sd["zone_net.2.weight"].T + sd["zone_net.2.bias"])
    y = y @ sd["zone_net.4.weight"].T + sd["zone_net.4.bias"]
    zone_enc = y.sum(dim=1) / n_zones
    c = torch.relu(torch.cat([o, zone_enc], dim=-1) @ sd["combine_net.0.weight"].T + sd["combine_net.0.bias"])
    logits = c @ sd["combine_net.2.weight"].T + sd["combine_net.2.bias"]
    return torch.log_softmax(logits, dim=-1).numpy()


def replay(Z, env, frames, L, seed):
    """Drive `env` for `frames` frames: zenv_policy(SKILL_SAMPLE), then zenv_step with auto-reset on every L-th frame
    (counted from this call's first frame); the per-frame record, and the final observation."""
    log = {k: [] for k in ("obs", "zone_obs", "skill", "logits", "hi_value", "action", "mu", "std", "value", "reward",
                           "done")}
    for t in range(frames):
        o, zo = env.observations()
        env.policy(Z.POLICY_SKILL_SAMPLE, policy_seed=seed)
        log["obs"].append(o)
        log["zone_obs"].append(zo)
        log["skill"].append(env.get(Z.F_SKILL))
        log["logits"].append(env.get(Z.F_SKILL_LOGITS))
        log["hi_value"].append(env.get(Z.F_SKILL_VALUE))
        log["action"].append(env.get(Z.F_ACTIONS))
        log["mu"].append(env.get(Z.F_POLICY_MU))
        log["std"].append(env.get(Z.F_POLICY_STD))
        log["value"].append(env.get(Z.F_POLICY_VALUE))
        env.step(None, auto_reset=(t + 1) % L == 0)
        _, _, r, d, _ = env.results()
        log["reward"].append(r)
        log["done"].append(d)
    rec = {k: np.stack(v) for k, v in log.items()}
    rec["obs_T"], rec["zone_obs_T"] = env.observations()
    return rec


def bookkeeping(reward, lo_reward, mask, cur_mask, lo_value, hi_value, next_lo_value, next_hi_value, L,
                discount=GAMMA, gae_lambda=LAM, dtype=np.float32):
    """_hier_policy_opt.py:104-161 in numpy float32, on time-major records: reward / lo_reward / mask / lo_value [T, N],
    hi_value [W, N], cur_mask (self.lo_mask after the frames), next_*_value [N].  Returns the low-level advantage
    [T, N]; the high-level reward, next_mask and advantage [W, N]; num_frames; the inverse-exps selection as
    (frame i, env j) index arrays in env-major order."""
    f = dtype                                             # float32: the device's arithmetic; float64 for a float64 record
    reward, lo_reward, mask = (np.asarray(a, f) for a in (reward, lo_reward, mask))
    T, N = reward.shape
    W = T // L
    hi_reward = np.zeros((W, N), f)
    hi_mask = np.zeros((W, N), f)
    hi_adv = np.zeros((W, N), f)
    for k in reversed(range(W)):
        r = np.zeros(N, f)
        for i in range(k * L, (k + 1) * L):
            r = (r + reward[i]).astype(f)
        hi_reward[k] = r
        nm = mask[(k + 1) * L] if k < W - 1 else np.asarray(cur_mask, f)
        nv = hi_value[k + 1] if k < W - 1 else np.asarray(next_hi_value, f)
        na = hi_adv[k + 1] if k < W - 1 else np.zeros(N, f)
        delta = r + nv * nm - hi_value[k]
        hi_adv[k] = delta + f(gae_lambda) * na * nm
        hi_mask[k] = nm
    lo_adv = np.zeros((T, N), f)
    for i in reversed(range(T)):
        nm = mask[i + 1] if i < T - 1 else np.asarray(cur_mask, f)
        nv = lo_value[i + 1] if i < T - 1 else np.asarray(next_lo_value, f)
        na = lo_adv[i + 1] if i < T - 1 else np.zeros(N, f)
        delta = lo_reward[i] + f(discount) * nv * nm - lo_value[i]
        lo_adv[i] = delta + f(discount) * f(gae_lambda) * na * nm
    # num_frames: every env's frames of a window up to and including its first done (done_{t-1} = 1 - mask[t])
    active = np.ones(N, bool)
    num_frames = 0
    for t in range(T):
        if t % L == 0:
            active[:] = True
        else:
            active &= mask[t] != 0
        num_frames += int(active.sum())
    jj, ii = np.nonzero(mask[1:].T != 0)                  # env-major: env j, then frame i (lo_masks[i+1][j])
    return {"lo_adv": lo_adv, "hi_reward": hi_reward, "hi_mask": hi_mask, "hi_adv": hi_adv, "num_frames": num_frames,
            "inverse_idx": (ii, jj)}
