"""TEST INFRASTRUCTURE -- restatements for zenv_collect_xy (checker only), shared by tests/test_gpu_xy_collect.py and
tests/test_xy_collect_cpu.py:
* ``goal_dist`` / ``lo_reward``: the distance of the goal from the robot (obs[1:3]) and the low level's reward, the
  progress towards the goal over one step inside a window, in numpy float32 -- one rounding per operation, as torch
* ``bookkeeping``: numpy float32 restatement of what collect_experiences of the xy-goals agent does besides the
  networks: the distance reward, both GAE recursions, the window sums, next_mask, num_frames
* ``replay``: a second handle driven frame by frame with zenv_policy(XY_SAMPLE) + zenv_step, auto-reset only on a
  window's last frame -- what one collection sees
* ``boot_noise``: the standard normal pair of the bootstrap goal g', the goal draw's arithmetic on its own stream
* ``hi_log_prob``: Normal(goal_mu, goal_std).log_prob(goal).sum(-1) in float64
"""
import numpy as np

from tests import philox_ref

LAM, GAMMA = 0.95, 0.99
TAG_XY_BOOT = 0x585942


def goal_dist(obs, goal, dtype=np.float32):
    """float32 [..]: sqrt((goal_x - obs[1])^2 + (goal_y - obs[2])^2), every operation rounded to float32 (or carried
    out in `dtype`: float64 for a float64 record)."""
    f = dtype
    obs, goal = np.asarray(obs, f), np.asarray(goal, f)
    dx = (goal[..., 0] - obs[..., 1]).astype(f)
    dy = (goal[..., 1] - obs[..., 2]).astype(f)
    return np.sqrt(((dx * dx).astype(f) + (dy * dy).astype(f)).astype(f)).astype(f)


def lo_reward(dist, mask, L, dtype=np.float32):
    """float32 [T, N]: (dist[t] - dist[t+1]) * (mask[t+1] * ((t+1) % L != 0)); frame T-1 is 0 (T is a multiple of L:
    the reference multiplies it by (T % L != 0) = 0).  dtype: the arithmetic's."""
    f = dtype
    dist, mask = np.asarray(dist, f), np.asarray(mask, f)
    T = dist.shape[0]
    out = np.zeros_like(dist)
    for t in range(T - 1):
        nm = (mask[t + 1] * f((t + 1) % L != 0)).astype(f)
        out[t] = ((dist[t] - dist[t + 1]).astype(f) * nm).astype(f)
    return out


def bookkeeping(dist, env_reward, mask, cur_mask, lo_value, hi_value, next_lo_value, next_hi_value, L,
                discount=GAMMA, gae_lambda=LAM, dtype=np.float32):
    """On time-major records: dist / env_reward / mask / lo_value [T, N], hi_value [W, N], cur_mask (the mask after the
    frames, carried into the next call), next_*_value [N].  Returns the low level's reward and advantage [T, N]; the
    high level's reward, next_mask and advantage [W, N]; num_frames.  dtype: the arithmetic's (float32: the device's;
    float64 for a float64 record)."""
    f = dtype
    env_reward, mask, lo_value = (np.asarray(a, f) for a in (env_reward, mask, lo_value))
    hi_value = np.asarray(hi_value, f)
    cur_mask = np.asarray(cur_mask, f)
    T, N = env_reward.shape
    W = T // L
    hi_reward = np.zeros((W, N), f)
    hi_mask = np.zeros((W, N), f)
    hi_adv = np.zeros((W, N), f)
    for k in reversed(range(W)):
        r = np.zeros(N, f)
        for i in range(k * L, (k + 1) * L):
            r = (r + env_reward[i]).astype(f)
        nm = mask[(k + 1) * L] if k < W - 1 else cur_mask
        nv = hi_value[k + 1] if k < W - 1 else np.asarray(next_hi_value, f)
        na = hi_adv[k + 1] if k < W - 1 else np.zeros(N, f)
        delta = r + nv * nm - hi_value[k]                           # no discount
        hi_adv[k] = delta + f(gae_lambda) * na * nm
        hi_reward[k], hi_mask[k] = r, nm
    lo_r = lo_reward(dist, mask, L, dtype)
    lo_adv = np.zeros((T, N), f)
    for i in reversed(range(T)):
        nm = mask[i + 1] if i < T - 1 else cur_mask
        nv = lo_value[i + 1] if i < T - 1 else np.asarray(next_lo_value, f)
        na = lo_adv[i + 1] if i < T - 1 else np.zeros(N, f)
        delta = lo_r[i] + f(discount) * nv * nm - lo_value[i]
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
    return {"lo_reward": lo_r, "lo_adv": lo_adv, "hi_reward": hi_reward, "hi_mask": hi_mask, "hi_adv": hi_adv,
            "num_frames": num_frames}


def replay(Z, env, frames, L, seed):
    """Drive `env` for `frames` frames: zenv_policy(XY_SAMPLE), then zenv_step with auto-reset on every L-th frame
    (counted from this call's first frame); the per-frame record, and the final observation."""
    log = {k: [] for k in ("obs", "zone_obs", "goal", "goal_mu", "goal_std", "hi_value", "action", "mu", "std", "value",
                           "reward", "done")}
    for t in range(frames):
        o, zo = env.observations()
        env.policy(Z.POLICY_XY_SAMPLE, policy_seed=seed)
        log["obs"].append(o)
        log["zone_obs"].append(zo)
        log["goal"].append(env.get(Z.F_XY_GOAL))
        log["goal_mu"].append(env.get(Z.F_XY_GOAL_MU))
        log["goal_std"].append(env.get(Z.F_XY_GOAL_STD))
        log["hi_value"].append(env.get(Z.F_XY_VALUE))
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


def boot_noise(n, seed, env_index0, step):
    """float64 [n, 2]: the standard normal pair of the bootstrap goal of envs 0 .. n-1 -- ``xy_ref.goal_noise``'s
    arithmetic (float64 Box-Muller on the two float32 uniforms, the angle formed in float32) on the bootstrap stream."""
    c = philox_ref._draw(n, seed, env_index0, step, TAG_XY_BOOT)
    u1 = philox_ref.uniform(c[0]).astype(np.float64)
    ang = (np.float32(6.283185307179586) * philox_ref.uniform(c[1])).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)


def hi_log_prob(goal, goal_mu, goal_std):
    """float64 [..]: Normal(goal_mu, goal_std).log_prob(goal).sum(-1) on float32 operands."""
    g, m, s = (np.asarray(a, np.float32).astype(np.float64) for a in (goal, goal_mu, goal_std))
    return (-0.5 * ((g - m) / s) ** 2 - np.log(s) - 0.5 * np.log(2 * np.pi)).sum(-1)
