"""One step of the Zone-goals hierarchical agent -- zenv_policy(POLICY_HIER_SAMPLE) + zenv_step -- at N = 500 and
65 536 for 25 zones (TSP) and ColourMatch (6 zones), against the same step with both networks in host torch (float32,
CPU): download obs / zone_obs / need-goal / available goals, the two forwards, zenv_set_goals, zenv_step(actions).

    python scripts/hier_step_time.py [steps] [--device-only]
Prints one line per configuration; host-torch steps are fewer at 65 536 envs (seconds each).  --device-only skips the
host-torch comparison (for a run under rocprofv3 --kernel-trace --stats)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import combinatorial_rl_tasks_amd as Z   # noqa: E402
from combinatorial_rl_tasks_amd import _native as nat   # noqa: E402
from tests import hier_ref   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
STEPS = int(ARGS[0]) if ARGS else 50
DEVICE_ONLY = "--device-only" in sys.argv


def make(cfg, n, hi, lo):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1, n, n_threads=16)
    env.schedule_sequential()
    env.enable_goals()
    env.reset()
    env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
    return env


def device_step(env, t):
    env.policy(nat.POLICY_HIER_SAMPLE, policy_seed=1)
    env.step(None, auto_reset=True)


def host_step(env, hi, lo):
    o, zo = env.observations()
    _, need, avail, goal = env.goal_info()
    new = np.full(env.num_envs, -1, np.int32)
    if need.any():
        idx = np.nonzero(need)[0]
        logits, _ = hier_ref.high(hi, o[idx], zo[idx], avail[idx])
        new[idx] = torch.distributions.Categorical(logits=torch.as_tensor(logits)).sample().numpy()
        env.set_goals(new)
        goal = np.where(need, new, goal)
    zg = zo[np.arange(env.num_envs), np.maximum(goal, 0), :2]
    mu, std, _ = hier_ref.low(lo, o, zo, zg)
    a = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(std)).sample().numpy()
    env.step(np.ascontiguousarray(a, np.float32), auto_reset=True)


def timed(fn, steps):
    t0 = time.perf_counter()
    for t in range(steps):
        fn(t)
    return (time.perf_counter() - t0) / steps


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # beyond that the shared host only thrashes
    torch.manual_seed(0)
    for name, cfg in (("TSP Z=25", Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40)),
                      ("ColourMatch Z=6", Z.config_for_id("ColourMatch-v0"))):
        hi, lo = hier_ref.random_state_dicts(Z.zone_feat(cfg), h=128, seed=0)
        for n in (500, 65536):
            env = make(cfg, n, hi, lo)
            for t in range(10):                      # past the first goal picks of every env
                device_step(env, t)
            env.sync()
            t0 = time.perf_counter()
            for t in range(STEPS):
                device_step(env, t)
            env.sync()
            dev = (time.perf_counter() - t0) / STEPS
            line = f"{name:16s} N {n:6d}: device {dev * 1e3:8.3f} ms/step ({n / dev / 1e6:7.2f} M env-steps/s)"
            if not DEVICE_ONLY:
                host = timed(lambda t: host_step(env, hi, lo), 3 if n > 10000 else 20)
                line += f"   host torch + set_goals {host * 1e3:9.1f} ms/step   ratio {host / dev:7.1f}x"
            print(line, flush=True)
            env.close()


if __name__ == "__main__":
    main()
