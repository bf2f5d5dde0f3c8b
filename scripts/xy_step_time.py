"""One step of the xy-goals agent -- zenv_policy(POLICY_XY_SAMPLE) + zenv_step with auto-reset -- at N = 500 and 65 536
for 25 zones (TSP) and ColourMatch (6 zones), alternating in one run with the same step of the fixed-length-skills agent
(S = 5): 7 windows each, reported as median and min..max.  h = 128, random-init weights, a period of 200 for both.  And
the same xy step with both networks in host torch (float32, CPU): download obs / zone_obs / episode lengths, the high
level for the envs at a multiple of the period, the low level for every env, zenv_step(actions).

    python scripts/xy_step_time.py [steps per window] [--device-only]
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
from tests import skill_ref, xy_ref   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
STEPS = int(ARGS[0]) if ARGS else 50
DEVICE_ONLY = "--device-only" in sys.argv
S, PERIOD, WINDOWS = 5, 200, 7


def make(cfg, n):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1, n, n_threads=16)
    env.schedule_sequential()
    env.reset()
    return env


def window(env, policy):
    env.sync()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        env.policy(policy, policy_seed=1)
        env.step(None, auto_reset=True)
    env.sync()
    return (time.perf_counter() - t0) / STEPS


def host_step(env, hi, lo, goal):
    o, zo = env.observations()
    pick = env.get(nat.F_EP_LEN) % PERIOD == 0               # i % skill_len == 0, i counted from the reset
    if pick.any():
        idx = np.nonzero(pick)[0]
        mu, std, _ = xy_ref.high(hi, o[idx], zo[idx])
        goal[idx] = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(std)).sample().numpy()
    mu, std, _ = xy_ref.low(lo, o, zo, goal)
    a = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(std)).sample().numpy()
    env.step(np.ascontiguousarray(a, np.float32), auto_reset=True)


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return f"{np.median(ts):8.3f} ms/step ({ts.min():.3f} .. {ts.max():.3f})"


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # beyond that the shared host only thrashes
    torch.manual_seed(0)
    for name, cfg in (("TSP Z=25", Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40)),
                      ("ColourMatch Z=6", Z.config_for_id("ColourMatch-v0"))):
        F = Z.zone_feat(cfg)
        hi, lo = xy_ref.random_state_dicts(F, 128, 0)
        shi, slo = skill_ref.random_state_dicts(F, S, h=128, seed=0)
        for n in (500, 65536):
            xy, sk = make(cfg, n), make(cfg, n)
            xy.load_xy(Z.xy_tensors_from_state_dicts(hi, lo), skill_len=PERIOD)
            sk.load_skills(Z.skill_tensors_from_state_dicts(shi, slo), skill_len=PERIOD)
            runs = ((xy, nat.POLICY_XY_SAMPLE, []), (sk, nat.POLICY_SKILL_SAMPLE, []))
            for env, policy, _ in runs:                  # past the first picks of every env
                for _ in range(10):
                    env.policy(policy, policy_seed=1)
                    env.step(None, auto_reset=True)
            for _ in range(WINDOWS):
                for env, policy, ts in runs:
                    ts.append(window(env, policy))
            line = f"{name:16s} N {n:6d}: xy {spread(runs[0][2])}   skill {spread(runs[1][2])}"
            if not DEVICE_ONLY:
                goal = np.zeros((n, 2), np.float32)
                k = 3 if n > 10000 else 20
                t0 = time.perf_counter()
                for _ in range(k):
                    host_step(xy, hi, lo, goal)
                host = (time.perf_counter() - t0) / k
                line += f"   xy in host torch {host * 1e3:9.1f} ms/step   ratio {host / np.median(runs[0][2]):7.1f}x"
            print(line, flush=True)
            xy.close()
            sk.close()


if __name__ == "__main__":
    main()
