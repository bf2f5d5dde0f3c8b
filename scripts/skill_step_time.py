"""One step of the fixed-length-skills agent -- zenv_policy(POLICY_SKILL_SAMPLE) + zenv_step -- at N = 500 and 65 536
for 25 zones (TSP) and ColourMatch (6 zones), against the same step with both networks in host torch (float32, CPU):
download obs / zone_obs / episode lengths, the high level for the envs at a multiple of skill_len, the low level for
every env, zenv_step(actions).  h = 128, S = 5, skill_len = 200 (evaluate_hier.py).

    python scripts/skill_step_time.py [steps] [--device-only]
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
from tests import skill_ref   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
STEPS = int(ARGS[0]) if ARGS else 50
DEVICE_ONLY = "--device-only" in sys.argv
S, SKILL_LEN = 5, 200


def make(cfg, n, hi, lo):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1, n, n_threads=16)
    env.schedule_sequential()
    env.reset()
    env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo), skill_len=SKILL_LEN)
    return env


def device_step(env, t):
    env.policy(nat.POLICY_SKILL_SAMPLE, policy_seed=1)
    env.step(None, auto_reset=True)


def host_step(env, hi, lo, skill):
    o, zo = env.observations()
    pick = env.get(nat.F_EP_LEN) % SKILL_LEN == 0            # i % skill_len == 0, i counted from the reset
    if pick.any():
        idx = np.nonzero(pick)[0]
        logits, _ = skill_ref.high(hi, o[idx], zo[idx])
        skill[idx] = torch.distributions.Categorical(logits=torch.as_tensor(logits)).sample().numpy()
    mu, std, _ = skill_ref.low(lo, o, zo, skill, S)
    a = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(std)).sample().numpy()
    env.step(np.ascontiguousarray(a, np.float32), auto_reset=True)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # beyond that the shared host only thrashes
    torch.manual_seed(0)
    for name, cfg in (("TSP Z=25", Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40)),
                      ("ColourMatch Z=6", Z.config_for_id("ColourMatch-v0"))):
        hi, lo = skill_ref.random_state_dicts(Z.zone_feat(cfg), S, h=128, seed=0)
        for n in (500, 65536):
            env = make(cfg, n, hi, lo)
            for t in range(10):                      # past the first skill picks of every env
                device_step(env, t)
            env.sync()
            t0 = time.perf_counter()
            for t in range(STEPS):
                device_step(env, t)
            env.sync()
            dev = (time.perf_counter() - t0) / STEPS
            line = f"{name:16s} N {n:6d}: device {dev * 1e3:8.3f} ms/step ({n / dev / 1e6:7.2f} M env-steps/s)"
            if not DEVICE_ONLY:
                skill = np.zeros(n, np.int64)
                k = 3 if n > 10000 else 20
                t0 = time.perf_counter()
                for t in range(k):
                    host_step(env, hi, lo, skill)
                host = (time.perf_counter() - t0) / k
                line += f"   host torch {host * 1e3:9.1f} ms/step   ratio {host / dev:7.1f}x"
            print(line, flush=True)
            env.close()


if __name__ == "__main__":
    main()
