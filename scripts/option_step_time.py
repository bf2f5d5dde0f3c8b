"""One step of the variable-length Options agent -- zenv_policy(POLICY_OPTION_SAMPLE) + zenv_step, auto-reset -- at
N = 500 and 65 536 for 25 zones (TSP) and ColourMatch (6 zones), h = 128, S = 5, random-init weights, with the measured
pick rate (the share of envs the high level runs for per step).  On the same box, in the same run:
  * both ways the high level finds its envs (ZENV_OPTION_COMPACT = 0: workgroups over env blocks that leave when no env
    of theirs picks; 1: workgroups over the compacted list of picking envs), alternating, REPEATS windows each;
  * the fixed-length-skills agent through POLICY_SKILL_SAMPLE at skill_len = 200 (almost no high level: the floor) and
    skill_len = 1 (every env picks on every step: the ceiling);
  * the same Options step with both networks in host torch (float32, CPU, 16 threads).

    python scripts/option_step_time.py [--device-only] [--quick]
Prints the median and the min .. max of the windows per variant.  --device-only skips the host-torch comparison (for a
run under rocprofv3 --kernel-trace --stats); --quick shortens the windows (a rehearsal, not a measurement)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import combinatorial_rl_tasks_amd as Z   # noqa: E402
from combinatorial_rl_tasks_amd import _native as nat   # noqa: E402
from tests import option_ref, skill_ref   # noqa: E402

DEVICE_ONLY = "--device-only" in sys.argv
QUICK = "--quick" in sys.argv
S, REPEATS = 5, 3 if QUICK else 7


def make(cfg, n):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1, n, n_threads=16)
    env.schedule_sequential()
    env.reset()
    return env


def window(env, policy, steps):
    env.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.policy(policy, policy_seed=1)
        env.step(None, auto_reset=True)
    env.sync()
    return (time.perf_counter() - t0) / steps


def host_step(env, hi, lo, skill):
    """evaluate_hier.py:63-75 with the networks on the host: download the observations, the high level for the envs
    without a skill, the low level for every env, the termination draw, zenv_step(actions)."""
    o, zo = env.observations()
    skill[env.get(nat.F_EP_LEN) == 0] = -1
    idx = np.nonzero(skill < 0)[0]
    if len(idx):
        logits, _ = option_ref.high(hi, o[idx], zo[idx])
        skill[idx] = torch.distributions.Categorical(logits=torch.as_tensor(logits)).sample().numpy()
    mu, std, _ = option_ref.low(lo, o, zo, skill, S)
    a = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(std)).sample()
    env.step(np.ascontiguousarray(a[:, :2].numpy(), np.float32), auto_reset=True)
    skill[(torch.rand(len(skill)) < torch.sigmoid(a[:, 2] * 4 - 3)).numpy()] = -1


def fmt(ts):
    ts = np.array(ts) * 1e3
    return f"{np.median(ts):8.3f} ms ({ts.min():.3f} .. {ts.max():.3f})"


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # beyond that the shared host only thrashes
    torch.manual_seed(0)
    for name, cfg in (("TSP Z=25", Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40)),
                      ("ColourMatch Z=6", Z.config_for_id("ColourMatch-v0"))):
        F = Z.zone_feat(cfg)
        hi, lo = option_ref.random_state_dicts(F, S, h=128, seed=0)
        shi, slo = skill_ref.random_state_dicts(F, S, h=128, seed=0)
        for n in (500, 65536):
            steps = (20 if n > 10000 else 200) if QUICK else (100 if n > 10000 else 2000)
            runs = []                                        # (label, env, policy)
            for compact in (0, 1):
                os.environ["ZENV_OPTION_COMPACT"] = str(compact)      # read by zenv_option_load
                env = make(cfg, n)
                env.load_options(Z.option_tensors_from_state_dicts(hi, lo))
                runs.append((f"options, {'compacted list' if compact else 'early exit'}", env, nat.POLICY_OPTION_SAMPLE))
            del os.environ["ZENV_OPTION_COMPACT"]
            for L, what in ((200, "floor"), (1, "ceiling")):
                env = make(cfg, n)
                env.load_skills(Z.skill_tensors_from_state_dicts(shi, slo), skill_len=L)
                runs.append((f"skills, skill_len {L} ({what})", env, nat.POLICY_SKILL_SAMPLE))
            for _, env, pol in runs:                          # warm-up: every kernel, past the first picks
                window(env, pol, 20)
            times = [[] for _ in runs]
            for _ in range(REPEATS):                          # alternating: what else runs on the box hits all alike
                for i, (_, env, pol) in enumerate(runs):
                    times[i].append(window(env, pol, steps))
            env = runs[1][1]
            rate = []
            for _ in range(20):
                env.policy(nat.POLICY_OPTION_SAMPLE, policy_seed=1)
                rate.append((env.get(nat.F_SKILL_AGE) == 1).mean())
                env.step(None, auto_reset=True)
            print(f"{name}, N = {n}: {steps} steps x {REPEATS} windows, pick rate {np.mean(rate):.4f} per step", flush=True)
            for (label, _, _), ts in zip(runs, times):
                print(f"    {label:32s} {fmt(ts)}", flush=True)
            if not DEVICE_ONLY:
                skill = np.full(n, -1, np.int64)
                k = 3 if n > 10000 else 20
                t0 = time.perf_counter()
                for _ in range(k):
                    host_step(env, hi, lo, skill)
                host = (time.perf_counter() - t0) / k
                dev = min(np.median(times[0]), np.median(times[1]))
                print(f"    {'options, host torch':32s} {host * 1e3:8.1f} ms   ratio {host / dev:7.1f}x", flush=True)
            for _, env, _ in runs:
                env.close()


if __name__ == "__main__":
    main()
