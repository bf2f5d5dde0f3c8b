"""One zenv_collect_skill (the skill planner's / DIAYN's collect_experiences) at N = 500 and 65 536 for 25 zones (TSP)
and ColourMatch (6 zones), against the same frames with the three networks in host torch (float32, CPU): per frame the
download of obs / zone_obs, the high level at every window's first frame, the low level, zenv_step (step_no_reset inside
a window), the inverse model on the next observation.  h = 128, S = 5, skill_len = 20, T = 100, diversity_coef = 0.1.
The host side times the frame loop only (its GAEs and layout would add to it).

    python scripts/skill_collect_time.py [calls] [--device-only]
Prints one line per configuration: the device's ms per call and per frame; host-torch frames are fewer at 65 536 envs
(seconds each).  --device-only skips the host-torch comparison (for a run under rocprofv3 --kernel-trace --stats)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import combinatorial_rl_tasks_amd as Z   # noqa: E402
from tests import skill_ref   # noqa: E402
from tests.skill_collect_ref import inverse_log_softmax, random_inverse_state_dict   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(ARGS[0]) if ARGS else 5
DEVICE_ONLY = "--device-only" in sys.argv
S, L, T, COEF = 5, 20, 100, 0.1


def make(cfg, n, hi, lo, inv):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1, n, n_threads=16)
    env.schedule_sequential()
    env.reset()
    env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo), skill_len=L)
    env.load_skill_inverse(Z.inverse_tensors_from_state_dict(inv, S))
    return env


def host_frame(env, hi, lo, inv, prior_lp, skill, t):
    o, zo = env.observations()
    if t % L == 0:
        logits, _ = skill_ref.high(hi, o, zo)
        skill[:] = torch.distributions.Categorical(logits=torch.as_tensor(logits)).sample().numpy()
    mu, std, _ = skill_ref.low(lo, o, zo, skill, S)
    a = torch.distributions.Normal(torch.as_tensor(mu), torch.as_tensor(std)).sample().numpy()
    env.step(np.ascontiguousarray(a, np.float32), auto_reset=(t + 1) % L == 0)
    o2, zo2, r, d, _ = env.results()
    lp = inverse_log_softmax(inv, o2, zo2)
    div = (lp[np.arange(len(skill)), skill] - prior_lp[skill]) * (1 - d)
    return r + COEF * div


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # beyond that the shared host only thrashes
    torch.manual_seed(0)
    prior = np.zeros(S, np.float32)
    prior_lp = np.log(np.full(S, 1.0 / S, np.float32))
    for name, cfg in (("TSP Z=25", Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40)),
                      ("ColourMatch Z=6", Z.config_for_id("ColourMatch-v0"))):
        F = Z.zone_feat(cfg)
        hi, lo = skill_ref.random_state_dicts(F, S, h=128, seed=0)
        inv = random_inverse_state_dict(F, S, h=128, seed=1)
        for n in (500, 65536):
            env = make(cfg, n, hi, lo, inv)
            env.collect_skills_on_device(T, 1, 0, 0.99, 0.95, COEF, prior)           # allocations, warm-up
            env.sync()
            t0 = time.perf_counter()
            for c in range(CALLS):
                env.collect_skills_on_device(T, 2 + c, 0, 0.99, 0.95, COEF, prior)
            env.sync()
            dev = (time.perf_counter() - t0) / CALLS
            line = (f"{name:16s} N {n:6d}: device {dev * 1e3:9.2f} ms/call ({dev / T * 1e3:7.3f} ms/frame, "
                    f"{n * T / dev / 1e6:7.2f} M frames/s)")
            if not DEVICE_ONLY:
                skill = np.zeros(n, np.int64)
                k = 2 if n > 10000 else 20
                t0 = time.perf_counter()
                for t in range(k):
                    host_frame(env, hi, lo, inv, prior_lp, skill, t)
                host = (time.perf_counter() - t0) / k
                line += f"   host torch {host * 1e3:9.1f} ms/frame   ratio {host / (dev / T):7.1f}x"
            print(line, flush=True)
            env.close()


if __name__ == "__main__":
    main()
