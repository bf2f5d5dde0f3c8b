"""One frame of zenv_collect_xy (the xy-goals agent's collect_experiences) against one step of the same agent driven
from the host -- zenv_policy(POLICY_XY_SAMPLE) + zenv_step, auto-reset on a window's last frame only -- at N = 500 and
65 536 for 25 zones (TSP) and ColourMatch (6 zones), h = 128, random-init weights, a period of 200 and T = 200 frames
per call (one window).  Both on the same box in the same run, alternating, REPEATS windows each; a collector window is
one or more whole calls, so its frames carry the call's fixed cost: the bootstrap pass of the high level over every env,
the low level under the bootstrap goal, the distance reward and both GAEs.

    python scripts/xy_collect_time.py [--quick] [--collect-only | --step-only]
Prints the median and the min .. max of the windows per variant, in ms per frame / per step.  --quick shortens the
windows (a rehearsal, not a measurement); --collect-only / --step-only run one of the two alone (for runs under
rocprofv3 --kernel-trace --stats, whose kernel names do not tell the two apart)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import combinatorial_rl_tasks_amd as Z   # noqa: E402
from combinatorial_rl_tasks_amd import _native as nat   # noqa: E402
from tests import xy_ref   # noqa: E402

QUICK = "--quick" in sys.argv
COLLECT_ONLY = "--collect-only" in sys.argv
STEP_ONLY = "--step-only" in sys.argv
PERIOD, T, REPEATS = 200, 200, 3 if QUICK else 7


def make(cfg, n, hi, lo):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1, n, n_threads=16)
    env.schedule_sequential()
    env.reset()
    env.load_xy(Z.xy_tensors_from_state_dicts(hi, lo), skill_len=PERIOD)
    return env


def step_window(env, steps):
    env.sync()
    t0 = time.perf_counter()
    for t in range(steps):
        env.policy(nat.POLICY_XY_SAMPLE, policy_seed=1)
        env.step(None, auto_reset=(t + 1) % PERIOD == 0)
    env.sync()
    return (time.perf_counter() - t0) / steps


def collect_window(env, calls):
    env.sync()
    t0 = time.perf_counter()
    for c in range(calls):
        env.collect_xy_on_device(T, 1 + c)
    env.sync()
    return (time.perf_counter() - t0) / (calls * T)


def fmt(ts):
    ts = np.array(ts) * 1e3
    return f"{np.median(ts):8.3f} ms ({ts.min():.3f} .. {ts.max():.3f})"


def main():
    for name, cfg in (("TSP Z=25", Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40)),
                      ("ColourMatch Z=6", Z.config_for_id("ColourMatch-v0"))):
        hi, lo = xy_ref.random_state_dicts(Z.zone_feat(cfg), 128, 0)
        for n in (500, 65536):
            calls = 1 if n > 10000 or QUICK else 5
            collector = None if STEP_ONLY else make(cfg, n, hi, lo)
            stepper = None if COLLECT_ONLY else make(cfg, n, hi, lo)
            if collector:
                collect_window(collector, 1)                 # warm-up: the allocations, every kernel
            if stepper:
                step_window(stepper, PERIOD)                 # a whole window, so that the next starts with the picks
            t_collect, t_step = [], []
            for _ in range(REPEATS):                          # alternating: what else runs on the box hits both alike
                if collector:
                    t_collect.append(collect_window(collector, calls))
                if stepper:
                    t_step.append(step_window(stepper, calls * T))
            print(f"{name}, N = {n}: {calls * T} frames x {REPEATS} windows, T = {T}, period {PERIOD}", flush=True)
            if collector:
                print(f"    {'zenv_collect_xy, per frame':36s} {fmt(t_collect)}", flush=True)
                collector.close()
            if stepper:
                print(f"    {'zenv_policy + zenv_step, per step':36s} {fmt(t_step)}", flush=True)
                stepper.close()


if __name__ == "__main__":
    main()
