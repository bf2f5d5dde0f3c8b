"""One frame of zenv_collect_option (the Options agent's collect_experiences) against one step of the same agent driven
from the host -- zenv_policy(POLICY_OPTION_SAMPLE) + zenv_step, auto-reset -- at N = 500 and 65 536 for 25 zones (TSP)
and ColourMatch (6 zones), h = 128, S = 5, random-init weights, T = 100 frames per call.  Both on the same box in the same
run, alternating, REPEATS windows each (the sizes and the method of scripts/option_step_time.py); a collector window is
one or more whole calls, so its frames carry the call's fixed cost: the bootstrap value, both GAEs, the row scan, the
gather, the carry and the one synchronisation.

    python scripts/option_collect_time.py [--quick] [--collect-only | --step-only]
Prints the median and the min .. max of the windows per variant, in ms per frame / per step, and the rows per call.
--quick shortens the windows (a rehearsal, not a measurement); --collect-only / --step-only run one of the two alone (for
runs under rocprofv3 --kernel-trace --stats, whose kernel names do not tell the two apart)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import combinatorial_rl_tasks_amd as Z   # noqa: E402
from combinatorial_rl_tasks_amd import _native as nat   # noqa: E402
from tests import option_ref   # noqa: E402

QUICK = "--quick" in sys.argv
COLLECT_ONLY = "--collect-only" in sys.argv
STEP_ONLY = "--step-only" in sys.argv
S, T, REPEATS = 5, 100, 3 if QUICK else 7


def make(cfg, n, hi, lo):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1, n, n_threads=16)
    env.schedule_sequential()
    env.reset()
    env.load_options(Z.option_tensors_from_state_dicts(hi, lo))
    return env


def step_window(env, steps):
    env.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.policy(nat.POLICY_OPTION_SAMPLE, policy_seed=1)
        env.step(None, auto_reset=True)
    env.sync()
    return (time.perf_counter() - t0) / steps


def collect_window(env, calls, rows):
    env.sync()
    t0 = time.perf_counter()
    for c in range(calls):
        rows.append(env.collect_options_on_device(T, 1 + c)[1])
    env.sync()
    return (time.perf_counter() - t0) / (calls * T)


def fmt(ts):
    ts = np.array(ts) * 1e3
    return f"{np.median(ts):8.3f} ms ({ts.min():.3f} .. {ts.max():.3f})"


def main():
    for name, cfg in (("TSP Z=25", Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40)),
                      ("ColourMatch Z=6", Z.config_for_id("ColourMatch-v0"))):
        hi, lo = option_ref.random_state_dicts(Z.zone_feat(cfg), S, h=128, seed=0)
        for n in (500, 65536):
            calls = (1 if QUICK else 2) if n > 10000 else (2 if QUICK else 20)
            collector = None if STEP_ONLY else make(cfg, n, hi, lo)
            stepper = None if COLLECT_ONLY else make(cfg, n, hi, lo)
            rows = []
            if collector:
                collect_window(collector, 1, rows)           # warm-up: the allocations, every kernel
                del rows[:]
            if stepper:
                step_window(stepper, 20)
            t_collect, t_step = [], []
            for _ in range(REPEATS):                          # alternating: what else runs on the box hits both alike
                if collector:
                    t_collect.append(collect_window(collector, calls, rows))
                if stepper:
                    t_step.append(step_window(stepper, calls * T))
            print(f"{name}, N = {n}: {calls * T} frames x {REPEATS} windows, T = {T}, {np.mean(rows) if rows else 0:.0f} rows per call",
                  flush=True)
            if collector:
                print(f"    {'zenv_collect_option, per frame':36s} {fmt(t_collect)}", flush=True)
                collector.close()
            if stepper:
                print(f"    {'zenv_policy + zenv_step, per step':36s} {fmt(t_step)}", flush=True)
                stepper.close()


if __name__ == "__main__":
    main()
