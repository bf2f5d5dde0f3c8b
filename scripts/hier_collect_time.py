"""Zone-goals experience collection (HierPolicyAlgo.collect_experiences): ZoneVecEnv.collect_hier -- every frame's
goal pick, low-level action, step and the semi-Markov bookkeeping on the device, one synchronisation per call --
against the same frames driven from the host: zenv_policy(POLICY_HIER_SAMPLE) + zenv_step on the device, and after
every frame the records downloaded (obs, zone_obs, goals, the high critic's value and logits, actions, mu / std /
value, rewards, done, need_next_goal) and the transitions kept in numpy, then both GAE recursions in numpy.  h = 128,
N = 500 and 65 536, TSP with 25 zones and ColourMatch.

    python scripts/hier_collect_time.py [frames_per_proc] [--device-only]
--device-only skips the host-driven loop (for a run under rocprofv3 --kernel-trace --stats)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import combinatorial_rl_tasks_amd as Z   # noqa: E402
from combinatorial_rl_tasks_amd import _native as nat   # noqa: E402
from tests import hier_ref   # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
T = int(ARGS[0]) if ARGS else 64
DEVICE_ONLY = "--device-only" in sys.argv


def make(cfg, n, hi, lo):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1, n, n_threads=16)
    env.schedule_sequential()
    env.enable_goals()
    env.reset()
    env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
    return env


def host_collect(env, T, state, discount=0.99, lam=0.95):
    """The same call driven from the host; state = (hi_reward, open transitions) carried between calls."""
    n = env.num_envs
    hi_reward, open_tr = state
    rec = {k: [] for k in ("obs", "zone_obs", "goal", "action", "value", "reward", "mask")}
    closed = [[] for _ in range(n)]
    mask = np.ones(n, np.float32)
    for _ in range(T):
        o, zo = env.observations()
        _, need, avail, _ = env.goal_info()
        env.policy(nat.POLICY_HIER_SAMPLE, policy_seed=1)
        goal, hv, logits = env.get(nat.F_GOAL), env.get(nat.F_HIER_VALUE), env.get(nat.F_HIER_LOGITS)
        for j in np.nonzero(need & (goal >= 0))[0]:
            open_tr[j] = (o[j], zo[j], goal[j], avail[j], hv[j], logits[j])
        rec["obs"].append(o)
        rec["zone_obs"].append(zo)
        rec["goal"].append(goal)
        rec["action"].append(env.get(nat.F_ACTIONS))
        rec["value"].append(env.get(nat.F_POLICY_VALUE))
        rec["mask"].append(mask)
        env.step(None, auto_reset=True)
        _, _, r, d, _ = env.results()
        sh, need_after, _, _ = env.goal_info()
        rec["reward"].append(sh.astype(np.float32))
        mask = 1.0 - d.astype(np.float32)
        hi_reward += r
        for j in np.nonzero(need_after)[0]:
            if open_tr[j] is not None:
                closed[j].append(open_tr[j] + (hi_reward[j], 0.0 if d[j] else 1.0))
                open_tr[j] = None
            hi_reward[j] = 0
    v, rw, m = (np.stack(rec[k]) for k in ("value", "reward", "mask"))
    adv = np.zeros_like(v)
    for i in reversed(range(T - 1)):
        delta = rw[i] + discount * v[i + 1] * m[i + 1] - v[i]
        adv[i] = delta + discount * lam * adv[i + 1] * m[i + 1]
    for j in range(n):
        an, vn = 0.0, 0.0
        for tr in reversed(closed[j]):
            delta = tr[6] + vn * tr[7] - tr[4]
            an = delta + lam * an * tr[7]
            vn = tr[4]
    return sum(len(c) for c in closed)


def main():
    for name, cfg in (("TSP Z=25", Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40)),
                      ("ColourMatch Z=6", Z.config_for_id("ColourMatch-v0"))):
        hi, lo = hier_ref.random_state_dicts(Z.zone_feat(cfg), h=128, seed=0)
        for n in (500, 65536):
            env = make(cfg, n, hi, lo)
            env.collect_hier_on_device(T)                # allocations and the first goal picks
            t0 = time.perf_counter()
            _, m = env.collect_hier_on_device(T)
            dev = time.perf_counter() - t0
            line = (f"{name:16s} N {n:6d} T {T}: collect_hier {dev / T * 1e3:7.3f} ms/frame "
                    f"({n * T / dev / 1e6:7.2f} M frames/s, M = {m})")
            if not DEVICE_ONLY:
                state = (np.zeros(n, np.float32), [None] * n)
                host_collect(env, 2, state)
                t0 = time.perf_counter()
                host_collect(env, T, state)
                host = time.perf_counter() - t0
                line += f"   host-driven {host / T * 1e3:8.2f} ms/frame ({n * T / host / 1e6:6.2f} M frames/s)  ratio {host / dev:6.1f}x"
            print(line, flush=True)
            env.close()


if __name__ == "__main__":
    main()
