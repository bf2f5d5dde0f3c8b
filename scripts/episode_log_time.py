"""Time of the per-episode log pass (zenv_episode_log, episode_log.hip) beside the collection it follows.

    python scripts/episode_log_time.py [--quick] [--envs N] [--frames T] [--env ID]

Default: N = 65 536 envs of PointTSP-v0, T = 64 frames per collection, random networks of hidden size 64.  Two
collectors: zenv_collect (the flat actor-critic) and zenv_collect_skill (4 skills, windows of 8 frames, no inverse
model).  For each, REPEATS windows of CALLS calls after a warm-up window, wall clock around a synchronise: the
collection alone, and the collection followed by zenv_episode_log; median and min .. max in ms per call, their
difference, and the bytes the pass reads -- the mask in the counting walk; the mask, the reward arrays and the
diversity reward in the scattering walk.  Episodes are cut to 40 steps so that entries are appended (about 1.6 per env
and call).  --quick shortens the run (a rehearsal, not a measurement)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
H, S, L = 64, 4, 8


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def random_tensors(shapes, seed):
    rs = np.random.RandomState(seed)
    return {k: (rs.standard_normal(s) * (0.1 if "_b" in k else 1.0 / np.sqrt(s[-1]))).astype(np.float32)
            for k, s in shapes.items()}


def main():
    sys.path.insert(0, ROOT)
    import combinatorial_rl_tasks_amd as Z
    from combinatorial_rl_tasks_amd import agents

    n, T, env_id = arg("--envs", 65536), arg("--frames", 64), arg("--env", "PointTSP-v0", str)
    calls, repeats = (2, 2) if QUICK else (5, 5)
    for name in ("zenv_collect", "zenv_collect_skill"):
        env = Z.ZoneVecEnv(Z.config_for_id(env_id, num_steps=40), n)
        env.build_bank(1, 4096, n_threads=16)
        env.schedule_sequential()
        env.reset()
        F = env.zone_feat
        if name == "zenv_collect":
            shapes = {k: v for k, v in agents.mlp_tensor_shapes(H, F).items() if "sigma" not in k}
            env.load_mlp(random_tensors(shapes, 1))
            collect = lambda c: env.collect_on_device(T, policy_seed=c)                      # noqa: E731
            arrays = 1                                   # return and reshaped return read the same record
        else:
            env.load_skills(random_tensors(agents.skill_tensor_shapes(H, S, F), 2), skill_len=L)
            collect = lambda c: env.collect_skills_on_device(T, policy_seed=c)               # noqa: E731
            arrays = 2                                   # the env reward and the diversity reward
        read = T * n * 4 * (1 + 1 + arrays)

        def window(with_log):
            env.sync()
            t0 = time.perf_counter()
            done = 0
            for c in range(calls):
                collect(c)
                if with_log:
                    done += env.episode_log_on_device().done
            env.sync()
            return (time.perf_counter() - t0) / calls, done / calls

        window(True)
        alone = np.array([window(False)[0] for _ in range(repeats)]) * 1e3
        both = [window(True) for _ in range(repeats)]
        with_log = np.array([b[0] for b in both]) * 1e3
        stats_t0 = time.perf_counter()
        stats = env.episode_log_stats()
        stats_ms = (time.perf_counter() - stats_t0) * 1e3
        extra = np.median(with_log) - np.median(alone)
        print(f"{env_id}: {n} envs x {T} frames, {name}; {repeats} windows of {calls} calls", flush=True)
        print(f"    collection alone            {np.median(alone):10.2f} ms per call ({alone.min():.2f} .. {alone.max():.2f})")
        print(f"    collection + episode log    {np.median(with_log):10.2f} ms per call ({with_log.min():.2f} .. "
              f"{with_log.max():.2f}), {np.mean([b[1] for b in both]):.0f} entries per call")
        print(f"    the pass                    {extra:10.2f} ms per call = {100 * extra / np.median(alone):.2f} % of the "
              f"collection; it reads {read / 1e6:.1f} MB")
        print(f"    episode_log_stats           {stats_ms:10.2f} ms for {len(stats)} columns "
              f"(return mean {stats['return_per_episode']['mean']:.4f})", flush=True)
        env.close()


if __name__ == "__main__":
    main()
