"""One update of the fixed-length-skills agent's two levels on the device (ZoneVecEnv.skppo_update's calls:
zenv_skppo_epoch, ppo_update.hip) against the torch autograd updates of examples/skill_planner_ppo_torch.py, on the same
collected experience, at two shapes:

    example    4 096 procs x 100 frames, skill_len 20, minibatches of 16 384 (low) / 819 (high), 4 epochs each, h = 128,
               S = 5 skills
    reference  16 procs x 2 000 frames, skill_len 20, minibatches of 1 600 (low) / 80 (high)

The inverse model's and the skill prior's updates are not timed here: scripts/diayn_update_time.py times them.

Both on the same box in the same run, alternating, REPEATS windows each; a window is one whole update (high level, then
low level, then handing the parameters to the acting agent), wall clock around a synchronise.

    python scripts/skppo_update_time.py [--quick] [--device-only | --torch-only] [--shape example|reference]
Prints the median and the min .. max of the windows per variant in ms per update, and both updates' two levels apart.
--quick shortens the run (a rehearsal, not a measurement); --device-only / --torch-only run one path alone.

    python scripts/skppo_update_time.py --run-all OUT_DIR
starts one child process per shape, each under its own `timeout`, and stops at the first that fails."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
DEVICE_ONLY = "--device-only" in sys.argv
TORCH_ONLY = "--torch-only" in sys.argv
SHAPE = sys.argv[sys.argv.index("--shape") + 1] if "--shape" in sys.argv else None
REPEATS = 2 if QUICK else 7
# procs, frames, low-level batch, the child's time limit in seconds; the high level's batch is batch // skill_len
SHAPES = {"example": (4096, 100, 16384, 420), "reference": (16, 2000, 1600, 300)}
EPOCHS, HIDDEN, SKILL_LEN, N_SKILLS = 4, 128, 20, 5


def run_all(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    extra = [a for a in sys.argv[1:] if a in ("--quick", "--device-only", "--torch-only")]
    for name, shape in SHAPES.items():
        cmd = ["timeout", "-k", "10", str(shape[3]), sys.executable, os.path.abspath(__file__), "--shape", name] + extra
        with open(os.path.join(out_dir, f"skppo_update_time_{name}.txt"), "w") as out:
            rc = subprocess.run(cmd, stdout=out, stderr=subprocess.STDOUT).returncode
        print(open(out.name).read(), flush=True)
        if rc != 0:                      # a fault, an abort or a time limit: nothing more is started on the device
            print(f"{name}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


def fmt(ts):
    ts = np.array(ts) * 1e3
    return f"{np.median(ts):9.2f} ms per update ({ts.min():.2f} .. {ts.max():.2f})"


def main():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import combinatorial_rl_tasks_amd as Z
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    import skill_planner_ppo_torch as ex

    for name, (procs, frames, batch, _) in SHAPES.items():
        if SHAPE and name != SHAPE:
            continue
        env = Z.ZoneVecEnv("PointTSP-v0", procs)
        env.build_bank(1, 4 * procs, n_threads=16)
        env.schedule_sequential(stride=procs)
        tenv = TorchZoneEnv(env)
        tenv.reset()
        torch.manual_seed(1)
        hi_batch = max(1, batch // SKILL_LEN)
        algo = ex.SkillPlannerPPO(tenv, N_SKILLS, HIDDEN, SKILL_LEN, frames, diversity_coef=0.0, epochs=EPOCHS,
                                  batch_size=batch, hi_epochs=EPOCHS, hi_batch_size=hi_batch, seed=1)
        rng = np.random.default_rng(1)
        tenv.skppo_init(algo.hi_net.state_dict(), algo.lo_net.state_dict(), lo=dict(max_batch=batch),
                        hi=dict(max_batch=hi_batch))
        t_collect = []
        for c in range(2 if QUICK else 3):                 # the first call allocates
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tenv.load_skills(algo.hi_net.state_dict(), algo.lo_net.state_dict(), skill_len=SKILL_LEN)
            lo, hi, _, _ = tenv.collect_skills(frames, policy_seed=7 + c)
            torch.cuda.synchronize()
            t_collect.append(time.perf_counter() - t0)
        M = int(hi["action"].shape[0])
        n_lo = procs * frames
        split = []

        def device_window():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(EPOCHS):
                tenv.skppo_epoch(1, Z.hppo_batch_indexes(M, rng), hi_batch)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(EPOCHS):
                tenv.skppo_epoch(0, Z.hppo_batch_indexes(n_lo, rng), batch)
            tenv.skppo_publish()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            split.append((t1 - t0, t2 - t1))
            return t2 - t0

        t_torch_split = []

        def torch_window():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            algo.update_hi_parameters(hi)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            algo.update_lo_parameters(lo)
            tenv.load_skills(algo.hi_net.state_dict(), algo.lo_net.state_dict(), skill_len=SKILL_LEN)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            t_torch_split.append((t1 - t0, t2 - t1))
            return t2 - t0

        if not TORCH_ONLY:
            device_window()                                # warm-up: every kernel once
        if not DEVICE_ONLY:
            torch_window()
        split.clear()
        t_torch_split.clear()
        t_dev, t_torch = [], []
        for _ in range(REPEATS):                           # alternating: what else runs on the box hits both alike
            if not TORCH_ONLY:
                t_dev.append(device_window())
            if not DEVICE_ONLY:
                t_torch.append(torch_window())
        mb_lo, mb_hi = EPOCHS * -(-n_lo // batch), EPOCHS * -(-M // hi_batch)
        print(f"{name}: {procs} procs x {frames} frames, skill_len {SKILL_LEN}, low level {n_lo} samples in minibatches of "
              f"{batch}, high level M = {M} rows in minibatches of {hi_batch}, {EPOCHS} epochs each = {mb_lo} + {mb_hi} "
              f"minibatches per update, h = {HIDDEN}, S = {N_SKILLS}; {REPEATS} windows", flush=True)
        print(f"    {'load_skills + collect_skills (after 1st)':38s} {np.median(t_collect[1:]) * 1e3:9.2f} ms", flush=True)
        for label, ts, parts in (("device update + publish", t_dev, split), ("torch update + load_skills", t_torch, t_torch_split)):
            if ts:
                print(f"    {label:38s} {fmt(ts)}", flush=True)
                print(f"    {'  high level':38s} {fmt([p[0] for p in parts])}", flush=True)
                print(f"    {'  low level + hand-over':38s} {fmt([p[1] for p in parts])}", flush=True)
        if t_dev and t_torch:
            print(f"    device / torch, medians: {np.median(t_dev) / np.median(t_torch):.3f}", flush=True)
        env.close()


if __name__ == "__main__":
    if "--run-all" in sys.argv:
        sys.exit(run_all(sys.argv[sys.argv.index("--run-all") + 1]))
    main()
