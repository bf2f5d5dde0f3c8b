"""One update of DIAYN's inverse model and skill prior on the device (TorchZoneEnv.diayn_update / diayn_prior_update /
diayn_publish: zenv_diayn_*, ppo_update.hip) against the torch updates of examples/skill_planner_ppo_torch.py
(update_inverse_parameters, update_skill_prior, then load_skill_inverse), on the same collected experience, at two shapes:

    example    4 096 procs x 100 frames, skill_len 20, minibatches of 16 384, inverse_epochs 4, h = 128, S = 5 skills
    reference  16 procs x 2 000 frames, skill_len 20, minibatches of 1 600

Both on the same box in the same run, alternating, REPEATS windows each; a window is one whole update (the kept list or
the boolean-mask compaction, the inverse model's epochs, the prior's step, handing the parameters to the acting
discriminator), wall clock around a synchronise.  The torch window compacts the samples as
``TorchZoneEnv.collect_skills`` does (a boolean mask over the [N, T-1] views), which is part of what the device path
replaces.

    python scripts/diayn_update_time.py [--quick] [--device-only | --torch-only] [--shape example|reference]
Prints the median and the min .. max of the windows per variant in ms per update.  --quick shortens the run (a rehearsal,
not a measurement).

    python scripts/diayn_update_time.py --run-all OUT_DIR
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
# procs, frames, batch, the child's time limit in seconds
SHAPES = {"example": (4096, 100, 16384, 300), "reference": (16, 2000, 1600, 240)}
EPOCHS, HIDDEN, SKILL_LEN, N_SKILLS = 4, 128, 20, 5


def run_all(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    extra = [a for a in sys.argv[1:] if a in ("--quick", "--device-only", "--torch-only")]
    for name, shape in SHAPES.items():
        cmd = ["timeout", "-k", "10", str(shape[3]), sys.executable, os.path.abspath(__file__), "--shape", name] + extra
        with open(os.path.join(out_dir, f"diayn_update_time_{name}.txt"), "w") as out:
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
        algo = ex.SkillPlannerPPO(tenv, N_SKILLS, HIDDEN, SKILL_LEN, frames, diversity_coef=0.1, epochs=EPOCHS,
                                  batch_size=batch, inverse_epochs=EPOCHS, inverse_batch_size=batch, seed=1)
        tenv.load_skills(algo.hi_net.state_dict(), algo.lo_net.state_dict(), skill_len=SKILL_LEN)
        tenv.load_skill_inverse(algo.inverse.state_dict(), N_SKILLS)
        tenv.diayn_init(algo.inverse.state_dict(), N_SKILLS, prior_logits=np.zeros(N_SKILLS, np.float32),
                        max_batch=batch)
        lo, hi, _, _ = tenv.collect_skills(frames, policy_seed=7, diversity_coef=0.1,
                                           skill_prior_logits=np.zeros(N_SKILLS, np.float32))
        torch.cuda.synchronize()
        kept = int(tenv.diayn_samples().numel())

        def device_window():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tenv.diayn_update(EPOCHS, batch, algo.gen)
            tenv.diayn_prior_update()
            tenv.diayn_publish()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def torch_window():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = lo["mask"][:, 1:] != 0
            inverse = {"obs": lo["obs"][:, 1:][keep], "zone_obs": lo["zone_obs"][:, 1:][keep],
                       "skill": lo["skill"][:, :-1][keep]}
            algo.update_inverse_parameters(inverse)
            algo.update_skill_prior(hi)
            tenv.load_skill_inverse(algo.inverse.state_dict(), N_SKILLS)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        if not TORCH_ONLY:
            device_window()                                # warm-up: every kernel once
        if not DEVICE_ONLY:
            torch_window()
        t_dev, t_torch = [], []
        for _ in range(REPEATS):                           # alternating: what else runs on the box hits both alike
            if not TORCH_ONLY:
                t_dev.append(device_window())
            if not DEVICE_ONLY:
                t_torch.append(torch_window())
        print(f"{name}: {procs} procs x {frames} frames, skill_len {SKILL_LEN}, {kept} kept samples of "
              f"{procs * (frames - 1)} in minibatches of {batch}, {EPOCHS} epochs = {EPOCHS * -(-kept // batch)} "
              f"minibatches per update, h = {HIDDEN}, S = {N_SKILLS}; {REPEATS} windows", flush=True)
        for label, ts in (("device inverse + prior + publish", t_dev),
                          ("torch inverse + prior + load_skill_inverse", t_torch)):
            if ts:
                print(f"    {label:44s} {fmt(ts)}", flush=True)
        if t_dev and t_torch:
            print(f"    device / torch, medians: {np.median(t_dev) / np.median(t_torch):.3f}", flush=True)
        env.close()


if __name__ == "__main__":
    if "--run-all" in sys.argv:
        sys.exit(run_all(sys.argv[sys.argv.index("--run-all") + 1]))
    main()
