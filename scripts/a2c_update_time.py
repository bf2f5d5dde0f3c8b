"""One A2C update of the flat actor-critic on the device (ZoneVecEnv.a2c_update: zenv_a2c_update, ppo_update.hip)
against the torch autograd update of examples/ppo_torch.py (``a2c_update``: the same chunks, gradients accumulated by
autograd), on the same collected experience, at two shapes:

    example    4 096 procs x 64 frames in chunks of 16 384, h = 185, PointTSP-v0 (examples/ppo_torch.py --algo a2c)
    reference  16 procs x 8 frames in one chunk (A2CAlgo's default frames per proc, train_ppo.py's 16 procs)

Both on the same box in the same run, alternating, REPEATS windows each; a window is one whole update (every chunk, the
clip, the RMSprop step and handing the parameters to the acting network), wall clock around a synchronise.

    python scripts/a2c_update_time.py [--quick] [--device-only | --torch-only] [--shape example|reference]
Prints the median and the min .. max of the windows per variant, in ms per update and per chunk.  --quick shortens the
run (a rehearsal, not a measurement); --device-only / --torch-only run one path alone (for runs under rocprofv3
--kernel-trace --stats)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import combinatorial_rl_tasks_amd as Z   # noqa: E402
from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv   # noqa: E402
import ppo_torch   # noqa: E402

QUICK = "--quick" in sys.argv
DEVICE_ONLY = "--device-only" in sys.argv
TORCH_ONLY = "--torch-only" in sys.argv
SHAPE = sys.argv[sys.argv.index("--shape") + 1] if "--shape" in sys.argv else None
REPEATS = 2 if QUICK else 7
SHAPES = {"example": (4096, 64, 16384), "reference": (16, 8, 128)}
HIDDEN = 185
HYPER = dict(lr=0.01, rmsprop_alpha=0.99, rmsprop_eps=1e-8, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=0.5)


def fmt(ts, per):
    ts = np.array(ts) * 1e3
    return (f"{np.median(ts):9.2f} ms per update ({ts.min():.2f} .. {ts.max():.2f}), "
            f"{np.median(ts) / per:8.3f} ms per chunk")


def main():
    dev = torch.device("cuda", 0)
    for name, (procs, frames, batch) in SHAPES.items():
        if SHAPE and name != SHAPE:
            continue
        env = Z.ZoneVecEnv("PointTSP-v0", procs)
        env.build_bank(1, 4 * procs, n_threads=16)
        env.schedule_sequential(stride=procs)
        tenv = TorchZoneEnv(env)
        tenv.reset()
        torch.manual_seed(1)
        model = ppo_torch.ActorCritic(env.zone_feat, HIDDEN).to(dev)
        opt = torch.optim.RMSprop(model.parameters(), HYPER["lr"], alpha=HYPER["rmsprop_alpha"], eps=HYPER["rmsprop_eps"])
        tenv.load_state_dict(model.state_dict())
        tenv.a2c_init(model.state_dict(), max_batch=batch, **HYPER)
        exps = tenv.collect(frames, policy_seed=7)
        torch.cuda.synchronize()
        chunks = -(-procs * frames // batch)

        def device_window():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tenv.a2c_update()
            tenv.a2c_publish()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def torch_window():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ppo_torch.a2c_update(model, opt, exps, batch, HYPER["entropy_coef"], HYPER["value_loss_coef"],
                                 HYPER["max_grad_norm"])
            tenv.load_state_dict(model.state_dict())
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        if not TORCH_ONLY:
            device_window()                                # warm-up: every kernel once, the index list uploaded
        if not DEVICE_ONLY:
            torch_window()
        t_dev, t_torch = [], []
        for _ in range(REPEATS):                           # alternating: what else runs on the box hits both alike
            if not TORCH_ONLY:
                t_dev.append(device_window())
            if not DEVICE_ONLY:
                t_torch.append(torch_window())
        print(f"{name}: {procs} procs x {frames} frames = {procs * frames} frames in {chunks} chunks of {batch}, "
              f"h = {HIDDEN}; {REPEATS} windows", flush=True)
        if t_dev:
            print(f"    {'device update + publish':34s} {fmt(t_dev, chunks)}", flush=True)
        if t_torch:
            print(f"    {'torch update + load_state_dict':34s} {fmt(t_torch, chunks)}", flush=True)
        env.close()


if __name__ == "__main__":
    main()
