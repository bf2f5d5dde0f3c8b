"""Time of one render launch (zenv_render, render.hip) beside the store-stream ceiling for the same bytes.

    python scripts/render_time.py [--quick] [--envs N] [--size S] [--env ID]

Default: 64 x 64 frames of all N = 65 536 envs of PointTSP-v0 after 40 greedy steps, into a device tensor: 805 MB per
launch.  A window is LAUNCHES launches enqueued back to back on the stream, wall clock around a synchronise, divided by
LAUNCHES; REPEATS windows after a warm-up one, median and min .. max printed in us per launch, with the bytes stored
per second.  Beside it, on the same box in the same run: ``zenv_probe_store_stream`` -- waves that do nothing but store
16 bytes per lane -- over the same number of bytes (one 12 288-byte tile per image), plain and non-temporal: what the
memory system takes for the stores alone.  --quick shortens the run (a rehearsal, not a measurement)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    sys.path.insert(0, ROOT)
    import combinatorial_rl_tasks_amd as Z
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv

    n, size, env_id = arg("--envs", 65536), arg("--size", 64), arg("--env", "PointTSP-v0", str)
    launches, repeats = (3, 2) if QUICK else (20, 7)
    env = Z.ZoneVecEnv(env_id, n)
    env.build_bank(1, 4096, n_threads=16)
    env.schedule_sequential()
    env.reset()
    env.rollout(40, Z.POLICY_GREEDY)
    tenv = TorchZoneEnv(env)
    frame_bytes = size * size * 3
    total = n * frame_bytes
    out = torch.empty((n, size, size, 3), dtype=torch.uint8, device=tenv.device)

    def window():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            tenv.render(width=size, height=size, marks=None, out=out)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / launches

    window()
    ts = np.array([window() for _ in range(repeats)]) * 1e6
    print(f"{env_id}: {n} envs x {size} x {size} x 3 = {total / 1e6:.1f} MB per launch; {repeats} windows of "
          f"{launches} launches", flush=True)
    print(f"    zenv_render                       {np.median(ts):10.1f} us per launch ({ts.min():.1f} .. {ts.max():.1f})"
          f"  = {total / np.median(ts) / 1e6:.2f} TB/s stored", flush=True)
    frame = out[n // 2].cpu().numpy()
    ref_colours = len({tuple(p) for p in frame.reshape(-1, 3)})
    print(f"    (env {n // 2}'s frame holds {ref_colours} distinct colours)", flush=True)
    del out
    torch.cuda.empty_cache()
    if frame_bytes % 16 == 0 and frame_bytes >= 1024:
        for name, policy in (("plain", 0), ("non-temporal", 2)):
            us = Z.vec_env.probe_store_stream(n, frame_bytes, steps=launches, cache_policy=policy, reps=repeats)
            print(f"    store stream, {name:13s}       {us:10.1f} us per pass over the same bytes"
                  f"               = {total / us / 1e6:.2f} TB/s", flush=True)
    else:
        print("    (the store-stream probe takes tiles of a multiple of 16 bytes, 1 KiB at least: not run)", flush=True)
    env.close()


if __name__ == "__main__":
    main()
