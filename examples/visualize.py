"""Watch an agent: the loop of the reference's ``scripts/visualize.py`` (``env.render(); action = agent.get_action(obs);
env.step(action)``) with the frames drawn on the device by ``ZoneVecEnv.render`` -- a top-down drawing of what the
agent observes, not MuJoCo's camera -- and written as an animation instead of shown in a window.

    python examples/visualize.py --env PointTSP-v1 --policy greedy --episodes 1
    python examples/visualize.py --env PointTSP-v0 --model storage/my_run --episodes 3 --out run.gif

``--model DIR`` names a reference model directory (or its ``status.pt``), loaded as ``evaluate()`` loads it: the actor
runs on the device in float32 and samples its actions as ``utils.Agent.get_action`` does (``--argmax``: the mean).
``--policy greedy`` / ``uniform`` are the library's scripted action sources.  One env is stepped; episode k runs on the
map of env seed ``--env-seed`` + k.  The file is an animated GIF when PIL can be imported, else the frames as an
``.npy`` array [frames, size, size, 3].
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import combinatorial_rl_tasks_amd as Z  # noqa: E402
from combinatorial_rl_tasks_amd.evaluate import EVAL_SEED0, load_model_state  # noqa: E402


def run(args):
    env = Z.ZoneVecEnv(args.env, 1, device=args.device)
    if args.model:
        tensors = Z.mlp_tensors_from_state_dict(load_model_state(args.model))
        policy = Z.POLICY_MLP_MEAN if args.argmax else Z.POLICY_MLP_SAMPLE
    else:
        policy = {"greedy": Z.POLICY_GREEDY, "uniform": Z.POLICY_UNIFORM}[args.policy]
    frames = []
    for episode in range(args.episodes):
        env.build_bank(args.env_seed + episode, 1, n_threads=1)
        env.schedule_sequential()
        env.reset()
        if args.model and episode == 0:
            env.load_mlp(tensors, precision="f32")
        total, steps = 0.0, 0
        while True:
            if steps % args.stride == 0:
                frames.append(env.render(width=args.size, height=args.size)[0])
            env.policy(policy, policy_seed=args.seed)
            env.step(None, auto_reset=False)
            _, _, reward, done, goal_met = env.results()
            total += float(reward[0]) * 0.99 ** steps
            steps += 1
            if done[0] or steps >= args.max_steps:
                frames.append(env.render(width=args.size, height=args.size)[0])
                print("%s --- Total reward: %.3f --- Eps len: %d" % ("Success!" if goal_met[0] else "Fail!", total, steps))
                break
    env.close()
    return np.stack(frames)


def write(frames, out, ms_per_frame):
    try:
        from PIL import Image
    except ImportError:
        out = os.path.splitext(out)[0] + ".npy"
        np.save(out, frames)
        return out
    images = [Image.fromarray(f, "RGB") for f in frames]
    images[0].save(out, save_all=True, append_images=images[1:], duration=ms_per_frame, loop=0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", required=True, help="registry id, e.g. PointTSP-v1")
    ap.add_argument("--model", default=None, help="a reference model directory or status.pt")
    ap.add_argument("--policy", choices=("greedy", "uniform"), default=None, help="a scripted policy instead of --model")
    ap.add_argument("--argmax", action="store_true", help="with --model: act with the mean instead of sampling")
    ap.add_argument("--seed", type=int, default=0, help="seed of the action source")
    ap.add_argument("--env-seed", type=int, default=EVAL_SEED0, help="env seed of the first episode's map")
    ap.add_argument("--episodes", type=int, default=10, help="number of episodes to visualize")
    ap.add_argument("--size", type=int, default=200, help="frame width and height in pixels")
    ap.add_argument("--stride", type=int, default=4, help="draw every stride-th step")
    ap.add_argument("--max-steps", type=int, default=1 << 30, help="cut an episode after this many steps")
    ap.add_argument("--pause", type=float, default=0.04, help="seconds per frame of the animation")
    ap.add_argument("--out", default="visualize.gif")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if (args.model is None) == (args.policy is None):
        ap.error("give exactly one of --model and --policy")
    if args.episodes < 1 or args.stride < 1 or args.size < 1:
        ap.error("--episodes, --stride and --size must be positive")
    frames = run(args)
    path = write(frames, args.out, int(round(1000 * args.pause)))
    print(f"{len(frames)} frames of {args.size} x {args.size} -> {path}")


if __name__ == "__main__":
    main()
