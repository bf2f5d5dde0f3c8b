"""Record the `logs` the reference's own collect_experiences return, as fixtures for tests/test_episode_log_ref_cpu.py.

Like make_agent_goldens.py (whose stand-in modules, toy environments and network builders this script imports and does
not change) it runs the reference's agent code at run time over scripted toy environments and stores only data: per
frame the env reward, the shaped reward, done and -- for DIAYN -- the diversity reward, and per call the returned
``logs``.  Five collectors, three consecutive calls each:

    base         BaseAlgo.collect_experiences (main), 6 procs, T = 8
    skills       main's HierPolicyAlgo with an inverse model, 5 procs, T = 8, skill_len = 4
    zone_goals   zone-goals' HierPolicyAlgo, 6 procs, T = 8
    options      options' HierPolicyAlgo, 6 procs, T = 8
    xy_goals     xy-goals' HierPolicyAlgo, 5 procs, T = 8, skill_len = 4

The environments are scripted so that the first call ends no episode, the second ends more than num_procs, episodes
span two calls, and -- under windows -- an env ends in the middle of a window and idles, and another on a window's last
frame; the counts are asserted from the stream the collector consumed.  The diversity reward is taken from a forward
hook on the inverse model and recomputed with the reference's own expression (main/src/torch_ac/algos/
_hier_policy_opt.py:84-89).

    python tests/golden/make_episode_log_goldens.py        writes tests/golden/episode_log_<variant>.npz

Not collected by pytest; the tests read only the .npz files.
"""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_agent_goldens as M  # noqa: E402

CALLS = 3
T, L = 8, 4
# step counters over an env's whole life at which its episodes end (ToyEnv.done_at); an idle env's counter stands still
FLAT_DONE = [(9, 10, 11), (12, 16), (13,), (16,), (20,), ()]
WINDOW_DONE = [(9, 13, 15), (10, 12), (12, 14), (20,), ()]
REACH = [(), (2,), (4, 10), (5,), (18,), (3,)]
LOG_KEYS = ("return_per_episode", "reshaped_return_per_episode", "num_frames_per_episode", "diversity_per_episode",
            "prediction_per_episode")
ITEMS = {"main": ("base", "skills"), "zone-goals": ("zone_goals",), "options": ("options",), "xy-goals": ("xy_goals",)}


def drive(out, item, algo, N, skill_len=None, inverse=None):
    """CALLS calls of algo.collect_experiences; the stream it consumed and the logs it returned into out[item/...]."""
    import torch
    import torch.nn.functional as F
    log = []
    M.log_calls(algo.env, ("step", "step_no_reset") if skill_len else ("step",), log)
    logits = []
    handle = inverse.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone())) if inverse else None
    M.seed_all(90)
    diversity = []
    for call in range(CALLS):
        n_logits = len(logits)
        logs = algo.collect_experiences()[1]
        for k in LOG_KEYS:
            if k in logs:
                out[f"{item}/call{call}/{k}"] = np.array(logs[k], np.float64)
        # options also reports termination_rate, a scalar of the call's termination draws and no episode log: not kept
        assert set(logs) - {"num_frames", "termination_rate"} <= set(LOG_KEYS), sorted(logs)
        out[f"{item}/call{call}/keys"] = np.array(sorted(logs))
        out[f"{item}/call{call}/num_frames"] = np.int64(logs["num_frames"])
        if inverse:
            assert len(logits) - n_logits == T
            steps = [x for x in log if x[0] != "reset"][call * T:(call + 1) * T]
            for i in range(T):
                done = torch.tensor(steps[i][2][2])
                skills = algo.hi_actions[i // skill_len].long()
                log_probs = F.log_softmax(logits[n_logits + i], dim=-1)
                d = (log_probs[torch.arange(N), skills] - F.log_softmax(algo.skill_logits, dim=0)[skills]) * ~done
                diversity.append(M.np_of(d).astype(np.float32))
    if handle:
        handle.remove()
    steps = [x for x in log if x[0] != "reset"]
    assert len(steps) == CALLS * T
    reward = np.array([s[2][1] for s in steps], np.float64)
    assert np.array_equal(reward, reward.astype(np.float32))
    done = np.array([s[2][2] for s in steps], bool)
    out[f"{item}/reward"] = reward.astype(np.float32)
    out[f"{item}/done"] = done
    out[f"{item}/shape"] = np.array([N, T, skill_len or 0, CALLS], np.int64)
    if item == "base":
        out[f"{item}/shaped_reward"] = np.array([[i["shaped_reward"] for i in s[2][3]] for s in steps], np.float32)
    if inverse:
        out[f"{item}/diversity"] = np.stack(diversity)
        assert np.any(out[f"{item}/diversity"] != 0)
    # the scripted cases, from the stream
    frame = np.arange(CALLS * T)
    if skill_len:
        idle = done & np.concatenate([np.zeros((1, N), bool), done[:-1] & ((frame[:-1] % skill_len) != skill_len - 1)[:, None]])
    else:
        idle = np.zeros_like(done)
    first = done & ~idle
    per_call = first.reshape(CALLS, T, N).sum(axis=(1, 2))
    assert per_call[0] == 0 and per_call[1] > N and per_call[2] > 0, per_call
    assert [len(out[f"{item}/call{c}/return_per_episode"]) for c in range(CALLS)] == [max(int(d), N) for d in per_call]
    assert (first.sum(axis=0) == 0).any()                                   # an env that never ends
    assert first[T:2 * T].any(axis=0).sum() >= 3                            # episodes that began in call 0 end in call 1
    if skill_len:
        assert idle.any() and first[(frame % skill_len) == skill_len - 1].any() \
            and first[(frame % skill_len) < skill_len - 1].any()
    print(f"{item}: episode ends per call {per_call.tolist()}, idle frames {int(idle.sum())}")


def child(variant, path):
    import torch
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    spaces = M.enter_variant(variant)
    import torch_ac
    rec = M.Recorder("f32")                                  # what the imported builders record is not kept
    f32, cpu, h = torch.float32, torch.device("cpu"), M.ZG_HYPER
    out = {}
    if variant == "main":
        from envs.wrappers import WaitWrapper
        model, Z, F, dist_value = M.flat_networks(rec, spaces, f32)["plain"]
        assert M.FLAT_NT == (len(FLAT_DONE), T)
        drive(out, "base", M.flat_algo(spaces, model, Z, F, dist_value, f32, FLAT_DONE, batch_size=16), len(FLAT_DONE))
        torch.set_default_dtype(f32)
        M.seed_all(7)
        Z, F = M.TSP
        hi, lo = M.skill_family_networks(rec, spaces, "skills", M.TSP, f32)
        inverse = M.inverse_network(rec, spaces, f32)
        logits0 = 0.3 * torch.randn(M.N_SKILLS, generator=torch.Generator().manual_seed(M.SEED + 8), dtype=f32)
        N = len(WINDOW_DONE)
        envs = [WaitWrapper(M.ToyEnv(spaces, j, Z, F, WINDOW_DONE[j])) for j in range(N)]
        algo = torch_ac.algos.HierPolicyAlgo(envs, hi, lo, inverse, logits0.clone(), cpu, M.widening(spaces, Z, F, f32),
                                             True, True, 1, 20, T, h["lr"], h["gae_lambda"], h["entropy_coef"],
                                             h["discount"], h["value_loss_coef"], 0.1, h["clip_eps"], 1, 10,
                                             h["hi_entropy_coef"], h["hi_value_coef"], h["hi_lr"], 1, 16, 3e-4,
                                             h["max_grad_norm"], h["optim_eps"], L, M.N_SKILLS)
        drive(out, "skills", algo, N, L, inverse)
    elif variant == "zone-goals":
        from hier_policy_value_models import HighPolicyValueModel, LoPolicyValueModel
        from utils.format import get_obss_preprocessor
        Z, F = M.TSP
        M.seed_all(3)
        obs_space, action_space = M.spaces_for(spaces, Z, F)
        shapes, _ = get_obss_preprocessor(obs_space)
        hi = HighPolicyValueModel(dict(shapes), Z, M.H)
        lo = LoPolicyValueModel(dict(shapes), action_space, 2, M.H)
        N = len(FLAT_DONE)
        envs = [M.ToyGoalEnv(spaces, j, Z, F, FLAT_DONE[j], REACH[j]) for j in range(N)]
        algo = torch_ac.algos.HierPolicyAlgo(envs, hi, lo, cpu, M.widening(spaces, Z, F, f32), 1, 20, T, h["lr"],
                                             h["gae_lambda"], h["entropy_coef"], h["discount"], h["value_loss_coef"],
                                             h["clip_eps"], 1, 12, h["hi_entropy_coef"], h["hi_value_coef"], h["hi_lr"],
                                             h["max_grad_norm"], h["optim_eps"])
        drive(out, "zone_goals", algo, N)
    elif variant == "options":
        from envs.wrappers import WaitWrapper
        Z, F = M.CM
        M.seed_all(5)
        hi, lo = M.skill_family_networks(rec, spaces, "options", M.CM, f32)
        N = len(FLAT_DONE)
        envs = [WaitWrapper(M.ToyEnv(spaces, j, Z, F, FLAT_DONE[j])) for j in range(N)]
        algo = torch_ac.algos.HierPolicyAlgo(envs, hi, lo, cpu, M.widening(spaces, Z, F, f32), True, True, 1, 20, T,
                                             h["lr"], h["gae_lambda"], h["entropy_coef"], h["discount"],
                                             h["value_loss_coef"], h["clip_eps"], 1, 10, h["hi_entropy_coef"],
                                             h["hi_value_coef"], h["hi_lr"], h["max_grad_norm"], h["optim_eps"],
                                             M.N_SKILLS)
        drive(out, "options", algo, N)
    else:
        from envs.wrappers import WaitWrapper
        from hier_policy_value_models import HighPolicyValueModel, LoPolicyValueModel
        Z, F = M.CM
        M.seed_all(4)
        obs_space, action_space = M.spaces_for(spaces, Z, F)
        shapes = {k: v.shape for k, v in obs_space.spaces.items()}
        hi = HighPolicyValueModel(dict(shapes), M.H)
        lo = LoPolicyValueModel(dict(shapes), action_space, M.H)
        N = len(WINDOW_DONE)
        envs = [WaitWrapper(M.ToyEnv(spaces, j, Z, F, WINDOW_DONE[j])) for j in range(N)]
        algo = torch_ac.algos.HierPolicyAlgo(envs, hi, lo, cpu, M.widening(spaces, Z, F, f32), 1, 20, T, h["lr"],
                                             h["gae_lambda"], h["entropy_coef"], h["discount"], h["value_loss_coef"],
                                             h["clip_eps"], 1, 10, h["hi_entropy_coef"], h["hi_value_coef"], h["hi_lr"],
                                             h["max_grad_norm"], h["optim_eps"], L)
        drive(out, "xy_goals", algo, N, L)
    with open(path, "wb") as f:
        pickle.dump(out, f)
    import multiprocessing
    for worker in multiprocessing.active_children():         # the reference's ParallelEnv leaves its workers to __del__
        worker.terminate()
    sys.stdout.flush()
    os._exit(0)


def main():
    before = M.tree_listing(M.REFERENCE)
    for variant, items in ITEMS.items():
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "out.pkl")
            env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONHASHSEED="0")
            subprocess.run([sys.executable, "-B", os.path.abspath(__file__), "--child", variant, path], check=True, env=env)
            with open(path, "rb") as f:
                out = pickle.load(f)
        for item in items:
            arrays = {k.split("/", 1)[1]: v for k, v in out.items() if k.startswith(item + "/")}
            dst = os.path.join(HERE, f"episode_log_{item}.npz")
            np.savez_compressed(dst, **arrays)
            print(f"wrote {os.path.relpath(dst)}: {len(arrays)} arrays, {os.path.getsize(dst)} bytes")
            assert os.path.getsize(dst) < 32 * 1024
    assert M.tree_listing(M.REFERENCE) == before, "the reference tree changed"


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:4])
    else:
        main()
