"""CPU: the numpy restatement of the reference's five logging loops (tests/episode_log_ref.py) reproduces the `logs`
the reference's own collect_experiences returned (tests/golden/episode_log_<variant>.npz, written by
tests/golden/make_episode_log_goldens.py) exactly -- lengths, order, values and num_frames -- over three consecutive
calls: one that ends no episode, one that ends more than num_procs, episodes that span two calls, and under windows an
env that ends mid-window and idles and one that ends on a window's last frame."""
import os

import numpy as np
import pytest

from tests.episode_log_ref import EpisodeLogRef

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# golden -> (the restatement's variant, the collector here)
CASES = {"base": ("base", "collect"), "skills": ("skills", "collect_skills"), "zone_goals": ("hier", "collect_hier"),
         "options": ("options", "collect_options"), "xy_goals": ("xy", "collect_xy")}


def _load(name):
    with np.load(os.path.join(GOLD, f"episode_log_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference_logs(zenv_mod, name):
    from combinatorial_rl_tasks_amd import agents
    variant, collector = CASES[name]
    g = _load(name)
    N, T, L, calls = (int(v) for v in g["shape"])
    assert calls == 3 and g["reward"].shape == g["done"].shape == (calls * T, N)
    ref = EpisodeLogRef(N, variant, L or None)
    reshaped = g["shaped_reward"] if name == "base" else g["reward"]
    if name == "base":
        assert np.any(reshaped != g["reward"])
    ended = []
    for c in range(calls):
        rows = slice(c * T, (c + 1) * T)
        logs = ref.collect(g["reward"][rows], reshaped[rows], g["done"][rows],
                           g["diversity"][rows] if "diversity" in g else None)
        # options' termination_rate is a scalar of the call's termination draws, not an episode log
        keys = set(str(k) for k in g[f"call{c}/keys"]) - {"termination_rate"}
        assert keys == set(agents.EPISODE_LOG_KEYS[collector]) == set(logs) - {"env_per_episode", "done"}
        assert logs["num_frames"] == int(g[f"call{c}/num_frames"])
        for k in sorted(keys - {"num_frames"}):
            want = g[f"call{c}/{k}"]
            got = np.array(logs[k], np.float64)
            assert got.shape == want.shape == (max(logs["done"], N),), (name, c, k)
            assert np.array_equal(got, want), (name, c, k, got, want)
        ended.append(logs["done"])
    assert ended[0] == 0 and ended[1] > N and ended[2] > 0
    if name == "skills":
        assert any(np.any(g[f"call{c}/diversity_per_episode"] != 0) for c in range(calls))
    if L:
        assert sum(int(g[f"call{c}/num_frames"]) for c in range(calls)) < calls * T * N      # an env idled


def test_restatement_rules_on_a_hand_made_case():
    """Two envs, windows of 2 frames: env 1 ends on frame 0 and idles on frame 1 (one entry, two frames counted into
    its sum, one active frame), ends again on frame 3 (a window's last frame); the tail of zeros makes up the keep."""
    ref = EpisodeLogRef(2, "xy", 2)
    reward = np.array([[1, 2], [1, 0], [1, 4], [1, 8]], np.float32)
    done = np.array([[0, 1], [0, 1], [0, 0], [0, 1]], bool)
    logs = ref.collect(reward, reward, done)
    assert logs["done"] == 2 and logs["num_frames"] == 4 + 3
    assert logs["return_per_episode"] == [2.0, 12.0] and logs["env_per_episode"] == [1, 1]
    assert logs["num_frames_per_episode"] == [1.0, 2.0]
    logs = EpisodeLogRef(2, "base").collect(reward, reward, done)
    assert logs["done"] == 3 and logs["return_per_episode"] == [2.0, 0.0, 12.0]
    assert logs["num_frames_per_episode"] == [1.0, 1.0, 2.0] and logs["num_frames"] == 8
    logs = EpisodeLogRef(2, "base").collect(reward[:1], reward[:1], done[:1])
    assert logs["return_per_episode"] == [0, 2.0] and logs["env_per_episode"] == [-1, 1]
