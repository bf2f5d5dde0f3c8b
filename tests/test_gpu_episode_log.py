"""zenv_episode_log on the device: after every one of the five collectors, the reference's `logs` -- every column, the
env column, kept, done and num_frames -- equal, value for value, to the numpy restatement of the reference's logging
loops (tests/episode_log_ref.py) fed the device's own recorded buffers; at the batch, frame-count and entry-count
edges of the kernels; the state rules; the statistics against math.fsum; and no effect on what the collectors record.

The scan of the (frame, wave) counts takes 256 counts per workgroup: T * ceil(N / 64) = 257 (N = 16385, T = 1) is that
boundary plus one, 514 (T = 2) spans three workgroups."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import hier_ref, option_ref, skill_ref, xy_ref
from tests.episode_log_ref import EpisodeLogRef, done_from_masks
from tests.skill_collect_ref import random_inverse_state_dict

pytestmark = pytest.mark.gpu

S, L = 4, 4
KINDS = ("flat", "flat_goal", "hier", "skills", "diayn", "options", "xy")
VARIANT = {"flat": "base", "flat_goal": "base", "hier": "hier", "skills": "skills", "diayn": "skills",
           "options": "options", "xy": "xy"}
COLLECTOR = {"flat": "collect", "flat_goal": "collect", "hier": "collect_hier", "skills": "collect_skills",
             "diayn": "collect_skills", "options": "collect_options", "xy": "collect_xy"}
PER_EPISODE = ("return_per_episode", "reshaped_return_per_episode", "num_frames_per_episode", "diversity_per_episode",
               "prediction_per_episode", "env_per_episode")


def _make(Z, kind, n, num_steps, seed=11, h=32, stagger=True, rewarding=True):
    """A handle of `n` envs with episodes of `num_steps` steps and the kind's random tiny networks loaded.  stagger (the
    handles that are not goal-conditioned): env i starts (2, 1, 0, 3)[i % 4] steps into its episode, so that under
    windows of 4 frames envs end on a window's first, middle and last frame.  rewarding: zones of
    radius 3.5 in the 6 x 6 arena, so that nearly every step visits a zone (reward 1) and an env that has visited all
    five ends early with (num_steps - steps) * 0.37 on top: returns that are neither 0 nor whole numbers."""
    from oracle import policy_ref as P
    over = dict(zones_size=3.5, time_saved_reward=0.37) if rewarding else {}
    env = Z.ZoneVecEnv(Z.config_for_id("PointTSP-v1", num_steps=num_steps, **over), n)
    env.build_bank(seed, n)
    env.schedule_sequential()
    if kind in ("flat_goal", "hier"):
        env.enable_goals()
    env.reset()
    if stagger and kind not in ("flat_goal", "hier"):
        for k in range(3):
            env.step(np.zeros((n, 2), np.float32), auto_reset=True)
            env.reset((np.arange(n) % 4 == k).astype(np.uint8))
    F = env.zone_feat
    if kind in ("flat", "flat_goal"):
        env.load_mlp(P.random_tensors(F, h=h, seed=3, critic=True), precision="f32")
        if kind == "flat_goal":
            env.set_goals((np.arange(n) % env.num_zones).astype(np.int32))
    elif kind == "hier":
        env.load_hier(Z.hier_tensors_from_state_dicts(*hier_ref.random_state_dicts(F, h=h, seed=3)))
    elif kind in ("skills", "diayn"):
        env.load_skills(Z.skill_tensors_from_state_dicts(*skill_ref.random_state_dicts(F, S, h=h, seed=3)), skill_len=L)
        if kind == "diayn":
            env.load_skill_inverse(Z.inverse_tensors_from_state_dict(random_inverse_state_dict(F, S, h=h, seed=4), S))
    elif kind == "options":
        env.load_options(Z.option_tensors_from_state_dicts(*option_ref.random_state_dicts(F, S, h=h, seed=3)))
    else:
        env.load_xy(Z.xy_tensors_from_state_dicts(*xy_ref.random_state_dicts(F, h=h, seed=3)), skill_len=L)
    return env


def _collect(env, kind, T, call):
    seed = 100 + call
    if kind in ("flat", "flat_goal"):
        env.collect_on_device(T, policy_seed=seed)
    elif kind == "hier":
        env.collect_hier_on_device(T, policy_seed=seed)
    elif kind == "skills":
        env.collect_skills_on_device(T, policy_seed=seed)
    elif kind == "diayn":
        env.collect_skills_on_device(T, policy_seed=seed, diversity_coef=0.5,
                                     skill_prior_logits=np.linspace(-1, 1, S).astype(np.float32))
    elif kind == "options":
        env.collect_options_on_device(T, policy_seed=seed)
    else:
        env.collect_xy_on_device(T, policy_seed=seed)


def _raw(Z, env, field, shape, dtype=np.float32):
    a = np.empty(shape, dtype)
    assert a.nbytes == env.field_bytes(field), (field, shape, env.field_bytes(field))
    Z._native.check(Z._native.lib().zenv_get(env._h, field, a.ctypes.data, 0))
    return a


def _records(Z, env, kind, T):
    """What the last collection recorded, time-major [T, N]: (env reward or None, reshaped, done, diversity or None)."""
    nat = Z._native
    n = env.num_envs
    mask = _raw(Z, env, nat.F_EXP_MASK, (T, n))
    done = done_from_masks(mask, 1 - env.get(nat.F_DONE).astype(np.float32))
    if kind == "flat":
        r = _raw(Z, env, nat.F_EXP_REWARD, (T, n))
        return r, r, done, None
    if kind == "flat_goal":
        return None, _raw(Z, env, nat.F_EXP_REWARD, (T, n)), done, None
    r = _raw(Z, env, nat.F_LO_ENV_REWARD, (T, n))
    div = _raw(Z, env, nat.F_LO_DIVERSITY, (T, n)) if kind in ("skills", "diayn") else None
    return r, r, done, div


def _same(Z, kind, got, want, tag):
    """Every key the collector reports, by value and exactly; the key set is the reference's plus env_per_episode."""
    from combinatorial_rl_tasks_amd import agents
    keys = set(agents.EPISODE_LOG_KEYS[COLLECTOR[kind]]) | {"env_per_episode"}
    assert set(got) == keys, (tag, sorted(got))
    assert isinstance(got["num_frames"], int) and got["num_frames"] == want["num_frames"], tag
    for k in sorted(keys - {"num_frames"}):
        a = got[k]
        assert isinstance(a, np.ndarray) and a.dtype == (np.int32 if k == "env_per_episode" else np.float32)
        b = np.asarray(want[k], a.dtype)
        assert a.shape == b.shape, (tag, k, a.shape, b.shape)
        assert np.array_equal(a, b), (tag, k, np.nonzero(a != b)[0][:8])


def _run(Z, kind, n, num_steps, Ts, env=None, ref=None):
    """Consecutive collections of Ts frames, the log taken after each and compared with the restatement.  Returns the
    handle, the restatement, the device logs and infos of every call."""
    env = env or _make(Z, kind, n, num_steps)
    ref = ref or EpisodeLogRef(n, VARIANT[kind], L if VARIANT[kind] in ("skills", "xy") else None)
    outs, infos = [], []
    for call, T in enumerate(Ts):
        _collect(env, kind, T, call)
        reward, reshaped, done, div = _records(Z, env, kind, T)
        got = env.episode_logs()
        info = env._eplog_info
        want = ref.collect(reshaped if reward is None else reward, reshaped, done, div)
        if reward is None:       # the env reward has no public record: test_goal_conditioned_return_is_the_env_reward
            assert got["return_per_episode"].shape == got["reshaped_return_per_episode"].shape
            got = dict(got, return_per_episode=np.asarray(want["return_per_episode"], np.float32))
        _same(Z, kind, got, want, (kind, n, call))
        assert info.done == want["done"] and info.kept == max(info.done, n) == len(got["env_per_episode"])
        if VARIANT[kind] in ("skills", "xy"):
            mask = _raw(Z, env, Z._native.F_EXP_MASK, (T, n))
            assert got["num_frames"] == Z.skill_num_frames(mask, L)
        else:
            assert got["num_frames"] == T * n
        outs.append(got)
        infos.append((info.kept, info.done, info.num_frames, info.columns))
    return env, ref, outs, infos


@pytest.mark.parametrize("kind", KINDS)
def test_every_collector_matches_the_restatement(zenv_mod, kind):
    """Three consecutive calls with a change of T between them (the carry and the tail survive it): the smallest T the
    collector allows (2, or one window), three windows, and a third length.  Episodes of at most 8 steps, shorter for an
    env that visits every zone, so that envs end in the middle of a window and idle, on a window's last frame, and
    across two calls."""
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import agents
    windowed = VARIANT[kind] in ("skills", "xy")
    Ts = (L, 3 * L, 2 * L) if windowed else (2, 3 * L, 5)
    env, _, outs, infos = _run(Z, kind, 65, 8, Ts)
    assert sum(i[1] for i in infos) > 65                     # more episodes ended than there are envs
    returns = np.concatenate([o["return_per_episode"] for o in outs])
    assert np.any(returns != 0) and np.any(returns != np.round(returns))
    assert all(i[3] == agents.episode_log_columns(COLLECTOR[kind]) for i in infos)
    if kind == "diayn":
        assert any(np.any(o["diversity_per_episode"] != 0) for o in outs)
    if kind == "skills":
        assert all(not np.any(o["diversity_per_episode"]) for o in outs)    # no inverse model: the reward is 0
    if windowed:
        assert all(not np.any(o["prediction_per_episode"]) for o in outs)
        assert any(o["num_frames"] < T * 65 for o, T in zip(outs, Ts))      # some env idled
    env.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["flat", "skills"])
def test_batch_edges(zenv_mod, kind, n):
    Z = zenv_mod
    env, _, _, infos = _run(Z, kind, n, 3, (8, 4, 8))
    assert sum(i[1] for i in infos) > 0
    env.close()


@pytest.mark.parametrize("T", [1, 2])
def test_scan_beyond_one_workgroup(zenv_mod, T):
    """N = 16385 is 257 waves: 257 counts with T = 1 (one workgroup of the scan plus one), 514 with T = 2.  Episodes
    of 2 steps: entries in every frame pair, on both sides of the boundary."""
    Z = zenv_mod
    n = 16385
    env, _, outs, infos = _run(Z, "flat", n, 2, (T, T, T))
    assert sum(i[1] for i in infos) >= n
    assert any(np.any(o["env_per_episode"] == n - 1) for o in outs)         # the 257th wave's only env
    env.close()


@pytest.mark.parametrize("case,num_steps,T", [("none", 1000, 8), ("few", 20, 8), ("many", 2, 8), ("all", 1, 8)])
def test_entry_counts(zenv_mod, case, num_steps, T):
    """D = 0 (the untouched tail of zeros, env -1), 0 < D < N (half of the envs are 13 steps ahead), D > N, D = T N."""
    Z = zenv_mod
    n = 65
    env = _make(Z, "flat", n, num_steps, rewarding=False)   # no env ends before num_steps
    if case == "few":                                         # every other env 13 steps into its episode
        for _ in range(13):
            env.step(np.zeros((n, 2), np.float32), auto_reset=True)
        env.reset((np.arange(n) % 2 == 0).astype(np.uint8))
    env, _, outs, infos = _run(Z, "flat", n, num_steps, (T,), env=env)
    kept, done = infos[0][:2]
    if case == "none":
        assert done == 0 and kept == n
        assert np.array_equal(outs[0]["env_per_episode"], np.full(n, -1, np.int32))
        for k in ("return_per_episode", "reshaped_return_per_episode", "num_frames_per_episode"):
            assert np.array_equal(outs[0][k], np.zeros(n, np.float32))
    elif case == "few":
        assert 0 < done < n and kept == n
        assert np.array_equal(outs[0]["env_per_episode"][:n - done], np.full(n - done, -1, np.int32))
    elif case == "many":
        assert done == T // 2 * n > n and kept == done
    else:
        assert done == T * n == kept
        assert np.array_equal(outs[0]["env_per_episode"], np.tile(np.arange(n, dtype=np.int32), T))
        assert np.array_equal(outs[0]["num_frames_per_episode"], np.ones(T * n, np.float32))
    env.close()


def test_goal_conditioned_return_is_the_env_reward(zenv_mod):
    """zenv_collect on a goal-conditioned handle records the shaped reward only: the env reward of every frame comes
    from a twin handle that collects the same frames one at a time (F_REWARD after each).  Both columns exactly; the
    two differ."""
    Z = zenv_mod
    nat = Z._native
    n, T = 65, 8
    a, b = _make(Z, "flat_goal", n, 5), _make(Z, "flat_goal", n, 5)
    ref = EpisodeLogRef(n, "base")
    differ = False
    for call in range(3):
        a.collect_on_device(T, policy_seed=100 + call)
        shaped = _raw(Z, a, nat.F_EXP_REWARD, (T, n))
        done = done_from_masks(_raw(Z, a, nat.F_EXP_MASK, (T, n)), 1 - a.get(nat.F_DONE).astype(np.float32))
        reward = np.empty((T, n), np.float32)
        for t in range(T):
            # the twin's draws: the same policy seed and step count
            b.collect_on_device(1, policy_seed=100 + call)
            reward[t] = b.get(nat.F_REWARD)
            assert np.array_equal(_raw(Z, b, nat.F_EXP_REWARD, (1, n))[0], shaped[t]), (call, t)
        got = a.episode_logs()
        _same(Z, "flat_goal", got, ref.collect(reward, shaped, done), ("twin", call))
        differ |= bool(np.any(got["return_per_episode"] != got["reshaped_return_per_episode"]))
        need, avail = a.goal_info()[1], a.goal_info()[2]
        g = np.full(n, -1, np.int32)
        for i in np.nonzero(need)[0]:
            opts = [z for z in range(a.num_zones) if (int(avail[i]) >> z) & 1]
            if opts:
                g[i] = opts[0]
        for e in (a, b):
            e.set_goals(g)
    assert differ
    a.close()
    b.close()


def test_last_logged_return_is_the_envs_own(zenv_mod):
    """Independent of the restatement: the env accumulates its episode's return in float64 (ZENV_F_LAST_RETURN), the
    log in float32.  A float32 sum of k terms is within (k - 1) 2^-24 sum|r| of the exact one, k <= num_steps."""
    Z = zenv_mod
    nat = Z._native
    n, num_steps, T = 65, 7, 8
    env = _make(Z, "flat", n, num_steps, stagger=False)     # every reward of every episode is recorded
    abs_sum = np.zeros(n)
    bound = np.zeros(n)
    seen = np.zeros(n, bool)
    last = np.zeros(n, np.float32)
    for call in range(3):
        env.collect_on_device(T, policy_seed=100 + call)
        reward, _, done, _ = _records(Z, env, "flat", T)
        for t in range(T):
            abs_sum += np.abs(reward[t].astype(np.float64))
            bound = np.where(done[t], num_steps * 2.0 ** -24 * abs_sum, bound)
            abs_sum = np.where(done[t], 0.0, abs_sum)
        got = env.episode_logs()
        for e, r in zip(got["env_per_episode"], got["return_per_episode"]):
            if e >= 0:
                last[e], seen[e] = r, True
        assert seen.all()
        want = env.get(nat.F_LAST_RETURN)
        err = np.abs(last.astype(np.float64) - want)
        print("last return: worst |log - env| %.3g, bound %.3g" % (err.max(), bound[np.argmax(err)]))
        assert np.all(err <= bound), (call, err.max())
        assert np.any(want != 0) and np.any(want != np.round(want))
    env.close()


@pytest.mark.parametrize("kind,num_steps,T", [("flat", 1000, 8), ("diayn", 2, 8), ("flat", 3, 1200)])
def test_statistics(zenv_mod, kind, num_steps, T):
    """count, min and max exactly; the sum within 2 (ceil(log2 n) + 2) 2^-53 sum|x| of math.fsum -- a pairwise tree of
    depth ceil(log2 n) (plus the zero padding of the fixed shape, which adds nothing) errs by at most depth 2^-53
    sum|x| to first order, doubled for the higher orders -- and the squares about the device's own mean within the
    same bound of fsum((x - mean)^2): the terms themselves are the same float64 operations on both sides.  n = 65
    (the zero tail), 130 (every column of DIAYN), and 26 000 (more than one workgroup of the reduction, two levels)."""
    Z = zenv_mod
    nat = Z._native
    n = 65
    env, _, outs, infos = _run(Z, kind, n, num_steps, (T,))
    kept = infos[0][0]
    if T == 1200:
        assert kept > 2 * 1024
    stats = env.episode_log_stats()
    assert set(stats) == set(outs[0]) - {"num_frames", "env_per_episode"}
    for key, s in stats.items():
        x = [float(v) for v in outs[0][key]]
        raw = (C.c_double * 5)()
        nat.check(nat.lib().zenv_episode_log_stats(env._h, nat.EPLOG_KEYS.index(key), raw))
        count, total, ssq, lo, hi = list(raw)
        assert count == kept == len(x) and lo == min(x) and hi == max(x)
        u = 2 * (math.ceil(math.log2(kept)) + 2) * 2.0 ** -53
        assert abs(total - math.fsum(x)) <= u * math.fsum(abs(v) for v in x), key
        mean = total / count
        sq = [(v - mean) * (v - mean) for v in x]
        assert abs(ssq - math.fsum(sq)) <= u * math.fsum(sq), key
        assert s == {"mean": mean, "std": (ssq / count) ** 0.5, "min": lo, "max": hi}
        assert s["std"] == pytest.approx(np.std(np.asarray(x)), rel=1e-12, abs=1e-300)
    env.close()


def test_state_rules(zenv_mod):
    """E_STATE before any collection and on a second call for the same collection; the other calls before the first
    log; an unknown column; episode_log_reset gives the result of a fresh handle; two handles with the same seeds give
    identical logs."""
    Z = zenv_mod
    nat = Z._native
    n, T = 65, 8
    a, b = _make(Z, "skills", n, 5), _make(Z, "skills", n, 5)
    info = nat.EpisodeLogInfo()
    raw = (C.c_double * 5)()
    ptr, count = C.c_void_p(), C.c_int64()
    assert nat.lib().zenv_episode_log(a._h, C.byref(info)) == Z.E_STATE
    assert nat.lib().zenv_episode_log_stats(a._h, 0, raw) == Z.E_STATE
    assert nat.lib().zenv_episode_log_tensor(a._h, 0, C.byref(ptr), C.byref(count)) == Z.E_STATE
    a.episode_log_reset()                                    # nothing carried yet: allowed
    first = []
    for call in range(2):
        logs = []
        for e in (a, b):
            _collect(e, "skills", T, call)
            logs.append(e.episode_logs())
        assert set(logs[0]) == set(logs[1])
        for k in logs[0]:
            assert np.array_equal(logs[0][k], logs[1][k]), k
        first.append(logs[0])
        with pytest.raises(Z.ZenvError) as ei:
            a.episode_logs()
        assert ei.value.code == Z.E_STATE
    for column in (-1, nat.EPLOG_COUNT):
        assert nat.lib().zenv_episode_log_tensor(a._h, column, C.byref(ptr), C.byref(count)) == Z.E_ARG
    assert nat.lib().zenv_episode_log_stats(a._h, nat.EPLOG_ENV, raw) == Z.E_ARG
    # after a reset the log of the next collection is a fresh object's: the restatement started anew
    a.episode_log_reset()
    _run(Z, "skills", n, 5, (T,), env=a)
    a.close()
    b.close()


def test_torch_tensors_alias_the_result(zenv_mod):
    import torch
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    Z = zenv_mod
    n, T = 65, 8
    a, b = _make(Z, "diayn", n, 5), _make(Z, "diayn", n, 5)
    tenv = TorchZoneEnv(a)
    for call in range(2):
        _collect(a, "diayn", T, call)
        _collect(b, "diayn", T, call)
        got, want = tenv.episode_logs(), b.episode_logs()
        assert set(got) == set(want) and got["num_frames"] == want["num_frames"]
        for k in PER_EPISODE:
            assert got[k].is_cuda and got[k].dtype == (torch.int32 if k == "env_per_episode" else torch.float32)
            assert got[k].data_ptr() == a.episode_log_ptr(Z._native.EPLOG_KEYS.index(k))[0]
            assert np.array_equal(got[k].cpu().numpy(), want[k]), k
        assert tenv.episode_log_stats() == b.episode_log_stats()
    a.close()
    b.close()


@pytest.mark.parametrize("kind", ["flat_goal", "hier", "diayn"])
def test_taking_the_log_leaves_the_records_alone(zenv_mod, kind):
    """Of two identical handles one takes the log after every collection, the other never: every ZENV_F_EXP_* buffer
    and the high-level records are bit-identical after three collections, and so is the env state."""
    Z = zenv_mod
    nat = Z._native
    n, T = 65, 2 * L
    a, b = _make(Z, kind, n, 5), _make(Z, kind, n, 5)
    for call in range(3):
        for e in (a, b):
            _collect(e, kind, T, call)
        a.episode_logs()
    fields = [nat.F_EXP_OBS, nat.F_EXP_ZONE_OBS, nat.F_EXP_ACTION, nat.F_EXP_LOG_PROB, nat.F_EXP_VALUE, nat.F_EXP_REWARD,
              nat.F_EXP_MASK, nat.F_EXP_ADVANTAGE, nat.F_EXP_RETURN]
    if kind != "flat_goal":
        fields += [nat.F_LO_ENV_REWARD, nat.F_HI_OBS, nat.F_HI_ZONE_OBS, nat.F_HI_ACTION, nat.F_HI_VALUE,
                   nat.F_HI_LOG_PROB, nat.F_HI_ADVANTAGE, nat.F_HI_RETURN, nat.F_HI_REWARD, nat.F_HI_MASK, nat.F_HI_COUNT]
    if kind == "diayn":
        fields += [nat.F_LO_SKILL, nat.F_LO_DIVERSITY]
    for f in fields:
        size = a.field_bytes(f)
        assert size == b.field_bytes(f), f
        assert np.array_equal(_raw(Z, a, f, (size,), np.uint8), _raw(Z, b, f, (size,), np.uint8)), f
    assert np.array_equal(a.get_state(), b.get_state()) and a.step_count == b.step_count
    a.close()
    b.close()
