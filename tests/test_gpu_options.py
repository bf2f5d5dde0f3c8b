"""The variable-length Options agent on the device (zenv_option_load / zenv_option_forward / ZENV_POLICY_OPTION_*): both
networks against the float32 torch restatement in tests/option_ref.py, the termination and action draws against the
host Philox, the option clock (a new skill exactly when the last option ended or the episode is new), the two ways the
high level finds its envs, MEAN mode, the keys, the replay identity with zenv_set_skills + zenv_step,
evaluate_options, the refusals and the coexistence with the other agents."""
import ctypes as C
import pickle

import numpy as np
import pytest

from tests import hier_ref, option_ref, philox_ref, skill_ref

pytestmark = pytest.mark.gpu

# the sampled third component against mu_2 + std_2 * z64 (z64: option_ref.term_noise, float64 Box-Muller on the device's
# uniforms): within ACT_ULPS float32 ulps of |mu_2| + std_2 * rad, the bar tests/test_gpu_hier_shapes.py sets for the
# action draw (the same logf / sqrtf / cosf; cosf's error is an ulp of 1, so the scale is the radius, not |z|)
ACT_ULPS = 4.0


def _cfg(Z, name, **over):
    """PointTSP-25 / TimedTSP-25 (the benchmark's 25-zone layouts) or a registry id."""
    if name == "PointTSP-25":
        return Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40, **over)
    if name == "TimedTSP-25":
        return Z.default_config(Z.TASK_TIMED_TSP, 25, zones_keepout=0.40, **over)
    return Z.config_for_id(name, **over)


def _env(Z, name, n, seed=11, first=None, maps=None, **over):
    """n envs on n maps; first: the one map every env plays; maps: that many maps, env i on map i % maps."""
    env = Z.ZoneVecEnv(_cfg(Z, name, **over), n)
    if maps is not None:
        env.build_bank(seed, maps)
        env.schedule_sequential(first=(np.arange(n) % maps).astype(np.int32), stride=0)
    elif first is None:
        env.build_bank(seed, n)
        env.schedule_sequential()
    else:
        env.build_bank(seed, 1)
        env.schedule_sequential(first=first, stride=0)
    env.reset()
    return env


def _load(Z, env, S, h=128, seed=0, critics=True, **kw):
    hi, lo = option_ref.random_state_dicts(env.zone_feat, S, h=h, seed=seed, critics=critics, **kw)
    env.load_options(Z.option_tensors_from_state_dicts(hi, lo))
    return hi, lo


def _tol(ref):
    return 1e-5 * np.maximum(1.0, np.abs(ref))


def _term(Z, env):
    return (env.get(Z.F_OPTION_TERM_MU), env.get(Z.F_OPTION_TERM_STD), env.get(Z.F_OPTION_TERM_ACTION),
            env.get(Z.F_OPTION_TERM_PROB))


def _check_networks(Z, env, hi, lo, S):
    """zenv_option_forward against option_ref on the device's own observations; returns the number of envs with a
    skill."""
    logits, hv, mu, std, lv, tmu, tstd, tprob = env.option_forward()
    o, zo = env.observations()
    skill = env.get(Z.F_SKILL)
    rl, rhv = option_ref.high(hi, o, zo)
    assert logits.shape == (env.num_envs, S) and mu.shape == (env.num_envs, 2)
    print("logits", float(np.abs(logits - rl).max()), "hi value", float(np.abs(hv - rhv).max()))
    assert np.all(np.abs(logits - rl) <= _tol(rl)), float(np.abs(logits - rl).max())
    assert np.all(np.abs(hv - rhv) <= _tol(rhv))
    has = skill >= 0
    rmu, rstd, rlv = option_ref.low(lo, o, zo, np.where(has, skill, 0), S)
    assert rmu.shape == (env.num_envs, 3)
    dmu, dstd = np.concatenate([mu, tmu[:, None]], axis=1), np.concatenate([std, tstd[:, None]], axis=1)
    print("mu", float(np.abs(dmu[has] - rmu[has]).max(initial=0)), "std", float(np.abs(dstd[has] - rstd[has]).max(initial=0)))
    assert np.all(np.abs(dmu[has] - rmu[has]) <= 1e-5), float(np.abs(dmu[has] - rmu[has]).max())
    assert np.all(np.abs(dstd[has] - rstd[has]) <= 1e-5)
    assert np.all(np.abs(lv[has] - rlv[has]) <= _tol(rlv[has]))
    ta = env.get(Z.F_OPTION_TERM_ACTION)
    assert np.array_equal(ta, tmu)                                  # the forward pass: a_2 = mu_2
    assert np.all(np.abs(tprob[has] - option_ref.term_prob(ta[has])) <= 1e-5)
    for a in (mu, std, lv, tmu, tstd, ta, tprob):
        assert not a[~has].any()
    return has.sum()


@pytest.mark.parametrize("name,h,S,n", [("PointTSP-25", 128, 5, 203), ("TimedTSP-25", 191, 1, 203),
                                        ("ColourMatch-v0", 1, 32, 203), ("PointTSP-25", 191, 32, 1027),
                                        ("ColourMatch-v0", 128, 5, 10241)])
def test_networks_match_torch(zenv_mod, name, h, S, n):
    Z = zenv_mod
    env = _env(Z, name, n, num_steps=150)
    hi, lo = _load(Z, env, S, h=h, seed=h + S)
    assert (env.get(Z.F_SKILL) == -1).all() and not env.get(Z.F_SKILL_AGE).any() and not env.get(Z.F_OPTION_ENDED).any()
    assert _check_networks(Z, env, hi, lo, S) == 0            # before any skill: the low level writes zeros
    rs = np.random.RandomState(S)
    for _ in range(25):
        env.step(rs.uniform(-1, 1, (n, 2)).astype(np.float32), auto_reset=True)
    # every skill value on some envs, every 7th env without one
    idx = np.arange(n)
    env.set_skills(np.where(idx % 7 == 0, -1, idx % S).astype(np.int32))
    skill = env.get(Z.F_SKILL)
    assert np.array_equal(skill, np.where(idx % 7 == 0, -1, idx % S))
    assert _check_networks(Z, env, hi, lo, S) == n - len(idx[::7])
    # the forward pass leaves the state alone
    assert np.array_equal(env.get(Z.F_SKILL), skill) and not env.get(Z.F_SKILL_AGE).any()
    assert not env.get(Z.F_OPTION_ENDED).any()
    if S > 1 and h > 1:      # the skill changes the low level's output, the third component included (at h = 1 the
        # one hidden unit may be dead under every skill: the outputs are then the biases)
        env.set_skills(np.zeros(n, np.int32))
        f0 = env.option_forward()
        env.set_skills(np.full(n, S - 1, np.int32))
        f1 = env.option_forward()
        assert not np.array_equal(f0[2], f1[2]) and not np.array_equal(f0[5], f1[5])
    env.close()


def check_draws(Z, seed, n=1501, S=5, steps=6, index0=123457):
    """OPTION_SAMPLE, every env, `steps` steps: ENDED == (u < TERM_PROB) with the host's uniform, exactly; TERM_ACTION is
    mu_2 + std_2 * z at the host's normal; TERM_PROB is sigmoid(4 a_2 - 3) of the device's own a_2; the skill and the
    first two action components are, bit for bit, those of a skill-agent handle holding the same tensors minus the
    third rows, in the same state, on the same seed.  Returns the worst distance of a_2 in ulps."""
    a_env = _env(Z, "PointTSP-25", n, num_steps=150)
    b_env = _env(Z, "PointTSP-25", n, num_steps=150)
    hi, lo = _load(Z, a_env, S, seed=17)
    b_env.load_skills(Z.skill_tensors_from_state_dicts(hi, option_ref.skill_planner_part(lo)), skill_len=10 ** 6)
    n_ended, worst = 0, 0.0
    for t in range(steps):
        step = a_env.step_count
        assert b_env.step_count == step
        a_env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=seed, env_index0=index0)
        skill, age = a_env.get(Z.F_SKILL), a_env.get(Z.F_SKILL_AGE)
        tmu, tstd, ta, tprob = _term(Z, a_env)
        ended = a_env.get(Z.F_OPTION_ENDED)
        assert (skill >= 0).all()
        # ---- the termination draw: float32 against float32, no env left out
        u = option_ref.term_uniform(n, seed, index0, step)
        assert u.dtype == np.float32 and tprob.dtype == np.float32
        assert np.array_equal(ended, (u < tprob).astype(np.int32)), f"step {t}"
        n_ended += ended.sum()
        assert np.all(np.abs(tprob - option_ref.term_prob(ta)) <= 1e-5)
        # ---- the third component
        z = option_ref.term_noise(n, seed, index0, step)
        c = philox_ref._draw(n, seed, index0, step, philox_ref.TAG_ACTION)
        rad = np.sqrt(-2.0 * np.log(philox_ref.uniform(c[2]).astype(np.float64)))
        want = tmu.astype(np.float64) + tstd.astype(np.float64) * z
        mag = np.abs(tmu.astype(np.float64)) + tstd.astype(np.float64) * rad
        ulps = np.abs(ta.astype(np.float64) - want) / (mag * 2.0 ** -23)
        worst = max(worst, float(ulps.max()))
        print("step", t, "a_2 ulps", float(ulps.max()), "ended", int(ended.sum()))
        assert ulps.max() <= ACT_ULPS, float(ulps.max())
        # ---- the skill agent in the same state: the envs that picked here are given their skill there, except on the
        # first call, where both pick (the same stream, the same inverse CDF)
        if t == 0:
            assert (age == 1).all()
        else:
            b_env.set_skills(np.where(age == 1, skill, -1).astype(np.int32))
        b_env.policy(Z.POLICY_SKILL_SAMPLE, policy_seed=seed, env_index0=index0)
        assert np.array_equal(b_env.get(Z.F_SKILL), skill), f"step {t}"
        for f in (Z.F_ACTIONS, Z.F_POLICY_MU, Z.F_POLICY_STD, Z.F_POLICY_VALUE):
            assert np.array_equal(a_env.get(f), b_env.get(f)), (t, f)
        a_env.step(None, auto_reset=True)
        b_env.step(None, auto_reset=True)
        for fa, fb in zip(a_env.results(), b_env.results()):
            assert np.array_equal(fa, fb), f"step {t}"
    assert n_ended > 0
    print("worst a_2 ulps", worst)
    a_env.close()
    b_env.close()
    return worst


@pytest.mark.parametrize("seed", [4, 0xDEADBEEF12345])
def test_draws_are_exact(zenv_mod, seed):
    """check_draws on 1 501 envs, S = 5, six steps."""
    check_draws(zenv_mod, seed)


def test_option_clock(zenv_mod):
    """320 steps with auto-reset on 37 ColourMatch envs with 40-step episodes.  A host mirror that sees only ENDED
    and the episode index says which envs must pick on each call: the skill changes only there, the age restarts there
    and otherwise counts up by one, a reset clears skill, age and ended."""
    Z = zenv_mod
    n, S = 37, 5
    env = _env(Z, "ColourMatch-v0", n, num_steps=40)
    _load(Z, env, S, seed=1)
    fresh = np.ones(n, bool)
    ended_prev = np.zeros(n, np.int32)
    episodes = env.get(Z.F_EPISODES)
    n_picks = n_fresh = n_end = 0
    for t in range(320):
        skill0, age0, ended0 = env.get(Z.F_SKILL), env.get(Z.F_SKILL_AGE), env.get(Z.F_OPTION_ENDED)
        assert (skill0[fresh] == -1).all() and not age0[fresh].any(), f"step {t}"
        assert np.array_equal(ended0, np.where(fresh, 0, ended_prev)), f"step {t}"
        assert (skill0[~fresh] >= 0).all()
        must_pick = fresh | (ended_prev == 1)
        env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=9)
        skill1, age1, ended1 = env.get(Z.F_SKILL), env.get(Z.F_SKILL_AGE), env.get(Z.F_OPTION_ENDED)
        assert (skill1 >= 0).all() and (skill1 < S).all()
        assert np.array_equal(skill1[~must_pick], skill0[~must_pick]), f"step {t}"
        assert np.array_equal(age1, np.where(must_pick, 1, age0 + 1)), f"step {t}"
        assert np.isin(ended1, (0, 1)).all()
        n_picks += must_pick.sum()
        n_fresh += (fresh & (t > 0)).sum()
        n_end += ended1.sum()
        env.step(None, auto_reset=True)
        e = env.get(Z.F_EPISODES)
        fresh, episodes, ended_prev = e != episodes, e, ended1
    assert n_fresh >= 7 * n and n_end > n and n_picks > n_fresh + n
    print("picks", int(n_picks), "after a reset", int(n_fresh), "options ended", int(n_end))

    # zenv_reset with a mask clears exactly the masked envs; zenv_set_skills clears the flag of the envs it sets
    for _ in range(40):                       # until some flags are up
        env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=10)
        if env.get(Z.F_OPTION_ENDED).sum() >= 2:
            break
        env.step(None, auto_reset=True)
    skill0, age0, ended0 = env.get(Z.F_SKILL), env.get(Z.F_SKILL_AGE), env.get(Z.F_OPTION_ENDED)
    up = np.flatnonzero(ended0)
    assert len(up) >= 2
    sets = np.full(n, -1, np.int32)
    sets[up[0]] = 2
    env.set_skills(sets)
    want = ended0.copy()
    want[up[0]] = 0
    assert np.array_equal(env.get(Z.F_OPTION_ENDED), want)
    assert env.get(Z.F_SKILL)[up[0]] == 2 and env.get(Z.F_SKILL_AGE)[up[0]] == 0
    mask = np.zeros(n, bool)
    mask[up[1]] = True
    mask[::3] = True
    env.reset(mask.astype(np.uint8))
    skill1, age1, ended1 = env.get(Z.F_SKILL), env.get(Z.F_SKILL_AGE), env.get(Z.F_OPTION_ENDED)
    assert (skill1[mask] == -1).all() and not age1[mask].any() and not ended1[mask].any()
    keep = ~mask
    keep[up[0]] = False
    assert np.array_equal(skill1[keep], skill0[keep]) and np.array_equal(age1[keep], age0[keep])
    assert np.array_equal(ended1[~mask], want[~mask])

    # auto_reset=0: a finished env idles -- zeros in every output, nothing ends, skill and age stay
    env.reset()
    for t in range(40):
        env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=11)
        env.step(None, auto_reset=False)
    assert env.get(Z.F_DONE).all()
    skill0, age0 = env.get(Z.F_SKILL), env.get(Z.F_SKILL_AGE)
    assert (skill0 >= 0).all() and (age0 >= 1).all()
    for pol in (Z.POLICY_OPTION_SAMPLE, Z.POLICY_OPTION_MEAN):
        env.policy(pol, policy_seed=12)
        for f in (Z.F_ACTIONS, Z.F_POLICY_MU, Z.F_POLICY_STD, Z.F_POLICY_VALUE, Z.F_OPTION_TERM_MU, Z.F_OPTION_TERM_STD,
                  Z.F_OPTION_TERM_ACTION, Z.F_OPTION_TERM_PROB, Z.F_OPTION_ENDED):
            assert not env.get(f).any(), f
        assert np.array_equal(env.get(Z.F_SKILL), skill0) and np.array_equal(env.get(Z.F_SKILL_AGE), age0)
    env.step(None, auto_reset=True)                              # the auto-reset step
    assert (env.get(Z.F_SKILL) == -1).all() and not env.get(Z.F_OPTION_ENDED).any()
    env.close()


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("n", [65536, 203])
def test_the_way_the_pickers_are_found_changes_nothing(zenv_mod, monkeypatch, n, compact):
    """Workgroups over env blocks (compact = 0) or over the compacted list of picking envs (1): for every env that
    picked, SKILL_LOGITS / SKILL_VALUE are bit for bit what option_forward gave on the same observations just before --
    where every env picks (the first call after a reset) and where about 5 % do (mu_2 = 0, std_2 at its floor: prob =
    sigmoid(-3) = 0.047)."""
    Z = zenv_mod
    monkeypatch.setenv("ZENV_OPTION_COMPACT", str(compact))
    S = 5
    env = _env(Z, "PointTSP-25", n, maps=min(n, 256), num_steps=150)
    _load(Z, env, S, seed=23, term_bias=0.0)
    rs = np.random.RandomState(n)
    for _ in range(5):                                # the envs of one map part ways
        env.step(rs.uniform(-1, 1, (n, 2)).astype(np.float32), auto_reset=True)
    must_pick = np.ones(n, bool)
    rates = []
    for t in range(5 if n > 1000 else 40):
        fl, fv = env.option_forward()[:2]
        skill0 = env.get(Z.F_SKILL)
        env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=31)
        logits, value, skill1 = env.get(Z.F_SKILL_LOGITS), env.get(Z.F_SKILL_VALUE), env.get(Z.F_SKILL)
        assert np.array_equal(logits[must_pick], fl[must_pick]), f"step {t}"
        assert np.array_equal(value[must_pick], fv[must_pick]), f"step {t}"
        assert np.array_equal(logits, fl) and np.array_equal(value, fv)      # and nobody else's rows were touched
        assert (skill1 >= 0).all() and np.array_equal(skill1[~must_pick], skill0[~must_pick])
        # the pick itself: the host's inverse CDF on the device's logits, where the uniform is clear of a boundary
        u = philox_ref.skill_uniform(n, 31, 0, env.step_count).astype(np.float64)
        cdf = np.cumsum(np.exp(logits.astype(np.float64)), axis=1)
        cdf /= cdf[:, -1:]
        clear = must_pick & (np.abs(cdf - u[:, None]).min(axis=1) > 1e-5)
        assert np.array_equal(skill1[clear], np.argmax(cdf > u[:, None], axis=1)[clear]), f"step {t}"
        if t > 0:
            rates.append(must_pick.mean())
        must_pick = env.get(Z.F_OPTION_ENDED) == 1
        env.step(None, auto_reset=True)
    print("pick rate", np.mean(rates))
    if n > 1000:
        assert 0.03 < np.mean(rates) < 0.07
    else:
        assert 0 < np.mean(rates) < 0.15
    env.close()


def test_termination_statistics(zenv_mod):
    """mu_2 a known constant, std_2 at its floor, 65 536 envs, one call: the fraction of options that end is within
    five binomial standard deviations of the mean of TERM_PROB (sd = sqrt(sum p (1 - p)) / N: the envs draw
    independently, env i with its own p_i)."""
    Z = zenv_mod
    n = 65536
    env = _env(Z, "PointTSP-25", n, maps=256)
    _load(Z, env, 5, seed=2, term_bias=1.0)
    env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=77)
    tmu, tstd, ta, tprob = _term(Z, env)
    mu2 = 2.0 * (1.0 / (1.0 + np.exp(-1.0)) - 0.5)
    assert np.all(np.abs(tmu - mu2) <= 1e-6) and np.all(np.abs(tstd - 1e-3) <= 1e-6)
    p = tprob.astype(np.float64)
    assert abs(p.mean() - option_ref.term_prob(mu2)) < 1e-3          # about 0.24
    sd = np.sqrt((p * (1.0 - p)).sum()) / n
    frac = env.get(Z.F_OPTION_ENDED).mean()
    print("ended", frac, "mean prob", p.mean(), "sd", sd)
    assert abs(frac - p.mean()) <= 5.0 * sd
    env.close()


def test_mean_policy_is_deterministic(zenv_mod):
    """OPTION_MEAN: the argmax skill, a = mu, a_2 = mu_2, ENDED == (TERM_PROB > 0.5); the seed changes nothing."""
    Z = zenv_mod
    n, S = 600, 5
    # (a) against torch, with a third mu_ row large enough to put TERM_PROB on both sides of 0.5
    env = _env(Z, "PointTSP-25", n, num_steps=200)
    hi, lo = option_ref.random_state_dicts(env.zone_feat, S, seed=5)
    lo["actor.mu_.weight"][2] *= 40.0
    env.load_options(Z.option_tensors_from_state_dicts(hi, lo))
    rs = np.random.RandomState(2)
    for _ in range(10):
        env.step(rs.uniform(-1, 1, (n, 2)).astype(np.float32))
    o, zo = env.observations()
    rl, rhv = option_ref.high(hi, o, zo)
    env.policy(Z.POLICY_OPTION_MEAN)
    skill = env.get(Z.F_SKILL)
    srt = np.sort(rl, axis=1)
    clear = srt[:, -1] - srt[:, -2] > 1e-4
    assert clear.sum() > n // 2
    assert np.array_equal(skill[clear], np.argmax(rl, axis=1)[clear])
    logits = env.get(Z.F_SKILL_LOGITS)
    assert np.all(np.abs(logits - rl) <= _tol(rl))
    a, mu = env.get(Z.F_ACTIONS), env.get(Z.F_POLICY_MU)
    assert np.array_equal(a, mu)
    tmu, tstd, ta, tprob = _term(Z, env)
    assert np.array_equal(ta, tmu)
    rmu, _, _ = option_ref.low(lo, o, zo, skill, S)
    assert np.all(np.abs(mu - rmu[:, :2]) <= 1e-5)
    assert np.all(np.abs(tmu - rmu[:, 2]) <= 1e-3)              # (the row scaled by 40: its rounding too)
    ended = env.get(Z.F_OPTION_ENDED)
    assert np.array_equal(ended, (tprob > np.float32(0.5)).astype(np.int32))
    print("MEAN: ended", int(ended.sum()), "of", n)
    assert (env.get(Z.F_SKILL_AGE) == 1).all()
    env.close()
    # (b) both outcomes by construction: mu_2 = 0.905 -> prob 0.65, every option ends; mu_2 = 0 -> 0.047, none does
    for bias, want in ((3.0, 1), (0.0, 0)):
        env = _env(Z, "ColourMatch-v0", 64)
        _load(Z, env, S, seed=6, term_bias=bias)
        for t in range(3):
            env.policy(Z.POLICY_OPTION_MEAN)
            assert (env.get(Z.F_OPTION_ENDED) == want).all()
            assert np.array_equal(env.get(Z.F_SKILL_AGE), np.full(64, 1 if want else t + 1))
            env.step(None, auto_reset=True)
        env.close()
    # (c) two runs on different seeds are identical
    envs = [_env(Z, "ColourMatch-v0", 128, num_steps=20) for _ in range(2)]
    for e in envs:
        hi, lo = option_ref.random_state_dicts(e.zone_feat, S, seed=7)
        lo["actor.mu_.weight"][2] *= 40.0
        e.load_options(Z.option_tensors_from_state_dicts(hi, lo))
    for t in range(30):
        for e, seed in zip(envs, (1, 2)):
            e.policy(Z.POLICY_OPTION_MEAN, policy_seed=seed)
        for f in (Z.F_SKILL, Z.F_SKILL_AGE, Z.F_OPTION_ENDED, Z.F_ACTIONS, Z.F_OPTION_TERM_ACTION, Z.F_OPTION_TERM_PROB):
            assert np.array_equal(envs[0].get(f), envs[1].get(f)), (t, f)
        for e in envs:
            e.step(None, auto_reset=True)
    for fa, fb in zip(envs[0].results(), envs[1].results()):
        assert np.array_equal(fa, fb)
    for e in envs:
        e.close()


def test_sampling_is_keyed_by_seed_env_and_step(zenv_mod):
    Z = zenv_mod
    n = 4096
    envs = [_env(Z, "ColourMatch-v0", n, seed=1000000, first=np.zeros(n, np.int32)) for _ in range(3)]
    for e in envs:
        _load(Z, e, 5, seed=9)
    for e, seed in zip(envs, (4, 4, 5)):
        e.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=seed)
    fields = (Z.F_SKILL, Z.F_ACTIONS, Z.F_OPTION_TERM_ACTION, Z.F_OPTION_ENDED)
    r = [[e.get(f) for f in fields] for e in envs]
    for x, y, z in zip(*r):
        assert np.array_equal(x, y) and not np.array_equal(x, z)
    # env_index0 shifts the key: env i of a handle at env_index0 = 1 draws what env i + 1 drew (one map, one state)
    envs[2].reset()
    envs[2].policy(Z.POLICY_OPTION_SAMPLE, policy_seed=4, env_index0=1)
    for f, x in zip(fields, r[0]):
        assert np.array_equal(envs[2].get(f)[:-1], x[1:]), f
    # ... and the step: the next call draws anew
    envs[0].step(np.zeros((n, 2), np.float32))
    envs[1].step(np.zeros((n, 2), np.float32))
    envs[0].policy(Z.POLICY_OPTION_SAMPLE, policy_seed=4)
    assert not np.array_equal(envs[0].get(Z.F_OPTION_TERM_ACTION), r[0][2])
    envs[1].policy(Z.POLICY_OPTION_SAMPLE, policy_seed=4)
    for f in fields:
        assert np.array_equal(envs[0].get(f), envs[1].get(f))
    for e in envs:
        e.close()


@pytest.mark.parametrize("name", ["PointTSP-25", "ColourMatch-v0"])
def test_replay_identity_with_set_skills_and_step(zenv_mod, name):
    """zenv_policy(OPTION_SAMPLE) + zenv_step == zenv_set_skills(the skills it picked) + zenv_step(its actions), bit for
    bit, the skill included."""
    Z = zenv_mod
    n, T = 256, 100
    a_env = _env(Z, name, n, num_steps=40)
    b_env = _env(Z, name, n, num_steps=40)
    _load(Z, a_env, 5, seed=3)
    _load(Z, b_env, 5, seed=3)
    n_new = 0
    for t in range(T):
        a_env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=77)
        skill, age, act = a_env.get(Z.F_SKILL), a_env.get(Z.F_SKILL_AGE), a_env.get(Z.F_ACTIONS)
        new = age == 1                        # picked at this step
        n_new += new.sum()
        b_env.set_skills(np.where(new, skill, -1).astype(np.int32))
        assert np.array_equal(b_env.get(Z.F_SKILL), skill), f"step {t}"
        a_env.step(None, auto_reset=True)
        b_env.step(act, auto_reset=True)
        for fa, fb in zip(a_env.results(), b_env.results()):
            assert np.array_equal(fa, fb), f"step {t}"
        assert np.array_equal(a_env.get(Z.F_SKILL), b_env.get(Z.F_SKILL)), f"step {t}"
    assert n_new > 3 * n
    a_env.close()
    b_env.close()


def test_evaluate_options(zenv_mod, tmp_path):
    import torch
    from combinatorial_rl_tasks_amd.evaluate import evaluate_options
    Z = zenv_mod
    hi, lo = option_ref.random_state_dicts(6, 5, h=128, seed=31)
    torch.save({"hi_model_state": hi, "lo_model_state": lo, "num_frames": 0}, tmp_path / "status.pt")
    cfg = Z.config_for_id("PointTSP-v0", num_steps=150)
    pkl = tmp_path / "results.pkl"
    kw = dict(n_maps=4, n_runs_per_map=3, max_steps=400)
    out = evaluate_options(cfg, str(tmp_path), pkl_path=str(pkl), n_skills=5, **kw)
    assert set(out) == {"return", "length", "goal_met", "terminations"}
    length, terms = np.array(out["length"]), np.array(out["terminations"])
    assert np.array(out["return"]).shape == (4, 3) and length.shape == (4, 3) and terms.shape == (4, 3)
    assert (length > 0).all()
    assert (terms >= 0).all() and (terms <= length).all() and terms.sum() > 0      # at most one per step
    with open(pkl, "rb") as f:
        assert pickle.load(f) == {"return": out["return"]}
    assert np.array(evaluate_options(cfg, (hi, lo))["return"]).shape == (100, 1)   # the script's protocol
    m1 = evaluate_options(cfg, str(tmp_path / "status.pt"), argmax=True, **kw)
    m2 = evaluate_options(cfg, (hi, lo), argmax=True, **kw)
    assert m1 == m2
    assert all(len(set(r)) == 1 for r in m1["return"])       # the runs of one map are identical under argmax
    with pytest.raises(ValueError, match="n_skills"):
        evaluate_options(cfg, (hi, lo), n_skills=2, **kw)
    with pytest.raises(ValueError, match="skill_tensors_from_state_dicts"):
        evaluate_options(cfg, (hi, option_ref.skill_planner_part(lo)), **kw)
    # the same trajectories by hand: map m, run r is env 3 m + r
    n = 12
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(1000000, 4)
    env.schedule_sequential(first=np.repeat(np.arange(4, dtype=np.int32), 3), stride=0)
    env.reset()
    env.load_options(Z.option_tensors_from_state_dicts(hi, lo))
    ended = np.zeros(n, np.int64)
    for t in range(400):
        env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=0)
        ended += env.get(Z.F_OPTION_ENDED)
        env.step(None, auto_reset=False)
        if env.get(Z.F_DONE).all():
            break
    assert np.array_equal(env.get(Z.F_LAST_RETURN).reshape(4, 3), np.array(out["return"]))
    assert np.array_equal(env.get(Z.F_LAST_LEN).reshape(4, 3), length)
    assert np.array_equal(ended.reshape(4, 3), terms)
    env.close()


def test_refusals(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    env = _env(Z, "PointTSP-v0", 8)
    t = Z.option_tensors_from_state_dicts(*option_ref.random_state_dicts(6, 3, h=32))

    def state_refused(*calls):
        for call in calls:
            with pytest.raises(Z.ZenvError) as e:
                call()
            assert e.value.code == Z.E_STATE

    def collect_skill():
        Z._native.check(nat.lib().zenv_collect_skill(env._h, 4, 1, 0, 0.99, 0.95, 0.0, None, 1))

    state_refused(lambda: env.policy(Z.POLICY_OPTION_MEAN), lambda: env.policy(Z.POLICY_OPTION_SAMPLE),
                  env.option_forward, lambda: env.set_skills(np.zeros(8, np.int32)))
    assert env.field_bytes(Z.F_OPTION_ENDED) == 0 and env.field_bytes(Z.F_OPTION_TERM_PROB) == 0
    # weight validation
    for F, S, h in ((6, 3, 192), (7, 3, 32), (6, 33, 32)):
        with pytest.raises(Z.ZenvError) as e:
            env.load_options(Z.option_tensors_from_state_dicts(*option_ref.random_state_dicts(F, S, h=h)))
        assert e.value.code == Z.E_ARG, (F, S, h)
    keep = {k: np.ascontiguousarray(v) for k, v in t.items()}

    def raw(**over):
        w = nat.OptionWeights(h_dim=32, n_skills=3, zone_feat=6, precision=nat.MLP_F32)
        for k, v in keep.items():
            setattr(w, k, v.ctypes.data)
        for k, v in over.items():
            setattr(w, k, v)
        return nat.lib().zenv_option_load(env._h, C.byref(w))

    assert raw(n_skills=0) == Z.E_ARG and raw(h_dim=0) == Z.E_ARG
    assert raw(precision=nat.MLP_BF16) == Z.E_ARG
    assert raw(lo_mu_w=None) == Z.E_ARG and raw(hi_logit_b=None) == Z.E_ARG
    assert raw(hi_critic_b2=None) == Z.E_ARG and raw(lo_critic_w1=None) == Z.E_ARG
    assert raw(hi_critic_w1=None, hi_critic_b1=None, hi_critic_w2=None, hi_critic_b2=None) == 0     # no critic: fine
    env.load_options(t)
    env.policy(Z.POLICY_OPTION_MEAN)
    assert env.field_bytes(Z.F_OPTION_ENDED) == 8 * 4
    # the policies are not rollout / collect policies
    for pol in (Z.POLICY_OPTION_SAMPLE, Z.POLICY_OPTION_MEAN):
        with pytest.raises(Z.ZenvError) as e:
            env.rollout(5, pol)
        assert e.value.code == Z.E_ARG
    # the loaded agent is the Options one: what runs the skill agent, or the flat network, refuses the handle
    state_refused(lambda: env.collect(4), collect_skill, env.skill_forward,
                  lambda: env.policy(Z.POLICY_SKILL_MEAN), lambda: env.policy(Z.POLICY_SKILL_SAMPLE))
    with pytest.raises(Z.ZenvError) as e:
        env.policy(10)
    assert e.value.code == Z.E_ARG
    # set_skills works as for the skill agent, out of range included
    env.set_skills(np.array([0, 1, 2, -1, 0, 1, 2, -1], np.int32))
    before = env.get(Z.F_SKILL)
    for bad in (3, -2):
        s = np.zeros(8, np.int32)
        s[5] = bad
        with pytest.raises(Z.ZenvError) as e:
            env.set_skills(s)
        assert e.value.code == Z.E_ARG
    assert np.array_equal(env.get(Z.F_SKILL), before)
    env.close()
    # a goal-conditioned / solver-ordered handle
    for enable in ("enable_goals", "enable_order"):
        env = Z.ZoneVecEnv(_cfg(Z, "PointTSP-v0"), 8)
        getattr(env, enable)()
        env.build_bank(11, 8)
        env.reset()
        with pytest.raises(Z.ZenvError) as e:
            env.load_options(t)
        assert e.value.code == Z.E_STATE
        env.close()


def test_one_agent_of_the_skill_family_per_handle(zenv_mod):
    """zenv_option_load drops skill weights, zenv_skill_load drops option weights; the later one works, the earlier one
    is refused, and either load resets the skill state."""
    Z = zenv_mod
    n, S = 64, 4
    env = _env(Z, "PointTSP-25", n)
    ohi, olo = option_ref.random_state_dicts(env.zone_feat, S, h=64, seed=1)
    shi, slo = skill_ref.random_state_dicts(env.zone_feat, S, h=64, seed=2)

    def refused(*calls):
        for call in calls:
            with pytest.raises(Z.ZenvError) as e:
                call()
            assert e.value.code == Z.E_STATE

    def cleared():
        return ((env.get(Z.F_SKILL) == -1).all() and not env.get(Z.F_SKILL_AGE).any()
                and (env.field_bytes(Z.F_OPTION_ENDED) == 0 or not env.get(Z.F_OPTION_ENDED).any()))

    for first in ("options", "skills"):
        order = ("options", "skills", "options") if first == "options" else ("skills", "options", "skills")
        for kind in order:
            if kind == "options":
                env.load_options(Z.option_tensors_from_state_dicts(ohi, olo))
                assert cleared()
                env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=3)
                refused(lambda: env.policy(Z.POLICY_SKILL_SAMPLE), env.skill_forward)
                logits, hv, mu, std, lv, tmu, tstd, tprob = env.option_forward()
                o, zo = env.observations()
                rl, _ = option_ref.high(ohi, o, zo)
                rmu, _, _ = option_ref.low(olo, o, zo, env.get(Z.F_SKILL), S)
            else:
                env.load_skills(Z.skill_tensors_from_state_dicts(shi, slo), skill_len=3)
                assert cleared()
                env.policy(Z.POLICY_SKILL_SAMPLE, policy_seed=3)
                refused(lambda: env.policy(Z.POLICY_OPTION_SAMPLE), env.option_forward)
                logits, hv, mu, std, lv = env.skill_forward()
                o, zo = env.observations()
                rl, _ = skill_ref.high(shi, o, zo)
                rmu, _, _ = skill_ref.low(slo, o, zo, env.get(Z.F_SKILL), S)
            assert (env.get(Z.F_SKILL) >= 0).all()
            assert np.all(np.abs(logits - rl) <= _tol(rl)) and np.all(np.abs(mu - rmu[:, :2]) <= 1e-5)
            env.step(None, auto_reset=True)
    env.close()


def test_options_leave_the_other_networks_alone(zenv_mod):
    """Loading options does not change zenv_mlp_load's outputs on the same handle; the Zone-goals agent's handle
    refuses them and keeps working."""
    from oracle import policy_ref as P
    Z = zenv_mod
    n = 300
    env = _env(Z, "PointTSP-v0", n)
    rs = np.random.RandomState(0)
    for _ in range(5):
        env.step(rs.uniform(-1, 1, (n, 2)).astype(np.float32))
    t = P.random_tensors(env.zone_feat, h=128, seed=5, critic=True)
    env.load_mlp(t, precision="f32")
    ref = env.mlp_forward(with_value=True)
    hi, lo = _load(Z, env, 5, seed=8)
    env.policy(Z.POLICY_OPTION_SAMPLE, policy_seed=3)
    out = env.mlp_forward(with_value=True)
    for a, b in zip(ref, out):
        assert np.array_equal(a, b)
    env.policy(Z.POLICY_MLP_MEAN)
    assert np.array_equal(env.get(Z.F_ACTIONS), ref[0])
    # and the option networks still answer after the flat one ran
    assert _check_networks(Z, env, hi, lo, 5) == n
    env.close()
    genv = _env(Z, "PointTSP-v0", 64)
    genv.enable_goals()
    genv.reset()
    ghi, glo = hier_ref.random_state_dicts(genv.zone_feat, h=64, seed=2)
    genv.load_hier(Z.hier_tensors_from_state_dicts(ghi, glo))
    with pytest.raises(Z.ZenvError):
        genv.load_options(Z.option_tensors_from_state_dicts(*option_ref.random_state_dicts(6, 2, h=32)))
    logits, hv, _, _, _ = genv.hier_forward()
    rl, rhv = hier_ref.high(ghi, *genv.observations(), genv.goal_info()[2])
    fin = np.isfinite(rl)
    assert np.all(np.abs(logits[fin] - rl[fin]) <= _tol(rl[fin]))
    genv.close()
