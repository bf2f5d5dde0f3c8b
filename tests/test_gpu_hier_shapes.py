"""The hierarchical agents' kernels (hier_f32.hip, skill_f32.hip, hier_collect.hip; encoder in hier_enc.hpp) at the edges
of their layout -- h around the 32-feature tiles up to 191, Z = 1..32 around the 32-row passes, ragged workgroups of
EB = 4 envs, S up to 32 -- against a float64 restatement of the same operations (tests/hier_ref.py, tests/skill_ref.py
with dtype=float64); the goal, skill and action draws env by env against the host Philox (tests/philox_ref.py); ties;
zone 31 (the sign bit of the availability mask); and zenv_collect_hier at the prefix-sum tile edges, at Z * F = 224,
across an M = 0 call and over several scan tiles."""
import numpy as np
import pytest
import torch

from tests import hier_ref, philox_ref, skill_ref
from tests.hier_collect_ref import GAMMA, LAM, expected_hi, log_softmax_at, replay

pytestmark = pytest.mark.gpu

TSP, TTSP, CM = 0, 1, 2
F64 = torch.float64
# Weight scale 3 (activations in the hundreds): torch's own float32 result is no longer within 1e-5 of the float64 one,
# and the kernels -- float32 with another summation order -- are held to K_F32 times torch float32's distance from
# float64 instead.  Where the kernel is off by more than the plain bar, the largest ratio |dev - ref64| / |ref32 - ref64|
# met on this sweep was 6.7 (the skill logits; 3.5 for the Zone-goals low-level value): K_F32 = 16 leaves room for
# another summation order without letting a wrong term through (a wrong term is off by O(1), not by a float32 ulp).
K_F32 = 16.0
# the sampled action against mu + std * eps64 (eps64: tests/philox_ref.py, float64 Box-Muller on the device's uniforms):
# within ACT_ULPS float32 ulps of |mu| + std * |eps|.  logf / cosf / sinf / sqrtf are the accurate ones (-fno-fast-math):
# the largest distance met was 1.3 ulps.  A draw of the wrong stream, step or env is off by O(std).
ACT_ULPS = 4.0
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


def _check(dev, r64, r32, scale, what):
    """|dev - ref64| <= max(1e-5 max(1, |ref64|), K_F32 |ref32 - ref64|), the second term only at weight scale > 1;
    -inf exactly where the reference has -inf.  Returns |dev - ref64| per element (0 at -inf)."""
    dev, r64, r32 = np.asarray(dev, np.float64), np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    fin = np.isfinite(r64)
    assert np.array_equal(np.isfinite(dev), fin), what
    assert np.all(dev[~fin] == r64[~fin]), what
    err = np.where(fin, np.abs(np.where(fin, dev, 0) - np.where(fin, r64, 0)), 0.0)
    base = 1e-5 * np.maximum(1.0, np.abs(np.where(fin, r64, 0)))
    d32 = np.where(fin, np.abs(np.where(fin, r32, 0) - np.where(fin, r64, 0)), 0.0)
    over = err > base
    if over.any():
        _note(what + " err/d32 (scale %g)" % scale, (err[over] / np.maximum(d32[over], 1e-30)).max())
    bar = np.maximum(base, K_F32 * d32) if scale > 1 else base
    bad = err > bar
    assert not bad.any(), "%s: %d elements, worst |dev - ref64| %.3g at |ref64| %.3g (|ref32 - ref64| %.3g)" % (
        what, bad.sum(), err[bad].max(), np.abs(r64[bad]).max(), d32[bad].max())
    return err


def _pattern(n, c):
    """Workgroup w (envs 4w .. 4w + 3) has ((w + c) % 5) active envs: 0, 1, 2, 3 and 4 across the batch."""
    i = np.arange(n)
    return (i % 4) < ((i // 4 + c) % 5)


def _cfg(Z, task, zones, **over):
    over.setdefault("zones_keepout", 0.3 if zones > 15 else 0.45)
    return Z.default_config(task, zones, **over)


def _env(Z, cfg, n, seed, goals, steps=3):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(seed, n)
    env.schedule_sequential()
    if goals:
        env.enable_goals()
    env.reset()
    rs = np.random.RandomState(seed)
    for _ in range(steps):
        env.step(rs.uniform(-1, 1, (n, 2)).astype(np.float32), auto_reset=True)
    return env


def _random_goals(env, active, rs):
    """A random available zone for every active env, -1 elsewhere."""
    avail = env.goal_info()[2]
    g = np.full(env.num_envs, -1, np.int32)
    for i in np.nonzero(active)[0]:
        opts = [z for z in range(env.num_zones) if (int(avail[i]) >> z) & 1]
        g[i] = rs.choice(opts)
    return g


def _goal_xy(env, goal):
    zo = env.observations()[1]
    return zo[np.arange(env.num_envs), np.where(goal >= 0, goal, 0), :2].astype(np.float32)


def _argmax_gap(l64):
    """-> (argmax over the finite logits, gap to the runner-up) per row; the gap is inf with one candidate."""
    best = np.argmax(l64, axis=1)
    if l64.shape[1] < 2:
        return best, np.full(len(l64), np.inf)
    srt = np.sort(l64, axis=1)
    gap = srt[:, -1] - srt[:, -2]
    return best, np.where(np.isfinite(gap), gap, np.inf)


def _drop_critics(sd, hi, lo):
    for d, keep in zip(sd, (hi, lo)):
        if not keep:
            for k in [k for k in d if k.startswith("critic.")]:
                del d[k]
    return sd


# (task, Z, h, N, weight scale, hi critic, lo critic): every h, Z and N edge of the issue at least once, F = 6 and 7
HIER_CASES = [
    (TSP, 1, 1, 1, 1.0, True, True), (TSP, 2, 2, 2, 0.1, True, False), (TTSP, 3, 31, 3, 1.0, False, True),
    (TSP, 7, 32, 4, 3.0, True, True), (CM, 8, 33, 5, 1.0, False, False), (TTSP, 9, 63, 7, 0.1, True, True),
    (TSP, 16, 65, 7, 3.0, True, False), (CM, 9, 127, 5, 1.0, True, True), (TTSP, 31, 129, 4, 1.0, False, True),
    (TSP, 32, 190, 3, 0.1, True, True), (TTSP, 32, 191, 7, 3.0, True, True), (CM, 16, 191, 2, 3.0, True, False),
    (TSP, 8, 2, 1, 3.0, False, True), (TSP, 9, 33, 10001, 1.0, True, True),
]


@pytest.mark.parametrize("ci", range(len(HIER_CASES)))
def test_hier_forward_and_mean_pick_sweep(zenv_mod, ci):
    Z = zenv_mod
    task, zones, h, n, scale, hc, lc = HIER_CASES[ci]
    env = _env(Z, _cfg(Z, task, zones), n, 101 + ci, goals=True)
    assert env.zone_feat == (6 if task == TSP else 7)
    hi, lo = _drop_critics(hier_ref.random_state_dicts(env.zone_feat, h=h, seed=ci, weight_scale=scale), hc, lc)
    env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
    rs = np.random.RandomState(ci)
    active = _pattern(n, ci)
    env.set_goals(_random_goals(env, active, rs))
    logits, hv, mu, std, lv = env.hier_forward()
    o, zo = env.observations()
    _, need, avail, goal0 = env.goal_info()
    assert np.array_equal(goal0 >= 0, active) and np.array_equal(need, ~active)
    rl64, rhv64 = hier_ref.high(hi, o, zo, avail, dtype=F64)
    rl32, rhv32 = hier_ref.high(hi, o, zo, avail)
    lerr = _check(logits, rl64, rl32, scale, "hier logits")
    _check(hv, rhv64, rhv32, scale, "hier hi value")
    if not hc:
        assert not hv.any()
    gxy = _goal_xy(env, goal0)
    r64 = hier_ref.low(lo, o, zo, gxy, dtype=F64)
    r32 = hier_ref.low(lo, o, zo, gxy)
    for name, d, a, b in zip(("mu", "std", "lo value"), (mu, std, lv), r64, r32):
        _check(d[active], a[active], b[active], scale, "hier " + name)
        assert not d[~active].any(), name                     # no goal: zeros exactly
    if not lc:
        assert not lv.any()

    # pick mode: the envs without a goal get the float64 argmax, the others keep theirs
    env.policy(Z.POLICY_HIER_MEAN)
    _, need1, _, goal = env.goal_info()
    assert np.array_equal(goal[active], goal0[active]) and (goal >= 0).all() and not need1.any()
    pick = ~active
    best, gap = _argmax_gap(rl64)
    clear = pick & (gap > np.maximum(1e-6, 2 * lerr.max(axis=1)))
    assert np.array_equal(goal[clear], best[clear])
    assert np.all((avail[pick] >> goal[pick].astype(np.uint32)) & 1)
    # the action is mu of the low level towards the new goals (every env has one now)
    a, mu1 = env.get(Z.F_ACTIONS), env.get(Z.F_POLICY_MU)
    assert np.array_equal(a, mu1)
    env.close()


# (task, Z, h, S, N, weight scale, hi critic, lo critic)
SKILL_CASES = [
    (TSP, 1, 1, 1, 1, 1.0, True, True), (TTSP, 2, 2, 2, 2, 0.1, False, True), (CM, 3, 31, 3, 3, 1.0, True, False),
    (TSP, 8, 32, 16, 4, 3.0, True, True), (TTSP, 9, 33, 31, 5, 1.0, False, False), (CM, 7, 63, 32, 7, 0.1, True, True),
    (TSP, 32, 191, 32, 7, 1.0, True, True), (TTSP, 31, 129, 31, 4, 3.0, True, False),
    (TSP, 16, 190, 2, 5, 1.0, False, True), (CM, 9, 65, 16, 3, 3.0, True, True), (TTSP, 32, 127, 1, 2, 3.0, True, True),
    (TSP, 8, 127, 3, 10001, 1.0, True, True),
]


@pytest.mark.parametrize("ci", range(len(SKILL_CASES)))
def test_skill_forward_and_mean_pick_sweep(zenv_mod, ci):
    Z = zenv_mod
    task, zones, h, S, n, scale, hc, lc = SKILL_CASES[ci]
    env = _env(Z, _cfg(Z, task, zones), n, 201 + ci, goals=False)
    hi, lo = _drop_critics(skill_ref.random_state_dicts(env.zone_feat, S, h=h, seed=ci, weight_scale=scale), hc, lc)
    env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo))
    rs = np.random.RandomState(ci)
    active = _pattern(n, ci + 2)
    skill0 = np.where(active, rs.randint(0, S, n), -1).astype(np.int32)
    if S > 1:
        skill0[np.nonzero(active)[0][:1]] = S - 1                # the last skill row at least once
    env.set_skills(skill0)
    logits, hv, mu, std, lv = env.skill_forward()
    o, zo = env.observations()
    assert logits.shape == (n, S) and np.array_equal(env.get(Z.F_SKILL), skill0)
    rl64, rhv64 = skill_ref.high(hi, o, zo, dtype=F64)
    rl32, rhv32 = skill_ref.high(hi, o, zo)
    lerr = _check(logits, rl64, rl32, scale, "skill logits")
    _check(hv, rhv64, rhv32, scale, "skill hi value")
    if not hc:
        assert not hv.any()
    sk = np.where(active, skill0, 0)
    r64 = skill_ref.low(lo, o, zo, sk, S, dtype=F64)
    r32 = skill_ref.low(lo, o, zo, sk, S)
    for name, d, a, b in zip(("mu", "std", "lo value"), (mu, std, lv), r64, r32):
        _check(d[active], a[active], b[active], scale, "skill " + name)
        assert not d[~active].any(), name                     # no skill: zeros exactly
    if not lc:
        assert not lv.any()

    env.policy(Z.POLICY_SKILL_MEAN)
    skill = env.get(Z.F_SKILL)
    assert np.array_equal(skill[active], skill0[active]) and (skill >= 0).all() and (skill < S).all()
    pick = ~active
    best, gap = _argmax_gap(rl64)
    clear = pick & (gap > np.maximum(1e-6, 2 * lerr.max(axis=1)))
    assert np.array_equal(skill[clear], best[clear])
    assert np.array_equal(env.get(Z.F_SKILL_AGE), np.ones(n, np.int32))     # 0 at the pick, + 1 for the action
    assert np.array_equal(env.get(Z.F_ACTIONS), env.get(Z.F_POLICY_MU))
    env.close()


# ---------------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("task", [TSP, TTSP])
def test_zone_31_and_zone_0_alone(zenv_mod, task):
    """Z = 32 with every zone but 31 visited from the start: bit 31 (the sign bit of the mask) is the only available
    goal, for the argmax and the draw alike; and every zone but 0."""
    Z = zenv_mod
    n = 23
    for vis0, want in ((0x7FFFFFFF, 31), (0xFFFFFFFE, 0)):
        for policy in (Z.POLICY_HIER_MEAN, Z.POLICY_HIER_SAMPLE):
            env = _env(Z, _cfg(Z, task, 32, visited0=vis0), n, 7, goals=True, steps=2)
            hi, lo = hier_ref.random_state_dicts(env.zone_feat, h=33, seed=31)
            env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
            _, need, avail, _ = env.goal_info()
            assert need.all() and (avail == (~np.uint32(vis0))).all()
            logits = env.hier_forward()[0]
            fin = np.isfinite(logits)
            assert fin[:, want].all() and fin.sum() == n
            env.policy(policy, policy_seed=3)
            assert (env.goal_info()[3] == want).all()
            env.close()


def test_no_available_zone(zenv_mod):
    """The mask is empty only once every zone is visited, which ends the TSP episode: with auto_reset off the env stays
    finished, and a finished env never picks (ZENV_POLICY_HIER_*: goal -1, action 0).  The forward pass still evaluates
    it: every logit -inf."""
    Z = zenv_mod
    n = 12
    env = _env(Z, _cfg(Z, TSP, 2, visited0=0b01, num_steps=1000), n, 13, goals=True, steps=0)
    hi, lo = hier_ref.random_state_dicts(env.zone_feat, h=32, seed=2)
    env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
    for _ in range(400):                                      # the greedy policy drives to zone 1, the last one
        env.policy(Z.POLICY_GREEDY)
        env.step(None, auto_reset=False)
        if env.get(Z.F_DONE).all():
            break
    assert env.get(Z.F_DONE).all()
    _, need, avail, goal = env.goal_info()
    assert not avail.any() and need.all() and (goal == -1).all()
    logits, hv = env.hier_forward()[:2]
    assert (logits == -np.inf).all() and np.isfinite(hv).all()
    for policy in (Z.POLICY_HIER_MEAN, Z.POLICY_HIER_SAMPLE):
        env.policy(policy, policy_seed=8)
        assert (env.goal_info()[3] == -1).all() and not env.get(Z.F_ACTIONS).any()
    env.close()


def _tie_sample(u, avail_rows):
    """The kernel's float32 inverse CDF on k equal logits: the first available index whose running count exceeds
    float32(u) * float32(k)."""
    out = []
    for ui, zs in zip(u, avail_rows):
        thr = np.float32(ui) * np.float32(len(zs))
        out.append(next((z for c, z in enumerate(zs, 1) if np.float32(c) > thr), zs[-1]))
    return np.array(out)


def test_ties_go_to_the_lowest_zone_and_the_exact_draw(zenv_mod):
    """actor.2's weight zeroed: every logit is its bias.  The argmax keeps the lowest available zone (strict >), and
    the draw lands where the kernel's float32 inverse CDF puts the host uniform, env by env."""
    Z = zenv_mod
    n, seed, index0 = 517, 0x1234567890, 77
    for policy in (Z.POLICY_HIER_MEAN, Z.POLICY_HIER_SAMPLE):
        env = _env(Z, _cfg(Z, TSP, 9, visited0=0b000000101), n, 17, goals=True, steps=4)
        hi, lo = hier_ref.random_state_dicts(env.zone_feat, h=65, seed=4)
        hi["actor.2.weight"] = torch.zeros_like(hi["actor.2.weight"])          # every logit = actor.2's bias
        env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
        rs = np.random.RandomState(1)
        env.set_goals(_random_goals(env, rs.rand(n) < 0.3, rs))
        _, need, avail, goal0 = env.goal_info()
        logits = env.hier_forward()[0]
        fin = np.isfinite(logits)
        assert np.all(logits[fin] == np.float32(hi["actor.2.bias"][0]))
        step = env.step_count
        env.policy(policy, policy_seed=seed, env_index0=index0)
        goal = env.goal_info()[3]
        pick = need & (goal0 < 0)
        assert pick.sum() > n // 2 and np.array_equal(goal[~pick], goal0[~pick])
        rows = [[z for z in range(9) if (int(avail[i]) >> z) & 1] for i in np.nonzero(pick)[0]]
        if policy == Z.POLICY_HIER_MEAN:
            want = np.array([r[0] for r in rows])
        else:
            u = philox_ref.goal_uniform(n, seed, index0, step)[pick]
            want = _tie_sample(u, rows)
            assert len(set(want.tolist())) > 3
        assert np.array_equal(goal[pick], want)
        env.close()


def test_skill_ties_go_to_skill_0_and_the_exact_draw(zenv_mod):
    """actor.discrete_.0 constant: S = 31 equal logits.  The argmax keeps skill 0, the draw is exact per env."""
    Z = zenv_mod
    n, S, seed, index0 = 401, 31, 99, 5
    for policy in (Z.POLICY_SKILL_MEAN, Z.POLICY_SKILL_SAMPLE):
        env = _env(Z, _cfg(Z, TTSP, 8), n, 19, goals=False, steps=4)
        hi, lo = skill_ref.random_state_dicts(env.zone_feat, S, h=33, seed=5)
        hi["actor.discrete_.0.weight"] = torch.zeros_like(hi["actor.discrete_.0.weight"])
        hi["actor.discrete_.0.bias"] = torch.full_like(hi["actor.discrete_.0.bias"], 0.3)
        env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo))
        active = _pattern(n, 1)
        env.set_skills(np.where(active, 3, -1).astype(np.int32))
        step = env.step_count
        env.policy(policy, policy_seed=seed, env_index0=index0)
        skill = env.get(Z.F_SKILL)
        assert (skill[active] == 3).all()
        pick = ~active
        if policy == Z.POLICY_SKILL_MEAN:
            want = np.zeros(pick.sum(), np.int64)
        else:
            u = philox_ref.skill_uniform(n, seed, index0, step)[pick]
            want = _tie_sample(u, [list(range(S))] * int(pick.sum()))
            assert len(set(want.tolist())) > 10
        assert np.array_equal(skill[pick], want)
        env.close()


# ---------------------------------------------------------------------------------------------------- exact draws
def _inverse_cdf(l64, u):
    """Categorical draw of the float64 softmax over the finite logits at uniform u: (index, |distance of u to the
    nearest CDF boundary|)."""
    m = np.where(np.isfinite(l64), l64, -np.inf).max(axis=1, keepdims=True)
    p = np.where(np.isfinite(l64), np.exp(l64 - m), 0.0)
    cdf = np.cumsum(p, axis=1) / p.sum(axis=1, keepdims=True)
    u = np.asarray(u, np.float64)[:, None]
    idx = np.argmax(cdf > u, axis=1)
    bound = np.where(p > 0, np.abs(cdf - u), np.inf).min(axis=1)
    return idx, bound


def _check_action(a, mu, std, n, seed, index0, step, what):
    eps = philox_ref.action_noise(n, seed, index0, step)
    mu, std = mu.astype(np.float64), std.astype(np.float64)
    want = mu + std * eps
    mag = np.abs(mu) + std * np.hypot(eps[:, :1], eps[:, 1:])
    ulps = np.abs(a.astype(np.float64) - want) / (mag * 2.0 ** -23)
    _note("action ulps " + what, ulps.max())
    assert ulps.max() <= ACT_ULPS, (what, float(ulps.max()))


@pytest.mark.parametrize("seed", [4, 0xDEADBEEF12345])
def test_hier_sample_draws_exactly(zenv_mod, seed):
    """HIER_SAMPLE: the goal of every picking env is the float64 inverse CDF at the host Philox uniform (envs within
    1e-5 of a CDF boundary excepted, and counted); the action is mu + std * eps at the host Box-Muller pair."""
    Z = zenv_mod
    n, index0 = 1500, 123457
    env = _env(Z, _cfg(Z, TSP, 9), n, 23, goals=True, steps=6)
    hi, lo = hier_ref.random_state_dicts(env.zone_feat, h=65, seed=6)
    env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
    rs = np.random.RandomState(seed & 0xFFFF)
    env.set_goals(_random_goals(env, _pattern(n, 3), rs))
    o, zo = env.observations()
    _, need, avail, goal0 = env.goal_info()
    l64, _ = hier_ref.high(hi, o, zo, avail, dtype=F64)
    step = env.step_count
    assert step > 0
    env.policy(Z.POLICY_HIER_SAMPLE, policy_seed=seed, env_index0=index0)
    goal = env.goal_info()[3]
    pick = need & (goal0 < 0)
    assert np.array_equal(goal[~pick], goal0[~pick]) and pick.sum() > n // 3
    u = philox_ref.goal_uniform(n, seed, index0, step)
    want, bound = _inverse_cdf(l64, u)
    near = pick & (bound < 1e-5)
    assert near.sum() <= 3
    ok = pick & ~near
    assert np.array_equal(goal[ok], want[ok]), np.nonzero(ok & (goal != want))[0][:8]
    assert len(set(goal[ok].tolist())) >= 5
    _check_action(env.get(Z.F_ACTIONS), env.get(Z.F_POLICY_MU), env.get(Z.F_POLICY_STD), n, seed, index0, step,
                  "HIER_SAMPLE")
    env.close()


@pytest.mark.parametrize("seed", [4, 0xDEADBEEF12345])
def test_skill_sample_draws_exactly(zenv_mod, seed):
    """SKILL_SAMPLE: the skill of every picking env is the float64 inverse CDF at the host Philox uniform; the action
    is mu + std * eps.  Weight scale 2, so that the skill probabilities are far from uniform."""
    Z = zenv_mod
    n, S, index0 = 1500, 16, 98765
    env = _env(Z, _cfg(Z, TTSP, 9), n, 29, goals=False, steps=5)
    hi, lo = skill_ref.random_state_dicts(env.zone_feat, S, h=65, seed=7, weight_scale=2.0)
    env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo))
    active = _pattern(n, 4)
    env.set_skills(np.where(active, 1, -1).astype(np.int32))
    o, zo = env.observations()
    l64, _ = skill_ref.high(hi, o, zo, dtype=F64)
    step = env.step_count
    env.policy(Z.POLICY_SKILL_SAMPLE, policy_seed=seed, env_index0=index0)
    skill = env.get(Z.F_SKILL)
    pick = ~active
    assert (skill[active] == 1).all()
    want, bound = _inverse_cdf(l64, philox_ref.skill_uniform(n, seed, index0, step))
    near = pick & (bound < 1e-5)
    assert near.sum() <= 3
    ok = pick & ~near
    assert np.array_equal(skill[ok], want[ok]), np.nonzero(ok & (skill != want))[0][:8]
    assert len(set(skill[ok].tolist())) >= 8
    _check_action(env.get(Z.F_ACTIONS), env.get(Z.F_POLICY_MU), env.get(Z.F_POLICY_STD), n, seed, index0, step,
                  "SKILL_SAMPLE")
    env.close()


def test_mlp_sample_action_draws_exactly(zenv_mod):
    """MLP_SAMPLE (the flat network, float32 kernel): the action is mu + std * eps at the host Box-Muller pair."""
    from oracle import policy_ref as P
    Z = zenv_mod
    n, seed, index0 = 1000, 0xABCDEF0123, 4242
    env = _env(Z, _cfg(Z, TSP, 9), n, 31, goals=False, steps=7)
    env.load_mlp(P.random_tensors(env.zone_feat, h=64, seed=2), precision="f32")
    step = env.step_count
    env.policy(Z.POLICY_MLP_SAMPLE, policy_seed=seed, env_index0=index0)
    _check_action(env.get(Z.F_ACTIONS), env.get(Z.F_POLICY_MU), env.get(Z.F_POLICY_STD), n, seed, index0, step,
                  "MLP_SAMPLE")
    env.close()


# ---------------------------------------------------------------------------------------------------- zenv_collect_hier
def _collect_env(Z, cfg, n, seed=11, first=None):
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(seed, n)
    if first is None:
        env.schedule_sequential()
    else:
        env.schedule_sequential(first=first, stride=0)          # env i restarts on map i: no dependence on N
    env.enable_goals()
    env.reset()
    return env


def _agent(Z, envs, F, h, seed):
    hi_sd, lo_sd = hier_ref.random_state_dicts(F, h=h, seed=seed)
    lo_sd["actor.mu_.bias"] = lo_sd["actor.mu_.bias"] + torch.tensor([4.0, 0.0])      # drive forward: goals reached
    for e in envs:
        e.load_hier(Z.hier_tensors_from_state_dicts(hi_sd, lo_sd))
    return hi_sd, lo_sd


def _check_rows(hi, exp_c, rec, n, nz):
    """The high-level rows of one call against the restatement's rows of that call."""
    counts = [len(r) for r in exp_c]
    assert np.array_equal(hi["count"], counts) and len(hi["action"]) == sum(counts)
    rows = [r for per_env in exp_c for r in per_env]
    if not rows:
        return 0
    tp = np.array([r["t_pick"] for r in rows])
    jj = np.repeat(np.arange(n), counts)
    assert np.array_equal(hi["action"], [r["goal"] for r in rows])
    assert np.array_equal(hi["obs"], rec["obs"][tp, jj]) and np.array_equal(hi["zone_obs"], rec["zone_obs"][tp, jj])
    bits = (rec["avail"][tp, jj][:, None] >> np.arange(nz, dtype=np.uint32)) & 1
    assert np.array_equal(hi["action_mask"], bits.astype(bool))
    assert np.array_equal(hi["value"], [r["value"] for r in rows])
    assert np.array_equal(hi["reward"], np.array([r["reward"] for r in rows], np.float32))
    assert np.array_equal(hi["mask"], [r["mask"] for r in rows])
    want_lp = [log_softmax_at(rec["logits"][t, j], g) for t, j, g in zip(tp, jj, hi["action"])]
    assert np.abs(hi["log_prob"] - want_lp).max() < 1e-5
    assert np.abs(hi["advantage"] - [r["adv"] for r in rows]).max() < 1e-5
    assert np.abs(hi["returnn"] - (hi["value"] + hi["advantage"])).max() < 1e-5
    return len(rows)


def _collect_vs_replay(Z, cfg, n, Ts, h, seed=5, wseed=3):
    """Calls of Ts[c] frames on one handle against zenv_policy(HIER_SAMPLE) + zenv_step on another; returns the rows
    per call, what the restatement met, and the handle's zone count."""
    a, b = _collect_env(Z, cfg, n), _collect_env(Z, cfg, n)
    _agent(Z, (a, b), a.zone_feat, h, wseed)
    outs, v_final = [], []
    for T in Ts:
        lo, hi = a.collect_hier(T, policy_seed=seed, discount=GAMMA, gae_lambda=LAM)
        outs.append(hi)
        v_final.append(a.get(Z.F_HIER_VALUE))
    rec = replay(Z, b, sum(Ts), seed)
    exp, seen = expected_hi(rec, Ts, len(Ts), v_final)
    n_rows = [_check_rows(hi, exp[c], rec, n, a.num_zones) for c, hi in enumerate(outs)]
    nz = a.num_zones
    a.close()
    b.close()
    return n_rows, seen, nz, outs


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_collect_hier_at_the_scan_tile_edge(zenv_mod, n):
    """One workgroup scans the per-env counts in tiles of 4 096: a batch one short of a tile, exactly one, one over."""
    Z = zenv_mod
    # episodes of 15 steps: both calls close transitions, some of them opened in the call before
    cfg = _cfg(Z, TSP, 6, num_steps=15)
    n_rows, seen, _, outs = _collect_vs_replay(Z, cfg, n, [20, 20], h=33)
    assert min(n_rows) >= n and seen["span"] > 0 and seen["mask0"] > 0, seen
    assert all((hi["count"] > 0).all() for hi in outs)        # the last env of the batch included


@pytest.mark.parametrize("h", [1, 191])
def test_collect_hier_with_the_widest_zone_rows(zenv_mod, h):
    """TimedTSP with 32 zones: rows of Z * F = 224 floats through the gather and the carry, h at both ends."""
    Z = zenv_mod
    cfg = _cfg(Z, TTSP, 32, num_steps=20)
    n_rows, seen, nz, outs = _collect_vs_replay(Z, cfg, 61, [15, 15], h=h)
    assert nz == 32 and outs[0]["zone_obs"].shape[1:] == (32, 7)
    assert min(n_rows) > 0 and seen["span"] > 0 and seen["mask0"] > 0, seen


def test_collect_hier_after_a_call_without_rows(zenv_mod):
    """A call that closes no transition (M = 0: nothing gathered) must still carry the transitions it opened: the
    next call's rows start with them, goal, value and log_prob of their pick in frame 0 of the empty call."""
    Z = zenv_mod
    n = 300
    cfg = _cfg(Z, TSP, 9, num_steps=20)
    n_rows, seen, _, outs = _collect_vs_replay(Z, cfg, n, [2, 25], h=65)
    assert n_rows[0] == 0 and len(outs[0]["action"]) == 0 and not outs[0]["count"].any()
    assert n_rows[1] > 0 and seen["span"] >= n // 2, seen


def test_collect_hier_rows_over_several_scan_tiles(zenv_mod):
    """N = 3 * 4 096 + 1: the rows of every env, split by cumsum(count), equal those of the same env in a handle of its
    own tail (the same maps, env_index0 shifted): a wrong offset at a tile boundary shows as a neighbour's rows."""
    Z = zenv_mod
    n, off, T, seed = 3 * 4096 + 1, 8190, 25, 9
    cfg = _cfg(Z, TSP, 6, num_steps=20, zones_size=0.5)
    big = _collect_env(Z, cfg, n, seed=11, first=np.arange(n, dtype=np.int32))
    small = _collect_env(Z, cfg, n - off, seed=11 + off, first=np.arange(n - off, dtype=np.int32))
    _agent(Z, (big, small), big.zone_feat, 33, 8)
    out = []
    for env, index0 in ((big, 0), (small, off)):
        calls = [env.collect_hier(T, policy_seed=seed, env_index0=index0)[1] for _ in range(2)]
        out.append(calls)
    big.close()
    small.close()
    for hb, hs in zip(*out):
        assert np.array_equal(hb["count"][off:], hs["count"])
        cb = np.concatenate([[0], np.cumsum(hb["count"])])
        cs = np.concatenate([[0], np.cumsum(hs["count"])])
        assert cb[-1] == len(hb["action"]) and cs[-1] == len(hs["action"])
        for tile in range(4):                                 # every scan tile has rows
            assert hb["count"][tile * 4096:(tile + 1) * 4096].sum() > 0
        for k in hb:
            if k == "count":
                continue
            assert np.array_equal(hb[k][cb[off]:], hs[k]), k
