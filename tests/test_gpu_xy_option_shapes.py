"""The xy-goals agent's (csrc/xy_f32.hip) and the Options agent's (csrc/option_f32.hip) kernels at the edges of their
layout, as tests/test_gpu_hier_shapes.py holds the Zone-goals and the fixed-length-skills agent:

* both networks over the HIER_CASES / SKILL_CASES grids (h around the 32-feature tiles up to 191, Z = 1 .. 32 around the
  32-row passes of encode_envs, N = 1 .. 7 and one five-digit N, workgroups of EB = 4 envs with 0 .. 4 active ones,
  S up to 32, absent critics, weight scales 0.1, 1 and 3) against the float64 restatement (tests/xy_ref.py,
  tests/option_ref.py with dtype=float64) under that module's rule _check / K_F32, with the sigmoid heads rescaled per
  case so that no pre-activation of the reference exceeds 4 (a saturated head hides a wrong term);
* an env's outputs do not depend on its slot in the workgroup or on its neighbours, for all four agents: two handles on
  one map bank, the second with its envs permuted, and two activity patterns on the same state, bit for bit;
* k_option_list's compacted picker list at its edges (a list of 0, 1, 4k + r entries, the last env alone, a short list
  right after a long one) against the early-exit form, bit for bit;
* the exact draws at S = 1 and 32 (Options) and in a workgroup of 1 and 3 envs (xy-goals)."""
import numpy as np
import pytest
import torch

from tests import hier_ref, option_ref, philox_ref, skill_ref, xy_ref
from tests.test_gpu_hier_shapes import (ACT_ULPS, CM, HIER_CASES, SKILL_CASES, TSP, WORST, _argmax_gap, _cfg, _check,
                                        _drop_critics, _env, _note, _pattern, _random_goals)
from tests.test_gpu_options import check_draws
from tests.test_gpu_xy_goals import _ulps

pytestmark = pytest.mark.gpu

F64 = torch.float64
PRE_MAX = 4.0          # the largest float64 head pre-activation a sweep case may have (sigmoid(4) = 0.982)
# Measured on the two sweeps (the report printed at the end of the module): no element of any output left the plain bar
# 1e-5 max(1, |ref64|), so the K_F32 term of _check never decided a case.  The worst |dev - ref64| in units of that bar,
# at weight scale 0.1 / 1 / 3: xy goal_mu 0.007 / 0.019 / 0.18, goal_std 0.006 / 0.009 / 0.08, hi value 0.002 / 0.024 /
# 0.30, mu 0.009 / 0.019 / 0.12, std 0.006 / 0.011 / 0.08, lo value 0.007 / 0.039 / 0.17; option logits 0.019 / 0.035 /
# 0.65, hi value 0.003 / 0.038 / 0.43, mu 0.010 / 0.040 / 0.15, std 0.004 / 0.020 / 0.04, lo value 0.001 / 0.068 / 0.27.
# The draws: a_2 0.89 ulps, the xy goal 0.80, the xy action 1.3 (bar ACT_ULPS = 4).


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        if k.startswith(("xy ", "option ")):
            print("xy / option shapes worst: %-44s %.4g" % (k, WORST[k]))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _cmp(dev, r64, r32, scale, what):
    """_check (which records err / d32 of the elements beyond the plain bar), and for the report, over all elements:
    the worst |dev - ref64| in units of the plain bar 1e-5 max(1, |ref64|), and the kernel's worst error over torch
    float32's worst error, max |dev - ref64| / max |ref32 - ref64|."""
    err = _check(dev, r64, r32, scale, what)
    if err.size:
        r64, r32 = np.asarray(r64, np.float64), np.asarray(r32, np.float64)
        fin = np.isfinite(r64)
        _note(what + " err/bar (scale %g)" % scale, (err / (1e-5 * np.maximum(1.0, np.abs(r64)))).max())
        d32 = np.abs(r32[fin] - r64[fin]).max(initial=0.0)
        if d32 > 0:
            _note(what + " max err/max d32 (scale %g)" % scale, err.max() / d32)
    return err


# ---------------------------------------------------------------------------------------------------- float64 sweeps
@pytest.mark.parametrize("ci", range(len(HIER_CASES)))
def test_xy_forward_and_mean_pick_sweep(zenv_mod, ci):
    Z = zenv_mod
    task, zones, h, n, scale, hc, lc = HIER_CASES[ci]
    env = _env(Z, _cfg(Z, task, zones), n, 301 + ci, goals=False)
    try:
        assert env.zone_feat == (6 if task == TSP else 7)
        hi, lo = _drop_critics(xy_ref.random_state_dicts(env.zone_feat, h=h, seed=ci, weight_scale=scale), hc, lc)
        rs = np.random.RandomState(ci)
        active = _pattern(n, ci)
        goals = rs.uniform(-2, 2, (n, 2)).astype(np.float32)
        o, zo = env.observations()
        for pre in xy_ref.normalise_heads(hi, lo, o, zo, goals, active):
            assert np.abs(pre).max(initial=0.0) <= PRE_MAX         # no head of the reference is saturated
        env.load_xy(Z.xy_tensors_from_state_dicts(hi, lo))
        env.set_xy_goals(goals, active)
        gmu, gstd, hv, mu, std, lv = env.xy_forward()
        for a, b in zip((o, zo), env.observations()):
            _same(a, b, "observations")
        _same(env.get(Z.F_XY_GOAL)[active], goals[active], "planted goals")
        assert np.array_equal(env.get(Z.F_XY_GOAL_AGE), np.where(active, 0, -1))

        r64, r32 = xy_ref.high(hi, o, zo, dtype=F64), xy_ref.high(hi, o, zo)
        for name, d, a, b in zip(("goal_mu", "goal_std", "hi value"), (gmu, gstd, hv), r64, r32):
            _cmp(d, a, b, scale, "xy " + name)                      # every env
        assert hc or not hv.any()
        g0 = np.where(active[:, None], goals, 0).astype(np.float32)
        r64, r32 = xy_ref.low(lo, o, zo, g0, dtype=F64), xy_ref.low(lo, o, zo, g0)
        for name, d, a, b in zip(("mu", "std", "lo value"), (mu, std, lv), r64, r32):
            _cmp(d[active], a[active], b[active], scale, "xy " + name)
            assert not d[~active].any(), name                      # no goal: zeros exactly
        assert lc or not lv.any()

        # XY_MEAN: the envs without a goal take goal_mu itself, the others keep theirs; the action is mu
        env.policy(Z.POLICY_XY_MEAN)
        goal1, gmu1 = env.get(Z.F_XY_GOAL), env.get(Z.F_XY_GOAL_MU)
        _same(goal1[~active], gmu1[~active], "picked goal")
        _same(goal1[active], goals[active], "kept goal")
        _same(gmu1, gmu, "goal_mu of the pick")                    # the same observations: the forward pass's rows
        mu1 = env.get(Z.F_POLICY_MU)
        _same(env.get(Z.F_ACTIONS), mu1, "action")
        assert np.array_equal(env.get(Z.F_XY_GOAL_AGE), np.ones(n, np.int32))
        _same(mu1[active], mu[active], "mu under a kept goal")
        # every env has a goal now: the low level of all of them under the device's own goals
        r64, r32 = xy_ref.low(lo, o, zo, goal1, dtype=F64), xy_ref.low(lo, o, zo, goal1)
        for name, f, a, b in zip(("mu", "std", "lo value"), (Z.F_POLICY_MU, Z.F_POLICY_STD, Z.F_POLICY_VALUE), r64, r32):
            _cmp(env.get(f), a, b, scale, "xy %s after the pick" % name)
    finally:
        env.close()


@pytest.mark.parametrize("ci", range(len(SKILL_CASES)))
def test_option_forward_and_mean_pick_sweep(zenv_mod, ci):
    Z = zenv_mod
    task, zones, h, S, n, scale, hc, lc = SKILL_CASES[ci]
    env = _env(Z, _cfg(Z, task, zones), n, 401 + ci, goals=False)
    try:
        hi, lo = _drop_critics(option_ref.random_state_dicts(env.zone_feat, S, h=h, seed=ci, weight_scale=scale), hc, lc)
        rs = np.random.RandomState(ci)
        active = _pattern(n, ci + 2)
        skill0 = np.where(active, rs.randint(0, S, n), -1).astype(np.int32)
        if S > 1 and active.any():
            skill0[np.nonzero(active)[0][:1]] = S - 1                # the last skill column at least once
            assert (skill0 == S - 1).any()
        o, zo = env.observations()
        pre = option_ref.normalise_heads(lo, o, zo, skill0, S)
        assert pre.shape == (active.sum(), 6) and np.abs(pre).max(initial=0.0) <= PRE_MAX
        env.load_options(Z.option_tensors_from_state_dicts(hi, lo))
        env.set_skills(skill0)
        logits, hv, mu, std, lv, tmu, tstd, tprob = env.option_forward()
        ta = env.get(Z.F_OPTION_TERM_ACTION)
        for a, b in zip((o, zo), env.observations()):
            _same(a, b, "observations")
        assert logits.shape == (n, S) and np.array_equal(env.get(Z.F_SKILL), skill0)

        rl64, rhv64 = option_ref.high(hi, o, zo, dtype=F64)
        rl32, rhv32 = option_ref.high(hi, o, zo)
        lerr = _cmp(logits, rl64, rl32, scale, "option logits")        # every env
        _cmp(hv, rhv64, rhv32, scale, "option hi value")
        assert hc or not hv.any()
        sk = np.where(active, skill0, 0)
        r64, r32 = option_ref.low(lo, o, zo, sk, S, dtype=F64), option_ref.low(lo, o, zo, sk, S)
        dmu, dstd = np.concatenate([mu, tmu[:, None]], axis=1), np.concatenate([std, tstd[:, None]], axis=1)
        for name, d, a, b in zip(("mu", "std", "lo value"), (dmu, dstd, lv), r64, r32):
            _cmp(d[active], a[active], b[active], scale, "option " + name)      # all three components
        _same(ta, tmu, "a_2 of the forward pass")
        assert np.all(np.abs(tprob[active] - option_ref.term_prob(ta[active])) <= 1e-5)
        for name, d in zip(("mu", "std", "lo value", "mu_2", "std_2", "a_2", "prob"), (mu, std, lv, tmu, tstd, ta, tprob)):
            assert not d[~active].any(), name                      # no skill: zeros exactly
        assert lc or not lv.any()

        # OPTION_MEAN: the envs without a skill get the float64 argmax, the others keep theirs
        env.policy(Z.POLICY_OPTION_MEAN)
        skill = env.get(Z.F_SKILL)
        assert np.array_equal(skill[active], skill0[active]) and (skill >= 0).all() and (skill < S).all()
        pick = ~active
        best, gap = _argmax_gap(rl64)
        clear = pick & (gap > np.maximum(1e-6, 2 * lerr.max(axis=1)))
        assert np.array_equal(skill[clear], best[clear])
        _same(env.get(Z.F_SKILL_LOGITS), logits, "logits of the pick")
        assert np.array_equal(env.get(Z.F_SKILL_AGE), np.ones(n, np.int32))
        tprob1 = env.get(Z.F_OPTION_TERM_PROB)
        assert np.array_equal(env.get(Z.F_OPTION_ENDED), (tprob1 > np.float32(0.5)).astype(np.int32))
        mu1, tmu1 = env.get(Z.F_POLICY_MU), env.get(Z.F_OPTION_TERM_MU)
        _same(env.get(Z.F_ACTIONS), mu1, "action")
        _same(env.get(Z.F_OPTION_TERM_ACTION), tmu1, "a_2")
        _same(mu1[active], mu[active], "mu under a kept skill")
        _same(tmu1[active], tmu[active], "mu_2 under a kept skill")
        # every env has a skill now: the low level of all of them under the device's own skills
        r64, r32 = option_ref.low(lo, o, zo, skill, S, dtype=F64), option_ref.low(lo, o, zo, skill, S)
        dmu = np.concatenate([mu1, tmu1[:, None]], axis=1)
        dstd = np.concatenate([env.get(Z.F_POLICY_STD), env.get(Z.F_OPTION_TERM_STD)[:, None]], axis=1)
        for name, d, a, b in zip(("mu", "std", "lo value"), (dmu, dstd, env.get(Z.F_POLICY_VALUE)), r64, r32):
            _cmp(d, a, b, scale, "option %s after the pick" % name)
    finally:
        env.close()


# ------------------------------------------------------------------------------- slots and neighbours change nothing
N_NB, H_NB, S_NB = 23, 33, 5
PERM = np.random.RandomState(12).permutation(N_NB)


class _Agent:
    """One of the four agents behind the same five calls.  n_hi: how many of forward()'s arrays are the high level's."""

    def __init__(self, Z, kind, F):
        self.Z, self.kind, self.n_hi = Z, kind, 3 if kind == "xy" else 2
        if kind == "hier":
            self.sd = hier_ref.random_state_dicts(F, h=H_NB, seed=41)
        elif kind == "skill":
            self.sd = skill_ref.random_state_dicts(F, S_NB, h=H_NB, seed=42)
        elif kind == "xy":
            self.sd = xy_ref.random_state_dicts(F, h=H_NB, seed=43)
        else:
            self.sd = option_ref.random_state_dicts(F, S_NB, h=H_NB, seed=44)

    def load(self, env):
        Z = self.Z
        if self.kind == "hier":
            env.load_hier(Z.hier_tensors_from_state_dicts(*self.sd))
        elif self.kind == "skill":
            env.load_skills(Z.skill_tensors_from_state_dicts(*self.sd))
        elif self.kind == "xy":
            env.load_xy(Z.xy_tensors_from_state_dicts(*self.sd))
        else:
            env.load_options(Z.option_tensors_from_state_dicts(*self.sd))

    def values(self, env, rs):
        """A goal or a skill for every env."""
        n = env.num_envs
        if self.kind == "hier":
            return _random_goals(env, np.ones(n, bool), rs)
        if self.kind == "xy":
            return rs.uniform(-2, 2, (n, 2)).astype(np.float32)
        return rs.randint(0, S_NB, n).astype(np.int32)

    def plant(self, env, active, vals):
        if self.kind == "hier":
            env.set_goals(np.where(active, vals, -1).astype(np.int32))
        elif self.kind == "xy":
            env.set_xy_goals(vals, active)
        else:
            env.set_skills(np.where(active, vals, -1).astype(np.int32))

    def forward(self, env):
        return getattr(env, self.kind + "_forward")()

    def planted(self, env):
        Z = self.Z
        if self.kind == "hier":
            return env.goal_info()[3] >= 0
        if self.kind == "xy":
            return env.get(Z.F_XY_GOAL_AGE) >= 0
        return env.get(Z.F_SKILL) >= 0


@pytest.mark.parametrize("task,zones", [(TSP, 25), (CM, 7), (TSP, 32), (TSP, 1)])
@pytest.mark.parametrize("kind", ["hier", "skill", "xy", "option"])
def test_an_env_does_not_depend_on_its_slot_or_its_neighbours(zenv_mod, kind, task, zones):
    """Handle A plays maps 0 .. 22 in order, handle B the same maps permuted, with A's actions permuted: B's env i is
    A's env PERM[i] in another workgroup slot among other neighbours.  Every output of the forward pass agrees bit for
    bit, under two activity patterns; and on A the low level of the envs active under both patterns is the same
    whichever of their neighbours are active.  A goal or skill cannot be taken away again, so the second pattern is
    planted after loading the weights anew (which clears the skill clock's state) or, for the Zone-goals agent, whose
    goals belong to the env, on a second pair of handles brought to the same state."""
    Z = zenv_mod
    n, perm, idx = N_NB, PERM, np.arange(N_NB)
    moved = perm % 4 != idx % 4
    assert moved.sum() * 4 >= 3 * n                                 # the permutation moves the slots ...
    assert set(perm[moved] % 4) == set(idx[moved] % 4) == {0, 1, 2, 3}        # ... from and to every one of them
    cfg = _cfg(Z, task, zones)
    acts = np.random.RandomState(zones).uniform(-1, 1, (3, n, 2)).astype(np.float32)
    opened = []

    def make(first):
        env = Z.ZoneVecEnv(cfg, n)
        opened.append(env)
        env.build_bank(777, n)
        env.schedule_sequential(first=first.astype(np.int32), stride=0)
        if kind == "hier":
            env.enable_goals()
        env.reset()
        for a in acts:
            env.step(a[first], auto_reset=True)
        agent.load(env)
        return env

    try:
        agent = _Agent(Z, kind, Z.zone_feat(cfg))
        A, B = make(idx), make(perm)
        for a, b in zip(A.observations(), B.observations()):
            _same(b, a[perm], "observations of the permuted handle")
            assert len(np.unique(a.reshape(n, -1), axis=0)) == n          # no two envs alike
        if kind == "hier":
            assert np.array_equal(B.goal_info()[2], A.goal_info()[2][perm])
        vals = agent.values(A, np.random.RandomState(5))
        outs = {}
        for c in (0, 3):
            active = _pattern(n, c)
            if c == 3:
                if kind == "hier":
                    A, B = make(idx), make(perm)
                    for a, b in zip(A.observations(), B.observations()):
                        _same(b, a[perm], "observations of the second pair")
                else:
                    agent.load(A)
                    agent.load(B)
            agent.plant(A, active, vals)
            agent.plant(B, active[perm], vals[perm])
            assert np.array_equal(agent.planted(A), active) and np.array_equal(agent.planted(B), active[perm])
            fa, fb = agent.forward(A), agent.forward(B)
            for k, (a, b) in enumerate(zip(fa, fb)):
                _same(b, a[perm], "output %d under pattern %d" % (k, c))
            for a in fa[agent.n_hi:]:
                assert a[active].any() and not a[~active].any()
            outs[c] = fa
        both = _pattern(n, 0) & _pattern(n, 3)
        assert both.sum() >= 4
        for k, (a, b) in enumerate(zip(outs[0], outs[3])):
            if k < agent.n_hi:
                _same(a, b, "high-level output %d" % k)                # the activity is not its business
            else:
                _same(a[both], b[both], "low-level output %d" % k)
    finally:
        for env in opened:
            env.close()


# ------------------------------------------------------------------------------- the compacted list of picking envs
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_option_picker_list_edges(zenv_mod, monkeypatch, n):
    """Two handles in the same state, the high level over env blocks (ZENV_OPTION_COMPACT=0) and over k_option_list's
    list (1), through planted picker sets: all, none, env 0, env N - 1, every other env, and env N - 1 right after
    all (stale entries beyond the count).  zenv_set_skills gives every env a skill, one OPTION_MEAN step ages it, and
    zenv_reset under the set's mask takes the skill from exactly the pickers (-1 in zenv_set_skills leaves an env as it
    is); the third mu_ row is the constant -100, so no option ends by itself."""
    Z = zenv_mod
    S, idx = 5, np.arange(n)
    fields = (Z.F_SKILL_LOGITS, Z.F_SKILL_VALUE, Z.F_SKILL, Z.F_SKILL_AGE, Z.F_OPTION_ENDED, Z.F_ACTIONS, Z.F_POLICY_MU,
              Z.F_POLICY_STD, Z.F_POLICY_VALUE, Z.F_OPTION_TERM_MU, Z.F_OPTION_TERM_STD, Z.F_OPTION_TERM_ACTION,
              Z.F_OPTION_TERM_PROB)
    sets = [("all", idx >= 0), ("none", idx < 0), ("env 0", idx == 0), ("env N - 1", idx == n - 1),
            ("every other", idx % 2 == 0), ("all again", idx >= 0), ("env N - 1 after all", idx == n - 1)]
    if n == 1:
        sets = sets[:2]                                            # the others coincide with "all"
    envs = []
    try:
        for compact in (0, 1):
            monkeypatch.setenv("ZENV_OPTION_COMPACT", str(compact))        # read by zenv_option_load
            env = _env(Z, _cfg(Z, TSP, 25), n, 601, goals=False)
            envs.append(env)
            hi, lo = option_ref.random_state_dicts(env.zone_feat, S, h=33, seed=n, term_bias=-100.0)
            env.load_options(Z.option_tensors_from_state_dicts(hi, lo))
            env.policy(Z.POLICY_OPTION_MEAN)                       # every env picks
            assert (env.get(Z.F_SKILL) >= 0).all()
            env.step(None, auto_reset=True)
        rs = np.random.RandomState(n)
        for name, mask in sets:
            skills = rs.randint(0, S, n).astype(np.int32)
            outs = []
            for env in envs:
                env.set_skills(skills)
                env.policy(Z.POLICY_OPTION_MEAN)                   # nobody picks
                env.step(None, auto_reset=True)
                if mask.any():
                    env.reset(mask.astype(np.uint8))
                skill0, age0 = env.get(Z.F_SKILL), env.get(Z.F_SKILL_AGE)
                # the planted set is the picking set: !finished && (skill < 0 || ended)
                assert np.array_equal(skill0 < 0, mask), name
                assert not env.get(Z.F_OPTION_ENDED).any() and not env.get(Z.F_DONE).any(), name
                assert np.array_equal(skill0[~mask], skills[~mask]) and np.array_equal(age0, np.where(mask, 0, 1)), name
                fl, fv = env.option_forward()[:2]
                held = env.get(Z.F_SKILL_LOGITS), env.get(Z.F_SKILL_VALUE)
                env.policy(Z.POLICY_OPTION_MEAN)
                logits, value = env.get(Z.F_SKILL_LOGITS), env.get(Z.F_SKILL_VALUE)
                _same(logits[mask], fl[mask], name + ": the pickers' logits")
                _same(value[mask], fv[mask], name + ": the pickers' value")
                _same(logits[~mask], held[0][~mask], name + ": the others' logits")
                _same(value[~mask], held[1][~mask], name + ": the others' value")
                skill1 = env.get(Z.F_SKILL)
                assert np.array_equal(skill1[mask], np.argmax(fl[mask], axis=1)), name      # the lowest index on ties
                assert np.array_equal(skill1[~mask], skill0[~mask]), name
                assert np.array_equal(env.get(Z.F_SKILL_AGE), np.where(mask, 1, age0 + 1)), name
                assert not env.get(Z.F_OPTION_ENDED).any(), name
                outs.append([env.get(f) for f in fields])
                env.step(None, auto_reset=True)
            for f, a, b in zip(fields, *outs):
                _same(a, b, "%s: field %d of the two handles" % (name, f))
    finally:
        for env in envs:
            env.close()


# ---------------------------------------------------------------------------------------------------- exact draws
@pytest.mark.parametrize("S", [1, 32])
def test_option_draws_are_exact_at_the_head_width_edges(zenv_mod, S):
    """tests/test_gpu_options.py::check_draws with one logit row and with kMaxSkills of them, 67 envs, two steps."""
    _note("option a_2 ulps (S = %d)" % S, check_draws(zenv_mod, 0xDEADBEEF12345, n=67, S=S, steps=2))


@pytest.mark.parametrize("n", [1, 3])
def test_xy_sample_draws_exactly_in_a_short_workgroup(zenv_mod, n):
    """One XY_SAMPLE step on fewer envs than a workgroup holds: the goal is goal_mu + goal_std * n at the host
    Box-Muller pair of the goal stream, the action mu + std * eps at that of the action stream."""
    Z = zenv_mod
    seed, index0 = 0xDEADBEEF12345, 2 ** 40 + 5
    env = _env(Z, _cfg(Z, TSP, 9), n, 701, goals=False)
    try:
        hi, lo = xy_ref.random_state_dicts(env.zone_feat, h=65, seed=6)
        env.load_xy(Z.xy_tensors_from_state_dicts(hi, lo))
        step = env.step_count
        assert step > 0
        env.policy(Z.POLICY_XY_SAMPLE, policy_seed=seed, env_index0=index0)
        goal, gmu, gstd = env.get(Z.F_XY_GOAL), env.get(Z.F_XY_GOAL_MU), env.get(Z.F_XY_GOAL_STD)
        u = _ulps(goal, gmu, gstd, xy_ref.goal_noise(n, seed, index0, step))
        _note("xy goal ulps", u.max())
        assert u.max() <= ACT_ULPS, float(u.max())
        assert (goal != gmu).any(axis=1).all() and np.array_equal(env.get(Z.F_XY_GOAL_AGE), np.ones(n, np.int32))
        u = _ulps(env.get(Z.F_ACTIONS), env.get(Z.F_POLICY_MU), env.get(Z.F_POLICY_STD),
                  philox_ref.action_noise(n, seed, index0, step))
        _note("xy action ulps", u.max())
        assert u.max() <= ACT_ULPS, float(u.max())
    finally:
        env.close()
