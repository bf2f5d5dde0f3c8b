"""zenv_collect_option: collect_experiences of the variable-length Options agent (options/src/torch_ac/algos/
_hier_policy_opt.py:10-205) on the device.  Checked against the same frames driven by zenv_policy(OPTION_SAMPLE) +
zenv_step on a second handle, where zenv_set_skills puts back the skill of every env whose episode ended while its option
went on (bit for bit), the torch restatement of both networks (tests/option_ref.py) and the numpy restatement of the
bookkeeping (tests/option_collect_ref.py): the semi-Markov rows, both GAE recursions, the T-1 frame cut, the env-major
flattening, the transition carried from call to call and the skill that survives an auto-reset."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import option_ref
from tests.option_collect_ref import GAMMA, LAM, expected_age, expected_hi, replay

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(Z, env_id, n, seed=11, **over):
    """A plain task handle: a registry id, or ("tsp", zones) for a PointTSP layout of that many zones."""
    if isinstance(env_id, tuple):
        cfg = Z.default_config(Z.TASK_TSP, env_id[1], zones_keepout=0.45, **over)
    else:
        cfg = Z.config_for_id(env_id, **over)
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(seed, n)
    env.schedule_sequential()
    env.reset()
    return env


def _pair(Z, env_id, n, S, h, wseed, num_steps=60, **kw):
    """Two handles of the same envs with the same option weights: the collector's and the replay's."""
    a, b = _env(Z, env_id, n, num_steps=num_steps), _env(Z, env_id, n, num_steps=num_steps)
    hi_sd, lo_sd = option_ref.random_state_dicts(a.zone_feat, S, h=h, seed=wseed, **kw)
    for e in (a, b):
        e.load_options(Z.option_tensors_from_state_dicts(hi_sd, lo_sd))
    return a, b, hi_sd, lo_sd


def _raw(Z, env, field, shape, dtype):
    """A whole time-major buffer (all T frames, the last included)."""
    a = np.empty(shape, dtype)
    assert a.nbytes == env.field_bytes(field), (field, a.nbytes, env.field_bytes(field))
    Z._native.check(Z._native.lib().zenv_get(env._h, field, a.ctypes.data, 0))
    return a


def _collect(Z, env, T, seed):
    lo, hi, rate = env.collect_options(T, policy_seed=seed, discount=GAMMA, gae_lambda=LAM)
    raw = {name: _raw(Z, env, f, s, dt) for name, (f, s, dt) in
           Z.option_experience_layout(env.num_envs, env.num_zones, env.zone_feat, T, 0)[0].items()}
    # what the fields hold is this call's: M rows, no action mask (every skill is always available)
    assert env.field_bytes(Z.F_HI_ACTION_MASK) == 0 and env.field_bytes(Z.F_HI_OBS) == 32 * len(hi["action"])
    return dict(lo=lo, hi=hi, rate=rate, raw=raw, v_final=env.get(Z.F_SKILL_VALUE), T=T)


def _normal_log_prob(a, mu, std):
    a, mu, std = (np.asarray(x, np.float64) for x in (a, mu, std))
    return -0.5 * ((a - mu) / std) ** 2 - np.log(std) - 0.5 * np.log(2 * np.pi)


def _check_call(Z, env, rec, t0, out, rows_per_env, prev_done, term_log_prob=True):
    """One call that began at frame t0 of the record `rec` against it: the low level bit for bit, the high-level rows
    against `rows_per_env` (expected_hi's rows of this call).  Returns the done flags of its last frame."""
    n, T = env.num_envs, out["T"]
    lo, hi, raw = out["lo"], out["hi"], out["raw"]
    fr = slice(t0, t0 + T)
    # ---- low level, every frame of the call (time-major raw buffers), bit for bit
    assert np.array_equal(raw["obs"], rec["obs"][fr]) and np.array_equal(raw["zone_obs"], rec["zone_obs"][fr])
    assert np.array_equal(raw["skill"], rec["skill"][fr])
    assert np.array_equal(raw["action"], rec["action"][fr])
    assert np.array_equal(raw["term_action"], rec["term_action"][fr])
    assert np.array_equal(raw["ended"].astype(bool), rec["ended"][fr])
    assert np.array_equal(raw["value"], rec["value"][fr])
    assert np.array_equal(raw["reward"], rec["reward"][fr]) and np.array_equal(raw["env_reward"], rec["reward"][fr])
    done_prev = np.concatenate([prev_done[None], rec["done"][fr][:-1]])
    assert np.array_equal(raw["mask"], 1.0 - done_prev.astype(np.float32))
    assert out["rate"] == pytest.approx(rec["ended"][fr].mean(), abs=1e-7)
    lp = _normal_log_prob(raw["action"], rec["mu"][fr], rec["std"][fr])
    print("log_prob", float(np.abs(lp - raw["log_prob"]).max()))
    assert np.abs(lp - raw["log_prob"]).max() < 2e-3
    if term_log_prob:
        lp2 = _normal_log_prob(raw["term_action"], rec["term_mu"][fr], rec["term_std"][fr])
        print("term log_prob", float(np.abs(lp2 - raw["term_log_prob"]).max()))
        assert np.abs(lp2 - raw["term_log_prob"]).max() < 2e-3
    # the T-1 frame cut, the three components and the GAE without bootstrap
    assert lo["obs"].shape == (n, T - 1, 8) and lo["action"].shape == (n, T - 1, 3) and lo["log_prob"].shape == (n, T - 1, 3)
    assert np.array_equal(lo["action"][..., :2], raw["action"][:T - 1].swapaxes(0, 1))
    assert np.array_equal(lo["action"][..., 2], raw["term_action"][:T - 1].T)
    assert np.array_equal(lo["log_prob"][..., 2], raw["term_log_prob"][:T - 1].T)
    assert lo["ended"].dtype == bool and np.array_equal(lo["ended"], rec["ended"][fr][:T - 1].T)
    assert np.array_equal(lo["skill"], rec["skill"][fr][:T - 1].T)
    adv = np.zeros((T, n), np.float32)
    for i in reversed(range(T - 1)):
        nm = raw["mask"][i + 1]
        delta = raw["reward"][i] + np.float32(GAMMA) * raw["value"][i + 1] * nm - raw["value"][i]
        adv[i] = delta + np.float32(GAMMA) * np.float32(LAM) * adv[i + 1] * nm
    assert np.abs(lo["advantage"] - adv[:T - 1].T).max() < 1e-5
    assert np.abs(lo["returnn"] - (lo["value"] + lo["advantage"])).max() < 1e-5
    assert not raw["advantage"][T - 1].any() and not raw["returnn"][T - 1].any()
    # ---- high level: env-major rows
    counts = [len(r) for r in rows_per_env]
    assert np.array_equal(hi["count"], counts) and len(hi["action"]) == sum(counts)
    rows = [r for per_env in rows_per_env for r in per_env]
    if rows:
        tp = np.array([r["t_pick"] for r in rows])
        jj = np.repeat(np.arange(n), counts)
        assert np.array_equal(hi["action"], [r["skill"] for r in rows])
        assert np.array_equal(hi["obs"], rec["obs"][tp, jj]) and np.array_equal(hi["zone_obs"], rec["zone_obs"][tp, jj])
        assert np.array_equal(hi["value"], [r["value"] for r in rows])
        assert np.array_equal(hi["reward"], np.array([r["reward"] for r in rows], np.float32))
        assert np.array_equal(hi["mask"], [r["mask"] for r in rows])
        want_lp = rec["logits"][tp, jj, hi["action"]]               # ZENV_F_SKILL_LOGITS is the log-softmax
        assert np.abs(hi["log_prob"] - want_lp).max() < 1e-5
        assert np.abs(hi["advantage"] - [r["adv"] for r in rows]).max() < 1e-5
        assert np.abs(hi["returnn"] - (hi["value"] + hi["advantage"])).max() < 1e-5
    return rec["done"][fr][-1]


def _run_and_check(Z, a, b, hi_sd, lengths, seed, term_log_prob=True):
    """Consecutive calls of `lengths` frames on `a` against the frames replayed on `b`.  Returns (outs, rec, exp, seen)."""
    n = a.num_envs
    rec = replay(Z, b, sum(lengths), seed)
    outs = [_collect(Z, a, T, seed) for T in lengths]
    exp, seen = expected_hi(rec, list(lengths), len(lengths), [o["v_final"] for o in outs])
    prev_done = np.zeros(n, bool)
    t0 = 0
    for c, out in enumerate(outs):
        prev_done = _check_call(Z, a, rec, t0, out, exp[c], prev_done, term_log_prob)
        t0 += out["T"]
    # the final observation and the final skill state are the replay's; the age counts on across the auto-resets
    o_a, zo_a = a.observations()
    o_b, zo_b = b.observations()
    assert np.array_equal(o_a, o_b) and np.array_equal(zo_a, zo_b)
    skill = a.get(Z.F_SKILL)
    assert np.array_equal(skill, b.get(Z.F_SKILL)) and np.array_equal(a.get(Z.F_OPTION_ENDED), b.get(Z.F_OPTION_ENDED))
    assert np.array_equal(a.get(Z.F_SKILL_AGE), np.where(skill >= 0, expected_age(rec), 0))
    assert a.step_count == b.step_count == sum(lengths)
    # the last bootstrap value is the high critic on the final observation
    _, rv = option_ref.high(hi_sd, o_a, zo_a)
    assert np.all(np.abs(outs[-1]["v_final"] - rv) <= 1e-5 * np.maximum(1.0, np.abs(rv)))
    return outs, rec, exp, seen


@pytest.mark.parametrize("env_id", ["PointTSP-v0", "PointTTSP-v0", "ColourMatch-v0"])
def test_collect_option_is_the_replayed_frames(zenv_mod, env_id):
    """Two consecutive calls of 45 frames against 90 replayed frames, 203 envs with episodes of 60 steps: every
    low-level record bit for bit, the rows' skill, obs, value, reward and mask exactly, the log_probs and both GAEs
    within the tolerances of the other collectors' tests.  A fresh network ends an option on about a tenth of the steps,
    so the 90 frames hold every case the bookkeeping has; the test counts them."""
    Z = zenv_mod
    a, b, hi_sd, _ = _pair(Z, env_id, 203, S=5, h=128, wseed=3)
    outs, rec, exp, seen = _run_and_check(Z, a, b, hi_sd, [45, 45], seed=77)
    print(env_id, "terminations", int(rec["ended"].sum()), "dones", int(rec["done"].sum()),
          "both", int((rec["ended"] & rec["done"]).sum()), seen)
    # the first call's bootstrap value too (the replay's frame 45 is its obs_T)
    _, rv = option_ref.high(hi_sd, rec["obs"][45], rec["zone_obs"][45])
    assert np.all(np.abs(outs[0]["v_final"] - rv) <= 1e-5 * np.maximum(1.0, np.abs(rv)))
    assert seen["span"] > 0, seen            # a transition spanning the call boundary
    assert seen["mask0"] > 0, seen           # a close with hi_mask 0
    assert seen["mask1"] > 0, seen           # a close with hi_mask 1
    assert seen["bootstrap"] > 0, seen       # a row whose V_next is V_hi(obs_T) with mask 1
    assert seen["survived"] > 0, seen        # a skill that survived an auto-reset with its transition open
    assert seen["no_rows"] > 0, seen         # an env with no rows in a call
    a.close()
    b.close()


def _quiet_seed(n, T, step0=0):
    """A policy seed whose termination uniforms (tests/option_ref.term_uniform) end no option of term_bias = -3
    (probability 0.0013) in frames 0 .. T-1 and at least one in frames T .. 2T-1, with no uniform near the threshold."""
    for seed in range(1, 400):
        u = np.stack([option_ref.term_uniform(n, seed, 0, step0 + t) for t in range(2 * T)])
        if (u[:T] > 0.002).all() and (u[T:] < 0.001).any() and not ((u[T:] >= 0.001) & (u[T:] <= 0.002)).any():
            return seed
    raise AssertionError("no seed found")


def test_options_that_never_end_give_no_rows_and_stay_open(zenv_mod):
    """term_bias = -3: an option ends with probability 0.0013 per frame.  The first call closes nothing -- M = 0, empty
    outputs -- and leaves every env's transition open; the second call closes some of them: rows whose pick, obs and
    value are the first call's frame 0 (the carry slot) and whose reward sums both calls across the auto-resets."""
    Z = zenv_mod
    n, T = 67, 12
    a, b, hi_sd, _ = _pair(Z, "PointTSP-v0", n, S=5, h=64, wseed=5, num_steps=9, term_bias=-3.0)
    seed = _quiet_seed(n, T, a.step_count)
    outs, rec, exp, seen = _run_and_check(Z, a, b, hi_sd, [T, T], seed, term_log_prob=False)
    hi0, hi1 = outs[0]["hi"], outs[1]["hi"]
    assert not rec["ended"][:T].any() and outs[0]["rate"] == 0.0
    assert not hi0["count"].any() and all(len(v) == 0 for k, v in hi0.items() if k != "count")
    assert hi0["zone_obs"].shape == (0, a.num_zones, a.zone_feat)
    assert len(hi1["action"]) == hi1["count"].sum() > 0
    first = [per_env[0] for per_env in exp[1] if per_env]             # every env's first row closes its carried transition
    assert all(r["t_pick"] == 0 for r in first) and seen["span"] == len(first) and seen["survived"] > 0
    a.close()
    b.close()


def test_frequent_endings_give_one_frame_transitions(zenv_mod):
    """term_bias = +3: an option ends with probability 0.65 per frame.  Many transitions last one frame, the counts
    match and the rows stay env-major."""
    Z = zenv_mod
    n = 131
    a, b, hi_sd, _ = _pair(Z, "ColourMatch-v0", n, S=5, h=64, wseed=6, num_steps=20, term_bias=3.0)
    outs, rec, exp, seen = _run_and_check(Z, a, b, hi_sd, [9, 6, 11], seed=8, term_log_prob=False)
    rows = [r for call in exp for per_env in call for r in per_env]
    assert sum(r["t_pick"] == r["t_close"] for r in rows) > 5 * n
    assert 0.55 < rec["ended"].mean() < 0.75
    for out in outs:
        assert out["hi"]["count"].sum() == len(out["hi"]["action"]) > 2 * n
    a.close()
    b.close()


def test_both_ways_of_finding_the_picking_envs_agree(zenv_mod, monkeypatch):
    """ZENV_OPTION_COMPACT=0 and =1 at load: identical buffers."""
    Z = zenv_mod
    n, T, S = 203, 14, 5
    outs = []
    for compact in ("0", "1"):
        monkeypatch.setenv("ZENV_OPTION_COMPACT", compact)
        env = _env(Z, "PointTSP-v0", n, num_steps=10)
        hi_sd, lo_sd = option_ref.random_state_dicts(env.zone_feat, S, h=64, seed=9)
        env.load_options(Z.option_tensors_from_state_dicts(hi_sd, lo_sd))
        outs.append([_collect(Z, env, T, 21) for _ in range(2)])
        env.close()
    for x, y in zip(*outs):
        assert len(x["hi"]["action"]) > 0
        for part in ("raw", "hi"):
            for k in x[part]:
                assert np.array_equal(x[part][k], y[part][k]), (part, k)
        assert np.array_equal(x["v_final"], y["v_final"])


@pytest.mark.parametrize("env_id,n,lengths,S,h", [
    ("PointTSP-v0", 1, [2, 2, 3, 2], 5, 64),             # one env, the shortest call
    ("PointTTSP-v0", 63, [2, 5], 1, 32),                 # S = 1: the only skill, every pick
    ("ColourMatch-v0", 65, [6, 4], 32, 48),              # S = 32, one env past a wave
    ("PointTSP-v0", 65, [5, 5], 5, 191),                 # the widest hidden layer
    (("tsp", 1), 63, [7, 6], 3, 32),                     # Z = 1
])
def test_edge_shapes(zenv_mod, env_id, n, lengths, S, h):
    Z = zenv_mod
    a, b, hi_sd, _ = _pair(Z, env_id, n, S=S, h=h, wseed=S + h, num_steps=4)
    _run_and_check(Z, a, b, hi_sd, lengths, seed=n + S)
    a.close()
    b.close()


@pytest.mark.parametrize("env_id,h", [("PointTSP-v0", 128), ("ColourMatch-v0", 64)])
def test_recorded_networks_match_torch(zenv_mod, env_id, h):
    """The recorded low-level value and three-component log_prob, and the rows' value and log_prob(skill), against
    tests/option_ref.py on the recorded observations and skills."""
    Z = zenv_mod
    n, T, S = 203, 16, 5
    env = _env(Z, env_id, n, num_steps=12)
    hi_sd, lo_sd = option_ref.random_state_dicts(env.zone_feat, S, h=h, seed=h)
    env.load_options(Z.option_tensors_from_state_dicts(hi_sd, lo_sd))
    lo, hi, _ = env.collect_options(T, policy_seed=9)
    f = lambda x, *s: np.ascontiguousarray(x).reshape(n * (T - 1), *s)
    assert (lo["skill"] >= 0).all()
    mu, std, val = option_ref.low(lo_sd, f(lo["obs"], 8), f(lo["zone_obs"], env.num_zones, env.zone_feat),
                                  f(lo["skill"]), S)
    tol = lambda ref: 1e-5 * np.maximum(1.0, np.abs(ref))
    assert np.all(np.abs(f(lo["value"]) - val) <= tol(val))
    lp = _normal_log_prob(f(lo["action"], 3), mu, std)
    print("log_prob", float(np.abs(lp - f(lo["log_prob"], 3)).max()))
    assert np.abs(lp - f(lo["log_prob"], 3)).max() < 2e-3
    assert len(hi["action"]) > n // 2
    logits, hv = option_ref.high(hi_sd, hi["obs"], hi["zone_obs"])
    assert np.all(np.abs(hi["value"] - hv) <= tol(hv))
    want = logits[np.arange(len(hv)), hi["action"]]
    assert np.all(np.abs(hi["log_prob"] - want) <= tol(want))
    logits_T, hv_T = option_ref.high(hi_sd, *env.observations())
    assert np.all(np.abs(env.get(Z.F_SKILL_VALUE) - hv_T) <= tol(hv_T))
    assert np.all(np.abs(env.get(Z.F_SKILL_LOGITS) - logits_T) <= tol(logits_T))
    env.close()


@pytest.mark.parametrize("how", ["reset", "partial reset", "load"])
def test_open_transitions_are_dropped(zenv_mod, how):
    """zenv_reset between two calls drops the open transition of the envs it resets (a partial mask: only theirs) and
    zeroes their hi_reward; zenv_option_load drops every one.  No row of the second call refers to a dropped transition:
    its rows are those of the same frames replayed with the same reset / load in between."""
    Z = zenv_mod
    n, T1, T2, seed = 150, 7, 9, 13
    a, b, hi_sd, lo_sd = _pair(Z, "PointTSP-v0", n, S=5, h=64, wseed=4, num_steps=30)
    mask = np.ones(n, bool) if how != "partial reset" else (np.arange(n) % 3 != 0)

    def between(env):
        if how == "load":
            env.load_options(Z.option_tensors_from_state_dicts(hi_sd, lo_sd))
        else:
            env.reset(None if how == "reset" else mask.astype(np.uint8))

    out1 = _collect(Z, a, T1, seed)
    between(a)
    out2 = _collect(Z, a, T2, seed)
    rec1 = replay(Z, b, T1, seed)
    between(b)
    rec2 = replay(Z, b, T2, seed)
    rec = {k: np.concatenate([rec1[k], rec2[k]]) for k in rec1}
    # what the drop throws away: the transitions open after the first call (every env picked at frame 0)
    last_pick = [np.nonzero(rec1["pick"][:, j])[0][-1] for j in range(n)]
    was_open = np.array([not rec1["ended"][last_pick[j]:, j].any() for j in range(n)])
    assert (was_open & mask).sum() > n // 4
    assert rec2["pick"][0][mask].all()                     # the envs that lost their skill pick again at once
    if how == "partial reset":
        assert not rec2["pick"][0][~mask & was_open].any() and (~mask & was_open).any()
    closed = dict(rec, ended=rec["ended"].copy())
    closed["ended"][T1 - 1, mask] = True                   # for the restatement: nothing stays open in these envs
    exp, seen = expected_hi(closed, [T1, T2], 2, [out1["v_final"], out2["v_final"]])
    exp1, _ = expected_hi(rec1, T1, 1, [out1["v_final"]])
    done1 = _check_call(Z, a, rec, 0, out1, exp1[0], np.zeros(n, bool))
    _check_call(Z, a, rec, T1, out2, exp[1], done1)        # self.mask belongs to the algorithm: a reset leaves it
    rows2 = [r for per_env in exp[1] for r in per_env]
    assert rows2 and all(r["t_pick"] >= T1 for j in np.nonzero(mask)[0] for r in exp[1][j])
    if how == "partial reset":
        assert any(r["t_pick"] < T1 for j in np.nonzero(~mask)[0] for r in exp[1][j])
    a.close()
    b.close()


def test_refusals(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    raw = lambda env, T, d=0.99, lam=0.95: nat.lib().zenv_collect_option(env._h, T, 1, 0, d, lam, C.byref(C.c_int64()))

    def code(env, T=8, d=0.99, lam=0.95):
        rc = raw(env, T, d, lam)
        assert rc < 0
        return rc
    from tests import skill_ref
    env = _env(Z, "PointTSP-v0", 16)
    assert code(env) == Z.E_STATE                                   # no weights at all
    env.load_skills(Z.skill_tensors_from_state_dicts(*skill_ref.random_state_dicts(env.zone_feat, 4, h=32)), skill_len=4)
    assert code(env) == Z.E_STATE                                   # skill weights are not option weights
    t = Z.option_tensors_from_state_dicts(*option_ref.random_state_dicts(env.zone_feat, 4, h=32))
    env.load_options({k: v for k, v in t.items() if "critic" not in k})
    assert code(env) == Z.E_STATE                                   # no critic
    for drop in ("hi", "lo"):                                       # one critic missing
        env.load_options({k: v for k, v in t.items() if not k.startswith(drop + "_critic")})
        assert code(env) == Z.E_STATE
    env.load_options(t)
    rc = nat.lib().zenv_collect_skill(env._h, 8, 1, 0, 0.99, 0.95, 0.0, None, 1)
    assert rc == Z.E_STATE                                          # the skill collector on an option handle
    assert code(env, 1) == Z.E_ARG and code(env, 0) == Z.E_ARG and code(env, -3) == Z.E_ARG     # T < 2
    assert code(env, 2 ** 27) == Z.E_ARG                            # T x 16 envs = 2^31
    for d, lam in ((float("nan"), 0.95), (0.99, float("nan")), (float("inf"), 0.95), (0.99, -float("inf")),
                   (1.5, 0.95), (0.99, -0.1), (-0.01, 0.5), (0.5, 1.01)):
        assert code(env, 8, d, lam) == Z.E_ARG, (d, lam)
    with pytest.raises(ValueError):
        env.collect_options(1)
    env.host_io(True)
    assert code(env) == Z.E_STATE                                   # host I/O
    env.host_io(False)
    lo_x, hi_x, rate = env.collect_options(4)
    assert lo_x["obs"].shape == (16, 3, 8) and 0.0 <= rate <= 1.0
    assert nat.lib().zenv_collect_option(env._h, 4, 1, 0, 0.99, 0.95, None) == 0      # n_hi may be null
    env.close()
    ring = Z.ZoneVecEnv(Z.config_for_id("PointTSP-v0", num_steps=5), 8)
    ring.build_bank(1, 8 * 4)
    ring.schedule_ring(np.arange(8, dtype=np.int32) * 4, 4)
    ring.reset()
    ring.load_options(t)
    assert code(ring, 5) == Z.E_STATE                               # beyond the ring's depth
    assert raw(ring, 4) == 0
    ring.close()
    goal = _env(Z, "PointTSP-v0", 8)
    goal.enable_goals()
    goal.reset()
    assert code(goal) == Z.E_STATE                                  # goal-conditioned
    goal.close()
    order = Z.ZoneVecEnv(Z.config_for_id("PointTSP-v0"), 8)
    order.enable_order()
    order.build_bank(1, 8)
    order.reset()
    assert code(order) == Z.E_STATE                                 # solver-ordered
    order.close()


def test_torch_tensors_alias_and_the_example_trains(zenv_mod):
    """TorchZoneEnv.collect_options: CUDA tensors aliasing the device buffers, equal to the numpy path; two iterations
    of examples/options_ppo_torch.py's updates run and change both networks' outputs."""
    import importlib.util
    import torch
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    Z = zenv_mod
    n, T, S = 64, 16, 5
    envs = [_env(Z, "PointTSP-v0", n, num_steps=30) for _ in range(2)]
    hi_sd, lo_sd = option_ref.random_state_dicts(envs[0].zone_feat, S, h=64, seed=4)
    envs[0].load_options(Z.option_tensors_from_state_dicts(hi_sd, lo_sd))
    lo_np, hi_np, rate_np = envs[0].collect_options(T, policy_seed=2)
    tz = TorchZoneEnv(envs[1])
    tz.load_options(hi_sd, lo_sd)
    lo_t, hi_t, rate_t = tz.collect_options(T, policy_seed=2)
    torch.cuda.synchronize()
    assert lo_t["obs"].is_cuda and lo_t["obs"].shape == (n, T - 1, 8)
    assert lo_t["obs"].data_ptr() == envs[1].device_ptr(Z._native.F_EXP_OBS)
    assert lo_t["action"].shape == (n, T - 1, 2) and lo_t["action"].data_ptr() == envs[1].device_ptr(Z._native.F_EXP_ACTION)
    assert lo_t["term_action"].shape == (n, T - 1)
    assert lo_t["term_action"].data_ptr() == envs[1].device_ptr(Z.F_LO_TERM_ACTION)
    assert lo_t["term_log_prob"].data_ptr() == envs[1].device_ptr(Z.F_LO_TERM_LOG_PROB)
    assert lo_t["ended"].dtype == torch.bool and lo_t["ended"].data_ptr() == envs[1].device_ptr(Z.F_LO_OPTION_ENDED)
    assert lo_t["skill"].data_ptr() == envs[1].device_ptr(Z.F_LO_SKILL)
    assert len(hi_np["action"]) > 0 and hi_t["zone_obs"].data_ptr() == envs[1].device_ptr(Z.F_HI_ZONE_OBS)
    assert hi_t["count"].data_ptr() == envs[1].device_ptr(Z.F_HI_COUNT)
    cat = lambda a, b: torch.cat([a, b.unsqueeze(-1)], dim=-1).cpu().numpy()
    assert np.array_equal(cat(lo_t["action"], lo_t["term_action"]), lo_np["action"])
    assert np.array_equal(cat(lo_t["log_prob"], lo_t["term_log_prob"]), lo_np["log_prob"])
    for k in lo_np:
        if k not in ("action", "log_prob"):
            assert np.array_equal(lo_t[k].cpu().numpy(), lo_np[k]), k
    for k in hi_np:
        assert np.array_equal(hi_t[k].cpu().numpy(), hi_np[k]), k
    assert float(rate_t) == pytest.approx(rate_np, abs=1e-7)
    envs[0].close()
    spec = importlib.util.spec_from_file_location("options_ppo_torch", os.path.join(ROOT, "examples", "options_ppo_torch.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    dev = tz.device
    torch.manual_seed(0)
    algo = ex.OptionsPPO(tz, n_skills=S, h=64, frames_per_proc=T, epochs=2, batch_size=256, hi_epochs=2, hi_batch_size=64)
    probe = (tz.obs.clone(), tz.zone_obs.clone(), torch.zeros(n, dtype=torch.long, device=dev))
    with torch.no_grad():
        before = (algo.hi_net(probe[0], probe[1])[0].logits.clone(), algo.lo_net(*probe)[0].mean.clone())
    for _ in range(2):
        logs = algo.iteration()
        assert np.isfinite(logs["lo_policy_loss"]) and np.isfinite(logs["hi_policy_loss"])
        assert 0.0 <= logs["termination_rate"] <= 1.0
    with torch.no_grad():
        after = (algo.hi_net(probe[0], probe[1])[0].logits, algo.lo_net(*probe)[0].mean)
    assert after[1].shape == (n, 3)
    assert not torch.allclose(before[0], after[0]) and not torch.allclose(before[1], after[1])
    envs[1].close()
