"""zenv_collect_xy: collect_experiences of the xy-goals agent (xy-goals/src/torch_ac/algos/_hier_policy_opt.py:10-192) on
the device.  Checked against the same frames driven by zenv_policy(XY_SAMPLE) + zenv_step on a second handle (bit for
bit), numpy float32 for the distance and the distance reward (bit for bit), the torch restatements of the two networks
(tests/xy_ref.py), the host Philox for the bootstrap goal (tests/philox_ref.py) and a numpy restatement of the
bookkeeping (tests/xy_collect_ref.py: both GAEs, the window sums, next_mask, num_frames, the mask carried from call to
call)."""
import numpy as np
import pytest

from tests import xy_ref
from tests.xy_collect_ref import GAMMA, LAM, bookkeeping, boot_noise, goal_dist, hi_log_prob, lo_reward, replay

pytestmark = pytest.mark.gpu

L, T, N = 8, 24, 203
ACT_ULPS = 4.0          # the bound of the goal-draw test (tests/test_gpu_xy_goals.py::test_sample_draws_exactly)
CFG = {"PointTSP-25": lambda Z, **o: Z.default_config(Z.TASK_TSP, 25, zones_keepout=0.40, **o),
       "TimedTSP-25": lambda Z, **o: Z.default_config(Z.TASK_TIMED_TSP, 25, zones_keepout=0.40, **o),
       "ColourMatch-v0": lambda Z, **o: Z.config_for_id("ColourMatch-v0", **o)}


def _env(Z, name, n, seed=11, num_steps=12, pre=4):
    """Episodes of num_steps = 12 (L = 8); after `pre` = 4 steps every other env is reset.  Episodes start at window
    starts after that, so the reset half ends in the middle of a window (frame 11, idle to frame 15) and the other half
    ends on a window's last frame (frame 7, mask 0 at frame 8), ends mid-window at frame 19 and idles through the end
    of the first call (mask 0 at the second call's first frame)."""
    env = Z.ZoneVecEnv(CFG[name](Z, num_steps=num_steps), n)
    env.build_bank(seed, n)
    env.schedule_sequential()
    env.reset()
    for _ in range(pre):
        env.step(np.zeros((n, 2), np.float32), auto_reset=True)
    if pre:
        env.reset((np.arange(n) % 2 == 0).astype(np.uint8))
    return env


def _load(Z, env, h=64, seed=3, skill_len=L, critics=True):
    hi, lo = xy_ref.random_state_dicts(env.zone_feat, h, seed, critics)
    env.load_xy(Z.xy_tensors_from_state_dicts(hi, lo), skill_len=skill_len)
    return hi, lo


def _raw(Z, env, field, shape, dtype):
    a = np.empty(shape, dtype)
    assert a.nbytes == env.field_bytes(field), (field, a.nbytes, env.field_bytes(field))
    Z._native.check(Z._native.lib().zenv_get(env._h, field, a.ctypes.data, 0))
    return a


def _collect(Z, env, seed, frames=T, skill_len=L):
    """One collection: (lo, hi, num_frames), the time-major raw low-level buffers, and the bootstrap's outputs."""
    out = env.collect_xy(frames, policy_seed=seed, discount=GAMMA, gae_lambda=LAM)
    lo_l, _ = Z.xy_experience_layout(env.num_envs, env.num_zones, env.zone_feat, frames, skill_len)
    raw = {name: _raw(Z, env, f, s, dt) for name, (f, s, dt) in lo_l.items()}
    boot = (env.get(Z.F_XY_BOOTSTRAP_GOAL), env.get(Z.F_XY_VALUE), env.get(Z.F_POLICY_VALUE))
    return out, raw, boot


def _tol(ref):
    return 1e-5 * np.maximum(1.0, np.abs(ref))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ulps(got, mu, std, eps):
    """The distance of a float32 draw from mu + std * eps in float32 ulps of |mu| + std * |eps| (the measure of
    tests/test_gpu_xy_goals.py); mu / std: the device's own float32 outputs, taken to float64."""
    mu, std = mu.astype(np.float64), std.astype(np.float64)
    mag = np.abs(mu) + std * np.hypot(eps[:, :1], eps[:, 1:])
    return np.abs(got.astype(np.float64) - (mu + std * eps)) / (mag * 2.0 ** -23)


def _check_call(Z, a, out, raw, boot, rec, c, calls, prev_done, hi_sd, lo_sd, seen, frames=T, skill_len=L):
    """Call c of `calls` on handle a against frames c * frames .. of the replay `rec`.  Returns the dones of its last
    frame (the next call's carried mask)."""
    lo, hi, num_frames = out
    n, Tn, Ln = a.num_envs, frames, skill_len
    W = Tn // Ln
    fr = slice(c * Tn, (c + 1) * Tn)
    done = rec["done"][fr]
    # ---- the low level, every frame, bit for bit
    for k in ("obs", "zone_obs", "goal", "action", "value"):
        assert np.array_equal(_bits(raw[k]), _bits(rec[k][fr])), k
    assert np.array_equal(_bits(raw["env_reward"]), _bits(rec["reward"][fr]))
    done_prev = np.concatenate([prev_done[None], done[:-1]])
    assert np.array_equal(raw["mask"], 1.0 - done_prev.astype(np.float32))
    if c > 0:
        seen["carried_mask0"] += int((raw["mask"][0] == 0).sum())
    # every env picks at every window's first frame and keeps the goal through the window
    for k in range(W):
        assert (raw["goal"][k * Ln:(k + 1) * Ln] == raw["goal"][k * Ln]).all()
    # ---- idle frames (WaitWrapper's no-op): reward 0, done 1, and zero obs after them (the done step itself returns
    # the terminal obs); the low level is evaluated on them all the same (the value check below covers every frame)
    for t in range(1, Tn):
        idle = done_prev[t].astype(bool) & (t % Ln != 0)
        seen["idle"] += int(idle.sum())
        assert not raw["env_reward"][t][idle].any() and done[t][idle].all()
        if t + 1 < Tn and (t + 1) % Ln:
            assert not raw["obs"][t + 1][idle].any() and not raw["zone_obs"][t + 1][idle].any()
            seen["idle_zero_obs_value"] += int((raw["value"][t + 1][idle] != 0).sum())
    first = done.astype(bool) & ~done_prev.astype(bool)
    seen["end_last_frame"] += int(first[Ln - 1::Ln].sum())
    seen["end_mid_window"] += int(sum(first[t].sum() for t in range(Tn) if (t + 1) % Ln))
    # ---- the distance and the distance reward: numpy float32 on the recorded obs, goal and mask, bit for bit
    assert np.array_equal(_bits(raw["goal_dist"]), _bits(goal_dist(raw["obs"], raw["goal"])))
    want_reward = lo_reward(raw["goal_dist"], raw["mask"], Ln)
    assert np.array_equal(_bits(raw["reward"]), _bits(want_reward))
    assert not raw["reward"][Ln - 1::Ln].any()
    # ---- the low network against torch: value and log_prob on every frame
    flat = lambda x, *s: np.ascontiguousarray(x).reshape(Tn * n, *s)
    mu, std, val = xy_ref.low(lo_sd, flat(raw["obs"], 8), flat(raw["zone_obs"], a.num_zones, a.zone_feat),
                              flat(raw["goal"], 2))
    err = np.abs(flat(raw["value"]) - val)
    print(f"call {c}: low value max err {float(err.max()):.3g}")
    assert np.all(err <= _tol(val))
    lp = -0.5 * ((flat(raw["action"], 2) - mu) / std) ** 2 - np.log(std) - 0.5 * np.log(2 * np.pi)
    err = np.abs(lp - flat(lo["log_prob"].swapaxes(0, 1), 2))
    print(f"call {c}: low log_prob max err {float(err.max()):.3g}")
    assert err.max() < 2e-3
    # ---- the high rows: env-major, row env * W + k, picked at frame k L
    tp = np.tile(np.arange(W) * Ln, n) + c * Tn
    jj = np.repeat(np.arange(n), W)
    assert np.array_equal(_bits(hi["obs"]), _bits(rec["obs"][tp, jj]))
    assert np.array_equal(_bits(hi["zone_obs"]), _bits(rec["zone_obs"][tp, jj]))
    assert np.array_equal(_bits(hi["goal"]), _bits(rec["goal"][tp, jj]))
    assert np.array_equal(_bits(hi["value"]), _bits(rec["hi_value"][tp, jj]))
    want_lp = hi_log_prob(rec["goal"][tp, jj], rec["goal_mu"][tp, jj], rec["goal_std"][tp, jj])
    err = np.abs(hi["log_prob"] - want_lp)
    print(f"call {c}: hi log_prob max err / tol {float((err / _tol(want_lp)).max()):.3g}")
    assert np.all(err <= _tol(want_lp))
    _, _, rv = xy_ref.high(hi_sd, hi["obs"], hi["zone_obs"])
    assert np.all(np.abs(hi["value"] - rv) <= _tol(rv))
    # ---- the bootstrap: V_hi(obs_T) and next_lo_value = V_lo(obs_T, g')
    g_boot, v_hi, v_lo = boot
    o_T = rec["obs"][(c + 1) * Tn] if c + 1 < calls else rec["obs_T"]
    zo_T = rec["zone_obs"][(c + 1) * Tn] if c + 1 < calls else rec["zone_obs_T"]
    _, _, rv_T = xy_ref.high(hi_sd, o_T, zo_T)
    _, _, rlv_T = xy_ref.low(lo_sd, o_T, zo_T, g_boot)
    assert np.all(np.abs(v_hi - rv_T) <= _tol(rv_T))
    assert np.all(np.abs(v_lo - rlv_T) <= _tol(rlv_T))
    if c + 1 < calls:                           # g' is not the next call's first pick (a stream of its own)
        assert (g_boot != rec["goal"][(c + 1) * Tn]).any(axis=1).all()
    # ---- the bookkeeping against numpy
    cur_mask = 1.0 - done[-1].astype(np.float32)
    ref = bookkeeping(raw["goal_dist"], raw["env_reward"], raw["mask"], cur_mask, raw["value"],
                      hi["value"].reshape(n, W).T, v_lo, v_hi, Ln)
    assert np.abs(raw["advantage"] - ref["lo_adv"]).max() < 1e-5
    assert np.abs(raw["returnn"] - (raw["value"] + raw["advantage"])).max() < 1e-5
    assert np.abs(hi["reward"] - ref["hi_reward"].T.reshape(-1)).max() < 1e-5
    assert np.array_equal(hi["mask"], ref["hi_mask"].T.reshape(-1))
    assert np.abs(hi["advantage"] - ref["hi_adv"].T.reshape(-1)).max() < 1e-5
    assert np.abs(hi["returnn"] - (hi["value"] + hi["advantage"])).max() < 1e-5
    assert np.array_equal(a.get(Z.F_HI_COUNT), np.full(n, W))
    assert a.field_bytes(Z.F_HI_ACTION_MASK) == 0 and a.field_bytes(Z.F_HI_ACTION) == 0
    assert num_frames == ref["num_frames"]
    # env-major layout of lo
    assert lo["obs"].shape == (n, Tn, 8) and np.array_equal(lo["goal"], raw["goal"].swapaxes(0, 1))
    assert np.array_equal(lo["reward"], raw["reward"].T) and hi["goal"].shape == (n * W, 2)
    return done[-1]


def _new_seen():
    return {"idle": 0, "end_last_frame": 0, "end_mid_window": 0, "carried_mask0": 0, "idle_zero_obs_value": 0}


def _collect_vs_replay(Z, a, b, hi_sd, lo_sd, seed, calls, frames=T, skill_len=L):
    """`calls` consecutive collections on a against the replay of calls * frames frames on b."""
    outs = [_collect(Z, a, seed, frames, skill_len) for _ in range(calls)]
    rec = replay(Z, b, calls * frames, skill_len, seed)
    o_end, zo_end = a.observations()
    assert np.array_equal(o_end, rec["obs_T"]) and np.array_equal(zo_end, rec["zone_obs_T"])
    # the goal state after the call: the last window's goal, age L (reset envs show no goal)
    age_a = a.get(Z.F_XY_GOAL_AGE)
    assert np.array_equal(age_a, b.get(Z.F_XY_GOAL_AGE)) and (age_a[age_a >= 0] == skill_len).all()
    assert np.array_equal(_bits(a.get(Z.F_XY_GOAL)), _bits(b.get(Z.F_XY_GOAL)))
    assert a.step_count == b.step_count
    seen = _new_seen()
    prev_done = np.zeros(a.num_envs, np.uint8)
    for c, (out, raw, boot) in enumerate(outs):
        prev_done = _check_call(Z, a, out, raw, boot, rec, c, calls, prev_done, hi_sd, lo_sd, seen, frames, skill_len)
    return outs, rec, seen


@pytest.mark.parametrize("name", ["PointTSP-25", "TimedTSP-25", "ColourMatch-v0"])
def test_collect_xy_is_the_replayed_frames(zenv_mod, name):
    """Two consecutive calls against zenv_policy(XY_SAMPLE) + zenv_step (auto-reset on each window's last frame only)
    on a second handle, both freshly loaded, so that the forced pick and the policy's own pick rule coincide."""
    Z = zenv_mod
    a, b = _env(Z, name, N), _env(Z, name, N)
    hi_sd, lo_sd = _load(Z, a)
    _load(Z, b)
    outs, rec, seen = _collect_vs_replay(Z, a, b, hi_sd, lo_sd, seed=21, calls=2)
    assert outs[0][0][2] < T * N                # num_frames: some frames were idle
    print(name, seen)
    # TimedTSP's episodes end on their time budget before num_steps, none on a window's last frame there: the other
    # two tasks cover that case
    if name == "TimedTSP-25":
        seen.pop("end_last_frame")
    assert all(v > 0 for v in seen.values()), seen
    a.close()
    b.close()


def test_bootstrap(zenv_mod):
    """g' = goal_mu + goal_std * n on its own Philox stream at the step index after the last frame; it is neither the
    goal stream's draw at that index nor the next call's first pick; next_lo_value is the low critic under g'; the
    handle's goal state is the last window's."""
    Z = zenv_mod
    seed = 0xDEADBEEF12345
    a = _env(Z, "PointTSP-25", N)
    hi_sd, lo_sd = _load(Z, a)
    step0 = a.step_count
    _, raw, (g_boot, v_hi, v_lo) = _collect(Z, a, seed)
    step = a.step_count
    assert step == step0 + T
    gmu, gstd = a.get(Z.F_XY_GOAL_MU), a.get(Z.F_XY_GOAL_STD)
    o_T, zo_T = a.observations()
    rmu, rstd, rv = xy_ref.high(hi_sd, o_T, zo_T)                # the bootstrap evaluated every env on obs_T
    assert np.all(np.abs(gmu - rmu) <= _tol(rmu)) and np.all(np.abs(gstd - rstd) <= _tol(rstd))
    assert np.all(np.abs(v_hi - rv) <= _tol(rv))
    u = _ulps(g_boot, gmu, gstd, boot_noise(N, seed, 0, step))
    print(f"bootstrap goal ulps {float(u.max()):.3g}")
    assert u.max() <= ACT_ULPS
    # ... a stream of its own: the goal stream's noise at the same index is another
    z = (g_boot.astype(np.float64) - gmu) / gstd
    assert (np.abs(z - xy_ref.goal_noise(N, seed, 0, step)).max(axis=1) > 1e-2).all()
    _, _, rlv = xy_ref.low(lo_sd, o_T, zo_T, g_boot)
    assert np.all(np.abs(v_lo - rlv) <= _tol(rlv))
    # the goal state of the handle is the last window's, not the bootstrap's
    age, goal = a.get(Z.F_XY_GOAL_AGE), a.get(Z.F_XY_GOAL)
    kept = age >= 0
    assert kept.any() and (age[kept] == L).all() and (age[~kept] == -1).all()
    assert np.array_equal(_bits(goal[kept]), _bits(raw["goal"][T - 1][kept]))
    assert (goal != g_boot).any(axis=1).all()
    # the next call's first pick differs from g'
    _, raw2, _ = _collect(Z, a, seed)
    assert (raw2["goal"][0] != g_boot).any(axis=1).all()
    a.close()


EDGES = [
    # name, n, h, skill_len, frames, calls
    ("PointTSP-25", 1, 64, 8, 24, 2),            # one env: a partial workgroup of one
    ("ColourMatch-v0", 5, 64, 8, 24, 2),         # a full and a partial workgroup
    ("PointTSP-25", 37, 32, 8, 8, 3),            # T = L: one window a call, only the bootstrap feeds the high GAE
    ("PointTSP-25", 37, 32, 1, 5, 3),            # L = 1: every frame picks, every frame auto-resets
    ("TimedTSP-25", 6, 191, 8, 16, 2),           # h = 191 with F = 7
]


@pytest.mark.parametrize("edge", EDGES, ids=["%s_N%d_h%d_L%d_T%d" % e[:5] for e in EDGES])
def test_edges(zenv_mod, edge):
    Z = zenv_mod
    name, n, h, skill_len, frames, calls = edge
    a, b = _env(Z, name, n), _env(Z, name, n)
    hi_sd, lo_sd = _load(Z, a, h=h, skill_len=skill_len)
    _load(Z, b, h=h, skill_len=skill_len)
    assert name != "TimedTSP-25" or a.zone_feat == 7
    outs, rec, seen = _collect_vs_replay(Z, a, b, hi_sd, lo_sd, seed=5, calls=calls, frames=frames, skill_len=skill_len)
    print(edge, seen)
    if skill_len == 1:
        assert all(not raw["reward"].any() for _, raw, _ in outs) and seen["idle"] == 0
    a.close()
    b.close()


def test_planted_goals_and_determinism(zenv_mod):
    """A handle that enters holding planted goals of age 3 still picks for every env on the first frame; a second handle
    with the same seed gives identical bytes."""
    Z = zenv_mod
    n, seed = 37, 9
    envs = [_env(Z, "PointTSP-25", n, pre=0) for _ in range(2)]
    planted = np.random.RandomState(1).uniform(-1, 1, (n, 2)).astype(np.float32)
    for e in envs:
        hi_sd, lo_sd = _load(Z, e)
        e.set_xy_goals(planted)
        for _ in range(3):
            e.policy(Z.POLICY_XY_SAMPLE, policy_seed=seed)
            e.step(None, auto_reset=False)
        assert (e.get(Z.F_XY_GOAL_AGE) == 3).all() and np.array_equal(e.get(Z.F_XY_GOAL), planted)
    step = envs[0].step_count
    res = [_collect(Z, e, seed) for e in envs]
    (lo, hi, nf), raw, boot = res[0]
    # every env picked on frame 0: the high level's draw at this step index, not the planted goal -- the policy's own
    # rule would have kept it for another five frames
    assert (raw["goal"][0] != planted).any(axis=1).all()
    gmu, gstd, _ = xy_ref.high(hi_sd, raw["obs"][0], raw["zone_obs"][0])
    z = (raw["goal"][0].astype(np.float64) - gmu) / gstd
    assert np.abs(z - xy_ref.goal_noise(n, seed, 0, step)).max() < 1e-3     # the bound of test_gpu_xy_goals.py's z check
    assert np.array_equal(_bits(hi["goal"].reshape(n, T // L, 2)[:, 0]), _bits(raw["goal"][0]))
    assert np.array_equal(_bits(hi["obs"].reshape(n, T // L, 8)[:, 0]), _bits(raw["obs"][0]))
    # identical bytes from the second handle
    (lo2, hi2, nf2), raw2, boot2 = res[1]
    for k in raw:
        assert np.array_equal(raw[k].view(np.uint8), raw2[k].view(np.uint8)), k
    for k in hi:
        assert np.array_equal(hi[k].view(np.uint8), hi2[k].view(np.uint8)), k
    for x, y in zip(boot, boot2):
        assert np.array_equal(_bits(x), _bits(y))
    assert nf == nf2
    for e in envs:
        e.close()


def test_refusals(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    lib = nat.lib()
    cfg = Z.config_for_id("PointTSP-v0")

    def refused(env, want, frames=16, discount=0.99, lam=0.95):
        steps, (o, zo) = env.step_count, env.observations()
        assert lib.zenv_collect_xy(env._h, frames, 1, 0, discount, lam) == want
        o2, zo2 = env.observations()
        assert env.step_count == steps and np.array_equal(o, o2) and np.array_equal(zo, zo2)

    env = Z.ZoneVecEnv(cfg, 16)
    env.build_bank(1, 16)
    env.reset()
    refused(env, Z.E_STATE)                                         # no zenv_xy_load
    hi, lo = xy_ref.random_state_dicts(env.zone_feat, 32)
    t = Z.xy_tensors_from_state_dicts(hi, lo)
    for drop in ("hi", "lo"):                                       # a critic missing
        env.load_xy({k: v for k, v in t.items() if not k.startswith(drop + "_critic")}, skill_len=L)
        refused(env, Z.E_STATE)
    env.load_xy(t, skill_len=L)
    for frames in (0, -8, 12, 4):                                   # T < 1, T % L != 0
        refused(env, Z.E_ARG, frames=frames)
    for d, lam in ((float("nan"), 0.95), (0.99, float("inf")), (1.5, 0.95), (0.99, -0.1), (-0.1, 0.95), (0.99, 1.5)):
        refused(env, Z.E_ARG, discount=d, lam=lam)
    with pytest.raises(ValueError):
        env.collect_xy(12)
    env.host_io(True)
    steps = env.step_count
    assert lib.zenv_collect_xy(env._h, 16, 1, 0, 0.99, 0.95) == Z.E_STATE and env.step_count == steps   # host I/O on
    env.host_io(False)
    assert lib.zenv_collect_xy(env._h, 16, 1, 0, 0.99, 0.95) == 0 and env.step_count == 16
    from tests import skill_ref
    shi, slo = skill_ref.random_state_dicts(env.zone_feat, 4, h=32)
    env.load_skills(Z.skill_tensors_from_state_dicts(shi, slo), skill_len=L)
    refused(env, Z.E_STATE)                                         # another agent's weights took the clock
    env.close()
    for enable in ("enable_goals", "enable_order"):                 # goal-conditioned / solver-ordered handles
        env = Z.ZoneVecEnv(cfg, 16)
        if enable == "enable_order":
            env.enable_order()
        env.build_bank(1, 16)
        if enable == "enable_goals":
            env.enable_goals()
        env.reset()
        refused(env, Z.E_STATE)
        env.close()
    env = Z.ZoneVecEnv(cfg, 16)                                     # before the first reset
    env.build_bank(1, 16)
    assert lib.zenv_collect_xy(env._h, 16, 1, 0, 0.99, 0.95) == Z.E_STATE
    env.close()


def test_torch_aliasing_and_one_update(zenv_mod):
    """TorchZoneEnv.collect_xy hands out tensors that alias the device buffers; one round of the example's two updates,
    the weights reloaded, and a second collection."""
    import importlib.util
    import os
    import torch
    Z = zenv_mod
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "xy_goals_ppo_torch.py")
    spec = importlib.util.spec_from_file_location("xy_goals_ppo_torch", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    env = _env(Z, "PointTSP-25", 257)
    tenv = TorchZoneEnv(env)
    algo = ex.XyGoalsPPO(tenv, h=32, skill_len=L, frames_per_proc=T, seed=1)
    lo, hi, num_frames = algo.collect()
    assert lo["value"].data_ptr() == env.device_ptr(Z._native.F_EXP_VALUE)
    assert hi["advantage"].data_ptr() == env.device_ptr(Z.F_HI_ADVANTAGE)
    assert hi["goal"].data_ptr() == env.device_ptr(Z.F_HI_GOAL)
    assert lo["goal"].shape == (257, T, 2) and hi["goal"].shape == (257 * T // L, 2)
    assert 0 < num_frames <= 257 * T
    before = {k: v.clone() for k, v in algo.hi.state_dict().items()}
    logs = algo.update(lo, hi)
    assert all(np.isfinite(v) for v in logs.values()), logs
    assert any(not torch.equal(before[k], v) for k, v in algo.hi.state_dict().items())
    lo2, hi2, _ = algo.collect()
    torch.cuda.synchronize()
    assert torch.isfinite(lo2["advantage"]).all() and torch.isfinite(hi2["advantage"]).all()
    env.close()
