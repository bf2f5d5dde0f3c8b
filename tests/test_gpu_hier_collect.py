"""zenv_collect_hier: collect_experiences of the Zone-goals agent (zone-goals/src/torch_ac/algos/_hier_policy_opt.py:9-171)
on the device.  Checked against the same frames driven by zenv_policy(HIER_SAMPLE) + zenv_step (bit for bit), the CPU
oracle (env half), the torch restatement of both networks (tests/hier_ref.py) and a numpy restatement of the
bookkeeping: the two GAE recursions, the T-1 frame cut, the env-major flattening and the transition carried from one
call to the next."""
import ctypes as C

import numpy as np
import pytest

from tests import hier_ref
from tests.hier_collect_ref import GAMMA, LAM
from tests.hier_collect_ref import expected_hi as _expected_hi, log_softmax_at as _log_softmax_at, replay as _replay

pytestmark = pytest.mark.gpu

BASE = {"PointTSP-v3": "PointTSP-v0", "PointTTSP-v3": "PointTTSP-v0", "ColourMatch-v3": "ColourMatch-v0"}


def _goal_env(Z, env_id, n, seed=11, **over):
    cfg = Z.config_for_id(BASE.get(env_id, env_id), **over)
    env = Z.ZoneVecEnv(cfg, n)
    env.build_bank(seed, n)
    env.schedule_sequential()
    env.enable_goals()
    env.reset()
    return env


def _load(Z, env, h=128, seed=0, critics=True):
    hi, lo = hier_ref.random_state_dicts(env.zone_feat, h=h, seed=seed, critics=critics)
    env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
    return hi, lo


def _raw(Z, env, field, shape, dtype=np.float32):
    """A whole time-major buffer (all T frames, the last included)."""
    a = np.empty(shape, dtype)
    assert a.nbytes == env.field_bytes(field)
    Z._native.check(Z._native.lib().zenv_get(env._h, field, a.ctypes.data, 0))
    return a


@pytest.mark.parametrize("env_id", ["PointTSP-v3", "PointTTSP-v3", "ColourMatch-v3"])
def test_collect_hier_is_the_replayed_frames(zenv_mod, env_id):
    """Two consecutive calls against zenv_policy(HIER_SAMPLE) + zenv_step on a second handle: every low-level record
    bit for bit, the high-level rows (goal, mask, obs, value, reward, hi_mask) exactly, log_prob and both GAEs within
    1e-5 of numpy; the transition open at the end of the first call is the first row of the second."""
    import torch
    Z = zenv_mod
    # Episodes of 60 steps; zones of radius 0.5 (keepout as usual) and a low level that drives forward (mu_'s bias), so
    # that some goals are reached.  The replay handle runs first; T is then chosen so that some env reaches its goal in
    # the last frame of a call: that transition closes with hi_mask 1 and no pick after it, so its V_next is
    # V_hi(obs_T) and the bootstrap value enters its advantage.  Two calls of T >= 31 frames also cover an episode end
    # (hi_mask 0) and a transition open across the boundary.
    n, calls, seed, frames = 203, 2, 77, 180
    a = _goal_env(Z, env_id, n, num_steps=60, zones_size=0.5)
    b = _goal_env(Z, env_id, n, num_steps=60, zones_size=0.5)
    hi_sd, lo_sd = hier_ref.random_state_dicts(a.zone_feat, h=128, seed=3)
    lo_sd["actor.mu_.bias"] = lo_sd["actor.mu_.bias"] + torch.tensor([4.0, 0.0])
    for e in (a, b):
        e.load_hier(Z.hier_tensors_from_state_dicts(hi_sd, lo_sd))
    rec = _replay(Z, b, frames, seed)
    reached = np.nonzero((rec["need_after"] & ~rec["done"].astype(bool)).any(1))[0]     # frames where a goal is reached
    candidates = sorted({t + 1 for t in reached if 31 <= t + 1 < frames // 2} |
                        {(t + 1) // 2 for t in reached if t % 2 == 1 and 31 <= (t + 1) // 2 < frames // 2})
    if env_id != "PointTTSP-v3":
        assert candidates, "no goal reached in a usable frame"
    T = candidates[-1] if candidates else frames // 2 - 1
    outs, v_final = [], []
    for c in range(calls):
        lo, hi = a.collect_hier(T, policy_seed=seed, discount=GAMMA, gae_lambda=LAM)
        raw = {name: _raw(Z, a, f, s) for name, (f, s, _) in
               Z.hier_experience_layout(n, a.num_zones, a.zone_feat, T, 0)[0].items()}
        outs.append((lo, hi, raw))
        v_final.append(a.get(Z.F_HIER_VALUE))
    o_end, zo_end = a.observations()
    _, need_end, avail_end, _ = a.goal_info()
    assert np.array_equal(o_end, rec["obs"][calls * T]) and np.array_equal(zo_end, rec["zone_obs"][calls * T])
    assert np.array_equal(need_end, rec["need"][calls * T]) and np.array_equal(avail_end, rec["avail"][calls * T])
    exp, seen = _expected_hi(rec, T, calls, v_final)
    prev_done = np.zeros(n, np.uint8)
    for c, (lo, hi, raw) in enumerate(outs):
        fr = slice(c * T, (c + 1) * T)
        # ---- low level, every frame of the call (time-major raw buffers), bit for bit
        assert np.array_equal(raw["obs"], rec["obs"][fr]) and np.array_equal(raw["zone_obs"], rec["zone_obs"][fr])
        assert np.array_equal(raw["action"], rec["action"][fr])
        assert np.array_equal(raw["value"], rec["value"][fr])
        assert np.array_equal(raw["reward"], rec["shaped"][fr].astype(np.float32))
        assert np.array_equal(raw["env_reward"], rec["reward"][fr])
        done_prev = np.concatenate([prev_done[None], rec["done"][fr][:-1]])
        assert np.array_equal(raw["mask"], 1.0 - done_prev.astype(np.float32))
        prev_done = rec["done"][fr][-1]
        g = rec["goal"][fr]
        has = g >= 0
        assert has.all()
        tt, jj = np.nonzero(has)
        want_goal = rec["zone_obs"][fr][tt, jj, g[tt, jj], :2]
        assert np.abs(raw["goal"][tt, jj] - want_goal).max() <= 1e-6
        mu, std = rec["mu"][fr], rec["std"][fr]
        lp = -0.5 * ((raw["action"] - mu) / std) ** 2 - np.log(std) - 0.5 * np.log(2 * np.pi)
        assert np.abs(lp - raw["log_prob"]).max() < 2e-3
        # the T-1 frame cut and the GAE without bootstrap
        assert lo["obs"].shape == (n, T - 1, 8) and lo["goal"].shape == (n, T - 1, 2)
        assert np.array_equal(lo["action"], raw["action"][:T - 1].swapaxes(0, 1))
        adv = np.zeros((T, n), np.float32)
        for i in reversed(range(T - 1)):
            nm = raw["mask"][i + 1]
            delta = raw["reward"][i] + np.float32(GAMMA) * raw["value"][i + 1] * nm - raw["value"][i]
            adv[i] = delta + np.float32(GAMMA) * np.float32(LAM) * adv[i + 1] * nm
        assert np.abs(lo["advantage"] - adv[:T - 1].T).max() < 1e-5
        assert np.abs(lo["returnn"] - (lo["value"] + lo["advantage"])).max() < 1e-5
        assert not raw["advantage"][T - 1].any()
        # ---- high level: env-major rows
        counts = [len(r) for r in exp[c]]
        assert np.array_equal(hi["count"], counts) and len(hi["action"]) == sum(counts)
        rows = [r for per_env in exp[c] for r in per_env]
        if not rows:
            continue
        tp = np.array([r["t_pick"] for r in rows])
        jj = np.repeat(np.arange(n), counts)
        assert np.array_equal(hi["action"], [r["goal"] for r in rows])
        assert np.array_equal(hi["obs"], rec["obs"][tp, jj]) and np.array_equal(hi["zone_obs"], rec["zone_obs"][tp, jj])
        bits = (rec["avail"][tp, jj][:, None] >> np.arange(a.num_zones, dtype=np.uint32)) & 1
        assert hi["action_mask"].dtype == bool and np.array_equal(hi["action_mask"], bits.astype(bool))
        assert np.array_equal(hi["value"], [r["value"] for r in rows])
        assert np.array_equal(hi["reward"], np.array([r["reward"] for r in rows], np.float32))
        assert np.array_equal(hi["mask"], [r["mask"] for r in rows])
        want_lp = [_log_softmax_at(rec["logits"][t, j], g) for t, j, g in zip(tp, jj, hi["action"])]
        assert np.abs(hi["log_prob"] - want_lp).max() < 1e-5
        assert np.abs(hi["advantage"] - [r["adv"] for r in rows]).max() < 1e-5
        assert np.abs(hi["returnn"] - (hi["value"] + hi["advantage"])).max() < 1e-5
        # the bootstrap value is the high critic on the final observation
        o_T, zo_T = rec["obs"][(c + 1) * T], rec["zone_obs"][(c + 1) * T]
        _, rv = hier_ref.high(hi_sd, o_T, zo_T, np.full(n, 0xFFFFFFFF, np.uint32))
        assert np.all(np.abs(v_final[c] - rv) <= 1e-5 * np.maximum(1.0, np.abs(rv)))
    # the test met every case it is about.  TimedTSP's episodes end by timeout before this agent reaches a goal: the
    # goal-reached close and the V_hi(obs_T) bootstrap are covered by the other two tasks.
    assert seen["span"] > 0 and seen["mask0"] > 0, seen
    if env_id != "PointTTSP-v3":
        assert seen["mask1"] > 0 and seen["bootstrap"] > 0, seen
    a.close()
    b.close()


def test_reset_between_calls_drops_the_open_transition(zenv_mod):
    """zenv_reset ends the episodes: the transition left open by the first call is dropped and hi_reward restarts at 0,
    so the second call's rows are those of a fresh start (the same frames replayed by zenv_policy + zenv_step with the
    same reset in between).  10 003 envs: the row offsets come from a prefix sum over several tiles and a ragged tail."""
    import torch
    Z = zenv_mod
    # the first call stays inside the episodes of 60 steps (the open transitions gather reward), the second (a new T)
    # outlasts one, so that every env closes at least one transition
    n, T, T2, seed = 10003, 45, 70, 5
    a = _goal_env(Z, "PointTSP-v3", n, num_steps=60, zones_size=0.5)
    b = _goal_env(Z, "PointTSP-v3", n, num_steps=60, zones_size=0.5)
    hi_sd, lo_sd = hier_ref.random_state_dicts(a.zone_feat, h=64, seed=6)
    lo_sd["actor.mu_.bias"] = lo_sd["actor.mu_.bias"] + torch.tensor([4.0, 0.0])
    for e in (a, b):
        e.load_hier(Z.hier_tensors_from_state_dicts(hi_sd, lo_sd))
    a.collect_hier(T, policy_seed=seed, gae_lambda=LAM)
    a.reset()
    lo, hi = a.collect_hier(T2, policy_seed=seed, gae_lambda=LAM)
    v_final = a.get(Z.F_HIER_VALUE)
    rec1 = _replay(Z, b, T, seed)
    b.reset()
    rec2 = _replay(Z, b, T2, seed)
    # what the reset throws away: hi_reward of the transition still open after the first call
    left = np.zeros(n, np.float32)
    for t in range(T):
        left = np.where(rec1["need_after"][t] != 0, np.float32(0), (left + rec1["reward"][t]).astype(np.float32))
    assert (left != 0).any()
    exp, _ = _expected_hi(rec2, T2, 1, [v_final])
    rows = [r for per_env in exp[0] for r in per_env]
    counts = [len(r) for r in exp[0]]
    assert np.array_equal(hi["count"], counts) and len(rows) > n
    tp = np.array([r["t_pick"] for r in rows])
    jj = np.repeat(np.arange(n), counts)
    assert np.array_equal(hi["action"], [r["goal"] for r in rows])
    assert np.array_equal(hi["obs"], rec2["obs"][tp, jj]) and np.array_equal(hi["zone_obs"], rec2["zone_obs"][tp, jj])
    assert np.array_equal(hi["reward"], np.array([r["reward"] for r in rows], np.float32))
    assert np.array_equal(hi["mask"], [r["mask"] for r in rows])
    assert np.abs(hi["advantage"] - [r["adv"] for r in rows]).max() < 1e-5
    a.close()
    b.close()


def test_env_half_matches_the_oracle(zenv_mod, oracle_mod):
    """The recorded goals and actions replayed through the CPU oracle (set_goal / step_goal, auto-reset) reproduce the
    recorded observations, shaped and env rewards and masks bit for bit, and every transition's reward (the float32 sum
    in step order)."""
    from tests.helpers import oracle_config_from
    Z, O = zenv_mod, oracle_mod
    n, T, seed0 = 48, 50, 31
    cfg = Z.config_for_id("PointTSP-v0", num_steps=40)
    env = _goal_env(Z, "PointTSP-v3", n, seed=seed0, num_steps=40)
    _load(Z, env, seed=8)
    refs = [O.OracleEnv(oracle_config_from(O, cfg)) for _ in range(n)]
    for i, e in enumerate(refs):
        e.reset(seed0 + i)
    need = np.ones(n, bool)
    hr = np.zeros(n, np.float32)
    open_ = np.zeros(n, bool)
    mask = np.ones(n, np.float32)
    n_close = 0
    goal_zone = np.full(n, -1)
    for call in range(2):
        lo, hi = env.collect_hier(T, policy_seed=5)
        raw = {name: _raw(Z, env, f, s) for name, (f, s, _) in
               Z.hier_experience_layout(n, env.num_zones, env.zone_feat, T, 0)[0].items()}
        hi_rows = np.concatenate([[0], np.cumsum(hi["count"])])
        k_env = np.zeros(n, int)
        for t in range(T):
            for i, e in enumerate(refs):
                o, zo = e.obs()
                assert np.array_equal(raw["obs"][t, i], o) and np.array_equal(raw["zone_obs"][t, i], zo), (call, t, i)
                assert raw["mask"][t, i] == mask[i]
                if need[i]:
                    # the goal picked at this frame: the zone whose centre / 3 is the recorded goal input
                    g = int(np.argmin(np.abs(zo[:, :2] - raw["goal"][t, i]).sum(1)))
                    assert np.abs(zo[g, :2] - raw["goal"][t, i]).max() <= 1e-6
                    assert e.available_goals()[g]
                    e.set_goal(g)
                    goal_zone[i] = g
                    open_[i] = True
                r, d, _, sh, nd = e.step_goal(raw["action"][t, i])
                assert raw["reward"][t, i] == np.float32(sh) and raw["env_reward"][t, i] == np.float32(r)
                hr[i] = np.float32(hr[i] + np.float32(r))
                if nd:
                    if open_[i]:
                        row = hi_rows[i] + k_env[i]
                        assert k_env[i] < hi["count"][i]
                        assert hi["reward"][row] == hr[i] and hi["mask"][row] == (0.0 if d else 1.0)
                        assert hi["action"][row] == goal_zone[i]
                        k_env[i] += 1
                        n_close += 1
                        open_[i] = False
                    hr[i] = 0
                need[i] = nd
                mask[i] = 0.0 if d else 1.0
                if d:
                    e.reset(seed0 + i)
        assert np.array_equal(k_env, hi["count"])
    assert n_close > n
    env.close()


@pytest.mark.parametrize("env_id,h", [("PointTSP-v3", 128), ("ColourMatch-v3", 64)])
def test_recorded_networks_match_torch(zenv_mod, env_id, h):
    """The recorded low-level value / log_prob and the high-level value / log_prob(goal) against tests/hier_ref.py on the
    recorded observations, goals and action masks."""
    Z = zenv_mod
    n, T = 203, 30
    env = _goal_env(Z, env_id, n, num_steps=25)
    hi_sd, lo_sd = _load(Z, env, h=h, seed=h)
    lo, hi = env.collect_hier(T, policy_seed=9)
    f = lambda x, *s: np.ascontiguousarray(x).reshape(n * (T - 1), *s)
    mu, std, val = hier_ref.low(lo_sd, f(lo["obs"], 8), f(lo["zone_obs"], env.num_zones, env.zone_feat), f(lo["goal"], 2))
    tol = lambda ref: 1e-5 * np.maximum(1.0, np.abs(ref))
    assert np.all(np.abs(f(lo["value"]) - val) <= tol(val))
    lp = -0.5 * ((f(lo["action"], 2) - mu) / std) ** 2 - np.log(std) - 0.5 * np.log(2 * np.pi)
    assert np.abs(lp - f(lo["log_prob"], 2)).max() < 2e-3
    assert len(hi["action"]) > n // 2
    bits = (hi["action_mask"].astype(np.uint32) << np.arange(env.num_zones, dtype=np.uint32)).sum(1)
    logits, hv = hier_ref.high(hi_sd, hi["obs"], hi["zone_obs"], bits)
    assert np.all(np.abs(hi["value"] - hv) <= tol(hv))
    want = [_log_softmax_at(l, g) for l, g in zip(logits, hi["action"])]
    assert np.abs(hi["log_prob"] - want).max() < 1e-4
    env.close()


def test_refusals(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    raw = lambda env, T, d=0.99, lam=0.95: nat.lib().zenv_collect_hier(env._h, T, 1, 0, d, lam, C.byref(C.c_int64()))

    def code(env, T=8, d=0.99, lam=0.95):
        rc = raw(env, T, d, lam)
        assert rc < 0
        return rc
    cfg = Z.config_for_id("PointTSP-v0")
    env = Z.ZoneVecEnv(cfg, 16)
    env.build_bank(1, 16)
    env.reset()
    assert code(env) == Z.E_STATE                                   # no goals
    env.enable_goals()
    env.reset()
    assert code(env) == Z.E_STATE                                   # no hier weights
    _load(Z, env, h=32, critics=False)
    assert code(env) == Z.E_STATE                                   # no critic
    hi, lo = hier_ref.random_state_dicts(6, h=32)
    t = Z.hier_tensors_from_state_dicts(hi, lo)
    for drop in ("hi", "lo"):                                       # one critic missing
        env.load_hier({k: v for k, v in t.items() if not k.startswith(drop + "_critic")})
        assert code(env) == Z.E_STATE
    env.load_hier(t)
    assert code(env, 1) == Z.E_ARG and code(env, 0) == Z.E_ARG     # T < 2
    assert code(env, 2 ** 27) == Z.E_ARG                            # T x 16 envs = 2^31
    for d, lam in ((float("nan"), 0.95), (0.99, float("nan")), (float("inf"), 0.95), (0.99, -float("inf")),
                   (1.5, 0.95), (0.99, -0.1), (-0.01, 0.5), (0.5, 1.01)):
        assert code(env, 8, d, lam) == Z.E_ARG, (d, lam)           # as zenv_collect_skill refuses them
    with pytest.raises(ValueError):
        env.collect_hier(1)
    env.host_io(True)
    assert code(env) == Z.E_STATE                                   # host I/O
    env.host_io(False)
    lo_x, hi_x = env.collect_hier(4)
    assert lo_x["obs"].shape == (16, 3, 8)
    env.close()
    order = Z.ZoneVecEnv(Z.config_for_id("PointTSP-v0"), 8)
    order.enable_order()
    order.build_bank(1, 8)
    order.reset()
    assert code(order) == Z.E_STATE                                 # solver-ordered
    order.close()


def test_flat_collect_on_a_goal_handle_is_unchanged(zenv_mod):
    """zenv_collect on a goal-conditioned handle still runs the flat network and records shaped rewards, also after a
    collect_hier on the same handle."""
    from oracle import policy_ref as P
    Z = zenv_mod
    n, T = 40, 6
    envs = [_goal_env(Z, "PointTSP-v3", n, num_steps=50) for _ in range(2)]
    t = P.random_tensors(6, seed=2, critic=True)
    nz = envs[0].num_zones
    for e in envs:
        e.load_mlp(t, precision="f32")
        e.set_goals(np.arange(n, dtype=np.int32) % nz)
    _load(Z, envs[1], seed=1)
    envs[1].collect_hier(5)
    _, need, avail, _ = envs[1].goal_info()
    first_free = np.array([min(z for z in range(nz) if (v >> z) & 1) for v in avail])
    envs[1].set_goals(np.where(need, first_free, -1).astype(np.int32))
    for e in envs:
        x = e.collect(T, policy_seed=3)
        _, _, val = P.forward_fp32(t, x["obs"].reshape(-1, 8), x["zone_obs"].reshape(n * T, nz, -1))
        assert np.abs(val.reshape(n, T) - x["value"]).max() < 1e-5          # the flat critic, not the hierarchical one
        assert np.array_equal(x["reward"][:, -1], e.goal_info()[0].astype(np.float32))   # shaped rewards
    for e in envs:
        e.close()


def test_torch_tensors_alias_and_the_example_trains(zenv_mod):
    """TorchZoneEnv.collect_hier: CUDA tensors aliasing the device buffers, equal to the numpy path; two iterations of
    examples/zone_goals_ppo_torch.py's update run and change both networks' outputs."""
    import importlib.util
    import os
    import torch
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    Z = zenv_mod
    n, T = 64, 24
    envs = [_goal_env(Z, "PointTSP-v3", n, num_steps=30) for _ in range(2)]
    for e in envs:
        _load(Z, e, h=64, seed=4)
    lo_np, hi_np = envs[0].collect_hier(T, policy_seed=2)
    tz = TorchZoneEnv(envs[1])
    lo_t, hi_t = tz.collect_hier(T, policy_seed=2)
    torch.cuda.synchronize()
    assert lo_t["obs"].is_cuda and lo_t["obs"].shape == (n, T - 1, 8)
    assert lo_t["obs"].data_ptr() == envs[1].device_ptr(Z._native.F_EXP_OBS)
    if len(hi_np["action"]):
        assert hi_t["zone_obs"].data_ptr() == envs[1].device_ptr(Z.F_HI_ZONE_OBS)
    for k in lo_np:
        assert np.array_equal(lo_t[k].cpu().numpy(), lo_np[k]), k
    for k in hi_np:
        assert np.array_equal(hi_t[k].cpu().numpy(), hi_np[k]), k
    assert hi_t["action_mask"].dtype == torch.bool
    envs[0].close()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "zone_goals_ppo_torch.py")
    spec = importlib.util.spec_from_file_location("zone_goals_ppo_torch", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    dev = tz.device
    torch.manual_seed(0)
    hi_net, lo_net = ex.HighPolicyValueModel(6, 64).to(dev), ex.LoPolicyValueModel(6, 64).to(dev)
    probe = (tz.obs.clone(), tz.zone_obs.clone(), torch.zeros(n, 2, device=dev))
    with torch.no_grad():
        before = (hi_net(probe[0], probe[1])[0].clone(), lo_net(*probe)[0].mean.clone())
    algo = ex.HierPPO(tz, hi_net, lo_net, frames_per_proc=T, epochs=2, batch_size=256)
    for _ in range(2):
        logs = algo.iteration()
        assert np.isfinite(logs["lo_policy_loss"]) and np.isfinite(logs["hi_policy_loss"])
    with torch.no_grad():
        after = (hi_net(probe[0], probe[1])[0], lo_net(*probe)[0].mean)
    assert not torch.allclose(before[0], after[0]) and not torch.allclose(before[1], after[1])
    envs[1].close()
