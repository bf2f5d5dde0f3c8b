"""zenv_collect (BaseAlgo.collect_experiences, base.py:131-227) on every path that writes an experience record: each
network kernel of the flat actor-critic (bf16 split / 32 / 64 layouts with Z >= 4 and Z < 4, the float16 build,
k_mlp_f32, k_mlp_zone_f32m and k_mlp_zone_s3 with one and two 32-env groups per wave, bf16x3, both critic kinds), both
step kernels and an uncompiled zone count, batches at the 4-env / 256-thread / layout edges, T = 1, T longer than an
episode, a change of T, a goal-conditioned handle re-goaled between calls, and a collect between the other stepping
paths.  Every case is checked against a twin handle driven through public calls (mlp_forward, policy(MLP_SAMPLE),
step): frames and the handle's state afterwards bit for bit; the action draw against the host Philox; log_prob, the
networks and the GAE against float64 restatements (tests/collect_ref.py); self.mask across calls, a change of T and
a zenv_reset."""
import numpy as np
import pytest
import torch

from tests import collect_ref

pytestmark = pytest.mark.gpu

F64 = torch.float64
TSP, TTSP, CM = 0, 1, 2
SEED = 0xC011EC7
# The sampled action against mu + std * eps64 (the bar of test_mlp_sample_action_draws_exactly; measured over this
# module: 1.9 ulps).
ACT_ULPS = 4.0
# log_prob: float32 z = (a - mu) / std, -z^2/2 - logf(std) - log(2 pi)/2 against the float64 restatement, within LP_U
# units of 2^-24 (z^2/2 + |log std| + log(2 pi)/2); measured 3.5 on every network path.  A wrong term is off by
# O(0.01 .. 1), i.e. by 1e5 such units.
LP_U = 8.0
# the GAE: within GAE_U units of 2^-24 times collect_ref.gae's magnitude (measured 1.95 for returnn, 1.73 for the
# advantage; a wrong mask or slot is off by O(|v|)).
GAE_U = 4.0
# the networks against the float64 restatement: the float32-grade modes at their stated tolerance (include/zenv.h,
# ZoneVecEnv.load_mlp) relative to max(1, |ref|); bf16 / f16 against the rounding-point emulation at the existing bars.
# Measured worst (mu / std / value): f32 2.8e-7 / 1.3e-7 / 4.0e-7, f16x3 2.3e-7 / 1.4e-7 / 4.8e-7, bf16x3 2.2e-6 /
# 9.5e-7 / 3.5e-6, bf16 7.4e-4 / 3.4e-4 / 1.9e-3, f16 1.1e-4 / 5.3e-5 / 1.3e-4.
NET_TOL = {"f32": 1e-5, "f16x3": 3e-6, "bf16x3": 2e-5, "bf16": 4e-3, "f16": 5e-4}
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("collect paths worst: %-40s %.4g" % (k, WORST[k]))


def _cfg(Z, task, zones, num_steps=12, **over):
    keep = {25: 0.40, 15: 0.55, 9: 0.30}.get(zones, 0.45)
    return Z.default_config(task, zones, zones_keepout=keep, num_steps=num_steps, **over)


def _pair(Z, cfg, n, seed0=7, goals=False, stagger=True):
    """Two identical handles; with stagger, 4 zero-action steps and then a reset of every other env, so that episodes
    end at two different frames."""
    out = []
    for _ in range(2):
        env = Z.ZoneVecEnv(cfg, n)
        env.build_bank(seed0, n)
        if goals:
            env.enable_goals()
        env.reset()
        if stagger:
            for _ in range(4):
                env.step(np.zeros((n, 2), np.float32), auto_reset=True)
            env.reset((np.arange(n) % 2 == 0).astype(np.uint8))
        out.append(env)
    return out


def _tensors(env, h, seed, dist):
    from oracle import policy_ref as P
    return P.random_tensors(env.zone_feat, h=h, seed=seed, critic=True, distributional=dist)


def _load(pair, t, precision, monkeypatch, switch=None):
    """load_mlp on both handles; switch: ZENV_MLP_F32_VALU / _F32_MFMA (read at load) or ZENV_MLP_LAYOUT=..."""
    for v in ("ZENV_MLP_F32_VALU", "ZENV_MLP_F32_MFMA", "ZENV_MLP_LAYOUT"):
        monkeypatch.delenv(v, raising=False)
    if switch:
        name, _, val = switch.partition("=")
        monkeypatch.setenv(name, val or "1")
    for env in pair:
        env.load_mlp(t, precision=precision)


def _replay(Z, twin, T, seed, index0, goals):
    """The frames of one collect, driven through public calls on the twin: time-major records and the final state."""
    nat = Z._native
    log = {k: [] for k in ("obs", "zone_obs", "mu", "std", "value", "action", "reward", "done", "step")}
    for _ in range(T):
        o, zo = twin.observations()
        fwd = twin.mlp_forward(with_value=True)
        log["step"].append(twin.step_count)
        twin.policy(Z.POLICY_MLP_SAMPLE, policy_seed=seed, env_index0=index0)
        mu, std = twin.get(nat.F_POLICY_MU), twin.get(nat.F_POLICY_STD)
        assert np.array_equal(mu, fwd[0]) and np.array_equal(std, fwd[1])
        log["obs"].append(o)
        log["zone_obs"].append(zo)
        log["mu"].append(mu)
        log["std"].append(std)
        log["value"].append(fwd[2])
        log["action"].append(twin.get(nat.F_ACTIONS))
        twin.step(None, auto_reset=True)
        _, _, r, d, _ = twin.results()
        log["reward"].append(twin.goal_info()[0].astype(np.float32) if goals else r)
        log["done"].append(d)
    rec = {k: np.stack(v) for k, v in log.items()}
    rec["sigma"] = fwd[3] if len(fwd) > 3 else None
    return rec


def _state(Z, env):
    nat = Z._native
    out = {"blob": env.get_state(), "step": np.array([env.step_count])}
    for name in ("F_EP_RETURN", "F_EP_LEN", "F_EPISODES", "F_LAST_RETURN", "F_LAST_LEN", "F_OBS", "F_ZONE_OBS"):
        out[name] = env.get(getattr(nat, name))
    out["F_ACTIONS"] = env.get(nat.F_ACTIONS).view(np.uint32)
    return out


def _same_state(Z, a, b, tag):
    sa, sb = _state(Z, a), _state(Z, b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), (tag, k)


def _rows(n, k=384):
    """The envs whose network outputs are recomputed in float64: all of a small batch, both ends and a spread of a big one."""
    if n <= k:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(96), np.arange(n - 96, n), np.linspace(0, n - 1, k - 192).astype(int)]))


def _collect_and_check(Z, pair, t, precision, T, gl, tag, carried, index0=0, goals=False, oracle=None):
    """One collect on pair[0], the same frames on pair[1]; checks (a) - (e).  carried: the self.mask the call must
    record at frame 0.  Returns 1 - done of the last frame (the mask the next call must carry) and the number of
    episode ends inside the call."""
    env, twin = pair
    nat = Z._native
    n = env.num_envs
    g, lam = gl
    step0 = env.step_count
    assert twin.step_count == step0
    x = env.collect(T, policy_seed=SEED, env_index0=index0, discount=g, gae_lambda=lam)
    boot = env.get(nat.F_POLICY_VALUE)                       # value(obs_T), the GAE's bootstrap
    rec = _replay(Z, twin, T, SEED, index0, goals)
    tm = {k: np.ascontiguousarray(v.swapaxes(0, 1)) for k, v in x.items()}      # time-major [T, N, ...]
    # (a) replay: the frames bit for bit, then the handles' state
    for k in ("obs", "zone_obs", "action", "value", "reward"):
        assert np.array_equal(tm[k].view(np.uint32), rec[k].view(np.uint32)), (tag, k)
    mask = np.concatenate([np.asarray(carried, np.float32)[None], 1.0 - rec["done"][:-1].astype(np.float32)])
    assert np.array_equal(tm["mask"], mask), tag                                   # (f) frame 0: the carried self.mask
    _same_state(Z, env, twin, tag)
    if oracle is not None:
        oracle(tm, rec)
    # (b) the draws: mu + std * eps at (seed, env_index0 + env, step count + t), from the kernel's own mu / std
    for k in range(T):
        assert rec["step"][k] == step0 + k
        u = collect_ref.action_draw_ulps(tm["action"][k], rec["mu"][k], rec["std"][k], SEED, index0, step0 + k)
        _note("action ulps", u.max())
        assert u.max() <= ACT_ULPS, (tag, k, float(u.max()))
    # (c) log_prob from the recorded action and the twin's mu / std, float64
    lp, mag = collect_ref.normal_log_prob(tm["action"], rec["mu"], rec["std"])
    u = np.abs(tm["log_prob"] - lp) / (mag * 2.0 ** -24)
    _note("log_prob units " + precision, u.max())
    assert u.max() <= LP_U, (tag, float(u.max()))
    # (d) the networks against float64 (f32-grade modes) or the rounding-point emulation (bf16 / f16)
    from oracle import policy_ref as P
    rows = _rows(n)
    ob = tm["obs"][:, rows].reshape(-1, 8)
    zo = tm["zone_obs"][:, rows].reshape(len(ob), env.num_zones, env.zone_feat)
    if precision in ("bf16", "f16"):
        ref = P.forward_bf16_emulated(t, ob, zo, dtype=torch.bfloat16 if precision == "bf16" else torch.float16)
    else:
        ref = P.forward_fp32(t, ob, zo, dtype=F64)
    for name, dev, want in zip(("mu", "std", "value"), (rec["mu"], rec["std"], rec["value"]), ref):
        dev = dev[:, rows].reshape(want.shape).astype(np.float64)
        err = np.abs(dev - want) / np.maximum(1.0, np.abs(want))
        _note("%s %s rel" % (name, precision), err.max())
        assert err.max() <= NET_TOL[precision], (tag, name, float(err.max()))
    assert np.abs(ref[2]).max() > 0.05 and ref[1].std() > 1e-3               # not a degenerate network
    # (e) the GAE in float64 from the recorded reward / value / mask and the bootstrap
    last = 1.0 - rec["done"][-1].astype(np.float32)
    adv, ret, gmag = collect_ref.gae(tm["reward"], tm["value"], tm["mask"], last, boot, np.float32(g), np.float32(lam))
    for name, dev, want in (("advantage", tm["advantage"], adv), ("returnn", tm["returnn"], ret)):
        scale = gmag + (np.abs(tm["value"]) if name == "returnn" else 0)
        u = np.abs(dev - want) / np.maximum(scale * 2.0 ** -24, 1e-30)
        _note("gae units %s (%g, %g)" % (name, g, lam), u.max())
        assert u.max() <= GAE_U, (tag, name, float(u.max()))
    return last, int(rec["done"].sum())


def _oracle_checker(Z, O, cfg, n, seed0):
    """For a small batch built without a stagger: the recorded actions replayed through the CPU oracle reproduce the
    recorded observations and rewards bit for bit."""
    from tests.helpers import oracle_config_from
    refs = [O.OracleEnv(oracle_config_from(O, cfg)) for _ in range(n)]
    for i, e in enumerate(refs):
        e.reset(seed0 + i)

    def check(tm, rec):
        for k in range(tm["obs"].shape[0]):
            for i, e in enumerate(refs):
                o_ref, zo_ref = e.obs()
                assert np.array_equal(tm["obs"][k, i], o_ref) and np.array_equal(tm["zone_obs"][k, i], zo_ref), (k, i)
                r, d, _ = e.step(tm["action"][k, i])
                assert tm["reward"][k, i] == np.float32(r) and bool(rec["done"][k, i]) == bool(d), (k, i)
                if d:
                    e.reset(seed0 + i)
    check.refs = refs
    return check


# (name, task, Z, N, h, distributional, step kernel, [(precision, switch)], [T per call], (discount, gae_lambda))
CASES = [
    ("n1_tsp25_f16x3", TSP, 25, 1, 64, False, "lane", [("f16x3", None)], [1, 2, 13], (0.99, 0.95)),
    ("n3_cm6_f32", CM, 6, 3, 185, True, "lane", [("f32", None)], [12, 25], (1.0, 1.0)),
    ("n255_ttsp15_bf16_f16", TTSP, 15, 255, 64, False, "lane", [("bf16", None), ("f16", None)], [13, 7], (1.0, 0.0)),
    ("n256_tsp3_bf16_bf16x3", TSP, 3, 256, 33, True, "lane", [("bf16", None), ("bf16x3", "ZENV_MLP_F32_MFMA")], [9],
     (0.0, 0.95)),
    ("n257_cm9_f32m_s3", CM, 9, 257, 191, True, "lane", [("f32", "ZENV_MLP_F32_MFMA"), ("f16x3", "ZENV_MLP_F32_MFMA")],
     [14, 3], (0.99, 0.95)),
    ("n2050_tsp25_wave_valu", TSP, 25, 2050, 64, False, "wave", [("f16x3", "ZENV_MLP_F32_VALU"), ("bf16", None)], [13],
     (0.99, 0.95)),
    ("n2047_ttsp7", TTSP, 7, 2047, 64, False, "lane", [("f16x3", None)], [2], (1.0, 1.0)),
    ("n2048_ttsp7", TTSP, 7, 2048, 64, True, "lane", [("f16x3", None), ("bf16x3", None)], [2], (1.0, 0.0)),
    ("n8192_cm6", CM, 6, 8192, 64, False, "lane", [("bf16", None)], [2], (0.0, 0.95)),
    ("n8193_cm6", CM, 6, 8193, 64, False, "lane", [("bf16", None), ("bf16", "ZENV_MLP_LAYOUT=split")], [2],
     (0.99, 0.95)),
    ("n10239_tsp5", TSP, 5, 10239, 33, True, "lane", [("f32", None)], [2], (1.0, 1.0)),
    ("n10240_tsp5", TSP, 5, 10240, 33, True, "lane", [("f32", None)], [2], (0.99, 0.95)),
    ("n32768_ttsp5", TTSP, 5, 32768, 32, False, "lane", [("f32", None), ("bf16", None), ("f16x3", None)], [2],
     (1.0, 0.0)),
    ("n32769_ttsp5", TTSP, 5, 32769, 32, True, "lane", [("f32", None), ("bf16", None), ("f16x3", None),
                                                         ("bf16x3", None)], [2], (0.0, 0.95)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_collect_path_matrix(zenv_mod, oracle_mod, case, monkeypatch):
    Z, O = zenv_mod, oracle_mod
    name, task, zones, n, h, dist, kern, modes, Ts, gl = case
    over = {"kernel": Z._native.KERNEL_WAVE_PER_ENV} if kern == "wave" else {}
    cfg = _cfg(Z, task, zones, **over)
    small = n <= 3
    pair = _pair(Z, cfg, n, stagger=not small)
    oracle = _oracle_checker(Z, O, cfg, n, 7) if small else None
    carried = np.ones(n, np.float32)
    dones = 0
    for m, (precision, switch) in enumerate(modes):
        t = _tensors(pair[0], h, 100 + m, dist)
        _load(pair, t, precision, monkeypatch, switch)
        if precision == "f16x3":
            assert pair[0].mlp_precision == "f16x3"
        for c, T in enumerate(Ts):
            tag = (name, precision, switch, c, T)
            carried, ended = _collect_and_check(Z, pair, t, precision, T, gl, tag, carried, index0=37 * c,
                                                oracle=oracle)
            dones += ended
    if max(Ts) > 12:                                    # longer than an episode: the mask and auto-reset were met
        assert dones > 0, "no episode ended inside a call"
    for e in pair:
        e.close()


def test_collect_after_a_reset_keeps_self_mask(zenv_mod, oracle_mod):
    """include/zenv.h: zenv_reset does not touch self.mask -- after a full and a masked reset the next call's frame 0
    still records 1 - done of the previous call's last frame.  Episodes of 12 steps, calls of 12 frames: every env
    ends on a call's last frame, so the carried mask is 0 (a reset to ones would show)."""
    Z, O = zenv_mod, oracle_mod
    n, T = 3, 12
    cfg = _cfg(Z, TSP, 25)
    pair = _pair(Z, cfg, n, stagger=False)
    oracle = _oracle_checker(Z, O, cfg, n, 7)
    t = _tensors(pair[0], 64, 5, False)
    for e in pair:
        e.load_mlp(t, precision="f32")
    carried, _ = _collect_and_check(Z, pair, t, "f32", T, (0.99, 0.95), "first", np.ones(n, np.float32), oracle=oracle)
    assert (carried == 0).all()
    for e in pair:
        e.reset()
    for i, e in enumerate(oracle.refs):
        e.reset(7 + i)
    carried, _ = _collect_and_check(Z, pair, t, "f32", T, (0.99, 0.95), "after reset", carried, oracle=oracle)
    assert (carried == 0).all()
    for e in pair:
        e.reset(np.array([1, 0, 0], np.uint8))
    oracle.refs[0].reset(7)
    _collect_and_check(Z, pair, t, "f32", 5, (0.99, 0.95), "after masked reset", carried, oracle=oracle)
    for e in pair:
        e.close()


def test_collect_between_the_other_stepping_paths(zenv_mod, monkeypatch):
    """A persistent rollout, a collect, a step_many chunk, a collect, host steps, a collect (with another T): each
    collect is the twin's replay and the handles' state stays equal throughout."""
    Z = zenv_mod
    n = 131
    cfg = _cfg(Z, TTSP, 15, num_steps=20)
    pair = _pair(Z, cfg, n)
    t = _tensors(pair[0], 64, 9, True)
    _load(pair, t, "f16x3", monkeypatch)
    rs = np.random.RandomState(1)
    carried = np.ones(n, np.float32)
    for e in pair:
        e.rollout(23, Z.POLICY_GREEDY, mode="persistent")
    _same_state(Z, *pair, "rollout")
    carried, _ = _collect_and_check(Z, pair, t, "f16x3", 9, (0.99, 0.95), "after rollout", carried)
    a = rs.uniform(-1, 1, (17, n, 2)).astype(np.float32)
    for e in pair:
        e.step_many(a, reset="every")
    _same_state(Z, *pair, "step_many")
    # step_many's steps leave self.mask alone: it is the collector's
    carried, _ = _collect_and_check(Z, pair, t, "f16x3", 9, (1.0, 1.0), "after step_many", carried)
    for _ in range(5):
        a = rs.uniform(-1, 1, (n, 2)).astype(np.float32)
        for e in pair:
            e.step(a, auto_reset=True)
    _collect_and_check(Z, pair, t, "f16x3", 21, (1.0, 0.0), "after host steps", carried)
    for e in pair:
        e.close()


def test_collect_on_a_regoaled_handle(zenv_mod, monkeypatch):
    """A goal-conditioned handle: 30 frames per call (envs that reach their goal wait for the next one, as the device
    does), then every env that needs a goal is given one on both handles, and a second call; the recorded reward is
    the shaped one."""
    Z = zenv_mod
    n = 131
    cfg = _cfg(Z, TSP, 25, num_steps=25)
    pair = _pair(Z, cfg, n, goals=True, stagger=False)
    g0 = (np.arange(n) % 25).astype(np.int32)
    for e in pair:
        e.set_goals(g0)
    t = _tensors(pair[0], 64, 4, False)
    _load(pair, t, "f32", monkeypatch)
    carried = np.ones(n, np.float32)
    rs = np.random.RandomState(2)
    regoaled = 0
    for c in range(3):
        carried, _ = _collect_and_check(Z, pair, t, "f32", 30, (0.99, 0.95), ("goals", c), carried,
                                        index0=1000 * c, goals=True)
        need, avail = pair[0].goal_info()[1], pair[0].goal_info()[2]
        assert np.array_equal(need, pair[1].goal_info()[1])
        g = np.full(n, -1, np.int32)
        for i in np.nonzero(need)[0]:
            opts = [z for z in range(25) if (int(avail[i]) >> z) & 1]
            if opts:
                g[i] = rs.choice(opts)
        regoaled += int((g >= 0).sum())
        for e in pair:
            e.set_goals(g)
    assert regoaled > 0
    for e in pair:
        e.close()


def test_collect_refusals(zenv_mod):
    """ZENV_E_ARG for what zenv_collect_skill refuses as well: a non-finite discount / gae_lambda, one outside [0, 1],
    frames x envs >= 2^31 -- before any state is touched (the call after them is the first collect)."""
    from oracle import policy_ref as P
    Z = zenv_mod
    lib = Z._native.lib()
    env = Z.ZoneVecEnv(_cfg(Z, TSP, 5), 2)
    env.build_bank(1, 2)
    env.reset()
    env.load_mlp(P.random_tensors(env.zone_feat, h=32, critic=True), precision="f32")
    for d, lam in ((float("nan"), 0.95), (0.99, float("nan")), (float("inf"), 0.95), (0.99, -float("inf")),
                   (1.5, 0.95), (0.99, -0.1), (-0.01, 0.5), (0.5, 1.01)):
        assert lib.zenv_collect(env._h, 4, 1, 0, d, lam) == Z.E_ARG, (d, lam)
    assert lib.zenv_collect(env._h, 2 ** 30, 1, 0, 0.99, 0.95) == Z.E_ARG            # 2^30 x 2 envs = 2^31
    assert lib.zenv_collect(env._h, 0, 1, 0, 0.99, 0.95) == Z.E_ARG
    for d, lam in ((0.0, 0.0), (1.0, 1.0)):                                           # the closed interval's ends
        assert lib.zenv_collect(env._h, 3, 1, 0, d, lam) == 0
    with pytest.raises(Z.ZenvError):
        env.collect(4, discount=float("nan"))
    env.close()
