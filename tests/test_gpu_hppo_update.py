"""The Zone-goals agent's two PPO updates on the device (zenv_hppo_*, ppo_update.hip) against the float64 restatement of
tests/hppo_update_ref.py, on the records of a real zenv_collect_hier.  Every comparison of two floating-point results
follows one rule (ppo_update_ref.check_rule): the device may deviate from the float64 run by 8 times what the float32
run of the same torch code on the CPU does, or by 8 ulp at the tensor's scale, whichever is larger.

Handles: goal-enabled, episodes of 12 steps and T = 33 frames, so every env's episode ends at frames 12 and 24 and
M >= 2 N high-level transitions close by construction.  Shapes: PointTSP-v0 (Z 15, F 6, h 185, N 24), ColourMatch-v0
(Z 6, F 7, h 7 and 64, N 5), PointTTSP-v0 (Z 15, F 7, h 191, N 8), 25 zones (h 32, N 4).  Rows 0-7 of the high level's
records are planted through TorchZoneEnv's aliases so that every loss branch is reached by construction."""
import math

import numpy as np
import pytest
import torch

from tests import hier_ref as H
from tests import hppo_update_ref as R
from tests import ppo_update_dev as D
from tests import ppo_update_ref as RF

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
T = D.HIER_T
CASES = {"tsp": ("PointTSP-v0", 185, 24), "cm7": ("ColourMatch-v0", 7, 5), "cm64": ("ColourMatch-v0", 64, 5),
         "ttsp": ("PointTTSP-v0", 191, 8), "z25": (None, 32, 4)}
LEVELS = D.LEVELS
HYPER = {"lo": R.LO_HYPER, "hi": R.HI_HYPER}
PLANTED = D.PLANTED
_SETUPS = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _SETUPS.values():
        s["env"].set_stream(None)
        s["env"].close()
    D.print_worst(REPORT, "hppo update", 44)


def _setup(Z, case, tag=""):
    """One handle per shape: fresh parameters loaded into the acting agent, one collect_hier, rows 0-7 planted."""
    key = case + tag
    if key not in _SETUPS:
        env_id, h, N = CASES[case]
        cfg = (Z.config_for_id(env_id, num_steps=12) if env_id
               else Z.default_config(0, 25, zones_keepout=0.40, num_steps=12))
        _SETUPS[key] = D.hier_setup(Z, cfg, h, N, seed=list(CASES).index(case))
    return _SETUPS[key]


_batch, _by_key, _init, _indexes = D.hier_batch, D.hier_by_key, D.hier_init, D.hier_indexes


def _check_minibatch(Z, s, level, sd, idx, hyper, tag):
    return D.hier_check_minibatch(Z, s, level, sd, idx, hyper, tag, REPORT)


LO_FRESH = [("tsp", 1), ("tsp", 37), ("tsp", 100), ("tsp", "all"), ("cm7", "all"), ("cm64", "all"), ("ttsp", "all"),
            ("z25", "all")]
HI_FRESH = [("tsp", 1), ("tsp", 33), ("tsp", "all"), ("cm7", "all"), ("cm64", "all"), ("ttsp", "all"), ("z25", "all")]


@pytest.mark.parametrize("case,batch", LO_FRESH)
def test_low_level_on_fresh_parameters(zenv_mod, case, batch):
    s = _setup(zenv_mod, case)
    idx = _indexes(s, "lo", batch, 1)
    assert s["total"]["lo"] - 1 in idx and len(idx) == (s["N"] * (T - 1) if batch == "all" else batch)
    stats, s64, s32 = _check_minibatch(zenv_mod, s, "lo", s["lo_sd"], idx, R.LO_HYPER, f"fresh-{case}")
    # unchanged parameters right after the collect: ratio = 1, so the policy loss is -mean(advantage)
    adv = _batch(s, "lo", idx, F64)["advantage"]
    R.check_rule(f"fresh-{case}/lo.policy_loss_at_ratio_1", stats[3], -float(adv.mean()), s32["policy_loss"], REPORT)
    assert stats[2] == 0.0


@pytest.mark.parametrize("case,batch", HI_FRESH)
def test_high_level_on_fresh_parameters(zenv_mod, case, batch):
    s = _setup(zenv_mod, case)
    idx = _indexes(s, "hi", batch, 2)
    assert s["M"] - 1 in idx
    if batch == "all":                                      # the planted rows: every branch has a sample
        b = _batch(s, "hi", idx, F64)
        hi, lo, val = R.branches("hi", R.model_from("hi", s["hi_sd"], s["F"], F64), b, R.HI_HYPER["clip_eps"])
        assert bool(hi[2]) and bool(lo[5]) and bool(val[6]) and bool(val[7]) and not bool(hi[3]) and not bool(lo[4])
        n_avail = b["action_mask"].sum(dim=1)
        assert int(n_avail[0]) == 1 and int(n_avail[1]) == s["Z"]
    stats, s64, s32 = _check_minibatch(zenv_mod, s, "hi", s["hi_sd"], idx, R.HI_HYPER, f"fresh-{case}")
    if batch != "all":                                      # rows as collected: ratio = 1
        adv = _batch(s, "hi", idx, F64)["advantage"]
        R.check_rule(f"fresh-{case}/hi.policy_loss_at_ratio_1", stats[3], -float(adv.mean()), s32["policy_loss"], REPORT)
    assert stats[2] == 0.0


@pytest.mark.parametrize("level,case", [("lo", "tsp"), ("lo", "cm7"), ("hi", "tsp"), ("hi", "cm64")])
def test_gradients_on_the_clipped_branches(zenv_mod, level, case):
    """Perturbed parameters and a narrow clip range: clipped samples of both kinds and their zero gradients."""
    s = _setup(zenv_mod, case)
    sd = R.perturbed(s["sd"][level])
    idx = np.arange(s["total"][level])
    hyper = dict(HYPER[level], clip_eps=RF.PERTURB_CLIP_EPS)
    hi, lo, val = R.branches(level, R.model_from(level, sd, s["F"], F64), _batch(s, level, idx, F64), hyper["clip_eps"])
    print("clipped samples:", int(hi.sum()), int(lo.sum()), int(val.sum()), "of", len(idx))
    assert int(hi.sum()) > 0 and int(lo.sum()) > 0 and int(val.sum()) > 0
    _check_minibatch(zenv_mod, s, level, sd, idx, hyper, f"clipped-{case}")


@pytest.mark.parametrize("level", ["lo", "hi"])
def test_a_repeated_index_adds_its_gradient(zenv_mod, level):
    s = _setup(zenv_mod, "tsp")
    idx = _indexes(s, level, 37, 3)
    idx[5] = idx[0]
    idx[20] = idx[0]
    _check_minibatch(zenv_mod, s, level, s["sd"][level], idx, HYPER[level], "repeat-tsp")


def test_frame_T_minus_1_is_never_read(zenv_mod):
    """NaN in frame T-1 of advantage, returnn, obs and goal: the low level's results are what they were, bit for bit."""
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "cm64")
    env, tenv, N = s["env"], s["tenv"], s["N"]
    idx = np.arange(N * (T - 1), dtype=np.int32)
    _init(s)
    env.hppo_minibatch(0, idx)
    before = (env.hppo_stats(0), env.hppo_tensors(0, nat.PPO_GRAD))
    raw = [tenv._alias(f, shape, np.float32) for f, shape in ((nat.F_EXP_ADVANTAGE, (T, N)), (nat.F_EXP_RETURN, (T, N)),
                                                               (nat.F_EXP_OBS, (T, N, 8)), (nat.F_LO_GOAL, (T, N, 2)))]
    saved = [t[T - 1].clone() for t in raw]
    try:
        for t in raw:
            t[T - 1] = float("nan")
        torch.cuda.synchronize()
        env.hppo_minibatch(0, idx)
        after = (env.hppo_stats(0), env.hppo_tensors(0, nat.PPO_GRAD))
    finally:
        for t, keep in zip(raw, saved):
            t[T - 1] = keep
        torch.cuda.synchronize()
    np.testing.assert_array_equal(before[0], after[0])
    assert np.all(np.isfinite(after[0]))
    for k in before[1]:
        np.testing.assert_array_equal(before[1][k], after[1][k], err_msg=k)
        assert np.all(np.isfinite(after[1][k])), k


def test_a_bad_recorded_goal_is_dropped(zenv_mod):
    """A recorded goal of Z and one marked unavailable: neither row is used -- the statistics and gradients are the
    float64 reference's of the other 31 rows times 31 / 33 (the means still divide by count), under the rule -- and the
    next synchronising call answers ZENV_E_ARG once."""
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "tsp")
    env, hi_t = s["env"], s["hi_t"]
    idx = np.arange(PLANTED, PLANTED + 33, dtype=np.int32)
    keep = np.delete(idx, [2, 3])
    _init(s)
    r_z, r_un = int(idx[2]), int(idx[3])
    saved = (hi_t["action"][r_z].clone(), hi_t["action_mask"][r_un].clone())
    try:
        hi_t["action"][r_z] = s["Z"]
        hi_t["action_mask"][r_un, hi_t["action"][r_un].long()] = False
        torch.cuda.synchronize()
        env.hppo_minibatch(1, idx)
        with pytest.raises(Z.ZenvError) as e:
            env.hppo_stats(1)
        assert e.value.code == Z.E_ARG and "goal" in str(e.value)
        stats = env.hppo_stats(1)[0]                        # reported once
        grads = _by_key(env, "hi", nat.PPO_GRAD)
    finally:
        hi_t["action"][r_z] = saved[0]
        hi_t["action_mask"][r_un] = saved[1]
        torch.cuda.synchronize()
    scale = 31.0 / 33.0
    (g64, s64), (g32, s32) = (R.gradients("hi", R.model_from("hi", s["hi_sd"], s["F"], dt), _batch(s, "hi", keep, dt),
                                          R.HI_HYPER) for dt in (F64, F32))
    for i, name in enumerate(R.STATS):
        R.check_rule(f"dropped/hi.stat.{name}", stats[i], s64[name] * scale, s32[name] * scale, REPORT)
    for key in g64:
        R.check_rule(f"dropped/hi.grad.{key}", grads[key], g64[key].numpy() * scale, g32[key].numpy() * scale, REPORT)


@pytest.mark.parametrize("level", ["lo", "hi"])
@pytest.mark.parametrize("max_grad_norm", [math.inf, 1e-4])
def test_clip_and_adam_from_identical_gradients(zenv_mod, level, max_grad_norm):
    """zenv_hppo_apply on the device's own gradients against the float64 arithmetic and float32 torch Adam, steps 1, 2
    and 10; no clip (the reference's setting: a factor of exactly 1) and a norm far above max_grad_norm."""
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "tsp")
    env, lv = s["env"], LEVELS[level]
    hyper = dict(HYPER[level], max_grad_norm=max_grad_norm)
    _init(s, **{level: dict(max_grad_norm=max_grad_norm)})
    env.hppo_minibatch(lv, np.arange(100 if level == "lo" else s["M"], dtype=np.int32))
    g = env.hppo_tensors(lv, nat.PPO_GRAD)
    names = list(g)
    norm = float(env.hppo_stats(lv)[0][5])
    assert norm > 100 * 1e-4
    p0 = env.hppo_tensors(lv)
    p64 = {n: p0[n].astype(np.float64) for n in names}
    m64 = {n: np.zeros_like(p64[n]) for n in names}
    v64 = {n: np.zeros_like(p64[n]) for n in names}
    coef = 1.0 if math.isinf(max_grad_norm) else RF.clip_coef(R.total_norm([torch.as_tensor(g[n]) for n in names]),
                                                               max_grad_norm)
    params32 = [torch.nn.Parameter(torch.as_tensor(p0[n]).clone()) for n in names]
    opt = torch.optim.Adam(params32, hyper["lr"], eps=hyper["adam_eps"], foreach=False)
    for step in range(1, 11):
        env.hppo_apply(lv)
        for n in names:
            R.adam_step(p64[n], coef * g[n].astype(np.float64), m64[n], v64[n], step, hyper["lr"], hyper["adam_eps"])
        for p, n in zip(params32, names):
            p.grad = torch.as_tensor(g[n]).clone()
        if math.isfinite(max_grad_norm):
            torch.nn.utils.clip_grad_norm_(params32, max_grad_norm, foreach=False)
        opt.step()
        if step in (1, 2, 10):
            assert env.hppo_get_step(lv) == step and env.hppo_get_step(1 - lv) == 0
            dev = {w: env.hppo_tensors(lv, w) for w in (nat.PPO_PARAM, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}
            for p, n in zip(params32, names):
                st = opt.state[p]
                tag = f"adam-{max_grad_norm:g}-step{step}"
                R.check_rule(f"{tag}/{level}.param.{n}", dev[nat.PPO_PARAM][n], p64[n], p.detach().numpy(), REPORT)
                R.check_rule(f"{tag}/{level}.exp_avg.{n}", dev[nat.PPO_EXP_AVG][n], m64[n], st["exp_avg"].numpy(), REPORT)
                R.check_rule(f"{tag}/{level}.exp_avg_sq.{n}", dev[nat.PPO_EXP_AVG_SQ][n], v64[n], st["exp_avg_sq"].numpy(),
                             REPORT)
    np.testing.assert_array_equal(env.hppo_tensors(lv, nat.PPO_GRAD)[names[2]], g[names[2]])   # the arena keeps the gradients


def _arenas(env, lv):
    nat = _nat()
    return {w: env.hppo_tensors(lv, w) for w in (nat.PPO_PARAM, nat.PPO_GRAD, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}


def _nat():
    from combinatorial_rl_tasks_amd import _native
    return _native


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=str(k))


def test_two_handles_from_the_same_state_give_the_same_bytes(zenv_mod):
    a, b = _setup(zenv_mod, "cm64"), _setup(zenv_mod, "cm64", tag="-twin")
    assert a["M"] == b["M"]
    _same(a["hi"], b["hi"])
    out = []
    for s in (a, b):
        _init(s, lo=dict(max_batch=64), hi=dict(max_batch=7))
        env = s["env"]
        rng = np.random.default_rng(4)
        for _ in range(2):
            env.hppo_epoch(1, rng.permutation(s["M"]).astype(np.int32), 7)
            env.hppo_epoch(0, rng.permutation(s["N"] * (T - 1)).astype(np.int32), 64)
        out.append(({lv: _arenas(env, lv) for lv in (0, 1)}, env.hppo_stats(0), env.hppo_stats(1),
                    env.hppo_get_step(0), env.hppo_get_step(1)))
    _same(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])
    assert out[0][3:] == out[1][3:] == (2 * 3, 2 * math.ceil(a["M"] / 7))
    assert out[0][1].shape == (3, 6) and out[0][2].shape == (math.ceil(a["M"] / 7), 6)


@pytest.mark.parametrize("level", ["lo", "hi"])
def test_an_update_leaves_everything_else_alone(zenv_mod, level):
    """One level's epoch: the other level's arenas, the flat learner's, the acting agent and the records, bit for bit."""
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import agents
    s = _setup(Z, "cm64")
    env, lv = s["env"], LEVELS[level]
    _init(s)
    env.ppo_init(RF.random_state_dict(s["F"], s["h"], seed=3), max_batch=16)
    lo_l, hi_l = agents.hier_experience_layout(s["N"], s["Z"], s["F"], T, s["M"])

    def snapshot():
        flat = {w: env.ppo_tensors(w) for w in range(4)}
        return dict(other=_arenas(env, 1 - lv), flat=flat, acting=dict(enumerate(env.hier_forward())),
                    lo=env._download(lo_l), hi=env._download(hi_l), steps=dict(a=np.array([env.hppo_get_step(1 - lv),
                                                                                           env.ppo_get_step()])))
    before = snapshot()
    p0 = env.hppo_tensors(lv)
    env.hppo_epoch(lv, np.arange(s["total"][level], dtype=np.int32), 64)
    assert env.hppo_get_step(lv) == math.ceil(s["total"][level] / 64)
    _same(before, snapshot())
    p1 = env.hppo_tensors(lv)
    assert all(float(np.abs(p1[k] - p0[k]).max()) > 0 for k in p0 if k != "hi_actor_b2")


def test_hppo_update_logs_and_index_order(zenv_mod):
    """hppo_update = the high level's epochs, then the low level's, each in the order of hppo_batch_indexes; the low
    level's logs are the means over all its minibatches, the high level's over the last epoch's."""
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import agents
    s = _setup(Z, "tsp")
    env, M, n_lo = s["env"], s["M"], s["N"] * (T - 1)
    _init(s, lo=dict(max_batch=256), hi=dict(max_batch=32))
    logs = env.hppo_update(2, 256, 2, 32, np.random.default_rng(5))
    assert env.hppo_get_step(1) == 2 * math.ceil(M / 32) and env.hppo_get_step(0) == 2 * 3
    after = {lv: _arenas(env, lv) for lv in (0, 1)}
    _init(s, lo=dict(max_batch=256), hi=dict(max_batch=32))
    rng = np.random.default_rng(5)
    for _ in range(2):
        env.hppo_epoch(1, agents.hppo_batch_indexes(M, rng), 32)
    hi_stats = env.hppo_stats(1)
    lo_stats = []
    for _ in range(2):
        env.hppo_epoch(0, agents.hppo_batch_indexes(n_lo, rng), 256)
        lo_stats.append(env.hppo_stats(0))
    _same(after, {lv: _arenas(env, lv) for lv in (0, 1)})
    assert hi_stats.shape == (math.ceil(M / 32), 6) and lo_stats[0].shape == (3, 6)
    want = {"hi": hi_stats.astype(np.float64).mean(axis=0), "lo": np.concatenate(lo_stats).astype(np.float64).mean(axis=0)}
    assert logs == {f"{lv}_{n}": want[lv][i] for lv in ("hi", "lo") for i, n in enumerate(R.STATS) if n != "value_std"}


def test_two_epochs_of_hppo_update_and_publish(zenv_mod):
    """hppo_update (2 epochs per level) beside the reference learners driven by the same orders, then hppo_publish: the
    published agent's outputs on the handle's current observations under the rule.  The logs of the three runs are
    printed for the record."""
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import agents
    s = _setup(Z, "tsp")
    env, M, n_lo = s["env"], s["M"], s["N"] * (T - 1)
    _init(s, lo=dict(max_batch=256), hi=dict(max_batch=32))
    logs = env.hppo_update(2, 256, 2, 32, np.random.default_rng(21))
    rng = np.random.default_rng(21)
    ref = {dt: {lv: R.RefLearner(lv, s["sd"][lv], s["F"], dt, HYPER[lv]) for lv in ("hi", "lo")} for dt in (F64, F32)}
    for lv, total, size in (("hi", M, 32), ("lo", n_lo, 256)):
        rows = {dt: [] for dt in ref}
        for epoch in range(2):
            order = agents.hppo_batch_indexes(total, rng)
            for dt in ref:
                got = [ref[dt][lv].minibatch(_batch(s, lv, order[at:at + size], dt)) for at in range(0, total, size)]
                rows[dt] = got if lv == "hi" else rows[dt] + got              # hi: the last epoch's; lo: all of them
        m64, m32 = (np.mean(np.array(rows[dt]), axis=0) for dt in (F64, F32))
        for i, name in enumerate(R.STATS):
            if name != "value_std":
                print(f"log {lv}_{name}: device {logs[f'{lv}_{name}']:.9g} float64 {m64[i]:.9g} float32 {m32[i]:.9g}")
    env.hppo_publish()
    logits, hv, mu, std, lv_ = env.hier_forward()
    obs, zone_obs = env.observations()
    _, _, avail, goal = env.goal_info()
    has = goal >= 0
    gxy = zone_obs[np.arange(s["N"]), np.where(has, goal, 0), :2].astype(np.float32)
    nets = {}
    for dt in ref:
        hi_p = {k: v.detach() for k, v in ref[dt]["hi"].model.state_dict().items()}
        lo_p = {k: v.detach() for k, v in ref[dt]["lo"].model.state_dict().items()}
        nets[dt] = H.high(hi_p, obs, zone_obs, avail, dt) + H.low(lo_p, obs, zone_obs, gxy, dt)
    fin = np.isfinite(nets[F64][0])
    assert np.array_equal(np.isfinite(logits), fin)
    R.check_rule("e2e/published.logits", logits[fin], nets[F64][0][fin], nets[F32][0][fin], REPORT)
    R.check_rule("e2e/published.hi_value", hv, nets[F64][1], nets[F32][1], REPORT)
    assert has.any()
    for i, name in ((2, "mu"), (3, "std"), (4, "lo_value")):
        dev = (mu, std, lv_)[i - 2]
        R.check_rule(f"e2e/published.{name}", dev[has], nets[F64][i][has], nets[F32][i][has], REPORT)


def test_torch_arenas_alias_the_learners(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "cm64")
    env, tenv = s["env"], s["tenv"]
    tenv.hppo_init(s["hi_sd"], s["lo_sd"], lo=dict(max_batch=64), hi=dict(max_batch=64))
    hi_sd, lo_sd = tenv.hppo_state_dicts()
    assert set(hi_sd) == set(s["hi_sd"]) and set(lo_sd) == set(s["lo_sd"]) and all(t.is_cuda for t in lo_sd.values())
    for got, want in ((hi_sd, s["hi_sd"]), (lo_sd, s["lo_sd"])):
        for k, v in want.items():
            np.testing.assert_array_equal(got[k].cpu().numpy(), v.numpy())
    for lv, total in ((0, s["N"] * (T - 1)), (1, s["M"])):
        idx = torch.arange(min(64, total), dtype=torch.int32, device=tenv.device)
        tenv.hppo_minibatch(lv, idx, apply=True)
        torch.cuda.synchronize()
        stats = tenv.hppo_stats(lv)
        assert stats.shape == (1, 6) and stats.is_cuda
        arena = tenv.hppo_arenas[lv]["grad"].cpu()           # the aliased arena is what the norm was taken of
        R.check_rule(f"alias/{'lo' if lv == 0 else 'hi'}.stat.grad_norm", float(stats[0, 5].cpu()),
                     float(arena.double().pow(2).sum().sqrt()), float(arena.pow(2).sum().sqrt()), REPORT)
    host_hi, host_lo = env.hppo_state_dicts()
    for got, host in ((hi_sd, host_hi), (lo_sd, host_lo)):         # the views see the step without a copy
        for k in host:
            np.testing.assert_array_equal(got[k].cpu().numpy(), host[k])
    assert float((lo_sd["actor.mu_.weight"].cpu() - s["lo_sd"]["actor.mu_.weight"]).abs().max()) > 0
    assert tenv.hppo_tensors(0, nat.PPO_GRAD)["lo_zone_w1"].shape == (64, 10 + s["F"])
    assert tenv.hppo_tensors(1, nat.PPO_GRAD)["hi_actor_w1"].shape == (64, 64 + s["F"])
    state = tenv.hppo_optimizer_state(1)
    assert len(state["state"]) == 16 and float(state["state"][0]["step"]) == 1.0
    # Adam's state round-trips through the host form
    env.hppo_load_optimizer_state(1, env.hppo_optimizer_state(1))
    assert env.hppo_get_step(1) == 1


def test_refusals(zenv_mod):
    Z = zenv_mod
    s = _setup(Z, "cm7")
    env, M, n_lo = s["env"], s["M"], s["N"] * (T - 1)
    _init(s, lo=dict(max_batch=33), hi=dict(max_batch=9))
    for lv, total, mb in ((0, n_lo, 33), (1, M, 9)):
        ok = np.arange(mb, dtype=np.int32)
        for bad_count in (0, mb + 1):                        # count > max_batch
            with pytest.raises(Z.ZenvError) as e:
                env.hppo_minibatch(lv, np.zeros(bad_count, np.int32))
            assert e.value.code == Z.E_ARG
        for bad in (-1, total, 2 ** 31 - 1):                 # a host index out of range: N (T-1), not N T; M
            idx = ok.copy()
            idx[3] = bad
            with pytest.raises(Z.ZenvError) as e:
                env.hppo_minibatch(lv, idx)
            assert e.value.code == Z.E_ARG
        with pytest.raises(Z.ZenvError) as e:
            env.hppo_epoch(lv, ok, mb + 1)
        assert e.value.code == Z.E_ARG
        idx = ok.copy()
        idx[3] = total - 1
        env.hppo_minibatch(lv, idx)
        assert np.all(np.isfinite(env.hppo_stats(lv)))
    for lv in (2, -1):
        with pytest.raises(Z.ZenvError) as e:
            env.hppo_apply(lv)
        assert e.value.code == Z.E_ARG
    # device-resident indexes far outside the buffers: only the guard keeps them from being read
    dev = torch.device("cuda", env.device)
    for lv, total in ((0, n_lo), (1, M)):
        idx = torch.arange(9, dtype=torch.int32, device=dev)
        idx[2] = 2 ** 31 - 1
        idx[5] = -(2 ** 31)
        idx[7] = total                                       # the first index past the end (frame T-1's for the low level)
        torch.cuda.synchronize()
        env.hppo_minibatch(lv, idx.data_ptr(), count=9)
        with pytest.raises(Z.ZenvError) as e:
            env.hppo_stats(lv)
        assert e.value.code == Z.E_ARG
        stats = env.hppo_stats(lv)                           # reported once
        assert stats.shape == (1, 6) and np.all(np.isfinite(stats))
        assert all(np.all(np.isfinite(g)) for g in env.hppo_tensors(lv, Z._native.PPO_GRAD).values())
    # ---- call order, on handles of their own
    hi_sd, lo_sd = s["hi_sd"], s["lo_sd"]
    one = np.zeros(1, np.int32)

    def refused(env, code=Z.E_STATE):
        for call in (lambda: env.hppo_minibatch(0, one), lambda: env.hppo_minibatch(1, one),
                     lambda: env.hppo_epoch(0, one, 1), lambda: env.hppo_epoch(1, one, 1)):
            with pytest.raises(Z.ZenvError) as e:
                call()
            assert e.value.code == code

    cfg = Z.config_for_id("ColourMatch-v0", num_steps=12)
    goal = Z.ZoneVecEnv(cfg, 2)
    plain = Z.ZoneVecEnv(cfg, 2)
    try:
        for e in (goal, plain):
            e.build_bank(1, 2)
            e.schedule_sequential()
        goal.enable_goals()
        goal.reset()
        plain.reset()
        refused(goal)                                        # no hppo_init
        with pytest.raises(Z.ZenvError) as e:
            goal.hppo_apply(0)
        assert e.value.code == Z.E_STATE
        goal.hppo_init(hi_sd, lo_sd, lo=dict(max_batch=8), hi=dict(max_batch=8))
        refused(goal)                                        # no collect_hier
        goal.load_hier(Z.hier_tensors_from_state_dicts(hi_sd, lo_sd))
        goal.collect_hier(2, policy_seed=1)                  # the first 2 frames of an episode: nothing closes
        assert goal.field_bytes(Z.F_HI_VALUE) == 0
        goal.hppo_minibatch(0, one)                          # the low level has its one frame per env ...
        with pytest.raises(Z.ZenvError) as e:
            goal.hppo_minibatch(1, one)                      # ... the high level no row: M = 0
        assert e.value.code == Z.E_STATE
        logs = goal.hppo_update(1, 8, 1, 8, np.random.default_rng(0))
        assert logs["hi_policy_loss"] == 0.0 and logs["hi_grad_norm"] == 0.0 and goal.hppo_get_step(1) == 0
        assert goal.hppo_get_step(0) == 1 and logs["lo_grad_norm"] > 0
        goal.collect_hier(T, policy_seed=1)
        goal.hppo_minibatch(1, one)
        from tests import ppo_update_ref as flat_ref
        goal.load_mlp(Z.mlp_tensors_from_state_dict(flat_ref.random_state_dict(goal.zone_feat, 7)), precision="f32")
        goal.collect(4, policy_seed=1)
        refused(goal)                                        # the last collector was collect
        goal.collect_hier(T, policy_seed=2)
        goal.hppo_minibatch(0, one)
        # a skill handle: collect_skills fills the same ZENV_F_HI_* / ZENV_F_EXP_* buffers with its own records
        from tests import skill_ref
        S = 3
        plain.load_skills(Z.skill_tensors_from_state_dicts(*skill_ref.random_state_dicts(plain.zone_feat, S, h=7)),
                          skill_len=2)
        plain.collect_skills(4, policy_seed=1)
        plain.hppo_init(hi_sd, lo_sd, lo=dict(max_batch=8), hi=dict(max_batch=8))
        refused(plain)                                       # the last collector was collect_skills
    finally:
        goal.close()
        plain.close()
