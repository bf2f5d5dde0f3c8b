"""The device agents on what the reference's own code made and computed (tests/golden/agent_*.npz, recorded by
tests/golden/make_agent_goldens.py): state_dicts exactly as the reference's modules emit them, through the project's
loaders into the device forwards of all five agents and the inverse model at 70 envs, and every device learner -- the
flat one with the plain and with the distributional critic, both levels of the Zone-goals, xy-goals, fixed-length-skills
and Options agents, DIAYN's inverse model and its skill prior -- on the reference's own experience, index lists and
hyper-parameters against what the reference's own update functions computed.  Small shapes only: N <= 70, T <= 33,
h = 32.  The forwards are held to the tolerances of the existing forward tests (1e-5 of max(1, |ref|), check_rule for
the flat agent) against the restatements tests/test_agent_goldens_cpu.py pins.

The learners (second half of this file).  The recorded exp/* rows are planted through TorchZoneEnv's aliases of a real
collection's buffers, fixture row i at the learner's own sample index i (the map is the *_update_ref batch functions',
and the batch they read back must be the fixture's rows), and read back bit for bit.  Every comparison is
ppo_update_ref.check_rule with the reference's float64 run as the truth and its float32 run as the ruler:
  one minibatch, apply = 0, index0   the statistics; every gradient of at most 256 elements against the recorded one;
                                     every larger one by its sketch [G v, u^T G] against the recorded sketch (or in
                                     full where the fixture has it) and element by element against the restatement's
                                     gradients on the same batch, which the CPU file pins to the same sketch
  index0 then index1 with Adam       both minibatches' statistics and the recorded (small) tensors' exp_avg, exp_avg_sq
                                     and param; for the flat learner the clip is active (factor < 1)
  the skill prior                    two diayn_prior_update steps on the recorded picks: logits and probabilities"""
import math
import types

import numpy as np
import pytest
import torch

from tests import hier_ref, option_ref, ppo_update_dev as D, ppo_update_ref as R, skill_collect_ref, skill_ref, xy_ref
from tests import diayn_update_dev as DD, opppo_update_dev as DO, skppo_update_dev as DS, xyppo_update_dev as DX
from tests import diayn_update_ref as RD, hppo_update_ref as RH, opppo_update_ref as RO, skppo_update_ref as RS
from tests import xyppo_update_ref as RX
from tests.agent_goldens import SMALL, hier_hyper, load, sketch, sub

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
N_FORWARD = 70


def _close(what, got, ref, rel=True):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got)), what
    err = np.abs(got[fin] - ref[fin])
    tol = 1e-5 * (np.maximum(1.0, np.abs(ref[fin])) if rel else 1.0)
    print(f"{what}: max |dev - ref| = {float(err.max(initial=0)):.3g}")
    assert np.all(err <= tol), (what, float(err.max()))


def _env(Z, env_id, goals=False, **over):
    env = Z.ZoneVecEnv(Z.config_for_id(env_id, **over), N_FORWARD)
    env.build_bank(11, N_FORWARD)
    env.schedule_sequential()
    if goals:
        env.enable_goals()
    env.reset()
    return env


@pytest.mark.parametrize("tag,env_id", [("plain", "PointTSP-v0"), ("dist", "ColourMatch-v0")])
def test_flat_loader_and_forward(zenv_mod, tag, env_id):
    """The reference-made ACModel state_dict (zero-initialised biases randomised, every key it emits) through
    mlp_tensors_from_state_dict / load_mlp; the forward on the handle's own observations after a few steps."""
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import agents
    sd = sub(load("main", "networks"), f"flat_{tag}/sd/")
    env = Z.ZoneVecEnv(Z.config_for_id(env_id), N_FORWARD)
    env.build_bank(11, 2 * N_FORWARD)
    env.reset()
    assert env.zone_feat == sd["env_model.zone_net_.0.weight"].shape[1] - 8
    env.load_mlp(agents.mlp_tensors_from_state_dict(sd), precision="f32")
    env.collect(3, policy_seed=5)
    out = env.mlp_forward(with_value=True)
    obs, zone_obs = env.get(Z.F_OBS), env.get(Z.F_ZONE_OBS)
    nets = {}
    for dt in (F64, F32):
        with torch.no_grad():
            nets[dt] = R.model_from(sd, env.zone_feat, dt)(torch.as_tensor(obs).to(dt), torch.as_tensor(zone_obs).to(dt))
    for i, name in enumerate(("mu", "std", "value") + (("value_sigma",) if tag == "dist" else ())):
        R.check_rule(f"golden-flat-{tag}/{name}", out[i], nets[F64][i].numpy(), nets[F32][i].numpy())
    env.close()


def test_zone_goals_loader_and_forward(zenv_mod):
    """HighPolicyValueModel / LoPolicyValueModel state_dicts through hier_tensors_from_state_dicts / load_hier; both
    networks after a few sampled steps, the goals being zone centres / 3."""
    Z = zenv_mod
    rec = sub(load("zone-goals", "networks"), "zone_goals/")
    hi, lo = sub(rec, "hi_sd/"), sub(rec, "lo_sd/")
    env = _env(Z, "PointTSP-v0", goals=True, num_steps=150)
    env.load_hier(Z.hier_tensors_from_state_dicts(hi, lo))
    for t in range(4):
        env.policy(Z.POLICY_HIER_SAMPLE, policy_seed=7)
        if t < 3:
            env.step(None, auto_reset=True)
    logits, hv, mu, std, lv = env.hier_forward()
    o, zo = env.observations()
    _, _, avail, goal = env.goal_info()
    rl, rhv = hier_ref.high(hi, o, zo, avail)
    _close("zone-goals logits", logits, rl)
    _close("zone-goals hi value", hv, rhv)
    has = goal >= 0
    assert has.sum() > N_FORWARD // 2
    xy = zo[np.arange(N_FORWARD), np.where(has, goal, 0), :2].astype(np.float32)
    rmu, rstd, rlv = hier_ref.low(lo, o, zo, xy)
    _close("zone-goals mu", mu[has], rmu[has], rel=False)
    _close("zone-goals std", std[has], rstd[has], rel=False)
    _close("zone-goals lo value", lv[has], rlv[has])
    env.close()


def test_xy_goals_loader_and_forward(zenv_mod):
    Z = zenv_mod
    rec = sub(load("xy-goals", "networks"), "xy_goals/")
    hi, lo = sub(rec, "hi_sd/"), sub(rec, "lo_sd/")
    env = _env(Z, "ColourMatch-v0", num_steps=150)
    env.load_xy(Z.xy_tensors_from_state_dicts(hi, lo), skill_len=4)
    for t in range(3):
        env.policy(Z.POLICY_XY_SAMPLE, policy_seed=7)
        env.step(None, auto_reset=True)
    gmu, gstd, hv, mu, std, lv = env.xy_forward()
    o, zo = env.observations()
    goal, age = env.get(Z.F_XY_GOAL), env.get(Z.F_XY_GOAL_AGE)
    rgmu, rgstd, rhv = xy_ref.high(hi, o, zo)
    _close("xy goal_mu", gmu, rgmu)
    _close("xy goal_std", gstd, rgstd)
    _close("xy hi value", hv, rhv)
    has = age >= 0
    assert has.sum() > N_FORWARD // 2
    rmu, rstd, rlv = xy_ref.low(lo, o, zo, np.where(has[:, None], goal, 0).astype(np.float32))
    _close("xy mu", mu[has], rmu[has])
    _close("xy std", std[has], rstd[has])
    _close("xy lo value", lv[has], rlv[has])
    env.close()


@pytest.mark.parametrize("agent", ["skills", "options"])
def test_skill_family_loader_and_forward(zenv_mod, agent):
    Z = zenv_mod
    rec = sub(load("main", "skill_networks") if agent == "skills" else load("options", "networks"), f"{agent}/")
    hi, lo, S = sub(rec, "hi_sd/"), sub(rec, "lo_sd/"), int(rec["in/n_skills"])
    env = _env(Z, "PointTSP-v0" if agent == "skills" else "ColourMatch-v0", num_steps=150)
    if agent == "skills":
        env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo), skill_len=4)
        policy, ref = Z.POLICY_SKILL_SAMPLE, skill_ref
    else:
        env.load_options(Z.option_tensors_from_state_dicts(hi, lo))
        policy, ref = Z.POLICY_OPTION_SAMPLE, option_ref
    for t in range(3):
        env.policy(policy, policy_seed=7)
        env.step(None, auto_reset=True)
    out = env.skill_forward() if agent == "skills" else env.option_forward()
    logits, hv, mu, std, lv = out[:5]
    o, zo = env.observations()
    skill = env.get(Z.F_SKILL)
    rl, rhv = ref.high(hi, o, zo)
    _close(f"{agent} logits", logits, rl)
    _close(f"{agent} hi value", hv, rhv)
    has = skill >= 0
    assert has.sum() > 0
    rmu, rstd, rlv = ref.low(lo, o, zo, np.where(has, skill, 0), S)
    if agent == "options":
        mu, std = np.concatenate([mu, out[5][:, None]], axis=1), np.concatenate([std, out[6][:, None]], axis=1)
    _close(f"{agent} mu", mu[has], rmu[has], rel=False)
    _close(f"{agent} std", std[has], rstd[has], rel=False)
    _close(f"{agent} lo value", lv[has], rlv[has])
    env.close()


def test_inverse_loader_and_forward(zenv_mod):
    """InverseModel's state_dict through inverse_tensors_from_state_dict / load_skill_inverse: the diversity reward of
    one collect_skills, log q(skill | next obs) - log p(skill), on the frames whose next observation is the next
    recorded one (no window end in between) and whose episode goes on."""
    Z = zenv_mod
    nets = load("main", "skill_networks")
    hi, lo, inv = sub(nets, "skills/hi_sd/"), sub(nets, "skills/lo_sd/"), sub(nets, "inverse/sd/")
    S, L, T = int(nets["inverse/in/n_skills"]), 4, 8
    env = _env(Z, "PointTSP-v0", num_steps=150)
    env.load_skills(Z.skill_tensors_from_state_dicts(hi, lo), skill_len=L)
    env.load_skill_inverse(Z.inverse_tensors_from_state_dict(inv, S))
    prior = np.linspace(-0.5, 0.5, S).astype(np.float32)
    lo_e, _, _, _ = env.collect_skills(T, policy_seed=3, diversity_coef=0.1, skill_prior_logits=prior)
    lp_prior = torch.log_softmax(torch.as_tensor(prior, dtype=F64), dim=0).numpy()
    checked = 0
    for t in range(T - 1):
        if (t + 1) % L == 0:
            continue
        keep = lo_e["mask"][:, t + 1] != 0                       # not done at frame t
        q = skill_collect_ref.inverse_log_softmax(inv, lo_e["obs"][:, t + 1], lo_e["zone_obs"][:, t + 1])
        sk = lo_e["skill"][:, t]
        want = q[np.arange(N_FORWARD), sk] - lp_prior[sk]
        _close(f"diversity frame {t}", lo_e["diversity"][keep, t], want[keep])
        checked += int(keep.sum())
    assert checked > N_FORWARD
    env.close()


def test_flat_learner_on_the_reference_batch(zenv_mod):
    """One ppo_minibatch (apply = 0) on the reference's recorded experience and its first index list: the statistics
    and every gradient tensor against what the reference's own update_parameters computed, float64 as the truth and
    float32 as the ruler.  The recorder read .grad after clip_grad_norm_ (ppo.py:122); the device's gradient arena holds
    the unclipped ones, so the recorded gradients are divided by the clip's factor min(1, max_norm / (norm + 1e-6))."""
    Z = zenv_mod
    nat = Z._native
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    rec = sub(load("main", "flat_update"), "flat_plain_update/")
    sd = sub(load("main", "networks"), "flat_plain/sd/")
    e, h = sub(rec, "exp/"), sub(rec, "hyper/")
    N, T = (int(v) for v in rec["shape/NT"])
    hyper = {k: float(h[k]) for k in ("lr", "adam_eps", "clip_eps", "entropy_coef", "value_loss_coef", "max_grad_norm")}
    s = D.flat_setup(Z, Z.config_for_id("PointTSP-v0"), 32, N, T, False, seed=0, sd=sd)
    env = s["env"]
    assert (env.num_zones, env.zone_feat) == e["zone_obs"].shape[1:]
    tenv = TorchZoneEnv(env)
    exps = tenv.collect(T, policy_seed=5)                   # [N, T, ...] views aliasing the handle's buffers
    for k in ("obs", "zone_obs", "action", "log_prob", "value", "advantage", "returnn"):
        a = e[k].reshape((N, T) + e[k].shape[1:])           # the reference's rows are [env][frame]
        assert tuple(exps[k].shape) == a.shape, k
        exps[k].copy_(torch.as_tensor(a).to(exps[k].device))
    torch.cuda.synchronize()
    env.ppo_init(sd, max_batch=N * T, **hyper)
    idx = rec["index0"].astype(np.int32)
    env.ppo_minibatch(idx)
    stats = env.ppo_stats()[0]
    grads = D.flat_by_key(env, nat.PPO_GRAD)
    want64, want32 = sub(rec, "f64/grad/"), sub(rec, "f32/grad/")
    assert set(grads) == set(want64) == set(want32) and len(grads) == 18
    coef = {p: R.clip_coef(float(rec[f"{p}/log/grad_norm"][0]), hyper["max_grad_norm"]) for p in ("f64", "f32")}
    assert coef["f64"] < 1.0
    for i, name in enumerate(R.STATS):
        if name != "value_std":
            R.check_rule(f"golden-flat/stat.{name}", stats[i], rec[f"f64/log/{name}"][0], rec[f"f32/log/{name}"][0])
    for key in want64:
        R.check_rule(f"golden-flat/grad.{key}", grads[key], want64[key] / coef["f64"], want32[key] / coef["f32"])
    env.close()


@pytest.mark.parametrize("level", ["lo", "hi"])
def test_zone_goals_learner_on_the_reference_batch(zenv_mod, level):
    """One hppo_minibatch (apply = 0) of a level on the reference's recorded experience and first index list against
    the reference's own recorded gradients (no clip at either level).  The low level's handle has the fixture's N and T;
    the high level's rows exist only where a collection wrote them, so its handle is one whose collection closes at
    least the fixture's M transitions (15 envs, 33 frames, 12-step episodes), and only those first M rows are used."""
    Z = zenv_mod
    nat = Z._native
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    rec = sub(load("zone-goals", f"{level}_update"), f"zone_goals_{level}_update/")
    nets = sub(load("zone-goals", "networks"), "zone_goals/")
    sd = {"hi": sub(nets, "hi_sd/"), "lo": sub(nets, "lo_sd/")}
    e, h = sub(rec, "exp/"), sub(rec, "hyper/")
    N, T = (int(v) for v in rec["shape/NT"]) if level == "lo" else (15, 33)
    env = Z.ZoneVecEnv(Z.config_for_id("PointTSP-v0", num_steps=12), N)
    env.build_bank(11, N)
    env.schedule_sequential()
    env.enable_goals()
    env.reset()
    assert (env.num_zones, env.zone_feat) == e["zone_obs"].shape[1:]
    env.load_hier(Z.hier_tensors_from_state_dicts(sd["hi"], sd["lo"]))
    tenv = TorchZoneEnv(env)
    lo_t, hi_t = tenv.collect_hier(T, policy_seed=5)
    dev = tenv.device
    if level == "lo":
        n = N * (T - 1)
        for k in ("obs", "zone_obs", "goal", "action", "log_prob", "value", "advantage", "returnn"):
            a = e[k].reshape((N, T - 1) + e[k].shape[1:])
            assert tuple(lo_t[k].shape) == a.shape, k
            lo_t[k].copy_(torch.as_tensor(a).to(dev))
    else:
        n = len(e["action"])
        assert int(hi_t["value"].shape[0]) >= n
        for k in ("obs", "zone_obs", "value", "log_prob", "advantage", "returnn"):
            hi_t[k][:n] = torch.as_tensor(e[k]).to(dev)
        hi_t["action"][:n] = torch.as_tensor(e["action"].astype(np.int32)).to(dev)
        hi_t["action_mask"][:n] = torch.as_tensor(e["action_mask"]).to(dev)
    torch.cuda.synchronize()
    pre = "hi_" if level == "hi" else ""
    over = dict(clip_eps=float(h["clip_eps"]), entropy_coef=float(h[pre + "entropy_coef"]),
                value_loss_coef=float(h["hi_value_coef" if level == "hi" else "value_loss_coef"]))
    big = dict(max_batch=max(N * (T - 1), int(hi_t["value"].shape[0])))
    env.hppo_init(sd["hi"], sd["lo"], lo=dict(big, **(over if level == "lo" else {})),
                  hi=dict(big, **(over if level == "hi" else {})))
    idx = rec["index0"].astype(np.int32)
    assert idx.max() < n
    env.hppo_minibatch(D.LEVELS[level], idx)
    stats = env.hppo_stats(D.LEVELS[level])[0]
    grads = D.hier_by_key(env, level, nat.PPO_GRAD)
    want64, want32 = sub(rec, "f64/grad/"), sub(rec, "f32/grad/")
    assert set(grads) == set(want64) == set(want32) and len(grads) == (16 if level == "hi" else 18)
    for i, name in enumerate(RH.STATS):
        if name != "value_std":
            R.check_rule(f"golden-zg-{level}/stat.{name}", stats[i], rec[f"f64/log/{name}"][0], rec[f"f32/log/{name}"][0])
    for key in want64:
        R.check_rule(f"golden-zg-{level}/grad.{key}", grads[key], want64[key], want32[key])
    env.close()


# ------------------------------------------------------------------------------------------------ every device learner
# learner -> (variant, the update's fixture, the networks' fixture, the networks' prefix, family, level)
SOURCES = {"flat_plain": ("main", "flat_update", "networks", "flat_plain/", "flat", None),
           "flat_dist": ("main", "flat_update", "networks", "flat_dist/", "flat", None),
           "zone_goals_hi": ("zone-goals", "hi_update", "networks", "zone_goals/", "zg", "hi"),
           "zone_goals_lo": ("zone-goals", "lo_update", "networks", "zone_goals/", "zg", "lo"),
           "xy_goals_hi": ("xy-goals", "updates", "networks", "xy_goals/", "xy", "hi"),
           "xy_goals_lo": ("xy-goals", "updates", "networks", "xy_goals/", "xy", "lo"),
           "skills_hi": ("main", "skill_updates", "skill_networks", "skills/", "sk", "hi"),
           "skills_lo": ("main", "skill_updates", "skill_networks", "skills/", "sk", "lo"),
           "options_hi": ("options", "updates", "networks", "options/", "op", "hi"),
           "options_lo": ("options", "updates", "networks", "options/", "op", "lo"),
           "inverse": ("main", "skill_updates", "skill_networks", "inverse/", "inv", None)}
NEW_LEARNERS = ["flat_dist", "xy_goals_hi", "xy_goals_lo", "skills_hi", "skills_lo", "options_hi", "options_lo", "inverse"]
# family -> (the restatement, the prefix of the handle's methods, name -> tensors by state_dict key, the task)
FAMILIES = {"zg": (RH, "hppo", D.hier_by_key, "PointTSP-v0"), "xy": (RX, "xyppo", DX.xy_by_key, "ColourMatch-v0"),
            "sk": (RS, "skppo", DS.sk_by_key, "PointTSP-v0"), "op": (RO, "opppo", DO.op_by_key, "ColourMatch-v0")}
H_DIM, N_SKILLS = 32, 5
UPD_N, UPD_T, UPD_L = 6, 8, 2                       # 48 low rows; with skill_len 2, 24 high rows
OP_T = UPD_T + 1                                    # the Options collector's low rows are frames 0 .. T - 2
INV_N, INV_T = 8, 6                                 # 8 x (6 - 1) = 40 inverse samples, one window per collection
ZG_HI_NT = (15, 33)                                 # a collection that closes at least the fixture's 30 transitions
_HANDLES = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _learner_teardown():
    yield
    for s in _HANDLES.values():
        s["env"].close()
    worst = {}
    for name, e_dev, e32, ratio in REPORT:
        key = name.split("/")[0]
        worst[key] = max(worst.get(key, (0.0, "")), (ratio, name))
    for k in sorted(worst):
        print("worst e_dev / max(e32, ulp): %-28s %.3f  (%s)" % (k, worst[k][0], worst[k][1]))


def _rule(failures, name, dev, ref64, ref32):
    """check_rule; a miss is kept for the end of the test, so that one run shows every figure."""
    try:
        return R.check_rule(name, dev, ref64, ref32, REPORT)
    except AssertionError as err:
        failures.append(str(err))
        return math.inf


def _handle(Z, key, sds=None):
    """One handle per family, with one real collection of the shape the fixtures need; its buffers are planted by every
    learner that uses it."""
    if key in _HANDLES:
        return _HANDLES[key]
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    tsp, cm = (Z.config_for_id(i, num_steps=12) for i in ("PointTSP-v0", "ColourMatch-v0"))
    if key == "xy":
        s = DX.xy_setup(Z, cm, H_DIM, UPD_N, seed=0, T=UPD_T, L=UPD_L)
    elif key == "sk":
        s = DS.sk_setup(Z, tsp, H_DIM, UPD_N, N_SKILLS, seed=0, T=UPD_T, L=UPD_L)
    elif key == "op":
        s = DO.op_setup(Z, cm, H_DIM, UPD_N, N_SKILLS, seed=0, T=OP_T, want_m=lambda m: m >= 24)
    elif key == "inv":
        s = DD.dy_setup(Z, tsp, H_DIM, INV_N, N_SKILLS, seed=0, T=INV_T, L=INV_T, plant=False)
    elif key in ("flat_plain", "flat_dist"):
        dist = key == "flat_dist"
        s = D.flat_setup(Z, Z.config_for_id("ColourMatch-v0" if dist else "PointTSP-v0"), H_DIM, UPD_N, UPD_T, dist,
                         seed=0, sd=sds)
        s["tenv"] = TorchZoneEnv(s["env"])
        s["lo_t"] = s["tenv"].collect(UPD_T, policy_seed=5)     # [N, T, ...] views aliasing the handle's buffers
    else:                                                        # "zg_lo", "zg_hi": see the Zone-goals test above
        N, T = (UPD_N, UPD_T + 1) if key == "zg_lo" else ZG_HI_NT
        env = Z.ZoneVecEnv(tsp, N)
        env.build_bank(11, N)
        env.schedule_sequential()
        env.enable_goals()
        env.reset()
        env.load_hier(Z.hier_tensors_from_state_dicts(*sds))
        tenv = TorchZoneEnv(env)
        lo_t, hi_t = tenv.collect_hier(T, policy_seed=5)
        s = dict(env=env, tenv=tenv, lo_t=lo_t, hi_t=hi_t, N=N, T=T)
    _HANDLES[key] = s
    return s


def _plant(views, arrays):
    """Write arrays (name -> host array in the view's shape and dtype) through the aliases, then read the buffers back:
    bit for bit what was written."""
    for k, a in arrays.items():
        assert tuple(views[k].shape) == a.shape, (k, tuple(views[k].shape), a.shape)
        views[k].copy_(torch.as_tensor(np.ascontiguousarray(a)).to(views[k].device))
    torch.cuda.synchronize()
    for k, a in arrays.items():
        got = np.ascontiguousarray(views[k].cpu().numpy())
        assert got.dtype == a.dtype and got.tobytes() == np.ascontiguousarray(a).tobytes(), k


def _rows(e, shape):
    """The fixture's rows [n, ...] as the collectors' [N, frames, ...]; integers as the device holds them."""
    return {k: (a.astype(np.int32) if a.dtype == np.int64 else a).reshape(shape + a.shape[1:]) for k, a in e.items()}


def _learner(Z, name):
    """The device learner `name` on a handle whose buffers hold the reference's recorded experience: the recorded rows
    planted and read back, and what the two checks below need of it."""
    nat = Z._native
    variant, part, net_part, net_prefix, family, level = SOURCES[name]
    rec = sub(load(variant, part), f"{name}_update/")
    nets = sub(load(variant, net_part), net_prefix)
    e, h = sub(rec, "exp/"), sub(rec, "hyper/")
    n = len(e["obs"])
    for k, v in sub(rec, "count/").items():
        assert v > 0, (name, k)
    L = types.SimpleNamespace(name=name, rec=rec, e=e, n=n, clip=None)
    if family == "flat":
        sd = sub(nets, "sd/")
        s = _handle(Z, name, sd)
        env, dist = s["env"], name == "flat_dist"
        hyper = {k: float(h[k]) for k in ("lr", "adam_eps", "clip_eps", "entropy_coef", "value_loss_coef", "max_grad_norm")}
        assert (UPD_N, UPD_T) == tuple(int(v) for v in rec["shape/NT"])
        _plant(s["lo_t"], _rows(e, (UPD_N, UPD_T)))             # the reference's rows are [env][frame]
        L.init = lambda: env.ppo_init(sd, max_batch=n, **hyper)
        L.minibatch, L.stats, L.step = env.ppo_minibatch, env.ppo_stats, env.ppo_get_step
        L.tensors = lambda which: D.flat_by_key(env, which)
        L.batch = lambda idx, dt: R.as_batch(D.host(s["lo_t"]), idx, dt)
        L.ref = lambda b, dt: R.gradients(R.model_from(sd, e["zone_obs"].shape[2], dt), b, hyper)
        L.columns = [(i, k) for i, k in enumerate(nat.PPO_STATS) if dist or k != "value_std"]
        L.n_keys = 20 if dist else 18
        L.clip = {p: R.clip_coef(float(rec[f"{p}/log/grad_norm"][0]), hyper["max_grad_norm"]) for p in ("f64", "f32")}
        assert L.clip["f64"] < 1.0 and L.clip["f32"] < 1.0       # the reference's clip was active
    elif family == "inv":
        sd = sub(nets, "sd/")
        s = _handle(Z, "inv")
        env, T1 = s["env"], INV_T - 1
        assert n == INV_N * T1
        lo_t = s["lo_t"]
        rows = _rows(e, (INV_N, T1))
        # sample (env, f) pairs the observation of frame f + 1 with the skill of frame f (diayn_update_ref.batch), and is
        # kept where the mask of frame f + 1 is not 0 (kept_samples): all 40 are
        views = {"obs": lo_t["obs"][:, 1:], "zone_obs": lo_t["zone_obs"][:, 1:], "skill": lo_t["skill"][:, :-1],
                 "mask": lo_t["mask"][:, 1:]}
        _plant(views, dict(rows, mask=np.ones((INV_N, T1), np.float32)))
        np.testing.assert_array_equal(RD.kept_samples(D.host(lo_t)["mask"]), np.arange(n))
        np.testing.assert_array_equal(env.diayn_samples(), np.arange(n))
        hyper = dict(lr=float(h["lr"]), adam_eps=float(h["optim_eps"]))
        L.init = lambda: env.diayn_init(sd, N_SKILLS, max_batch=n, **hyper)
        L.minibatch, L.stats, L.step = env.diayn_minibatch, env.diayn_stats, env.diayn_get_step
        L.tensors = lambda which: DD.dy_by_key(env, which)
        L.batch = lambda idx, dt: RD.batch(D.host(lo_t), idx, dt)
        L.ref = lambda b, dt: RD.gradients(RD.model_from(sd, e["zone_obs"].shape[2], dt), b)
        L.columns = [(0, "loss")]
        L.n_keys = 10
    else:
        RM, prefix, by_key, _ = FAMILIES[family]
        sds = {"hi": sub(nets, "hi_sd/"), "lo": sub(nets, "lo_sd/")}
        s = _handle(Z, family if family != "zg" else f"zg_{level}", (sds["hi"], sds["lo"]))
        env, lv = s["env"], D.LEVELS[level]
        if level == "lo":
            frames = n // UPD_N
            rows = _rows(e, (UPD_N, frames))
            if family == "op":                                   # the third component has buffers of its own
                rows["term_action"], rows["action"] = rows["action"][..., 2], rows["action"][..., :2]
                rows["term_log_prob"], rows["log_prob"] = rows["log_prob"][..., 2], rows["log_prob"][..., :2]
            _plant(s["lo_t"], rows)
            L.batch = lambda idx, dt: RM.lo_batch(D.host(s["lo_t"]), idx, dt)
        else:
            rows = _rows(e, (n,))
            assert int(s["hi_t"]["value"].shape[0]) >= n
            _plant({k: s["hi_t"][k][:n] for k in rows}, rows)
            L.batch = lambda idx, dt: RM.hi_batch({k: v for k, v in D.host(s["hi_t"]).items() if k != "count"}, idx, dt)
        hyper = hier_hyper(h, level)
        mine = dict({k: v for k, v in hyper.items() if k != "max_grad_norm"}, max_batch=64)   # no clip: the default
        other = dict(max_batch=64)
        L.init = lambda: getattr(env, prefix + "_init")(sds["hi"], sds["lo"], lo=mine if level == "lo" else other,
                                                         hi=mine if level == "hi" else other)
        L.minibatch = lambda idx, apply=False: getattr(env, prefix + "_minibatch")(lv, idx, apply)
        L.stats = lambda: getattr(env, prefix + "_stats")(lv)
        L.step = lambda: getattr(env, prefix + "_get_step")(lv)
        L.tensors = lambda which: by_key(env, level, which)
        L.ref = lambda b, dt: RM.gradients(level, RM.model_from(level, sds[level], e["zone_obs"].shape[2], dt), b, hyper)
        L.columns = [(i, k) for i, k in enumerate(nat.PPO_STATS) if k != "value_std"]
        L.n_keys = 18 if level == "lo" or family == "xy" else 16
    assert (env.num_zones, env.zone_feat) == e["zone_obs"].shape[1:]
    # the project's own index -> (env, frame) map reads the fixture's row i at sample index i
    b = L.batch(np.arange(n), F32)
    for k, a in e.items():
        np.testing.assert_array_equal(b[k].numpy(), a, err_msg=f"{name}: {k}")
    assert max(int(rec["index0"].max()), int(rec["index1"].max())) < n
    return L


def _stats_rule(failures, L, tag, row, i):
    """A statistics row against the reference's i-th minibatch."""
    for col, k in L.columns:
        _rule(failures, f"{tag}/stat{i}.{k}", row[col], L.rec[f"f64/log/{k}"][i], L.rec[f"f32/log/{k}"][i])
    if (2, "value_std") not in L.columns and L.name != "inverse":
        assert row[2] == 0.0


def _check_first_minibatch(Z, name):
    """One minibatch (apply = 0) on the reference's first index list."""
    nat = Z._native
    L = _learner(Z, name)
    rec, tag, failures = L.rec, f"golden-{name}", []
    L.init()
    L.minibatch(rec["index0"].astype(np.int32))
    stats, grads = L.stats()[0], L.tensors(nat.PPO_GRAD)
    ref = {p: L.ref(L.batch(rec["index0"], dt), dt) for p, dt in (("f64", F64), ("f32", F32))}
    full, sketched = sub(rec, "f64/grad/"), sub(rec, "f64/sketch/")
    assert set(grads) == set(ref["f64"][0]) == set(full) | set(sketched) and len(grads) == L.n_keys
    assert set(full) == set(sub(rec, "f32/grad/")) and set(sketched) == set(sub(rec, "f32/sketch/"))
    _stats_rule(failures, L, tag, stats, 0)
    if name == "inverse":                                       # the reference logs no norm here: the restatement's
        _rule(failures, f"{tag}/stat0.grad_norm", stats[5], ref["f64"][1]["grad_norm"], ref["f32"][1]["grad_norm"])
        assert np.all(stats[1:5] == 0)
    # the recorder read .grad after the flat learner's clip; the device's gradient arena holds the unclipped ones
    c64, c32 = (L.clip["f64"], L.clip["f32"]) if L.clip else (1.0, 1.0)
    large = 0
    for key, g in grads.items():
        assert g.shape == tuple(ref["f64"][0][key].shape), key
        if key in full:
            assert g.size <= SMALL or name not in NEW_LEARNERS
            _rule(failures, f"{tag}/grad.{key}", g, full[key] / c64, rec[f"f32/grad/{key}"] / c32)
        else:
            assert g.size > SMALL
            _rule(failures, f"{tag}/sketch.{key}", sketch(g), sketched[key] / c64, rec[f"f32/sketch/{key}"] / c32)
        if g.size > SMALL:
            large += 1
            _rule(failures, f"{tag}/restated.{key}", g, ref["f64"][0][key].numpy(), ref["f32"][0][key].numpy())
    assert large >= 4 and L.step() == 0
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", NEW_LEARNERS)
def test_learner_on_the_reference_batch(zenv_mod, name):
    """One minibatch (apply = 0) of each learner the reference's batches had not reached: the flat learner with the
    distributional critic (value_std included, the recorded gradients divided by the recorded clip factor), both levels
    of the xy-goals, fixed-length-skills and Options agents (the skill families' batches leave skill 3 without a
    sample) and DIAYN's inverse model."""
    _check_first_minibatch(zenv_mod, name)


@pytest.mark.parametrize("name", list(SOURCES))
def test_two_minibatches_with_adam(zenv_mod, name):
    """index0 then index1, each with its clip and Adam step, as the reference's update ran them: both rows of
    statistics, and Adam's moments and the parameters of every tensor the fixture keeps (those of at most 256 elements:
    every bias and head) after the second step.  The flat learner's clip is active in the recording, so its moments and
    parameters are the first comparison of the device's clip with the reference's own numbers.

    param after Adam is ill-conditioned where the first-step gradient is tiny (one step's sensitivity to a gradient
    error is lr eps / (|g| + eps)^2; in the recorded Zone-goals high level the reference's own float32 run is 48 445 ulp
    from its float64 run in actor.2.bias, whose float64 gradient is 2.8e-17: a softmax over zones ignores a shared
    bias).  check_rule's per-tensor base carries that through e32: every element of every recorded parameter is
    compared, none is left out."""
    Z = zenv_mod
    nat = Z._native
    L = _learner(Z, name)
    rec, tag, failures = L.rec, f"adam-{name}", []
    L.init()
    for i in range(2):
        L.minibatch(rec[f"index{i}"].astype(np.int32), True)
        _stats_rule(failures, L, tag, L.stats()[0], i)
    assert L.step() == 2
    kept = sorted(sub(rec, "f64/param/"))
    assert kept == sorted(sub(rec, "f64/exp_avg/")) == sorted(sub(rec, "f64/exp_avg_sq/")) and len(kept) >= 6
    for which, what in ((nat.PPO_EXP_AVG, "exp_avg"), (nat.PPO_EXP_AVG_SQ, "exp_avg_sq"), (nat.PPO_PARAM, "param")):
        dev = L.tensors(which)
        for key in kept:
            assert dev[key].shape == rec[f"f64/{what}/{key}"].shape
            _rule(failures, f"{tag}/{what}.{key}", dev[key], rec[f"f64/{what}/{key}"], rec[f"f32/{what}/{key}"])
    assert not failures, "\n".join(failures)


def test_skill_prior_on_the_reference_picks(zenv_mod):
    """Two diayn_prior_update steps from the reference's logits, learning rate and eps on its recorded picks (the
    high level's 24 rows, skill 3 never among them) against the logits and probabilities its update_skill_prior left."""
    Z = zenv_mod
    rec = sub(load("main", "skill_updates"), "prior_update/")
    nets = load("main", "skill_networks")
    assert rec["count/skills_without_a_sample"] > 0
    s = _handle(Z, "sk")
    env, actions = s["env"], rec["actions"].astype(np.int32)
    assert len(actions) == s["M"] == int(s["hi_t"]["action"].shape[0])
    _plant({"action": s["hi_t"]["action"]}, {"action": actions})
    np.testing.assert_array_equal(rec["f32/logits0"], rec["f64/logits0"])
    env.diayn_init(sub(nets, "inverse/sd/"), N_SKILLS, prior_logits=rec["f32/logits0"],
                   prior=dict(lr=float(rec["hyper/lr"]), adam_eps=float(rec["hyper/optim_eps"])), max_batch=64)
    np.testing.assert_array_equal(env.diayn_prior_logits(), rec["f32/logits0"])
    failures = []
    for step in (1, 2):
        logits = env.diayn_prior_update()
        probs = torch.softmax(torch.as_tensor(logits, dtype=F64), dim=0).numpy()
        _rule(failures, f"golden-prior/logits{step}", logits, rec[f"f64/logits{step}"], rec[f"f32/logits{step}"])
        _rule(failures, f"golden-prior/probs{step}", probs, rec[f"f64/probs{step}"], rec[f"f32/probs{step}"])
    assert not failures, "\n".join(failures)
