"""What the GPU tests of the Options agent's device learners share (test_gpu_opppo_update.py and its *_shapes file):
handles with a real collect_options, the planted records, and the comparison of one minibatch -- every gradient tensor
and the six statistics -- with the float64 / float32 references of tests/opppo_update_ref.py under
ppo_update_ref.check_rule.  Each test file keeps its own cache of handles and its own report list and passes them in.

Collection.  A plain task handle; the acting agent comes from option_ref.random_state_dicts(..., term_bias=b): the third
component's mean is 2 (sigmoid(b) - 0.5) for every input and its std sits at the floor, so an option ends with
probability sigmoid(4 mu_2 - 3) per frame -- about 0.73 at b = +20 (mu_2 = 1) and about 1e-3 at b = -20 (mu_2 = -1).  M,
the number of transitions the call closed, depends on the draws; the setup collects with the first policy seed from 5
on at which M is what the test needs (at least 8 and no multiple of 32; or exactly 0) and asserts that one was found.
The CPU replay of tests/option_collect_ref.py drives a device handle, so M cannot be confirmed without the device.

Learners.  Initialised from ordinary random_state_dicts (no term_bias): no std sits at its 1e-3 floor.

Planted, through TorchZoneEnv's aliases of the device buffers:
  high  rows 0-7 (M >= 8): the recorded log_prob, advantage, value and return such that every loss branch is reached by
        construction
  low   frames 0 .. T-2 of envs 1 .. N-1: the skill of flat sample i is i % S, so that a run of S consecutive samples
        holds every skill; all three action components drawn anew from the float64 learner network's Normal under the
        planted skill (a seeded generator), with the recorded log_probs and value that network's own (ratio 1 up to
        rounding).  Components 0-1 go to ZENV_F_EXP_ACTION / _LOG_PROB, component 2 to ZENV_F_LO_TERM_ACTION /
        _TERM_LOG_PROB.  Env 0 keeps what the collector recorded; frame T-1 is nobody's sample."""
import numpy as np
import torch

from tests import option_ref
from tests import opppo_update_ref as R
from tests import ppo_update_ref as RF
from tests.ppo_update_dev import PLANTED, host, print_worst  # noqa: F401  (re-exported)

F32, F64 = torch.float32, torch.float64
LEVELS = {"lo": 0, "hi": 1}
ENDS_OFTEN, ENDS_NEVER = 20.0, -20.0


def op_setup(Z, cfg, h, N, S, seed, T=12, term_bias=ENDS_OFTEN, want_m=None):
    """A plain task handle: the acting agent loaded with `term_bias`, one collect_options of T frames whose M satisfies
    want_m (default: M >= 8 and M % 32 != 0), the learners' parameters drawn apart, then the planted records (module
    docstring)."""
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    want_m = want_m or (lambda m: m >= PLANTED and m % 32 != 0)
    env = Z.ZoneVecEnv(cfg, N)
    env.build_bank(11, N)
    env.schedule_sequential()
    env.reset()
    F, Zn = env.zone_feat, env.num_zones
    act_hi, act_lo = option_ref.random_state_dicts(F, S, h=h, seed=seed, term_bias=term_bias)
    hi_sd, lo_sd = option_ref.random_state_dicts(F, S, h=h, seed=seed)
    env.load_options(Z.option_tensors_from_state_dicts(act_hi, act_lo))
    tenv = TorchZoneEnv(env)
    for policy_seed in range(5, 13):
        lo_t, hi_t, _ = tenv.collect_options(T, policy_seed=policy_seed)
        M = int(hi_t["count"].sum().item())
        if want_m(M):
            break
    assert want_m(M), M
    assert tuple(lo_t["skill"].shape) == (N, T - 1) and (M == 0 or int(hi_t["value"].shape[0]) == M)
    torch.cuda.synchronize()
    dev = tenv.device
    collected = host(lo_t)["skill"]
    assert collected.min() >= 0 and collected.max() < S
    if N > 1:
        skill = (np.arange(N * (T - 1)) % S).reshape(N, T - 1)[1:]
        rows = {k: v[1:] for k, v in host(lo_t).items()}
        rows["skill"] = skill
        b = R.lo_batch(rows, np.arange((N - 1) * (T - 1)), F64)
        with torch.no_grad():
            mu, std, v = R.model_from("lo", lo_sd, F, F64)(b["obs"], b["zone_obs"], b["skill"])
            noise = torch.randn(mu.shape, generator=torch.Generator().manual_seed(4000 + seed), dtype=F64)
            action = (mu + std * noise).float()
            lp = torch.distributions.Normal(mu, std).log_prob(action.double()).float()
        shape = (N - 1, T - 1)
        lo_t["skill"][1:] = torch.as_tensor(skill, dtype=torch.int32, device=dev)
        lo_t["action"][1:] = action[:, :2].reshape(shape + (2,)).to(dev)
        lo_t["term_action"][1:] = action[:, 2].reshape(shape).to(dev)
        lo_t["log_prob"][1:] = lp[:, :2].reshape(shape + (2,)).to(dev)
        lo_t["term_log_prob"][1:] = lp[:, 2].reshape(shape).to(dev)
        lo_t["value"][1:] = v.float().reshape(shape).to(dev)
        lo_t["returnn"][1:] = lo_t["value"][1:] + lo_t["advantage"][1:]
        torch.cuda.synchronize()
    if M >= PLANTED:
        model = R.model_from("hi", hi_sd, F, F64)
        rows = {k: v[:PLANTED] for k, v in host(hi_t).items() if k != "count"}
        b = R.hi_batch(rows, np.arange(PLANTED), F64)
        with torch.no_grad():
            logits, v = model(b["obs"], b["zone_obs"])
            lp = torch.log_softmax(logits, dim=1).gather(1, b["action"].view(-1, 1)).squeeze(1)
        # the learner is not the agent that acted: rows 0-1 and 6-7 at ratio 1 under the learner, rows 2-3 at ratio
        # e^0.5 above the range, rows 4-5 at e^-0.5 below it; the advantage's sign picks the branch
        hi_t["log_prob"][:PLANTED] = lp.float().to(dev)
        hi_t["log_prob"][2:4] = (lp[2:4] - 0.5).float().to(dev)
        hi_t["log_prob"][4:6] = (lp[4:6] + 0.5).float().to(dev)
        hi_t["advantage"][2:6] = torch.tensor([0.9, -0.8, 0.7, -1.1], device=dev)
        # rows 6-7: the recorded value 1 away, the return just past the new value: the clipped term is the larger one
        hi_t["value"][6:8] = (v[6:8] + torch.tensor([-1.0, 1.0], dtype=F64)).float().to(dev)
        hi_t["returnn"][6:8] = (v[6:8] + torch.tensor([0.05, -0.05], dtype=F64)).float().to(dev)
        torch.cuda.synchronize()
    hi_host = host(hi_t) if M else {}
    return dict(env=env, tenv=tenv, hi_sd=hi_sd, lo_sd=lo_sd, sd={"hi": hi_sd, "lo": lo_sd}, act_sd=(act_hi, act_lo), F=F,
                Z=Zn, h=h, S=S, N=N, M=M, T=T, lo_t=lo_t, hi_t=hi_t, lo=host(lo_t), hi=hi_host,
                total={"lo": N * (T - 1), "hi": M}, policy_seed=policy_seed)


def refresh(s):
    """The host copies after a test planted something more."""
    torch.cuda.synchronize()
    s["lo"] = host(s["lo_t"])
    s["hi"] = host(s["hi_t"]) if s["M"] else {}


def assert_planted_branches(s, idx=None):
    """Every branch has a sample among the planted rows."""
    b = op_batch(s, "hi", np.arange(PLANTED) if idx is None else idx, F64)
    hi, lo, val = R.branches("hi", R.model_from("hi", s["hi_sd"], s["F"], F64), b, R.HI_HYPER["clip_eps"])
    assert bool(hi[2]) and bool(lo[5]) and bool(val[6]) and bool(val[7]) and not bool(hi[3]) and not bool(lo[4])


def assert_every_skill(s, idx):
    """Every skill 0 .. S-1 occurs among the low-level samples idx."""
    skills = s["lo"]["skill"].reshape(-1)[np.asarray(idx, np.int64)]
    assert set(skills.tolist()) == set(range(s["S"])), sorted(set(skills.tolist()))


def op_batch(s, level, idx, dt):
    return R.lo_batch(s["lo"], idx, dt) if level == "lo" else R.hi_batch(s["hi"], idx, dt)


def op_keys(level):
    from combinatorial_rl_tasks_amd import agents
    hi, lo = agents.opppo_state_dict_keys()
    return hi if level == "hi" else lo


def op_by_key(env, level, which):
    t = env.opppo_tensors(LEVELS[level], which)
    return {key: t[name] for name, key in op_keys(level).items()}


def op_init(s, sd=None, lo=None, hi=None):
    sd = sd or s["sd"]
    big = dict(max_batch=max(max(s["total"].values()), 1))
    s["env"].opppo_init(sd["hi"], sd["lo"], lo=dict(big, **(lo or {})), hi=dict(big, **(hi or {})))


def op_ref_pair(s, level, sd, idx, hyper, scale=1.0):
    """((grads64, stats64), (grads32, stats32)) of the samples idx, everything times `scale`."""
    out = []
    for dt in (F64, F32):
        g, st = R.gradients(level, R.model_from(level, sd, s["F"], dt), op_batch(s, level, idx, dt), hyper)
        out.append(({k: v.numpy() * scale for k, v in g.items()}, {k: v * scale for k, v in st.items()}))
    return out


def op_compare(Z, s, level, ref, tag, report):
    """The six statistics and every gradient tensor the learner holds now against `ref` (op_ref_pair) under the rule."""
    env = s["env"]
    stats = env.opppo_stats(LEVELS[level])[0]
    grads = op_by_key(env, level, Z._native.PPO_GRAD)
    (g64, s64), (g32, s32) = ref
    assert len(grads) == (18 if level == "lo" else 16) and set(grads) == set(g64)
    for i, name in enumerate(R.STATS):
        RF.check_rule(f"{tag}/{level}.stat.{name}", stats[i], s64[name], s32[name], report)
    for key in g64:
        assert grads[key].shape == tuple(g64[key].shape)
        RF.check_rule(f"{tag}/{level}.grad.{key}", grads[key], g64[key], g32[key], report)
    return stats, s64, s32


def op_check_minibatch(Z, s, level, sd, idx, hyper, tag, report):
    """apply = 0 on `sd`: the six statistics and every gradient tensor under the rule."""
    over = {k: hyper[k] for k in ("clip_eps", "entropy_coef", "value_loss_coef")}
    op_init(s, dict(s["sd"], **{level: sd}), **{level: over})
    s["env"].opppo_minibatch(LEVELS[level], np.asarray(idx, np.int32))
    return op_compare(Z, s, level, op_ref_pair(s, level, sd, idx, hyper), tag, report)


def op_indexes(s, level, batch, seed):
    """`batch` sample indexes ("all": every one); the last valid index is always among them.  High level: batches
    smaller than everything come from the rows that are not planted."""
    total = s["total"][level]
    if batch == "all":
        return np.arange(total)
    first = PLANTED if level == "hi" and total > PLANTED else 0
    idx = first + np.random.default_rng(seed).permutation(total - first)[:batch]
    idx[-1] = total - 1
    return idx


def arenas(env, lv, prefix="opppo"):
    from combinatorial_rl_tasks_amd import _native as nat
    return {w: getattr(env, prefix + "_tensors")(lv, w)
            for w in (nat.PPO_PARAM, nat.PPO_GRAD, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}


def grad_arena(s, lv):
    """The whole gradient arena, padding included."""
    from combinatorial_rl_tasks_amd import _native as nat
    tenv = s["tenv"]
    ptr, count = s["env"].opppo_tensor_ptr(lv, nat.PPO_GRAD, -1)
    with torch.cuda.device(tenv.device):
        return tenv._alias_ptr(ptr, (count,)).cpu().numpy().copy()


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k])
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=str(k))
