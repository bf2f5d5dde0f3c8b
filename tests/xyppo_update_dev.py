"""What the GPU tests of the xy-goals device learners share (test_gpu_xyppo_update.py and its *_shapes file): handles
with a real collect_xy, the planted high-level rows, and the comparison of one minibatch -- every gradient tensor and the
six statistics -- with the float64 / float32 references of tests/xyppo_update_ref.py under ppo_update_ref.check_rule.
Each test file keeps its own cache of handles and its own report list and passes them in."""
import numpy as np
import torch

from tests import ppo_update_ref as RF
from tests import xy_ref
from tests import xyppo_update_ref as R
from tests.ppo_update_dev import PLANTED, host, print_worst  # noqa: F401  (re-exported)

F32, F64 = torch.float32, torch.float64
LEVELS = {"lo": 0, "hi": 1}


def xy_setup(Z, cfg, h, N, seed, T=12, L=4):
    """A plain task handle: fresh parameters loaded into the acting agent with skill_len L, one collect_xy of T frames
    (W = T / L windows, M = N W rows).  With M >= 8, rows 0-7 of the high level's records are planted through
    TorchZoneEnv's aliases so that every loss branch is reached by construction."""
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    env = Z.ZoneVecEnv(cfg, N)
    env.build_bank(11, N)
    env.schedule_sequential()
    env.reset()
    F, Zn = env.zone_feat, env.num_zones
    hi_sd, lo_sd = xy_ref.random_state_dicts(F, h=h, seed=seed)
    env.load_xy(Z.xy_tensors_from_state_dicts(hi_sd, lo_sd), skill_len=L)
    tenv = TorchZoneEnv(env)
    lo_t, hi_t, _ = tenv.collect_xy(T, policy_seed=5)
    M = int(hi_t["value"].shape[0])
    assert M == N * (T // L)
    torch.cuda.synchronize()
    if M >= PLANTED:
        model = R.model_from("hi", hi_sd, F, F64)
        rows = {k: v[:PLANTED] for k, v in host(hi_t).items()}
        b = R.hi_batch(rows, np.arange(PLANTED), F64)
        with torch.no_grad():
            mu, std, v = model(b["obs"], b["zone_obs"])
            lp = torch.distributions.Normal(mu, std).log_prob(b["goal"]).sum(dim=1)
        dev = tenv.device
        # rows 2-3: ratio e^0.5 above the range, rows 4-5: e^-0.5 below it; the advantage's sign picks the branch
        hi_t["log_prob"][2:4] = (lp[2:4] - 0.5).float().to(dev)
        hi_t["log_prob"][4:6] = (lp[4:6] + 0.5).float().to(dev)
        hi_t["advantage"][2:6] = torch.tensor([0.9, -0.8, 0.7, -1.1], device=dev)
        # rows 6-7: the recorded value 1 away, the return just past the new value: the clipped term is the larger one
        hi_t["value"][6:8] = (v[6:8] + torch.tensor([-1.0, 1.0], dtype=F64)).float().to(dev)
        hi_t["returnn"][6:8] = (v[6:8] + torch.tensor([0.05, -0.05], dtype=F64)).float().to(dev)
        torch.cuda.synchronize()
    return dict(env=env, tenv=tenv, hi_sd=hi_sd, lo_sd=lo_sd, sd={"hi": hi_sd, "lo": lo_sd}, F=F, Z=Zn, h=h, N=N, M=M,
                T=T, L=L, lo_t=lo_t, hi_t=hi_t, lo=host(lo_t), hi=host(hi_t), total={"lo": N * T, "hi": M})


def assert_planted_branches(s, idx=None):
    """Every branch has a sample among the planted rows."""
    b = xy_batch(s, "hi", np.arange(PLANTED) if idx is None else idx, F64)
    hi, lo, val = R.branches("hi", R.model_from("hi", s["hi_sd"], s["F"], F64), b, R.HI_HYPER["clip_eps"])
    assert bool(hi[2]) and bool(lo[5]) and bool(val[6]) and bool(val[7]) and not bool(hi[3]) and not bool(lo[4])


def xy_batch(s, level, idx, dt):
    return R.lo_batch(s["lo"], idx, dt) if level == "lo" else R.hi_batch(s["hi"], idx, dt)


def xy_keys(level):
    from combinatorial_rl_tasks_amd import agents
    hi, lo = agents.xyppo_state_dict_keys()
    return hi if level == "hi" else lo


def xy_by_key(env, level, which):
    t = env.xyppo_tensors(LEVELS[level], which)
    return {key: t[name] for name, key in xy_keys(level).items()}


def xy_init(s, sd=None, lo=None, hi=None):
    sd = sd or s["sd"]
    big = dict(max_batch=max(s["total"].values()))
    s["env"].xyppo_init(sd["hi"], sd["lo"], lo=dict(big, **(lo or {})), hi=dict(big, **(hi or {})))


def xy_ref_pair(s, level, sd, idx, hyper, scale=1.0):
    """((grads64, stats64), (grads32, stats32)) of the samples idx, everything times `scale`."""
    out = []
    for dt in (F64, F32):
        g, st = R.gradients(level, R.model_from(level, sd, s["F"], dt), xy_batch(s, level, idx, dt), hyper)
        out.append(({k: v.numpy() * scale for k, v in g.items()}, {k: v * scale for k, v in st.items()}))
    return out


def xy_compare(Z, s, level, ref, tag, report):
    """The six statistics and every gradient tensor the learner holds now against `ref` (xy_ref_pair) under the rule."""
    env = s["env"]
    stats = env.xyppo_stats(LEVELS[level])[0]
    grads = xy_by_key(env, level, Z._native.PPO_GRAD)
    (g64, s64), (g32, s32) = ref
    assert len(grads) == 18 and set(grads) == set(g64)
    for i, name in enumerate(R.STATS):
        RF.check_rule(f"{tag}/{level}.stat.{name}", stats[i], s64[name], s32[name], report)
    for key in g64:
        assert grads[key].shape == tuple(g64[key].shape)
        RF.check_rule(f"{tag}/{level}.grad.{key}", grads[key], g64[key], g32[key], report)
    return stats, s64, s32


def xy_check_minibatch(Z, s, level, sd, idx, hyper, tag, report):
    """apply = 0 on `sd`: the six statistics and every gradient tensor under the rule."""
    over = {k: hyper[k] for k in ("clip_eps", "entropy_coef", "value_loss_coef")}
    xy_init(s, dict(s["sd"], **{level: sd}), **{level: over})
    s["env"].xyppo_minibatch(LEVELS[level], np.asarray(idx, np.int32))
    return xy_compare(Z, s, level, xy_ref_pair(s, level, sd, idx, hyper), tag, report)


def xy_indexes(s, level, batch, seed):
    """`batch` sample indexes ("all": every one); the last valid index is always among them.  High level: batches
    smaller than everything come from the rows that are not planted."""
    total = s["total"][level]
    if batch == "all":
        return np.arange(total)
    first = PLANTED if level == "hi" and total > PLANTED else 0
    idx = first + np.random.default_rng(seed).permutation(total - first)[:batch]
    idx[-1] = total - 1
    return idx


def arenas(env, lv):
    from combinatorial_rl_tasks_amd import _native as nat
    return {w: env.xyppo_tensors(lv, w) for w in (nat.PPO_PARAM, nat.PPO_GRAD, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}


def grad_arena(s, lv):
    """The whole gradient arena, padding included."""
    from combinatorial_rl_tasks_amd import _native as nat
    tenv = s["tenv"]
    ptr, count = s["env"].xyppo_tensor_ptr(lv, nat.PPO_GRAD, -1)
    with torch.cuda.device(tenv.device):
        return tenv._alias_ptr(ptr, (count,)).cpu().numpy().copy()


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k])
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=str(k))
