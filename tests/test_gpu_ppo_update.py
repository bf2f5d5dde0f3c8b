"""The flat actor-critic's PPO update on the device (zenv_ppo_*, ppo_update.hip) against the float64 restatement of
tests/ppo_update_ref.py, on experience of a real zenv_collect.  Every comparison of two floating-point results follows
one rule (ppo_update_ref.check_rule): the device may deviate from the float64 run by 8 times what the float32 run of
the same torch code on the CPU does, or by 8 ulp at the tensor's scale, whichever is larger.

Shapes: PointTSP-v0 (Z 15, F 6, h 185, 24 envs x 16 frames; batches 1, 37, 100, 384), ColourMatch-v0 (Z 6, F 7, h 7 and
64, 5 x 8; 33, 40), PointTTSP-v0 (Z 15, F 7, h 191, 8 x 8; 64), 25 zones (h 32, 4 x 4; 16); the distributional critic on
the PointTSP and ColourMatch rows."""
import numpy as np
import pytest
import torch

from tests import ppo_update_dev as D
from tests import ppo_update_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
CASES = {"tsp": ("PointTSP-v0", 185, 24, 16), "cm7": ("ColourMatch-v0", 7, 5, 8), "cm64": ("ColourMatch-v0", 64, 5, 8),
         "ttsp": ("PointTTSP-v0", 191, 8, 8), "z25": (None, 32, 4, 4)}
_SETUPS = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _SETUPS.values():
        s["env"].close()
    D.print_worst(REPORT, "ppo update", 40)


def _setup(Z, case, dist):
    """One handle per (shape, critic): fresh parameters loaded into the acting network, one collect."""
    key = (case, dist)
    if key not in _SETUPS:
        env_id, h, N, T = CASES[case]
        cfg = Z.config_for_id(env_id) if env_id else Z.default_config(0, 25, zones_keepout=0.40)
        _SETUPS[key] = D.flat_setup(Z, cfg, h, N, T, dist, seed=len(_SETUPS))
    return _SETUPS[key]


_by_key = D.flat_by_key


def _check_minibatch(Z, s, sd, idx, hyper, tag):
    return D.flat_check_minibatch(Z, s, sd, idx, hyper, tag, REPORT)


FRESH = [("tsp", False, 1), ("tsp", False, 37), ("tsp", False, 100), ("tsp", False, 384), ("tsp", True, 100),
         ("cm7", False, 33), ("cm7", True, 40), ("cm64", False, 40), ("cm64", True, 33), ("ttsp", False, 64),
         ("z25", False, 16)]


@pytest.mark.parametrize("case,dist,batch", FRESH)
def test_forward_and_gradients_on_fresh_parameters(zenv_mod, case, dist, batch):
    s = _setup(zenv_mod, case, dist)
    total = s["N"] * s["T"]
    idx = np.random.default_rng(batch).permutation(total)[:batch]
    stats, s64, s32 = _check_minibatch(zenv_mod, s, s["sd"], idx, R.HYPER, f"fresh-{case}")
    # unchanged parameters right after the collect: ratio = 1, so the policy loss is -mean(advantage)
    adv = R.as_batch(s["exps"], idx, F64)["advantage"]
    R.check_rule(f"fresh-{case}/policy_loss_at_ratio_1", stats[3], -float(adv.mean()), s32["policy_loss"], REPORT)


@pytest.mark.parametrize("case,dist,batch", [("tsp", False, 100), ("tsp", True, 100), ("cm64", False, 40)])
def test_gradients_on_the_clipped_branches(zenv_mod, case, dist, batch):
    """The perturbed parameters of test_ppo_update_ref_cpu.py's condition: clipped samples and their zero gradients."""
    s = _setup(zenv_mod, case, dist)
    sd = R.perturbed(s["sd"])
    idx = np.random.default_rng(7).permutation(s["N"] * s["T"])[:batch]
    hyper = dict(R.HYPER, clip_eps=R.PERTURB_CLIP_EPS)
    hi, lo, val = R.branches(R.model_from(sd, s["F"], F64), R.as_batch(s["exps"], idx, F64), hyper["clip_eps"])
    print("clipped fractions on the collected experience:", float(hi.double().mean()), float(lo.double().mean()),
          float(val.double().mean()))
    assert int(hi.sum()) > 0 and int(lo.sum()) > 0 and (dist or int(val.sum()) > 0)
    _check_minibatch(zenv_mod, s, sd, idx, hyper, f"clipped-{case}")


@pytest.mark.parametrize("case,dist", [("tsp", False), ("cm7", True)])
def test_a_repeated_index_adds_its_gradient(zenv_mod, case, dist):
    s = _setup(zenv_mod, case, dist)
    idx = np.random.default_rng(3).permutation(s["N"] * s["T"])[:37]
    idx[5] = idx[0]
    idx[36] = idx[0]
    _check_minibatch(zenv_mod, s, s["sd"], idx, R.HYPER, f"repeat-{case}")


@pytest.mark.parametrize("max_grad_norm", [1e3, 1e-4])
def test_clip_and_adam_from_identical_gradients(zenv_mod, max_grad_norm):
    """zenv_ppo_apply on the device's own gradients against the float64 arithmetic and float32 torch Adam, steps 1, 2
    and 10; a gradient norm below max_grad_norm and one far above."""
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "tsp", False)
    env = s["env"]
    hyper = dict(R.HYPER, max_grad_norm=max_grad_norm)
    env.ppo_init(s["sd"], max_batch=384, **hyper)
    env.ppo_minibatch(np.arange(100, dtype=np.int32))
    g = env.ppo_tensors(nat.PPO_GRAD)
    names = list(g)
    norm = float(env.ppo_stats()[0][5])
    assert (norm < max_grad_norm) == (max_grad_norm > 1.0) and (max_grad_norm > 1.0 or norm > 100 * max_grad_norm)
    p0 = env.ppo_tensors()
    p64 = {n: p0[n].astype(np.float64) for n in names}
    m64 = {n: np.zeros_like(p64[n]) for n in names}
    v64 = {n: np.zeros_like(p64[n]) for n in names}
    coef = R.clip_coef(R.total_norm([torch.as_tensor(g[n]) for n in names]), max_grad_norm)
    params32 = [torch.nn.Parameter(torch.as_tensor(p0[n]).clone()) for n in names]
    opt = torch.optim.Adam(params32, hyper["lr"], eps=hyper["adam_eps"], foreach=False)
    for step in range(1, 11):
        env.ppo_apply()
        for n in names:
            R.adam_step(p64[n], coef * g[n].astype(np.float64), m64[n], v64[n], step, hyper["lr"], hyper["adam_eps"])
        for p, n in zip(params32, names):
            p.grad = torch.as_tensor(g[n]).clone()
        torch.nn.utils.clip_grad_norm_(params32, max_grad_norm, foreach=False)
        opt.step()
        if step in (1, 2, 10):
            assert env.ppo_get_step() == step
            dev = {w: env.ppo_tensors(w) for w in (nat.PPO_PARAM, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}
            for p, n in zip(params32, names):
                st = opt.state[p]
                tag = f"adam-{max_grad_norm:g}-step{step}"
                R.check_rule(f"{tag}/param.{n}", dev[nat.PPO_PARAM][n], p64[n], p.detach().numpy(), REPORT)
                R.check_rule(f"{tag}/exp_avg.{n}", dev[nat.PPO_EXP_AVG][n], m64[n], st["exp_avg"].numpy(), REPORT)
                R.check_rule(f"{tag}/exp_avg_sq.{n}", dev[nat.PPO_EXP_AVG_SQ][n], v64[n], st["exp_avg_sq"].numpy(), REPORT)
    np.testing.assert_array_equal(env.ppo_tensors(nat.PPO_GRAD)["zone_w2"], g["zone_w2"])   # the arena keeps the gradients


def _snapshot(env):
    nat = env_nat(env)
    return {w: env.ppo_tensors(w) for w in (nat.PPO_PARAM, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}, env.ppo_get_step()


def env_nat(env):
    from combinatorial_rl_tasks_amd import _native
    return _native


def _restore(env, snap):
    tensors, step = snap
    for w, t in tensors.items():
        env.ppo_set_tensors(t, w)
    env.ppo_set_step(step)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=str(k))


@pytest.mark.parametrize("dist", [False, True])
def test_two_epochs_end_to_end(zenv_mod, dist):
    """2 epochs x 4 minibatches (100, 100, 100, 84 of 384) through ppo_epoch against the reference learners driven by
    the same order; then the published network on the handle's current observations."""
    Z = zenv_mod
    s = _setup(Z, "tsp", dist)
    env = s["env"]
    env.ppo_init(s["sd"], max_batch=100, **R.HYPER)
    rng = np.random.default_rng(21)
    orders = [R.batch_indexes(384, 16, 0, rng), R.batch_indexes(384, 16, 2, rng)]
    ref = {dt: R.RefLearner(s["sd"], s["F"], dt, R.HYPER) for dt in (F64, F32)}
    dev_stats, ref_stats = [], {F64: [], F32: []}
    for order in orders:
        assert len(order) == 384
        env.ppo_epoch(order, 100)
        dev_stats.append(env.ppo_stats())
        for dt in ref:
            for lo in range(0, 384, 100):
                ref_stats[dt].append(ref[dt].minibatch(R.as_batch(s["exps"], order[lo:lo + 100], dt)))
    dev_stats = np.concatenate(dev_stats)
    assert dev_stats.shape == (8, 6) and env.ppo_get_step() == 8
    r64, r32 = np.array(ref_stats[F64]), np.array(ref_stats[F32])
    for i, name in enumerate(R.STATS):
        R.check_rule(f"e2e/stat.{name}", dev_stats[:, i], r64[:, i], r32[:, i], REPORT)
    # the acting network is the learner's only after ppo_publish
    env.ppo_publish(precision="f32")
    out = env.mlp_forward(with_value=True)
    obs, zone_obs = env.get(Z.F_OBS), env.get(Z.F_ZONE_OBS)
    nets = {}
    for dt in ref:
        with torch.no_grad():
            nets[dt] = ref[dt].model(torch.as_tensor(obs).to(dt), torch.as_tensor(zone_obs).to(dt))
    for i, name in enumerate(("mu", "std", "value") + (("value_sigma",) if dist else ())):
        R.check_rule(f"e2e/published.{name}", out[i], nets[F64][i].numpy(), nets[F32][i].numpy(), REPORT)


def test_ppo_update_logs_and_index_order(zenv_mod):
    """ppo_update = the epochs of ppo_batch_indexes (odd calls drop the rollouts' last frames) through ppo_epoch; its
    logs are the means of the last epoch's statistics."""
    Z = zenv_mod
    from combinatorial_rl_tasks_amd import agents
    s = _setup(Z, "tsp", False)
    env = s["env"]
    env.ppo_init(s["sd"], max_batch=100, **R.HYPER)
    snap = _snapshot(env)
    logs = env.ppo_update(2, 100, np.random.default_rng(5))
    assert env.ppo_batch_num == 2 and env.ppo_get_step() == 4 + 4          # 384 -> 4 batches; 360 -> 4 batches
    after = _snapshot(env)
    _restore(env, snap)
    rng = np.random.default_rng(5)
    for batch_num in (0, 1):
        order = agents.ppo_batch_indexes(384, 16, batch_num, rng)
        assert len(order) == (384 if batch_num == 0 else 360)
        env.ppo_epoch(order, 100)
    stats = env.ppo_stats()
    assert stats.shape == (4, 6)
    _same(after[0][Z._native.PPO_PARAM], env.ppo_tensors())
    want = stats.astype(np.float64).mean(axis=0)
    assert logs == {"entropy": want[0], "value": want[1], "policy_loss": want[3], "value_loss": want[4],
                    "grad_norm": want[5]}


def test_determinism_state_and_what_an_update_leaves_alone(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, "tsp", False)
    env = s["env"]
    env.ppo_init(s["sd"], max_batch=100, **R.HYPER)
    acting0 = env.mlp_forward(with_value=True)
    exp0 = env._download(env._experience_rows(s["T"]))
    order = R.batch_indexes(384, 16, 0, np.random.default_rng(1))
    env.ppo_epoch(order, 100)                       # some optimizer state to start from
    snap = _snapshot(env)
    env.ppo_epoch(order[::-1].copy(), 100)
    first = (_snapshot(env), env.ppo_stats())
    _restore(env, snap)
    env.ppo_epoch(order[::-1].copy(), 100)
    again = (_snapshot(env), env.ppo_stats())
    for w in first[0][0]:
        _same(first[0][0][w], again[0][0][w])
    np.testing.assert_array_equal(first[1], again[1])
    assert first[0][1] == again[0][1] == 8
    # apply = 1 is apply = 0 followed by ppo_apply
    _restore(env, snap)
    env.ppo_minibatch(order[:100], apply=True)
    fused = _snapshot(env)
    _restore(env, snap)
    env.ppo_minibatch(order[:100], apply=False)
    env.ppo_apply()
    split = _snapshot(env)
    for w in fused[0]:
        _same(fused[0][w], split[0][w])
    assert fused[1] == split[1] == 5
    # a round trip of Adam's state through torch.optim.Adam's state_dict continues bit-identically
    _restore(env, snap)
    state = env.ppo_optimizer_state()
    model = R.model_from(env.ppo_state_dict(), s["F"], F32)
    opt = torch.optim.Adam(model.parameters(), R.HYPER["lr"], eps=R.HYPER["adam_eps"])
    opt.load_state_dict({"state": {i: {k: torch.as_tensor(v) for k, v in st.items()} for i, st in state["state"].items()},
                         "param_groups": state["param_groups"]})
    saved = opt.state_dict()
    assert [float(st["step"]) for st in saved["state"].values()] == [4.0] * 18
    env.ppo_load_state_dict(R.random_state_dict(s["F"], s["h"], seed=99))      # scramble, then restore
    env.ppo_load_optimizer_state({"state": {}, "param_groups": saved["param_groups"]})
    assert env.ppo_get_step() == 0
    env.ppo_load_state_dict(model.state_dict())
    env.ppo_load_optimizer_state(saved)
    env.ppo_epoch(order[::-1].copy(), 100)
    for w in first[0][0]:
        _same(first[0][0][w], _snapshot(env)[0][w])
    # the acting network and the experience are untouched by all of it
    acting1 = env.mlp_forward(with_value=True)
    for a, b in zip(acting0, acting1):
        np.testing.assert_array_equal(a, b)
    exp1 = env._download(env._experience_rows(s["T"]))
    for k in exp0:
        np.testing.assert_array_equal(exp0[k], exp1[k], err_msg=k)


def test_torch_arenas_alias_the_learner(zenv_mod):
    Z = zenv_mod
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    s = _setup(Z, "cm64", True)
    env = s["env"]
    tenv = TorchZoneEnv(env)
    try:
        tenv.ppo_init(s["sd"], max_batch=40, **R.HYPER)
        sd = tenv.ppo_state_dict()
        assert set(sd) == set(s["sd"]) and all(t.is_cuda for t in sd.values())
        model = R.model_from(s["sd"], s["F"], F32).to(tenv.device)
        model.load_state_dict(sd)
        for k, v in s["sd"].items():
            np.testing.assert_array_equal(sd[k].cpu().numpy(), v.numpy())
        idx = torch.arange(40, dtype=torch.int32, device=tenv.device)
        tenv.ppo_minibatch(idx, apply=True)
        torch.cuda.synchronize()
        host = env.ppo_state_dict()
        for k in host:                                   # the views see the step without a copy
            np.testing.assert_array_equal(sd[k].cpu().numpy(), host[k])
        assert float((sd["critic_sigma.weight"].cpu() - s["sd"]["critic_sigma.weight"]).abs().max()) > 0
        g = tenv.ppo_views(Z._native.PPO_GRAD)
        assert float(tenv.ppo_arenas["grad"].pow(2).sum().sqrt().cpu()) == pytest.approx(
            float(tenv.ppo_stats()[0, 5].cpu()), rel=1e-5)
        assert g["zone_w1"].shape == (64, 15)
        opt_state = tenv.ppo_optimizer_state()
        assert len(opt_state["state"]) == 20 and float(opt_state["state"][0]["step"]) == 1.0
    finally:
        env.set_stream(None)


def test_guards(zenv_mod):
    Z = zenv_mod
    s = _setup(Z, "cm7", False)
    env = s["env"]
    total = s["N"] * s["T"]
    env.ppo_init(s["sd"], max_batch=33, **R.HYPER)
    ok = np.arange(33, dtype=np.int32)
    for bad_count in (0, 34):
        with pytest.raises(Z.ZenvError) as e:
            env.ppo_minibatch(np.zeros(bad_count, np.int32))
        assert e.value.code == Z.E_ARG
    for bad in (-1, total, 2 ** 31 - 1):
        idx = ok.copy()
        idx[7] = bad
        with pytest.raises(Z.ZenvError) as e:
            env.ppo_minibatch(idx)
        assert e.value.code == Z.E_ARG
    with pytest.raises(Z.ZenvError) as e:
        env.ppo_epoch(ok, 34)
    assert e.value.code == Z.E_ARG
    # device-resident indexes: far outside the buffers in both directions -- only the guard keeps them from being read
    dev = torch.device("cuda", env.device)
    idx = torch.as_tensor(ok).to(dev)
    idx[3] = 2 ** 31 - 1
    idx[20] = -(2 ** 31)
    torch.cuda.synchronize()
    env.ppo_minibatch(idx.data_ptr(), count=33)
    with pytest.raises(Z.ZenvError) as e:
        env.ppo_stats()
    assert e.value.code == Z.E_ARG and "index" in str(e.value)
    stats = env.ppo_stats()                              # reported once
    assert stats.shape == (1, 6) and np.all(np.isfinite(stats))
    grads = env.ppo_tensors(Z._native.PPO_GRAD)
    assert all(np.all(np.isfinite(g)) for g in grads.values())
    # the other 31 samples are the whole loss: the sums of a 31-sample minibatch, divided by 33
    keep = np.delete(ok, [3, 20])
    env.ppo_minibatch(keep)
    small = env.ppo_stats()[0]
    np.testing.assert_allclose(stats[0][:5], small[:5] * (31.0 / 33.0), rtol=1e-5, atol=1e-7)
    # call order
    fresh = Z.ZoneVecEnv(Z.config_for_id("ColourMatch-v0"), 2)
    try:
        fresh.build_bank(1, 2)
        fresh.reset()
        with pytest.raises(Z.ZenvError) as e:
            fresh.ppo_minibatch(np.zeros(1, np.int32))
        assert e.value.code == Z.E_STATE                 # no learner
        fresh.ppo_init(s["sd"], max_batch=4)
        for call in (lambda: fresh.ppo_minibatch(np.zeros(1, np.int32)), lambda: fresh.ppo_epoch(np.zeros(2, np.int32), 2)):
            with pytest.raises(Z.ZenvError) as e:
                call()
            assert e.value.code == Z.E_STATE             # no experience
    finally:
        fresh.close()
