"""The flat learner on a solver-ordered handle's 7-wide rows (zenv_order_rows; zenv_ppo_* at F = 7 on the records of a
zenv_collect that holds visits, an auto-reset and the shaped reward): one minibatch without a step, then one epoch of
two minibatches, against tests/ppo_update_ref.py under the rule of tests/test_gpu_ppo_update.py
(ppo_update_ref.check_rule: 8 times the float32 run's own deviation from the float64 run, or 8 ulp at the tensor's
scale); and the same call twice from the same state gives the same bits.

Shapes: tests/order_rows_cases.py -- 70 envs x 6 frames = 420 samples, 15 zones with h 185 and 5 zones with h 8.
The index lists leave out the few samples on which the float64 and float32 torch runs cannot tell which way a ReLU
gate opens (ppo_update_dev.decided_samples)."""
import numpy as np
import pytest
import torch

from tests import order_rows_cases as K
from tests import ppo_update_dev as D
from tests import ppo_update_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
CASES = [(15, 185), (5, 8)]
_SETUPS = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _SETUPS.values():
        s["env"].close()
    D.print_worst(REPORT, "order rows ppo update", 40)


def _setup(Z, zones, h):
    if (zones, h) not in _SETUPS:
        from combinatorial_rl_tasks_amd import agents
        env = K.make_env(Z, zones)
        sd = R.random_state_dict(env.net_zone_feat, h, False, seed=zones)
        assert tuple(sd["env_model.zone_net_.0.weight"].shape) == (h, 15)
        env.load_mlp(agents.mlp_tensors_from_state_dict(sd), precision="f32")
        exps = {k: np.ascontiguousarray(v) for k, v in env.collect(K.T, policy_seed=5).items()}
        logs = env.episode_logs()
        # what the learner is compared on holds visits, an auto-reset and the order feature
        assert (logs["return_per_episode"] >= 1).sum() >= K.N // 2 and (exps["mask"] == 0).sum() == K.N
        assert exps["zone_obs"].shape == (K.N, K.T, zones, 7) and exps["zone_obs"][..., 6].any()
        decided = D.decided_samples(R.model_from(sd, 7, F64), R.model_from(sd, 7, F32), exps)
        print(f"order rows learner Z={zones} h={h}: {int((~decided).sum())} of {decided.size} samples hold an undecided gate")
        assert decided.sum() >= 0.85 * decided.size
        _SETUPS[(zones, h)] = dict(env=env, sd=sd, exps=exps, F=7, Z=zones, h=h, N=K.N, T=K.T, dist=False, decided=decided)
    return _SETUPS[(zones, h)]


def _covers_visits_and_resets(s, idx):
    """The samples compared hold first frames after an auto-reset (mask 0) and frames of envs that visited."""
    mask = s["exps"]["mask"].reshape(-1)[idx]
    return (mask == 0).sum() >= 10 and (idx // K.T % 2 == 0).sum() >= len(idx) // 4


@pytest.mark.parametrize("zones,h", CASES)
@pytest.mark.parametrize("batch", [37, 420])
def test_one_minibatch_without_a_step(zenv_mod, zones, h, batch):
    s = _setup(zenv_mod, zones, h)
    idx = np.random.default_rng(batch).permutation(K.N * K.T)[:batch]
    idx = idx[s["decided"][idx]]                        # (see decided_samples)
    assert len(idx) >= 0.85 * batch and (batch < 420 or _covers_visits_and_resets(s, idx))
    stats, s64, s32 = D.flat_check_minibatch(zenv_mod, s, s["sd"], idx, R.HYPER, f"order-{zones}-{h}", REPORT, max_batch=420)
    assert s["env"].ppo_get_step() == 0
    # the gradient of the order value's input column is there, and is the reference's (checked above with the tensor)
    g = D.flat_by_key(s["env"], zenv_mod._native.PPO_GRAD)["env_model.zone_net_.0.weight"]
    assert g.shape == (h, 15) and np.abs(g[:, 14]).max() > 0
    # unchanged parameters right after the collect: ratio = 1, so the policy loss is -mean(advantage)
    adv = R.as_batch(s["exps"], idx, F64)["advantage"]
    R.check_rule(f"order-{zones}-{h}/policy_loss_at_ratio_1", stats[3], -float(adv.mean()), s32["policy_loss"], REPORT)


def _state(env, nat):
    return {w: env.ppo_tensors(w) for w in (nat.PPO_PARAM, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}, env.ppo_get_step()


@pytest.mark.parametrize("zones,h", CASES)
def test_one_epoch_of_two_minibatches_and_the_same_bits_twice(zenv_mod, zones, h):
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, zones, h)
    env = s["env"]
    total = K.N * K.T
    env.ppo_init(s["sd"], max_batch=200, **R.HYPER)
    start = _state(env, nat)
    # the epoch's order: a permutation of all frames (recurrence 1, batch_num 0), 200 decided samples for the first
    # minibatch, and for the second up to 200 of the rest that are decided under the parameters the first one leaves
    # (see decided_samples; the reference learners say which)
    perm = R.batch_indexes(total, K.T, 0, np.random.default_rng(21))
    assert len(perm) == total
    first = perm[s["decided"][perm]][:200]
    ref = {dt: R.RefLearner(s["sd"], s["F"], dt, R.HYPER) for dt in (F64, F32)}
    ref_stats = {dt: [ref[dt].minibatch(R.as_batch(s["exps"], first, dt))] for dt in ref}
    rest = perm[~np.isin(perm, first)]
    second = rest[D.decided_samples(ref[F64].model, ref[F32].model, s["exps"])[rest]][:200]
    assert len(first) == 200 and 150 <= len(second) <= 200
    assert _covers_visits_and_resets(s, first) and _covers_visits_and_resets(s, second)
    for dt in ref:
        ref_stats[dt].append(ref[dt].minibatch(R.as_batch(s["exps"], second, dt)))
    order = np.concatenate([first, second]).astype(np.int32)
    env.ppo_epoch(order, 200)
    dev_stats = env.ppo_stats()
    assert dev_stats.shape == (2, 6) and env.ppo_get_step() == 2
    r64, r32 = np.array(ref_stats[F64]), np.array(ref_stats[F32])
    for i, name in enumerate(R.STATS):
        R.check_rule(f"order-epoch-{zones}-{h}/stat.{name}", dev_stats[:, i], r64[:, i], r32[:, i], REPORT)
    after = _state(env, nat)
    params = D.flat_by_key(env, nat.PPO_PARAM)
    p64, p32 = ref[F64].model.state_dict(), ref[F32].model.state_dict()
    assert set(params) == set(p64)
    for key in params:
        R.check_rule(f"order-epoch-{zones}-{h}/param.{key}", params[key], p64[key].numpy(), p32[key].numpy(), REPORT)
    assert not np.array_equal(after[0][nat.PPO_PARAM]["zone_w1"][:, 14], start[0][nat.PPO_PARAM]["zone_w1"][:, 14])
    # the same call from the same state: the same bits
    for w, tensors in start[0].items():
        env.ppo_set_tensors(tensors, w)
    env.ppo_set_step(start[1])
    env.ppo_epoch(order, 200)
    again = _state(env, nat)
    assert again[1] == after[1] == 2 and K.same_bits(env.ppo_stats(), dev_stats)
    for w in after[0]:
        for name in after[0][w]:
            assert K.same_bits(again[0][w][name], after[0][w][name]), (w, name)
    # the acting network is the learner's after ppo_publish: on the handle's current 7-wide rows
    env.ppo_publish(precision="f32")
    out = env.mlp_forward(with_value=True)
    obs, rows = env.get(Z.F_OBS), K.want_rows(env, Z)
    nets = {}
    for dt in ref:
        with torch.no_grad():
            nets[dt] = ref[dt].model(torch.as_tensor(obs).to(dt), torch.as_tensor(rows).to(dt))
    for i, name in enumerate(("mu", "std", "value")):
        R.check_rule(f"order-epoch-{zones}-{h}/published.{name}", out[i], nets[F64][i].numpy(), nets[F32][i].numpy(), REPORT)
