"""DIAYN's inverse-model update and skill prior on the device (zenv_diayn_*, ppo_update.hip) against the float64
restatement of tests/diayn_update_ref.py, on the records of a real zenv_collect_skill.  Every comparison of two
floating-point results follows one rule (ppo_update_ref.check_rule): the device may deviate from the float64 run by 8
times what the float32 run of the same torch code on the CPU does, or by 8 ulp at the tensor's scale, whichever is larger.

Handles: plain task handles, episodes of 10 steps, N = 16 envs, skill_len 4 and T = 12 frames: every env finishes inside
its third window and idles to the window's end, so the mask has zeros and N (T - 1) = 176 sample indexes of which fewer
are kept.  Shapes: PointTSP-v0 (Z 15, F 6, h 128, S 5), ColourMatch-v0 (Z 6, F 7, h 33, S 7)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import diayn_update_dev as D
from tests import diayn_update_ref as R
from tests import ppo_update_ref as RF

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
N, T, L = 16, 12, 4
CASES = {"tsp": ("PointTSP-v0", 128, 5), "cm": ("ColourMatch-v0", 33, 7)}
_SETUPS = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _teardown():
    yield
    for s in _SETUPS.values():
        s["env"].set_stream(None)
        s["env"].close()
    D.print_worst(REPORT, "diayn update", 44)


def _setup(Z, case, tag="", **kw):
    key = case + tag
    if key not in _SETUPS:
        env_id, h, S = CASES[case]
        _SETUPS[key] = D.dy_setup(Z, Z.config_for_id(env_id, num_steps=10), h, N, S, seed=list(CASES).index(case), T=T,
                                  L=L, **kw)
    return _SETUPS[key]


def _rc(Z, fn, *args):
    return getattr(Z._native.lib(), fn)(*args)


def test_the_collection_has_envs_that_finish_inside_windows(zenv_mod):
    s = _setup(zenv_mod, "tsp")
    mask = s["lo"]["mask"]
    assert (s["Z"], s["F"], s["S"], s["total"]) == (15, 6, 5, 176)
    assert 0 < len(s["kept"]) < s["total"] and np.any(mask[:, 1:] == 0) and np.any(mask[:, 1:] != 0)
    assert np.any(mask[:, 1:-1] == 0)                     # zeros off the window boundaries too
    assert set(s["lo"]["skill"].reshape(-1)[:].tolist()) <= set(range(5))


@pytest.mark.parametrize("batch", ["all", 37])
@pytest.mark.parametrize("case", list(CASES))
def test_minibatch_gradients(zenv_mod, case, batch):
    s = _setup(zenv_mod, case)
    idx = D.dy_indexes(s, batch, 1)
    assert len(idx) == (len(s["kept"]) if batch == "all" else batch) and s["kept"][-1] in idx
    b = R.batch(s["lo"], idx, F64)
    assert set(b["skill"].tolist()) == set(range(s["S"]))
    D.dy_check_minibatch(zenv_mod, s, s["sd"], idx, f"fresh-{case}", REPORT)
    D.dy_check_minibatch(zenv_mod, s, R.perturbed(s["sd"]), idx, f"perturbed-{case}", REPORT)


@pytest.mark.parametrize("case", list(CASES))
def test_adam_steps(zenv_mod, case):
    """Parameters and both moments after apply at steps 1, 2 and 10 against torch's Adam in float64 / float32."""
    Z = zenv_mod
    nat = Z._native
    s = _setup(Z, case)
    env = s["env"]
    D.dy_init(s)
    refs = {dt: R.RefLearner(s["sd"], s["F"], dt) for dt in (F64, F32)}
    rng = np.random.default_rng(3)
    for step in range(1, 11):
        idx = s["kept"][rng.permutation(len(s["kept"]))[:48]]
        env.diayn_minibatch(idx.astype(np.int32), apply=True)
        for dt, ref in refs.items():
            ref.minibatch(R.batch(s["lo"], idx, dt))
        if step not in (1, 2, 10):
            continue
        assert env.diayn_get_step() == step
        got = {w: D.dy_by_key(env, w) for w in (nat.PPO_PARAM, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}
        for key, p64 in refs[F64].model.named_parameters():
            p32 = dict(refs[F32].model.named_parameters())[key]
            st64, st32 = refs[F64].opt.state[p64], refs[F32].opt.state[p32]
            for what, w, a64, a32 in (("param", nat.PPO_PARAM, p64.detach(), p32.detach()),
                                      ("exp_avg", nat.PPO_EXP_AVG, st64["exp_avg"], st32["exp_avg"]),
                                      ("exp_avg_sq", nat.PPO_EXP_AVG_SQ, st64["exp_avg_sq"], st32["exp_avg_sq"])):
                RF.check_rule(f"adam{step}-{case}/{what}.{key}", got[w][key], a64.numpy(), a32.numpy(), REPORT)


def test_epoch_is_its_minibatches_bit_for_bit_and_repeats(zenv_mod):
    Z = zenv_mod
    s = _setup(Z, "cm")
    env = s["env"]
    order = s["kept"][np.random.default_rng(5).permutation(len(s["kept"]))].astype(np.int32)
    bs = 40
    assert len(order) % bs != 0                               # a short last minibatch
    runs = []
    for mode in ("epoch", "steps", "epoch"):
        D.dy_init(s)
        if mode == "epoch":
            env.diayn_epoch(order, bs)
            stats = env.diayn_stats()
        else:
            rows = []
            for lo in range(0, len(order), bs):
                env.diayn_minibatch(order[lo:lo + bs], apply=True)
                rows.append(env.diayn_stats()[0])
            stats = np.stack(rows)
        runs.append((D.arenas(env), stats, env.diayn_get_step()))
    assert runs[0][2] == runs[1][2] == (len(order) + bs - 1) // bs
    for other in runs[1:]:
        D.same(runs[0][0], other[0])
        np.testing.assert_array_equal(runs[0][1], other[1])
    # the same minibatch from the same state: the same bits, padding of the arena included
    D.dy_init(s)
    env.diayn_minibatch(order[:bs])
    first = D.grad_arena(s)
    env.diayn_minibatch(order[bs:2 * bs])
    env.diayn_minibatch(order[:bs])
    np.testing.assert_array_equal(first, D.grad_arena(s))
    # on the device: the list aliased, indexed by a permutation there
    tenv = s["tenv"]
    kept_dev = tenv.diayn_samples()
    np.testing.assert_array_equal(kept_dev.cpu().numpy(), s["kept"])
    perm = torch.as_tensor(np.random.default_rng(5).permutation(len(s["kept"])), device=tenv.device)
    D.dy_init(s)
    tenv.diayn_epoch(kept_dev[perm].contiguous(), bs)
    D.same(runs[0][0], D.arenas(env))


def test_sample_list_on_the_collection_and_on_planted_masks(zenv_mod):
    Z = zenv_mod
    s = _setup(Z, "tsp", "-masks", plant=False)
    env, mask = s["env"], s["lo_t"]["mask"]
    kept = env.diayn_samples()
    assert kept.dtype == np.int32
    np.testing.assert_array_equal(kept, s["kept"])
    np.testing.assert_array_equal(kept, R.kept_samples_loops(s["lo"]["mask"]))
    assert env.field_bytes(Z.F_DIAYN_SAMPLES) == 4 * len(kept)
    saved = mask.clone()
    try:
        mask[:] = 1.0
        D.refresh(s)
        np.testing.assert_array_equal(env.diayn_samples(), np.arange(N * (T - 1)))
        mask[3, 1] = 0.0
        mask[5, T - 1] = 0.0
        mask[7, 0] = 0.0                                   # frame 0's flag is nobody's
        D.refresh(s)
        want = np.setdiff1d(np.arange(N * (T - 1)), [3 * (T - 1), 5 * (T - 1) + T - 2])
        np.testing.assert_array_equal(env.diayn_samples(), want)
        np.testing.assert_array_equal(s["kept"], want)
        mask[:] = 0.0
        D.refresh(s)
        assert len(env.diayn_samples()) == 0 and env.field_bytes(Z.F_DIAYN_SAMPLES) == 0
        # nothing kept: the update calls refuse, diayn_update skips and logs nan
        D.dy_init(s)
        idx = np.zeros(4, np.int32)
        assert _rc(Z, "zenv_diayn_minibatch", env._h, idx.ctypes.data, 4, 0, 0) == Z.E_STATE
        assert _rc(Z, "zenv_diayn_epoch", env._h, idx.ctypes.data, 4, 2, 0) == Z.E_STATE
        before = D.arenas(env)
        logs = env.diayn_update(2, 32, np.random.default_rng(0))
        assert R.isnan(logs["loss"]) and R.isnan(env.diayn_logs()["loss"]) and env.diayn_get_step() == 0
        D.same(before, D.arenas(env))
    finally:
        mask.copy_(saved)
        D.refresh(s)
    np.testing.assert_array_equal(env.diayn_samples(), s["kept"])


@pytest.mark.parametrize("how", ["keep_flag", "skill_low", "skill_high", "device_index"])
def test_a_dropped_sample_adds_nothing_and_is_reported_once(zenv_mod, how):
    Z = zenv_mod
    s = _setup(Z, "cm")
    env, tenv = s["env"], s["tenv"]
    idx = D.dy_indexes(s, 33, 2).astype(np.int32)
    victim = 7
    e, f = int(idx[victim]) // (T - 1), int(idx[victim]) % (T - 1)
    rest = np.delete(idx, victim)
    scale = len(rest) / len(idx)                             # the means still divide by count
    ref = D.dy_ref_pair(s, s["sd"], rest, scale)
    D.dy_init(s)
    env.sync()
    sk, mk = s["lo_t"]["skill"], s["lo_t"]["mask"]
    saved = (sk[e, f].clone(), mk[e, f + 1].clone())
    try:
        if how == "keep_flag":
            mk[e, f + 1] = 0.0
        elif how == "skill_low":
            sk[e, f] = -1
        elif how == "skill_high":
            sk[e, f] = s["S"]
        torch.cuda.synchronize()
        if how == "device_index":
            bad = idx.copy()
            bad[victim] = N * (T - 1)
            assert _rc(Z, "zenv_diayn_minibatch", env._h, bad.ctypes.data, len(bad), 0, 0) == Z.E_ARG    # on the host
            tenv.diayn_minibatch(torch.as_tensor(bad, device=tenv.device))
        else:
            if how == "keep_flag":                           # the list is taken again: the collection still keeps others
                assert int(idx[victim]) not in env.diayn_samples()
            env.diayn_minibatch(idx)
        with pytest.raises(Z.ZenvError) as err:
            env.sync()
        assert err.value.code == Z.E_ARG
        env.sync()                                           # once
        D.dy_compare(Z, s, ref, f"drop-{how}", REPORT)
        assert np.all(np.isfinite(D.grad_arena(s)))
    finally:
        sk[e, f], mk[e, f + 1] = saved
        torch.cuda.synchronize()


@pytest.mark.parametrize("S", [1, 5])
def test_prior(zenv_mod, S):
    Z = zenv_mod
    if S == 5:
        s = _setup(Z, "tsp")
    else:
        if "tsp-S1" not in _SETUPS:
            _SETUPS["tsp-S1"] = D.dy_setup(Z, Z.config_for_id("PointTSP-v0", num_steps=10), 32, N, 1, seed=4, T=T, L=L)
        s = _SETUPS["tsp-S1"]
    env = s["env"]
    actions = s["hi"]["action"]
    assert len(actions) == N * T // L and actions.min() >= 0 and actions.max() < S
    logits0 = (0.3 * np.arange(S) - 0.2).astype(np.float32)
    env.diayn_init(s["sd"], S, prior_logits=logits0)
    np.testing.assert_array_equal(env.diayn_prior_logits(), logits0)
    refs = {dt: R.PriorRef(logits0, dt) for dt in (F64, F32)}
    for step in range(1, 11):
        got = env.diayn_prior_update()
        want = {dt: ref.step(actions) for dt, ref in refs.items()}
        if step in (1, 2, 10):
            RF.check_rule(f"prior{step}-S{S}/logits", got, want[F64], want[F32], REPORT)
    if S == 1:
        np.testing.assert_array_equal(got, logits0)         # the gradient is exactly 0
        return
    assert np.any(got != logits0)
    # the counts are the histogram of the picks: one step from zero moments moves logit s by -lr sign(p_s - count_s / M)
    env.diayn_init(s["sd"], S, prior_logits=np.zeros(S, np.float32))
    g = R.prior_gradient(np.zeros(S), actions, S)
    np.testing.assert_array_equal(np.bincount(actions, minlength=S), np.round((1.0 / S - g) * len(actions)))
    moved = env.diayn_prior_update()
    np.testing.assert_allclose(moved, -1e-2 * np.sign(g), rtol=0, atol=1e-6)
    # a pick outside [0, S) is dropped and flagged
    hi_a = s["hi_t"]["action"]
    saved = hi_a[2].clone()
    try:
        hi_a[2] = S
        torch.cuda.synchronize()
        env.diayn_init(s["sd"], S, prior_logits=np.zeros(S, np.float32))
        assert _rc(Z, "zenv_diayn_prior_update", env._h) == Z.E_ARG
        env.sync()
        dropped = np.delete(actions, 2)
        g2 = R.prior_gradient(np.zeros(S), dropped, S) + np.bincount(dropped, minlength=S) * (1.0 / len(dropped)
                                                                                           - 1.0 / len(actions))
        np.testing.assert_allclose(env.diayn_prior_logits(), -1e-2 * np.sign(g2), rtol=0, atol=1e-6)
    finally:
        hi_a[2] = saved
        torch.cuda.synchronize()


def test_publish_changes_the_next_collection_as_a_hand_load_does(zenv_mod):
    Z = zenv_mod
    env_id, h, S = CASES["cm"]

    def run(publish):
        s = D.dy_setup(Z, Z.config_for_id(env_id, num_steps=10), h, N, S, seed=1, T=T, L=L)
        env = s["env"]
        try:
            before = s["lo"]["diversity"].copy()
            D.dy_init(s, lr=1e-2)
            env.diayn_epoch(s["kept"], 64)
            read_back = env.diayn_tensors()
            if publish:
                env.diayn_publish()
            else:
                env.load_skill_inverse(read_back)
            lo, _, _, _ = env.collect_skills(T, policy_seed=9, diversity_coef=0.1, skill_prior_logits=s["prior"])
            return before, lo["diversity"].copy(), read_back
        finally:
            env.close()

    b1, after_publish, t1 = run(True)
    b2, after_load, t2 = run(False)
    np.testing.assert_array_equal(b1, b2)
    D.same(t1, t2)
    np.testing.assert_array_equal(after_publish, after_load)
    assert np.any(after_publish != 0)
    # the acting discriminator before the update gives another reward on the same frames
    s = D.dy_setup(Z, Z.config_for_id(env_id, num_steps=10), h, N, S, seed=1, T=T, L=L)
    try:
        lo, _, _, _ = s["env"].collect_skills(T, policy_seed=9, diversity_coef=0.1, skill_prior_logits=s["prior"])
        assert np.any(lo["diversity"] != after_publish)
    finally:
        s["env"].close()


def test_state_guards(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    from tests import hier_ref, option_ref, skppo_update_dev
    cfg = Z.config_for_id("PointTSP-v0", num_steps=10)
    idx = np.zeros(4, np.int32)
    n = C.c_int64()

    def refused(env, code=Z.E_STATE):
        assert _rc(Z, "zenv_diayn_minibatch", env._h, idx.ctypes.data, 4, 0, 0) == code
        assert _rc(Z, "zenv_diayn_epoch", env._h, idx.ctypes.data, 4, 2, 0) == code

    s = _setup(Z, "tsp", "-guards")
    env = s["env"]
    # before init
    refused(env)
    assert _rc(Z, "zenv_diayn_apply", env._h) == Z.E_STATE
    assert _rc(Z, "zenv_diayn_prior_update", env._h) == Z.E_STATE
    assert _rc(Z, "zenv_diayn_samples", env._h, C.byref(n)) == 0 and n.value == len(s["kept"])    # needs no learner
    assert env.field_bytes(Z.F_DIAYN_STATS) == 0
    D.dy_init(s)
    env.diayn_minibatch(s["kept"][:8])
    assert env.field_bytes(Z.F_DIAYN_STATS) == 24
    # a learner with another S
    other = D.random_inverse_state_dict(s["F"], 3, h=16, seed=0)
    env.diayn_init(other, 3, prior_logits=np.zeros(3, np.float32))
    refused(env)
    assert _rc(Z, "zenv_diayn_prior_update", env._h) == Z.E_STATE
    # a failed init leaves no learner
    with pytest.raises(Z.ZenvError):
        env.diayn_init(s["sd"], s["S"], max_batch=0)
    D.dy_init(s)
    # the skills agent's learners run beside it on the same handle
    skppo_update_dev.sk_init(dict(s, sd={"hi": s["hi_sd"], "lo": s["lo_sd"]}, total={"lo": N * T, "hi": N * T // L}))
    env.skppo_minibatch(0, np.arange(16, dtype=np.int32))
    env.diayn_minibatch(s["kept"][:8])
    env.sync()
    assert np.all(np.isfinite(env.skppo_stats(0))) and np.all(np.isfinite(env.diayn_stats()))
    # T = 1
    env.configure_skills(1)
    env.collect_skills(1, policy_seed=3, diversity_coef=0.0, skill_prior_logits=s["prior"])
    refused(env)
    assert _rc(Z, "zenv_diayn_samples", env._h, C.byref(n)) == Z.E_STATE
    # another collector's records
    env.load_options(Z.option_tensors_from_state_dicts(*option_ref.random_state_dicts(s["F"], s["S"], h=16, seed=1)))
    env.collect_options(T, policy_seed=2)
    refused(env)
    assert _rc(Z, "zenv_diayn_samples", env._h, C.byref(n)) == Z.E_STATE
    assert _rc(Z, "zenv_diayn_prior_update", env._h) == Z.E_STATE
    # Zone-goals and xy-goals records
    for kind in ("hier", "xy"):
        e2 = Z.ZoneVecEnv(cfg, N)
        try:
            e2.build_bank(11, N)
            e2.schedule_sequential()
            if kind == "hier":
                e2.enable_goals()
            e2.reset()
            e2.diayn_init(s["sd"], s["S"], prior_logits=np.zeros(s["S"], np.float32))
            if kind == "hier":
                e2.load_hier(Z.hier_tensors_from_state_dicts(*hier_ref.random_state_dicts(s["F"], h=16, seed=1)))
                e2.collect_hier(T, policy_seed=2)
            else:
                from tests import xy_ref
                e2.load_xy(Z.xy_tensors_from_state_dicts(*xy_ref.random_state_dicts(s["F"], h=16, seed=1)), skill_len=L)
                e2.collect_xy(T, policy_seed=2)
            refused(e2)
            assert _rc(Z, "zenv_diayn_prior_update", e2._h) == Z.E_STATE
        finally:
            e2.close()
    assert nat.F_DIAYN_SAMPLES == 84
