"""CPU: the C boundary of DIAYN's inverse-model learner and skill prior (zenv_diayn_*) -- the symbols, the field numbers,
the argument checks, which need no device, and the arena's names and order (InverseModel's parameters() order)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import diayn_update_ref as R
from tests.skill_collect_ref import random_inverse_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("zenv_diayn_check", "zenv_diayn_init", "zenv_diayn_tensor", "zenv_diayn_read", "zenv_diayn_write",
             "zenv_diayn_get_step", "zenv_diayn_set_step", "zenv_diayn_samples", "zenv_diayn_minibatch",
             "zenv_diayn_apply", "zenv_diayn_epoch", "zenv_diayn_prior_init", "zenv_diayn_prior_update",
             "zenv_diayn_prior_read", "zenv_diayn_prior_write")


def _weights(Z, F, h, drop=(), zone_feat=None, S=5, precision=None):
    nat = Z._native
    t = Z.inverse_tensors_from_state_dict(random_inverse_state_dict(F, S, h=h, seed=2), S)
    w = nat.SkillInverseWeights(h_dim=h, n_skills=S, zone_feat=F if zone_feat is None else zone_feat,
                                precision=nat.MLP_F32 if precision is None else precision)
    keep = {}
    for name, a in t.items():
        if name not in drop:
            keep[name] = a = np.ascontiguousarray(a, np.float32)
            setattr(w, name, a.ctypes.data)
    return w, keep


def _config(Z, **kw):
    d = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.0, entropy_coef=0.0, value_loss_coef=0.0, max_grad_norm=math.inf,
             max_batch=64, distributional_value=0)
    d.update(kw)
    return Z._native.PpoConfig(**d)


def _check(Z, cfg, w, pc):
    return Z._native.lib().zenv_diayn_check(C.byref(cfg), C.byref(w), C.byref(pc))


def test_symbols_fields_and_header(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    text = open(os.path.join(ROOT, "include", "zenv.h")).read()
    for name in FUNCTIONS:
        assert f"int {name}(" in text
        assert hasattr(nat.lib(), name)
    assert (nat.F_DIAYN_STATS, nat.F_DIAYN_SAMPLES) == (83, 84) == (Z.F_DIAYN_STATS, Z.F_DIAYN_SAMPLES)
    assert "ZENV_F_DIAYN_STATS = 83" in text and "ZENV_F_DIAYN_SAMPLES = 84" in text
    assert "ZENV_F_COUNT = 85\n" in text and "Before these two fields,\n     * ZENV_F_COUNT = 83\n" in text
    assert (nat.F_OPPPO_LO_STATS, nat.F_OPPPO_HI_STATS, nat.F_PPO_STATS) == (81, 82, 74)
    assert "inverse model and skill prior are not here" not in text
    assert "updates\n * stay with the caller" not in text
    assert "zenv_skill_inverse_weights *init" in text


def test_null_arguments(zenv_mod):
    Z = zenv_mod
    lib = Z._native.lib()
    idx = np.zeros(4, np.int32)
    p, n, s = C.c_void_p(), C.c_int64(), C.c_int64()
    assert lib.zenv_diayn_init(None, None, None) == Z.E_ARG
    assert lib.zenv_diayn_check(None, None, None) == Z.E_ARG
    assert lib.zenv_diayn_tensor(None, 0, 0, C.byref(p), C.byref(n)) == Z.E_ARG
    assert lib.zenv_diayn_get_step(None, C.byref(s)) == Z.E_ARG
    assert lib.zenv_diayn_set_step(None, 1) == Z.E_ARG
    assert lib.zenv_diayn_samples(None, C.byref(n)) == Z.E_ARG
    assert lib.zenv_diayn_minibatch(None, idx.ctypes.data, 4, 0, 0) == Z.E_ARG
    assert lib.zenv_diayn_apply(None) == Z.E_ARG
    assert lib.zenv_diayn_epoch(None, idx.ctypes.data, 4, 2, 0) == Z.E_ARG
    assert lib.zenv_diayn_read(None, 0, 0, idx.ctypes.data) == Z.E_ARG
    assert lib.zenv_diayn_write(None, 0, 0, idx.ctypes.data) == Z.E_ARG
    assert lib.zenv_diayn_prior_init(None, idx.ctypes.data, 4, 1e-2, 1e-8) == Z.E_ARG
    assert lib.zenv_diayn_prior_update(None) == Z.E_ARG
    assert lib.zenv_diayn_prior_read(None, idx.ctypes.data) == Z.E_ARG
    assert lib.zenv_diayn_prior_write(None, idx.ctypes.data) == Z.E_ARG


@pytest.mark.parametrize("env_id", ["PointTSP-v0", "ColourMatch-v0"])
def test_check_argument_rules(zenv_mod, env_id):
    Z = zenv_mod
    nat = Z._native
    cfg = Z.config_for_id(env_id)
    F = Z.zone_feat(cfg)
    ok = _config(Z)
    w, keep = _weights(Z, F, 16)
    assert _check(Z, cfg, w, ok) == 0
    for h in (0, 192):
        bad, k2 = _weights(Z, F, 16)
        bad.h_dim = h
        assert _check(Z, cfg, bad, ok) == Z.E_ARG
        assert b"h_dim" in nat.lib().zenv_last_error()
    w191, k191 = _weights(Z, F, 191, S=32)
    assert _check(Z, cfg, w191, ok) == 0
    for S in (0, 33):
        bad, k2 = _weights(Z, F, 16)
        bad.n_skills = S
        assert _check(Z, cfg, bad, ok) == Z.E_ARG
        assert b"n_skills" in nat.lib().zenv_last_error()
    for S in (1, 32):
        w_s, k_s = _weights(Z, F, 16, S=S)
        assert _check(Z, cfg, w_s, ok) == 0
    other, k3 = _weights(Z, F, 16, zone_feat=13 - F)
    assert _check(Z, cfg, other, ok) == Z.E_ARG
    assert b"zone_feat" in nat.lib().zenv_last_error()
    for name in nat.SKILL_INVERSE_TENSORS:
        bad, k2 = _weights(Z, F, 16, drop=(name,))
        assert _check(Z, cfg, bad, ok) == Z.E_ARG, name
    for precision in (nat.MLP_BF16, nat.MLP_F16):
        bad, k2 = _weights(Z, F, 16, precision=precision)
        assert _check(Z, cfg, bad, ok) == Z.E_ARG
        assert b"precision" in nat.lib().zenv_last_error()
    assert _check(Z, cfg, w, _config(Z, distributional_value=1)) == Z.E_ARG
    for name in ("lr", "adam_eps", "clip_eps", "entropy_coef", "value_loss_coef", "max_grad_norm"):
        for v in (-1e-3, math.nan, math.inf, -math.inf):
            want = 0 if (name == "max_grad_norm" and v == math.inf) else Z.E_ARG
            assert _check(Z, cfg, w, _config(Z, **{name: v})) == want, (name, v)
        assert _check(Z, cfg, w, _config(Z, **{name: 0.0})) == 0
    for mb in (0, -1):
        assert _check(Z, cfg, w, _config(Z, max_batch=mb)) == Z.E_ARG
    assert _check(Z, cfg, w191, _config(Z, max_batch=16384)) == 0
    assert _check(Z, cfg, w191, _config(Z, max_batch=2 ** 31 - 1)) == Z.E_ARG
    assert b"2^31" in nat.lib().zenv_last_error()
    limit = 2 ** 31 // (2 * 192 * cfg.num_zones)      # the two zone-row activations alone reach 2^31 floats here
    assert _check(Z, cfg, w191, _config(Z, max_batch=limit + 32)) == Z.E_ARG


@pytest.mark.parametrize("F", [6, 7])
def test_key_order_is_the_modules_parameters_order(zenv_mod, F):
    from combinatorial_rl_tasks_amd import agents
    nat = zenv_mod._native
    keys = agents.diayn_state_dict_keys()
    assert zenv_mod.diayn_state_dict_keys is agents.diayn_state_dict_keys
    assert list(keys) == list(nat.SKILL_INVERSE_TENSORS) and len(keys) == 10
    assert [f[0] for f in nat.SkillInverseWeights._fields_][4:] == list(keys)
    sd = random_inverse_state_dict(F, 5, h=16, seed=1)
    model = R.model_from(sd, F, R.torch.float32)
    assert list(keys.values()) == [k for k, _ in model.named_parameters()] == list(sd)
    shapes = agents.inverse_tensor_shapes(16, 5, F)
    for (name, key), p in zip(keys.items(), model.parameters()):
        assert shapes[name] == tuple(p.shape)


def test_python_surface(zenv_mod):
    Z = zenv_mod
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    names = ("diayn_init", "diayn_samples", "diayn_update", "diayn_stats", "diayn_logs", "diayn_prior_update",
             "diayn_prior_logits", "diayn_publish", "diayn_minibatch", "diayn_apply", "diayn_epoch", "diayn_tensors",
             "diayn_set_tensors", "diayn_state_dict", "diayn_load_state_dict", "diayn_optimizer_state",
             "diayn_load_optimizer_state", "diayn_get_step", "diayn_set_step", "diayn_tensor_ptr")
    for cls in (Z.ZoneVecEnv, TorchZoneEnv):
        for name in names:
            assert hasattr(cls, name), (cls, name)
    d = Z.ZoneVecEnv.DIAYN
    assert d["lr"] == 3e-4 and d["adam_eps"] == 1e-8 and d["max_grad_norm"] == math.inf
    assert Z.ZoneVecEnv.DIAYN_PRIOR == dict(lr=1e-2, adam_eps=1e-8)
    ex = open(os.path.join(ROOT, "examples", "skill_planner_ppo_torch.py")).read()
    assert "diayn_publish" in ex and "diayn_prior_update" in ex
