"""The eleven learner slots of one handle -- flat PPO, the Zone-goals, xy-goals, fixed-length-skills and Options pairs,
DIAYN's inverse model, flat A2C -- are eleven learners: each answers for itself before its init, keeps its own step count
and arenas beside the others and across another family's re-init, and fills its own statistics field and no other.
4 envs, 2 zones, hidden size 8, 2 skills; the only learner kernel that runs is one flat PPO minibatch."""
import numpy as np
import pytest

from tests import hier_ref, option_ref, ppo_update_ref, skill_collect_ref, skill_ref, xy_ref

pytestmark = pytest.mark.gpu

N, ZONES, H, NS = 4, 2, 8, 2
PAIRS = ("hppo", "xyppo", "skppo", "opppo")
SLOTS = [("ppo", None)] + [(key, level) for key in PAIRS for level in (0, 1)] + [("diayn", None), ("a2c", None)]
LEVEL_2 = "level 2: 0 is the low level, 1 the high level"


def _call(env, slot, name, *args):
    key, level = slot
    return getattr(env, f"{key}_{name}")(*(() if level is None else (level,)), *args)


def _refused(Z, code, f):
    with pytest.raises(Z.ZenvError) as e:
        f()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def _expected_counts(Z, env):
    """slot -> the floats of one arena: every tensor of the slot, in its family's shape, starts on a 64-float boundary"""
    V = Z.vec_env
    F = env.zone_feat
    flat = (V.ppo_state_dict_keys(False), V.mlp_tensor_shapes(H, F))
    tensors = {("ppo", None): flat, ("a2c", None): flat,
               ("diayn", None): (V.diayn_state_dict_keys(), V.inverse_tensor_shapes(H, NS, F))}
    for key in PAIRS:
        fam = V._FAMILIES[key]
        hi_keys, lo_keys = fam.keys()
        shapes = fam.shapes(H, NS, F) if fam.skills else fam.shapes(H, F)
        tensors[(key, 0)], tensors[(key, 1)] = (lo_keys, shapes), (hi_keys, shapes)
    return {slot: sum((int(np.prod(shapes[name])) + 63) // 64 * 64 for name in keys)
            for slot, (keys, shapes) in tensors.items()}


def _init_skills(env):
    env.skppo_init(*env.sk_sds, lo=dict(max_batch=8), hi=dict(max_batch=8))


def test_eleven_slots_of_one_handle(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    assert len(SLOTS) == 11
    env = Z.ZoneVecEnv(Z.config_for_id("PointTSP-v0", num_zones=ZONES), N)
    try:
        # ---- before any init: every slot answers with its family's refusal, a level that does not exist with the levels'
        for slot in SLOTS:
            assert f"zenv_{slot[0]}_init first" in _refused(Z, Z.E_STATE, lambda: _call(env, slot, "get_step"))
        for key in PAIRS:
            assert LEVEL_2 in _refused(Z, Z.E_ARG, lambda: _call(env, (key, 2), "get_step"))
        # ---- all seven families on the one handle
        F = env.zone_feat
        sd = ppo_update_ref.random_state_dict(F, H, seed=2)
        env.sk_sds = skill_ref.random_state_dicts(F, NS, h=H, seed=5)
        env.ppo_init(sd, max_batch=8)
        env.hppo_init(*hier_ref.random_state_dicts(F, h=H, seed=3), lo=dict(max_batch=8), hi=dict(max_batch=8))
        env.xyppo_init(*xy_ref.random_state_dicts(F, h=H, seed=4), lo=dict(max_batch=8), hi=dict(max_batch=8))
        _init_skills(env)
        env.opppo_init(*option_ref.random_state_dicts(F, NS, h=H, seed=7), lo=dict(max_batch=8), hi=dict(max_batch=8))
        env.diayn_init(skill_collect_ref.random_inverse_state_dict(F, NS, h=H, seed=6), NS, max_batch=8)
        env.a2c_init(sd, max_batch=8)
        for i, slot in enumerate(SLOTS):
            _call(env, slot, "set_step", 100 + i)
        assert [_call(env, slot, "get_step") for slot in SLOTS] == [100 + i for i in range(11)]
        arenas = {slot: _call(env, slot, "tensor_ptr", nat.PPO_PARAM, -1) for slot in SLOTS}
        assert len({ptr for ptr, _ in arenas.values()}) == 11
        assert {slot: count for slot, (_, count) in arenas.items()} == _expected_counts(Z, env)
        # ---- one family's re-init leaves the other nine slots alone
        _init_skills(env)
        skills = [("skppo", 0), ("skppo", 1)]
        for i, slot in enumerate(SLOTS):
            if slot in skills:
                assert _call(env, slot, "get_step") == 0
            else:
                assert _call(env, slot, "get_step") == 100 + i
                assert _call(env, slot, "tensor_ptr", nat.PPO_PARAM, -1) == arenas[slot]
        # ---- a flat PPO minibatch fills the flat PPO statistics and no other field
        env.build_bank(500, N)
        env.schedule_sequential()
        env.load_mlp(Z.mlp_tensors_from_state_dict(sd), precision="f32")
        env.reset()
        env.collect_on_device(2)
        env.ppo_minibatch(np.arange(4, dtype=np.int32))
        env.sync()
        fields = [nat.F_PPO_STATS, *nat.HPPO_STATS_FIELDS, *nat.XYPPO_STATS_FIELDS, *nat.SKPPO_STATS_FIELDS,
                  *nat.OPPPO_STATS_FIELDS, nat.F_DIAYN_STATS, nat.F_A2C_STATS]
        assert len(set(fields)) == 11
        assert [env.field_bytes(f) for f in fields] == [6 * 4] + [0] * 10
        assert env.ppo_stats().shape == (1, 6)
    finally:
        env.close()
