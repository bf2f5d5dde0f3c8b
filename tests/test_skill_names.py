"""CPU: the state_dict -> zenv_skill_weights name mapping of the fixed-length-skills agent
(vec_env.skill_tensors_from_state_dicts), the shape of the C boundary it feeds, and the argument checks that need no
device."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import hier_ref, skill_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_tensor_is_mapped_with_its_shape(zenv_mod):
    Z = zenv_mod
    hi, lo = skill_ref.random_state_dicts(7, 5, h=40, seed=3)
    t = Z.skill_tensors_from_state_dicts(hi, lo)
    nat = Z._native
    assert set(t) == set(nat.SKILL_HI_TENSORS + nat.SKILL_HI_CRITIC + nat.SKILL_LO_TENSORS + nat.SKILL_LO_CRITIC)
    assert t["hi_zone_w1"].shape == (40, 15) and t["lo_zone_w1"].shape == (40, 20)
    assert t["hi_comb_w"].shape == (40, 48) and t["lo_comb_w"].shape == (40, 53)
    assert t["hi_enc_w"].shape == (40, 40) and t["hi_logit_w"].shape == (5, 40) and t["hi_logit_b"].shape == (5,)
    assert t["lo_enc_w"].shape == (40, 45) and t["lo_critic_w1"].shape == (40, 45) and t["hi_critic_w1"].shape == (40, 40)
    assert t["lo_mu_w"].shape == (2, 40) and t["lo_std_b"].shape == (2,)
    assert all(a.dtype == np.float32 for a in t.values())
    np.testing.assert_array_equal(t["hi_logit_w"], hi["actor.discrete_.0.weight"].numpy())
    np.testing.assert_array_equal(t["hi_enc_b"], hi["actor.enc_.0.0.bias"].numpy())
    np.testing.assert_array_equal(t["lo_enc_w"], lo["actor.enc_.0.0.weight"].numpy())
    np.testing.assert_array_equal(t["lo_critic_w2"], lo["critic.2.weight"].numpy())


@pytest.mark.parametrize("F,S,h", [(6, 1, 16), (7, 2, 128), (6, 32, 191)])
def test_h_and_s_are_inferred_from_the_shapes(zenv_mod, F, S, h):
    t = zenv_mod.skill_tensors_from_state_dicts(*skill_ref.random_state_dicts(F, S, h=h, seed=S))
    assert t["hi_logit_w"].shape == (S, h)
    assert t["lo_zone_w1"].shape == (h, 8 + S + F)


def test_critics_are_optional(zenv_mod):
    hi, lo = skill_ref.random_state_dicts(6, 3, h=16, critics=False)
    t = zenv_mod.skill_tensors_from_state_dicts(hi, lo)
    assert not any("critic" in k for k in t)


def test_zone_goals_checkpoint_is_refused(zenv_mod):
    hi, lo = hier_ref.random_state_dicts(6, h=16)
    with pytest.raises(ValueError, match="Zone-goals checkpoint"):
        zenv_mod.skill_tensors_from_state_dicts(hi, lo)


def test_missing_and_misshaped_tensors_are_named(zenv_mod):
    hi, lo = skill_ref.random_state_dicts(6, 4, h=16)
    del hi["actor.discrete_.0.bias"]
    with pytest.raises(ValueError, match=r"hi_model_state has no 'actor.discrete_.0.bias'"):
        zenv_mod.skill_tensors_from_state_dicts(hi, lo)
    hi, lo = skill_ref.random_state_dicts(6, 4, h=16)
    lo["env_model.zone_net_.0.weight"] = lo["env_model.zone_net_.0.weight"][:, 1:]      # one skill column short
    with pytest.raises(ValueError, match=r"lo_model_state\['env_model.zone_net_.0.weight'\] has shape \(16, 17\), "
                                         r"expected \(16, 18\)"):
        zenv_mod.skill_tensors_from_state_dicts(hi, lo)
    hi, lo = skill_ref.random_state_dicts(6, 4, h=16)
    lo["actor.enc_.0.0.weight"] = lo["actor.enc_.0.0.weight"][:, :16]                   # no skill columns
    with pytest.raises(ValueError, match="actor.enc_.0.0.weight"):
        zenv_mod.skill_tensors_from_state_dicts(hi, lo)


def test_struct_constants_and_header(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    n_ptr = len(nat.SKILL_HI_TENSORS + nat.SKILL_HI_CRITIC + nat.SKILL_LO_TENSORS + nat.SKILL_LO_CRITIC)
    assert n_ptr == 34 and C.sizeof(nat.SkillWeights) == 16 + 8 * n_ptr
    assert (Z.POLICY_SKILL_SAMPLE, Z.POLICY_SKILL_MEAN) == (6, 7)
    assert (Z.F_SKILL, Z.F_SKILL_AGE, Z.F_SKILL_LOGITS, Z.F_SKILL_VALUE) == (51, 52, 53, 54)
    assert (Z.F_HIER_LOGITS, Z.F_HI_COUNT) == (36, 50)          # the existing numbers stay
    text = open(os.path.join(ROOT, "include", "zenv.h")).read()
    for name in ("zenv_skill_load", "zenv_skill_configure", "zenv_set_skills", "zenv_skill_forward"):
        assert f"int {name}(" in text
        assert hasattr(nat.lib(), name)
    assert "ZENV_F_COUNT = 55" in text and "ZENV_POLICY_SKILL_MEAN = 7" in text
    # the struct's fields in the header's order
    body = text[text.index("typedef struct zenv_skill_weights"):text.index("} zenv_skill_weights;")]
    ptrs = [f[0] for f in nat.SkillWeights._fields_[4:]]
    at = [body.index(f"*{p}") for p in ptrs]
    assert at == sorted(at)


def test_argument_checks_without_a_device(zenv_mod):
    Z = zenv_mod
    lib = Z._native.lib()
    # a null handle / null weights are refused before anything touches a device
    assert lib.zenv_skill_load(None, None) == Z.E_ARG
    assert lib.zenv_skill_configure(None, 200) == Z.E_ARG
    assert lib.zenv_set_skills(None, None) == Z.E_ARG
    assert lib.zenv_skill_forward(None) == Z.E_ARG
    with pytest.raises(ValueError, match="precision"):
        Z.ZoneVecEnv.load_skills(None, {}, precision="bf16")
