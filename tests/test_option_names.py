"""CPU: the state_dict -> zenv_option_weights name mapping of the variable-length Options agent
(vec_env.option_tensors_from_state_dicts), the shape of the C boundary it feeds, and the argument checks that need no
device."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import hier_ref, option_ref, skill_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_tensor_is_mapped_with_its_shape(zenv_mod):
    Z = zenv_mod
    hi, lo = option_ref.random_state_dicts(7, 5, h=40, seed=3)
    t = Z.option_tensors_from_state_dicts(hi, lo)
    nat = Z._native
    assert set(t) == set(nat.SKILL_HI_TENSORS + nat.SKILL_HI_CRITIC + nat.SKILL_LO_TENSORS + nat.SKILL_LO_CRITIC)
    assert {k: v.shape for k, v in t.items()} == Z.option_tensor_shapes(40, 5, 7)
    assert t["hi_zone_w1"].shape == (40, 15) and t["lo_zone_w1"].shape == (40, 20)
    assert t["hi_comb_w"].shape == (40, 48) and t["lo_comb_w"].shape == (40, 53)
    assert t["hi_enc_w"].shape == (40, 40) and t["hi_logit_w"].shape == (5, 40) and t["hi_logit_b"].shape == (5,)
    assert t["lo_enc_w"].shape == (40, 45) and t["lo_critic_w1"].shape == (40, 45) and t["hi_critic_w1"].shape == (40, 40)
    assert t["lo_mu_w"].shape == (3, 40) and t["lo_mu_b"].shape == (3,)
    assert t["lo_std_w"].shape == (3, 40) and t["lo_std_b"].shape == (3,)
    assert all(a.dtype == np.float32 for a in t.values())
    np.testing.assert_array_equal(t["hi_logit_w"], hi["actor.discrete_.0.weight"].numpy())
    np.testing.assert_array_equal(t["lo_mu_w"], lo["actor.mu_.weight"].numpy())
    np.testing.assert_array_equal(t["lo_std_b"], lo["actor.std_.bias"].numpy())
    np.testing.assert_array_equal(t["lo_enc_w"], lo["actor.enc_.0.0.weight"].numpy())
    np.testing.assert_array_equal(t["lo_critic_w2"], lo["critic.2.weight"].numpy())
    # everything but the four head tensors has the skill planner's shape
    sk = Z.vec_env.skill_tensor_shapes(40, 5, 7)
    assert {k for k, v in Z.option_tensor_shapes(40, 5, 7).items() if v != sk[k]} == {"lo_mu_w", "lo_mu_b", "lo_std_w",
                                                                                     "lo_std_b"}


@pytest.mark.parametrize("F,S,h", [(6, 1, 16), (7, 2, 128), (6, 32, 191)])
def test_h_s_and_f_are_inferred_from_the_shapes(zenv_mod, F, S, h):
    t = zenv_mod.option_tensors_from_state_dicts(*option_ref.random_state_dicts(F, S, h=h, seed=S))
    assert t["hi_logit_w"].shape == (S, h)
    assert t["lo_zone_w1"].shape == (h, 8 + S + F)
    assert t["lo_mu_w"].shape == (3, h)


def test_critics_are_optional(zenv_mod):
    hi, lo = option_ref.random_state_dicts(6, 3, h=16, critics=False)
    t = zenv_mod.option_tensors_from_state_dicts(hi, lo)
    assert not any("critic" in k for k in t)


def test_other_agents_checkpoints_are_refused_by_name(zenv_mod):
    Z = zenv_mod
    with pytest.raises(ValueError, match="skill_tensors_from_state_dicts"):
        Z.option_tensors_from_state_dicts(*skill_ref.random_state_dicts(6, 5, h=16))
    with pytest.raises(ValueError, match="hier_tensors_from_state_dicts"):
        Z.option_tensors_from_state_dicts(*hier_ref.random_state_dicts(6, h=16))
    # and the skill planner's loader still refuses an Options checkpoint
    with pytest.raises(ValueError, match="option_tensors_from_state_dicts"):
        Z.skill_tensors_from_state_dicts(*option_ref.random_state_dicts(6, 5, h=16))


def test_missing_and_misshaped_tensors_are_named(zenv_mod):
    hi, lo = option_ref.random_state_dicts(6, 4, h=16)
    del lo["actor.std_.bias"]
    with pytest.raises(ValueError, match=r"lo_model_state has no 'actor.std_.bias'"):
        zenv_mod.option_tensors_from_state_dicts(hi, lo)
    hi, lo = option_ref.random_state_dicts(6, 4, h=16)
    lo["actor.std_.weight"] = lo["actor.std_.weight"][:2]              # mu_ has three rows, std_ two
    with pytest.raises(ValueError, match=r"lo_model_state\['actor.std_.weight'\] has shape \(2, 16\), "
                                         r"expected \(3, 16\)"):
        zenv_mod.option_tensors_from_state_dicts(hi, lo)


def test_struct_constants_and_header(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    n_ptr = len(nat.SKILL_HI_TENSORS + nat.SKILL_HI_CRITIC + nat.SKILL_LO_TENSORS + nat.SKILL_LO_CRITIC)
    assert n_ptr == 34 and C.sizeof(nat.OptionWeights) == 16 + 8 * n_ptr
    assert C.sizeof(nat.SkillWeights) == 16 + 8 * 34                     # the skill agent's struct keeps its size
    assert [f[0] for f in nat.OptionWeights._fields_[:4]] == ["h_dim", "n_skills", "zone_feat", "precision"]
    assert (Z.POLICY_OPTION_SAMPLE, Z.POLICY_OPTION_MEAN) == (8, 9)
    assert (Z.POLICY_SKILL_SAMPLE, Z.POLICY_SKILL_MEAN) == (6, 7)
    assert (Z.F_OPTION_TERM_MU, Z.F_OPTION_TERM_STD, Z.F_OPTION_TERM_ACTION, Z.F_OPTION_TERM_PROB,
            Z.F_OPTION_ENDED) == (58, 59, 60, 61, 62)
    assert (Z.F_SKILL, Z.F_SKILL_BOOTSTRAP, Z.F_HI_COUNT) == (51, 57, 50)  # the existing numbers stay
    text = open(os.path.join(ROOT, "include", "zenv.h")).read()
    for name in ("zenv_option_load", "zenv_option_forward"):
        assert f"int {name}(" in text
        assert hasattr(nat.lib(), name)
    for s in ("ZENV_F_COUNT = 63", "ZENV_F_OPTION_TERM_MU = 58", "ZENV_F_OPTION_TERM_STD = 59",
              "ZENV_F_OPTION_TERM_ACTION = 60", "ZENV_F_OPTION_TERM_PROB = 61", "ZENV_F_OPTION_ENDED = 62",
              "ZENV_POLICY_OPTION_SAMPLE = 8", "ZENV_POLICY_OPTION_MEAN = 9"):
        assert s in text, s
    # the struct's fields in the header's order
    body = text[text.index("typedef struct zenv_option_weights"):text.index("} zenv_option_weights;")]
    ptrs = [f[0] for f in nat.OptionWeights._fields_[4:]]
    at = [body.index(f"*{p}") for p in ptrs]
    assert at == sorted(at)
    ints = [body.index(f"int32_t {f[0]};") for f in nat.OptionWeights._fields_[:4]]
    assert ints == sorted(ints) and ints[-1] < at[0]


def test_argument_checks_without_a_device(zenv_mod):
    Z = zenv_mod
    lib = Z._native.lib()
    # a null handle / null weights are refused before anything touches a device
    assert lib.zenv_option_load(None, None) == Z.E_ARG
    assert lib.zenv_option_forward(None) == Z.E_ARG
    w = Z._native.OptionWeights(h_dim=16, n_skills=3, zone_feat=6, precision=Z._native.MLP_F32)
    assert lib.zenv_option_load(None, C.byref(w)) == Z.E_ARG
    with pytest.raises(ValueError, match="precision"):
        Z.ZoneVecEnv.load_options(None, {}, precision="bf16")
