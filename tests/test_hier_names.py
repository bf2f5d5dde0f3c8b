"""CPU: the state_dict -> zenv_hier_weights name mapping of the Zone-goals agent (vec_env.hier_tensors_from_state_dicts)
and the shape of the C boundary it feeds."""
import ctypes as C

import numpy as np
import pytest

from tests import hier_ref


def test_every_tensor_is_mapped_with_its_shape(zenv_mod):
    Z = zenv_mod
    hi, lo = hier_ref.random_state_dicts(7, h=40, seed=3)
    t = Z.hier_tensors_from_state_dicts(hi, lo)
    nat = Z._native
    assert set(t) == set(nat.HIER_HI_TENSORS + nat.HIER_HI_CRITIC + nat.HIER_LO_TENSORS + nat.HIER_LO_CRITIC)
    assert t["hi_zone_w1"].shape == (40, 15) and t["lo_zone_w1"].shape == (40, 17)
    assert t["hi_comb_w"].shape == (40, 48) and t["lo_comb_w"].shape == (40, 50)
    assert t["hi_actor_w1"].shape == (40, 47) and t["hi_actor_w2"].shape == (1, 40)
    assert t["lo_mu_w"].shape == (2, 40) and t["lo_std_b"].shape == (2,)
    assert all(a.dtype == np.float32 for a in t.values())
    np.testing.assert_array_equal(t["hi_actor_w1"], hi["actor.0.weight"].numpy())
    np.testing.assert_array_equal(t["lo_enc_b"], lo["actor.enc_.0.0.bias"].numpy())
    np.testing.assert_array_equal(t["lo_critic_w2"], lo["critic.2.weight"].numpy())


def test_critics_are_optional(zenv_mod):
    hi, lo = hier_ref.random_state_dicts(6, h=16, critics=False)
    t = zenv_mod.hier_tensors_from_state_dicts(hi, lo)
    assert not any("critic" in k for k in t)


def test_missing_key_is_named(zenv_mod):
    hi, lo = hier_ref.random_state_dicts(6, h=16)
    del lo["actor.std_.bias"]
    with pytest.raises(ValueError, match=r"lo_model_state has no 'actor.std_.bias'"):
        zenv_mod.hier_tensors_from_state_dicts(hi, lo)


def test_misshaped_tensor_is_named(zenv_mod):
    hi, lo = hier_ref.random_state_dicts(6, h=16)
    hi["actor.0.weight"] = hi["actor.0.weight"][:, :-1]
    with pytest.raises(ValueError, match=r"hi_model_state\['actor.0.weight'\] has shape \(16, 21\), expected \(16, 22\)"):
        zenv_mod.hier_tensors_from_state_dicts(hi, lo)
    hi, lo = hier_ref.random_state_dicts(6, h=16)
    lo["env_model.zone_net_.0.weight"] = lo["env_model.zone_net_.0.weight"][:, 2:]      # no goal columns
    with pytest.raises(ValueError, match="zone_net_.0.weight"):
        zenv_mod.hier_tensors_from_state_dicts(hi, lo)


def test_struct_and_constants(zenv_mod):
    nat = zenv_mod._native
    n_ptr = len(nat.HIER_HI_TENSORS + nat.HIER_HI_CRITIC + nat.HIER_LO_TENSORS + nat.HIER_LO_CRITIC)
    assert C.sizeof(nat.HierWeights) == 16 + 8 * n_ptr
    assert (zenv_mod.POLICY_HIER_SAMPLE, zenv_mod.POLICY_HIER_MEAN) == (4, 5)
    assert (zenv_mod.F_HIER_LOGITS, zenv_mod.F_HIER_VALUE) == (36, 37)
