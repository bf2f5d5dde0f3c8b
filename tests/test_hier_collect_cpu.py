"""CPU: the host side of ZoneVecEnv.collect_hier -- the names, shapes and dtypes of the lo_exps / hi_exps buffers it
hands out, the field ids and prototype of the C boundary, and the argument checks made before the library is called."""
import numpy as np
import pytest


def test_layout_names_shapes_and_fields(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    lo, hi = Z.hier_experience_layout(7, 25, 6, 12, 30)
    assert set(lo) == {"obs", "zone_obs", "goal", "action", "log_prob", "value", "advantage", "returnn", "reward",
                       "env_reward", "mask"}
    assert lo["obs"] == (nat.F_EXP_OBS, (12, 7, 8), np.float32)
    assert lo["zone_obs"] == (nat.F_EXP_ZONE_OBS, (12, 7, 25, 6), np.float32)
    assert lo["goal"] == (nat.F_LO_GOAL, (12, 7, 2), np.float32)
    assert lo["log_prob"][1] == (12, 7, 2) and lo["reward"][0] == nat.F_EXP_REWARD
    assert lo["env_reward"] == (nat.F_LO_ENV_REWARD, (12, 7), np.float32)
    assert set(hi) == {"obs", "zone_obs", "action", "action_mask", "value", "log_prob", "advantage", "returnn",
                       "reward", "mask"}
    assert hi["obs"] == (nat.F_HI_OBS, (30, 8), np.float32)
    assert hi["zone_obs"] == (nat.F_HI_ZONE_OBS, (30, 25, 6), np.float32)
    assert hi["action"] == (nat.F_HI_ACTION, (30,), np.int32)
    assert hi["action_mask"] == (nat.F_HI_ACTION_MASK, (30, 25), np.uint8)
    assert all(hi[k][1] == (30,) for k in ("value", "log_prob", "advantage", "returnn", "reward", "mask"))
    # the [N, T-1, ...] view collect_hier hands out of a time-major buffer is the reference's lo_exps order
    T, N = 5, 3
    a = np.arange(T * N * 2, dtype=np.float32).reshape(T, N, 2)
    view = a[:T - 1].swapaxes(0, 1)
    flat = np.ascontiguousarray(view).reshape(N * (T - 1), 2)
    assert np.array_equal(flat, [a[i, j] for j in range(N) for i in range(T - 1)])   # for j: for i < T-1


def test_field_ids_and_prototype(zenv_mod):
    Z = zenv_mod
    nat = Z._native
    assert (Z.F_LO_GOAL, Z.F_LO_ENV_REWARD, Z.F_HI_OBS, Z.F_HI_COUNT) == (38, 39, 40, 50)
    assert (Z.F_HI_REWARD, Z.F_HI_MASK) == (48, 49)
    assert "zenv_collect_hier" in nat.exported_symbols()
    fn = nat.lib().zenv_collect_hier
    assert len(fn.argtypes) == 7


@pytest.mark.parametrize("bad", [dict(frames_per_proc=1), dict(frames_per_proc=0), dict(frames_per_proc=2.5),
                                 dict(frames_per_proc=True), dict(discount=1.5), dict(gae_lambda=-0.1),
                                 dict(policy_seed=-1), dict(env_index0=2 ** 64)])
def test_argument_checks(zenv_mod, bad):
    Z = zenv_mod
    args = dict(frames_per_proc=8, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95)
    args.update(bad)
    with pytest.raises(ValueError):
        Z.check_collect_hier_args(**args)


def test_checks_come_before_the_library(zenv_mod):
    """collect_hier refuses bad arguments without touching the handle (none exists here: no GPU needed)."""
    Z = zenv_mod
    env = object.__new__(Z.ZoneVecEnv)
    with pytest.raises(ValueError, match="at least 2"):
        env.collect_hier(1)
    with pytest.raises(ValueError, match="gae_lambda"):
        env.collect_hier(16, gae_lambda=2.0)
    assert Z.check_collect_hier_args(16, 3, 4, 0.9, 0.8) == (16, 3, 4, 0.9, 0.8)
