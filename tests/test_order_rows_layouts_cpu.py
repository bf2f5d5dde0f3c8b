"""CPU: the layouts of tests/order_rows_cases.py do on the CPU oracle what the GPU tests rely on -- some envs visit a
zone of their route inside a 6-step window, and every env ends an episode (time limit, num_steps = 4) and is reset
inside it -- whatever the actions are.  So a GPU test that asserts "a visit and an auto-reset happened in what I
compared" asserts something these layouts guarantee."""
import numpy as np
import pytest

from tests import order_rows_cases as K
from tests.helpers import oracle_config_from


@pytest.mark.parametrize("zones", K.ZONES)
@pytest.mark.parametrize("fresh", [False, True])
def test_layouts_visit_and_reset_within_six_steps(zenv_mod, oracle_mod, zones, fresh):
    Z, O = zenv_mod, oracle_mod
    cfgs = K.configs(Z, zones)
    robots, zxy, ranks, seeds = K.layouts(Z, zones)
    assert robots.shape == (K.N, 3) and zxy.shape == (K.N, zones, 2) and ranks.shape == (K.N, zones)
    assert all(sorted(r) == list(range(zones)) for r in ranks)
    rs = np.random.RandomState(1)
    visit_step = np.full(K.N, -1)
    resets = np.zeros(K.N, int)
    stale = 0
    for i in range(K.N):
        e = O.OracleEnv(oracle_config_from(O, cfgs[1 - i % 2]))
        e.reset_order(int(seeds[i]), ranks[i], fresh_first_obs=fresh)
        rob, zz = e.layout                                  # the oracle samples the layouts set_bank is given
        assert np.array_equal(rob, robots[i]) and np.array_equal(zz, zxy[i])
        assert e.order_vals().any() == fresh               # the reference's first observation: self.route = []
        for t in range(K.T):
            r, done, _, _ = e.step_order(rs.uniform(-1, 1, 2).astype(np.float32))
            if r >= 1.0 and visit_step[i] < 0:
                visit_step[i] = t
            if done:
                assert t == K.NUM_STEPS - 1 + K.NUM_STEPS * resets[i]
                left = e.route
                e.reset_order(int(seeds[i]), ranks[i], fresh_first_obs=fresh)
                resets[i] += 1
                if not fresh and left:                     # a time-limit end: the leftover route shows in the first rows
                    stale += 1
                    assert e.order_vals()[left[0]] == 1.0
    assert (visit_step[0::2] == 0).all()                   # the robot starts inside zone 0: visited on the first step
    assert (visit_step[1::2] == -1).all()                  # the plain layouts keep the robot away from every zone
    assert (resets == 1).all() and (fresh or stale == K.N)
