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


# ------------------------------------------------------------------------------------------ the edge shapes (K.CASES)
REACHABLE = {3: {(0, 3), (1, 2), (2, 1), (3, 0)}, 1: {(0, 1), (3, 2), (2, 3), (1, 0)}, 2: {(0, 2), (2, 0)}, 0: {(0, 0)}}


def test_lead_tail_restates_the_store_grid():
    """Slot t starts t * total floats behind a 16-byte-aligned base: the floats up to the next boundary lead, what the
    whole pieces behind them leave over is the tail; a pair is reachable only with the batch's total mod 4."""
    for n, zones in K.CASES.values():
        total = 7 * n * zones
        for t in range(8):
            lead, tail = K.lead_tail(n, zones, t)
            assert 0 <= lead <= 3 and 0 <= tail <= 3 and lead <= total
            assert (t * total + lead) % 4 == 0 and (total - lead - tail) % 4 == 0
            assert (lead, tail) in REACHABLE[total % 4]
    assert K.lead_tail(1, 1, 3) == (3, 0)                   # 7 floats: three lead, exactly one whole piece
    assert [K.lead_tail(3, 5, t) for t in range(4)] == [(0, 1), (3, 2), (2, 3), (1, 0)]


def test_the_cases_reach_every_lead_and_tail_also_on_a_last_slot():
    """A condition on the inputs, not a measurement: over K.CASES and T = 1..6 the frame slots of a collection meet all
    eleven reachable (lead, tail) pairs, and each of them also on the LAST slot of a collection -- the only slot where a
    tail overrun is not overwritten by the next frame's rows (it lands in exp.action)."""
    everywhere, last = {}, {}
    for name, (n, zones) in K.CASES.items():
        for frames in range(1, 7):
            for t in range(frames):
                everywhere.setdefault(K.lead_tail(n, zones, t), (name, frames, t))
            last.setdefault(K.lead_tail(n, zones, frames - 1), (name, frames))
    want = set().union(*REACHABLE.values())
    assert len(want) == 11
    for pair in sorted(want):
        print(f"(lead, tail) = {pair}: first met at {everywhere.get(pair)}, as a last slot at {last.get(pair)}")
    assert set(everywhere) == want and set(last) == want
    # the edge cases alone leave out only total = 2 mod 4, which the N = 70 shapes bring
    edge_last = {K.lead_tail(*K.CASES[c], frames - 1) for c in K.EDGE_CASES for frames in range(1, 7)}
    assert want - edge_last == REACHABLE[2]
    assert {K.lead_tail(*K.CASES[c], frames - 1) for c in ("base15", "base5") for frames in range(1, 7)} == REACHABLE[2]


@pytest.mark.parametrize("case", K.EDGE_CASES)
@pytest.mark.parametrize("fresh", [False, True])
def test_edge_layouts_visit_and_reset_within_six_steps(zenv_mod, oracle_mod, case, fresh):
    """What test_gpu_order_edges.py relies on, for every edge shape: an even env visits zone 0 on its first step and
    again on the first step after its reset; every env is reset inside six steps.  With more than one zone the episode
    ends by its time limit on the fourth step (a stale first observation for fresh=False) unless every zone lay over
    the start.  With ONE zone the visit
    empties the route and ends the episode: an even env visits, finishes and is reset on EVERY step, and its first
    observations never show a leftover route; an odd env runs into the time limit like anywhere else."""
    Z, O = zenv_mod, oracle_mod
    n, zones = K.CASES[case]
    cfgs = K.configs(Z, zones)
    robots, zxy, ranks, seeds = K.layouts(Z, zones, n)
    assert robots.shape == (n, 3) and zxy.shape == (n, zones, 2) and ranks.shape == (n, zones)
    assert all(sorted(r) == list(range(zones)) for r in ranks)
    rs = np.random.RandomState(1)
    visits = [[] for _ in range(n)]
    dones = [[] for _ in range(n)]
    stale = np.zeros(n, int)
    for i in range(n):
        e = O.OracleEnv(oracle_config_from(O, cfgs[1 - i % 2]))
        e.reset_order(int(seeds[i]), ranks[i], fresh_first_obs=fresh)
        rob, zz = e.layout
        assert np.array_equal(rob, robots[i]) and np.array_equal(zz, zxy[i])
        assert e.order_vals().any() == fresh
        for t in range(K.T):
            r, done, _, _ = e.step_order(rs.uniform(-1, 1, 2).astype(np.float32))
            if r >= 1.0:
                visits[i].append(t)
            if done:
                dones[i].append(t)
                left = e.route
                e.reset_order(int(seeds[i]), ranks[i], fresh_first_obs=fresh)
                if not fresh and left:
                    stale[i] += 1
                    assert e.order_vals()[left[0]] == 1.0
    for i in range(n):
        if zones == 1 and i % 2 == 0:
            assert visits[i] == dones[i] == list(range(K.T)) and stale[i] == 0
        elif i % 2 == 0:
            # zone 0 on the first step and on the first one after the reset; the pinned layouts switch the keep-outs
            # off, so a later zone may lie over the start too and is visited on the steps behind
            first = [t for t in visits[i] if t <= dones[i][0]]
            assert first[0] == 0 and dones[i][0] + 1 in visits[i]
            assert dones[i][0] == (K.NUM_STEPS - 1 if len(first) < zones else first[-1])
            assert fresh or len(first) == zones or stale[i] >= 1
        else:
            assert visits[i] == [] and dones[i] == [K.NUM_STEPS - 1] and (fresh or stale[i] == 1)
