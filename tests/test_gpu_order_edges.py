"""Solver-ordered handles (TSPOrderEnv; K7 k_order_reset / k_order_step, K22 k_order_rows, the 7-wide zenv_collect and
the flat learner at F = 7) at their alignment, zone-count and batch edges.  Shapes: tests/order_rows_cases.py CASES;
tests/test_order_rows_layouts_cpu.py shows on the CPU that their frame slots meet every (lead, tail) pair of K22's
16-byte store grid, each also on a last slot, and that the layouts visit and reset as the tests here assert.

Everything the env or K22 produces is compared bit for bit: with a twin handle driven by zenv_step, or with the CPU
oracle.  No bound is new:
  network outputs   MLP_BOUND of test_gpu_order_rows.py::test_network_on_the_seven_wide_rows_matches_torch, on that
                    test's weight family (_tensors)
  learner           ppo_update_ref.check_rule on ppo_update_dev.decided_samples with the 85 % floor, as
                    test_gpu_order_rows_update.py::test_one_minibatch_without_a_step
  episode logs      2.4e-7 of test_gpu_order_rows.py::test_episode_logs_sum_the_env_reward_and_the_shaped_one (a sum of
                    four float32 terms of magnitude at most 1)

A waiting env -- finished under auto_reset=False and stepped again -- is WaitWrapper.step's (wrappers.py:34-50): zero
observation, the order column included, reward 0, done, no shaped reward; its route stays what the finishing step left."""
import numpy as np
import pytest

from tests import order_rows_cases as K
from tests import test_gpu_order_rows as B
from tests.helpers import oracle_config_from

pytestmark = pytest.mark.gpu

KERNELS = ("lane", "wave")


def _kernel(Z, kern):
    return {"kernel": Z._native.KERNEL_WAVE_PER_ENV} if kern == "wave" else {}


def _make(Z, case, fresh=False, kern="lane", num_steps=K.NUM_STEPS):
    n, zones = K.CASES[case]
    return K.make_env(Z, zones, fresh=fresh, n=n, num_steps=num_steps, **_kernel(Z, kern))


def _oracles(Z, O, case, fresh, num_steps=K.NUM_STEPS):
    """The CPU oracle's envs on the layouts of the case, reset as the handle is."""
    n, zones = K.CASES[case]
    cfgs = [oracle_config_from(O, c) for c in K.configs(Z, zones, num_steps)]
    robots, zxy, ranks, seeds = K.layouts(Z, zones, n)
    refs = [O.OracleEnv(cfgs[1 - i % 2]) for i in range(n)]
    for i, e in enumerate(refs):
        e.reset_order(int(seeds[i]), ranks[i], fresh_first_obs=fresh)
        assert np.array_equal(e.layout[1], zxy[i])
    return refs, ranks, seeds


def _route(pos_row):
    return [int(z) for z in np.argsort(pos_row, kind="stable") if pos_row[z] >= 0]


def _rows_three_ways(Z, env, tenv, tag):
    """get(F_ORDER_ROWS), TorchZoneEnv.net_rows and get_head(F_ORDER_ROWS) all hold [zone_obs row, order value]."""
    n = env.num_envs
    want = K.want_rows(env, Z)
    assert want.shape == (n, env.num_zones, 7)
    assert K.same_bits(env.get(Z.F_ORDER_ROWS), want), tag
    assert K.same_bits(tenv.net_rows.cpu().numpy(), want), tag
    first = n // 2
    count = min(7, n - first)
    assert K.same_bits(env.get_head(Z.F_ORDER_ROWS, count, first), want[first:first + count]), tag
    return want


# -------------------------------------------------------------------------------- 1: rows on every store alignment
def _collect_with_twin(Z, case, frames, fresh):
    """collect(frames) on one handle and the same frames on a twin that draws its own actions (zenv_policy) and steps
    with zenv_step: the twin's records, and the rows read three ways after its reset and after each of its steps."""
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    n, zones = K.CASES[case]
    env, twin = _make(Z, case, fresh), _make(Z, case, fresh)
    t = B._tensors(8 if zones < 15 else 33, seed=7)
    for e in (env, twin):
        e.load_mlp(t, precision="f32")
    x = {k: np.ascontiguousarray(v) for k, v in env.collect(frames, policy_seed=3, discount=0.99, gae_lambda=0.95).items()}
    logs = env.episode_logs()
    ttwin = TorchZoneEnv(twin)
    rec = dict(rows=[], obs=[], action=[], value=[], shaped=[], reward=[], done=[])
    for k in range(frames):
        rec["rows"].append(_rows_three_ways(Z, twin, ttwin, (case, "twin before step", k)))
        rec["obs"].append(twin.get(Z.F_OBS))
        rec["value"].append(twin.mlp_forward(with_value=True)[2])
        twin.policy(Z.POLICY_MLP_SAMPLE, policy_seed=3)
        rec["action"].append(twin.get(Z.F_ACTIONS))
        twin.step(None, auto_reset=True)
        _, _, r, done, _ = twin.results()
        rec["shaped"].append(twin.get(Z.F_SHAPED_REWARD))
        rec["reward"].append(r)
        rec["done"].append(done)
    _rows_three_ways(Z, twin, ttwin, (case, "twin after the last step"))
    rec = {k: np.stack(v, axis=1) for k, v in rec.items()}
    return dict(env=env, twin=twin, x=x, logs=logs, rec=rec, t=t)


ROWS = [(case, frames, fresh) for case in ("one", "odd15", "blocks3") for frames in range(1, 7) for fresh in (False, True)]
ROWS += [(case, frames, False) for case in ("z32", "base5") for frames in (1, 2)]      # totals 0 and 2 mod 4


@pytest.mark.parametrize("case,frames,fresh", ROWS)
def test_collected_rows_bit_for_bit_on_every_store_alignment(zenv_mod, case, frames, fresh):
    """Frame slot t of exp.zone_obs starts t * 7 * N * Z floats behind an aligned base: K22 writes `lead` floats before
    its first 16-byte piece and cuts the last piece to `tail`.  The last slot's tail ends where exp.action begins: the
    recorded actions are compared with the twin's OWN draws, so an overrun shows there."""
    from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
    Z = zenv_mod
    n, zones = K.CASES[case]
    c = _collect_with_twin(Z, case, frames, fresh)
    env, twin, x, rec = c["env"], c["twin"], c["x"], c["rec"]
    try:
        slots = [K.lead_tail(n, zones, k) for k in range(frames)]
        print(f"order edges rows {case} N={n} Z={zones} T={frames} fresh={fresh}: (lead, tail) of slots 0..{frames - 1} = "
              f"{slots}; last slot {slots[-1]}")
        assert x["zone_obs"].shape == (n, frames, zones, 7) and x["obs"].shape == (n, frames, 8)
        assert env.field_bytes(Z._native.F_EXP_ZONE_OBS) == frames * n * zones * 7 * 4
        for k in range(frames):
            assert K.same_bits(x["zone_obs"][:, k], rec["rows"][:, k]), (k, slots[k])
            assert K.same_bits(x["obs"][:, k], rec["obs"][:, k]), k
            assert K.same_bits(x["action"][:, k], rec["action"][:, k]), (k, "exp.action", slots[-1])
            assert K.same_bits(x["value"][:, k], rec["value"][:, k]), k
        assert K.same_bits(x["reward"], rec["shaped"].astype(np.float32))           # base.py:159-162
        not_done = 1.0 - rec["done"].astype(np.float32)
        assert (x["mask"][:, 0] == 1).all() and np.array_equal(x["mask"][:, 1:], not_done[:, :-1])
        # the handle ends where the twin is, and shows the same rows three ways
        for a, b in zip(env.results() + env.order_info() + (env.order_routes(),),
                        twin.results() + twin.order_info() + (twin.order_routes(),)):
            assert np.array_equal(a, b)
        final = _rows_three_ways(Z, env, TorchZoneEnv(env), (case, "after the collect"))
        assert K.same_bits(final, K.want_rows(twin, Z))
        # what was compared: a visit on the first frame, the auto-reset, a non-zero order column
        assert (rec["reward"][0::2, 0] >= 1).all()
        column = np.concatenate([x["zone_obs"][..., 6].reshape(-1), final[..., 6].reshape(-1)])
        if zones == 1:
            # one zone: the visit empties the route and ends the episode, so every frame is a visit and an auto-reset,
            # the reference's first observation shows the (empty) leftover route and the build's opt-out the new one
            assert rec["done"].all() and (rec["reward"] >= 1).all()
            assert (column == 1.0).all() if fresh else not column.any()
        else:
            assert column.any() and (fresh or not x["zone_obs"][:, 0, :, 6].any())
            if frames >= K.NUM_STEPS:
                assert rec["done"][:, K.NUM_STEPS - 1].all() and rec["shaped"][:, K.NUM_STEPS - 1].any()
                assert not np.array_equal(x["reward"], rec["reward"])
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------------ 2: K7 in lockstep with the CPU oracle
@pytest.mark.parametrize("case", ["one", "edge255", "edge256", "edge257", "z32"])
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("fresh", [False, True])
def test_order_kernels_lockstep_with_the_oracle_at_the_edge_shapes(zenv_mod, oracle_mod, case, kern, fresh):
    """The loop of test_gpu_parity.py::test_solver_ordered_variant_lockstep at num_steps = 12 for 40 steps, on both step
    kernels (K1w writes the visit_zone / term_xy K7 reads), with a masked reset of every third env after step 20."""
    Z, O = zenv_mod, oracle_mod
    n, zones = K.CASES[case]
    num_steps, steps = 12, 40
    env = _make(Z, case, fresh, kern, num_steps=num_steps)
    refs, ranks, seeds = _oracles(Z, O, case, fresh, num_steps)

    def same_order_state(tag):
        sh, val = env.order_info()
        pos = env.order_routes()
        assert np.array_equal(val, np.stack([e.order_vals() for e in refs])), tag
        for i, e in enumerate(refs):
            assert _route(pos[i]) == e.route, (tag, i)
        return sh

    assert not same_order_state("reset").any() and env.get(Z.F_ORDER_VAL).any() == fresh
    rs = np.random.RandomState(3)
    n_visits = n_limit = n_finished = n_stale = 0
    for t in range(steps):
        o, zo = env.observations()
        pos = env.order_routes()
        tgt = np.argmax(pos == 0, axis=1)                      # steer to the first zone of the remaining route, with noise
        d = zo[np.arange(n), tgt, :2] * 3.0 - o[:, 1:3] * 3.0
        ang = np.arctan2(d[:, 1], d[:, 0]) - np.arctan2(o[:, 4], o[:, 3])
        ang = (ang + np.pi) % (2 * np.pi) - np.pi
        a = np.stack([np.where(np.abs(ang) < 0.6, 1.0, 0.0), np.clip(2 * ang, -1, 1)], 1).astype(np.float32)
        a += rs.normal(0, 0.05, a.shape).astype(np.float32)
        env.step(a, auto_reset=True)
        _, _, r, dn, _ = env.results()
        sh = env.get(Z.F_SHAPED_REWARD)
        for i, e in enumerate(refs):
            r_ref, d_ref, _, sh_ref = e.step_order(a[i])
            assert (r[i], dn[i]) == (np.float32(r_ref), d_ref) and sh[i] == sh_ref, (t, i, sh[i], sh_ref)
            n_visits += r_ref >= 1.0
            if d_ref:
                left = e.route
                e.reset_order(int(seeds[i]), ranks[i], fresh_first_obs=fresh)      # penv.py:8-11
                n_limit += bool(left)
                n_finished += not left
                if not fresh and left:
                    n_stale += 1
                    assert e.order_vals()[left[0]] == 1.0 and len(e.route) == zones
        same_order_state(t)
        if t == 20:
            mask = (np.arange(n) % 3 == 0).astype(np.uint8)
            env.reset(mask)
            for i in np.nonzero(mask)[0]:
                refs[i].reset_order(int(seeds[i]), ranks[i], fresh_first_obs=fresh)
            sh = same_order_state("masked reset")
            assert not sh[mask != 0].any()
            assert np.array_equal(env.get(Z.F_OBS), np.stack([e.obs()[0] for e in refs]))
    print(f"order edges lockstep {case} {kern} fresh={fresh}: {n_visits} visits, {n_limit} time-limit ends, "
          f"{n_finished} finished tours, {n_stale} stale first observations (the oracle's counts)")
    # the oracle's own counts (the device agreed with it on every step): the pinned even envs visit on the first step of
    # every episode; with one zone that visit finishes the tour, otherwise the 12-step limit ends the odd envs' episodes
    # on steps 11, 23 and 35 (11 and 32 for those the masked reset restarted)
    even = (n + 1) // 2
    assert n_visits >= 3 * even
    if zones == 1:
        assert n_finished >= steps and n_stale == 0
    else:
        assert n_limit >= 2 * (n // 2) and (fresh or n_stale == n_limit)
    env.close()


def test_the_largest_route_reaches_position_31_and_two_to_the_minus_31(zenv_mod):
    Z = zenv_mod
    env = _make(Z, "z32", fresh=True)
    pos, val = env.order_routes(), env.get(Z.F_ORDER_VAL)
    assert pos.dtype == np.int8 and (np.sort(pos, axis=1) == np.arange(32)).all()
    assert (val == np.ldexp(np.float32(1), -pos.astype(np.int32))).all() and val.min() == np.float32(2.0 ** -31)
    assert K.same_bits(env.get(Z.F_ORDER_ROWS), K.want_rows(env, Z))
    env.close()


# ------------------------------------------------------------------------------------------------ 3: no auto-reset
@pytest.mark.parametrize("case", ["odd15", "edge257"])
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("fresh", [False, True])
def test_a_waiting_env_shows_a_zero_order_column_and_keeps_its_route(zenv_mod, oracle_mod, case, kern, fresh):
    """auto_reset=False (what evaluate() steps with) past every episode's end, five steps more, a masked reset of the
    finished envs of odd index, three steps more.  The finishing step carries the real terminal observation and its
    feature; every step behind it is WaitWrapper's: reward 0, done, shaped reward 0, F_OBS, F_ZONE_OBS and all seven
    columns of F_ORDER_ROWS zero.  order_routes() keeps the leftover route, which the masked reset's first observation
    shows (the reference's reset(), fresh=False)."""
    Z, O = zenv_mod, oracle_mod
    n, zones = K.CASES[case]
    env = _make(Z, case, fresh, kern)
    refs, ranks, seeds = _oracles(Z, O, case, fresh)
    rs = np.random.RandomState(11)
    finished = np.zeros(n, bool)
    counts = dict(waits=0, finishing=0, leftover=0)

    def step_and_compare(tag):
        a = rs.uniform(-1, 1, (n, 2)).astype(np.float32)
        kept = env.order_routes()
        env.step(a, auto_reset=False)
        obs, zo, r, dn, _ = env.results()
        sh, val = env.order_info()
        rows, pos = env.get(Z.F_ORDER_ROWS), env.order_routes()
        assert K.same_bits(rows, K.want_rows(env, Z)), tag
        for i, e in enumerate(refs):
            if finished[i]:                                           # WaitWrapper.step's else branch
                assert r[i] == 0 and dn[i] and sh[i] == 0, (tag, i, r[i], dn[i], sh[i])
                assert not obs[i].any() and not zo[i].any(), (tag, i)
                assert not rows[i].any() and not val[i].any(), (tag, i, rows[i][:, 6])
                assert np.array_equal(pos[i], kept[i]) and _route(pos[i]) == e.route, (tag, i)
                counts["waits"] += 1
                continue
            r_ref, d_ref, _, sh_ref = e.step_order(a[i])
            o_ref, zo_ref = e.obs()
            assert (r[i], dn[i]) == (np.float32(r_ref), d_ref) and sh[i] == sh_ref, (tag, i)
            assert np.array_equal(obs[i], o_ref) and np.array_equal(zo[i], zo_ref), (tag, i)
            assert np.array_equal(val[i], e.order_vals()) and _route(pos[i]) == e.route, (tag, i)
            if d_ref:
                finished[i] = True
                counts["finishing"] += 1
                counts["leftover"] += bool(val[i].any())
    for t in range(K.NUM_STEPS):
        step_and_compare(("to the end", t))
    assert finished.all() and counts["leftover"] >= n // 2               # the terminal observation keeps its feature
    for t in range(5):
        step_and_compare(("waiting", t))
    assert counts["waits"] == 5 * n
    mask = (finished & (np.arange(n) % 2 == 1)).astype(np.uint8)
    assert mask.any()
    left = {i: refs[i].route for i in np.nonzero(mask)[0]}
    env.reset(mask)
    for i in left:
        refs[i].reset_order(int(seeds[i]), ranks[i], fresh_first_obs=fresh)
        finished[i] = False
    sh, val = env.order_info()
    obs, zo = env.observations()
    pos = env.order_routes()
    stale = 0
    for i, e in enumerate(refs):
        if mask[i]:
            o_ref, zo_ref = e.obs()
            assert np.array_equal(obs[i], o_ref) and np.array_equal(zo[i], zo_ref) and sh[i] == 0, i
            assert np.array_equal(val[i], e.order_vals()) and _route(pos[i]) == e.route and len(e.route) == zones, i
            if not fresh and left[i]:
                stale += 1
                assert val[i][left[i][0]] == 1.0                        # the leftover route's first zone
        else:
            assert not obs[i].any() and not zo[i].any() and not val[i].any(), i
    assert fresh or stale == int(mask.sum())
    assert K.same_bits(env.get(Z.F_ORDER_ROWS), K.want_rows(env, Z))
    for t in range(3):
        step_and_compare(("after the masked reset", t))
    assert counts["waits"] == 5 * n + 3 * (n - int(mask.sum())) and not finished[mask != 0].any()
    print(f"order edges waiting {case} {kern} fresh={fresh}: {counts}, {stale} stale first observations")
    env.close()


# ----------------------------------------------------------------------------- 4: the network on the 7-wide rows
NET_CASES = ["one", "odd15", "z32", "edge257"]
NET_PATHS = [("bf16", None), ("f16", None), ("f32", "valu"), ("f32", "mfma"), ("bf16x3", "mfma"), ("f16x3", "mfma")]
_STEPPED = {}


def _stepped(Z, case):
    """A handle of the case past its auto-reset, shared by the network tests (they only load and evaluate).  One zone:
    the build's opt-out, the only setting in which that shape shows a non-zero order column at all."""
    if case not in _STEPPED:
        n, zones = K.CASES[case]
        env = _make(Z, case, fresh=zones == 1)
        rs = np.random.RandomState(zones)
        visits = resets = 0
        for _ in range(K.NUM_STEPS + 1):
            env.step(B._random_actions(rs, n), auto_reset=True)
            _, _, r, done, _ = env.results()
            visits, resets = visits + int((r >= 1).sum()), resets + int(done.sum())
        assert visits >= (n + 1) // 2 and resets >= n
        _STEPPED[case] = env
    return _STEPPED[case]


@pytest.fixture(scope="module", autouse=True)
def _close_stepped():
    yield
    for env in _STEPPED.values():
        env.close()
    _STEPPED.clear()


@pytest.mark.parametrize("case", NET_CASES)
@pytest.mark.parametrize("h", [1, 33, 191])
@pytest.mark.parametrize("precision,zone_part", NET_PATHS)
def test_network_on_the_seven_wide_rows_at_the_shape_edges(zenv_mod, case, h, precision, zone_part, monkeypatch):
    """Z = 1 (below the split layout's Z >= 4), Z = 32 (the runtime-Z instantiation at F = 7), N = 1 and N = 257, at
    widths 1, 33 and 191, on every path of test_gpu_order_rows.py::test_network_on_the_seven_wide_rows_matches_torch
    and, for bf16, every batch layout; that test's bounds on that test's weight family."""
    from oracle import policy_ref as P
    Z = zenv_mod
    for v in ("ZENV_MLP_F32_VALU", "ZENV_MLP_F32_MFMA", "ZENV_MLP_LAYOUT"):
        monkeypatch.delenv(v, raising=False)
    if zone_part:
        monkeypatch.setenv("ZENV_MLP_F32_VALU" if zone_part == "valu" else "ZENV_MLP_F32_MFMA", "1")
    n, zones = K.CASES[case]
    env = _stepped(Z, case)
    t = B._tensors(h, seed=zones + h)
    env.load_mlp(t, precision=precision)
    obs, rows = env.get(Z.F_OBS), K.want_rows(env, Z)
    assert K.same_bits(env.get(Z.F_ORDER_ROWS), rows) and rows[..., 6].any()
    ref = P.forward_fp32(t, obs, rows)
    bound = B.MLP_BOUND[precision]
    for layout in (None, "split", "32", "64") if precision == "bf16" else (None,):
        if layout:
            monkeypatch.setenv("ZENV_MLP_LAYOUT", layout)
        out = env.mlp_forward(with_value=True)
        for name, a, b in zip(("mu", "std", "value"), out, ref):
            err = float(np.abs(a - b).max())
            print(f"order edges net {case} {precision}/{zone_part}/{layout} h={h} {name}: max error {err:.3g} (bound {bound:g})")
            assert a.shape == b.shape and np.isfinite(a).all() and err <= bound, (name, layout, err)
        env.policy(Z.POLICY_MLP_MEAN)
        assert K.same_bits(env.get(Z.F_ACTIONS), out[0]), layout


@pytest.mark.parametrize("case,kern", [("edge257", "wave"), ("one", "lane")])
def test_rollout_samples_and_steps_as_policy_and_step_by_hand(zenv_mod, case, kern):
    Z = zenv_mod
    n, zones = K.CASES[case]
    env, twin = _make(Z, case, zones == 1, kern), _make(Z, case, zones == 1, kern)
    t = B._tensors(33, seed=6, critic=False)
    for e in (env, twin):
        e.load_mlp(t, precision="f32")
    steps = K.NUM_STEPS + 2
    env.rollout(steps, Z.POLICY_MLP_SAMPLE, policy_seed=4)
    visits = resets = 0
    for _ in range(steps):
        twin.policy(Z.POLICY_MLP_SAMPLE, policy_seed=4)
        twin.step(None, auto_reset=True)
        _, _, r, done, _ = twin.results()
        visits, resets = visits + int((r >= 1).sum()), resets + int(done.sum())
    for a, b in zip(env.results() + env.order_info() + (env.get(Z.F_ORDER_ROWS), env.order_routes(), env.get(Z.F_ACTIONS)),
                    twin.results() + twin.order_info() + (twin.get(Z.F_ORDER_ROWS), twin.order_routes(), twin.get(Z.F_ACTIONS))):
        assert K.same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b)
    assert visits >= (n + 1) // 2 and resets >= n and env.step_count == twin.step_count == steps
    assert env.get(Z.F_ORDER_ROWS)[..., 6].any()
    env.close()
    twin.close()


# ------------------------------------------------------------------------- 5: the learner on an odd-offset record
# case, frames, h, parameter seed.  odd15: 3 envs x 5 frames = 15 samples over 75 zone rows (N * T * Z * 7 = 525);
# edge257: 771 samples (80 955).  The 85 % floor of decided samples was checked on the CPU for these seeds with the two
# torch models on the oracle's observations of the same layouts under random actions: 15 of 15 and 719 of 771.
LEARN = [("odd15", 5, 8, 2), ("edge257", 3, 185, 15)]
_LEARN = {}
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _close_learners():
    import tests.ppo_update_dev as D
    yield
    for s in _LEARN.values():
        s["env"].close()
    _LEARN.clear()
    D.print_worst(REPORT, "order edges ppo update", 40)


def _learner(Z, case, frames, h, seed):
    import torch
    from combinatorial_rl_tasks_amd import agents
    from tests import ppo_update_dev as D
    from tests import ppo_update_ref as R
    if case not in _LEARN:
        n, zones = K.CASES[case]
        assert (n * frames * zones * 7) % 2 == 1                 # exp.action and all behind it: an odd float offset
        env = _make(Z, case)
        sd = R.random_state_dict(7, h, False, seed=seed)
        env.load_mlp(agents.mlp_tensors_from_state_dict(sd), precision="f32")
        exps = {k: np.ascontiguousarray(v) for k, v in env.collect(frames, policy_seed=5).items()}
        assert exps["zone_obs"].shape == (n, frames, zones, 7) and exps["zone_obs"][..., 6].any()
        assert ((exps["mask"] == 0).sum() == n) == (frames > K.NUM_STEPS)      # odd15: the auto-reset is in the record
        decided = D.decided_samples(R.model_from(sd, 7, torch.float64), R.model_from(sd, 7, torch.float32), exps)
        print(f"order edges learner {case} T={frames} h={h}: {int((~decided).sum())} of {decided.size} samples hold an "
              "undecided gate")
        assert decided.sum() >= 0.85 * decided.size
        _LEARN[case] = dict(env=env, sd=sd, exps=exps, F=7, Z=zones, h=h, N=n, T=frames, dist=False, decided=decided)
    return _LEARN[case]


@pytest.mark.parametrize("case,frames,h,seed", LEARN)
def test_learner_minibatch_over_all_decided_samples_of_an_odd_offset_record(zenv_mod, case, frames, h, seed):
    from tests import ppo_update_dev as D
    from tests import ppo_update_ref as R
    s = _learner(zenv_mod, case, frames, h, seed)
    total = s["N"] * frames
    idx = np.random.default_rng(1).permutation(total)
    idx = idx[s["decided"][idx]]
    assert len(idx) >= 0.85 * total
    D.flat_check_minibatch(zenv_mod, s, s["sd"], idx, R.HYPER, f"edge-{case}", REPORT, max_batch=total)
    assert s["env"].ppo_get_step() == 0
    g = D.flat_by_key(s["env"], zenv_mod._native.PPO_GRAD)["env_model.zone_net_.0.weight"]
    assert g.shape == (h, 15) and np.abs(g[:, 14]).max() > 0


@pytest.mark.parametrize("case,frames,h,seed", LEARN)
def test_learner_epoch_of_two_minibatches_and_the_same_bits_twice(zenv_mod, case, frames, h, seed):
    import torch
    from tests import ppo_update_dev as D
    from tests import ppo_update_ref as R
    Z = zenv_mod
    nat = Z._native
    s = _learner(Z, case, frames, h, seed)
    env = s["env"]
    total = s["N"] * frames
    size = (2 * total) // 5                                   # two minibatches of 40 % each: room to leave samples out
    env.ppo_init(s["sd"], max_batch=size, **R.HYPER)

    def state():
        return {w: env.ppo_tensors(w) for w in (nat.PPO_PARAM, nat.PPO_EXP_AVG, nat.PPO_EXP_AVG_SQ)}, env.ppo_get_step()

    start = state()
    perm = R.batch_indexes(total, frames, 0, np.random.default_rng(21))
    first = perm[s["decided"][perm]][:size]
    ref = {dt: R.RefLearner(s["sd"], 7, dt, R.HYPER) for dt in (torch.float64, torch.float32)}
    ref_stats = {dt: [ref[dt].minibatch(R.as_batch(s["exps"], first, dt))] for dt in ref}
    rest = perm[~np.isin(perm, first)]
    second = rest[D.decided_samples(ref[torch.float64].model, ref[torch.float32].model, s["exps"])[rest]][:size]
    assert len(first) == size and 0.85 * size <= len(second) <= size
    for dt in ref:
        ref_stats[dt].append(ref[dt].minibatch(R.as_batch(s["exps"], second, dt)))
    order = np.concatenate([first, second]).astype(np.int32)
    env.ppo_epoch(order, size)
    dev_stats = env.ppo_stats()
    assert dev_stats.shape == (2, 6) and env.ppo_get_step() == 2
    r64, r32 = np.array(ref_stats[torch.float64]), np.array(ref_stats[torch.float32])
    for i, name in enumerate(R.STATS):
        R.check_rule(f"edge-epoch-{case}/stat.{name}", dev_stats[:, i], r64[:, i], r32[:, i], REPORT)
    after = state()
    params = D.flat_by_key(env, nat.PPO_PARAM)
    p64, p32 = ref[torch.float64].model.state_dict(), ref[torch.float32].model.state_dict()
    assert set(params) == set(p64)
    for key in params:
        R.check_rule(f"edge-epoch-{case}/param.{key}", params[key], p64[key].numpy(), p32[key].numpy(), REPORT)
    assert not np.array_equal(after[0][nat.PPO_PARAM]["zone_w1"][:, 14], start[0][nat.PPO_PARAM]["zone_w1"][:, 14])
    for w, tensors in start[0].items():                       # the same call from the same state: the same bits
        env.ppo_set_tensors(tensors, w)
    env.ppo_set_step(start[1])
    env.ppo_epoch(order, size)
    again = state()
    assert again[1] == after[1] == 2 and K.same_bits(env.ppo_stats(), dev_stats)
    for w in after[0]:
        for name in after[0][w]:
            assert K.same_bits(again[0][w][name], after[0][w][name]), (w, name)


# -------------------------------------------------------------- 6: the episode log and the film, odd-offset record
def test_episode_logs_and_film_of_an_odd_offset_record(zenv_mod):
    """odd15 at T = 5: exp.action and every buffer behind it start at an odd float offset.  The logs under the rule of
    test_gpu_order_rows.py::test_episode_logs_sum_the_env_reward_and_the_shaped_one (every env ends one episode, on
    frame 3; four float32 terms of magnitude at most 1: 2 ulp(1) = 2.4e-7); the film byte for byte."""
    Z = zenv_mod
    n, zones = K.CASES["odd15"]
    frames = 5
    c = _collect_with_twin(Z, "odd15", frames, False)
    film = _make(Z, "odd15")
    try:
        logs, rec, x = c["logs"], c["rec"], c["x"]
        assert np.array_equal(logs["env_per_episode"], np.arange(n)) and logs["num_frames"] == n * frames
        assert (logs["num_frames_per_episode"] == K.NUM_STEPS).all()
        f = np.float32
        ret, resh = np.zeros(n, f), np.zeros(n, f)
        for k in range(K.NUM_STEPS):
            ret = ret + rec["reward"][:, k].astype(f)
            resh = resh + x["reward"][:, k]
        assert np.abs(logs["return_per_episode"] - ret).max() <= 2.4e-7
        assert np.abs(logs["reshaped_return_per_episode"] - resh).max() <= 2.4e-7
        assert (ret[0::2] >= 1).all() and (ret[1::2] == 0).all() and np.abs(resh - ret).max() > 0.5
        assert c["env"].experience_frames() == frames
        want = {e: [] for e in (0, n - 1)}
        for k in range(frames):
            for e in want:
                want[e].append(film.render(first=e, count=1, width=64, height=64, marks=None)[0])
            film.step(x["action"][:, k], auto_reset=True)
        for e in want:
            got = c["env"].render_experience(e, width=64, height=64)
            assert got.shape == (frames, 64, 64, 3) and got.any()
            assert np.array_equal(got, np.stack(want[e])), e
    finally:
        for e in (c["env"], c["twin"], film):
            e.close()
