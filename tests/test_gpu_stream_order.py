"""Ordering of the env's entry points on a caller's busy side stream (tests/stream_stall.py has the method and the
classification): the stepping calls, the consumer direction, TorchZoneEnv's closed loop, the calls that read caller
host memory, the layout banks and schedules, the calls that synchronise, and two handles on two streams.

Every sequence runs four times: once on each of two handles with a sync() after every call and OTHER argument values
(the warm-up: it allocates every buffer the sequence needs, so that nothing is allocated, resized or freed behind a
stall, and leaves valid but different contents in every buffer a misordered kernel could read early), then on handle A
behind stalls of its side stream, then on the twin with a sync() after every call.  A and the twin must then agree bit
for bit.  N = 257: a ragged last wave and workgroup."""
import numpy as np
import pytest

from tests import stream_stall as S
from tests.stream_stall import ASYNC, HOST_ARG, WAITS, N, Pair

pytestmark = pytest.mark.gpu

KMAX = 257          # crosses ZENV_ROLLOUT_CHUNK = 256

CONFIGS = {
    "tsp15": lambda Z: Z.config_for_id("PointTSP-v0", num_steps=40),       # lane layout, persistent kernel
    "zones7": lambda Z: Z.default_config(0, 7, num_steps=40),              # no lane instantiation: single-step launches
    "colour": lambda Z: Z.config_for_id("ColourMatch-v0", num_steps=40),
    "timed": lambda Z: Z.config_for_id("PointTTSP-v0", num_steps=40),
}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    S.print_observed()


def _plain(Z, name, **kw):
    def make():
        env = Z.ZoneVecEnv(CONFIGS[name](Z), N, **kw)
        env.build_bank(1000, N)
        env.schedule_sequential()
        return env
    return make


def _scratch(tenv, variant):
    """The torch tensors a sequence works with, made once (in the warm-up)."""
    import torch
    t = tenv.scratch
    if "src" not in t:
        assert variant == 0
        g = torch.Generator().manual_seed(5)
        t["src"] = (torch.rand(KMAX, N, 2, generator=g) * 2 - 1).to(tenv.device)
        t["act"] = torch.zeros(N, 2, device=tenv.device)
        t["chunk"] = torch.zeros(KMAX, N, 2, device=tenv.device)
        for name in ("obs", "zone_obs", "reward"):
            for tag in ("a", "b"):
                t[f"{name}_{tag}"] = torch.zeros_like(getattr(tenv, name))
        t["ep_return"] = torch.zeros(N, dtype=torch.float64, device=tenv.device)
        t["ep_len"] = torch.zeros(N, dtype=torch.int32, device=tenv.device)
        torch.cuda.synchronize()
    return t


def _consume(d, tenv, t, tag):
    """The consumer direction: torch copies of the aliased output buffers, enqueued on the handle's stream."""
    with d.torch():
        for name in ("obs", "zone_obs", "reward"):
            t[f"{name}_{tag}"].copy_(getattr(tenv, name))
    return {f"{name}_{tag}": t[f"{name}_{tag}"] for name in ("obs", "zone_obs", "reward")}


def core_sequence(Z, d, tenv, variant):
    import torch
    env, t = d.env, _scratch(tenv, variant)
    seed, scale = 11 + variant, (0.5, -1.0)[variant]
    out = {}
    d.run(ASYNC, "zenv_reset", lambda: env.reset())
    d.run(ASYNC, "zenv_policy", lambda: env.policy(Z.POLICY_GREEDY, policy_seed=seed))
    d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))
    with d.torch():                                   # the action tensor is computed behind the stall
        torch.mul(t["src"][0], scale, out=t["act"])
    d.run(ASYNC, "zenv_step(device actions)", lambda: env.step_device(t["act"].data_ptr()))
    out.update(_consume(d, tenv, t, "a"))
    i = 0
    for K in (3, KMAX):
        for mode in ("never", "every", "last"):
            with d.torch(fresh=K > 3):                # (a new stall in front of a chunk that takes long to enqueue)
                torch.mul(t["src"][:K], scale * (1.0 - 0.1 * i), out=t["chunk"][:K])
            d.run(ASYNC, f"zenv_step_many(device, K={K}, {mode})",
                  lambda: env.step_many(None, reset=mode, actions_ptr=(t["chunk"].data_ptr(), K)))
            i += 1
    for mode in ("persistent", "per_step", "unfused"):
        d.run(ASYNC, f"zenv_rollout(ASYNC, {mode})",
              lambda: env.rollout(5, Z.POLICY_UNIFORM, policy_seed=seed, mode=mode, wait=False), fresh=mode == "persistent")
    out.update(_consume(d, tenv, t, "b"))
    idle = d.run(ASYNC, "zenv_query", env.done)
    assert not (d.stalled and idle), "zenv_query called the stalled stream idle"
    ep_return = d.run(ASYNC, "zenv_device_ptr(EP_RETURN)", lambda: tenv.ep_return)
    ep_len = d.run(ASYNC, "zenv_device_ptr(EP_LEN)", lambda: tenv.ep_len)
    with d.torch():
        t["ep_return"].copy_(ep_return)
        t["ep_len"].copy_(ep_len)
    out.update(ep_return=t["ep_return"], ep_len=t["ep_len"])
    return out


def _chunk_records(env):
    r, dn = env.chunk_results()
    return dict(chunk_reward=r, chunk_done=dn)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_core_stepping_behind_a_stall(zenv_mod, config):
    """reset, policy, step(NULL), step(device tensor computed behind the stall), step_many from a device pointer (K = 3
    and 257, the three reset modes), the three asynchronous rollouts, zenv_query and the stream-ordered unpacking of
    EP_RETURN / EP_LEN: all return with the stall still running, and the handle ends as its twin.  The torch copies of
    the aliased obs / zone_obs / reward taken on the same stream are the twin's."""
    p = Pair(zenv_mod, _plain(zenv_mod, config))
    try:
        st = p.check(core_sequence, f"core[{config}]", _chunk_records)
        assert st.stalls <= 10
    finally:
        p.close()


def test_wave_per_env_layout_behind_a_stall(zenv_mod):
    """The same sequence on the wave-per-env kernels (K1w has its own launcher)."""
    Z = zenv_mod
    p = Pair(Z, _plain(Z, "tsp15", kernel=Z._native.KERNEL_WAVE_PER_ENV))
    try:
        p.check(core_sequence, "core[wave-per-env]", _chunk_records)
    finally:
        p.close()


def test_torch_closed_loop_on_a_side_stream(zenv_mod):
    """TorchZoneEnv built inside ``with torch.cuda.stream(side)``: the closed loop of
    test_torch_policy_closed_loop_without_host_copies, 20 steps, one stall in front; the property copies ep_return /
    ep_len (zenv_device_ptr refreshes them stream-ordered) taken right after the loop hold all 20 steps."""
    import torch
    Z = zenv_mod
    p = Pair(Z, _plain(Z, "timed"))
    w = {}

    def loop(Z, d, tenv, variant):
        env, dev = d.env, tenv.device
        if not w:
            g = torch.Generator().manual_seed(3)
            w["w1"] = (torch.randn(8 + 7, 32, generator=g) * 0.5).to(dev)
            w["w2"] = (torch.randn(8 + 32, 2, generator=g) * 0.5).to(dev)
        t = tenv.scratch
        if "ret" not in t:
            t["ret"] = torch.zeros(N, dtype=torch.float64, device=dev)
            t["len"] = torch.zeros(N, dtype=torch.int32, device=dev)
            t["o"], t["zo"] = torch.zeros_like(tenv.obs), torch.zeros_like(tenv.zone_obs)
        sign = (1.0, -1.0)[variant]
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        obs = {"obs": tenv.obs, "zone_obs": tenv.zone_obs}
        for _ in range(20):
            with d.torch():
                x = torch.cat([obs["obs"][:, None, :].expand(N, 15, 8), obs["zone_obs"]], dim=-1)
                emb = torch.relu(x @ w["w1"]).mean(dim=1)
                a = torch.tanh(sign * (torch.cat([obs["obs"], emb], dim=-1) @ w["w2"])).contiguous()
            obs = d.run(ASYNC, "zenv_step(device actions)", lambda: tenv.step(a))[0]
        ret = d.run(ASYNC, "zenv_device_ptr(EP_RETURN)", lambda: tenv.ep_return)
        ln = d.run(ASYNC, "zenv_device_ptr(EP_LEN)", lambda: tenv.ep_len)
        with d.torch():
            t["ret"].copy_(ret)
            t["len"].copy_(ln)
            t["o"].copy_(obs["obs"])
            t["zo"].copy_(obs["zone_obs"])
        return dict(ep_return=t["ret"], ep_len=t["len"], obs=t["o"], zone_obs=t["zo"])

    try:
        st = p.check(loop, "torch closed loop")
        assert st.stalls == 1, "the loop outlasted its one stall"
        ep_len = p.env.get(Z.F_EP_LEN)
        assert 1 <= ep_len.max() <= 20 and np.array_equal(ep_len, p.tenv.scratch["len"].cpu().numpy())
    finally:
        p.close()


@pytest.mark.parametrize("memory", ["pageable", "pinned"])
def test_calls_that_read_caller_host_memory(zenv_mod, memory):
    """Masked reset, step with a host array, step_many with a host chunk.  Pageable numpy memory is overwritten in place
    with other valid values the moment the call returns; page-locked memory (zenv_host_alloc) is left alone until the
    stream has been synchronised.  Either way the handle ends as the twin that was fed the original values.  Whether
    each call returned with the stall still running or blocked until it ended is recorded (printed with -s)."""
    Z = zenv_mod
    p = Pair(Z, _plain(Z, "tsp15"))
    shapes = dict(mask=((N,), np.uint8), act=((N, 2), np.float32), every=((3, N, 2), np.float32), last=((3, N, 2), np.float32))

    def sequence(Z, d, tenv, variant):
        env, t = d.env, tenv.scratch
        if "mask" not in t:
            for name, (shape, dt) in shapes.items():
                t[name] = np.zeros(shape, dt) if memory == "pageable" else env._own_pinned_array(shape, dt)
        rs = np.random.RandomState(100 + variant)
        vals = dict(mask=rs.randint(0, 2, N).astype(np.uint8), act=rs.uniform(-1, 1, (N, 2)).astype(np.float32),
                    every=rs.uniform(-1, 1, (3, N, 2)).astype(np.float32), last=rs.uniform(-1, 1, (3, N, 2)).astype(np.float32))
        other = dict(mask=1 - vals["mask"], act=-vals["act"], every=-vals["every"], last=-vals["last"])

        def call(name, what, fn):
            t[name][...] = vals[name]
            d.run(HOST_ARG, f"{what} ({memory})", fn)
            if memory == "pageable":
                t[name][...] = other[name]                  # the moment the call returns

        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        for k in range(3):
            d.run(ASYNC, "zenv_policy", lambda: env.policy(Z.POLICY_GREEDY, policy_seed=40 + variant))
            d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))
        call("mask", "zenv_reset(mask)", lambda: env.reset(t["mask"]))
        d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))
        call("act", "zenv_step(host actions)", lambda: env.step(t["act"]))
        call("every", "zenv_step_many(host chunk, every)", lambda: env.step_many(t["every"], reset="every"))
        call("last", "zenv_step_many(host chunk, last)", lambda: env.step_many(t["last"], reset="last"))
        d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))         # replays the action buffer the chunk left

    try:
        p.check(sequence, f"host arguments[{memory}]", _chunk_records)
        # the mask took effect: an env the mask named restarted its episode three steps ago, the others ran on
        assert len(set(p.env.get(Z.F_EP_LEN).tolist())) > 1
    finally:
        p.close()


@pytest.mark.parametrize("n_env", [257, 4099])
def test_large_pageable_chunk_is_consumed_before_the_call_returns(zenv_mod, n_env):
    """The runtime handles a pageable source differently by size (a bounce buffer for small copies, chunked or pinned
    transfers beyond it): a 257-step host chunk of 0.5 MB (257 envs) and of 8.4 MB (4099 envs), overwritten in place
    the moment zenv_step_many returns behind a stall.  The handle must end as the twin fed the original chunk."""
    Z = zenv_mod

    def make():
        env = Z.ZoneVecEnv(CONFIGS["tsp15"](Z), n_env)
        env.build_bank(1000, n_env)
        env.schedule_sequential()
        return env

    def sequence(Z, d, tenv, variant):
        env, t = d.env, tenv.scratch
        if "big" not in t:
            t["big"] = np.zeros((KMAX, n_env, 2), np.float32)
        rs = np.random.RandomState(300 + variant)
        vals = rs.uniform(-1, 1, t["big"].shape).astype(np.float32)
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        d.run(ASYNC, "zenv_policy", lambda: env.policy(Z.POLICY_GREEDY, policy_seed=4))
        d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))
        t["big"][...] = vals
        d.run(HOST_ARG, f"zenv_step_many(host chunk of {t['big'].nbytes >> 10} KB, pageable)",
              lambda: env.step_many(t["big"], reset="every"))
        t["big"][...] = -vals[::-1]                             # the moment the call returns
        d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))

    p = Pair(Z, make)
    try:
        p.check(sequence, f"large host chunk[{n_env}]", _chunk_records)
    finally:
        p.close()


def bank_sequence(Z, d, tenv, variant):
    """zenv_bank_update twice in a row (the staging image's event), resets into the refilled slots, then
    zenv_bank_update_device and resets into those."""
    env = d.env
    rs = np.random.RandomState(7 + variant)
    base = 20000 + 5000 * variant

    def pick(k):
        return rs.permutation(N)[:100].astype(np.int32), (base + 200 * k + np.arange(100)).astype(np.int64)

    def steps(k):
        for _ in range(k):
            d.run(ASYNC, "zenv_policy", lambda: env.policy(Z.POLICY_GREEDY, policy_seed=3 + variant))
            d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))

    d.run(ASYNC, "zenv_reset", lambda: env.reset())
    steps(2)
    (s1, q1), (s2, q2), (s3, q3) = pick(0), pick(1), pick(2)
    d.run(ASYNC, "zenv_bank_update", lambda: env.update_bank(s1, q1))
    # the second refill waits for the first one's copy out of the shared image: it blocks until the stall has ended
    d.run(HOST_ARG, "zenv_bank_update, the second in a row", lambda: env.update_bank(s2, q2))
    d.run(ASYNC, "zenv_reset", lambda: env.reset())
    steps(3)
    d.run(ASYNC, "zenv_bank_update_device", lambda: env.update_bank_device(s3, q3))
    d.run(ASYNC, "zenv_reset", lambda: env.reset())
    steps(3)


def _bank(env):
    out = env.read_bank()
    st = env.sample_status()
    out.update(n_failed=np.int64(st["n_failed"]), n_sampled_total=np.int64(st["n_sampled_total"]), failed_slots=st["slots"])
    return out


def _timed_device(Z):
    def make():
        env = Z.ZoneVecEnv(CONFIGS["timed"](Z), N)
        env.timed_layouts_device()
        env.build_bank_device(1000, N)
        env.schedule_sequential()
        return env
    return make


def _order_device(Z):
    def make():
        env = Z.ZoneVecEnv(CONFIGS["tsp15"](Z), N)
        env.enable_order()
        env.order_routes_device()
        env.build_bank_device(1000, N)
        env.schedule_sequential()
        return env
    return make


@pytest.mark.parametrize("handle", ["plain", "timed_layouts_device", "order_routes_device"])
def test_bank_refills_behind_a_stall(zenv_mod, handle):
    Z = zenv_mod
    make = {"plain": _plain(Z, "tsp15"), "timed_layouts_device": _timed_device(Z), "order_routes_device": _order_device(Z)}[handle]
    p = Pair(Z, make)
    try:
        p.check(bank_sequence, f"banks[{handle}]", _bank)
    finally:
        p.close()


def test_ring_refill_behind_a_stall(zenv_mod):
    """zenv_ring_stream's ring, refilled on the device behind a stall, and steps that reset into the refilled slots."""
    Z = zenv_mod

    def make():
        env = Z.ZoneVecEnv(Z.config_for_id("PointTSP-v0", num_steps=8), N)
        env.ring_stream(3000 + 10 * np.arange(N, dtype=np.int64), 2)
        return env

    def sequence(Z, d, tenv, variant):
        env = d.env
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        d.run(ASYNC, "zenv_ring_refill", env.ring_refill)
        for _ in range(3):
            for _ in range(9):                                  # num_steps = 8: every env ends an episode
                d.run(ASYNC, "zenv_policy", lambda: env.policy(Z.POLICY_UNIFORM, policy_seed=5 + variant))
                d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))
            d.run(ASYNC, "zenv_ring_refill", env.ring_refill)

    p = Pair(Z, make)
    try:
        p.check(sequence, "ring", _bank)
        seeds = p.env.read_bank()["seeds"].reshape(N, 2)
        assert np.all(p.env.get(Z.F_EPISODES) >= 6) and np.all(seeds.max(axis=1) >= 3000 + 10 * np.arange(N) + 6)
    finally:
        p.close()


def _step(Z, d, env, seed):
    d.run(ASYNC, "zenv_policy", lambda: env.policy(Z.POLICY_GREEDY, policy_seed=seed))
    d.run(ASYNC, "zenv_step(NULL)", lambda: env.step(None))


def test_readers_wait_for_the_stalled_step(zenv_mod):
    """get, get_rows, get_many (results_into), step_results, get_state and set_state straight after a stalled step: each
    returns with the marker complete and hands back the values after that step."""
    Z = zenv_mod
    nat = Z._native
    p = Pair(Z, _plain(Z, "tsp15"))

    def sequence(Z, d, tenv, variant):
        env, t = d.env, tenv.scratch
        if "o" not in t:
            t["o"], t["r"] = np.zeros((N, 8), np.float32), np.zeros(N, np.float32)
        seed, out = 60 + variant, {}
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        _step(Z, d, env, seed)
        out["get"] = d.run(WAITS, "zenv_get", lambda: env.get(nat.F_OBS))
        _step(Z, d, env, seed)
        out["get_rows"] = d.run(WAITS, "zenv_get_rows", lambda: env.get_head(nat.F_ZONE_OBS, 130, 127))
        _step(Z, d, env, seed)
        d.run(WAITS, "zenv_get_many", lambda: env.results_into([nat.F_OBS, nat.F_REWARD], [t["o"], t["r"]]))
        out["get_many_obs"], out["get_many_reward"] = t["o"].copy(), t["r"].copy()
        _step(Z, d, env, seed)
        res = d.run(WAITS, "zenv_step_results", lambda: env.step_results(np.full((N, 2), 0.25 * (1 + variant), np.float32)))
        out.update({f"step_results_{i}": r for i, r in enumerate(res)})
        _step(Z, d, env, seed)
        blob = d.run(WAITS, "zenv_get_state", env.get_state)
        out["blob"] = blob
        _step(Z, d, env, seed)
        _step(Z, d, env, seed)
        d.run(WAITS, "zenv_set_state", lambda: env.set_state(blob))          # back to the snapshot: two steps undone
        out["after_set_state"] = d.run(WAITS, "zenv_get_state", env.get_state)
        _step(Z, d, env, seed)
        return out

    try:
        st = p.check(sequence, "readers", ms=60.0)
        assert st.stalls <= 10
    finally:
        p.close()


def test_bank_and_schedule_calls_wait_for_the_stalled_step(zenv_mod):
    """bank_read, sample_status, the three schedule_* calls and set_stream (to the handle's own stream and back) straight
    after a stalled step."""
    import torch
    Z = zenv_mod

    def make():
        env = Z.ZoneVecEnv(CONFIGS["tsp15"](Z), N)
        env.build_bank(0, 2 * N)
        env.schedule_sequential()
        return env

    p = Pair(Z, make)

    def sequence(Z, d, tenv, variant):
        env, t = d.env, _scratch(tenv, variant)
        seed, out = 70 + variant, {}
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        _step(Z, d, env, seed)
        out.update(d.run(WAITS, "zenv_bank_read", lambda: env.read_bank(5, 200)))
        _step(Z, d, env, seed)
        status = d.run(WAITS, "zenv_sample_status", env.sample_status)
        out["n_failed"] = np.int64(status["n_failed"])
        _step(Z, d, env, seed)
        first = ((np.arange(N) * 3 + variant) % (2 * N)).astype(np.int32)
        d.run(WAITS, "zenv_schedule_sequential", lambda: env.schedule_sequential(first, 1))
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        _step(Z, d, env, seed)
        d.run(WAITS, "zenv_schedule_ring", lambda: env.schedule_ring((np.arange(N) * 2).astype(np.int32), 2))
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        _step(Z, d, env, seed)
        d.run(WAITS, "zenv_schedule_fixed_seeds",
              lambda: env.schedule_fixed_seeds(np.arange(N, dtype=np.uint64) + 9 + variant, 0, 2 * N - 1))
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        _step(Z, d, env, seed)
        if d.stalled:
            d.run(WAITS, "zenv_set_stream(own)", lambda: env.set_stream(None))      # drains the stream it leaves
        out["obs_on_own_stream"] = env.get(Z.F_OBS)
        env.step(None)                                          # (A: on its own stream, the side stream stays idle)
        env.sync()
        if d.stalled:
            env.set_stream(p.side.cuda_stream)                  # and back: the next step waits for the tensor again
        with d.torch():
            torch.mul(t["src"][1], 0.75 - variant, out=t["act"])
        d.run(ASYNC, "zenv_step(device actions)", lambda: env.step_device(t["act"].data_ptr()))
        _step(Z, d, env, seed)
        return out

    try:
        st = p.check(sequence, "banks and schedules", ms=60.0)
        assert st.stalls <= 10
        assert torch.cuda.current_stream() != p.side
    finally:
        p.close()


def test_goal_calls_wait_for_the_stalled_step(zenv_mod):
    """solver_goals and set_goals on a goal-conditioned ColourMatch handle straight after a stalled step."""
    Z = zenv_mod

    def make():
        env = Z.ZoneVecEnv(CONFIGS["colour"](Z), N)
        env.enable_goals()
        env.build_bank(300, N)
        env.schedule_sequential()
        return env

    def sequence(Z, d, tenv, variant):
        env, out = d.env, {}
        d.run(ASYNC, "zenv_reset", lambda: env.reset())
        for k in range(3):
            goals = d.run(WAITS, "zenv_solver_goals", env.solver_goals)
            need = env.get(Z.F_NEED_GOAL).astype(bool)
            out[f"solver_goals_{k}"] = goals
            d.run(WAITS, "zenv_set_goals", lambda: env.set_goals(np.where(need, np.maximum(goals, 0), -1).astype(np.int32)))
            for _ in range(4):
                _step(Z, d, env, 80 + variant)
        out["goal"], out["shaped"] = env.get(Z.F_GOAL), env.get(Z.F_SHAPED_REWARD)
        return out

    p = Pair(Z, make)
    try:
        p.check(sequence, "goals", ms=60.0)
    finally:
        p.close()


def test_two_handles_on_two_side_streams(zenv_mod):
    """Two handles on two side streams, calls interleaved, one stream stalled and one free: each ends as its solo run."""
    import torch
    Z = zenv_mod
    make = _plain(Z, "tsp15")
    envs = [make() for _ in range(4)]                            # A, B interleaved; their solo twins
    sides = [S.side_stream(), S.side_stream()]
    seeds = (91, 92)

    def calls(env, seed):
        return [lambda: env.reset()] + [f for _ in range(6) for f in (
            lambda: env.policy(Z.POLICY_GREEDY, policy_seed=seed), lambda: env.step(None))] + [
            lambda: env.rollout(7, Z.POLICY_UNIFORM, policy_seed=seed, wait=False)]

    try:
        for env, seed in zip(envs, seeds + seeds):              # warm-up: the persistent kernel's parameter block
            for f in calls(env, seed + 100):
                f()
            env.sync()
        # the stalled handle's side stream runs beside that handle's own stream and beside the free handle's stream
        sides[0] = S.pick_side_stream(Z, envs[0], also_reset=tuple(envs[1:]))
        scratch = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(8):
            sides[1] = S.side_stream()
            probe, done = S.stall(sides[0], 30.0), torch.cuda.Event()
            with torch.cuda.stream(sides[1]):
                scratch.add_(1.0)
                done.record(sides[1])
            while not done.query() and not probe.query():          # bounded by the stall
                pass
            beside = done.query() and not probe.query()
            torch.cuda.synchronize()
            if beside:
                break
        assert beside, "INCONCLUSIVE: no second side stream runs beside the stalled one (one hardware queue)"
        envs[1].set_stream(sides[1].cuda_stream)
        envs[0].set_stream(sides[0].cuda_stream)
        marker = S.stall(sides[0])
        for fa, fb in zip(calls(envs[0], seeds[0]), calls(envs[1], seeds[1])):
            fa()
            fb()
        free = torch.cuda.Event()
        free.record(sides[1])
        free.synchronize()                                      # the free stream runs while the other is stalled
        assert envs[1].done() and not envs[0].done()
        S.assert_still_pending(marker, "the interleaved calls and the free handle's work")
        sides[0].synchronize()
        for env, seed in zip(envs[2:], seeds):
            for f in calls(env, seed):
                f()
                env.sync()
        for i in (0, 1):
            S.assert_twins_equal(Z, envs[i], envs[i + 2], f"handle {'AB'[i]} against its solo run")
    finally:
        torch.cuda.synchronize()
        for env in envs:
            env.set_stream(None)
            env.close()
