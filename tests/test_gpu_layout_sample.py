"""GPU: layouts sampled on the device (K20) -- every bank row the device writes equals the host sampler's, bit for bit;
what the device gives up on or refuses stays untouched and is reported; the streamed ring holds the episodes it must;
ParallelEnv(device_layouts=True) plays what the default plays."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("robot", "zone_xy", "aux", "seeds", "first")
COUNTS = (1, 63, 64, 65, 130)

CONFIGS = {
    "PointTSP-v0": (lambda Z: Z.config_for_id("PointTSP-v0"), 180),     # seed 188 restarts 15 times
    "ColourMatch-v0": (lambda Z: Z.config_for_id("ColourMatch-v0"), 1),
    "z25k40": (lambda Z: Z.default_config(0, 25, zones_keepout=0.40), 1800),   # seed 1859 restarts 4 times
    "z32k35": (lambda Z: Z.default_config(0, 32, zones_keepout=0.35), 1),
    "z1": (lambda Z: Z.default_config(0, 1), 1),
    "PointTSP-v4": (lambda Z: Z.config_for_id("PointTSP-v4"), 1),
}


def _same_rows(a, b, rows=slice(None)):
    return [f for f in FIELDS if not np.array_equal(a[f][rows].view(np.uint8), b[f][rows].view(np.uint8))]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_device_bank_equals_host_bank(zenv_mod, name):
    Z = zenv_mod
    make, seed_first = CONFIGS[name]
    env = Z.ZoneVecEnv(make(Z), 4)
    for count in COUNTS:
        seeds = np.arange(seed_first, seed_first + count, dtype=np.int64)
        env.build_bank_seeds(seeds)
        want = env.read_bank()
        env.build_bank_seeds_device(seeds)
        got = env.read_bank()
        assert env.bank_size == count and np.array_equal(got["seeds"], seeds)
        assert _same_rows(want, got) == [], (name, count)
        assert env.sample_status()["n_failed"] == 0
    env.build_bank_device(seed_first, 65)              # the contiguous form is the same call
    assert _same_rows(env.read_bank(), {f: v[:65] for f, v in want.items()}) == []
    env.close()


@pytest.fixture(scope="module")
def hard_seeds(zenv_mod):
    """8 seeds of 1..200 of a config so tight that some need more host restarts than a device wave is allowed."""
    Z = zenv_mod
    cfg = Z.default_config(0, 32, zones_keepout=0.40)
    restarts = {s: Z.sample_layout(cfg, s)[3] for s in range(1, 201)}
    hard = [s for s, r in restarts.items() if r > Z.DEVICE_RESTARTS]
    assert hard and len(hard) < 8, restarts
    easy = [s for s, r in restarts.items() if r <= Z.DEVICE_RESTARTS][:8 - len(hard)]
    seeds = np.array(sorted(hard + easy), np.int64)
    return cfg, seeds, np.array([s in hard for s in seeds]), easy[0]


def test_host_finishes_what_the_device_gives_up_on(zenv_mod, hard_seeds):
    Z = zenv_mod
    cfg, seeds, is_hard, easy = hard_seeds
    env = Z.ZoneVecEnv(cfg, 2)
    env.build_bank_seeds(seeds)
    want = env.read_bank()
    env.build_bank_seeds_device(seeds)                  # synchronous: the host sampler fills the unfinished slots in
    assert _same_rows(want, env.read_bank()) == []
    assert env.sample_status()["n_failed"] == 0         # ... and takes the reports with it
    # asynchronous refill of the same seeds over a bank of one easy map: the hard slots stay, and are listed
    env.build_bank_seeds(np.full(8, easy, np.int64))
    base = env.read_bank()
    total0 = env.sample_status()["n_sampled_total"]
    env.update_bank_device(np.arange(8, dtype=np.int32), seeds)
    st = env.sample_status()
    got = env.read_bank()
    assert st["n_failed"] == int(is_hard.sum()) == len(st["slots"])
    order = np.argsort(st["slots"])
    assert np.array_equal(st["slots"][order], np.flatnonzero(is_hard))
    assert np.array_equal(st["seeds"][order], seeds[is_hard])
    assert (st["codes"] == Z.SAMPLE_UNFINISHED).all()
    assert st["n_sampled_total"] - total0 == int((~is_hard).sum())
    assert _same_rows(base, got, is_hard) == [] and _same_rows(want, got, ~is_hard) == []
    st = env.sample_status()                            # taking the list clears it
    assert st["n_failed"] == 0 and len(st["slots"]) == 0
    env.close()


def test_seed_out_of_range(zenv_mod):
    Z = zenv_mod
    env = Z.ZoneVecEnv("PointTSP-v1", 3)
    env.build_bank(7, 5)
    before = env.read_bank()
    for bad in (2 ** 32 - 1, -1):
        with pytest.raises(Z.ZenvError) as ei:
            env.build_bank_seeds_device([1, bad, 2])
        assert ei.value.code == Z.E_ARG
        assert env.bank_size == 5 and _same_rows(before, env.read_bank()) == []
    # the kernel's own range check: a refill leaves the slot alone and says why
    env.update_bank_device([4, 1, 3], [2 ** 32 - 1, 50, -1])
    st = env.sample_status()
    got = env.read_bank()
    order = np.argsort(st["slots"])
    assert st["n_failed"] == 2 and st["slots"][order].tolist() == [3, 4] and (st["codes"] == Z.SAMPLE_SEED_RANGE).all()
    assert st["seeds"][order].tolist() == [-1, 2 ** 32 - 1]
    keep = np.array([True, False, True, True, True])
    assert _same_rows(before, got, keep) == [] and got["seeds"][1] == 50
    env.close()


@pytest.mark.parametrize("count", [1, 65])
def test_update_bank_device_equals_update_bank(zenv_mod, count):
    Z = zenv_mod
    N = 130
    rng = np.random.default_rng(count)
    slots = rng.permutation(N)[:count].astype(np.int32)            # scattered, no slot twice
    seeds = 5000 + rng.permutation(1000)[:count].astype(np.int64)
    twins = [Z.ZoneVecEnv("PointTSP-v0", N) for _ in range(2)]
    for env in twins:
        env.build_bank(180, N)
    twins[0].update_bank(slots, seeds)
    twins[1].update_bank_device(slots, seeds)
    assert _same_rows(twins[0].read_bank(), twins[1].read_bank()) == []
    assert twins[1].sample_status()["n_failed"] == 0
    for env in twins:
        env.reset()
    first = [env.step_results(None) for env in twins]
    for a, b in zip(*first):
        assert np.array_equal(a, b)
    for t in range(20):
        act = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
        out = [env.step_results(act) for env in twins]
        for a, b in zip(*out):
            assert np.array_equal(a, b), t
    for env in twins:
        env.close()


@pytest.mark.parametrize("depth", [3, 1, 4])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_ring_holds_the_episodes_it_must(zenv_mod, depth, k):
    Z = zenv_mod
    N = 5
    seed0 = np.array([100, 2000, 30000, 180, 77], np.int64)
    env = Z.ZoneVecEnv("PointTSP-v0", N)
    env.ring_stream(seed0, depth)
    assert env.bank_size == N * depth
    assert env.sample_status()["n_sampled_total"] == N * depth
    for _ in range(k):
        env.reset()
    env.ring_refill()
    st = env.sample_status()
    assert st["n_failed"] == 0 and st["n_sampled_total"] == N * depth + N * min(k, depth)
    # slot i*depth + j holds episode e_j: the smallest e >= k with e mod depth == j
    j = np.arange(depth)
    e = k + (j - k % depth) % depth
    want_seeds = (seed0[:, None] + e[None, :]).reshape(-1)
    got = env.read_bank()
    assert np.array_equal(got["seeds"], want_seeds)
    host = Z.ZoneVecEnv("PointTSP-v0", N)
    host.build_bank_seeds(want_seeds)
    assert _same_rows(host.read_bank(), got) == []
    env.ring_refill()                                   # nothing is stale: nothing is sampled
    assert env.sample_status()["n_sampled_total"] == st["n_sampled_total"]
    # the next episode each env plays is episode k: the layout of seed0 + k
    env.reset()
    assert np.array_equal(env.get(Z.F_SEED), seed0 + k)
    env.close()
    host.close()


def test_ring_refill_needs_a_streamed_ring(zenv_mod):
    Z = zenv_mod
    env = Z.ZoneVecEnv("PointTSP-v1", 4)
    with pytest.raises(Z.ZenvError) as ei:
        env.ring_refill()                               # no bank at all
    assert ei.value.code == Z.E_STATE
    env.build_bank(1, 12)
    env.schedule_ring(np.arange(4, dtype=np.int32) * 3, 3)      # a ring the host laid
    with pytest.raises(Z.ZenvError) as ei:
        env.ring_refill()
    assert ei.value.code == Z.E_STATE and "zenv_ring_stream" in str(ei.value)
    env.ring_stream(np.arange(4, dtype=np.int64) * 10, 3)
    env.ring_refill()
    env.schedule_sequential()                           # another schedule replaces the streamed ring
    with pytest.raises(Z.ZenvError) as ei:
        env.ring_refill()
    assert ei.value.code == Z.E_STATE
    env.close()


def test_parallel_env_device_layouts_plays_the_default(zenv_mod):
    from combinatorial_rl_tasks_amd.envs import make_test_env
    from combinatorial_rl_tasks_amd.penv import ParallelEnv
    P = 16
    rng = np.random.default_rng(3)
    acts = rng.uniform(-1, 1, (20, 3, P, 2)).astype(np.float32)
    runs = []
    for device_layouts in (False, True):
        pe = ParallelEnv([make_test_env("PointTSP-v1", seed=4000 + 100000 * i) for i in range(P)],
                         device_layouts=device_layouts)
        log = []
        for r in range(20):
            log.append(pe.reset())
            for t in range(3):
                log.append(pe.step(acts[r, t]))
        log.append(pe.vec.get(zenv_mod.F_SEED).tolist())
        runs.append(log)
        pe.close()

    def same(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(a, b)
    assert runs[0][-1] == [4000 + 100000 * i + 19 for i in range(P)]
    for n, (a, b) in enumerate(zip(*runs)):
        assert same(a, b), n


def test_host_only_handles_refuse_device_sampling(zenv_mod):
    Z = zenv_mod
    from combinatorial_rl_tasks_amd.envs import make_test_env
    from combinatorial_rl_tasks_amd.penv import ParallelEnv
    timed = Z.ZoneVecEnv("PointTTSP-v1", 2)
    ordered = Z.ZoneVecEnv("PointTSP-v1", 2)
    ordered.enable_order()
    for env, word in ((timed, "TimedTSP"), (ordered, "solver-ordered")):
        env.build_bank(1, 4)
        before = env.read_bank()
        calls = (lambda: env.build_bank_device(1, 4), lambda: env.build_bank_seeds_device([1, 2]),
                 lambda: env.update_bank_device([0], [9]), lambda: env.ring_stream([1, 2], 2), lambda: env.ring_refill())
        for call in calls:
            with pytest.raises(Z.ZenvError) as ei:
                call()
            assert ei.value.code == Z.E_STATE and word in str(ei.value)
        assert _same_rows(before, env.read_bank()) == []
        env.close()
    with pytest.raises(ValueError, match="TimedTSP"):
        ParallelEnv([make_test_env("PointTTSP-v1", seed=1)], device_layouts=True)
