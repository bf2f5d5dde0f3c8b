"""GPU: the device layout sampler (K20 / K21) beyond one grid and past the failure list -- the second and third trip of
the grid-stride loops (banks, scattered refills and the streamed ring at more than kMaxGrid = 8192 entries), and more
failures in one launch than SampleStatus lists (1024): the guard in front of the list, the builders' redo-every-slot
path and errors, and the repair loop ParallelEnv runs.  Every comparison is byte for byte against the host path; the
inputs are pinned without a GPU by tests/test_layout_scale_cases_cpu.py."""
import numpy as np
import pytest

from tests.layout_scale_cases import HOST_ATTEMPTS, MAX_GRID, PASSES3, host_restarts, tight_config

pytestmark = pytest.mark.gpu

FIELDS = ("robot", "zone_xy", "aux", "seeds", "first")


def _same_rows(a, b, rows=slice(None)):
    return [f for f in FIELDS if not np.array_equal(a[f][rows].view(np.uint8), b[f][rows].view(np.uint8))]


def _plain(Z, cfg):
    return Z.ZoneVecEnv(cfg, 2)


def _timed(Z, cfg):
    env = Z.ZoneVecEnv(cfg, 2)
    env.timed_layouts_device()
    return env


def _order(Z, cfg, n=2, device_routes=True):
    env = Z.ZoneVecEnv(cfg, n)
    env.enable_order()
    if device_routes:
        env.order_routes_device()
    return env


# name -> (config, handle, first seed, counts).  No seed of these ranges restarts more than 16 times on the host, so the
# device finishes every one and n_sampled_total counts them all.
BANKS = {
    "PointTSP-v0": ("PointTSP-v0", _plain, 180, (MAX_GRID, MAX_GRID + 1, PASSES3)),
    "ColourMatch-v0": ("ColourMatch-v0", _plain, 1, (PASSES3,)),
    "PointTTSP-v1": ("PointTTSP-v1", _timed, 1, (PASSES3,)),
    "PointTSP-v0-order": ("PointTSP-v0", _order, 180, (PASSES3,)),
    "PointTSP-v4": ("PointTSP-v4", _plain, 1, (PASSES3,)),          # five fixed zone locations
}


# ---------------------------------------------------------------- a. banks over more than one grid
@pytest.mark.parametrize("name", sorted(BANKS))
def test_device_bank_over_several_grids_equals_host_bank(zenv_mod, name):
    Z = zenv_mod
    env_id, make, seed_first, counts = BANKS[name]
    env = make(Z, Z.config_for_id(env_id))
    all_seeds = np.arange(seed_first, seed_first + max(counts), dtype=np.int64)
    env.build_bank_seeds(all_seeds)
    want = env.read_bank()                                  # the host bank, once: a shorter bank is its first rows
    for count in counts:
        total0 = env.sample_status()["n_sampled_total"]
        env.build_bank_seeds_device(all_seeds[:count])
        got = env.read_bank()
        assert env.bank_size == count and np.array_equal(got["seeds"], all_seeds[:count])
        assert _same_rows({f: v[:count] for f, v in want.items()}, got) == [], (name, count)
        if make is _order:
            assert np.array_equal(np.sort(got["aux"], 1), np.tile(np.arange(env.num_zones), (count, 1)))
        st = env.sample_status()
        assert st["n_failed"] == 0 and len(st["slots"]) == 0
        assert st["n_sampled_total"] - total0 == count, (name, count)
    env.close()


# ---------------------------------------------------------------- b. scattered refill over more than one grid
@pytest.mark.parametrize("order", [False, True])
def test_scattered_refill_over_several_grids_with_failures_mixed_in(zenv_mod, order):
    Z = zenv_mod
    S = PASSES3
    cfg = Z.default_config(0, 3)
    rng = np.random.default_rng(17)
    slots = rng.permutation(S).astype(np.int32)
    seeds = 5000 + np.arange(S, dtype=np.int64)
    bad = np.arange(S) % 17 == 0
    seeds[bad] = np.where(np.arange(bad.sum()) % 2 == 0, -1, 2 ** 32 - 1)
    assert bad.sum() == 964 < Z.SAMPLE_STATUS_CAP           # every one is listed
    twins = [_order(Z, cfg, 2, device_routes=bool(i)) if order else Z.ZoneVecEnv(cfg, 2) for i in range(2)]
    for env in twins:
        env.build_bank_seeds(np.full(S, 77, np.int64))
    total0 = twins[1].sample_status()["n_sampled_total"]
    twins[0].update_bank(slots[~bad], seeds[~bad])
    twins[1].update_bank_device(slots, seeds)
    st = twins[1].sample_status()
    got = twins[1].read_bank()
    assert _same_rows(twins[0].read_bank(), got) == []
    assert (got["seeds"][slots[bad]] == 77).all() and np.array_equal(got["seeds"][slots[~bad]], seeds[~bad])
    assert st["n_failed"] == 964 == len(st["slots"])
    listed = sorted(zip(st["slots"].tolist(), st["seeds"].tolist(), st["codes"].tolist()))
    assert listed == sorted((int(sl), int(sd), Z.SAMPLE_SEED_RANGE) for sl, sd in zip(slots[bad], seeds[bad]))
    assert st["n_sampled_total"] - total0 == S - 964
    st = twins[1].sample_status()
    assert st["n_failed"] == 0 and len(st["slots"]) == 0
    for env in twins:
        env.close()


# ---------------------------------------------------------------- c. the ring over more than one grid
def test_ring_over_several_grids(zenv_mod):
    Z = zenv_mod
    N, depth = 2731, 3
    assert N * depth == MAX_GRID + 1
    seed0 = 1000 * np.arange(N, dtype=np.int64)
    env = Z.ZoneVecEnv("PointTSP-v1", N)
    host = Z.ZoneVecEnv("PointTSP-v1", 2)
    env.ring_stream(seed0, depth)
    total = env.sample_status()["n_sampled_total"]
    assert env.bank_size == N * depth and total == N * depth
    k = 0
    for k_total in (1, 3, 7):                               # 7 >= 2 * depth: the ring wraps twice between two refills
        k_new = k_total - k
        for _ in range(k_new):
            env.reset()
        k = k_total
        env.ring_refill()
        st = env.sample_status()
        assert st["n_failed"] == 0 and st["n_sampled_total"] - total == N * min(k_new, depth), k
        total = st["n_sampled_total"]
        # slot i*depth + j holds episode e_j: the smallest e >= k with e mod depth == j
        j = np.arange(depth)
        e = k + (j - k % depth) % depth
        want_seeds = (seed0[:, None] + e[None, :]).reshape(-1)
        got = env.read_bank()
        assert np.array_equal(got["seeds"], want_seeds), k
        host.build_bank_seeds(want_seeds)
        assert _same_rows(host.read_bank(), got) == [], k
        env.ring_refill()                                   # nothing is stale: nothing is sampled
        st = env.sample_status()
        assert st["n_failed"] == 0 and st["n_sampled_total"] == total, k
    env.reset()
    assert np.array_equal(env.get(Z.F_SEED), seed0 + 7)
    env.close()
    host.close()


# ---------------------------------------------------------------- d. the failure list overflows
def test_failure_list_stops_at_its_cap(zenv_mod):
    """1100 refused seeds in one launch: 1024 are listed, all are counted, nothing behind the list is written -- the
    config's fixed zone locations sit in the same allocation right behind it, and the bank built from them afterwards is
    the host's."""
    Z = zenv_mod
    S, n_bad = 1200, 1100
    rng = np.random.default_rng(5)
    slots = rng.permutation(S).astype(np.int32)
    bad = np.zeros(S, bool)
    bad[rng.permutation(S)[:n_bad]] = True
    i = np.arange(S, dtype=np.int64)
    seeds = np.where(bad, np.where(i % 2 == 0, 2 ** 32 - 1 + i, -1 - i), 7000 + i)      # every refused seed differs
    twins = [Z.ZoneVecEnv("PointTSP-v4", 4) for _ in range(2)]
    assert twins[0].cfg.n_zones_locations == 5
    for env in twins:
        env.build_bank(1, S)
    before = twins[1].read_bank()
    total0 = twins[1].sample_status()["n_sampled_total"]
    twins[0].update_bank(slots[~bad], seeds[~bad])
    twins[1].update_bank_device(slots, seeds)
    st = twins[1].sample_status()
    got = twins[1].read_bank()
    assert st["n_failed"] == n_bad and len(st["slots"]) == Z.SAMPLE_STATUS_CAP == 1024
    assert len(set(st["slots"].tolist())) == 1024
    asked = {int(sl): int(sd) for sl, sd in zip(slots[bad], seeds[bad])}
    assert all(asked.get(sl) == sd for sl, sd in zip(st["slots"].tolist(), st["seeds"].tolist()))
    assert (st["codes"] == Z.SAMPLE_SEED_RANGE).all()
    assert st["n_sampled_total"] - total0 == S - n_bad
    keep = np.zeros(S, bool)
    keep[slots[bad]] = True
    assert _same_rows(before, got, keep) == []              # the refused slots are untouched
    assert _same_rows(twins[0].read_bank(), got) == []      # ... and the 100 others are the host's
    assert np.array_equal(got["seeds"][slots[~bad]], seeds[~bad])
    st = twins[1].sample_status()
    assert st["n_failed"] == 0 and len(st["slots"]) == 0
    twins[0].build_bank(1, 200)
    twins[1].build_bank_device(1, 200)                      # samples from the device copy of zones_locations
    assert _same_rows(twins[0].read_bank(), twins[1].read_bank()) == []
    assert twins[1].sample_status()["n_failed"] == 0
    for env in twins:
        env.close()


def test_builders_wait_for_collected_reports(zenv_mod):
    Z = zenv_mod
    env = Z.ZoneVecEnv("PointTSP-v1", 2)
    env.build_bank(1, 6)
    env.update_bank_device([2, 4], [50, -1])
    want = env.read_bank()
    assert want["seeds"].tolist() == [1, 2, 50, 4, 5, 6]
    for call in (lambda: env.build_bank_device(1, 4), lambda: env.build_bank_seeds_device([3, 4]),
                 lambda: env.ring_stream([1, 9], 2)):
        with pytest.raises(Z.ZenvError) as ei:
            call()
        assert ei.value.code == Z.E_STATE and "zenv_sample_status" in str(ei.value)
        assert env.bank_size == 6 and _same_rows(want, env.read_bank()) == []
    st = env.sample_status()
    assert st["n_failed"] == 1 and st["slots"].tolist() == [4] and st["seeds"].tolist() == [-1]
    env.build_bank_device(1, 4)
    host = Z.ZoneVecEnv("PointTSP-v1", 2)
    host.build_bank(1, 4)
    assert _same_rows(host.read_bank(), env.read_bank()) == []
    env.close()
    host.close()


def test_synchronous_build_with_more_failures_than_the_list_holds(zenv_mod):
    """TIGHT seeds 1..2000: the device gives up on more than 1024, the report names only the first 1024, so the builder
    looks at every slot -- and the bank is the host's.  One notch tighter the host fails on seed 1078: the builder says
    so and leaves the handle as it was."""
    Z = zenv_mod
    seeds = np.arange(1, 2001, dtype=np.int64)
    hard = host_restarts(Z, 1.589, 1, 2001)[:2000] > Z.DEVICE_RESTARTS
    assert hard.sum() > Z.SAMPLE_STATUS_CAP
    env = Z.ZoneVecEnv(tight_config(Z), 2)
    env.build_bank_seeds(seeds)
    want = env.read_bank()
    env.build_bank(5, 3)
    env.build_bank_seeds_device(seeds)
    assert env.bank_size == 2000 and _same_rows(want, env.read_bank()) == []
    st = env.sample_status()
    assert st["n_failed"] == 0 and len(st["slots"]) == 0
    assert st["n_sampled_total"] == int((~hard).sum())      # the device wrote what it could finish, the host the rest
    env.close()

    assert host_restarts(Z, 1.590, 1, 2000)[1077] == HOST_ATTEMPTS
    env = Z.ZoneVecEnv(tight_config(Z, 1.590), 2)
    env.build_bank(1, 3)
    before = env.read_bank()
    with pytest.raises(Z.ZenvError) as ei:
        env.build_bank_seeds_device(seeds)
    assert ei.value.code == Z.E_LAYOUT and "seed 1078" in str(ei.value)
    assert env.bank_size == 3 and _same_rows(before, env.read_bank()) == []
    assert env.sample_status()["n_failed"] == 0
    env.build_bank_device(1, 3)                             # the handle still builds an ordinary bank
    assert _same_rows(before, env.read_bank()) == []
    env.close()


def test_ring_repair_loop_with_more_failures_than_the_list_holds(zenv_mod):
    """What ParallelEnv._repair does after a ring_refill: update_bank on the listed slots and, when more failed than
    were listed, ring_refill again -- which names the rest only because update_bank rewrote the repaired slots' seeds."""
    Z = zenv_mod
    N = 2000
    seed0 = np.arange(1, N + 1, dtype=np.int64)
    hard = host_restarts(Z, 1.589, 1, 2001)[1:] > Z.DEVICE_RESTARTS        # seeds 2..2001: slot i's next episode
    cap = Z.SAMPLE_STATUS_CAP
    assert cap < hard.sum() < 2 * cap
    env = Z.ZoneVecEnv(tight_config(Z), N)
    env.ring_stream(seed0, 1)
    env.reset()
    total0 = env.sample_status()["n_sampled_total"]
    env.ring_refill()
    st = env.sample_status()
    assert st["n_failed"] == int(hard.sum()) and len(st["slots"]) == cap
    assert (st["codes"] == Z.SAMPLE_UNFINISHED).all()
    first = st["slots"]
    assert len(set(first.tolist())) == cap and hard[first].all() and np.array_equal(st["seeds"], seed0[first] + 1)
    total1 = st["n_sampled_total"]
    assert total1 - total0 == int((~hard).sum())
    env.update_bank(st["slots"], st["seeds"])
    env.ring_refill()
    st = env.sample_status()
    rest = np.setdiff1d(np.flatnonzero(hard), first)
    assert st["n_failed"] == len(rest) == len(st["slots"])
    assert np.array_equal(np.sort(st["slots"]), rest)       # exactly the remaining hard ones, none already repaired
    order = np.argsort(st["slots"])
    assert np.array_equal(st["seeds"][order], seed0[rest] + 1) and (st["codes"] == Z.SAMPLE_UNFINISHED).all()
    assert st["n_sampled_total"] == total1
    env.update_bank(st["slots"], st["seeds"])
    env.ring_refill()
    st = env.sample_status()
    assert st["n_failed"] == 0 and len(st["slots"]) == 0 and st["n_sampled_total"] == total1
    host = Z.ZoneVecEnv(tight_config(Z), 2)
    host.build_bank_seeds(seed0 + 1)
    assert _same_rows(host.read_bank(), env.read_bank()) == []
    env.close()
    host.close()


def test_ring_that_runs_off_the_seed_range(zenv_mod):
    Z = zenv_mod
    top = 2 ** 32 - 1
    env = Z.ZoneVecEnv("PointTSP-v1", 2)
    env.ring_stream([top - 2, 10], 2)                       # slots: top - 2, top - 1 | 10, 11
    before = env.read_bank()
    assert before["seeds"].tolist() == [top - 2, top - 1, 10, 11]
    env.reset()                                             # episode 0 taken: slot j wants the smallest e >= 1 with e mod 2 == j
    host = Z.ZoneVecEnv("PointTSP-v1", 2)
    host.build_bank_seeds([top - 2, top - 1, 12, 11])
    for _ in range(2):                                      # the slot stays stale: every refill reports it again
        env.ring_refill()
        st = env.sample_status()
        assert st["n_failed"] == 1 and st["slots"].tolist() == [0] and st["seeds"].tolist() == [top]
        assert st["codes"].tolist() == [Z.SAMPLE_SEED_RANGE]
        got = env.read_bank()
        assert _same_rows(before, got, slice(0, 2)) == [] and _same_rows(host.read_bank(), got) == []
    assert st["n_sampled_total"] == 4 + 1
    env.close()
    host.close()
