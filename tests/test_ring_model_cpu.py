"""The streamed ring's contract on its numpy model (tests/ring_model.py), without a GPU: up to `depth` takes per env
between two refills always read the episode wanted; one more replays a map; and so does a reset() followed by `depth`
takes with no refill in between -- the explicit reset took a map too (the order examples/ppo_torch.py had)."""
import numpy as np
import pytest

from tests.ring_model import RingModel

DEPTHS = (1, 2, 3, 4, 7)


@pytest.mark.parametrize("depth", DEPTHS)
def test_takes_within_the_depth_read_the_episode_wanted(depth):
    rng = np.random.default_rng(depth)
    n = 130
    seed0 = rng.integers(0, 2 ** 31, n)
    ring = RingModel(seed0, depth)
    assert np.array_equal(ring.bank_seeds(), (seed0[:, None] + np.arange(depth)).reshape(-1))
    total = np.zeros(n, np.int64)
    seen_partial = seen_none = seen_all = False
    for call in range(40):
        counts = rng.integers(0, depth + 1, n)               # 0 .. depth, a different count for each env
        if call % 8 == 7:
            counts[:] = 0
        if call % 8 == 3:
            counts[:] = depth
        assert ring.take_counts(counts) == 0, call
        total += counts
        assert np.array_equal(ring.k, total)
        if total.min() > 0:
            assert np.array_equal(ring.played_seed(), seed0 + total - 1)
        stale = ring.refill()
        assert stale == counts.sum(), call                   # a refill samples what was taken since the last, no more
        seen_partial |= 0 < stale < n * depth
        seen_none |= stale == 0
        seen_all |= stale == n * depth
        assert ring.refill() == 0                            # nothing is stale: nothing is sampled
        held = ring.held
        assert np.array_equal(held % depth, np.tile(np.arange(depth), (n, 1)))
        assert np.all(held >= total[:, None]) and np.all(held < total[:, None] + depth)
        assert np.array_equal(ring.bank_seeds().reshape(n, depth), seed0[:, None] + held)
    assert seen_none and seen_all and (seen_partial or depth == 1 and n == 1)
    assert total.min() < total.max() and total.min() > 2 * depth   # desynchronised, every ring wrapped more than once


@pytest.mark.parametrize("depth", DEPTHS)
def test_one_take_more_than_the_depth_replays_a_map(depth):
    ring = RingModel([100, 2000], depth)
    ring.take_counts([2, 5])                                 # anywhere in the stream
    ring.refill()
    k = ring.k.copy()
    assert ring.take_counts([depth, depth]) == 0
    wanted, got = ring.take([True, False])
    assert wanted[0] == k[0] + depth and got[0] == k[0]      # the slot still holds the episode played `depth` takes ago
    assert wanted[1] == got[1] == -1
    ring.refill()                                            # a refill repairs the ring from the env's episode index
    assert ring.take_counts([depth, depth]) == 0


@pytest.mark.parametrize("depth", DEPTHS)
def test_reset_then_depth_takes_without_a_refill_replays_a_map(depth):
    """reset(), then a first collection that ends `depth` episodes of an env, with no refill after the reset: the
    collection's last take wants episode `depth` from slot 0, which still holds episode 0."""
    ring = RingModel([7], depth)
    wanted, got = ring.take()                                # the explicit reset: episode 0
    assert wanted[0] == got[0] == 0
    for e in range(1, depth):
        wanted, got = ring.take()
        assert wanted[0] == got[0] == e
    wanted, got = ring.take()
    assert wanted[0] == depth and got[0] == 0
    # ... and with the refill after the reset the same collection plays episodes 1 .. depth
    ring = RingModel([7], depth)
    ring.take()
    assert ring.refill() == 1
    assert ring.take_counts([depth]) == 0
    assert ring.played_seed()[0] == 7 + depth
