"""tests/philox_ref.py, the host restatement of the device's draws, against the Random123 known answers of
Philox4x32-10 and the properties of its uniform mapping (CPU only)."""
import numpy as np
import pytest

from tests import philox_ref as R

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    assert [int(x) for x in R.philox4x32_10(ctr, key)] == list(want)


def test_vectorised_equals_scalar():
    rs = np.random.RandomState(1)
    ctr = [rs.randint(0, 2 ** 32, 64, dtype=np.uint64) for _ in range(4)]
    key = [rs.randint(0, 2 ** 32, 64, dtype=np.uint64) for _ in range(2)]
    out = R.philox4x32_10(ctr, key)
    for i in range(0, 64, 7):
        one = R.philox4x32_10([c[i] for c in ctr], [k[i] for k in key])
        assert [int(x[i]) for x in out] == [int(x) for x in one]


def test_uniform_mapping():
    x = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFEFF, 0xFFFFFFFF], np.uint32)
    u = R.uniform(x)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -25) and u[1] == u[0] and u[2] == np.float32(1.5 * 2.0 ** -24)
    # above 2^23 the + 0.5 rounds to even in float32: the device's top uniform is exactly 1
    assert u[-1] == np.float32(1.0) and 0 < u.min() and u.max() <= 1
    assert np.all(np.diff(u) >= 0)


def test_streams_are_keyed_by_tag_env_step_and_seed():
    n = 4096
    g = R.goal_uniform(n, 7, 0, 3)
    s = R.skill_uniform(n, 7, 0, 3)
    assert g.shape == (n,) and g.dtype == np.float32 and not np.array_equal(g, s)
    assert np.array_equal(R.goal_uniform(n - 5, 7, 5, 3), g[5:])          # the global env index, not the local one
    assert not np.array_equal(R.goal_uniform(n, 7, 0, 4), g)
    assert not np.array_equal(R.goal_uniform(n, 8, 0, 3), g)
    assert not np.array_equal(R.goal_uniform(n, 7 + (1 << 32), 0, 3), g)  # both key words
    # the upper counter word: env index 2^32 + i is not env i
    assert not np.array_equal(R.goal_uniform(4, 7, 1 << 32, 3), g[:4])
    for u in (g, s):
        assert abs(u.mean() - 0.5) < 0.02 and 0 < u.min() and u.max() <= 1
    eps = R.action_noise(n, 7, 0, 3)
    assert eps.shape == (n, 2) and eps.dtype == np.float64
    assert abs(eps.mean()) < 0.05 and abs(eps.std() - 1) < 0.05 and abs(np.corrcoef(eps.T)[0, 1]) < 0.05
    # the action stream is the counter of tag 0x4D4C50: its first word is the first Box-Muller uniform
    c = R.philox4x32_10((np.arange(n, dtype=np.uint64), 0, 3, R.TAG_ACTION), (7, 0))
    u1 = R.uniform(c[0]).astype(np.float64)
    assert np.allclose(np.hypot(eps[:, 0], eps[:, 1]), np.sqrt(-2 * np.log(u1)), rtol=1e-12, atol=1e-12)
