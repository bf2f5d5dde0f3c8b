"""The streamed ring's contract (zenv_ring_stream / zenv_ring_refill, include/zenv.h) as a few lines of numpy: env i owns
`depth` slots, slot j holds one episode index, a take reads slot k mod depth and moves k on, a refill puts into slot j
the smallest episode e >= k with e mod depth == j.  tests/test_ring_model_cpu.py checks the contract on it without a
GPU; tests/test_gpu_ring_stream_paths.py takes the bank seeds it expects of the device from it."""
import numpy as np


class RingModel:
    def __init__(self, seed0, depth):
        self.seed0 = np.asarray(seed0, np.int64).copy()
        self.depth = int(depth)
        n = len(self.seed0)
        self.k = np.zeros(n, np.int64)                                   # maps env i has taken = its next episode's index
        self.held = np.tile(np.arange(self.depth, dtype=np.int64), (n, 1))   # episode held by slot j of env i

    def take(self, mask=None):
        """Every env under `mask` (None: all) takes a map.  Returns (episode it wanted, episode its slot held), [N]
        each, -1 where the env took nothing: the two differ where a map is replayed."""
        m = np.ones(len(self.k), bool) if mask is None else np.asarray(mask).astype(bool)
        i = np.flatnonzero(m)
        wanted = np.full(len(self.k), -1, np.int64)
        got = wanted.copy()
        wanted[i] = self.k[i]
        got[i] = self.held[i, self.k[i] % self.depth]
        self.k[i] += 1
        return wanted, got

    def take_counts(self, counts):
        """Env i takes counts[i] maps, one at a time.  Returns how many of them were not the episode wanted."""
        counts = np.asarray(counts, np.int64)
        wrong = 0
        for t in range(int(counts.max(initial=0))):
            wanted, got = self.take(counts > t)
            wrong += int((wanted != got).sum())
        return wrong

    def wanted_held(self):
        j = np.arange(self.depth, dtype=np.int64)[None, :]
        k = self.k[:, None]
        return k + (j - k % self.depth) % self.depth

    def refill(self):
        """Brings every ring back ahead of its env.  Returns how many slots changed: the layouts a refill samples."""
        want = self.wanted_held()
        stale = int((want != self.held).sum())
        self.held = want
        return stale

    def bank_seeds(self):
        """The seeds column of the bank, slot i * depth + j."""
        return (self.seed0[:, None] + self.held).reshape(-1)

    def played_seed(self):
        """Seed of the map each env is on (ZENV_F_SEED) if no map was replayed or skipped; needs k >= 1."""
        return self.seed0 + self.k - 1
