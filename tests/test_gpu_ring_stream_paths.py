"""The streamed layout ring (zenv_ring_stream / zenv_ring_refill, K20 and K21) under every way of stepping a handle and
under the five collectors, where envs desynchronise: k_ring_stale sees a different episode index for each env, a call
takes between 0 and `depth` maps from an env's ring, and the refill is enqueued behind one call and before the next with
no host synchronisation.

Handle A is the code under test: ring_stream(seed0, depth), ring_refill() after every call that can take a map (reset()
and reset(mask) included), nothing that synchronises between a refill and the call after it.  Handle B is the reference:
the same config and calls over a host-built bank of seed0[i] + e, e = 0 .. E - 1, on a host-laid ring so deep (E maps per
env, more than the sequence takes) that it never wraps and is never refilled -- its slot arithmetic has nothing to do
with a refill.  After every call every public field the call writes is compared by value, bit for bit: both handles run
the same kernels on the same layouts, so no comparison here has a tolerance.

Independent of B: ZENV_F_SEED[i] == seed0[i] + k_i - 1 after every call, k_i = the maps env i has taken, counted from the
explicit resets made and the done flags the calls recorded; and, in sequences that may synchronise, the layouts a refill
samples (sample_status) and the bank's seeds column (read_bank) against the numpy model of the contract
(tests/ring_model.py)."""
import importlib.util
import os

import numpy as np
import pytest

from tests import hier_ref, option_ref, skill_ref, xy_ref
from tests.layout_scale_cases import MAX_GRID, host_restarts, tight_config
from tests.ring_model import RingModel
from tests.skill_collect_ref import random_inverse_state_dict
from tests.test_gpu_state_paths import _fields

pytestmark = pytest.mark.gpu

SEED = 0x5EED
S, L, H = 4, 4, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANK_FIELDS = ("robot", "zone_xy", "aux", "seeds", "first")


def _tsp(Z, num_steps):
    """PointTSP-v1 with zones of radius 3.5 in the 6 x 6 arena (nearly every step visits a zone) and a time-saved bonus
    of 0.37 per step: the config of tests/test_gpu_episode_log.py, returns that are neither 0 nor whole numbers."""
    return Z.config_for_id("PointTSP-v1", num_steps=num_steps, zones_size=3.5, time_saved_reward=0.37)


def _record_fields(nat):
    """Every ZENV_F_EXP_*, ZENV_F_LO_* and ZENV_F_HI_* buffer: a collector's are those with a size after its call."""
    return sorted((getattr(nat, name), name) for name in dir(nat) if name.startswith(("F_EXP_", "F_LO_", "F_HI_")))


# what test_gpu_episode_log.py::test_taking_the_log_leaves_the_records_alone lists, by collector: these must be there
_EXP = ("F_EXP_OBS", "F_EXP_ZONE_OBS", "F_EXP_ACTION", "F_EXP_LOG_PROB", "F_EXP_VALUE", "F_EXP_REWARD", "F_EXP_MASK",
        "F_EXP_ADVANTAGE", "F_EXP_RETURN")
_HI = ("F_LO_ENV_REWARD", "F_HI_OBS", "F_HI_ZONE_OBS", "F_HI_VALUE", "F_HI_LOG_PROB", "F_HI_ADVANTAGE", "F_HI_RETURN",
       "F_HI_REWARD", "F_HI_MASK", "F_HI_COUNT")
RECORDS = {"flat": _EXP, "hier": _EXP + _HI + ("F_HI_ACTION",), "skills": _EXP + _HI + ("F_HI_ACTION", "F_LO_SKILL"),
           "diayn": _EXP + _HI + ("F_HI_ACTION", "F_LO_SKILL", "F_LO_DIVERSITY"),
           "options": _EXP + _HI + ("F_HI_ACTION", "F_LO_SKILL", "F_LO_TERM_ACTION", "F_LO_TERM_LOG_PROB",
                                    "F_LO_OPTION_ENDED"),
           "xy": _EXP + _HI + ("F_HI_GOAL", "F_LO_GOAL", "F_LO_GOAL_DIST")}


def _raw(Z, env, field):
    a = np.empty(env.field_bytes(field), np.uint8)
    Z._native.check(Z._native.lib().zenv_get(env._h, field, a.ctypes.data, 0))
    return a


class Twin:
    """Handles A (streamed ring, refilled) and B (a host ring of `maps` maps per env, never refilled) and the count of
    maps each env has taken."""

    def __init__(self, Z, cfg, n, depth, maps, timed=False, order=False, prepare=None, seed0=None, refill=True, **over):
        self.Z, self.nat, self.n, self.depth, self.maps, self.order = Z, Z._native, n, depth, maps, order
        self.seed0 = 5000 + 1000 * np.arange(n, dtype=np.int64) if seed0 is None else np.asarray(seed0, np.int64)
        assert maps < 1000 or seed0 is not None              # the envs' seed ranges stay apart: a foreign slot shows
        self.a, self.b = Z.ZoneVecEnv(cfg, n, **over), Z.ZoneVecEnv(cfg, n, **over)
        for e in (self.a, self.b):
            if timed:
                e.timed_layouts_device()                     # both on the shared sampler's deadlines
            if order:
                e.enable_order()                             # before the bank: the routes ride in it
        if order:
            self.a.order_routes_device()                     # A solves its tours on the device (K21), B on the host
        self.a.ring_stream(self.seed0, depth)
        seeds = (self.seed0[:, None] + np.arange(maps, dtype=np.int64)[None, :]).reshape(-1)
        if timed:
            self.b.build_bank_seeds_device(seeds)            # build_bank_seeds on such a handle is the libm sampler
        else:
            self.b.build_bank_seeds(seeds)
        self.b.schedule_ring(np.arange(n, dtype=np.int32) * maps, maps)
        if prepare:
            for e in (self.a, self.b):
                prepare(e)
        self.refill = refill
        self.model = RingModel(self.seed0, depth)
        self.k = np.zeros(n, np.int64)
        self.episodes = np.zeros(n, np.int64)
        self.seen = set()
        self.judging = True
        self.log = []                                        # (tag, what _outputs() read of A) of every compared call

    def close(self):
        assert self.k.max() <= self.maps, "B's ring wrapped: the reference needs more maps"
        self.a.close()
        self.b.close()

    # ------------------------------------------------------------------ reading
    def _outputs(self, env, kind):
        out = {name: env.get(f) for name, f in _fields(self.Z)}
        out["seed"] = env.get(self.nat.F_SEED)
        if kind in ("every", "last"):
            out["chunk_reward"], out["chunk_done"] = env.chunk_results()
        if self.order:
            out["shaped_reward"], out["order_val"] = env.order_info()
            out["order_pos"] = env.order_routes()
        if kind in RECORDS:
            for f, name in _record_fields(self.nat):
                if env.field_bytes(f):
                    out[name] = _raw(self.Z, env, f)
            assert set(RECORDS[kind]) <= set(out), (kind, sorted(set(RECORDS[kind]) - set(out)))
            for key, v in env.episode_logs().items():
                out["log:" + key] = np.asarray(v)
        return out

    @staticmethod
    def same(a, b, tag):
        assert a.keys() == b.keys(), (tag, sorted(set(a) ^ set(b)))
        for name in a:
            x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
            assert x.dtype == y.dtype and x.shape == y.shape, (tag, name, x.dtype, y.dtype, x.shape, y.shape)
            rows = x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8)
            assert not rows.any(), (tag, name, int(rows.sum()), np.flatnonzero(rows)[:8])

    def _taken(self, kind, out, mask):
        """Maps every env took in the call, from what the call recorded on A."""
        episodes = out["episodes"].astype(np.int64)
        ended, self.episodes = episodes - self.episodes, episodes
        if kind == "reset":
            assert not ended.any()
            return np.ones(self.n, np.int64) if mask is None else np.asarray(mask).astype(np.int64)
        if kind == "step":
            taken = out["done"].astype(np.int64)
        elif kind == "every":
            taken = out["chunk_done"].sum(axis=0).astype(np.int64)
        elif kind == "last":
            taken = out["chunk_done"][-1].astype(np.int64)   # finished envs wait, the chunk's last step resets them
        else:
            taken = ended                                    # rollouts and collectors keep no per-step done flags
        assert np.array_equal(taken, ended), (kind, taken[:8], ended[:8])
        return taken

    # ------------------------------------------------------------------ calling
    def call(self, fn, kind, tag, mask=None, refill=None, judge=True):
        """fn(env) on both handles; A's ring was refilled behind the previous call with no synchronisation since.
        Everything the call wrote is read and compared, then A's refill is enqueued (refill=False: the caller's
        business; judge=False: the call is part of a group between two refills that the caller judges)."""
        fn(self.a)
        fn(self.b)
        out = self._outputs(self.a, kind)
        taken = self._taken(kind, out, mask)
        assert taken.max() <= self.depth, tag                # the guard's rule
        self.k += taken
        self.model.take_counts(taken)
        assert np.array_equal(self.model.k, self.k)
        wrong = np.flatnonzero(out["seed"] != self.seed0 + self.k - 1)       # independent of B: the seed identity
        assert wrong.size == 0, (tag, "seed identity", wrong[:8], (out["seed"] - self.seed0)[wrong[:8]], self.k[wrong[:8]])
        self.same(out, self._outputs(self.b, kind), tag)
        self.taken = taken
        if kind != "reset" and judge:
            self.judge(taken)
        self.log.append((tag, out))
        if (self.refill if refill is None else refill):
            self.ring_refill()
        return out

    def judge(self, taken):
        """What the envs took between two refills of the driven sequence (resets and the stagger do not count)."""
        if not self.judging:
            return
        if (taken == self.depth).any():
            self.seen.add("full")
        if (taken == 0).any():
            self.seen.add("zero")
        if taken.min() < taken.max():
            self.seen.add("mixed")

    def ring_refill(self):
        self.a.ring_refill()
        stale = self.model.refill()
        if self.k.min() < self.k.max():
            self.seen.add("desync")
        if 0 < stale < self.n * self.depth:
            self.seen.add("partial")
        return stale

    def reset(self, mask=None, tag="reset"):
        m = None if mask is None else np.asarray(mask, np.uint8)
        return self.call(lambda e: e.reset(m), "reset", tag, mask=m)

    def stagger(self):
        """Env i starts (2, 1, 0, 3)[i % 4] steps into its episode (tests/test_gpu_episode_log.py's start): three steps,
        a ragged reset(mask) after each, a refill behind every one of the six calls."""
        zero = np.zeros((self.n, 2), np.float32)
        self.judging = False
        for g in range(3):
            self.call(lambda e: e.step(zero, auto_reset=True), "step", ("stagger step", g))
            self.reset(np.arange(self.n) % 4 == g, ("stagger reset", g))
        self.judging = True

    STAGGER_MAPS = 5                                         # at most: three auto-resets, one masked reset, and one spare


def _must_see(t, want):
    """The conditions that keep a sequence from passing vacuously."""
    assert want <= t.seen, (sorted(want - t.seen), sorted(t.seen))


# ============================================================================ stepping paths
def _actions(rng, K, n):
    """Host actions with a few NaNs (the exception branch ends an episode early: irregular lengths)."""
    a = rng.uniform(-1, 1, (K, n, 2)).astype(np.float32)
    a[rng.random((K, n)) < 0.01, 0] = np.nan
    return a


def _drive(Z, t, path, depth, calls, rng):
    """`calls` calls of `path` on the twin, each of them as many auto-resetting steps as the ring guard allows."""
    n = t.n
    for c in range(calls):
        tag = (path, c)
        if path == "step":
            # `depth` single steps and ONE refill behind them: the contract's limit, not a refill per step
            group = np.zeros(n, np.int64)
            for s in range(depth):
                a = _actions(rng, 1, n)[0]
                t.call(lambda e: e.step(a, auto_reset=True), "step", tag + (s,), refill=False, judge=False)
                group += t.taken
            t.judge(group)
            t.ring_refill()
        elif path in ("many_every", "reset_mask"):
            a = _actions(rng, depth, n)
            t.call(lambda e: e.step_many(a, reset="every"), "every", tag)
            if path == "reset_mask":
                t.reset(rng.random(n) < 0.3, tag + ("mask",))
        elif path == "many_last":
            a = _actions(rng, depth + 1, n)                  # K > depth: allowed, only the last step resets
            t.call(lambda e: e.step_many(a, reset="last"), "last", tag)
        else:
            mode = {"rollout_persistent": "persistent", "rollout_sliced": "persistent", "rollout_per_step": "per_step",
                    "rollout_unfused": "unfused"}[path]
            t.call(lambda e: e.rollout(depth, Z.POLICY_UNIFORM, SEED, mode=mode), "rollout", tag)


def _want(path, n, depth, num_steps):
    """What a sequence of `path` must have met, by its episode lengths: an episode lasts num_steps steps (fewer after a
    NaN action), a call is `depth` auto-resetting steps (many_last: depth + 1 steps, one reset)."""
    want = set()
    if n > 1:
        want.add("desync")                                   # the stagger's masked resets alone
    if n * depth > 1:
        want.add("partial")
    if path == "many_last":
        if depth == 1:
            want.add("full")
        if depth + 1 < num_steps:
            want.add("zero")
    else:
        if num_steps == 1 or depth == 1:
            want.add("full")                                 # an episode ends on every step / a call is one step
        if depth < num_steps:
            want.add("zero")                                 # some call ends no episode of some env
    return want


PATHS = ("step", "many_every", "many_last", "rollout_persistent", "rollout_per_step", "rollout_unfused", "reset_mask")
SHAPES = [(n, d, s) for n in (1, 65, 130) for d in (1, 2, 3, 4) for s in (1, 3)]        # (N, depth, num_steps)
CASES = [(p, n, d, s) for p in PATHS for (n, d, s) in SHAPES] + \
    [("rollout_sliced", 130, d, s) for d in (1, 2, 3, 4) for s in (1, 3)]


@pytest.mark.parametrize("path,n,depth,num_steps", CASES)
def test_stepping_paths_play_the_streamed_maps(zenv_mod, path, n, depth, num_steps):
    """5 calls (episodes of one step) or 9 (of three): every ring wraps more than once."""
    Z = zenv_mod
    calls = 5 if num_steps == 1 else 9
    if path == "many_last":
        calls = 2 * depth + 3                                # a call takes at most one map
    per_call = depth + (1 if path == "reset_mask" else 0)
    t = Twin(Z, _tsp(Z, num_steps), n, depth, 1 + Twin.STAGGER_MAPS + calls * (1 if path == "many_last" else per_call))
    if path == "rollout_sliced":
        for e in (t.a, t.b):
            e.set_rollout_slice(64)                          # a launch covers one tile of the three
    t.reset()
    t.stagger()
    _drive(Z, t, path, depth, calls, np.random.default_rng(len(path) + 10 * n + depth))
    assert t.k.min() > 2 * depth, t.k.min()                  # every ring wrapped more than once
    _must_see(t, _want(path, n, depth, num_steps))
    t.close()


def test_a_sequence_nobody_reads(zenv_mod):
    """call, refill, call, refill, ... with no read and no synchronisation at all (rollouts enqueued only): the state
    at the end equals B's, and the seeds the envs are on follow from the episodes they finished."""
    Z = zenv_mod
    nat = Z._native
    n, depth, calls = 130, 3, 9
    t = Twin(Z, _tsp(Z, 3), n, depth, 2 + calls * 2 * depth + calls)
    rng = np.random.default_rng(4)
    masks = [(rng.random(n) < 0.3).astype(np.uint8) for _ in range(calls)]
    chunks = [_actions(rng, depth, n) for _ in range(calls)]
    for e, refill in ((t.a, t.a.ring_refill), (t.b, lambda: None)):
        e.reset()
        refill()
        for c in range(calls):
            e.rollout(depth, Z.POLICY_UNIFORM, SEED, mode="persistent", wait=False)
            refill()
            e.reset(masks[c])
            refill()
            e.step_many(chunks[c], reset="every")
            refill()
    out = t._outputs(t.a, "every")
    t.same(out, t._outputs(t.b, "every"), "unread")
    k = 1 + np.sum(masks, axis=0) + out["episodes"]
    assert np.array_equal(out["seed"], t.seed0 + k - 1)
    assert k.min() < k.max() and k.min() > 2 * depth
    t.k = k
    t.close()


# ============================================================================ the solver-ordered handle
@pytest.mark.parametrize("path,n,depth,num_steps", [("step", 65, 2, 3), ("many_every", 65, 3, 3), ("many_last", 130, 2, 3),
                                                    ("many_every", 130, 4, 1), ("reset_mask", 1, 2, 3)])
def test_solver_ordered_handle_plays_the_streamed_maps(zenv_mod, path, n, depth, num_steps):
    """order_routes_device: A's tours are solved by the wave that samples the layout, B's on the host; order_info() and
    order_routes() are compared too.  zenv_rollout refuses such a handle (as the collectors do), streamed ring or not."""
    Z = zenv_mod
    calls = 2 * depth + 3 if path == "many_last" else (5 if num_steps == 1 else 9)
    per_call = 1 if path == "many_last" else depth + (1 if path == "reset_mask" else 0)
    t = Twin(Z, _tsp(Z, num_steps), n, depth, 1 + Twin.STAGGER_MAPS + calls * per_call, order=True)
    t.reset()
    t.stagger()
    _drive(Z, t, path, depth, calls, np.random.default_rng(n + depth))
    assert t.k.min() > 2 * depth
    _must_see(t, _want(path, n, depth, num_steps))
    assert any(np.any(out["order_val"] != 0) for _, out in t.log) and any(np.any(out["order_pos"] >= 0) for _, out in t.log)
    before = t.a.get_state()
    with pytest.raises(Z.ZenvError) as ei:
        t.a.rollout(1, Z.POLICY_UNIFORM, SEED)
    assert ei.value.code == Z.E_STATE and "zenv_step" in str(ei.value)
    assert np.array_equal(t.a.get_state(), before)
    t.close()


# ============================================================================ collectors
def _load(Z, env, kind):
    """The kind's random tiny networks (tests/test_gpu_episode_log.py's)."""
    from oracle import policy_ref as P
    F = env.zone_feat
    if kind == "flat":
        env.load_mlp(P.random_tensors(F, h=H, seed=3, critic=True), precision="f32")
    elif kind == "hier":
        env.enable_goals()
        env.load_hier(Z.hier_tensors_from_state_dicts(*hier_ref.random_state_dicts(F, h=H, seed=3)))
    elif kind in ("skills", "diayn"):
        env.load_skills(Z.skill_tensors_from_state_dicts(*skill_ref.random_state_dicts(F, S, h=H, seed=3)), skill_len=L)
        if kind == "diayn":
            env.load_skill_inverse(Z.inverse_tensors_from_state_dict(random_inverse_state_dict(F, S, h=H, seed=4), S))
    elif kind == "options":
        env.load_options(Z.option_tensors_from_state_dicts(*option_ref.random_state_dicts(F, S, h=H, seed=3)))
    else:
        env.load_xy(Z.xy_tensors_from_state_dicts(*xy_ref.random_state_dicts(F, h=H, seed=3)), skill_len=L)


def _collect(env, kind, T, call):
    seed = 100 + call
    if kind == "flat":
        env.collect_on_device(T, policy_seed=seed)
    elif kind == "hier":
        env.collect_hier_on_device(T, policy_seed=seed)
    elif kind == "skills":
        env.collect_skills_on_device(T, policy_seed=seed)
    elif kind == "diayn":
        env.collect_skills_on_device(T, policy_seed=seed, diversity_coef=0.5,
                                     skill_prior_logits=np.linspace(-1, 1, S).astype(np.float32))
    elif kind == "options":
        env.collect_options_on_device(T, policy_seed=seed)
    else:
        env.collect_xy_on_device(T, policy_seed=seed)


# (case, task config, collector, num_steps, calls): a call is `depth` frames, or `depth` windows of L frames
COLLECTORS = {
    "flat": ("tsp", "flat", 3, 8), "hier": ("tsp", "hier", 2, 8), "skills": ("tsp", "skills", 6, 6),
    "diayn": ("tsp", "diayn", 6, 6), "options": ("tsp", "options", 3, 8), "xy": ("tsp", "xy", 6, 6),
    "timed_flat": ("timed", "flat", 16, 20), "colour_flat": ("colour", "flat", 4, 9),
}


@pytest.mark.parametrize("case", sorted(COLLECTORS))
def test_collectors_play_the_streamed_maps(zenv_mod, case):
    """N = 65, depth = 3, h = 32.  Every record the collector fills, the episode logs and the handle's fields after
    every collection.  TimedTSP: device deadlines on both handles, episodes of at most 16 steps so that deadlines
    expire."""
    Z = zenv_mod
    task, kind, num_steps, calls = COLLECTORS[case]
    n, depth = 65, 3
    windowed = kind in ("skills", "diayn", "xy")
    T = depth * L if windowed else depth
    cfg = {"tsp": lambda: _tsp(Z, num_steps), "timed": lambda: Z.config_for_id("PointTTSP-v1", num_steps=num_steps),
           "colour": lambda: Z.config_for_id("ColourMatch-v0", num_steps=num_steps)}[task]()
    t = Twin(Z, cfg, n, depth, 1 + Twin.STAGGER_MAPS + calls * depth, timed=task == "timed",
             prepare=lambda e: _load(Z, e, kind))
    t.reset()
    if kind != "hier":                                       # a goal-conditioned handle is stepped with goals only
        t.stagger()
    for c in range(calls):
        out = t.call(lambda e: _collect(e, kind, T, c), kind, (case, c))
    assert t.k.min() > depth and t.k.max() > 2 * depth, (t.k.min(), t.k.max())       # the rings wrapped
    want = {"partial"}
    if kind != "hier":
        want.add("desync")
    if num_steps > T:
        want.add("zero")
    _must_see(t, want)
    if task == "timed":
        assert len(np.unique(t.a.read_bank()["aux"])) > 8    # deadlines all over the 16 steps: some expire
    if task == "tsp":
        assert any(np.any(o["log:return_per_episode"] != 0) for _, o in t.log if "log:return_per_episode" in o)
    t.close()


@pytest.mark.parametrize("kind", ["flat", "skills"])
def test_collectors_take_a_whole_ring_in_one_call(zenv_mod, kind):
    """Episodes of one step: every frame (every window of the skill collector) takes a map, `depth` of them a call."""
    Z = zenv_mod
    n, depth, calls = 65, 3, 5
    T = depth * L if kind == "skills" else depth
    t = Twin(Z, _tsp(Z, 1), n, depth, 1 + Twin.STAGGER_MAPS + calls * depth, prepare=lambda e: _load(Z, e, kind))
    t.reset()
    t.stagger()
    for c in range(calls):
        t.call(lambda e: _collect(e, kind, T, c), kind, (kind, c))
    _must_see(t, {"full", "desync", "partial"})
    assert "zero" not in t.seen and t.k.min() > 2 * depth
    t.close()


# ============================================================================ more than one sampling grid
def test_mixed_staleness_over_more_than_one_grid(zenv_mod):
    """N = 4097, depth = 4: 16 388 slots, three trips of the refill's grid-stride loops for some blocks, with rings
    that are stale by a different amount each."""
    Z = zenv_mod
    n, depth, calls = 4097, 4, 4
    assert n * depth > 2 * MAX_GRID
    t = Twin(Z, _tsp(Z, 3), n, depth, 1 + Twin.STAGGER_MAPS + calls * depth)
    t.reset()
    t.stagger()
    for c in range(calls):
        t.call(lambda e: e.rollout(depth, Z.POLICY_UNIFORM, SEED, mode="persistent"), "rollout", ("grid", c))
    _must_see(t, {"desync", "partial", "mixed"})
    assert t.k.min() > depth
    t.close()


# ============================================================================ the guard on a streamed ring
def test_guard_edge_on_a_streamed_ring(zenv_mod):
    """The rule host rings have (tests/test_gpu_state_paths.py::test_collectors_refuse_to_outrun_a_ring): depth + 1
    auto-resetting steps or frames in one call is E_STATE and leaves the handle untouched; exactly `depth` passes and
    plays the maps it must."""
    Z = zenv_mod
    n, depth = 65, 3
    env = Z.ZoneVecEnv(_tsp(Z, 1), n)
    seed0 = 700 + 50 * np.arange(n, dtype=np.int64)
    env.ring_stream(seed0, depth)
    _load(Z, env, "flat")
    env.reset()
    env.ring_refill()
    k = 1
    a = np.zeros((depth + 1, n, 2), np.float32)
    over = (lambda: env.rollout(depth + 1, Z.POLICY_UNIFORM, SEED), lambda: env.rollout(depth + 1, Z.POLICY_UNIFORM, SEED, mode="per_step"),
            lambda: env.rollout(depth + 1, Z.POLICY_UNIFORM, SEED, mode="unfused"), lambda: env.step_many(a, reset="every"),
            lambda: env.collect_on_device(depth + 1, policy_seed=3))
    at = (lambda: env.rollout(depth, Z.POLICY_UNIFORM, SEED), lambda: env.rollout(depth, Z.POLICY_UNIFORM, SEED, mode="per_step"),
          lambda: env.rollout(depth, Z.POLICY_UNIFORM, SEED, mode="unfused"), lambda: env.step_many(a[:depth], reset="every"),
          lambda: env.collect_on_device(depth, policy_seed=3))
    for refused, allowed in zip(over, at):
        before = env.get_state()
        with pytest.raises(Z.ZenvError) as ei:
            refused()
        assert ei.value.code == Z.E_STATE
        assert np.array_equal(env.get_state(), before)
        allowed()
        k += depth
        assert np.array_equal(env.get(Z.F_SEED), seed0 + k - 1)
        env.ring_refill()
    env.step_many(a, reset="last")                           # depth + 1 steps, one reset: allowed
    assert np.array_equal(env.get(Z.F_SEED), seed0 + k)
    env.close()


# ============================================================================ snapshot
def test_snapshot_rewinds_the_ring(zenv_mod):
    """get_state() after call 2; calls 3 and 4 with their refills; set_state(), ring_refill() -- the ring now holds
    episodes past the rewound episode index, the refill must bring the earlier ones back -- and calls 3 and 4 again give
    the recorded outputs bit for bit."""
    Z = zenv_mod
    n, depth = 65, 3
    t = Twin(Z, _tsp(Z, 3), n, depth, 1 + Twin.STAGGER_MAPS + 4 * depth + 4)
    rng = np.random.default_rng(9)
    chunks = [_actions(rng, depth, n) for _ in range(4)]
    t.reset()
    t.stagger()

    def run(c):
        if c % 2:
            return t.call(lambda e: e.step_many(chunks[c], reset="every"), "every", ("snap", c))
        return t.call(lambda e: e.rollout(depth, Z.POLICY_UNIFORM, SEED, mode="persistent"), "rollout", ("snap", c))
    run(0)
    run(1)
    blobs = t.a.get_state(), t.b.get_state()
    k2, episodes2, step2 = t.k.copy(), t.episodes.copy(), t.a.step_count
    first = [run(2), run(3)]
    assert (t.k > k2).all()                                  # every env moved on: every ring holds later episodes now
    t.a.set_state(blobs[0])
    t.b.set_state(blobs[1])
    assert t.a.step_count == step2
    t.k, t.episodes = k2.copy(), episodes2.copy()
    t.model.k = k2.copy()
    assert t.ring_refill() > 0
    again = [run(2), run(3)]
    for c, (x, y) in enumerate(zip(first, again)):
        t.same(x, y, ("replayed", 2 + c))
    t.close()


# ============================================================================ the refill's work (may synchronise)
@pytest.mark.parametrize("n,depth,num_steps", [(1, 2, 3), (65, 1, 3), (65, 3, 3), (130, 4, 1)])
def test_a_refill_samples_what_was_taken(zenv_mod, n, depth, num_steps):
    """sample_status()["n_sampled_total"] grows over each refill by sum_i (k_i now - k_i at the previous refill), every
    term at most `depth`; read_bank()["seeds"] is slot j <- seed0 + e_j, e_j = k_i + (j - k_i mod depth) mod depth, with
    each env's own k_i; at the end the whole bank is the host sampler's for those seeds."""
    Z = zenv_mod
    calls = 6
    t = Twin(Z, _tsp(Z, num_steps), n, depth, 1 + Twin.STAGGER_MAPS + calls * (depth + 1), refill=False)
    rng = np.random.default_rng(n + depth)
    total = t.a.sample_status()["n_sampled_total"]
    assert total == n * depth
    k_prev = t.k.copy()
    sampled = []

    def refill(tag):
        nonlocal total, k_prev
        grew = t.k - k_prev
        assert grew.max() <= depth
        stale = t.ring_refill()
        st = t.a.sample_status()
        assert st["n_failed"] == 0
        assert st["n_sampled_total"] - total == grew.sum() == stale, (tag, st["n_sampled_total"] - total, grew.sum(), stale)
        total, k_prev = st["n_sampled_total"], t.k.copy()
        sampled.append(stale)
        e = t.k[:, None] + (np.arange(depth)[None, :] - t.k[:, None] % depth) % depth
        assert np.array_equal(t.model.held, e)
        assert np.array_equal(t.a.read_bank()["seeds"], t.model.bank_seeds()), tag
        t.a.ring_refill()                                    # nothing is stale: nothing is sampled
        assert t.a.sample_status()["n_sampled_total"] == total, tag

    zero = np.zeros((n, 2), np.float32)
    t.reset()
    refill("reset")
    for g in range(3):                                       # the stagger, a checked refill behind each call
        t.call(lambda e: e.step(zero, auto_reset=True), "step", ("stagger step", g))
        refill(("stagger step", g))
        t.reset(np.arange(n) % 4 == g, ("stagger reset", g))
        refill(("stagger reset", g))
    for c in range(calls):
        if c % 2:
            a = _actions(rng, depth, n)
            t.call(lambda e: e.step_many(a, reset="every"), "every", ("work", c))
        else:
            t.call(lambda e: e.rollout(depth, Z.POLICY_UNIFORM, SEED, mode="persistent"), "rollout", ("work", c))
        refill(("work", c))
        t.reset(rng.random(n) < 0.3, ("work mask", c))
        refill(("work mask", c))
    assert any(0 < s < n * depth for s in sampled) or n * depth == 1
    if n > 1:
        assert "desync" in t.seen
    host = Z.ZoneVecEnv(_tsp(Z, num_steps), 2)
    host.build_bank_seeds(t.model.bank_seeds())
    want, got = host.read_bank(), t.a.read_bank()
    assert [f for f in BANK_FIELDS if not np.array_equal(want[f].view(np.uint8), got[f].view(np.uint8))] == []
    host.close()
    t.close()


# ============================================================================ repair in the loop
def test_repair_in_the_loop(zenv_mod):
    """A config the device sampler gives up on for most seeds (tight_config), episodes of one step, depth 2, the flat
    collector: between calls what ParallelEnv._repair does -- sample_status(), update_bank() on the listed slots.  The
    list is exactly the stale slots whose seed needs more host restarts than a device wave is allowed; the host
    finishes every one; A equals B throughout."""
    Z = zenv_mod
    n, depth, calls = 8, 2, 5
    seed0 = 1 + 40 * np.arange(n, dtype=np.int64)
    maps = 2 + calls * depth
    restarts = host_restarts(Z, 1.589, 1, 2001)
    played = (seed0[:, None] + np.arange(maps + depth)[None, :]).reshape(-1)
    assert played.max() <= 2001 and restarts[played - 1].max() < 10000       # the host finishes every seed
    t = Twin(Z, tight_config(Z), n, depth, maps, prepare=lambda e: _load(Z, e, "flat"), seed0=seed0, refill=False,
             num_steps=1)
    given_up = 0

    def refill_and_repair(tag):
        nonlocal given_up
        want = t.model.wanted_held()
        slots = np.flatnonzero((want != t.model.held).reshape(-1))
        seeds = (seed0[:, None] + want).reshape(-1)[slots]
        hard = restarts[seeds - 1] > Z.DEVICE_RESTARTS
        t.ring_refill()
        st = t.a.sample_status()
        order = np.argsort(st["slots"])
        assert st["n_failed"] == hard.sum() == len(st["slots"]), (tag, st["n_failed"], hard.sum())
        assert np.array_equal(st["slots"][order], slots[hard]) and np.array_equal(st["seeds"][order], seeds[hard]), tag
        assert (st["codes"] == Z.SAMPLE_UNFINISHED).all()
        if st["n_failed"]:
            t.a.update_bank(st["slots"], st["seeds"])
        given_up += int(st["n_failed"])
        assert np.array_equal(t.a.read_bank()["seeds"], t.model.bank_seeds()), tag

    t.reset()
    refill_and_repair("reset")
    for c in range(calls):
        t.call(lambda e: _collect(e, "flat", depth, c), "flat", ("repair", c))
        refill_and_repair(("repair", c))
    assert given_up >= 1                                     # the device gave up on at least one seed
    _must_see(t, {"full"})
    assert np.array_equal(t.k, np.full(n, 1 + calls * depth))
    t.close()


# ============================================================================ the example's call order
def _load_ppo_example():
    spec = importlib.util.spec_from_file_location("ppo_torch_example", os.path.join(ROOT, "examples", "ppo_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("updates", [1, 2])
def test_the_examples_call_order_plays_every_map_once(zenv_mod, monkeypatch, updates):
    """examples/ppo_torch.py --fresh-layouts as it stands: train() with episodes of one step and frames_per_proc =
    depth, so that every collection takes `depth` maps of every env.  What the handle holds when train() closes it --
    the seed each env is on, its observation (the first of that map) and its episode count -- equals twin B's after the
    same number of steps; the first collection's last map is episode `depth`, not a replay of episode 0 (which is what
    the loop played before it refilled behind its initial reset(): updates = 1 failed then; after a second collection
    the ring had recovered, so updates = 2 only checks that the loop goes on playing the stream)."""
    pytest.importorskip("torch")
    Z = zenv_mod
    nat = Z._native
    ex = _load_ppo_example()
    n, depth, seed = 65, 3, 7
    final = {}

    class Spy(Z.ZoneVecEnv):
        def close(self):
            if getattr(self, "_h", None) is not None and self._h.value:
                for name, f in (("seed", nat.F_SEED), ("obs", nat.F_OBS), ("zone_obs", nat.F_ZONE_OBS),
                                ("episodes", nat.F_EPISODES)):
                    final[name] = self.get(f)
            super().close()

    class Package:                                           # the example's `Z`, with the spying handle
        def __getattr__(self, name):
            return Spy if name == "ZoneVecEnv" else getattr(Z, name)

    monkeypatch.setattr(ex, "Z", Package())
    cfg = _tsp(Z, 1)
    ex.train(env_id=cfg, procs=n, frames_per_proc=depth, updates=updates, epochs=1, batch_size=n * depth, hidden=H,
             seed=seed, log=lambda row: None, fresh_layouts=True)
    seed0 = seed + (np.arange(n, dtype=np.int64) << 20)
    maps = 1 + updates * depth
    assert np.array_equal(final["episodes"], np.full(n, updates * depth, np.int32))
    b = Z.ZoneVecEnv(cfg, n)
    b.build_bank_seeds((seed0[:, None] + np.arange(maps, dtype=np.int64)[None, :]).reshape(-1))
    b.schedule_ring(np.arange(n, dtype=np.int32) * maps, maps)
    b.reset()
    for _ in range(updates):
        b.step_many(np.zeros((depth, n, 2), np.float32), reset="every")     # an episode is one step whatever the action
    for name, f in (("seed", nat.F_SEED), ("obs", nat.F_OBS), ("zone_obs", nat.F_ZONE_OBS), ("episodes", nat.F_EPISODES)):
        assert np.array_equal(final[name], b.get(f)), name
    assert np.array_equal(final["seed"], seed0 + maps - 1)
    b.close()
