"""TEST INFRASTRUCTURE -- ordering of the library's entry points on a caller's BUSY side stream.

The value tests run every call on an idle device, on the handle's own stream or on the legacy null stream (which
serialises against every blocking stream): a launch that took the wrong stream, or a copy out of caller memory that the
call did not wait for, still finishes "in time" there.  Here the handle sits on a torch side stream (non-blocking, like
the handle's own) that is stalled by a calibrated ``torch.cuda._sleep``; the calls under test are issued while the
stall is still running -- a ``marker`` event right behind the sleep proves it -- and the results are compared bit for
bit with a twin handle that ran the same sequence with a ``sync()`` after every call.

``CLASSES`` puts every ``zenv_*`` function of ``_native._PROTOTYPES`` into exactly one class
(tests/test_stream_contract_cpu.py keeps the table complete):

  ASYNC      returns with its work enqueued: the marker is still pending afterwards
  WAITS      synchronises the handle's stream: the marker is complete on return and what the call hands back is as of
             everything enqueued before it
  HOST_ARG   asynchronous, but reads caller HOST memory when given a host pointer (the same call with NULL or a device
             pointer is ASYNC).  Pageable memory may be overwritten the moment the call returns; page-locked memory
             (zenv_host_alloc) only once the stream has reached the call.  No pending assertion: whether the runtime
             stages a pageable source or waits for the stream is the runtime's business and is only recorded (measured:
             it returns at once up to a 0.5 MB source and waits for the stream at 8 MB)
  NO_DEVICE  nothing is put on, or waited for on, a handle's stream (the reason stands beside each)
"""
import contextlib

import numpy as np

ASYNC, WAITS, HOST_ARG, NO_DEVICE = "ASYNC", "WAITS", "HOST_ARG", "NO_DEVICE"
DEFAULT_STALL_MS, MAX_STALL_MS = 150.0, 500.0

_HOST = "host arithmetic on its arguments"
_FIELD = "reads a host-side member of the handle"
_FLAG = "sets a host-side switch that later launches take by value"
_PTR = "hands out an address or a size; the memory is not touched"
_CHECK = "validates its arguments on the host"
_STEP = "the host's count of Adam steps ENQUEUED so far (it moves when an update call returns, not when it has run)"
_OWN = "no handle: allocates its own buffers and waits for them on the null stream"

_LEARNERS = ("ppo", "hppo", "xyppo", "skppo", "opppo", "diayn")


def _table():
    t = {}

    def put(cls, names, why=""):
        for n in names.split():
            assert n not in t, n
            t[n] = (cls, why)

    # ---- nothing on a handle's stream
    put(NO_DEVICE, "zenv_last_error zenv_version zenv_build_flags zenv_rollout_chunk zenv_config_size", "a constant")
    put(NO_DEVICE, "zenv_device_count", "asks the runtime for the device count; creates no context")
    put(NO_DEVICE, "zenv_config_for_id zenv_default_config zenv_zone_feat zenv_sample_layout zenv_fixed_seed_sequence "
                   "zenv_sample_layout_shared zenv_sample_layout_timed zenv_layout_thresholds zenv_route_ranks "
                   "zenv_route_ranks_shared", _HOST)
    put(NO_DEVICE, "zenv_num_envs zenv_get_config zenv_bank_size zenv_step_count zenv_state_bytes zenv_field_bytes "
                   "zenv_results_layout zenv_comm_info", _FIELD)
    put(NO_DEVICE, "zenv_order_configure zenv_skill_configure zenv_set_rollout_slice zenv_timed_layouts_device "
                   "zenv_order_routes_device", _FLAG)
    put(NO_DEVICE, " ".join(f"zenv_{p}_check" for p in _LEARNERS) + " zenv_render_check", _CHECK)
    put(NO_DEVICE, " ".join(f"zenv_{p}_tensor" for p in _LEARNERS) + " zenv_episode_log_tensor", _PTR)
    put(NO_DEVICE, " ".join(f"zenv_{p}_{g}et_step" for p in _LEARNERS for g in "gs"), _STEP)
    put(NO_DEVICE, "zenv_diayn_prior_init zenv_diayn_prior_read zenv_diayn_prior_write",
        "the skill prior's logits and Adam state live on the host (the first also allocates the histogram)")
    put(NO_DEVICE, "zenv_host_alloc zenv_host_free", "page-locked host memory; no stream involved")
    put(NO_DEVICE, "zenv_comm_unique_id", "asks RCCL for an id; no handle")
    put(NO_DEVICE, "zenv_det_ops zenv_probe_store_stream", _OWN)
    # ---- asynchronous on the handle's stream
    put(ASYNC, "zenv_policy zenv_mlp_forward zenv_hier_forward zenv_skill_forward zenv_option_forward zenv_xy_forward")
    put(ASYNC, "zenv_collect zenv_collect_skill zenv_collect_xy",
        "once the experience buffers of that T exist; zenv_collect_skill reads its host prior during the call")
    put(ASYNC, "zenv_bank_update zenv_bank_update_device",
        "the host arguments are copied into a page-locked image during the call; a second call while the first one's "
        "copy is still queued waits for it (the image's event)")
    put(ASYNC, "zenv_ring_refill zenv_episode_log_reset")
    put(ASYNC, " ".join(f"zenv_{p}_apply" for p in _LEARNERS))
    put(ASYNC, "zenv_device_ptr", "the fields kept inside the step kernels' records are unpacked stream-ordered")
    put(ASYNC, "zenv_query", "asks whether the stream is idle; never waits")
    # ---- asynchronous, may read caller host memory
    put(HOST_ARG, "zenv_reset", "mask")
    put(HOST_ARG, "zenv_step", "actions with actions_on_device == 0")
    put(HOST_ARG, "zenv_step_many", "actions with actions_on_device == 0 (the first chunk of a size allocates: WAITS)")
    put(HOST_ARG, " ".join(f"zenv_{p}_minibatch zenv_{p}_epoch" for p in _LEARNERS), "idx / order with on_device == 0")
    put(HOST_ARG, "zenv_render", "marks with marks_on_device == 0; with a host dst the call is WAITS")
    # ---- synchronise the handle's stream
    put(WAITS, "zenv_create zenv_destroy zenv_set_stream zenv_sync")
    put(WAITS, "zenv_bank_build zenv_bank_build_seeds zenv_bank_set zenv_bank_build_device zenv_bank_build_seeds_device "
               "zenv_ring_stream zenv_sample_status zenv_bank_read zenv_route_ranks_device")
    put(WAITS, "zenv_schedule_sequential zenv_schedule_ring zenv_schedule_fixed_seeds")
    put(WAITS, "zenv_order_enable zenv_order_rows zenv_goal_enable zenv_set_goals zenv_solver_goals zenv_set_skills "
               "zenv_set_xy_goals")
    put(WAITS, "zenv_mlp_load zenv_hier_load zenv_skill_load zenv_skill_inverse_load zenv_option_load zenv_xy_load")
    put(WAITS, "zenv_rollout", "ASYNC with ZENV_ROLLOUT_ASYNC")
    put(WAITS, "zenv_collect_hier zenv_collect_option", "one synchronisation, to learn M")
    put(WAITS, " ".join(f"zenv_{p}_init zenv_{p}_read zenv_{p}_write" for p in _LEARNERS))
    put(WAITS, "zenv_diayn_samples zenv_diayn_prior_update", "one synchronisation, to learn a count / the histogram")
    put(WAITS, "zenv_get zenv_get_rows zenv_get_many zenv_step_results zenv_host_io zenv_step_host zenv_get_state "
               "zenv_set_state zenv_debug_state")
    put(WAITS, "zenv_episode_log zenv_episode_log_read zenv_episode_log_stats")
    put(WAITS, "zenv_comm_init zenv_comm_destroy zenv_allgather zenv_comm_barrier zenv_comm_allreduce_max",
        "multi-GPU: classified, tested by the RCCL tests only")
    return t


CLASSES = _table()


def class_of(name):
    return CLASSES[name][0]


# ------------------------------------------------------------------ the stall
_cycles_per_ms = None
OBSERVED = {}          # HOST_ARG call -> set of "returned at once" / "blocked until the stall ended"


def side_stream():
    import torch
    return torch.cuda.Stream()


def cycles_per_ms():
    """``torch.cuda._sleep`` cycles per millisecond on this device, measured once per process with two events on a
    side stream (no clock rate is assumed: the sleep is lengthened until it takes a measurable time)."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        s = side_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles, ms = 1_000_000, 0.0
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)                # (the kernel's first launch loads its code object)
            s.synchronize()
            for _ in range(6):
                e0.record(s)
                torch.cuda._sleep(cycles)
                e1.record(s)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 20.0:
                    break
                cycles = int(cycles * min(max(30.0 / max(ms, 1e-3), 2.0), 1000.0))
        assert ms >= 5.0, f"a sleep of {cycles} cycles took {ms} ms: not measurable"
        _cycles_per_ms = cycles / ms
        print(f"[stream_stall] torch.cuda._sleep: {_cycles_per_ms:.0f} cycles per ms ({cycles} cycles in {ms:.2f} ms)")
    return _cycles_per_ms


def stall(stream, ms=DEFAULT_STALL_MS):
    """A sleep of `ms` on `stream` and a marker event right behind it; returns the marker."""
    import torch
    assert 0 < ms <= MAX_STALL_MS, ms
    cycles = int(cycles_per_ms() * ms)
    marker = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        marker.record(stream)
    return marker


def assert_still_pending(marker, what=""):
    """The stall in front of the calls under test is still running.  If it is not, nothing was shown."""
    assert not marker.query(), f"INCONCLUSIVE: the stall ended before {what or 'the calls under test'} returned"


def assert_complete(marker, what=""):
    assert marker.query(), f"{what or 'the call'} returned while the stream had not reached it: it did not synchronise"


class Stalled:
    """Issues calls on a handle whose side stream is kept stalled, by class:

      st.run(ASYNC, "what", fn)       fn(), then the marker must still be pending
      st.run(WAITS, "what", fn)       fn(), then the marker must be complete (what fn returned is returned); the next
                                      call gets a fresh stall
      st.run(HOST_ARG, "what", fn)    fn(), whether it returned at once or blocked is recorded in OBSERVED; re-armed

    The twin runs the same calls through ``Synced``."""
    stalled = True

    def __init__(self, env, stream, ms=DEFAULT_STALL_MS, max_stalls=10):
        self.env, self.stream, self.ms = env, stream, ms
        self.marker, self.stalls, self.max_stalls = None, 0, max_stalls

    def arm(self, fresh=False):
        """A stall is in front of the next call: the running one, or a new one when that has ended -- or, with `fresh`,
        a new one behind whatever is queued (before a call whose enqueueing takes long)."""
        if fresh or self.marker is None or self.marker.query():
            assert self.stalls < self.max_stalls, "more stalls than the test was sized for"
            self.stalls += 1
            self.marker = stall(self.stream, self.ms)
        return self.marker

    def torch(self, fresh=False):
        """Context: torch work of the sequence goes on the stalled stream, BEHIND a stall that is still running -- a
        tensor the next call reads is then still to be computed when that call is issued."""
        import torch
        assert_still_pending(self.arm(fresh), "the torch work in front of the call under test was enqueued")
        return torch.cuda.stream(self.stream)

    def torch_idle(self):
        """Context: torch work on the handle's stream while NO stall is running (pre-filling a buffer)."""
        import torch
        assert self.marker is None or self.marker.query(), "a stall is still running"
        return torch.cuda.stream(self.stream)

    def run(self, cls, what, fn, fresh=False):
        marker = self.arm(fresh)
        out = fn()
        if cls == ASYNC:
            assert_still_pending(marker, what)
        elif cls == WAITS:
            assert_complete(marker, what)
            self.marker = None
        else:
            assert cls == HOST_ARG, cls
            OBSERVED.setdefault(what, set()).add(
                "blocked until the stall ended" if marker.query() else "returned at once")
        return out

    def finish(self):
        self.stream.synchronize()
        self.marker = None


class Synced:
    """The twin's driver, and the warm-up's: every call with a ``sync()`` behind it; the sequence's torch work runs on
    `stream` (None: torch's current stream) between two device synchronisations."""
    stalled = False

    def __init__(self, env, stream=None):
        self.env, self.stream = env, stream

    @contextlib.contextmanager
    def torch(self, fresh=False):
        import torch
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext():
            yield
        torch.cuda.synchronize()

    torch_idle = torch

    def run(self, cls, what, fn, fresh=False):
        out = fn()
        self.env.sync()
        return out

    def finish(self):
        self.env.sync()


def print_observed():
    for what in sorted(OBSERVED):
        print(f"[stream_stall] HOST_ARG {what}: {', '.join(sorted(OBSERVED[what]))}")


# ------------------------------------------------------------------ the twin comparison
def published(Z, env):
    """Every published per-env field as host arrays (each zenv_get synchronises)."""
    nat = Z._native
    fields = dict(obs=nat.F_OBS, zone_obs=nat.F_ZONE_OBS, reward=nat.F_REWARD, done=nat.F_DONE, goal_met=nat.F_GOAL_MET,
                  exception=nat.F_EXCEPTION, episodes=nat.F_EPISODES, last_return=nat.F_LAST_RETURN,
                  last_len=nat.F_LAST_LEN, ep_return=nat.F_EP_RETURN, ep_len=nat.F_EP_LEN, actions=nat.F_ACTIONS)
    return {name: env.get(f) for name, f in fields.items()}


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
        bad = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))
        raise AssertionError(f"{what}: {bad.size} of {a.nbytes} bytes differ from the twin's, first at byte {bad[0]}")


def same_dicts(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], dict):
            same_dicts(a[k], b[k], f"{what}.{k}")
        else:
            same_bits(np.asarray(a[k]), np.asarray(b[k]), f"{what}.{k}")


def assert_twins_equal(Z, env, twin, what, extra=None):
    """get_state() blobs and every published field bit for bit; extra(env) -> dict of the arrays the sequence wrote."""
    same_bits(env.get_state(), twin.get_state(), f"{what}: get_state")
    same_dicts(published(Z, env), published(Z, twin), what)
    assert env.step_count == twin.step_count, what
    if extra is not None:
        same_dicts(extra(env), extra(twin), what)


# ------------------------------------------------------------------ a handle on a side stream and its twin
N = 257          # a ragged last wave and workgroup


def _host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def pick_side_stream(Z, env, also_reset=(), tries=8, ms=30.0):
    """A side stream that does not share a hardware queue with the handle's own stream.  Streams are spread over a few
    hardware queues, and work on two streams of one queue runs in issue order: a launch that strayed to the handle's own
    stream would then wait behind the stall by accident and go unnoticed.  Probe: with a candidate stalled, a policy
    launch into a scratch tensor on the handle's own stream (no state of the handle changes) must finish while the stall
    is still running.  `env` and the handles of `also_reset` (its twin) are reset once, so that they keep one history.
    Without such a stream a run cannot tell a stray launch from a right one: it fails as inconclusive."""
    import torch
    for e in (env,) + tuple(also_reset):
        e.reset()
        e.sync()
    probe = torch.zeros(env.num_envs, 2, device="cuda")
    torch.cuda.synchronize()
    for _ in range(tries):
        side = side_stream()                                       # (torch hands its pool's streams out in turn)
        marker = stall(side, ms)
        env.policy(Z.POLICY_UNIFORM, dst_ptr=probe.data_ptr())
        while not env.done() and not marker.query():               # bounded by the stall
            pass
        independent = env.done() and not marker.query()
        side.synchronize()
        env.sync()
        if independent:
            return side
    raise AssertionError(f"INCONCLUSIVE: none of {tries} side streams runs beside the handle's own stream (they share "
                         "its hardware queue): a launch on the wrong stream could not be told from a right one")


class Pair:
    """Handle A on a side stream, and its twin on its own."""

    def __init__(self, Z, make):
        import torch
        from combinatorial_rl_tasks_amd.torch_interop import TorchZoneEnv
        self.Z, self.torch = Z, torch
        self.env, self.twin = make(), make()
        try:
            self.side = pick_side_stream(Z, self.env, also_reset=(self.twin,))
        except BaseException:
            self.env.close()
            self.twin.close()
            raise
        with torch.cuda.stream(self.side):
            self.tenv = TorchZoneEnv(self.env)                     # puts the handle on the current (side) stream
        self.ttwin = TorchZoneEnv(self.twin, use_current_stream=False)
        self.tenv.scratch, self.ttwin.scratch = {}, {}

    def check(self, sequence, what, extra=None, **stall):
        Z, torch = self.Z, self.torch
        sequence(Z, Synced(self.env, self.side), self.tenv, 0)
        sequence(Z, Synced(self.twin), self.ttwin, 0)
        torch.cuda.synchronize()
        st = Stalled(self.env, self.side, **stall)
        got = sequence(Z, st, self.tenv, 1)
        st.finish()
        assert st.stalls >= 1
        want = sequence(Z, Synced(self.twin), self.ttwin, 1)
        torch.cuda.synchronize()
        same_dicts({k: _host(v) for k, v in (got or {}).items()}, {k: _host(v) for k, v in (want or {}).items()}, what)
        assert_twins_equal(Z, self.env, self.twin, what, extra)
        return st

    def close(self):
        self.torch.cuda.synchronize()
        for e in (self.env, self.twin):
            e.set_stream(None)
            e.close()
