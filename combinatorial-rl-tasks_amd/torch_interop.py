"""Zero-copy hand-off between the env buffers and a device-resident PyTorch policy.

The reference moves every observation to the host and every action back
(``main/src/torch_ac/algos/base.py:139-145``: ``preprocess_obss(self.obs, device)`` ...
``action.cpu().numpy()`` ... ``self.env.step``).  Here the env's output buffers are exposed as
``torch`` tensors that ALIAS device memory (no copy, through ``__cuda_array_interface__``), the
env is put on torch's current stream, and ``step`` takes the action tensor's device address: a
closed loop policy -> step -> policy never leaves the GPU and needs no synchronisation.

torch is plumbing here (device memory, streams); no env arithmetic runs through it.
"""
import numpy as np

from . import _native as nat
from .vec_env import _FIELD_DTYPES

_TYPESTR = {np.dtype(np.float32): "<f4", np.dtype(np.float64): "<f8", np.dtype(np.uint8): "|u1",
            np.dtype(np.int32): "<i4", np.dtype(np.int64): "<i8"}


class _DeviceView:
    """Minimal __cuda_array_interface__ (v2) carrier for a buffer owned by the env handle."""

    def __init__(self, ptr, shape, dtype):
        self.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": _TYPESTR[np.dtype(dtype)],
                                         "data": (int(ptr), False), "version": 2, "strides": None}


# The thin learner methods TorchZoneEnv has of each family (key -> calls), the rest of a family's being written out in
# the class.  ppo / a2c name their tensor views `views`.
_PAIR_CALLS = ("init", "tensors", "set_tensors", "state_dicts", "load_state_dicts", "optimizer_state",
               "load_optimizer_state", "minibatch", "apply", "epoch", "stats", "publish", "update")
_ACCESS_CALLS = ("tensor_ptr", "get_step", "set_step")
_TORCH_CALLS = {
    "ppo": ("views", "state_dict", "load_state_dict", "optimizer_state", "load_optimizer_state", "minibatch", "apply",
            "epoch", "stats"),
    "a2c": ("views", "state_dict", "load_state_dict", "optimizer_state", "load_optimizer_state", "apply", "stats"),
    "hppo": _PAIR_CALLS, "xyppo": _PAIR_CALLS, "skppo": _PAIR_CALLS, "opppo": _PAIR_CALLS + _ACCESS_CALLS,
    "diayn": ("tensors", "set_tensors", "state_dict", "load_state_dict", "optimizer_state", "load_optimizer_state",
              "minibatch", "apply", "epoch", "stats") + _ACCESS_CALLS,
}


_WEIGHTS = {"hppo": "zenv_hier_weights", "xyppo": "zenv_xy_weights", "skppo": "zenv_skill_weights",
            "opppo": "zenv_option_weights", "diayn": "zenv_skill_inverse_weights"}


def _torch_docs(key, weights):
    """call -> docstring of the installed methods that have one."""
    if key in ("ppo", "a2c"):
        optimiser = "Adam" if key == "ppo" else "RMSprop"
        return {
            "views": "zenv_mlp_weights name -> CUDA tensor ALIASING that tensor of an arena, in its state_dict shape.",
            "state_dict": "The learner's parameters under ACModel's state_dict names, as CUDA tensors ALIASING the "
                          f"parameter arena:\n        ``model.load_state_dict(tenv.{key}_state_dict())`` copies them "
                          "into a torch module on the shared stream.",
            "load_state_dict": "Overwrite the learner's parameters from an ACModel state_dict (tensors on any device), "
                               "on the stream.",
            "optimizer_state": f"{optimiser}'s state in the shape of ``torch.optim.{optimiser}.state_dict()``: copies, "
                               "parameter i\n        the i-th of ``ACModel.parameters()``.",
            "minibatch": f"``ZoneVecEnv.{key}_minibatch``; idx may be an int32 CUDA tensor (never copied, checked on the "
                         "device).",
            "epoch": f"``ZoneVecEnv.{key}_epoch``; order may be an int32 CUDA tensor.",
            "stats": "float32 CUDA tensor [minibatches, 6] ALIASING the statistics of the last ppo_minibatch / ppo_epoch "
                     "(not\n        synchronised)." if key == "ppo" else
                     "float32 CUDA tensor [1, 5] ALIASING the statistics of the last a2c_apply / a2c_update (not "
                     "synchronised).",
        }
    level = "" if key == "diayn" else "the level's "
    docs = {
        "tensors": f"{weights} name -> CUDA tensor ALIASING that tensor of " +
                   ("the arena" if key == "diayn" else "a level's arena") + ", in its state_dict shape.",
        "optimizer_state": f"``ZoneVecEnv.{key}_optimizer_state`` with the moments as CUDA copies.",
        "minibatch": f"``ZoneVecEnv.{key}_minibatch``; idx may be an int32 CUDA tensor (never copied, checked on the "
                     "device).",
        "epoch": f"``ZoneVecEnv.{key}_epoch``; order may be an int32 CUDA tensor.",
        "stats": f"float32 CUDA tensor [minibatches, 6] ALIASING the statistics of {level}last {key}_minibatch / "
                 f"{key}_epoch\n        (not synchronised).",
    }
    if key == "diayn":
        docs["state_dict"] = "InverseModel's state_dict as CUDA tensors ALIASING the parameter arena."
        return docs
    docs.update({
        "init": f"``ZoneVecEnv.{key}_init`` with each level's four arenas as flat float32 CUDA tensors ALIASING device "
                f"memory in\n        ``self.{key}_arenas[level]`` (valid until the next {key}_init or ``env.close()``).",
        "set_tensors": "Overwrite the tensors of a level's arena that `tensors` names (tensors on any device), on the "
                       "stream.",
        "state_dicts": "(hi_model_state, lo_model_state) as CUDA tensors ALIASING the two parameter arenas.",
    })
    return docs


def _torch_forwarders(fam):
    """call -> the method <key>_<call> of TorchZoneEnv: the family's piece of the shared implementation, or the env's
    own method where tensors change nothing.  A pair's take the level first."""
    key = fam.key

    def of_env(call):
        return lambda self, *args, **kw: getattr(self.env, f"{key}_{call}")(*args, **kw)

    if fam.levels:
        def init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
            getattr(self.env, key + "_init")(hi_state_dict, lo_state_dict, lo=lo, hi=hi)
            setattr(self, key + "_arenas", {level: self._learner_arenas(key, level) for level in (0, 1)})

        def tensors(self, level, which=nat.PPO_PARAM):
            return self._learner_views(key, level, which)

        def set_tensors(self, level, tensors, which=nat.PPO_PARAM):
            self._learner_set_tensors(key, level, tensors, which)

        def state_dicts(self):
            return self._learner_state_dict(key, 1), self._learner_state_dict(key, 0)

        def load_state_dicts(self, hi_state_dict, lo_state_dict):
            self._learner_load_state_dict(key, 1, hi_state_dict)
            self._learner_load_state_dict(key, 0, lo_state_dict)

        def optimizer_state(self, level):
            return self._learner_optimizer_state(key, level)

        def load_optimizer_state(self, level, state):
            of_env("load_optimizer_state")(self, level, state)

        def minibatch(self, level, idx, apply=False):
            ptr, count = self._ppo_index_arg(idx)
            of_env("minibatch")(self, level, ptr, apply=apply, count=count)

        def apply(self, level):
            of_env("apply")(self, level)

        def epoch(self, level, order, batch_size):
            ptr, count = self._ppo_index_arg(order)
            of_env("epoch")(self, level, ptr, batch_size, count=count)

        def stats(self, level):
            return self._learner_stats(key, level)

        def publish(self):
            of_env("publish")(self)

        def update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
            return of_env("update")(self, epochs, batch_size, hi_epochs, hi_batch_size, rng)

        def tensor_ptr(self, level, which, index):
            return of_env("tensor_ptr")(self, level, which, index)

        def get_step(self, level):
            return of_env("get_step")(self, level)

        def set_step(self, level, step):
            of_env("set_step")(self, level, step)

        return locals()

    def tensors(self, which=nat.PPO_PARAM):
        return self._learner_views(key, None, which)

    def views(self, which=nat.PPO_PARAM):
        return self._learner_views(key, None, which)

    def set_tensors(self, tensors, which=nat.PPO_PARAM):
        self._learner_set_tensors(key, None, tensors, which)

    def state_dict(self):
        return self._learner_state_dict(key)

    def load_state_dict(self, state_dict):
        self._learner_load_state_dict(key, None, state_dict)

    def optimizer_state(self):
        return self._learner_optimizer_state(key)

    def load_optimizer_state(self, state):
        of_env("load_optimizer_state")(self, state)

    def minibatch(self, idx, apply=False):
        ptr, count = self._ppo_index_arg(idx)
        of_env("minibatch")(self, ptr, apply=apply, count=count)

    def apply(self):
        of_env("apply")(self)

    def epoch(self, order, batch_size):
        ptr, count = self._ppo_index_arg(order)
        of_env("epoch")(self, ptr, batch_size, count=count)

    def stats(self):
        return self._learner_stats(key)

    def tensor_ptr(self, which, index):
        return of_env("tensor_ptr")(self, which, index)

    def get_step(self):
        return of_env("get_step")(self)

    def set_step(self, step):
        of_env("set_step")(self, step)

    return locals()


def _install_forwarders(cls):
    from .vec_env import _FAMILIES
    for key, calls in _TORCH_CALLS.items():
        fam = _FAMILIES[key]
        made, docs = _torch_forwarders(fam), _torch_docs(key, _WEIGHTS.get(key))
        for call in calls:
            f = made[call]
            f.__name__ = f"{key}_{call}"
            f.__qualname__ = f"{cls.__name__}.{f.__name__}"
            f.__doc__ = docs.get(call)
            setattr(cls, f.__name__, f)
    return cls


@_install_forwarders
class TorchZoneEnv:
    """Tensor view of a ``ZoneVecEnv``: ``obs (N,8)``, ``zone_obs (N,Z,F)``, ``reward (N,)`` float32,
    ``done``/``goal_met (N,)`` uint8, ``last_return (N,)`` float64, ``episodes (N,)`` int32 -- aliases of the
    env's device buffers, valid until ``env.close()``; they change in place on every ``step``.

    ``ep_return (N,)`` float64 and ``ep_len (N,)`` int32 are properties instead: the running episode's figures live
    inside the step kernels' records, and ``zenv_device_ptr`` hands out a plain copy brought up to date by that call
    (stream-ordered).  Each access re-aliases that copy, so the tensor read holds every step enqueued before the
    access; a tensor kept from an earlier access is only brought up to date by a later access (or a get)."""

    def __init__(self, env, use_current_stream=True):
        import torch
        self._torch = torch
        self.env = env
        self.device = torch.device("cuda", env.device)
        with torch.cuda.device(self.device):
            if use_current_stream:
                env.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
            self.obs = self._alias(nat.F_OBS)
            self.zone_obs = self._alias(nat.F_ZONE_OBS)
            self.reward = self._alias(nat.F_REWARD)
            self.done = self._alias(nat.F_DONE)
            self.goal_met = self._alias(nat.F_GOAL_MET)
            self.last_return = self._alias(nat.F_LAST_RETURN)
            self.episodes = self._alias(nat.F_EPISODES)

    @property
    def ep_return(self):
        """Undiscounted return of the running episode, as of this access (see the class docstring)."""
        with self._torch.cuda.device(self.device):
            return self._alias(nat.F_EP_RETURN)

    @property
    def ep_len(self):
        """Steps of the running episode, as of this access (see the class docstring)."""
        with self._torch.cuda.device(self.device):
            return self._alias(nat.F_EP_LEN)

    def _alias(self, field, shape=None, dtype=None):
        """A tensor over a device buffer of the handle; shape and dtype default to the env's own for that field."""
        view = _DeviceView(self.env.device_ptr(field), self.env._shape(field) if shape is None else shape,
                           _FIELD_DTYPES[field] if dtype is None else dtype)
        t = self._torch.as_tensor(view, device=self.device)
        assert t.data_ptr() == self.env.device_ptr(field), "torch copied instead of aliasing"
        return t

    def _alias_layout(self, layout, skip=False):
        """Every buffer of a layout (name -> (field id, shape, dtype)) aliased.  skip: the buffers hold nothing (no
        high-level row yet) -- empty tensors of the right dtype on the env's device instead."""
        torch = self._torch
        if skip:
            return {name: torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name), device=self.device)
                    for name, (_, shape, dt) in layout.items()}
        return {name: self._alias(field, shape, dt) for name, (field, shape, dt) in layout.items()}

    def reset(self, mask=None):
        self.env.reset(mask)
        return {"obs": self.obs, "zone_obs": self.zone_obs}

    def order_rows(self, enable=True):
        """``ZoneVecEnv.order_rows``: the flat network, ``collect`` (``zone_obs [N, T, Z, 7]``, the shaped reward) and the
        ``ppo_*`` calls on the reference's (Z, 7) rows of a solver-ordered handle.  ``self.zone_obs`` stays the 6-wide
        alias; ``net_rows`` shows what the network reads."""
        self.env.order_rows(enable)

    @property
    def net_zone_feat(self):
        """``ZoneVecEnv.net_zone_feat``: the width of the rows the flat network reads (7 with ``order_rows()`` on)."""
        return self.env.net_zone_feat

    @property
    def net_rows(self):
        """The rows the flat network reads, float32 ``(N, Z, net_zone_feat)``: ``zone_obs`` itself, or with
        ``order_rows()`` on the (Z, 7) rows assembled as of this access (``_native.F_ORDER_ROWS``, stream-ordered)."""
        if self.env.net_zone_feat == self.env.zone_feat:
            return self.zone_obs
        with self._torch.cuda.device(self.device):
            return self._alias(nat.F_ORDER_ROWS)

    def load_state_dict(self, state_dict, precision="auto"):
        """Put an ACModel state_dict (main/src/flat_model.py:24-52 names; torch tensors on any device) into the
        device actor-critic that ``collect`` and the ``POLICY_MLP_*`` action sources run.  precision: see
        ``ZoneVecEnv.load_mlp`` -- the default is float32-grade (the reference's modules are float32); "bf16" is the
        fast reduced-precision mode."""
        from .vec_env import mlp_tensors_from_state_dict
        self.env.load_mlp(mlp_tensors_from_state_dict(state_dict), precision=precision)

    def collect(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """collect_experiences (torch_ac/algos/base.py:131-227) on the device; returns exps.* as float32 CUDA
        tensors [N, T, ...] ALIASING the handle's experience buffers (overwritten by the next collect;
        transposed views of time-major memory, so ``reshape(N*T, ...)`` copies them once).  Enqueued
        on the shared stream like everything else: no synchronisation, no host copy."""
        self.env.collect_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
        raw = self._alias_layout(self.env._experience_rows(frames_per_proc))
        return {name: t.transpose(0, 1) for name, t in raw.items()}     # [N, T, ...] views of time-major memory

    def _alias_ptr(self, ptr, shape, dtype=np.float32):
        t = self._torch.as_tensor(_DeviceView(ptr, shape, dtype), device=self.device)
        assert t.data_ptr() == ptr, "torch copied instead of aliasing"
        return t

    # ------------------------------------------------------------------ the collectors' per-episode logs (K19)
    def episode_logs(self):
        """``ZoneVecEnv.episode_logs`` for the collector that ran last, the per-episode values as CUDA tensors
        (float32; ``env_per_episode`` int32) ALIASING the handle's result buffers: they stay valid until the next
        ``episode_logs`` call, which overwrites (and may reallocate) them.  ``num_frames`` is an int.  Once per
        collection; waits for the device once, to learn how many episodes ended."""
        from .vec_env import episode_log_keys
        info = self.env.episode_log_on_device()
        out = {}
        with self._torch.cuda.device(self.device):
            for key in episode_log_keys(info.columns) + (nat.EPLOG_KEYS[nat.EPLOG_ENV],):
                column = nat.EPLOG_KEYS.index(key)
                ptr, count = self.env.episode_log_ptr(column)
                out[key] = self._alias_ptr(ptr, (count,), np.int32 if column == nat.EPLOG_ENV else np.float32)
        out["num_frames"] = int(info.num_frames)
        return out

    def episode_log_stats(self):
        """``ZoneVecEnv.episode_log_stats``: {key: {"mean", "std", "min", "max"}} of the last ``episode_logs``."""
        return self.env.episode_log_stats()

    def episode_log_reset(self):
        """``ZoneVecEnv.episode_log_reset``: the logs of a fresh algo object."""
        self.env.episode_log_reset()

    # ------------------------------------------------------------------ the device learners
    # One implementation per piece, parameterised by the family (vec_env._FAMILIES) and, for a pair, the level; the
    # thin <key>_* methods are installed from _TORCH_CALLS (_install_forwarders).  Here follow the pieces, then what a
    # family has of its own.
    _ARENAS = (("param", nat.PPO_PARAM), ("grad", nat.PPO_GRAD), ("exp_avg", nat.PPO_EXP_AVG),
               ("exp_avg_sq", nat.PPO_EXP_AVG_SQ))
    _A2C_ARENAS = (("param", nat.A2C_PARAM), ("grad", nat.A2C_GRAD), ("square_avg", nat.A2C_SQUARE_AVG))

    def _learner_arenas(self, family, level=None):
        """name -> flat float32 CUDA tensor ALIASING a whole arena of the learner (padding between the tensors included)."""
        learner = self.env._learner_of(family, level)
        with self._torch.cuda.device(self.device):
            out = {}
            for name, which in (self._A2C_ARENAS if learner.family.rmsprop else self._ARENAS):
                ptr, count = learner.tensor_ptr(which, -1)
                out[name] = self._alias_ptr(ptr, (count,))
            return out

    def _learner_views(self, family, level=None, which=nat.PPO_PARAM):
        """tensor name -> CUDA tensor ALIASING that tensor of an arena, in its state_dict shape."""
        learner = self.env._learner_of(family, level)
        learner._need_init()
        with self._torch.cuda.device(self.device):
            return {name: self._alias_ptr(learner.tensor_ptr(which, i)[0], learner.shapes[name])
                    for i, name in enumerate(learner.keys)}

    def _learner_set_tensors(self, family, level, tensors, which):
        views = self._learner_views(family, level, which)
        for name, src in tensors.items():
            views[name].copy_(self._torch.as_tensor(src))

    def _learner_state_dict(self, family, level=None):
        views = self._learner_views(family, level)
        return {key: views[name] for name, key in self.env._learner_of(family, level).keys.items()}

    def _learner_load_state_dict(self, family, level, state_dict):
        for key, dst in self._learner_state_dict(family, level).items():
            dst.copy_(state_dict[key])

    def _learner_optimizer_state(self, family, level=None):
        """The learner's ``optimizer_state`` with the step as a tensor and the moments as CUDA copies."""
        torch = self._torch
        out = self.env._learner_of(family, level).optimizer_state()
        out["state"] = {i: {k: torch.tensor(v) if k == "step" else torch.from_numpy(v).to(self.device)
                            for k, v in s.items()} for i, s in out["state"].items()}
        return out

    def _learner_stats(self, family, level=None):
        learner = self.env._learner_of(family, level)
        field, cols = learner.stats_field, learner.family.stats_cols
        rows = self.env.field_bytes(field) // (4 * cols)
        with self._torch.cuda.device(self.device):
            return self._alias(field, (rows, cols), np.float32)

    def _ppo_index_arg(self, idx):
        torch = self._torch
        if isinstance(idx, torch.Tensor):
            if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.device == self.device):
                raise ValueError("device indices must be a contiguous int32 CUDA tensor on the env's device")
            return idx.data_ptr(), idx.numel()
        return idx, None

    # ------------------------------------------------------------------ the flat actor-critic's PPO and A2C updates
    def ppo_init(self, state_dict, **hyper):
        """``ZoneVecEnv.ppo_init`` with the four arenas -- parameters, gradients, exp_avg, exp_avg_sq -- as flat float32
        CUDA tensors ALIASING device memory in ``self.ppo_arenas`` (padding between the tensors included; valid until
        the next ppo_init or ``env.close()``)."""
        self.env.ppo_init(state_dict, **hyper)
        self.ppo_arenas = self._learner_arenas("ppo")

    def ppo_publish(self, precision="auto"):
        self.env.ppo_publish(precision=precision)

    def ppo_update(self, epochs, batch_size, rng):
        return self.env.ppo_update(epochs, batch_size, rng)

    def a2c_init(self, state_dict, **hyper):
        """``ZoneVecEnv.a2c_init`` with the three arenas -- parameters, gradients, square_avg -- as flat float32 CUDA
        tensors ALIASING device memory in ``self.a2c_arenas`` (padding between the tensors included; valid until the
        next a2c_init or ``env.close()``)."""
        self.env.a2c_init(state_dict, **hyper)
        self.a2c_arenas = self._learner_arenas("a2c")

    def a2c_accumulate(self, idx, total, first):
        """``ZoneVecEnv.a2c_accumulate``; idx may be an int32 CUDA tensor (never copied, checked on the device)."""
        ptr, count = self._ppo_index_arg(idx)
        self.env.a2c_accumulate(ptr, total, first, count=count)

    def a2c_publish(self, precision="auto"):
        self.env.a2c_publish(precision=precision)

    def a2c_update(self):
        return self.env.a2c_update()

    # ------------------------------------------------------------------ DIAYN's inverse model and learned skill prior
    def diayn_init(self, inverse_state_dict, n_skills, prior_logits=None, prior=None, **hyper):
        """``ZoneVecEnv.diayn_init`` from an InverseModel state_dict (tensors on any device), with the four arenas as flat
        float32 CUDA tensors ALIASING device memory in ``self.diayn_arenas`` (valid until the next diayn_init or
        ``env.close()``)."""
        from .vec_env import inverse_tensors_from_state_dict
        if not any(k in inverse_state_dict for k in nat.SKILL_INVERSE_TENSORS):
            inverse_state_dict = inverse_tensors_from_state_dict(inverse_state_dict, n_skills)
        self.env.diayn_init(inverse_state_dict, n_skills, prior_logits=prior_logits, prior=prior, **hyper)
        self.diayn_arenas = self._learner_arenas("diayn")

    def diayn_samples(self):
        """int32 CUDA tensor [count] ALIASING the kept sample indexes of the last ``collect_skills`` (compacted on the
        device; the call waits for the count).  Valid until the next diayn_samples or collection."""
        count = self.env.diayn_samples_on_device()
        with self._torch.cuda.device(self.device):
            if not count:
                return self._torch.empty(0, dtype=self._torch.int32, device=self.device)
            return self._alias(nat.F_DIAYN_SAMPLES, (count,), np.int32)

    def diayn_update(self, epochs, batch_size, generator=None):
        """``ZoneVecEnv.diayn_update`` with the list, the permutations (``torch.randperm`` from `generator`, a CUDA
        torch.Generator or None) and the indexing on the device: nothing but the count reaches the host."""
        torch = self._torch
        kept = self.diayn_samples()
        rows = None
        for e in range(int(epochs)):
            if not kept.numel():
                break
            order = kept[torch.randperm(kept.numel(), device=self.device, generator=generator)].contiguous()
            self.diayn_epoch(order, batch_size)
            if e == 0:
                rows = self.diayn_stats().clone()         # the next epoch overwrites the buffer
        self.env._diayn_first_epoch = None if rows is None else rows.cpu().numpy()
        return self.env.diayn_logs()

    def diayn_logs(self):
        return self.env.diayn_logs()

    def diayn_prior_update(self):
        return self.env.diayn_prior_update()

    def diayn_prior_logits(self):
        return self.env.diayn_prior_logits()

    def diayn_publish(self):
        self.env.diayn_publish()

    def load_hier(self, hi_state_dict, lo_state_dict):
        """Put HighPolicyValueModel / LoPolicyValueModel state_dicts (zone-goals/src/hier_policy_value_models.py; torch
        tensors on any device) into the device agent that ``collect_hier`` runs -- after every update."""
        from .vec_env import hier_tensors_from_state_dicts
        self.env.load_hier(hier_tensors_from_state_dicts(hi_state_dict, lo_state_dict))

    def collect_hier(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """HierPolicyAlgo.collect_experiences on the device; returns (lo, hi) as CUDA tensors ALIASING the handle's
        buffers (named and shaped as ``ZoneVecEnv.collect_hier``: lo [N, T-1, ...] views of time-major memory, hi flat
        [M, ...], action_mask a bool view of uint8 memory, count [N]).  Valid until the next collect_hier.  Ends with
        one synchronisation (the host learns M)."""
        from .vec_env import hier_experience_layout
        env = self.env
        T, M = env.collect_hier_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
        lo_l, hi_l = hier_experience_layout(env.num_envs, env.num_zones, env.zone_feat, T, M)
        lo = {name: t[:T - 1].transpose(0, 1) for name, t in self._alias_layout(lo_l).items()}
        hi = self._alias_layout(hi_l, skip=not M)
        hi["action_mask"] = hi["action_mask"].view(self._torch.bool)
        hi["count"] = self._alias(nat.F_HI_COUNT)
        return lo, hi

    def load_skills(self, hi_state_dict, lo_state_dict, skill_len=200):
        """Put the skill planner's HighPolicyValueModel / LoPolicyValueModel state_dicts (main/src/
        hier_policy_value_models.py; torch tensors on any device) into the device agent that ``collect_skills`` runs --
        after every update."""
        from .vec_env import skill_tensors_from_state_dicts
        self.env.load_skills(skill_tensors_from_state_dicts(hi_state_dict, lo_state_dict), skill_len=skill_len)

    def load_xy(self, hi_state_dict, lo_state_dict, skill_len=200):
        """Put the xy-goals agent's HighPolicyValueModel / LoPolicyValueModel state_dicts (xy-goals/src/
        hier_policy_value_models.py; torch tensors on any device) into the device agent that POLICY_XY_SAMPLE /
        POLICY_XY_MEAN run."""
        from .vec_env import xy_tensors_from_state_dicts
        self.env.load_xy(xy_tensors_from_state_dicts(hi_state_dict, lo_state_dict), skill_len=skill_len)

    def collect_xy(self, frames_per_proc, policy_seed=0, env_index0=0, discount=0.99, gae_lambda=0.95):
        """collect_experiences of the xy-goals agent on the device; returns (lo, hi, num_frames) named and shaped as
        ``ZoneVecEnv.collect_xy``: lo and hi are CUDA tensors ALIASING the handle's buffers (lo [N, T, ...] views of
        time-major memory, hi flat [M, ...]), valid until the next collect; num_frames is a Python int (it waits for
        the collection)."""
        from .vec_env import xy_experience_layout, skill_num_frames
        env = self.env
        T, M = env.collect_xy_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
        L = T * env.num_envs // M
        lo_l, hi_l = xy_experience_layout(env.num_envs, env.num_zones, env.zone_feat, T, L)
        lo = {name: t.transpose(0, 1) for name, t in self._alias_layout(lo_l).items()}
        return lo, self._alias_layout(hi_l), skill_num_frames(lo["mask"].transpose(0, 1), L)

    def load_skill_inverse(self, state_dict, n_skills):
        """Put an InverseModel state_dict (main/src/inverse_model.py) into the device discriminator of the diversity
        reward -- after every update."""
        from .vec_env import inverse_tensors_from_state_dict
        self.env.load_skill_inverse(inverse_tensors_from_state_dict(state_dict, n_skills))

    def collect_skills(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95,
                       diversity_coef=0.0, skill_prior_logits=None, sample_hi=True):
        """collect_experiences of the skill planner / DIAYN on the device; returns (lo, hi, inverse, num_frames) named
        and shaped as ``ZoneVecEnv.collect_skills``: lo and hi are CUDA tensors ALIASING the handle's buffers (lo
        [N, T, ...] views of time-major memory, hi flat [M, ...]), valid until the next collect; inverse is compacted
        into new tensors and num_frames is a Python int (both wait for the collection)."""
        from .vec_env import skill_experience_layout, skill_num_frames
        env = self.env
        T, M = env.collect_skills_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda,
                                            diversity_coef, skill_prior_logits, sample_hi)
        L = T * env.num_envs // M
        lo_l, hi_l = skill_experience_layout(env.num_envs, env.num_zones, env.zone_feat, T, L)
        lo = {name: t.transpose(0, 1) for name, t in self._alias_layout(lo_l).items()}
        hi = self._alias_layout(hi_l)
        keep = lo["mask"][:, 1:] != 0
        inverse = {"obs": lo["obs"][:, 1:][keep], "zone_obs": lo["zone_obs"][:, 1:][keep],
                   "skill": lo["skill"][:, :-1][keep]}
        return lo, hi, inverse, skill_num_frames(lo["mask"].transpose(0, 1), L)

    def load_options(self, hi_state_dict, lo_state_dict):
        """Put the Options agent's HighPolicyValueModel / LoPolicyValueModel state_dicts (options/src/
        hier_policy_value_models.py; torch tensors on any device) into the device agent that ``collect_options`` runs --
        after every update.  Loading drops the transitions the last collection left open."""
        from .vec_env import option_tensors_from_state_dicts
        self.env.load_options(option_tensors_from_state_dicts(hi_state_dict, lo_state_dict))

    def collect_options(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """collect_experiences of the Options agent on the device; returns (lo, hi, termination_rate) as CUDA tensors
        ALIASING the handle's buffers, named as ``option_experience_layout``: lo [N, T-1, ...] views of time-major
        memory -- action / log_prob hold the first two components, the third is a tensor of its own (term_action /
        term_log_prob [N, T-1]; ``torch.cat`` gives the reference's three) and ended is a bool view of uint8 memory --
        hi flat [M, ...] and count [N].  termination_rate is a 0-d tensor (the mean over all T * N frames), not yet
        synchronised.  Valid until the next collect_options.  Ends with one synchronisation (the host learns M)."""
        from .vec_env import option_experience_layout
        env = self.env
        T, M = env.collect_options_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
        lo_l, hi_l = option_experience_layout(env.num_envs, env.num_zones, env.zone_feat, T, M)
        raw = self._alias_layout(lo_l)
        rate = raw["ended"].float().mean()
        raw["ended"] = raw["ended"].view(self._torch.bool)
        lo = {name: t[:T - 1].transpose(0, 1) for name, t in raw.items()}
        hi = self._alias_layout(hi_l, skip=not M)
        hi["count"] = self._alias(nat.F_HI_COUNT)
        return lo, hi, rate

    # ------------------------------------------------------------------ rendering (K18)
    def _render_marks(self, marks, count, auto):
        """marks argument -> contiguous float32 CUDA tensor [count, 2] or None; auto() builds the "auto" ones."""
        torch = self._torch
        if isinstance(marks, str):
            if marks != "auto":
                raise ValueError('marks is "auto", None or [count, 2]')
            marks = auto()
        if marks is None:
            return None
        marks = torch.as_tensor(marks, dtype=torch.float32, device=self.device).contiguous()
        if tuple(marks.shape) != (count, 2):
            raise ValueError(f"marks must have shape ({count}, 2)")
        return marks

    def _render_into(self, source, env, first, count, width, height, view, robot_radius, marks, out):
        torch = self._torch
        self.env.render_check(source, env, first, count, width, height, view, robot_radius)
        shape = (int(count), int(height), int(width), 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif not (out.is_cuda and out.device == self.device and out.dtype == torch.uint8 and out.is_contiguous()
                  and tuple(out.shape) == shape):
            raise ValueError(f"out must be a contiguous uint8 CUDA tensor of shape {shape} on the env's device")
        self.env._render(source, env, first, count, width, height, view, robot_radius,
                         None if marks is None else marks.data_ptr(), True, out.data_ptr(), True)
        return out

    def _auto_marks(self, first, count):
        """``ZoneVecEnv._auto_marks`` on the device: no copy to the host, no synchronisation."""
        torch, env = self._torch, self.env
        nan = torch.full((), float("nan"), dtype=torch.float32, device=self.device)
        if env.field_bytes(nat.F_GOAL):
            goal = self._alias(nat.F_GOAL)[first:first + count].long()
            rows = self.zone_obs[first:first + count]
            picked = rows[torch.arange(count, device=self.device), goal.clamp(min=0)]
            shown = (goal >= 0) & (picked[:, 5] != 0)
            return torch.where(shown[:, None], picked[:, :2], nan)
        if env.field_bytes(nat.F_XY_GOAL):
            goal = self._alias(nat.F_XY_GOAL)[first:first + count]
            age = self._alias(nat.F_XY_GOAL_AGE)[first:first + count]
            return torch.where((age >= 0)[:, None], goal, nan)
        return None

    def render(self, first=0, count=None, width=100, height=100, view=1.25, robot_radius=0.1, marks="auto", out=None):
        """``ZoneVecEnv.render`` into a ``torch.uint8`` CUDA tensor [count, height, width, 3] that the kernel fills in
        place (``out=`` reuses one): enqueued on the shared stream, no host copy, no synchronisation.  marks may be a
        CUDA tensor [count, 2]."""
        first = int(first)
        count = self.env.num_envs - first if count is None else int(count)
        with self._torch.cuda.device(self.device):
            self.env.render_check(nat.RENDER_CURRENT, 0, first, count, width, height, view, robot_radius)
            marks = self._render_marks(marks, count, lambda: self._auto_marks(first, count))
            return self._render_into(nat.RENDER_CURRENT, 0, first, count, width, height, view, robot_radius, marks, out)

    def render_experience(self, env, first=0, count=None, width=100, height=100, view=1.25, robot_radius=0.1,
                          marks="auto", out=None):
        """``ZoneVecEnv.render_experience`` into a ``torch.uint8`` CUDA tensor [count, height, width, 3]: the film of
        one env of the last collection, one launch on the shared stream, nothing brought to the host."""
        venv = self.env
        first, T = int(first), venv.experience_frames()
        count = max(T - first, 1) if count is None else int(count)

        def auto():
            if not (T and getattr(venv, "_exp_has_goals", False) and 0 <= first and first + count <= T
                    and 0 <= int(env) < venv.num_envs):
                return None
            return self._alias(nat.F_LO_GOAL, (T, venv.num_envs, 2), np.float32)[first:first + count, int(env)]
        with self._torch.cuda.device(self.device):
            marks = self._render_marks(marks, count, auto)
            return self._render_into(nat.RENDER_EXPERIENCE, env, first, count, width, height, view, robot_radius,
                                     marks, out)

    def step(self, actions, auto_reset=True):
        """actions: float32 CUDA tensor (N, 2) on the env's device (contiguous).  Asynchronous: the
        step kernel is enqueued behind whatever produced ``actions`` on the shared stream."""
        torch = self._torch
        if not (actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
                and tuple(actions.shape) == (self.env.num_envs, 2) and actions.device == self.device):
            raise ValueError("actions must be a contiguous float32 CUDA tensor of shape (N, 2) on the env's device")
        self.env.step_device(actions.data_ptr(), auto_reset=auto_reset)
        return {"obs": self.obs, "zone_obs": self.zone_obs}, self.reward, self.done, self.goal_met
