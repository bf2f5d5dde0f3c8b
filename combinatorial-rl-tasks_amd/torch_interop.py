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

    # ------------------------------------------------------------------ the flat actor-critic's PPO update

    def ppo_init(self, state_dict, **hyper):
        """``ZoneVecEnv.ppo_init`` with the four arenas -- parameters, gradients, exp_avg, exp_avg_sq -- as flat float32
        CUDA tensors ALIASING device memory in ``self.ppo_arenas`` (padding between the tensors included; valid until
        the next ppo_init or ``env.close()``)."""
        self.env.ppo_init(state_dict, **hyper)
        with self._torch.cuda.device(self.device):
            self.ppo_arenas = {}
            for name, which in (("param", nat.PPO_PARAM), ("grad", nat.PPO_GRAD), ("exp_avg", nat.PPO_EXP_AVG),
                                ("exp_avg_sq", nat.PPO_EXP_AVG_SQ)):
                ptr, count = self.env.ppo_tensor_ptr(which, -1)
                self.ppo_arenas[name] = self._alias_ptr(ptr, (count,))

    def ppo_views(self, which=nat.PPO_PARAM):
        """zenv_mlp_weights name -> CUDA tensor ALIASING that tensor of an arena, in its state_dict shape."""
        from .vec_env import mlp_tensor_shapes
        shapes = mlp_tensor_shapes(self.env._ppo_h, self.env.net_zone_feat)
        with self._torch.cuda.device(self.device):
            return {name: self._alias_ptr(self.env.ppo_tensor_ptr(which, i)[0], shapes[name])
                    for i, name in enumerate(self.env._ppo_keys)}

    def ppo_state_dict(self):
        """The learner's parameters under ACModel's state_dict names, as CUDA tensors ALIASING the parameter arena:
        ``model.load_state_dict(tenv.ppo_state_dict())`` copies them into a torch module on the shared stream."""
        views = self.ppo_views()
        return {key: views[name] for name, key in self.env._ppo_keys.items()}

    def ppo_load_state_dict(self, state_dict):
        """Overwrite the learner's parameters from an ACModel state_dict (tensors on any device), on the stream."""
        for key, dst in self.ppo_state_dict().items():
            dst.copy_(state_dict[key])

    def ppo_optimizer_state(self):
        """Adam's state in the shape of ``torch.optim.Adam.state_dict()`` (train_ppo.py:116-122): copies, parameter i
        the i-th of ``ACModel.parameters()``."""
        torch = self._torch
        out = self.env.ppo_optimizer_state()
        out["state"] = {i: {"step": torch.tensor(s["step"]), "exp_avg": torch.from_numpy(s["exp_avg"]).to(self.device),
                            "exp_avg_sq": torch.from_numpy(s["exp_avg_sq"]).to(self.device)}
                        for i, s in out["state"].items()}
        return out

    def ppo_load_optimizer_state(self, state):
        self.env.ppo_load_optimizer_state(state)

    def _ppo_index_arg(self, idx):
        torch = self._torch
        if isinstance(idx, torch.Tensor):
            if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.device == self.device):
                raise ValueError("device indices must be a contiguous int32 CUDA tensor on the env's device")
            return idx.data_ptr(), idx.numel()
        return idx, None

    def ppo_minibatch(self, idx, apply=False):
        """``ZoneVecEnv.ppo_minibatch``; idx may be an int32 CUDA tensor (never copied, checked on the device)."""
        ptr, count = self._ppo_index_arg(idx)
        self.env.ppo_minibatch(ptr, apply=apply, count=count)

    def ppo_apply(self):
        self.env.ppo_apply()

    def ppo_epoch(self, order, batch_size):
        """``ZoneVecEnv.ppo_epoch``; order may be an int32 CUDA tensor."""
        ptr, count = self._ppo_index_arg(order)
        self.env.ppo_epoch(ptr, batch_size, count=count)

    def ppo_stats(self):
        """float32 CUDA tensor [minibatches, 6] ALIASING the statistics of the last ppo_minibatch / ppo_epoch (not
        synchronised)."""
        rows = self.env.field_bytes(nat.F_PPO_STATS) // 24
        with self._torch.cuda.device(self.device):
            return self._alias(nat.F_PPO_STATS, (rows, 6), np.float32)

    def ppo_publish(self, precision="auto"):
        self.env.ppo_publish(precision=precision)

    def ppo_update(self, epochs, batch_size, rng):
        return self.env.ppo_update(epochs, batch_size, rng)

    # ------------------------------------------------------------------ the flat actor-critic's A2C update

    def a2c_init(self, state_dict, **hyper):
        """``ZoneVecEnv.a2c_init`` with the three arenas -- parameters, gradients, square_avg -- as flat float32 CUDA
        tensors ALIASING device memory in ``self.a2c_arenas`` (padding between the tensors included; valid until the
        next a2c_init or ``env.close()``)."""
        self.env.a2c_init(state_dict, **hyper)
        with self._torch.cuda.device(self.device):
            self.a2c_arenas = {}
            for name, which in (("param", nat.A2C_PARAM), ("grad", nat.A2C_GRAD), ("square_avg", nat.A2C_SQUARE_AVG)):
                ptr, count = self.env.a2c_tensor_ptr(which, -1)
                self.a2c_arenas[name] = self._alias_ptr(ptr, (count,))

    def a2c_views(self, which=nat.A2C_PARAM):
        """zenv_mlp_weights name -> CUDA tensor ALIASING that tensor of an arena, in its state_dict shape."""
        from .vec_env import mlp_tensor_shapes
        shapes = mlp_tensor_shapes(self.env._a2c_h, self.env.net_zone_feat)
        with self._torch.cuda.device(self.device):
            return {name: self._alias_ptr(self.env.a2c_tensor_ptr(which, i)[0], shapes[name])
                    for i, name in enumerate(self.env._a2c_keys)}

    def a2c_state_dict(self):
        """The learner's parameters under ACModel's state_dict names, as CUDA tensors ALIASING the parameter arena."""
        views = self.a2c_views()
        return {key: views[name] for name, key in self.env._a2c_keys.items()}

    def a2c_load_state_dict(self, state_dict):
        """Overwrite the learner's parameters from an ACModel state_dict (tensors on any device), on the stream."""
        for key, dst in self.a2c_state_dict().items():
            dst.copy_(state_dict[key])

    def a2c_optimizer_state(self):
        """RMSprop's state in the shape of ``torch.optim.RMSprop.state_dict()``: copies, parameter i the i-th of
        ``ACModel.parameters()``."""
        torch = self._torch
        out = self.env.a2c_optimizer_state()
        out["state"] = {i: {"step": torch.tensor(s["step"]), "square_avg": torch.from_numpy(s["square_avg"]).to(self.device)}
                        for i, s in out["state"].items()}
        return out

    def a2c_load_optimizer_state(self, state):
        self.env.a2c_load_optimizer_state(state)

    def a2c_accumulate(self, idx, total, first):
        """``ZoneVecEnv.a2c_accumulate``; idx may be an int32 CUDA tensor (never copied, checked on the device)."""
        ptr, count = self._ppo_index_arg(idx)
        self.env.a2c_accumulate(ptr, total, first, count=count)

    def a2c_apply(self):
        self.env.a2c_apply()

    def a2c_stats(self):
        """float32 CUDA tensor [1, 5] ALIASING the statistics of the last a2c_apply / a2c_update (not synchronised)."""
        rows = self.env.field_bytes(nat.F_A2C_STATS) // 20
        with self._torch.cuda.device(self.device):
            return self._alias(nat.F_A2C_STATS, (rows, 5), np.float32)

    def a2c_publish(self, precision="auto"):
        self.env.a2c_publish(precision=precision)

    def a2c_update(self):
        return self.env.a2c_update()

    # ------------------------------------------------------------------ the Zone-goals agent's two PPO updates
    def hppo_init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
        """``ZoneVecEnv.hppo_init`` with each level's four arenas as flat float32 CUDA tensors ALIASING device memory in
        ``self.hppo_arenas[level]`` (valid until the next hppo_init or ``env.close()``)."""
        self.env.hppo_init(hi_state_dict, lo_state_dict, lo=lo, hi=hi)
        with self._torch.cuda.device(self.device):
            self.hppo_arenas = {}
            for level in (nat.HPPO_LO, nat.HPPO_HI):
                self.hppo_arenas[level] = {}
                for name, which in (("param", nat.PPO_PARAM), ("grad", nat.PPO_GRAD), ("exp_avg", nat.PPO_EXP_AVG),
                                    ("exp_avg_sq", nat.PPO_EXP_AVG_SQ)):
                    ptr, count = self.env.hppo_tensor_ptr(level, which, -1)
                    self.hppo_arenas[level][name] = self._alias_ptr(ptr, (count,))

    def hppo_tensors(self, level, which=nat.PPO_PARAM):
        """zenv_hier_weights name -> CUDA tensor ALIASING that tensor of a level's arena, in its state_dict shape."""
        learner = self.env._learner(level)
        with self._torch.cuda.device(self.device):
            return {name: self._alias_ptr(learner.tensor_ptr(which, i)[0], learner.shapes[name])
                    for i, name in enumerate(learner.keys)}

    def hppo_set_tensors(self, level, tensors, which=nat.PPO_PARAM):
        """Overwrite the tensors of a level's arena that `tensors` names (tensors on any device), on the stream."""
        views = self.hppo_tensors(level, which)
        for name, src in tensors.items():
            views[name].copy_(self._torch.as_tensor(src))

    def hppo_state_dicts(self):
        """(hi_model_state, lo_model_state) as CUDA tensors ALIASING the two parameter arenas."""
        out = []
        for level in (nat.HPPO_HI, nat.HPPO_LO):
            views = self.hppo_tensors(level)
            out.append({key: views[name] for name, key in self.env._learner(level).keys.items()})
        return tuple(out)

    def hppo_load_state_dicts(self, hi_state_dict, lo_state_dict):
        for dst_sd, src_sd in zip(self.hppo_state_dicts(), (hi_state_dict, lo_state_dict)):
            for key, dst in dst_sd.items():
                dst.copy_(src_sd[key])

    def hppo_optimizer_state(self, level):
        """``ZoneVecEnv.hppo_optimizer_state`` with the moments as CUDA copies."""
        torch = self._torch
        out = self.env.hppo_optimizer_state(level)
        out["state"] = {i: {"step": torch.tensor(s["step"]), "exp_avg": torch.from_numpy(s["exp_avg"]).to(self.device),
                            "exp_avg_sq": torch.from_numpy(s["exp_avg_sq"]).to(self.device)}
                        for i, s in out["state"].items()}
        return out

    def hppo_load_optimizer_state(self, level, state):
        self.env.hppo_load_optimizer_state(level, state)

    def hppo_minibatch(self, level, idx, apply=False):
        """``ZoneVecEnv.hppo_minibatch``; idx may be an int32 CUDA tensor (never copied, checked on the device)."""
        ptr, count = self._ppo_index_arg(idx)
        self.env.hppo_minibatch(level, ptr, apply=apply, count=count)

    def hppo_apply(self, level):
        self.env.hppo_apply(level)

    def hppo_epoch(self, level, order, batch_size):
        """``ZoneVecEnv.hppo_epoch``; order may be an int32 CUDA tensor."""
        ptr, count = self._ppo_index_arg(order)
        self.env.hppo_epoch(level, ptr, batch_size, count=count)

    def hppo_stats(self, level):
        """float32 CUDA tensor [minibatches, 6] ALIASING the statistics of the level's last hppo_minibatch / hppo_epoch
        (not synchronised)."""
        field = nat.HPPO_STATS_FIELDS[level]
        rows = self.env.field_bytes(field) // 24
        with self._torch.cuda.device(self.device):
            return self._alias(field, (rows, 6), np.float32)

    def hppo_publish(self):
        self.env.hppo_publish()

    def hppo_update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        return self.env.hppo_update(epochs, batch_size, hi_epochs, hi_batch_size, rng)

    # ------------------------------------------------------------------ the xy-goals agent's two PPO updates
    def xyppo_init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
        """``ZoneVecEnv.xyppo_init`` with each level's four arenas as flat float32 CUDA tensors ALIASING device memory in
        ``self.xyppo_arenas[level]`` (valid until the next xyppo_init or ``env.close()``)."""
        self.env.xyppo_init(hi_state_dict, lo_state_dict, lo=lo, hi=hi)
        with self._torch.cuda.device(self.device):
            self.xyppo_arenas = {}
            for level in (nat.XYPPO_LO, nat.XYPPO_HI):
                self.xyppo_arenas[level] = {}
                for name, which in (("param", nat.PPO_PARAM), ("grad", nat.PPO_GRAD), ("exp_avg", nat.PPO_EXP_AVG),
                                    ("exp_avg_sq", nat.PPO_EXP_AVG_SQ)):
                    ptr, count = self.env.xyppo_tensor_ptr(level, which, -1)
                    self.xyppo_arenas[level][name] = self._alias_ptr(ptr, (count,))

    def xyppo_tensors(self, level, which=nat.PPO_PARAM):
        """zenv_xy_weights name -> CUDA tensor ALIASING that tensor of a level's arena, in its state_dict shape."""
        learner = self.env._xy_learner(level)
        with self._torch.cuda.device(self.device):
            return {name: self._alias_ptr(learner.tensor_ptr(which, i)[0], learner.shapes[name])
                    for i, name in enumerate(learner.keys)}

    def xyppo_set_tensors(self, level, tensors, which=nat.PPO_PARAM):
        """Overwrite the tensors of a level's arena that `tensors` names (tensors on any device), on the stream."""
        views = self.xyppo_tensors(level, which)
        for name, src in tensors.items():
            views[name].copy_(self._torch.as_tensor(src))

    def xyppo_state_dicts(self):
        """(hi_model_state, lo_model_state) as CUDA tensors ALIASING the two parameter arenas."""
        out = []
        for level in (nat.XYPPO_HI, nat.XYPPO_LO):
            views = self.xyppo_tensors(level)
            out.append({key: views[name] for name, key in self.env._xy_learner(level).keys.items()})
        return tuple(out)

    def xyppo_load_state_dicts(self, hi_state_dict, lo_state_dict):
        for dst_sd, src_sd in zip(self.xyppo_state_dicts(), (hi_state_dict, lo_state_dict)):
            for key, dst in dst_sd.items():
                dst.copy_(src_sd[key])

    def xyppo_optimizer_state(self, level):
        """``ZoneVecEnv.xyppo_optimizer_state`` with the moments as CUDA copies."""
        torch = self._torch
        out = self.env.xyppo_optimizer_state(level)
        out["state"] = {i: {"step": torch.tensor(s["step"]), "exp_avg": torch.from_numpy(s["exp_avg"]).to(self.device),
                            "exp_avg_sq": torch.from_numpy(s["exp_avg_sq"]).to(self.device)}
                        for i, s in out["state"].items()}
        return out

    def xyppo_load_optimizer_state(self, level, state):
        self.env.xyppo_load_optimizer_state(level, state)

    def xyppo_minibatch(self, level, idx, apply=False):
        """``ZoneVecEnv.xyppo_minibatch``; idx may be an int32 CUDA tensor (never copied, checked on the device)."""
        ptr, count = self._ppo_index_arg(idx)
        self.env.xyppo_minibatch(level, ptr, apply=apply, count=count)

    def xyppo_apply(self, level):
        self.env.xyppo_apply(level)

    def xyppo_epoch(self, level, order, batch_size):
        """``ZoneVecEnv.xyppo_epoch``; order may be an int32 CUDA tensor."""
        ptr, count = self._ppo_index_arg(order)
        self.env.xyppo_epoch(level, ptr, batch_size, count=count)

    def xyppo_stats(self, level):
        """float32 CUDA tensor [minibatches, 6] ALIASING the statistics of the level's last xyppo_minibatch / xyppo_epoch
        (not synchronised)."""
        field = nat.XYPPO_STATS_FIELDS[level]
        rows = self.env.field_bytes(field) // 24
        with self._torch.cuda.device(self.device):
            return self._alias(field, (rows, 6), np.float32)

    def xyppo_publish(self):
        self.env.xyppo_publish()

    def xyppo_update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        return self.env.xyppo_update(epochs, batch_size, hi_epochs, hi_batch_size, rng)

    # ------------------------------------------------------------------ the fixed-length-skills agent's two PPO updates
    def skppo_init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
        """``ZoneVecEnv.skppo_init`` with each level's four arenas as flat float32 CUDA tensors ALIASING device memory in
        ``self.skppo_arenas[level]`` (valid until the next skppo_init or ``env.close()``)."""
        self.env.skppo_init(hi_state_dict, lo_state_dict, lo=lo, hi=hi)
        with self._torch.cuda.device(self.device):
            self.skppo_arenas = {}
            for level in (nat.SKPPO_LO, nat.SKPPO_HI):
                self.skppo_arenas[level] = {}
                for name, which in (("param", nat.PPO_PARAM), ("grad", nat.PPO_GRAD), ("exp_avg", nat.PPO_EXP_AVG),
                                    ("exp_avg_sq", nat.PPO_EXP_AVG_SQ)):
                    ptr, count = self.env.skppo_tensor_ptr(level, which, -1)
                    self.skppo_arenas[level][name] = self._alias_ptr(ptr, (count,))

    def skppo_tensors(self, level, which=nat.PPO_PARAM):
        """zenv_skill_weights name -> CUDA tensor ALIASING that tensor of a level's arena, in its state_dict shape."""
        learner = self.env._sk_learner(level)
        with self._torch.cuda.device(self.device):
            return {name: self._alias_ptr(learner.tensor_ptr(which, i)[0], learner.shapes[name])
                    for i, name in enumerate(learner.keys)}

    def skppo_set_tensors(self, level, tensors, which=nat.PPO_PARAM):
        """Overwrite the tensors of a level's arena that `tensors` names (tensors on any device), on the stream."""
        views = self.skppo_tensors(level, which)
        for name, src in tensors.items():
            views[name].copy_(self._torch.as_tensor(src))

    def skppo_state_dicts(self):
        """(hi_model_state, lo_model_state) as CUDA tensors ALIASING the two parameter arenas."""
        out = []
        for level in (nat.SKPPO_HI, nat.SKPPO_LO):
            views = self.skppo_tensors(level)
            out.append({key: views[name] for name, key in self.env._sk_learner(level).keys.items()})
        return tuple(out)

    def skppo_load_state_dicts(self, hi_state_dict, lo_state_dict):
        for dst_sd, src_sd in zip(self.skppo_state_dicts(), (hi_state_dict, lo_state_dict)):
            for key, dst in dst_sd.items():
                dst.copy_(src_sd[key])

    def skppo_optimizer_state(self, level):
        """``ZoneVecEnv.skppo_optimizer_state`` with the moments as CUDA copies."""
        torch = self._torch
        out = self.env.skppo_optimizer_state(level)
        out["state"] = {i: {"step": torch.tensor(s["step"]), "exp_avg": torch.from_numpy(s["exp_avg"]).to(self.device),
                            "exp_avg_sq": torch.from_numpy(s["exp_avg_sq"]).to(self.device)}
                        for i, s in out["state"].items()}
        return out

    def skppo_load_optimizer_state(self, level, state):
        self.env.skppo_load_optimizer_state(level, state)

    def skppo_minibatch(self, level, idx, apply=False):
        """``ZoneVecEnv.skppo_minibatch``; idx may be an int32 CUDA tensor (never copied, checked on the device)."""
        ptr, count = self._ppo_index_arg(idx)
        self.env.skppo_minibatch(level, ptr, apply=apply, count=count)

    def skppo_apply(self, level):
        self.env.skppo_apply(level)

    def skppo_epoch(self, level, order, batch_size):
        """``ZoneVecEnv.skppo_epoch``; order may be an int32 CUDA tensor."""
        ptr, count = self._ppo_index_arg(order)
        self.env.skppo_epoch(level, ptr, batch_size, count=count)

    def skppo_stats(self, level):
        """float32 CUDA tensor [minibatches, 6] ALIASING the statistics of the level's last skppo_minibatch / skppo_epoch
        (not synchronised)."""
        field = nat.SKPPO_STATS_FIELDS[level]
        rows = self.env.field_bytes(field) // 24
        with self._torch.cuda.device(self.device):
            return self._alias(field, (rows, 6), np.float32)

    def skppo_publish(self):
        self.env.skppo_publish()

    def skppo_update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        return self.env.skppo_update(epochs, batch_size, hi_epochs, hi_batch_size, rng)

    # ------------------------------------------------------------------ DIAYN's inverse model and learned skill prior
    def diayn_init(self, inverse_state_dict, n_skills, prior_logits=None, prior=None, **hyper):
        """``ZoneVecEnv.diayn_init`` from an InverseModel state_dict (tensors on any device), with the four arenas as flat
        float32 CUDA tensors ALIASING device memory in ``self.diayn_arenas`` (valid until the next diayn_init or
        ``env.close()``)."""
        from .vec_env import inverse_tensors_from_state_dict
        if not any(k in inverse_state_dict for k in nat.SKILL_INVERSE_TENSORS):
            inverse_state_dict = inverse_tensors_from_state_dict(inverse_state_dict, n_skills)
        self.env.diayn_init(inverse_state_dict, n_skills, prior_logits=prior_logits, prior=prior, **hyper)
        with self._torch.cuda.device(self.device):
            self.diayn_arenas = {}
            for name, which in (("param", nat.PPO_PARAM), ("grad", nat.PPO_GRAD), ("exp_avg", nat.PPO_EXP_AVG),
                                ("exp_avg_sq", nat.PPO_EXP_AVG_SQ)):
                ptr, count = self.env.diayn_tensor_ptr(which, -1)
                self.diayn_arenas[name] = self._alias_ptr(ptr, (count,))

    def diayn_tensors(self, which=nat.PPO_PARAM):
        """zenv_skill_inverse_weights name -> CUDA tensor ALIASING that tensor of the arena, in its state_dict shape."""
        learner = self.env._diayn_learner()
        with self._torch.cuda.device(self.device):
            return {name: self._alias_ptr(learner.tensor_ptr(which, i)[0], learner.shapes[name])
                    for i, name in enumerate(learner.keys)}

    def diayn_set_tensors(self, tensors, which=nat.PPO_PARAM):
        views = self.diayn_tensors(which)
        for name, src in tensors.items():
            views[name].copy_(self._torch.as_tensor(src))

    def diayn_state_dict(self):
        """InverseModel's state_dict as CUDA tensors ALIASING the parameter arena."""
        views = self.diayn_tensors()
        return {key: views[name] for name, key in self.env._diayn_learner().keys.items()}

    def diayn_load_state_dict(self, state_dict):
        for key, dst in self.diayn_state_dict().items():
            dst.copy_(state_dict[key])

    def diayn_tensor_ptr(self, which, index):
        return self.env.diayn_tensor_ptr(which, index)

    def diayn_get_step(self):
        return self.env.diayn_get_step()

    def diayn_set_step(self, step):
        self.env.diayn_set_step(step)

    def diayn_optimizer_state(self):
        """``ZoneVecEnv.diayn_optimizer_state`` with the moments as CUDA copies."""
        torch = self._torch
        out = self.env.diayn_optimizer_state()
        out["state"] = {i: {"step": torch.tensor(s["step"]), "exp_avg": torch.from_numpy(s["exp_avg"]).to(self.device),
                            "exp_avg_sq": torch.from_numpy(s["exp_avg_sq"]).to(self.device)}
                        for i, s in out["state"].items()}
        return out

    def diayn_load_optimizer_state(self, state):
        self.env.diayn_load_optimizer_state(state)

    def diayn_samples(self):
        """int32 CUDA tensor [count] ALIASING the kept sample indexes of the last ``collect_skills`` (compacted on the
        device; the call waits for the count).  Valid until the next diayn_samples or collection."""
        count = self.env.diayn_samples_on_device()
        with self._torch.cuda.device(self.device):
            if not count:
                return self._torch.empty(0, dtype=self._torch.int32, device=self.device)
            return self._alias(nat.F_DIAYN_SAMPLES, (count,), np.int32)

    def diayn_minibatch(self, idx, apply=False):
        """``ZoneVecEnv.diayn_minibatch``; idx may be an int32 CUDA tensor (never copied, checked on the device)."""
        ptr, count = self._ppo_index_arg(idx)
        self.env.diayn_minibatch(ptr, apply=apply, count=count)

    def diayn_apply(self):
        self.env.diayn_apply()

    def diayn_epoch(self, order, batch_size):
        """``ZoneVecEnv.diayn_epoch``; order may be an int32 CUDA tensor."""
        ptr, count = self._ppo_index_arg(order)
        self.env.diayn_epoch(ptr, batch_size, count=count)

    def diayn_stats(self):
        """float32 CUDA tensor [minibatches, 6] ALIASING the statistics of the last diayn_minibatch / diayn_epoch (not
        synchronised)."""
        rows = self.env.field_bytes(nat.F_DIAYN_STATS) // 24
        with self._torch.cuda.device(self.device):
            return self._alias(nat.F_DIAYN_STATS, (rows, 6), np.float32)

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

    # ------------------------------------------------------------------ the Options agent's two PPO updates
    def opppo_init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
        """``ZoneVecEnv.opppo_init`` with each level's four arenas as flat float32 CUDA tensors ALIASING device memory in
        ``self.opppo_arenas[level]`` (valid until the next opppo_init or ``env.close()``)."""
        self.env.opppo_init(hi_state_dict, lo_state_dict, lo=lo, hi=hi)
        with self._torch.cuda.device(self.device):
            self.opppo_arenas = {}
            for level in (nat.OPPPO_LO, nat.OPPPO_HI):
                self.opppo_arenas[level] = {}
                for name, which in (("param", nat.PPO_PARAM), ("grad", nat.PPO_GRAD), ("exp_avg", nat.PPO_EXP_AVG),
                                    ("exp_avg_sq", nat.PPO_EXP_AVG_SQ)):
                    ptr, count = self.env.opppo_tensor_ptr(level, which, -1)
                    self.opppo_arenas[level][name] = self._alias_ptr(ptr, (count,))

    def opppo_tensors(self, level, which=nat.PPO_PARAM):
        """zenv_option_weights name -> CUDA tensor ALIASING that tensor of a level's arena, in its state_dict shape."""
        learner = self.env._op_learner(level)
        with self._torch.cuda.device(self.device):
            return {name: self._alias_ptr(learner.tensor_ptr(which, i)[0], learner.shapes[name])
                    for i, name in enumerate(learner.keys)}

    def opppo_set_tensors(self, level, tensors, which=nat.PPO_PARAM):
        """Overwrite the tensors of a level's arena that `tensors` names (tensors on any device), on the stream."""
        views = self.opppo_tensors(level, which)
        for name, src in tensors.items():
            views[name].copy_(self._torch.as_tensor(src))

    def opppo_state_dicts(self):
        """(hi_model_state, lo_model_state) as CUDA tensors ALIASING the two parameter arenas."""
        out = []
        for level in (nat.OPPPO_HI, nat.OPPPO_LO):
            views = self.opppo_tensors(level)
            out.append({key: views[name] for name, key in self.env._op_learner(level).keys.items()})
        return tuple(out)

    def opppo_load_state_dicts(self, hi_state_dict, lo_state_dict):
        for dst_sd, src_sd in zip(self.opppo_state_dicts(), (hi_state_dict, lo_state_dict)):
            for key, dst in dst_sd.items():
                dst.copy_(src_sd[key])

    def opppo_tensor_ptr(self, level, which, index):
        return self.env.opppo_tensor_ptr(level, which, index)

    def opppo_get_step(self, level):
        return self.env.opppo_get_step(level)

    def opppo_set_step(self, level, step):
        self.env.opppo_set_step(level, step)

    def opppo_optimizer_state(self, level):
        """``ZoneVecEnv.opppo_optimizer_state`` with the moments as CUDA copies."""
        torch = self._torch
        out = self.env.opppo_optimizer_state(level)
        out["state"] = {i: {"step": torch.tensor(s["step"]), "exp_avg": torch.from_numpy(s["exp_avg"]).to(self.device),
                            "exp_avg_sq": torch.from_numpy(s["exp_avg_sq"]).to(self.device)}
                        for i, s in out["state"].items()}
        return out

    def opppo_load_optimizer_state(self, level, state):
        self.env.opppo_load_optimizer_state(level, state)

    def opppo_minibatch(self, level, idx, apply=False):
        """``ZoneVecEnv.opppo_minibatch``; idx may be an int32 CUDA tensor (never copied, checked on the device)."""
        ptr, count = self._ppo_index_arg(idx)
        self.env.opppo_minibatch(level, ptr, apply=apply, count=count)

    def opppo_apply(self, level):
        self.env.opppo_apply(level)

    def opppo_epoch(self, level, order, batch_size):
        """``ZoneVecEnv.opppo_epoch``; order may be an int32 CUDA tensor."""
        ptr, count = self._ppo_index_arg(order)
        self.env.opppo_epoch(level, ptr, batch_size, count=count)

    def opppo_stats(self, level):
        """float32 CUDA tensor [minibatches, 6] ALIASING the statistics of the level's last opppo_minibatch / opppo_epoch
        (not synchronised)."""
        field = nat.OPPPO_STATS_FIELDS[level]
        rows = self.env.field_bytes(field) // 24
        with self._torch.cuda.device(self.device):
            return self._alias(field, (rows, 6), np.float32)

    def opppo_publish(self):
        self.env.opppo_publish()

    def opppo_update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        return self.env.opppo_update(epochs, batch_size, hi_epochs, hi_batch_size, rng)

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
