"""ZoneVecEnv -- the batched, device-resident surface of the zone-env hot path.

One object = N independent PointTSP / TimedTSP / ColourMatch environments stepped by one
HIP kernel launch on one MI355X.  This is the thing that replaces the reference's
``ParallelEnv`` process pool (main/src/torch_ac/torch_utils/penv.py:26-66): ``step`` takes a
(N, 2) float32 action array and returns struct-of-arrays results; finished envs are
re-reset inside the same launch and report the next episode's first observation with the
terminal reward/done, exactly like ``worker`` (penv.py:7-11).
"""
import ctypes as C
import dataclasses
import math

import numpy as np

from . import _native as nat
from ._native import Config, ZenvError, check, lib
from .agents import (_HIER_ENC, _HIER_CRITIC, HIER_HI_KEYS, HIER_LO_KEYS, SKILL_HI_KEYS, SKILL_LO_KEYS,   # noqa: F401
                     XY_HI_KEYS, XY_LO_KEYS, xy_tensor_shapes, xy_tensors_from_state_dicts,
                     INVERSE_KEYS, _lo_rows, mlp_tensors_from_state_dict, mlp_tensor_shapes, hier_tensor_shapes,
                     skill_tensor_shapes, option_tensor_shapes, inverse_tensor_shapes, hier_tensors_from_state_dicts,
                     skill_tensors_from_state_dicts, option_tensors_from_state_dicts, inverse_tensors_from_state_dict,
                     check_collect_hier_args, check_collect_skill_args, check_collect_option_args,
                     hier_experience_layout, skill_experience_layout, option_experience_layout, skill_num_frames,
                     check_collect_xy_args, xy_experience_layout, ppo_state_dict_keys, ppo_batch_indexes,
                     hppo_state_dict_keys, hppo_batch_indexes, xyppo_state_dict_keys, skppo_state_dict_keys,
                     opppo_state_dict_keys, diayn_state_dict_keys, diayn_kept_samples,
                     EPISODE_LOG_KEYS, episode_log_columns, episode_log_keys, synthesize_stats)

_FIELD_DTYPES = {
    nat.F_OBS: np.float32, nat.F_ZONE_OBS: np.float32, nat.F_REWARD: np.float32,
    nat.F_DONE: np.uint8, nat.F_GOAL_MET: np.uint8, nat.F_EP_RETURN: np.float64,
    nat.F_EP_LEN: np.int32, nat.F_LAST_RETURN: np.float64, nat.F_LAST_LEN: np.int32,
    nat.F_EPISODES: np.int32, nat.F_VISIT_COUNT: np.int32, nat.F_SEED: np.int64,
    nat.F_ACTIONS: np.float32, nat.F_POLICY_MU: np.float32, nat.F_POLICY_STD: np.float32,
    nat.F_POLICY_VALUE: np.float32, nat.F_SHAPED_REWARD: np.float64, nat.F_NEED_GOAL: np.uint8,
    nat.F_AVAILABLE_GOALS: np.uint32, nat.F_GOAL: np.int32, nat.F_ORDER_VAL: np.float32,
    nat.F_EXCEPTION: np.uint8, nat.F_POLICY_VALUE_SIGMA: np.float32, nat.F_ORDER_POS: np.int8,
    nat.F_HIER_LOGITS: np.float32, nat.F_HIER_VALUE: np.float32,
    nat.F_LO_GOAL: np.float32, nat.F_LO_ENV_REWARD: np.float32, nat.F_HI_OBS: np.float32, nat.F_HI_ZONE_OBS: np.float32,
    nat.F_HI_ACTION: np.int32, nat.F_HI_ACTION_MASK: np.uint8, nat.F_HI_VALUE: np.float32, nat.F_HI_LOG_PROB: np.float32,
    nat.F_HI_ADVANTAGE: np.float32, nat.F_HI_RETURN: np.float32, nat.F_HI_REWARD: np.float32, nat.F_HI_MASK: np.float32,
    nat.F_HI_COUNT: np.int32, nat.F_SKILL: np.int32, nat.F_SKILL_AGE: np.int32, nat.F_SKILL_LOGITS: np.float32,
    nat.F_SKILL_VALUE: np.float32, nat.F_LO_SKILL: np.int32, nat.F_LO_DIVERSITY: np.float32,
    nat.F_SKILL_BOOTSTRAP: np.int32, nat.F_OPTION_TERM_MU: np.float32, nat.F_OPTION_TERM_STD: np.float32,
    nat.F_OPTION_TERM_ACTION: np.float32, nat.F_OPTION_TERM_PROB: np.float32, nat.F_OPTION_ENDED: np.int32,
    nat.F_LO_TERM_ACTION: np.float32, nat.F_LO_TERM_LOG_PROB: np.float32, nat.F_LO_OPTION_ENDED: np.uint8,
    nat.F_XY_GOAL: np.float32, nat.F_XY_GOAL_MU: np.float32, nat.F_XY_GOAL_STD: np.float32, nat.F_XY_VALUE: np.float32,
    nat.F_XY_GOAL_AGE: np.int32, nat.F_HI_GOAL: np.float32, nat.F_LO_GOAL_DIST: np.float32,
    nat.F_XY_BOOTSTRAP_GOAL: np.float32, nat.F_PPO_STATS: np.float32,
    nat.F_HPPO_LO_STATS: np.float32, nat.F_HPPO_HI_STATS: np.float32,
    nat.F_XYPPO_LO_STATS: np.float32, nat.F_XYPPO_HI_STATS: np.float32,
    nat.F_SKPPO_LO_STATS: np.float32, nat.F_SKPPO_HI_STATS: np.float32,
    nat.F_OPPPO_LO_STATS: np.float32, nat.F_OPPPO_HI_STATS: np.float32,
    nat.F_DIAYN_STATS: np.float32, nat.F_DIAYN_SAMPLES: np.int32, nat.F_ORDER_ROWS: np.float32,
    nat.F_A2C_STATS: np.float32,
}


def _as_host_f32(v):
    """A torch tensor (any device) or anything numpy takes -> numpy float32."""
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32)


@dataclasses.dataclass(frozen=True)
class _LearnerFamily:
    """What the methods <key>_* of one learner family differ in.  The C functions are zenv_<key>_*; a family with
    levels is a pair of learners (level 0 the low one, 1 the high one) whose C functions take the level."""
    key: str
    stats_fields: tuple                 # the statistics field by level (one entry without levels)
    docs: dict                          # forwarder -> its docstring, for those that have one
    levels: bool = False
    stats_cols: int = 6
    rmsprop: bool = False               # the optimiser state is RMSprop's (square_avg), not Adam's
    # a pair's init (_pair_init) and publish (_pair_publish)
    weights: type = None                # the struct of zenv_<key>_init
    skills: bool = False                # its weights carry n_skills
    tensors_from: object = None         # (hi_state_dict, lo_state_dict) -> the struct's tensors by name
    keys: object = None                 # () -> (hi, lo) dicts: tensor name -> state_dict key, in arena order
    shapes: object = None               # (h, [S,] F) -> tensor name -> shape
    defaults: tuple = ()                # the names of ZoneVecEnv's default settings, (low, high)
    loader: str = None                  # the ZoneVecEnv method that hands tensors to the acting agent
    loader_skill_len: bool = False      # ... and takes the handle's current skill_len
    # a pair's update (_pair_update)
    lo_drops_last: bool = False         # the low level trains on frames 0 .. T-2 of every env, not on all T
    m_from: tuple = ()                  # (field, bytes per row): where the number of high-level rows M is read from
    needs_rows: bool = False            # M = 0 is an error; else the high level is skipped and its logs are zeros
    no_experience: str = ""             # the ZENV_E_STATE message when the handle holds none of the agent's records

    @property
    def prefix(self):
        return f"zenv_{self.key}_"


class _Learner:
    """One device learner behind the <key>_* methods of a family: the arenas' tensors under their names, the optimiser's
    state (Adam's; RMSprop's for a2c_*), the update calls and the statistics.  keys empty: a learner not created through
    this object -- every call of it goes to the library, which answers ZENV_E_STATE (ZENV_E_ARG for a level that does
    not exist)."""

    def __init__(self, handle, family, level, keys=None, shapes=None, lr=0.0, adam_eps=0.0, rmsprop_alpha=None):
        self._h, self.family, self.level, self.keys, self.shapes = handle, family, level, keys or {}, shapes or {}
        self.lr, self.adam_eps, self.rmsprop_alpha = lr, adam_eps, rmsprop_alpha
        self.stats_field = family.stats_fields[level if family.levels and level in (0, 1) else 0]

    def _call(self, name, *args):
        level = (int(self.level),) if self.family.levels else ()
        check(getattr(lib(), self.family.prefix + name)(self._h, *level, *args))

    def tensor_ptr(self, which, index):
        p, n = C.c_void_p(), C.c_int64()
        self._call("tensor", int(which), int(index), C.byref(p), C.byref(n))
        return p.value, n.value

    def _need_init(self):
        """Before the learner's init there are no names to walk: let the library refuse."""
        if not self.keys:
            self.tensor_ptr(nat.PPO_PARAM, -1)
            raise ZenvError(nat.E_STATE, "the learner was not created through this object: call its init here")

    def tensors(self, which=nat.PPO_PARAM):
        self._need_init()
        out = {}
        for i, name in enumerate(self.keys):
            out[name] = a = np.empty(self.shapes[name], np.float32)
            self._call("read", int(which), i, a.ctypes.data)
        return out

    def set_tensors(self, tensors, which=nat.PPO_PARAM):
        self._need_init()
        for i, name in enumerate(self.keys):
            if name in tensors:
                a = np.ascontiguousarray(tensors[name], np.float32)
                if a.shape != self.shapes[name]:
                    raise ValueError(f"{name}: shape {a.shape}, expected {self.shapes[name]}")
                self._call("write", int(which), i, a.ctypes.data)

    def state_dict(self):
        t = self.tensors()
        return {key: t[name] for name, key in self.keys.items()}

    def load_state_dict(self, state_dict):
        self.set_tensors({name: _as_host_f32(state_dict[key]) for name, key in self.keys.items()})

    def optimizer_state(self):
        if self.family.rmsprop:
            return self._rmsprop_state()
        m, v = self.tensors(nat.PPO_EXP_AVG), self.tensors(nat.PPO_EXP_AVG_SQ)
        step = self.get_step()
        state = {i: {"step": float(step), "exp_avg": m[name], "exp_avg_sq": v[name]}
                 for i, name in enumerate(self.keys)} if step else {}
        group = {"lr": self.lr, "betas": (0.9, 0.999), "eps": self.adam_eps, "weight_decay": 0,
                 "amsgrad": False, "params": list(range(len(self.keys)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state(self, state):
        if self.family.rmsprop:
            return self._load_rmsprop_state(state)
        names = list(self.keys)
        st = state["state"]
        zeros = {n: np.zeros(self.shapes[n], np.float32) for n in names}
        self.set_tensors({n: _as_host_f32(st[i]["exp_avg"]) for i, n in enumerate(names)} if st else zeros,
                         nat.PPO_EXP_AVG)
        self.set_tensors({n: _as_host_f32(st[i]["exp_avg_sq"]) for i, n in enumerate(names)} if st else zeros,
                         nat.PPO_EXP_AVG_SQ)
        self.set_step(int(float(st[0]["step"])) if st else 0)

    def _rmsprop_state(self):
        """``torch.optim.RMSprop.state_dict()``'s shape (momentum 0, not centered): ``step`` and ``square_avg``."""
        v = self.tensors(nat.A2C_SQUARE_AVG)
        step = self.get_step()
        state = {i: {"step": float(step), "square_avg": v[name]} for i, name in enumerate(self.keys)} if step else {}
        group = {"lr": self.lr, "momentum": 0, "alpha": self.rmsprop_alpha, "eps": self.adam_eps, "centered": False,
                 "weight_decay": 0, "params": list(range(len(self.keys)))}
        return {"state": state, "param_groups": [group]}

    def _load_rmsprop_state(self, state):
        names = list(self.keys)
        st = state["state"]
        zeros = {n: np.zeros(self.shapes[n], np.float32) for n in names}
        self.set_tensors({n: _as_host_f32(st[i]["square_avg"]) for i, n in enumerate(names)} if st else zeros,
                         nat.A2C_SQUARE_AVG)
        self.set_step(int(float(st[0]["step"])) if st else 0)

    def accumulate(self, idx, total, first, count=None):
        ptr, n, dev, keep = self._indices(idx, count)
        self._call("accumulate", C.c_void_p(ptr), n, dev, int(total), int(bool(first)))

    def update(self):
        self._call("update")

    def get_step(self):
        n = C.c_int64()
        self._call("get_step", C.byref(n))
        return n.value

    def set_step(self, step):
        self._call("set_step", int(step))

    @staticmethod
    def _indices(idx, count):
        """(address, count, on_device, the array to keep alive) of a host int32 array or a device address."""
        if isinstance(idx, (int, np.integer)):
            return int(idx), int(count), 1, None
        a = np.ascontiguousarray(idx, np.int32).reshape(-1)
        return a.ctypes.data, a.size, 0, a

    def minibatch(self, idx, apply=False, count=None):
        ptr, n, dev, keep = self._indices(idx, count)
        self._call("minibatch", C.c_void_p(ptr), n, dev, int(bool(apply)))

    def apply(self):
        self._call("apply")

    def epoch(self, order, batch_size, count=None):
        ptr, n, dev, keep = self._indices(order, count)
        self._call("epoch", C.c_void_p(ptr), n, int(batch_size), dev)

    def stats(self):
        cols = self.family.stats_cols
        rows = lib().zenv_field_bytes(self._h, self.stats_field) // (4 * cols)
        out = np.empty((rows, cols), np.float32)
        if rows:
            check(lib().zenv_get(self._h, self.stats_field, out.ctypes.data, 0))
        return out


def _pair_docs(key, weights, minibatch):
    """The docstrings of a pair's forwarders; minibatch: the family's own, the index order of its two levels."""
    return {
        "tensor_ptr": "``ppo_tensor_ptr`` of a level's arenas.",
        "tensors": f"Every tensor of a level's arena as a new host array, under its {weights} name (hi_* / lo_*).",
        "state_dicts": "(hi_model_state, lo_model_state): both learners' parameters under the reference's names (host "
                       "copies).",
        "optimizer_state": "A level's Adam state in the shape of ``torch.optim.Adam.state_dict()``: parameter i is the "
                           "i-th of the\n        module's ``parameters()``.",
        "minibatch": minibatch,
        "stats": f"float32 [minibatches, 6] of the level's last {key}_minibatch / {key}_epoch (``_native.PPO_STATS``' "
                 "columns,\n        value_std = 0).  Waits for the device.",
    }


_FLAT_DOCS = {
    "tensors": "Every tensor of an arena as a new host array, under its zenv_mlp_weights name.",
    "set_tensors": "Overwrite the tensors of an arena that `tensors` names (zenv_mlp_weights names).",
    "state_dict": "The learner's parameters under the reference ACModel's state_dict names (host float32 copies).",
    "load_state_dict": "Overwrite the learner's parameters from an ACModel state_dict (every key must be there).",
}

_FAMILIES = {f.key: f for f in (
    _LearnerFamily(
        "ppo", (nat.F_PPO_STATS,), dict(
            _FLAT_DOCS,
            tensor_ptr="(device pointer, element count) of tensor `index` (arena order; -1: the whole arena) of arena "
                       "`which`\n        (``_native.PPO_PARAM`` / ``PPO_GRAD`` / ``PPO_EXP_AVG`` / ``PPO_EXP_AVG_SQ``).",
            optimizer_state="Adam's state in the shape of ``torch.optim.Adam.state_dict()`` (train_ppo.py:116-122), host "
                            "arrays: parameter\n        i is the i-th of ``ACModel.parameters()``.",
            load_optimizer_state="Restore Adam's moments and step count from ``ppo_optimizer_state`` / "
                                 "``torch.optim.Adam.state_dict()``.",
            minibatch="Forward, loss and backward on the samples idx (host int32 array, or a device address with count): "
                      "the\n        gradients stay in their arena, the statistics in ``ppo_stats()[0]``; apply: the clip "
                      "and Adam step too.\n        Index i is env i // T, frame i % T of the last collect.  Asynchronous.",
            apply="clip_grad_norm_ and one Adam step on whatever the gradient arena holds.",
            epoch="The minibatches order[k * batch_size : (k + 1) * batch_size] in sequence (the last one short), each "
                  "with\n        its clip and Adam step; no host synchronisation.  ``ppo_stats()`` has a row per minibatch.",
            stats="float32 [minibatches, 6] of the last ppo_minibatch / ppo_epoch: ``_native.PPO_STATS`` names the "
                  "columns\n        (ppo.py:93-100, :121).  Waits for the device.")),
    _LearnerFamily(
        "a2c", (nat.F_A2C_STATS,), dict(
            _FLAT_DOCS,
            tensor_ptr="(device pointer, element count) of tensor `index` (arena order; -1: the whole arena) of arena "
                       "`which`\n        (``_native.A2C_PARAM`` / ``A2C_GRAD`` / ``A2C_SQUARE_AVG``).",
            optimizer_state="RMSprop's state in the shape of ``torch.optim.RMSprop.state_dict()`` (``step``, "
                            "``square_avg``), host arrays:\n        parameter i is the i-th of ``ACModel.parameters()``.",
            load_optimizer_state="Restore square_avg and the step count from ``a2c_optimizer_state`` / "
                                 "``torch.optim.RMSprop.state_dict()``:\n        the ``optimizer_state`` of an A2C run's "
                                 "status.pt resumes here.",
            apply="The gradient norm, clip_grad_norm_ and one RMSprop step on whatever the gradient arena holds; the "
                  "five\n        statistics of the accumulated frames go to ``a2c_stats()``.",
            stats="float32 [1, 5] of the last a2c_apply / a2c_update ([0, 5] before the first): ``_native.A2C_STATS`` "
                  "names the\n        columns.  Waits for the device."),
        stats_cols=len(nat.A2C_STATS), rmsprop=True),
    _LearnerFamily(
        "hppo", nat.HPPO_STATS_FIELDS, _pair_docs(
            "hppo", "zenv_hier_weights",
            "``ppo_minibatch`` on the records of the last ``collect_hier``.  Low level: index i is env i // (T-1), frame"
            "\n        i % (T-1) (lo_exps' order); high level: row i of the M closed transitions."),
        levels=True, weights=nat.HierWeights, tensors_from=hier_tensors_from_state_dicts, keys=hppo_state_dict_keys,
        shapes=hier_tensor_shapes, defaults=("HPPO_LO", "HPPO_HI"), loader="load_hier", lo_drops_last=True,
        m_from=(nat.F_HI_VALUE, 4), no_experience="collect_hier first: the handle holds no experience"),
    _LearnerFamily(
        "xyppo", nat.XYPPO_STATS_FIELDS, _pair_docs(
            "xyppo", "zenv_xy_weights",
            "``ppo_minibatch`` on the records of the last ``collect_xy``.  Low level: index i is env i // T, frame i % T"
            "\n        (lo_exps' order, every frame); high level: row i of the M = N T / skill_len windows."),
        levels=True, weights=nat.XyWeights, tensors_from=xy_tensors_from_state_dicts, keys=xyppo_state_dict_keys,
        shapes=xy_tensor_shapes, defaults=("XYPPO_LO", "XYPPO_HI"), loader="load_xy", loader_skill_len=True,
        m_from=(nat.F_HI_GOAL, 8), needs_rows=True,
        no_experience="collect_xy first: the handle holds no experience of the xy-goals agent"),
    _LearnerFamily(
        "skppo", nat.SKPPO_STATS_FIELDS, _pair_docs(
            "skppo", "zenv_skill_weights",
            "``ppo_minibatch`` on the records of the last ``collect_skills``.  Low level: index i is env i // T, frame "
            "i % T\n        (lo_exps' order, every frame); high level: row i of the M = N T / skill_len windows."),
        levels=True, weights=nat.SkillWeights, skills=True, tensors_from=skill_tensors_from_state_dicts,
        keys=skppo_state_dict_keys, shapes=skill_tensor_shapes, defaults=("SKPPO_LO", "SKPPO_HI"), loader="load_skills",
        loader_skill_len=True, m_from=(nat.F_HI_ACTION, 4), needs_rows=True,
        no_experience="collect_skills first: the handle holds no experience of the fixed-length-skills agent"),
    _LearnerFamily(
        "opppo", nat.OPPPO_STATS_FIELDS, _pair_docs(
            "opppo", "zenv_option_weights",
            "``ppo_minibatch`` on the records of the last ``collect_options``.  Low level: index i is env i // (T - 1), "
            "frame\n        i % (T - 1) (lo_exps' order; frame T - 1 is never read); high level: row i of the M closed "
            "transitions (M >= 1)."),
        levels=True, weights=nat.OptionWeights, skills=True, tensors_from=option_tensors_from_state_dicts,
        keys=opppo_state_dict_keys, shapes=option_tensor_shapes, defaults=("OPPPO_LO", "OPPPO_HI"), loader="load_options",
        lo_drops_last=True, m_from=(nat.F_HI_ACTION, 4),
        no_experience="collect_options first: the handle holds no experience of the Options agent"),
    _LearnerFamily(
        "diayn", (nat.F_DIAYN_STATS,), {
            "tensor_ptr": "``ppo_tensor_ptr`` of the inverse model's arenas.",
            "tensors": "Every tensor of the arena as a new host array, under its zenv_skill_inverse_weights name.",
            "state_dict": "The learner's parameters under InverseModel's names (host copies).",
            "optimizer_state": "Adam's state in the shape of ``torch.optim.Adam.state_dict()``: parameter i is the i-th "
                               "of ``parameters()``.",
            "minibatch": "``ppo_minibatch`` of the inverse model on the sample indexes idx (entries of "
                         "``diayn_samples()``).",
            "stats": "float32 [minibatches, 6] of the last diayn_minibatch / diayn_epoch: column 0 the cross-entropy "
                     "loss, column\n        5 the gradient norm, columns 1-4 zero.  Waits for the device."}),
)}


def _forwarders(fam):
    """call -> the method <key>_<call> of ZoneVecEnv for the thin forwarders of a family: each finds the learner and
    hands its arguments on.  A pair's take the level first and have state_dicts / load_state_dicts for both levels."""
    key = fam.key
    if fam.levels:
        def tensor_ptr(self, level, which, index):
            return self._learner_of(key, level).tensor_ptr(which, index)

        def tensors(self, level, which=nat.PPO_PARAM):
            return self._learner_of(key, level).tensors(which)

        def set_tensors(self, level, tensors, which=nat.PPO_PARAM):
            self._learner_of(key, level).set_tensors(tensors, which)

        def state_dicts(self):
            return self._learner_of(key, 1).state_dict(), self._learner_of(key, 0).state_dict()

        def load_state_dicts(self, hi_state_dict, lo_state_dict):
            self._learner_of(key, 1).load_state_dict(hi_state_dict)
            self._learner_of(key, 0).load_state_dict(lo_state_dict)

        def optimizer_state(self, level):
            return self._learner_of(key, level).optimizer_state()

        def load_optimizer_state(self, level, state):
            self._learner_of(key, level).load_optimizer_state(state)

        def get_step(self, level):
            return self._learner_of(key, level).get_step()

        def set_step(self, level, step):
            self._learner_of(key, level).set_step(step)

        def minibatch(self, level, idx, apply=False, count=None):
            self._learner_of(key, level).minibatch(idx, apply, count)

        def apply(self, level):
            self._learner_of(key, level).apply()

        def epoch(self, level, order, batch_size, count=None):
            self._learner_of(key, level).epoch(order, batch_size, count)

        def stats(self, level):
            return self._learner_of(key, level).stats()

        return dict(tensor_ptr=tensor_ptr, tensors=tensors, set_tensors=set_tensors, state_dicts=state_dicts,
                    load_state_dicts=load_state_dicts, optimizer_state=optimizer_state,
                    load_optimizer_state=load_optimizer_state, get_step=get_step, set_step=set_step, minibatch=minibatch,
                    apply=apply, epoch=epoch, stats=stats)

    def tensor_ptr(self, which, index):
        return self._learner_of(key).tensor_ptr(which, index)

    def tensors(self, which=nat.PPO_PARAM):
        return self._learner_of(key).tensors(which)

    def set_tensors(self, tensors, which=nat.PPO_PARAM):
        self._learner_of(key).set_tensors(tensors, which)

    def state_dict(self):
        return self._learner_of(key).state_dict()

    def load_state_dict(self, state_dict):
        self._learner_of(key).load_state_dict(state_dict)

    def optimizer_state(self):
        return self._learner_of(key).optimizer_state()

    def load_optimizer_state(self, state):
        self._learner_of(key).load_optimizer_state(state)

    def get_step(self):
        return self._learner_of(key).get_step()

    def set_step(self, step):
        self._learner_of(key).set_step(step)

    def minibatch(self, idx, apply=False, count=None):
        self._learner_of(key).minibatch(idx, apply, count)

    def apply(self):
        self._learner_of(key).apply()

    def epoch(self, order, batch_size, count=None):
        self._learner_of(key).epoch(order, batch_size, count)

    def stats(self):
        return self._learner_of(key).stats()

    out = dict(tensor_ptr=tensor_ptr, tensors=tensors, set_tensors=set_tensors, state_dict=state_dict,
               load_state_dict=load_state_dict, optimizer_state=optimizer_state,
               load_optimizer_state=load_optimizer_state, get_step=get_step, set_step=set_step, apply=apply, stats=stats)
    if not fam.rmsprop:         # the A2C learner has accumulate / update instead (ZoneVecEnv.a2c_accumulate, a2c_update)
        out.update(minibatch=minibatch, epoch=epoch)
    return out


def _install_forwarders(cls):
    for fam in _FAMILIES.values():
        for call, f in _forwarders(fam).items():
            f.__name__ = f"{fam.key}_{call}"
            f.__qualname__ = f"{cls.__name__}.{f.__name__}"
            f.__doc__ = fam.docs.get(call)
            setattr(cls, f.__name__, f)
    return cls


def ppo_logs(stats, distributional):
    """The logs dict of update_parameters (ppo.py:137-153) from the [minibatches, 6] statistics of an epoch."""
    mean = np.asarray(stats, np.float64).mean(axis=0)
    return {name: float(mean[i]) for i, name in enumerate(nat.PPO_STATS) if distributional or name != "value_std"}


def a2c_logs(stats):
    """The logs dict of A2CAlgo.update_parameters (a2c.py:85-91) from the [1, 5] statistics of an update."""
    row = np.asarray(stats, np.float64).reshape(-1, len(nat.A2C_STATS))[0]
    return {name: float(row[i]) for i, name in enumerate(nat.A2C_STATS)}


def config_for_id(env_id, **overrides):
    """Config of a registry id (envs/__init__.py:88-141); unknown id -> RuntimeError."""
    cfg = Config()
    rc = lib().zenv_config_for_id(env_id.encode(), C.byref(cfg))
    if rc != 0:
        raise RuntimeError("Unknown environment")   # make_env.py:18,34,51
    return apply_overrides(cfg, overrides)


def default_config(task, num_zones, **overrides):
    cfg = Config()
    check(lib().zenv_default_config(int(task), int(num_zones), C.byref(cfg)))
    return apply_overrides(cfg, overrides)


def apply_overrides(cfg, overrides):
    for k, v in overrides.items():
        if k == "damping":
            for i in range(3):
                cfg.damping[i] = float(v[i])
        elif k == "robot_locations":              # Engine 'robot_locations': [] or [(x, y)]
            cfg.n_robot_locations = len(v)
            for i, c in enumerate(v[:1]):
                cfg.robot_location[0], cfg.robot_location[1] = float(c[0]), float(c[1])
            if len(v) > 1:
                raise ValueError("at most one robot location")
        elif k == "zones_locations":              # Engine 'zones_locations': the first len(v) zones are fixed
            if len(v) > nat.MAX_ZONES:
                raise ValueError("too many zones_locations")
            cfg.n_zones_locations = len(v)
            for i, c in enumerate(v):
                cfg.zones_locations[i][0], cfg.zones_locations[i][1] = float(c[0]), float(c[1])
        elif k == "robot_rot":                    # Engine 'robot_rot': None = random
            cfg.robot_rot_fixed = 0 if v is None else 1
            cfg.robot_rot = 0.0 if v is None else float(v)
        elif not hasattr(cfg, k):
            raise KeyError(f"unknown config key {k!r}")
        else:
            setattr(cfg, k, v)
    return cfg


def zone_feat(cfg):
    return lib().zenv_zone_feat(C.byref(cfg))


def comm_unique_id():
    """rank 0 of a sharded job: the RCCL unique id (128 bytes) every rank passes to ZoneVecEnv.comm_init."""
    buf = (C.c_char * nat.COMM_ID_BYTES)()
    check(lib().zenv_comm_unique_id(buf))
    return bytes(buf.raw)


def probe_store_stream(n_tiles, tile_bytes, steps=64, cache_policy=0, reps=3, device=0):
    """us per step of a bare write-only row stream of the step kernels' shape (zenv_probe_store_stream)."""
    us = C.c_float(0)
    check(lib().zenv_probe_store_stream(int(device), int(n_tiles), int(tile_bytes), int(steps), int(cache_policy),
                                        int(reps), C.byref(us)))
    return us.value


def sample_layout(cfg, seed):
    """Host half of reset() for ``env.seed(seed); env.reset()``.

    Returns (robot_xyrot[3], zone_xy[Z,2], aux[Z], restarts)."""
    Z = cfg.num_zones
    robot = np.zeros(3, np.float64)
    zones = np.zeros((Z, 2), np.float64)
    aux = np.zeros(Z, np.int32)
    restarts = C.c_int32(0)
    check(lib().zenv_sample_layout(C.byref(cfg), int(seed), robot.ctypes.data, zones.ctypes.data,
                                   aux.ctypes.data, C.byref(restarts)))
    return robot, zones, aux, restarts.value


def sample_layout_shared(cfg, seed):
    """``sample_layout`` through the source the device sampler is compiled from (zenv_sample_layout_shared): the same
    results, bit for bit, without a GPU.  TSP and ColourMatch configs."""
    Z = cfg.num_zones
    robot = np.zeros(3, np.float64)
    zones = np.zeros((Z, 2), np.float64)
    aux = np.zeros(Z, np.int32)
    restarts = C.c_int32(0)
    check(lib().zenv_sample_layout_shared(C.byref(cfg), int(seed), robot.ctypes.data, zones.ctypes.data,
                                          aux.ctypes.data, C.byref(restarts)))
    return robot, zones, aux, restarts.value


def sample_layout_timed(cfg, seed):
    """``sample_layout`` of a TimedTSP config through the shared sampler (zenv_sample_layout_timed): the layout the
    device samples once ``ZoneVecEnv.timed_layouts_device()`` is on, bit for bit, without a GPU.  The deadlines go through
    the shared ``det_log`` instead of libm's ``log``: numpy's deadlines wherever ``beta * num_steps`` is not within a few
    ulps of an integer."""
    Z = cfg.num_zones
    robot = np.zeros(3, np.float64)
    zones = np.zeros((Z, 2), np.float64)
    aux = np.zeros(Z, np.int32)
    restarts = C.c_int32(0)
    check(lib().zenv_sample_layout_timed(C.byref(cfg), int(seed), robot.ctypes.data, zones.ctypes.data,
                                         aux.ctypes.data, C.byref(restarts)))
    return robot, zones, aux, restarts.value


_DET_OPS = {"log": nat.DET_OP_LOG, "div": nat.DET_OP_DIV, "sqrt": nat.DET_OP_SQRT}


def det_ops(op, a, b=None, on_device=False):
    """Elementwise ``det_log(a)`` / ``det_div(a, b)`` / ``det_sqrt(a)`` of csrc/det_log.hpp (zenv_det_ops; op "log",
    "div", "sqrt" or a DET_OP_* code), as the host compiles them or, with on_device, as gfx950 does (needs a GPU).
    A test hook: the two must agree bit for bit."""
    code = _DET_OPS.get(op, op)
    x = np.ascontiguousarray(a, np.float64).reshape(-1)
    y = None
    if code == nat.DET_OP_DIV:
        if b is None:
            raise ValueError("det_ops('div') takes two operands")
        y = np.ascontiguousarray(np.broadcast_to(np.asarray(b, np.float64).reshape(-1), x.shape))
    out = np.empty_like(x)
    check(lib().zenv_det_ops(int(code), x.ctypes.data, None if y is None else y.ctypes.data, out.ctypes.data, x.size,
                             int(bool(on_device))))
    return out.reshape(np.shape(a))


def layout_thresholds(cfg):
    """The keepout test's two right-hand sides A (a zone against the robot, a zone against a zone) and for each the
    threshold T with ``sqrt(s) < A  <=>  s < T`` that the shared sampler compares d^2 with (zenv_layout_thresholds).

    Returns (rhs[2], thr[2])."""
    rhs = np.zeros(2, np.float64)
    thr = np.zeros(2, np.float64)
    check(lib().zenv_layout_thresholds(C.byref(cfg), rhs.ctypes.data, thr.ctypes.data))
    return rhs, thr


def route_ranks(robot_xy, zone_xy):
    """The built-in visiting order of a layout (TSPOrderEnv without OR-tools): rank[z] = position of zone z in a
    tour: TSP_Solver.get_optim_route's problem (closed tour from the robot, int64(10 x distance) arcs,
    PATH_CHEAPEST_ARC + local search) solved without OR-tools."""
    r = np.ascontiguousarray(robot_xy, np.float64)[:2].copy()
    z = np.ascontiguousarray(zone_xy, np.float64)
    rank = np.zeros(z.shape[0], np.int32)
    check(lib().zenv_route_ranks(r.ctypes.data, z.ctypes.data, z.shape[0], rank.ctypes.data))
    return rank


def route_ranks_shared(robot_xy, zone_xy, moves=False):
    """``route_ranks`` through the source the device solver is compiled from (zenv_route_ranks_shared): the same
    ranks, element for element, without a GPU.  moves=True: returns (rank, moves[5]) -- the accepted moves per operator
    (or-opt of chains 1, 2, 3, exchange, 2-opt).  ZenvError(E_ARG) for a non-finite coordinate or one beyond +-1e9."""
    r = np.ascontiguousarray(robot_xy, np.float64).reshape(-1)[:2].copy()
    z = np.ascontiguousarray(zone_xy, np.float64).reshape(-1, 2)
    rank = np.zeros(z.shape[0], np.int32)
    mv = np.zeros(5, np.int32)
    check(lib().zenv_route_ranks_shared(r.ctypes.data, z.ctypes.data, z.shape[0], rank.ctypes.data,
                                        mv.ctypes.data if moves else None))
    return (rank, mv) if moves else rank


def fixed_seed_sequence(rng_seed, min_seed, max_seed, count):
    """Seeds FixedSeedsWrapper.reset (wrappers.py:20-23) would draw, without numpy's Generator."""
    out = np.zeros(count, np.int64)
    check(lib().zenv_fixed_seed_sequence(int(rng_seed), int(min_seed), int(max_seed), int(count),
                                         out.ctypes.data))
    return out


@_install_forwarders
class ZoneVecEnv:
    """N device-resident zone envs.

    Parameters
    ----------
    cfg : Config or registry id (str)
    num_envs : N
    device : HIP device ordinal
    """

    def __init__(self, cfg, num_envs, device=0, **overrides):
        if isinstance(cfg, str):
            cfg = config_for_id(cfg, **overrides)
        elif overrides:
            cfg = apply_overrides(cfg.copy(), overrides)
        self.cfg = cfg
        self.num_envs = int(num_envs)
        self.num_zones = cfg.num_zones
        self.zone_feat = zone_feat(cfg)
        self.device = int(device)
        self._h = C.c_void_p()
        self._learners = {}         # (family key, level or None) -> _Learner, of the learners created through this object
        check(lib().zenv_create(C.byref(cfg), self.num_envs, self.device, C.byref(self._h)))

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().zenv_destroy(self._h)
            self._h = C.c_void_p()
            # the handle's own page-locked images (copy=False views of step_results() die with the env)
            ptrs = [a.ctypes.data for a in getattr(self, "_own_pinned", [])]
            self._own_pinned, self._slab, self._slab_views, self._goal_host = [], None, None, None
            self._host_actions, self._host_io = None, False      # (zenv_host_io's buffers went with the handle)
            for ptr in ptrs:
                lib().zenv_host_free(C.c_void_p(ptr))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ bank / schedule
    def build_bank(self, seed_first, count, n_threads=8):
        check(lib().zenv_bank_build(self._h, int(seed_first), int(count), int(n_threads)))

    def build_bank_seeds(self, seeds, n_threads=8):
        s = np.ascontiguousarray(seeds, np.int64).reshape(-1)
        check(lib().zenv_bank_build_seeds(self._h, s.ctypes.data, s.size, int(n_threads)))

    def set_bank(self, robot_xyrot, zone_xy, aux=None, seeds=None):
        robot = np.ascontiguousarray(robot_xyrot, np.float64).reshape(-1, 3)
        S = robot.shape[0]
        zones = np.ascontiguousarray(zone_xy, np.float64).reshape(S, self.num_zones, 2)
        aux_a = None if aux is None else np.ascontiguousarray(aux, np.int32).reshape(S, self.num_zones)
        seeds_a = None if seeds is None else np.ascontiguousarray(seeds, np.int64).reshape(S)
        check(lib().zenv_bank_set(self._h, robot.ctypes.data, zones.ctypes.data,
                                  None if aux_a is None else aux_a.ctypes.data,
                                  None if seeds_a is None else seeds_a.ctypes.data, S))

    @property
    def bank_size(self):
        return lib().zenv_bank_size(self._h)

    def schedule_sequential(self, first=None, stride=0):
        f = None if first is None else np.ascontiguousarray(first, np.int32)
        if f is not None and f.shape != (self.num_envs,):
            raise ValueError("first must have shape (num_envs,)")
        check(lib().zenv_schedule_sequential(self._h, None if f is None else f.ctypes.data, int(stride)))

    def schedule_ring(self, first, depth):
        """Env i walks round the slots first[i] .. first[i] + depth - 1 (zenv_schedule_ring); ``update_bank`` keeps
        the ring ahead of it."""
        f = np.ascontiguousarray(first, np.int32)
        if f.shape != (self.num_envs,):
            raise ValueError("first must have shape (num_envs,)")
        check(lib().zenv_schedule_ring(self._h, f.ctypes.data, int(depth)))

    def update_bank(self, slots, seeds, n_threads=4):
        """Refill bank slots in place with the layouts of `seeds` (zenv_bank_update; stream-ordered)."""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        sd = np.ascontiguousarray(seeds, np.int64).reshape(-1)
        if sl.shape != sd.shape:
            raise ValueError("one seed per slot")
        check(lib().zenv_bank_update(self._h, sl.ctypes.data, sd.ctypes.data, sl.size, int(n_threads)))

    # ---- layouts sampled on the device (K20): only seeds cross the bus.  TSP / ColourMatch handles; TimedTSP and
    # solver-ordered handles raise ZenvError(E_STATE) and stay on the host calls above -- a TimedTSP handle until
    # timed_layouts_device() opts in, a solver-ordered one until order_routes_device() does
    def timed_layouts_device(self, enable=True):
        """Let the device-sampling calls below take this TimedTSP handle (zenv_timed_layouts_device): its bank is then
        ``sample_layout_timed``'s, deadlines through the shared det_log, and ``update_bank`` refills with that sampler
        too.  ZenvError(E_ARG) on another task's handle or unless beta_a > 1 and beta_b > 1."""
        check(lib().zenv_timed_layouts_device(self._h, int(bool(enable))))

    sample_layout_timed = staticmethod(sample_layout_timed)
    det_ops = staticmethod(det_ops)

    def order_routes_device(self, enable=True):
        """Let the device-sampling calls below take this solver-ordered handle (zenv_order_routes_device): the wave
        that samples a layout solves its tour (K21) and the row's aux column is ``route_ranks``' -- the same bank as
        ``build_bank``'s, bit for bit.  A row the device refills always carries the built-in tour, never ranks put
        there with ``set_bank(aux=...)``.  ZenvError(E_ARG) unless ``enable_order()`` came first."""
        check(lib().zenv_order_routes_device(self._h, int(bool(enable))))

    def route_ranks_device(self, robot, zones, moves=False):
        """``route_ranks`` of a batch on the device, one wave per layout (zenv_route_ranks_device; synchronous, any
        handle): robot (count, 2), zones (count, Z', 2) with any 1 <= Z' <= MAX_ZONES -> rank (count, Z') int32 and,
        with moves=True, also moves (count, 5)."""
        z = np.ascontiguousarray(zones, np.float64)
        if z.ndim != 3 or z.shape[2] != 2:
            raise ValueError("zones must have shape (count, num_zones, 2)")
        r = np.ascontiguousarray(np.asarray(robot, np.float64)[..., :2])
        if r.shape != (z.shape[0], 2):
            raise ValueError("robot must have shape (count, 2)")
        rank = np.zeros(z.shape[:2], np.int32)
        mv = np.zeros((z.shape[0], 5), np.int32)
        check(lib().zenv_route_ranks_device(self._h, r.ctypes.data, z.ctypes.data, z.shape[0], z.shape[1],
                                            rank.ctypes.data, mv.ctypes.data if moves else None))
        return (rank, mv) if moves else rank

    def build_bank_device(self, seed_first, count):
        """``build_bank`` sampled on the device (zenv_bank_build_device; synchronous, same bank bit for bit)."""
        check(lib().zenv_bank_build_device(self._h, int(seed_first), int(count)))

    def build_bank_seeds_device(self, seeds):
        """``build_bank_seeds`` sampled on the device (zenv_bank_build_seeds_device)."""
        s = np.ascontiguousarray(seeds, np.int64).reshape(-1)
        check(lib().zenv_bank_build_seeds_device(self._h, s.ctypes.data, s.size))

    def update_bank_device(self, slots, seeds):
        """``update_bank`` sampled on the device (zenv_bank_update_device; stream-ordered).  A slot whose seed the device
        could not finish keeps its contents and shows up in ``sample_status()``."""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        sd = np.ascontiguousarray(seeds, np.int64).reshape(-1)
        if sl.shape != sd.shape:
            raise ValueError("one seed per slot")
        check(lib().zenv_bank_update_device(self._h, sl.ctypes.data, sd.ctypes.data, sl.size))

    def ring_stream(self, seed0, depth):
        """Env i's k-th episode is the layout of env seed ``seed0[i] + k``, for ever: a num_envs x depth bank sampled
        on the device, a ring schedule over it (zenv_ring_stream) and ``ring_refill()`` to keep it ahead -- at least
        once per `depth` episodes of an env.  An explicit ``reset()`` / ``reset(mask)`` takes a map from the ring like
        an auto-reset does, and the ring guard does not count it: call ``ring_refill()`` after it too.  Memory: 88 +
        20 Z bytes per slot (588 B at Z = 25)."""
        s = np.ascontiguousarray(seed0, np.int64)
        if s.shape != (self.num_envs,):
            raise ValueError("seed0 must have shape (num_envs,)")
        check(lib().zenv_ring_stream(self._h, s.ctypes.data, int(depth)))

    def ring_refill(self):
        """Resample, on the device, every ring slot whose episode is behind its env (zenv_ring_refill): asynchronous,
        stream-ordered, no host synchronisation."""
        check(lib().zenv_ring_refill(self._h))

    def sample_status(self):
        """Synchronise and take the device sampler's failure list (zenv_sample_status).

        Returns dict(slots, seeds, codes, n_failed, n_sampled_total): the listed entries (at most SAMPLE_STATUS_CAP;
        codes SAMPLE_UNFINISHED / SAMPLE_SEED_RANGE), how many entries were left untouched since the last call, and
        the layouts the device has written since the handle was made."""
        cap = nat.SAMPLE_STATUS_CAP
        slots, seeds, codes = np.zeros(cap, np.int32), np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        n_failed, total = C.c_int32(0), C.c_int64(0)
        check(lib().zenv_sample_status(self._h, slots.ctypes.data, seeds.ctypes.data, codes.ctypes.data, cap,
                                       C.byref(n_failed), C.byref(total)))
        n = min(n_failed.value, cap)
        return dict(slots=slots[:n].copy(), seeds=seeds[:n].copy(), codes=codes[:n].copy(), n_failed=n_failed.value,
                    n_sampled_total=total.value)

    def read_bank(self, first=0, count=None):
        """Synchronise and copy bank rows out (zenv_bank_read): dict(robot [count,4] (x, y, cos(rot/2), sin(rot/2)),
        zone_xy [count,Z,2], aux [count,Z], seeds [count], first [count,12] float32 (first observation, first greedy
        action, pad))."""
        first = int(first)
        count = self.bank_size - first if count is None else int(count)
        n, Z = max(count, 0), self.num_zones
        out = dict(robot=np.zeros((n, 4), np.float64), zone_xy=np.zeros((n, Z, 2), np.float64),
                   aux=np.zeros((n, Z), np.int32), seeds=np.zeros(n, np.int64), first=np.zeros((n, 12), np.float32))
        check(lib().zenv_bank_read(self._h, first, count, out["robot"].ctypes.data, out["zone_xy"].ctypes.data,
                                   out["aux"].ctypes.data, out["seeds"].ctypes.data, out["first"].ctypes.data))
        return out

    def schedule_fixed_seeds(self, rng_seeds, min_seed, max_seed):
        s = np.ascontiguousarray(rng_seeds, np.uint64)
        if s.shape != (self.num_envs,):
            raise ValueError("rng_seeds must have shape (num_envs,)")
        check(lib().zenv_schedule_fixed_seeds(self._h, s.ctypes.data, int(min_seed), int(max_seed)))

    # ------------------------------------------------------------------ hot path
    def reset(self, mask=None):
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            if m.shape != (self.num_envs,):
                raise ValueError("mask must have shape (num_envs,)")
        check(lib().zenv_reset(self._h, None if m is None else m.ctypes.data))

    def step(self, actions=None, auto_reset=True):
        """actions: (N,2) float32 ndarray (host), or None to use the device action buffer."""
        if actions is None:
            check(lib().zenv_step(self._h, None, 0, int(bool(auto_reset))))
            return
        a = np.ascontiguousarray(actions, np.float32)
        if a.shape != (self.num_envs, 2):
            raise ValueError(f"actions must have shape ({self.num_envs}, 2)")
        check(lib().zenv_step(self._h, a.ctypes.data, 0, int(bool(auto_reset))))

    _RESET_MODES = {"never": nat.CHUNK_NO_RESET, "every": nat.CHUNK_RESET_EVERY, "last": nat.CHUNK_RESET_LAST}

    def step_many(self, actions, reset="every", actions_ptr=None):
        """An action chunk (zenv_step_many): K steps of caller-supplied actions, one launch of the persistent kernel per
        256 steps.  actions: (K, N, 2) float32 (host), or actions_ptr = (device address, K) for a device buffer.
        reset: "every" (K x step), "never" (K x step_no_reset) or "last" (K - 1 x step_no_reset, then one step: the
        fixed-length-skill loop, _hier_policy_opt.py:68-71).  Asynchronous like step(); afterwards observations() /
        results() hold the last step, chunk_results() every step's reward and done flag."""
        mode = self._RESET_MODES[reset]
        if actions_ptr is not None:
            ptr, k = actions_ptr
            check(lib().zenv_step_many(self._h, C.c_void_p(int(ptr)), 1, int(k), mode))
            return
        a = np.ascontiguousarray(actions, np.float32)
        if a.ndim != 3 or a.shape[1:] != (self.num_envs, 2) or a.shape[0] < 1:
            raise ValueError(f"actions must have shape (K, {self.num_envs}, 2)")
        check(lib().zenv_step_many(self._h, a.ctypes.data, 0, int(a.shape[0]), mode))

    def chunk_results(self):
        """(reward float32 (K,N), done bool (K,N)) of the last step_many(), time-major."""
        k = lib().zenv_field_bytes(self._h, nat.F_CHUNK_DONE) // self.num_envs
        r = np.empty((k, self.num_envs), np.float32)
        d = np.empty((k, self.num_envs), np.uint8)
        check(lib().zenv_get(self._h, nat.F_CHUNK_REWARD, r.ctypes.data, 0))
        check(lib().zenv_get(self._h, nat.F_CHUNK_DONE, d.ctypes.data, 0))
        return r, d.astype(bool)

    def step_device(self, actions_ptr, auto_reset=True):
        """actions_ptr: integer device address of a float32 [N,2] buffer (zero-copy policies)."""
        check(lib().zenv_step(self._h, C.c_void_p(int(actions_ptr)), 1, int(bool(auto_reset))))

    def policy(self, policy, policy_seed=0x5EED, env_index0=0, dst_ptr=None):
        check(lib().zenv_policy(self._h, int(policy), int(policy_seed), int(env_index0),
                                None if dst_ptr is None else C.c_void_p(int(dst_ptr))))

    def rollout(self, steps, policy, policy_seed=0x5EED, env_index0=0, auto_reset=True,
                time_step_kernel=False, fused=True, event_stride=1, mode=None, wait=True):
        """K closed-loop steps a_t = policy(obs_t, t); step(a_t) on the handle's stream.

        mode "persistent" (default): one launch advances every env by up to 256 steps, state in
        registers, all per-step outputs still written on every step; "per_step": one step-kernel
        launch per step which also emits the next action; "unfused" (or fused=False): per-step
        launches with a stand-alone policy kernel before each.  Same results in all three.

        Returns (ms_total, ms_step_kernel_avg or None), both from HIP events on that stream;
        the kernel figure is kernel time per step (see include/zenv.h)."""
        if mode is None:
            mode = "persistent" if fused else "unfused"
        flags = {"persistent": 0, "per_step": nat.ROLLOUT_PER_STEP, "unfused": nat.ROLLOUT_UNFUSED}[mode]
        if not wait:            # enqueue only (ZENV_ROLLOUT_ASYNC): collect with done() / sync(); no times
            flags |= nat.ROLLOUT_ASYNC
        total = C.c_float(0)
        kern = C.c_float(0)
        check(lib().zenv_rollout(self._h, int(steps), int(policy), int(policy_seed),
                                 int(env_index0), int(bool(auto_reset)),
                                 flags, int(event_stride), C.byref(total),
                                 C.byref(kern) if time_step_kernel else None))
        return total.value, (kern.value if time_step_kernel else None)

    def set_rollout_slice(self, envs_per_launch):
        """Envs one persistent launch covers (default 65 536; 0 = the whole batch in one launch): zenv_set_rollout_slice."""
        check(lib().zenv_set_rollout_slice(self._h, int(envs_per_launch)))

    # ------------------------------------------------------------------ solver-ordered variant (8(f) row 3)
    def enable_order(self, fresh_route_in_first_obs=False):
        """TSPOrderEnv semantics (TSP_order_env.py:13-113); call before build_bank / set_bank -- an episode's
        route is the bank's aux column (built-in PATH_CHEAPEST_ARC + local-search tour, or the caller's ranks).
        Default = the reference's reset(): the first observation of an episode is built before generate_route()
        (:108-113) and carries the order feature of the route the env was left with.  fresh_route_in_first_obs=True:
        the first observation shows the new episode's route (the build's opt-out, not reference behaviour)."""
        check(lib().zenv_order_enable(self._h))
        check(lib().zenv_order_configure(self._h, nat.ORDER_FRESH_FIRST_OBS if fresh_route_in_first_obs else 0))

    def order_rows(self, enable=True):
        """The flat network on the reference's (Z, 7) rows (zenv_order_rows; TSP_order_env.py:37-47): while on,
        ``net_zone_feat`` is 7 and ``load_mlp``, ``mlp_forward``, the MLP policies of ``policy`` / ``rollout``,
        ``collect`` and the ``ppo_*`` calls take rows of [zone_obs row (6), order value]; ``get(F_ORDER_ROWS)`` shows
        them.  ``collect`` then records float32(shaped_reward) as the reward (base.py:159-162).  Toggling drops the loaded
        network, the flat learner and the experience buffers: load them again.  ZenvError(E_STATE) unless
        ``enable_order()`` came first."""
        check(lib().zenv_order_rows(self._h, int(bool(enable))))
        if bool(enable) != getattr(self, "_order_rows", False):      # (no change: nothing was dropped)
            for key in ("ppo", "a2c"):                                # the library dropped both flat learners
                self._learners.pop((key, None), None)
        self._order_rows = bool(enable)

    @property
    def net_zone_feat(self):
        """The width of the zone rows the flat network reads, records and trains on: ``zone_feat``, or 7 on a
        solver-ordered handle with ``order_rows()`` on."""
        return self.zone_feat + (1 if getattr(self, "_order_rows", False) else 0)

    def order_info(self):
        """(shaped_reward float64 [N], order feature float32 [N,Z] of the last observation: 0.5^(position in the route
        that observation saw))."""
        return self.get(nat.F_SHAPED_REWARD), self.get(nat.F_ORDER_VAL)

    def order_routes(self):
        """self.route of every env as positions: int8 [N,Z], position of zone z in the remaining route, -1 = not in it."""
        return self.get(nat.F_ORDER_POS)

    # ------------------------------------------------------------------ goal-conditioned variant (8(f) row 3)
    def enable_goals(self):
        """TSPNextCityEnv / TimedTSPNextCityEnv semantics (TSP_next_city_env.py:41-109): after this every
        ``step`` also yields shaped_reward / need_next_goal / available goals, see ``goal_info``."""
        check(lib().zenv_goal_enable(self._h))

    def set_goals(self, goals):
        """goals: int32 [N], -1 = leave that env's goal alone (penv.py:76-80 set_goal, batched)."""
        g = np.ascontiguousarray(goals, np.int32)
        if g.shape != (self.num_envs,):
            raise ValueError(f"goals must have shape ({self.num_envs},)")
        check(lib().zenv_set_goals(self._h, g.ctypes.data))

    def solver_goals(self):
        """ColourMatchSolverEnv.solver_get_next_goal (zone-goals/envs/colour_match_solver_env.py:57-97) of every env:
        int32 [N], the nearest zone a cheapest recolouring plan has to cycle."""
        g = np.empty(self.num_envs, np.int32)
        check(lib().zenv_solver_goals(self._h, g.ctypes.data))
        return g

    def goal_info(self):
        """(shaped_reward float64 [N], need_next_goal bool [N], available uint32 bit masks [N], goal int32 [N])."""
        if getattr(self, "_goal_host", None) is None:      # page-locked images: four downloads, one synchronisation
            fields = (nat.F_SHAPED_REWARD, nat.F_NEED_GOAL, nat.F_AVAILABLE_GOALS, nat.F_GOAL)
            self._goal_host = (fields, [self._own_pinned_array(self._shape(f), _FIELD_DTYPES[f]) for f in fields])
        fields, arrays = self._goal_host
        self.results_into(fields, arrays)
        return (arrays[0].copy(), arrays[1].astype(bool), arrays[2].copy(), arrays[3].copy())

    # ------------------------------------------------------------------ actor network
    @staticmethod
    def _load_weights(struct, names, tensors, want):
        """Point struct.<name> at tensors[name], made contiguous float32 and checked against the shape want[name], for
        every name.  Returns the arrays: the caller holds them until its zenv_*_load call has copied them."""
        keep = {}
        for name in names:
            a = np.ascontiguousarray(tensors[name], np.float32)
            if a.shape != want[name]:
                raise ValueError(f"{name}: shape {a.shape}, expected {want[name]}")
            keep[name] = a
            setattr(struct, name, a.ctypes.data)
        return keep

    @staticmethod
    def _two_level_names(tensors, names, hi_critic, lo_critic):
        """The tensors a hierarchical agent's load hands over: both networks, and each critic that is there."""
        return names + (hi_critic if "hi_critic_w1" in tensors else ()) + (lo_critic if "lo_critic_w1" in tensors else ())

    def load_mlp(self, tensors, precision="auto"):
        """The reference's ZoneEnvModel + actor (env_model.py:48-79, policy_network.py:12-53) for the
        device policies POLICY_MLP_MEAN / POLICY_MLP_SAMPLE.  tensors: dict of float32 arrays named as in
        ``_native.MLP_TENSORS`` (see ``mlp_tensors_from_state_dict``), state_dict layout [out][in].

        precision -- the default keeps the reference's float32 arithmetic (its modules are torch float32):
          "auto" (default)  "f16x3", or "f32" when the weights leave float16's range (ZENV_E_RANGE at load); the mode
                            taken is in ``self.mlp_precision``
          "f16x3"           the 16-bit matrix instruction on hi / lo split float16 operands, three products per k-step:
                            mu / std / value within 3e-6 of torch float32 at 0.30 of "f32"'s time.  float16's range applies:
                            a weight >= 32 768 is refused here, an input / activation >= 65 520 raises
                            ZenvError(E_RANGE) at the next call that waits for the device (then load with "f32")
          "f32"             float32 throughout (f32 MFMA / FMA): within 1e-5 of torch float32
          "bf16x3"          the split with bfloat16 halves: within 2e-5 at 0.35 of "f32"'s time, float32's RANGE -- for
                            networks "f16x3" refuses when 1e-5 is not needed
        Reduced precision, opt-in (narrower arithmetic than the reference's -- for throughput experiments, not parity):
          "bf16"            bf16 MFMA kernels, 8x faster than "f32"; mu / std within 4e-2 of torch float32 by contract
          "f16"             the same kernels on float16 operands: within 1e-3; float16's range guaranteed by a bound on the
                            zone layers at load plus run-time checks (E_RANGE otherwise)."""
        if precision == "auto":
            try:
                self.load_mlp(tensors, precision="f16x3")
            except ZenvError as e:
                if e.code != nat.E_RANGE:
                    raise
                self.load_mlp(tensors, precision="f32")
            return
        h = int(np.asarray(tensors["zone_b1"]).shape[0])
        cols = np.asarray(tensors["zone_w1"]).shape[-1]
        if cols != 8 + self.net_zone_feat:
            raise ValueError(f"zone_w1 has {cols} input columns, this handle's network reads 8 + {self.net_zone_feat}"
                             " (obs + a zone row" + (" with the order value: order_rows() is on)"
                                                     if self.net_zone_feat != self.zone_feat else ")"))
        w = nat.MlpWeights(h_dim=h, precision={"bf16": nat.MLP_BF16, "f32": nat.MLP_F32, "bf16x3": nat.MLP_BF16X3,
                                                   "f16x3": nat.MLP_F16X3, "f16": nat.MLP_F16}[precision])
        names = nat.MLP_TENSORS + (nat.MLP_CRITIC_TENSORS if "critic_w1" in tensors else ()) + (
            nat.MLP_SIGMA_TENSORS if "critic_sigma_w" in tensors else ())
        self._mlp_has_critic = "critic_w1" in tensors
        self._mlp_distributional = "critic_sigma_w" in tensors
        keep = self._load_weights(w, names, tensors, mlp_tensor_shapes(h, self.net_zone_feat))   # alive across the load
        check(lib().zenv_mlp_load(self._h, C.byref(w)))
        self.mlp_precision = precision

    def mlp_forward(self, with_value=False):
        """(mu, std) float32 [N,2] of the actor's Normal for the current observations; with_value: also
        the critic's value float32 [N] (needs the critic tensors in load_mlp)."""
        check(lib().zenv_mlp_forward(self._h))
        out = (self.get(nat.F_POLICY_MU), self.get(nat.F_POLICY_STD))
        if with_value:
            if not getattr(self, "_mlp_has_critic", False):
                raise ValueError("load_mlp was called without critic tensors")
            out += (self.get(nat.F_POLICY_VALUE),)
            if getattr(self, "_mlp_distributional", False):     # value = (mu, sigma), flat_model.py:57-60
                out += (self.get(nat.F_POLICY_VALUE_SIGMA),)
        return out

    # ------------------------------------------------------------------ Zone-goals hierarchical agent
    def load_hier(self, tensors, precision="f32"):
        """HighPolicyValueModel + LoPolicyValueModel (zone-goals/src/hier_policy_value_models.py:19-86) for
        ``hier_forward`` and the device policies POLICY_HIER_SAMPLE / POLICY_HIER_MEAN.  tensors: dict of float32
        arrays named as in ``_native.HIER_*`` (see ``hier_tensors_from_state_dicts``); each critic is optional.  Needs
        ``enable_goals()`` first.  precision: "f32" (the only one built: float32 throughout, within 1e-5 of torch)."""
        if precision != "f32":
            raise ValueError(f"precision {precision!r}: the hierarchical agent is built in float32 only")
        h = int(np.asarray(tensors["hi_zone_b1"]).shape[0])
        F = int(np.asarray(tensors["hi_zone_w1"]).shape[1]) - 8
        names = self._two_level_names(tensors, nat.HIER_HI_TENSORS + nat.HIER_LO_TENSORS, nat.HIER_HI_CRITIC,
                                      nat.HIER_LO_CRITIC)
        w = nat.HierWeights(h_dim=h, precision=nat.MLP_F32, zone_feat=F)
        keep = self._load_weights(w, names, tensors, hier_tensor_shapes(h, F))   # alive across the load
        check(lib().zenv_hier_load(self._h, C.byref(w)))
        self._hier_critics = ("hi_critic_w1" in tensors, "lo_critic_w1" in tensors)

    def hier_forward(self):
        """Both networks on the current observations: (logits float32 [N,Z] with -inf at unavailable zones, high-level
        value [N], mu [N,2], std [N,2], low-level value [N]); the low level towards each env's current goal, zeros for
        an env without one.  Values are 0 without the critic tensors."""
        check(lib().zenv_hier_forward(self._h))
        return (self.get(nat.F_HIER_LOGITS), self.get(nat.F_HIER_VALUE), self.get(nat.F_POLICY_MU),
                self.get(nat.F_POLICY_STD), self.get(nat.F_POLICY_VALUE))

    # ------------------------------------------------------------------ fixed-length-skills agent
    def load_skills(self, tensors, skill_len=200, precision="f32"):
        """HighPolicyValueModel + LoPolicyValueModel of the skill planner (main/src/hier_policy_value_models.py:19-76)
        for ``skill_forward`` and the device policies POLICY_SKILL_SAMPLE / POLICY_SKILL_MEAN, which pick a new skill
        every ``skill_len`` steps of an episode (evaluate_hier.py:21, :63-64).  tensors: dict of float32 arrays named
        as in ``_native.SKILL_*`` (see ``skill_tensors_from_state_dicts``); each critic is optional.  A plain task
        handle only (not ``enable_goals`` / ``enable_order``).  Every env starts without a skill.  precision: "f32"
        (the only one built: float32 throughout, within 1e-5 of torch)."""
        if precision != "f32":
            raise ValueError(f"precision {precision!r}: the skill agent is built in float32 only")
        logit = np.asarray(tensors["hi_logit_w"])
        S, h = int(logit.shape[0]), int(logit.shape[1])
        F = int(np.asarray(tensors["hi_zone_w1"]).shape[1]) - 8
        names = self._two_level_names(tensors, nat.SKILL_HI_TENSORS + nat.SKILL_LO_TENSORS, nat.SKILL_HI_CRITIC,
                                      nat.SKILL_LO_CRITIC)
        w = nat.SkillWeights(h_dim=h, n_skills=S, zone_feat=F, precision=nat.MLP_F32)
        keep = self._load_weights(w, names, tensors, skill_tensor_shapes(h, S, F))   # alive across the load
        check(lib().zenv_skill_configure(self._h, int(skill_len)))
        check(lib().zenv_skill_load(self._h, C.byref(w)))
        if S != getattr(self, "_skill_n", S) or h != getattr(self, "_skill_h", h):
            self._skill_inverse = False                      # zenv_skill_load dropped an inverse model of other shapes
        self._skill_n, self._skill_h, self._skill_len = S, h, int(skill_len)

    def configure_skills(self, skill_len):
        """A new skill every ``skill_len`` steps (>= 1) from the next pick on."""
        check(lib().zenv_skill_configure(self._h, int(skill_len)))
        self._skill_len = int(skill_len)

    def set_skills(self, skills):
        """skills: int32 [N] in -1 .. S-1; env i gets skills[i] with its age restarting at 0, -1 leaves it alone."""
        s = np.ascontiguousarray(skills, np.int32)
        if s.shape != (self.num_envs,):
            raise ValueError(f"skills must have shape ({self.num_envs},)")
        check(lib().zenv_set_skills(self._h, s.ctypes.data))

    def skill_forward(self):
        """Both networks on the current observations: (log-softmax logits float32 [N,S], high-level value [N], mu [N,2],
        std [N,2], low-level value [N]); the low level under each env's current skill (``get(F_SKILL)``), zeros for an
        env without one.  Values are 0 without the critic tensors.  The skill state does not move."""
        check(lib().zenv_skill_forward(self._h))
        return (self.get(nat.F_SKILL_LOGITS), self.get(nat.F_SKILL_VALUE), self.get(nat.F_POLICY_MU),
                self.get(nat.F_POLICY_STD), self.get(nat.F_POLICY_VALUE))

    # ------------------------------------------------------------------ variable-length Options agent
    def load_options(self, tensors, precision="f32"):
        """HighPolicyValueModel + LoPolicyValueModel of the Options agent (options/src/hier_policy_value_models.py) for
        ``option_forward`` and the device policies POLICY_OPTION_SAMPLE / POLICY_OPTION_MEAN, which pick a new skill
        whenever the last one's option ended (options/scripts/evaluate_hier.py:63-75).  tensors: dict of float32 arrays
        named as in ``_native.SKILL_*`` with three rows in lo_mu_* / lo_std_* (see ``option_tensors_from_state_dicts``);
        each critic is optional.  A plain task handle only.  A handle holds one agent of the skill family: this drops
        loaded skill (and inverse) weights, ``load_skills`` drops these.  Every env starts without a skill."""
        if precision != "f32":
            raise ValueError(f"precision {precision!r}: the Options agent is built in float32 only")
        logit = np.asarray(tensors["hi_logit_w"])
        S, h = int(logit.shape[0]), int(logit.shape[1])
        F = int(np.asarray(tensors["hi_zone_w1"]).shape[1]) - 8
        names = self._two_level_names(tensors, nat.SKILL_HI_TENSORS + nat.SKILL_LO_TENSORS, nat.SKILL_HI_CRITIC,
                                      nat.SKILL_LO_CRITIC)
        w = nat.OptionWeights(h_dim=h, n_skills=S, zone_feat=F, precision=nat.MLP_F32)
        keep = self._load_weights(w, names, tensors, option_tensor_shapes(h, S, F))   # alive across the load
        check(lib().zenv_option_load(self._h, C.byref(w)))
        self._skill_inverse = False
        self._skill_n, self._skill_h = S, h

    def option_forward(self):
        """Both networks on the current observations, the state untouched: ``skill_forward``'s five arrays (log-softmax
        logits [N,S], high-level value [N], mu [N,2], std [N,2], low-level value [N]) and the third actor output as
        (mu_2, std_2, prob = sigmoid(4 mu_2 - 3)), float32 [N] each; zeros for an env without a skill."""
        check(lib().zenv_option_forward(self._h))
        return (self.get(nat.F_SKILL_LOGITS), self.get(nat.F_SKILL_VALUE), self.get(nat.F_POLICY_MU),
                self.get(nat.F_POLICY_STD), self.get(nat.F_POLICY_VALUE), self.get(nat.F_OPTION_TERM_MU),
                self.get(nat.F_OPTION_TERM_STD), self.get(nat.F_OPTION_TERM_PROB))

    def collect_options(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """collect_experiences of the Options agent (options/src/torch_ac/algos/_hier_policy_opt.py:10-205) on the
        device with the loaded agent (``load_options`` with both critics).  Returns (lo, hi, termination_rate), the
        reference's lo_exps / hi_exps and logs['termination_rate'], numpy:
          lo  [N, T-1, ...]: obs, zone_obs, skill, action [.., 3] and log_prob [.., 3] (the third component decides the
              termination), ended (bool, the termination draw), value, advantage, returnn, reward, env_reward (the
              same), mask -- reshape(N*(T-1), ...) is the reference's flat order
          hi  [M, ...] env-major: obs, zone_obs, action (the skill, int32), value, log_prob, advantage, returnn
              (hi_exps), reward and mask (what the GAE used); and count (int32 [N], rows of every env: sum = M)
          termination_rate  the share of all T * N frames whose option ended (:182)
        Unlike the device policies, the collector lets a skill survive an auto-reset, as the reference's training loop
        does.  The transition an env has open at the end stays on the device and is the first of its next call; the
        handle must not be stepped by other means in between."""
        T, M = self.collect_options_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
        lo_l, hi_l = option_experience_layout(self.num_envs, self.num_zones, self.zone_feat, T, M)
        raw = self._download(lo_l)
        rate = float(raw["ended"].mean())
        raw["action"] = np.concatenate([raw["action"], raw.pop("term_action")[..., None]], axis=-1)
        raw["log_prob"] = np.concatenate([raw["log_prob"], raw.pop("term_log_prob")[..., None]], axis=-1)
        raw["ended"] = raw["ended"].view(bool)
        lo = {name: a[:T - 1].swapaxes(0, 1) for name, a in raw.items()}
        hi = self._download(hi_l, skip=not M)
        hi["count"] = self.get(nat.F_HI_COUNT)
        return lo, hi, rate

    def collect_options_on_device(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """The same collection, results left in the handle's device buffers (``option_experience_layout`` names them).
        Returns (T, M)."""
        T, seed, index0, discount, gae_lambda = check_collect_option_args(frames_per_proc, policy_seed, env_index0,
                                                                          discount, gae_lambda)
        m = C.c_int64(0)
        check(lib().zenv_collect_option(self._h, T, seed, index0, discount, gae_lambda, C.byref(m)))
        self._exp_has_goals = False
        return T, int(m.value)

    # ------------------------------------------------------------------ xy-goals hierarchical agent
    def load_xy(self, tensors, skill_len=200, precision="f32"):
        """HighPolicyValueModel + LoPolicyValueModel of the xy-goals agent (xy-goals/src/hier_policy_value_models.py:
        19-72) for ``xy_forward`` and the device policies POLICY_XY_SAMPLE / POLICY_XY_MEAN, which draw a new goal in
        the plane every ``skill_len`` steps of an episode (evaluate_xy_hrl.py:21, :62-66).  tensors: dict of float32
        arrays named as in ``_native.XY_*`` (see ``xy_tensors_from_state_dicts``); each critic is optional.  A plain
        task handle only.  The agent runs on the skill family's per-env clock: this drops loaded skill, option and
        inverse weights, ``load_skills`` / ``load_options`` drop these.  Every env starts without a goal.  precision:
        "f32" (the only one built: float32 throughout, within 1e-5 of torch)."""
        if precision != "f32":
            raise ValueError(f"precision {precision!r}: the xy-goals agent is built in float32 only")
        h = int(np.asarray(tensors["hi_zone_b1"]).shape[0])
        F = int(np.asarray(tensors["hi_zone_w1"]).shape[1]) - 8
        names = self._two_level_names(tensors, nat.XY_HI_TENSORS + nat.XY_LO_TENSORS, nat.XY_HI_CRITIC,
                                      nat.XY_LO_CRITIC)
        w = nat.XyWeights(h_dim=h, zone_feat=F, precision=nat.MLP_F32)
        keep = self._load_weights(w, names, tensors, xy_tensor_shapes(h, F))   # alive across the load
        check(lib().zenv_skill_configure(self._h, int(skill_len)))
        check(lib().zenv_xy_load(self._h, C.byref(w)))
        self._skill_inverse = False
        self._skill_len = int(skill_len)

    def set_xy_goals(self, goals, mask=None):
        """goals: float32 [N, 2]; env i with mask[i] (mask None = every env) gets goals[i] with its age restarting at
        0.  A non-finite goal under the mask is refused (E_ARG) with nothing changed."""
        g = np.ascontiguousarray(goals, np.float32)
        if g.shape != (self.num_envs, 2):
            raise ValueError(f"goals must have shape ({self.num_envs}, 2)")
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
            if m.shape != (self.num_envs,):
                raise ValueError(f"mask must have shape ({self.num_envs},)")
        check(lib().zenv_set_xy_goals(self._h, g.ctypes.data, None if m is None else m.ctypes.data))

    def xy_forward(self):
        """Both networks on the current observations: (goal_mu float32 [N,2], goal_std [N,2], high-level value [N], mu
        [N,2], std [N,2], low-level value [N]); the low level under each env's current goal (``get(F_XY_GOAL)``), zeros
        for an env without one (``get(F_XY_GOAL_AGE)`` = -1).  Values are 0 without the critic tensors.  The state does
        not move."""
        check(lib().zenv_xy_forward(self._h))
        return (self.get(nat.F_XY_GOAL_MU), self.get(nat.F_XY_GOAL_STD), self.get(nat.F_XY_VALUE),
                self.get(nat.F_POLICY_MU), self.get(nat.F_POLICY_STD), self.get(nat.F_POLICY_VALUE))

    def collect_xy(self, frames_per_proc, policy_seed=0, env_index0=0, discount=0.99, gae_lambda=0.95):
        """collect_experiences of the xy-goals agent (xy-goals/src/torch_ac/algos/_hier_policy_opt.py:10-192) on the
        device with the loaded agent (``load_xy`` with both critics).  Returns (lo, hi, num_frames) under the
        reference's names, numpy:
          lo  [N, T, ...]: obs, zone_obs, goal, action, log_prob, value, advantage, returnn, reward (the
              distance-to-goal reward), goal_dist, env_reward, mask -- reshape(N*T, ...) is the reference's flat order
          hi  [M, ...] env-major, M = N T / skill_len: obs, zone_obs, goal, value, log_prob (summed over the goal's two
              dimensions), advantage, returnn (hi_exps), reward (the window's sum of env rewards) and mask (its
              next_mask)
          num_frames  logs['num_frames']"""
        T, M = self.collect_xy_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
        L = T * self.num_envs // M
        lo_l, hi_l = xy_experience_layout(self.num_envs, self.num_zones, self.zone_feat, T, L)
        lo = {name: a.swapaxes(0, 1) for name, a in self._download(lo_l).items()}
        return lo, self._download(hi_l), skill_num_frames(lo["mask"].swapaxes(0, 1), L)

    def collect_xy_on_device(self, frames_per_proc, policy_seed=0, env_index0=0, discount=0.99, gae_lambda=0.95):
        """The same collection, results left in the handle's device buffers (``xy_experience_layout`` names them).
        Returns (T, M)."""
        L = getattr(self, "_skill_len", 200)                  # zenv_skill_configure's default until load_xy
        T, seed, index0, discount, gae_lambda = check_collect_xy_args(frames_per_proc, L, policy_seed, env_index0,
                                                                      discount, gae_lambda)
        check(lib().zenv_collect_xy(self._h, T, seed, index0, discount, gae_lambda))
        self._exp_has_goals = True          # ZENV_F_LO_GOAL holds this collection's goals (render_experience's marks)
        return T, self.num_envs * (T // L)

    def load_skill_inverse(self, tensors, precision="f32"):
        """InverseModel, DIAYN's discriminator (main/src/inverse_model.py), for the diversity reward of
        ``collect_skills``.  tensors: dict of float32 arrays named as in ``_native.SKILL_INVERSE_TENSORS`` (see
        ``inverse_tensors_from_state_dict``); its h, S and F must be those of the loaded skill weights."""
        if precision != "f32":
            raise ValueError(f"precision {precision!r}: the inverse model is built in float32 only")
        w2 = np.asarray(tensors["comb_w2"])
        S, h = int(w2.shape[0]), int(w2.shape[1])
        F = int(np.asarray(tensors["zone_w1"]).shape[1]) - 8
        w = nat.SkillInverseWeights(h_dim=h, n_skills=S, zone_feat=F, precision=nat.MLP_F32)
        keep = self._load_weights(w, nat.SKILL_INVERSE_TENSORS, tensors,   # alive across the load
                                  inverse_tensor_shapes(h, S, F))
        check(lib().zenv_skill_inverse_load(self._h, C.byref(w)))
        self._skill_inverse = True

    def collect_skills(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95,
                       diversity_coef=0.0, skill_prior_logits=None, sample_hi=True):
        """HierPolicyAlgo.collect_experiences of the skill planner / DIAYN (main/src/torch_ac/algos/
        _hier_policy_opt.py:9-233) on the device with the loaded skill agent (``load_skills`` with both critics) and,
        for the diversity reward, ``load_skill_inverse``.  sample_hi=False is the reference's train_hi == False:
        uniform skills.  Returns (lo, hi, inverse, num_frames) under the reference's names, numpy:
          lo  [N, T, ...]: obs, zone_obs, skill, action, log_prob, value, advantage, returnn, reward (lo_reward),
              env_reward, diversity, mask -- reshape(N*T, ...) is the reference's flat order (lo_exps)
          hi  [M, ...] env-major, M = N T / skill_len: obs, zone_obs, action (the skill), value, log_prob, advantage,
              returnn (hi_exps), reward (the window's sum) and mask (its next_mask)
          inverse  obs, zone_obs, skill: lo obs of frame i+1 with the skill of frame i where mask[i+1], env-major
          num_frames  logs['num_frames']"""
        T, M = self.collect_skills_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda,
                                             diversity_coef, skill_prior_logits, sample_hi)
        L = T * self.num_envs // M
        lo_l, hi_l = skill_experience_layout(self.num_envs, self.num_zones, self.zone_feat, T, L)
        lo = {name: a.swapaxes(0, 1) for name, a in self._download(lo_l).items()}
        hi = self._download(hi_l)
        keep = lo["mask"][:, 1:] != 0                                   # [N, T-1], env-major
        inverse = {"obs": lo["obs"][:, 1:][keep], "zone_obs": lo["zone_obs"][:, 1:][keep],
                   "skill": lo["skill"][:, :-1][keep]}
        return lo, hi, inverse, skill_num_frames(lo["mask"].swapaxes(0, 1), L)

    def collect_skills_on_device(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95,
                                 diversity_coef=0.0, skill_prior_logits=None, sample_hi=True):
        """The same collection, results left in the handle's device buffers (``skill_experience_layout`` names them).
        Returns (T, M)."""
        L = getattr(self, "_skill_len", 200)                  # zenv_skill_configure's default until load_skills
        T, seed, index0, discount, gae_lambda, coef, prior = check_collect_skill_args(
            frames_per_proc, L, policy_seed, env_index0, discount, gae_lambda, diversity_coef, skill_prior_logits,
            getattr(self, "_skill_n", None), getattr(self, "_skill_inverse", False))
        check(lib().zenv_collect_skill(self._h, T, seed, index0, discount, gae_lambda, coef,
                                       None if prior is None else prior.ctypes.data, 1 if sample_hi else 0))
        self._exp_has_goals = False
        return T, self.num_envs * (T // L)

    # ------------------------------------------------------------------ one PPO rollout
    def collect(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """BaseAlgo.collect_experiences (main/src/torch_ac/algos/base.py:131-227) on the device with the loaded
        actor-critic.  Returns a dict of env-major arrays [N, T, ...] -- reshape(N*T, ...) gives exps.* of the
        reference (:211-227): obs, zone_obs, action, log_prob, value, reward, mask, advantage, returnn (transposed
        views of time-major buffers: reshape copies them once)."""
        T = int(frames_per_proc)
        self.collect_on_device(T, policy_seed, env_index0, discount, gae_lambda)
        return {name: a.swapaxes(0, 1) for name, a in self._download(self._experience_rows(T)).items()}

    def collect_on_device(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """The same rollout, results left in the handle's device buffers (``experience_layout`` names them)."""
        check(lib().zenv_collect(self._h, int(frames_per_proc), int(policy_seed), int(env_index0),
                                 float(discount), float(gae_lambda)))
        self._exp_has_goals = False

    def experience_layout(self, frames_per_proc):
        """name -> (field id, shape in memory, time_major) of the float32 buffers one collect of T frames per env
        fills.  Everything is time-major [T, N, ...] in memory (the step kernel writes the observations in place, the
        head kernel and the GAE scan touch whole lines); ``collect`` hands out the [N, T, ...] views."""
        return {name: (field, shape, True) for name, (field, shape, _) in self._experience_rows(frames_per_proc).items()}

    def _experience_rows(self, frames_per_proc):
        """The same buffers as name -> (field id, shape in memory, dtype), the form of the agents' layouts."""
        return _lo_rows(self.num_envs, self.num_zones, self.net_zone_feat, int(frames_per_proc))

    # ------------------------------------------------------------------ the collectors' per-episode logs (K20)
    def episode_log_on_device(self):
        """zenv_episode_log: the reference's ``logs`` of the last collection (any of the five collectors), left in
        device buffers.  Once per collection; waits for the device once.  Returns the ``EpisodeLogInfo`` (kept, done,
        num_frames, columns)."""
        info = nat.EpisodeLogInfo()
        check(lib().zenv_episode_log(self._h, C.byref(info)))
        self._eplog_info = info
        return info

    def episode_log_ptr(self, column):
        """(device pointer, count) of a ``_native.EPLOG_*`` column of the last ``episode_log_on_device``."""
        ptr, count = C.c_void_p(), C.c_int64()
        check(lib().zenv_episode_log_tensor(self._h, int(column), C.byref(ptr), C.byref(count)))
        return ptr.value, count.value

    def episode_logs(self):
        """The second value of collect_experiences (main/src/torch_ac/algos/base.py:233-247 and the four trees'
        _hier_policy_opt.py), for the collector that ran last: ``return_per_episode``, ``reshaped_return_per_episode``
        and ``num_frames_per_episode`` (numpy float32 [max(done, N)]), ``num_frames`` (int), ``diversity_per_episode`` /
        ``prediction_per_episode`` where the reference's dict has them (``agents.EPISODE_LOG_KEYS``), and
        ``env_per_episode`` (int32, -1 for the initial zero entries).  The running sums and the last N entries are
        carried from call to call as the algo object carries them.  Once per collection."""
        info = self.episode_log_on_device()
        out = {}
        for key in episode_log_keys(info.columns) + (nat.EPLOG_KEYS[nat.EPLOG_ENV],):
            column = nat.EPLOG_KEYS.index(key)
            a = np.empty(info.kept, np.int32 if column == nat.EPLOG_ENV else np.float32)
            check(lib().zenv_episode_log_read(self._h, column, a.ctypes.data))
            out[key] = a
        out["num_frames"] = int(info.num_frames)
        return out

    def episode_log_stats(self):
        """{key: {"mean", "std", "min", "max"}} of every per-episode key of the last ``episode_logs`` /
        ``episode_log_on_device``: utils.synthesize (main/src/utils/other.py:15-21) reduced on the device in float64,
        std the population's as ``numpy.std``."""
        info = getattr(self, "_eplog_info", None)
        columns = info.columns if info is not None else 1          # no log yet: the library answers E_STATE
        out = {}
        for key in episode_log_keys(columns):
            stats = (C.c_double * 5)()
            check(lib().zenv_episode_log_stats(self._h, nat.EPLOG_KEYS.index(key), stats))
            out[key] = synthesize_stats(stats)
        return out

    def episode_log_reset(self):
        """Zero the running sums and the tail: the logs of a fresh algo object."""
        check(lib().zenv_episode_log_reset(self._h))

    # ------------------------------------------------------------------ the device learners
    # The thin methods of the seven families -- <key>_tensor_ptr, _tensors, _set_tensors, _state_dict(s),
    # _load_state_dict(s), _optimizer_state, _load_optimizer_state, _get_step, _set_step, _minibatch, _apply, _epoch and
    # _stats -- are installed from _FAMILIES (_install_forwarders); here are the inits, updates and publishes.
    def _learner_of(self, family, level=None):
        """The learner of a family (of a pair: of its level); before its init a bare one without tensor names: every
        call of it goes to the library, which answers ZENV_E_STATE (ZENV_E_ARG for a level that does not exist)."""
        fam = _FAMILIES[family]
        level = int(level) if fam.levels else None
        return self._learners.get((fam.key, level)) or _Learner(self._h, fam, level)

    # what the flat learners' tests have always reached for: the tensor names of the two, and the A2C learner itself
    _ppo_keys = property(lambda self: self._learner_of("ppo").keys)
    _a2c_keys = property(lambda self: self._learner_of("a2c").keys)
    _a2c = property(lambda self: self._learner_of("a2c"))

    def _flat_weights(self, state_dict_or_tensors):
        """(struct, tensors, shapes, what to keep alive across the call) of the flat learners' inits."""
        d = state_dict_or_tensors
        tensors = dict(d) if "zone_w1" in d else mlp_tensors_from_state_dict(d)
        h = int(np.asarray(tensors["zone_b1"]).shape[0])
        w = nat.MlpWeights(h_dim=h, precision=nat.MLP_F32)
        names = [n for n in nat.MLP_TENSORS + nat.MLP_CRITIC_TENSORS + nat.MLP_SIGMA_TENSORS if n in tensors]
        shapes = mlp_tensor_shapes(h, self.net_zone_feat)
        return w, tensors, shapes, self._load_weights(w, names, tensors, shapes)

    # ------------------------------------------------------------------ the flat actor-critic's PPO update
    def ppo_init(self, state_dict_or_tensors, lr=0.001, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.01,
                 value_loss_coef=0.5, max_grad_norm=0.5, max_batch=256, distributional_value=None):
        """The learner of update_parameters (torch_ac/algos/ppo.py:30-155) on the device: float32 master parameters
        from an ACModel state_dict (or the named tensors of ``mlp_tensors_from_state_dict``), their gradients and
        Adam's two moments, and the workspace of minibatches up to max_batch samples.  The defaults are PPOAlgo's
        (ppo.py:11-14).  distributional_value: None = whatever the tensors hold (critic_sigma).  Separate from
        ``load_mlp``: ``ppo_publish`` hands the parameters to the acting network."""
        w, tensors, shapes, keep = self._flat_weights(state_dict_or_tensors)     # keep: alive across the call
        if distributional_value is None:
            distributional_value = "critic_sigma_w" in tensors
        pc = nat.PpoConfig(lr=lr, adam_eps=adam_eps, clip_eps=clip_eps, entropy_coef=entropy_coef,
                           value_loss_coef=value_loss_coef, max_grad_norm=max_grad_norm, max_batch=int(max_batch),
                           distributional_value=int(bool(distributional_value)))
        check(lib().zenv_ppo_init(self._h, C.byref(w), C.byref(pc)))
        del keep
        self._learners[("ppo", None)] = _Learner(self._h, _FAMILIES["ppo"], None,
                                                 ppo_state_dict_keys(bool(distributional_value)), shapes, lr, adam_eps)
        self.ppo_batch_num = 0          # PPOAlgo.batch_num (ppo.py:28)

    def ppo_publish(self, precision="auto"):
        """Hand the learner's parameters to the acting network: read them back (0.7 MB) and ``load_mlp`` them, so
        the next collect acts with them.  One synchronisation per update."""
        self.load_mlp(self.ppo_tensors(), precision=precision)

    def ppo_update(self, epochs, batch_size, rng):
        """update_parameters (ppo.py:30-155) on the experience of the last collect: `epochs` passes in the order of
        ``ppo_batch_indexes`` (the permutation from the caller's numpy Generator, ``self.ppo_batch_num`` counting the
        calls).  Returns the reference's logs: the means over the last epoch's minibatches (ppo.py:137-153)."""
        T = lib().zenv_field_bytes(self._h, nat.F_EXP_VALUE) // (4 * self.num_envs)
        if T < 1:
            raise ZenvError(nat.E_STATE, "collect first: the handle holds no experience")
        for _ in range(int(epochs)):
            order = ppo_batch_indexes(self.num_envs * T, T, self.ppo_batch_num, rng)
            self.ppo_batch_num += 1
            self.ppo_epoch(order, batch_size)
        return ppo_logs(self.ppo_stats(), "critic_sigma_w" in self._learner_of("ppo").keys)

    # ------------------------------------------------------------------ the flat actor-critic's A2C update
    def a2c_init(self, state_dict_or_tensors, lr=0.01, rmsprop_alpha=0.99, rmsprop_eps=1e-8, entropy_coef=0.01,
                 value_loss_coef=0.5, max_grad_norm=0.5, max_batch=256):
        """The learner of A2CAlgo.update_parameters (torch_ac/algos/a2c.py:21-93, recurrence 1) on the device, beside
        the ``ppo_*`` one: float32 master parameters from an ACModel state_dict (or the named tensors of
        ``mlp_tensors_from_state_dict``), their gradients and RMSprop's square_avg.  The defaults are A2CAlgo's
        (a2c.py:10-12).  max_batch is the chunk an update walks the collection in: it sizes the activation
        workspace, not the batch the loss is averaged over, which is always all N x T frames.  The plain critic only."""
        w, _, shapes, keep = self._flat_weights(state_dict_or_tensors)           # keep: alive across the call
        ac = nat.A2cConfig(lr=lr, rmsprop_alpha=rmsprop_alpha, rmsprop_eps=rmsprop_eps, entropy_coef=entropy_coef,
                           value_loss_coef=value_loss_coef, max_grad_norm=max_grad_norm, max_batch=int(max_batch))
        check(lib().zenv_a2c_init(self._h, C.byref(w), C.byref(ac)))
        del keep
        self._learners[("a2c", None)] = _Learner(self._h, _FAMILIES["a2c"], None, ppo_state_dict_keys(False), shapes, lr,
                                                 rmsprop_eps, rmsprop_alpha)

    def a2c_accumulate(self, idx, total, first, count=None):
        """One chunk of an update over `total` frames: forward, loss and backward on the samples idx (host int32 array,
        or a device address with count; at most max_batch of them).  first: the chunk opens the update and overwrites
        the gradient arena, else it adds onto it.  Every mean divides by `total`.  Asynchronous."""
        self._learner_of("a2c").accumulate(idx, total, first, count)

    def a2c_publish(self, precision="auto"):
        """Hand the learner's parameters to the acting network (``load_mlp``), so the next collect acts with them."""
        self.load_mlp(self.a2c_tensors(), precision=precision)

    def a2c_update(self):
        """A2CAlgo.update_parameters on the experience of the last collect: all N x T frames in index order, in
        chunks of max_batch, one clip and RMSprop step.  Returns the reference's logs (a2c.py:85-91)."""
        self._learner_of("a2c").update()
        return a2c_logs(self.a2c_stats())

    # ------------------------------------------------------------------ the hierarchical agents' pairs of PPO updates
    def _pair_init(self, family, hi_state_dict, lo_state_dict, lo, hi):
        """zenv_<family>_init from the agent's two state_dicts with both critics; lo / hi: what to change from the
        family's default settings.  Registers the two learners."""
        fam = _FAMILIES[family]
        tensors = fam.tensors_from(hi_state_dict, lo_state_dict)
        F = int(tensors["hi_zone_w1"].shape[1]) - 8
        if fam.skills:
            S, h = (int(v) for v in tensors["hi_logit_w"].shape)
            dims, own = (h, S, F), dict(n_skills=S)
        else:
            h = int(tensors["hi_zone_b1"].shape[0])
            dims, own = (h, F), {}
        hi_keys, lo_keys = fam.keys()
        missing = [n for n in list(hi_keys) + list(lo_keys) if n not in tensors]
        if missing:
            raise ValueError(f"the update needs both critics: no {missing[0]}")
        shapes = fam.shapes(*dims)
        w = fam.weights(h_dim=h, zone_feat=F, precision=nat.MLP_F32, **own)
        keep = self._load_weights(w, list(hi_keys) + list(lo_keys), tensors, shapes)      # alive across the call
        cfgs = [nat.PpoConfig(distributional_value=0, **dict(getattr(self, base), **(over or {})))
                for base, over in zip(fam.defaults, (lo, hi))]
        check(getattr(lib(), fam.prefix + "init")(self._h, C.byref(w), C.byref(cfgs[0]), C.byref(cfgs[1])))
        del keep
        for level, keys in enumerate((lo_keys, hi_keys)):
            self._learners[(fam.key, level)] = _Learner(self._h, fam, level, keys, shapes, cfgs[level].lr,
                                                        cfgs[level].adam_eps)

    def _pair_publish(self, family):
        """Read both learners' parameters back and hand them to the family's acting agent."""
        fam = _FAMILIES[family]
        tensors = dict(self._learner_of(family, 1).tensors(), **self._learner_of(family, 0).tensors())
        extra = dict(skill_len=getattr(self, "_skill_len", 200)) if fam.loader_skill_len else {}
        getattr(self, fam.loader)(tensors, **extra)

    def _pair_update(self, family, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        """A pair's update_parameters on the records of the agent's last collection: the high level first (skipped, its
        logs zeros, when no row closed and the family allows that), then the low level, each epoch in the order of
        ``hppo_batch_indexes`` from the caller's numpy Generator.  Returns the reference's logs under lo_* / hi_*: the
        low level's are means over all its minibatches, the high level's over the last epoch's."""
        fam = _FAMILIES[family]
        T = lib().zenv_field_bytes(self._h, nat.F_EXP_VALUE) // (4 * self.num_envs)
        M = lib().zenv_field_bytes(self._h, fam.m_from[0]) // fam.m_from[1]
        lo_frames = T - 1 if fam.lo_drops_last else T
        if lo_frames < 1 or (fam.needs_rows and M < 1):
            raise ZenvError(nat.E_STATE, fam.no_experience)
        hi, lo = self._learner_of(family, 1), self._learner_of(family, 0)
        names = [(i, n) for i, n in enumerate(nat.PPO_STATS) if n != "value_std"]
        logs = {"hi_" + n: 0.0 for _, n in names}
        for _ in range(int(hi_epochs) if M else 0):
            hi.epoch(hppo_batch_indexes(M, rng), hi_batch_size)
        if M and int(hi_epochs) > 0:
            mean = hi.stats().astype(np.float64).mean(axis=0)
            logs = {"hi_" + n: float(mean[i]) for i, n in names}
        rows = []
        for _ in range(int(epochs)):
            lo.epoch(hppo_batch_indexes(self.num_envs * lo_frames, rng), batch_size)
            rows.append(lo.stats())
        mean = np.concatenate(rows).astype(np.float64).mean(axis=0) if rows else np.zeros(6)
        logs.update({"lo_" + n: float(mean[i]) for i, n in names})
        return logs

    # the examples' hyper-parameters (examples/zone_goals_ppo_torch.py, xy_goals_, skill_planner_ and options_ppo_torch.py;
    # the reference takes the norm and does not clip)
    HPPO_LO = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.003, value_loss_coef=0.5, max_grad_norm=math.inf,
                   max_batch=16384)
    HPPO_HI = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.2, entropy_coef=0.01, value_loss_coef=0.5, max_grad_norm=math.inf,
                   max_batch=4096)
    XYPPO_LO, XYPPO_HI = dict(HPPO_LO), dict(HPPO_HI)
    SKPPO_LO, SKPPO_HI = dict(HPPO_LO), dict(HPPO_HI)
    OPPPO_LO, OPPPO_HI = dict(HPPO_LO), dict(HPPO_HI)

    # ---- the Zone-goals agent
    def hppo_init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
        """The two learners of HierPolicyAlgo (zone-goals/src/torch_ac/algos/_hier_policy_opt.py:197-370) on the
        device, from HighPolicyValueModel / LoPolicyValueModel state_dicts with both critics: float32 master
        parameters, gradients, Adam's moments and a workspace per level.  lo / hi: dicts of the settings to change from
        ``HPPO_LO`` / ``HPPO_HI`` (lr, adam_eps, clip_eps, entropy_coef, value_loss_coef, max_grad_norm, max_batch).
        `level` in the other hppo_* methods: ``_native.HPPO_LO`` = 0, ``HPPO_HI`` = 1.  Separate from ``load_hier``:
        ``hppo_publish`` hands the parameters to the acting agent."""
        self._pair_init("hppo", hi_state_dict, lo_state_dict, lo, hi)

    def hppo_publish(self):
        """Hand both learners' parameters to the acting agent: read them back and ``load_hier`` them, so the next
        ``collect_hier`` acts with them."""
        self._pair_publish("hppo")

    def hppo_update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        """update_parameters (_hier_policy_opt.py:197-212) on the records of the last ``collect_hier``: the high level
        first, then the low level, each epoch in the order of ``hppo_batch_indexes`` from the caller's numpy Generator.
        Returns the reference's logs under lo_* / hi_*: the low level's are means over all its minibatches (its lists
        start before the epoch loop, :215-224), the high level's over the last epoch's (:293-300).  With M = 0 the high
        level is skipped and its logs are 0.0."""
        return self._pair_update("hppo", epochs, batch_size, hi_epochs, hi_batch_size, rng)

    # ---- the xy-goals agent
    def xyppo_init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
        """The two learners of the xy-goals agent (xy-goals/src/torch_ac/algos/_hier_policy_opt.py:195-363) on the
        device, from its HighPolicyValueModel / LoPolicyValueModel state_dicts with both critics: float32 master
        parameters, gradients, Adam's moments and a workspace per level.  lo / hi: dicts of the settings to change from
        ``XYPPO_LO`` / ``XYPPO_HI``.  `level` in the other xyppo_* methods: ``_native.XYPPO_LO`` = 0, ``XYPPO_HI`` = 1.
        Separate from ``load_xy``: ``xyppo_publish`` hands the parameters to the acting agent."""
        self._pair_init("xyppo", hi_state_dict, lo_state_dict, lo, hi)

    def xyppo_publish(self):
        """Hand both learners' parameters to the acting agent: read them back and ``load_xy`` them with the handle's
        current skill_len, so the next ``collect_xy`` acts with them."""
        self._pair_publish("xyppo")

    def xyppo_update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        """update_parameters (xy-goals' _hier_policy_opt.py:195-197) on the records of the last ``collect_xy``: the high
        level first, then the low level, each epoch in the order of ``hppo_batch_indexes`` from the caller's numpy
        Generator.  Returns the reference's logs under lo_* / hi_*: the low level's are means over all its minibatches
        (its lists start before the epoch loop), the high level's over the last epoch's."""
        return self._pair_update("xyppo", epochs, batch_size, hi_epochs, hi_batch_size, rng)

    # ---- the fixed-length-skills agent
    def skppo_init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
        """The two learners of the fixed-length-skills agent (main/src/torch_ac/algos/_hier_policy_opt.py:265-419; DIAYN
        trains the same two) on the device, from its HighPolicyValueModel / LoPolicyValueModel state_dicts with both
        critics: float32 master parameters, gradients, Adam's moments and a workspace per level.  lo / hi: dicts of the
        settings to change from ``SKPPO_LO`` / ``SKPPO_HI``.  `level` in the other skppo_* methods: ``_native.SKPPO_LO``
        = 0, ``SKPPO_HI`` = 1.  Separate from ``load_skills``: ``skppo_publish`` hands the parameters to the acting
        agent.  The inverse model's and the skill prior's updates are the ``diayn_*`` methods'."""
        self._pair_init("skppo", hi_state_dict, lo_state_dict, lo, hi)

    def skppo_publish(self):
        """Hand both learners' parameters to the acting agent: read them back and ``load_skills`` them with the
        handle's current skill_len, so the next ``collect_skills`` acts with them.  A loaded inverse model stays."""
        self._pair_publish("skppo")

    def skppo_update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        """update_parameters (main's _hier_policy_opt.py:254-263, train_lo and train_hi) on the records of the last
        ``collect_skills``: the high level first, then the low level, each epoch in the order of ``hppo_batch_indexes``
        from the caller's numpy Generator.  Returns the reference's logs under lo_* / hi_*: the low level's are means
        over all its minibatches (its lists start before the epoch loop), the high level's over the last epoch's."""
        return self._pair_update("skppo", epochs, batch_size, hi_epochs, hi_batch_size, rng)

    # ---- the Options agent
    def opppo_init(self, hi_state_dict, lo_state_dict, lo=None, hi=None):
        """The two learners of the Options agent (options/src/torch_ac/algos/_hier_policy_opt.py:208-381) on the device,
        from its HighPolicyValueModel / LoPolicyValueModel state_dicts with both critics: float32 master parameters,
        gradients, Adam's moments and a workspace per level.  lo / hi: dicts of the settings to change from ``OPPPO_LO``
        / ``OPPPO_HI``.  `level` in the other opppo_* methods: ``_native.OPPPO_LO`` = 0, ``OPPPO_HI`` = 1.  Separate from
        ``load_options``: ``opppo_publish`` hands the parameters to the acting agent."""
        self._pair_init("opppo", hi_state_dict, lo_state_dict, lo, hi)

    def opppo_publish(self):
        """Hand both learners' parameters to the acting agent: read them back and ``load_options`` them, so the next
        ``collect_options`` acts with them.  Like every ``load_options`` this drops the transitions the last collection
        left open, exactly as the torch example's reload does: an option still running when a collection ends is not
        trained on, its skill is picked again."""
        self._pair_publish("opppo")

    def opppo_update(self, epochs, batch_size, hi_epochs, hi_batch_size, rng):
        """update_hi_parameters, then update_lo_parameters (options/src/torch_ac/algos/_hier_policy_opt.py:208-381) on the
        records of the last ``collect_options``: the high level first and only if some transition closed (M >= 1; with
        M = 0 the hi_* logs are zeros), then the low level over N (T - 1) indexes, each epoch in the order of
        ``hppo_batch_indexes`` from the caller's numpy Generator.  Returns the reference's logs under lo_* / hi_*: the low
        level's are means over all its minibatches, the high level's over the last epoch's."""
        return self._pair_update("opppo", epochs, batch_size, hi_epochs, hi_batch_size, rng)

    # ------------------------------------------------------------------ DIAYN's inverse model and learned skill prior
    # the example's hyper-parameters (examples/skill_planner_ppo_torch.py; the reference does not clip this optimiser);
    # clip_eps, entropy_coef and value_loss_coef belong to zenv_ppo_config and are not used
    DIAYN = dict(lr=3e-4, adam_eps=1e-8, clip_eps=0.0, entropy_coef=0.0, value_loss_coef=0.0, max_grad_norm=math.inf,
                 max_batch=16384)
    DIAYN_PRIOR = dict(lr=1e-2, adam_eps=1e-8)

    def diayn_init(self, inverse_tensors, n_skills, prior_logits=None, prior=None, **hyper):
        """DIAYN's two remaining updates on the device (main/src/torch_ac/algos/_hier_policy_opt.py:421-464): a learner
        for InverseModel -- float32 master parameters, gradients, Adam's moments and a workspace -- from its tensors
        (``inverse_tensors_from_state_dict``; a state_dict is converted) and, with prior_logits (an array of n_skills
        logits), the learned skill prior with its own Adam state.  hyper: the settings to change from ``DIAYN``; prior:
        from ``DIAYN_PRIOR``.  Separate from ``load_skill_inverse``: ``diayn_publish`` hands the parameters to the acting
        discriminator."""
        if any(k in inverse_tensors for k in nat.SKILL_INVERSE_TENSORS):
            tensors = {k: _as_host_f32(v) for k, v in inverse_tensors.items()}
        else:
            tensors = inverse_tensors_from_state_dict(inverse_tensors, n_skills)
        S, h = (int(v) for v in np.asarray(tensors["comb_w2"]).shape)
        if S != int(n_skills):
            raise ValueError(f"combine_net.2 has {S} outputs, n_skills is {int(n_skills)}")
        F = int(np.asarray(tensors["zone_w1"]).shape[1]) - 8
        keys = diayn_state_dict_keys()
        shapes = inverse_tensor_shapes(h, S, F)
        w = nat.SkillInverseWeights(h_dim=h, n_skills=S, zone_feat=F, precision=nat.MLP_F32)
        keep = self._load_weights(w, list(keys), tensors, shapes)                 # alive across the call
        cfg = nat.PpoConfig(distributional_value=0, **dict(self.DIAYN, **hyper))
        check(lib().zenv_diayn_init(self._h, C.byref(w), C.byref(cfg)))
        del keep
        self._learners[("diayn", None)] = _Learner(self._h, _FAMILIES["diayn"], None, keys, shapes, cfg.lr, cfg.adam_eps)
        self._diayn_S = S
        if prior_logits is not None:
            logits = np.ascontiguousarray(_as_host_f32(prior_logits).reshape(-1))
            if logits.size != S:
                raise ValueError(f"prior_logits has {logits.size} entries, n_skills is {S}")
            p = dict(self.DIAYN_PRIOR, **(prior or {}))
            check(lib().zenv_diayn_prior_init(self._h, logits.ctypes.data, S, float(p["lr"]), float(p["adam_eps"])))

    def diayn_samples_on_device(self):
        """Compact the kept sample indexes of the last ``collect_skills`` on the device (``_native.F_DIAYN_SAMPLES``);
        returns their number.  Waits for the device."""
        n = C.c_int64()
        check(lib().zenv_diayn_samples(self._h, C.byref(n)))
        return n.value

    def diayn_samples(self):
        """int32 [count]: the sample indexes the inverse model trains on, ascending -- sample i = env * (T - 1) + f pairs
        the observation of frame f + 1 with the skill of frame f, kept where the mask of frame f + 1 is not 0
        (``diayn_kept_samples`` is the same rule on the host)."""
        count = self.diayn_samples_on_device()
        out = np.empty(count, np.int32)
        if count:
            check(lib().zenv_get(self._h, nat.F_DIAYN_SAMPLES, out.ctypes.data, 0))
        return out

    def diayn_update(self, epochs, batch_size, rng):
        """update_inverse_parameters (main's _hier_policy_opt.py:421-447) on the records of the last ``collect_skills``:
        every epoch a permutation of the kept samples from the caller's numpy Generator, cut into batches.  Stores and
        returns ``diayn_logs()``.  With no kept sample the inverse model is left alone and the loss is nan."""
        kept = self.diayn_samples()
        rows = None
        for e in range(int(epochs)):
            if not kept.size:
                break
            self.diayn_epoch(kept[hppo_batch_indexes(kept.size, rng)], batch_size)
            if e == 0:
                rows = self.diayn_stats()
        self._diayn_first_epoch = rows
        return self.diayn_logs()

    def diayn_logs(self):
        """{"loss": the mean cross-entropy over the first epoch's minibatches of the last ``diayn_update``}, as the
        reference logs it; nan when nothing was trained."""
        rows = getattr(self, "_diayn_first_epoch", None)
        return {"loss": float(np.asarray(rows, np.float64)[:, 0].mean()) if rows is not None and len(rows) else math.nan}

    def diayn_prior_update(self):
        """update_skill_prior (main's _hier_policy_opt.py:449-464): one Adam step of the skill prior's logits on the
        picks of the last ``collect_skills``.  Returns the new logits."""
        check(lib().zenv_diayn_prior_update(self._h))
        return self.diayn_prior_logits()

    def diayn_prior_logits(self):
        """float32 [S]: the learned skill prior's logits -- what the next ``collect_skills`` takes as
        ``skill_prior_logits``."""
        S = getattr(self, "_diayn_S", None) or getattr(self, "_skill_n", None) or 32
        out = np.zeros(32, np.float32)
        check(lib().zenv_diayn_prior_read(self._h, out.ctypes.data))
        return out[:S].copy()

    def diayn_set_prior_logits(self, logits):
        a = np.zeros(32, np.float32)
        v = _as_host_f32(logits).reshape(-1)
        a[:v.size] = v
        check(lib().zenv_diayn_prior_write(self._h, a.ctypes.data))

    def diayn_publish(self):
        """Hand the learner's parameters to the acting discriminator: read the 10 tensors back and
        ``load_skill_inverse`` them, so the next ``collect_skills`` takes its diversity reward from them."""
        self.load_skill_inverse(self.diayn_tensors())

    # ------------------------------------------------------------------ Zone-goals training experience
    def collect_hier(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """HierPolicyAlgo.collect_experiences (zone-goals/src/torch_ac/algos/_hier_policy_opt.py:9-171) on the device
        with the loaded hierarchical agent (``load_hier`` with both critics, ``enable_goals``).  Returns (lo, hi), the
        reference's lo_exps / hi_exps as numpy arrays:
          lo  [N, T-1, ...]: obs, zone_obs, goal, action, log_prob, value, advantage, returnn, reward (shaped),
              env_reward, mask -- reshape(N*(T-1), ...) is the reference's flat order
          hi  [M, ...] env-major: obs, zone_obs, action (int32), action_mask (bool [M, Z]), value, log_prob,
              advantage, returnn (hi_exps), reward and mask (what the GAE used); and count (int32 [N], rows of every
              env: sum = M)
        The transition an env has open at the end stays on the device and is the first of its next call."""
        T, M = self.collect_hier_on_device(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
        lo_l, hi_l = hier_experience_layout(self.num_envs, self.num_zones, self.zone_feat, T, M)
        lo = {name: a[:T - 1].swapaxes(0, 1) for name, a in self._download(lo_l).items()}
        hi = self._download(hi_l, skip=not M)
        hi["action_mask"] = hi["action_mask"].view(bool)
        hi["count"] = self.get(nat.F_HI_COUNT)
        return lo, hi

    def collect_hier_on_device(self, frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
        """The same collection, results left in the handle's device buffers (``hier_experience_layout`` names them).
        Returns (T, M)."""
        T, seed, index0, discount, gae_lambda = check_collect_hier_args(frames_per_proc, policy_seed, env_index0,
                                                                        discount, gae_lambda)
        m = C.c_int64(0)
        check(lib().zenv_collect_hier(self._h, T, seed, index0, discount, gae_lambda, C.byref(m)))
        self._exp_has_goals = True          # ZENV_F_LO_GOAL holds this collection's goals (render_experience's marks)
        return T, int(m.value)

    def sync(self):
        check(lib().zenv_sync(self._h))

    def done(self):
        """Non-blocking: has everything enqueued on the handle's stream finished (zenv_query)?"""
        rc = lib().zenv_query(self._h)
        if rc < 0:
            check(rc)
        return rc == 1

    # ------------------------------------------------------------------ multi-GPU: the one collective (native RCCL)
    def comm_init(self, rank, world, unique_id):
        """Join the job's RCCL communicator (collective: every rank calls it).  unique_id: the 128 bytes rank 0 got
        from ``comm_unique_id()``, handed over by the host (sharding.FileRendezvous)."""
        uid = bytes(unique_id)
        if len(uid) != nat.COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {nat.COMM_ID_BYTES} bytes")
        check(lib().zenv_comm_init(self._h, int(rank), int(world), uid))
        self.comm_rank, self.comm_world = int(rank), int(world)

    @property
    def comm_library(self):
        path = C.c_char_p()
        check(lib().zenv_comm_info(self._h, None, None, C.byref(path)))
        return (path.value or b"").decode()

    def allgather(self, field):
        """ncclAllGather of one per-env figure over the job's ranks -> [world * N] on the host, ordered by global env
        index (float64 fields arrive as float32, int32 fields as int32)."""
        world = getattr(self, "comm_world", 0)
        if not world:
            raise nat.ZenvError(nat.E_STATE, "comm_init first")
        dt = np.int32 if _FIELD_DTYPES[field] == np.int32 else np.float32
        out = np.empty(world * self.num_envs, dt)
        check(lib().zenv_allgather(self._h, int(field), out.ctypes.data, 0))
        return out

    def comm_barrier(self):
        check(lib().zenv_comm_barrier(self._h))

    def comm_max(self, value):
        v = C.c_double(float(value))
        check(lib().zenv_comm_allreduce_max(self._h, C.byref(v)))
        return v.value

    def set_stream(self, hip_stream=None):
        """Enqueue all further work on the caller's HIP stream (an integer hipStream_t, e.g.
        ``torch.cuda.current_stream().cuda_stream``); None = the handle's own stream again.  0 is the null
        stream (torch's default stream): it goes down as hipStreamLegacy, since NULL means "own stream"
        in the C ABI."""
        if hip_stream is None:
            ptr = None
        else:
            ptr = C.c_void_p(int(hip_stream) if int(hip_stream) else nat.HIP_STREAM_LEGACY)
        check(lib().zenv_set_stream(self._h, ptr))

    @property
    def step_count(self):
        return lib().zenv_step_count(self._h)

    # ------------------------------------------------------------------ results
    def _shape(self, field):
        N = self.num_envs
        if field == nat.F_OBS:
            return (N, nat.OBS_DIM)
        if field in (nat.F_ORDER_VAL, nat.F_ORDER_POS, nat.F_HIER_LOGITS):
            return (N, self.num_zones)
        if field == nat.F_SKILL_LOGITS:
            return (N, getattr(self, "_skill_n", 0))
        if field == nat.F_ZONE_OBS:
            return (N, self.num_zones, self.zone_feat)
        if field == nat.F_ORDER_ROWS:           # empty while order_rows() is off
            return (N if self.net_zone_feat != self.zone_feat else 0, self.num_zones, self.zone_feat + 1)
        if field in (nat.F_ACTIONS, nat.F_POLICY_MU, nat.F_POLICY_STD, nat.F_XY_GOAL, nat.F_XY_GOAL_MU,
                     nat.F_XY_GOAL_STD, nat.F_XY_BOOTSTRAP_GOAL):
            return (N, 2)
        return (N,)

    def get(self, field, out=None):
        if out is None:
            out = np.empty(self._shape(field), _FIELD_DTYPES[field])
        assert out.nbytes == lib().zenv_field_bytes(self._h, field)
        if field == nat.F_ORDER_ROWS and out.nbytes == 0:
            return out
        check(lib().zenv_get(self._h, field, out.ctypes.data, 0))
        return out

    def _download(self, layout, skip=False):
        """Every buffer of a layout (name -> (field id, shape, dtype)) as a new host array.  skip: the buffers hold
        nothing (no high-level row yet) -- the empty arrays, the library untouched."""
        out = {}
        for name, (field, shape, dtype) in layout.items():
            out[name] = a = np.empty(shape, dtype)
            if not skip:
                assert a.nbytes == lib().zenv_field_bytes(self._h, field)
                check(lib().zenv_get(self._h, field, a.ctypes.data, 0))
        return out

    def get_head(self, field, count, first_env=0):
        """Rows [first_env, first_env + count) of an env-major field (zenv_get_rows)."""
        shape = (int(count),) + tuple(self._shape(field)[1:])
        out = np.empty(shape, _FIELD_DTYPES[field])
        check(lib().zenv_get_rows(self._h, int(field), int(first_env), int(count), out.ctypes.data))
        return out

    def get_into_device(self, field, dst_ptr):
        check(lib().zenv_get(self._h, field, C.c_void_p(int(dst_ptr)), 1))

    def device_ptr(self, field):
        p = C.c_void_p()
        check(lib().zenv_device_ptr(self._h, field, C.byref(p)))
        return p.value

    def field_bytes(self, field):
        return lib().zenv_field_bytes(self._h, field)

    def observations(self):
        return self.get(nat.F_OBS), self.get(nat.F_ZONE_OBS)

    # ------------------------------------------------------------------ host-policy surface at PCIe rate
    def pinned_array(self, shape, dtype):
        """A numpy array in page-locked host memory (zenv_host_alloc): uploads from it / downloads into it are
        plain DMA.  The memory stays allocated until the process ends (arrays may outlive the env)."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        ptr = lib().zenv_host_alloc(max(nbytes, 1))
        if not ptr:
            raise nat.ZenvError(nat.E_HIP, "zenv_host_alloc failed")
        buf = (C.c_char * max(nbytes, 1)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def _own_pinned_array(self, shape, dtype):
        a = self.pinned_array(shape, dtype)
        if getattr(self, "_own_pinned", None) is None:
            self._own_pinned = []
        self._own_pinned.append(a)
        return a

    def results_into(self, fields, arrays):
        """Downloads of several fields, one synchronisation (zenv_get_many); arrays should be pinned_array()s."""
        f = (C.c_int * len(fields))(*[int(x) for x in fields])
        d = (C.c_void_p * len(fields))(*[a.ctypes.data for a in arrays])
        check(lib().zenv_get_many(self._h, len(fields), f, d))

    # results of up to this many bytes per step (16 envs of 25 zones: 10 KB) are worth keeping in host memory: two copy
    # enqueues cost more than the kernel writing them over the bus itself
    HOST_IO_MAX_BYTES = 256 << 10

    def host_io(self, enable=True):
        """zenv_host_io: the results slab and the action buffer in page-locked HOST memory that the kernels write / read
        themselves -- step_results() is then one launch and one wait, no upload, no download (for small batches driven
        by a host policy: ParallelEnv and the single-env gym surface switch it on by themselves, enable="if small":
        results of at most HOST_IO_MAX_BYTES per step)."""
        if enable == "if small":
            enable = lib().zenv_results_layout(self._h, (C.c_int64 * nat.N_RESULTS)()) <= self.HOST_IO_MAX_BYTES
        res, act = C.c_void_p(), C.c_void_p()
        check(lib().zenv_host_io(self._h, int(bool(enable)), C.byref(res), C.byref(act)))
        self._slab = self._slab_views = self._host_actions = None
        self._host_io = bool(enable)
        if enable:
            off = (C.c_int64 * nat.N_RESULTS)()
            total = lib().zenv_results_layout(self._h, off)
            self._host_actions = np.ctypeslib.as_array((C.c_float * (2 * self.num_envs)).from_address(act.value)).reshape(
                self.num_envs, 2)
            self._results_slab(raw=np.ctypeslib.as_array((C.c_uint8 * total).from_address(res.value)))
        return self

    def _results_slab(self, raw=None):
        """One page-locked host image of the handle's results slab, with typed views of its pieces."""
        if getattr(self, "_slab", None) is None:
            off = (C.c_int64 * nat.N_RESULTS)()
            total = lib().zenv_results_layout(self._h, off)
            if raw is None:
                raw = self._own_pinned_array((total,), np.uint8)
            N, Zn, F = self.num_envs, self.num_zones, self.zone_feat

            def view(i, count, dtype, shape):
                return raw[off[i]:off[i] + count * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
            self._slab = raw
            self._slab_views = (view(nat.RESULT_OBS, N * 8, np.float32, (N, 8)),
                                view(nat.RESULT_ZONE_OBS, N * Zn * F, np.float32, (N, Zn, F)),
                                view(nat.RESULT_REWARD, N, np.float32, (N,)),
                                view(nat.RESULT_DONE, N, np.uint8, (N,)).view(bool),
                                view(nat.RESULT_GOAL_MET, N, np.uint8, (N,)).view(bool),
                                view(nat.RESULT_EXCEPTION, N, np.uint8, (N,)).view(bool))
        return self._slab

    def step_results(self, actions=None, auto_reset=True, copy=True):
        """One env.step() of a host policy in ONE call (zenv_step_results): action upload, step, download of every
        per-step result, one synchronisation.  actions None: just the download (after reset()).  Returns
        (obs, zone_obs, reward, done, goal_met, exception); with copy=False the arrays are views of one page-locked
        buffer that the next call overwrites."""
        a = None
        if actions is not None:
            a = np.ascontiguousarray(actions, np.float32)
            if a.shape != (self.num_envs, 2):
                raise ValueError(f"actions must have shape ({self.num_envs}, 2)")
        if copy and self.num_envs * self.num_zones * self.zone_feat * 4 > (8 << 20):
            # a big batch whose caller wants its own arrays: download each field straight into them (a second pass
            # over tens of MB through the page-locked image would cost more than the extra synchronisations)
            if a is not None:
                self.step(a, auto_reset=auto_reset)
            return (self.get(nat.F_OBS), self.get(nat.F_ZONE_OBS), self.get(nat.F_REWARD),
                    self.get(nat.F_DONE).view(bool), self.get(nat.F_GOAL_MET).view(bool),
                    self.get(nat.F_EXCEPTION).view(bool))
        if getattr(self, "_host_io", False):      # the kernel reads the actions from, and writes the results to, host memory
            if a is not None:
                self._host_actions[...] = a
                check(lib().zenv_step_host(self._h, int(bool(auto_reset))))
            else:
                self.sync()
            return tuple(v.copy() for v in self._slab_views) if copy else self._slab_views
        slab = self._results_slab()
        check(lib().zenv_step_results(self._h, None if a is None else a.ctypes.data, int(bool(auto_reset)),
                                      slab.ctypes.data))
        return tuple(v.copy() for v in self._slab_views) if copy else self._slab_views

    def results(self):
        """(obs, zone_obs, reward, done, goal_met) of the last step, as host arrays."""
        return self.step_results(None)[:5]

    # ------------------------------------------------------------------ rendering (K18)
    def _render(self, source, env, first, count, width, height, view, robot_radius, marks_ptr, marks_on_device,
                dst_ptr, dst_on_device):
        """zenv_render with raw addresses (marks_ptr None: no marks)."""
        rc = nat.RenderConfig(int(width), int(height), int(source), int(env), float(view), float(robot_radius))
        check(lib().zenv_render(self._h, C.byref(rc), int(first), int(count),
                                None if marks_ptr is None else C.c_void_p(int(marks_ptr)), int(bool(marks_on_device)),
                                C.c_void_p(int(dst_ptr)), int(bool(dst_on_device))))

    def render_check(self, source, env, first, count, width, height, view, robot_radius):
        """zenv_render_check for this handle's config and batch: raises ZenvError(E_ARG) naming the argument."""
        rc = nat.RenderConfig(int(width), int(height), int(source), int(env), float(view), float(robot_radius))
        check(lib().zenv_render_check(C.byref(self.cfg), C.byref(rc), self.num_envs, int(first), int(count)))

    def _render_host(self, source, env, first, count, width, height, view, robot_radius, marks, out):
        self.render_check(source, env, first, count, width, height, view, robot_radius)
        shape = (int(count), int(height), int(width), 3)
        if out is None:
            out = np.empty(shape, np.uint8)
        elif out.dtype != np.uint8 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"out must be a contiguous uint8 array of shape {shape}")
        if marks is not None:
            marks = np.ascontiguousarray(marks, np.float32)
            if marks.shape != (int(count), 2):
                raise ValueError(f"marks must have shape ({int(count)}, 2)")
        self._render(source, env, first, count, width, height, view, robot_radius,
                     None if marks is None else marks.ctypes.data, False, out.ctypes.data, False)
        return out

    def _auto_marks(self, first, count):
        """What render() marks by itself: the goal zone's centre / 3 where ZENV_F_GOAL >= 0 -- a goal-conditioned
        handle's goal, a solver-ordered handle's next city of the route --, the current goal on an xy-goals handle,
        else nothing.  float32 [count, 2] with NaN rows for the envs without a goal, or None."""
        if self.field_bytes(nat.F_GOAL):
            goal = self.get_head(nat.F_GOAL, count, first)
            rows = self.get_head(nat.F_ZONE_OBS, count, first)
            marks = np.full((count, 2), np.nan, np.float32)
            idx = np.nonzero(goal >= 0)[0]
            picked = rows[idx, goal[idx]]
            drawn = picked[:, 5] != 0                   # (an idle env's all-zero observation has no goal to show)
            marks[idx[drawn]] = picked[drawn, :2]
            return marks
        if self.field_bytes(nat.F_XY_GOAL):
            goal = self.get_head(nat.F_XY_GOAL, count, first)
            age = self.get_head(nat.F_XY_GOAL_AGE, count, first)
            return np.where(age[:, None] >= 0, goal, np.float32(np.nan)).astype(np.float32)
        return None

    def render(self, first=0, count=None, width=100, height=100, view=1.25, robot_radius=0.1, marks="auto", out=None):
        """Envs first .. first + count - 1 (count None: to the last) as they were last observed, drawn top-down on the
        device (zenv_render, ZENV_RENDER_CURRENT): np.uint8 [count, height, width, 3], RGB, row 0 at +y.  The square
        shown is [-view, view]^2 in observation units (world / 3: the arena's extent 3 is 1.0).  marks: "auto" (see
        _auto_marks), None, or float32 [count, 2] points to ring (a NaN row: none).  What the reference's
        ZoneEnvBase.render(mode='rgb_array') is for, without MuJoCo's camera: DESIGN.md 4 K18 has the drawing rules."""
        first = int(first)
        count = self.num_envs - first if count is None else int(count)
        if isinstance(marks, str):
            if marks != "auto":
                raise ValueError('marks is "auto", None or an array [count, 2]')
            self.render_check(nat.RENDER_CURRENT, 0, first, count, width, height, view, robot_radius)
            marks = self._auto_marks(first, count)
        return self._render_host(nat.RENDER_CURRENT, 0, first, count, width, height, view, robot_radius, marks, out)

    def experience_frames(self):
        """T of the last collection (0: the handle holds no experience)."""
        return int(self.field_bytes(nat.F_EXP_OBS) // (self.num_envs * nat.OBS_DIM * 4))

    def render_experience(self, env, first=0, count=None, width=100, height=100, view=1.25, robot_radius=0.1,
                          marks="auto", out=None):
        """Frames first .. first + count - 1 (count None: to the last recorded) of ONE env of the last collection
        (any collect_*), drawn in a single launch from the time-major experience buffers (zenv_render,
        ZENV_RENDER_EXPERIENCE): np.uint8 [count, height, width, 3].  marks "auto": the goal the low level acted under
        (ZENV_F_LO_GOAL) where the last collection recorded one -- collect_hier, collect_xy -- else none."""
        first, T = int(first), self.experience_frames()
        if count is None:
            count = max(T - first, 1)           # (no experience: the library answers E_STATE)
        count = int(count)
        if isinstance(marks, str):
            if marks != "auto":
                raise ValueError('marks is "auto", None or an array [count, 2]')
            marks = None
            if T and getattr(self, "_exp_has_goals", False) and 0 <= first and first + count <= T \
                    and 0 <= int(env) < self.num_envs:
                marks = self.get(nat.F_LO_GOAL, np.empty((T, self.num_envs, 2), np.float32))[first:first + count, int(env)]
        return self._render_host(nat.RENDER_EXPERIENCE, env, first, count, width, height, view, robot_radius, marks, out)

    # ------------------------------------------------------------------ snapshots / debug
    def get_state(self):
        n = lib().zenv_state_bytes(self._h)
        buf = np.empty(n, np.uint8)
        check(lib().zenv_get_state(self._h, buf.ctypes.data, n))
        return buf

    def set_state(self, blob):
        b = np.ascontiguousarray(blob, np.uint8)
        check(lib().zenv_set_state(self._h, b.ctypes.data, b.nbytes))

    def debug_state(self):
        N, Z = self.num_envs, self.num_zones
        out = dict(qpos=np.empty((N, 3)), qvel=np.empty((N, 3)),
                   zone_state=np.empty((N, Z), np.int32), cooldown=np.empty((N, Z), np.int32),
                   steps=np.empty(N, np.int32))
        check(lib().zenv_debug_state(self._h, out["qpos"].ctypes.data, out["qvel"].ctypes.data,
                                     out["zone_state"].ctypes.data, out["cooldown"].ctypes.data,
                                     out["steps"].ctypes.data))
        return out


__all__ = ["ZoneVecEnv", "Config", "ZenvError", "config_for_id", "default_config",
           "sample_layout", "fixed_seed_sequence", "zone_feat"]
