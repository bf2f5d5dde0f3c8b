"""What the five device agents -- the flat actor-critic, Zone-goals, fixed-length skills / DIAYN, Options and xy-goals
-- need on the host before and after a call into the library: checkpoint (state_dict) -> named float32 tensors, the shape every
tensor must have, the argument rules of the collectors, the layout of the experience buffers they fill and the keys of
the per-episode logs each reports.

Pure functions of their arguments: numpy and the constants of ``_native`` only, never the shared library.
``vec_env`` imports every public name back, so ``vec_env.hier_tensors_from_state_dicts`` etc. stay valid.
"""
import numpy as np

from . import _native as nat


def _as_f32(v):
    """A torch tensor (any device) or anything numpy takes -> numpy float32."""
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32)


# zenv_hier_weights name -> state_dict key (zone-goals/src/hier_policy_value_models.py:19-86, env_model.py:48-116,
# policy_network.py:9-62): hi_model_state and lo_model_state of status.pt (zone-goals/src/utils/storage.py:57-61)
_HIER_ENC = {"zone_w1": "env_model.zone_net_.0.weight", "zone_b1": "env_model.zone_net_.0.bias",
             "zone_w2": "env_model.zone_net_.2.weight", "zone_b2": "env_model.zone_net_.2.bias",
             "zone_w3": "env_model.zone_net_.4.weight", "zone_b3": "env_model.zone_net_.4.bias",
             "comb_w": "env_model.combine_net_.weight", "comb_b": "env_model.combine_net_.bias"}
_HIER_CRITIC = {"critic_w1": "critic.0.weight", "critic_b1": "critic.0.bias",
                "critic_w2": "critic.2.weight", "critic_b2": "critic.2.bias"}
HIER_HI_KEYS = dict(_HIER_ENC, actor_w1="actor.0.weight", actor_b1="actor.0.bias", actor_w2="actor.2.weight",
                    actor_b2="actor.2.bias")
HIER_LO_KEYS = dict(_HIER_ENC, enc_w="actor.enc_.0.0.weight", enc_b="actor.enc_.0.0.bias", mu_w="actor.mu_.weight",
                    mu_b="actor.mu_.bias", std_w="actor.std_.weight", std_b="actor.std_.bias")
# zenv_skill_weights name -> state_dict key (main/src/hier_policy_value_models.py:19-76, env_model.py:81-117,
# policy_network.py:9-55): hi_model_state and lo_model_state of status.pt (main/scripts/train_skill_planner.py:152-163)
SKILL_HI_KEYS = dict(_HIER_ENC, enc_w="actor.enc_.0.0.weight", enc_b="actor.enc_.0.0.bias",
                     logit_w="actor.discrete_.0.weight", logit_b="actor.discrete_.0.bias")
SKILL_LO_KEYS = HIER_LO_KEYS
# zenv_xy_weights name -> state_dict key (xy-goals/src/hier_policy_value_models.py:19-72): the high level has the flat
# ACModel's keys with a plain critic, the low level the Zone-goals low level's
XY_HI_KEYS = dict(HIER_LO_KEYS)
XY_LO_KEYS = HIER_LO_KEYS
# zenv_skill_inverse_weights name -> state_dict key of InverseModel (main/src/inverse_model.py), DIAYN's discriminator
INVERSE_KEYS = {"zone_w1": "zone_net.0.weight", "zone_b1": "zone_net.0.bias", "zone_w2": "zone_net.2.weight",
                "zone_b2": "zone_net.2.bias", "zone_w3": "zone_net.4.weight", "zone_b3": "zone_net.4.bias",
                "comb_w1": "combine_net.0.weight", "comb_b1": "combine_net.0.bias",
                "comb_w2": "combine_net.2.weight", "comb_b2": "combine_net.2.bias"}


def _zone_net_shapes(h, x, F):
    """The zone net over rows of x own features + F zone features."""
    return {"zone_w1": (h, x + F), "zone_b1": (h,), "zone_w2": (h, h), "zone_b2": (h,), "zone_w3": (h, h),
            "zone_b3": (h,)}


def _enc_shapes(h, x, F):
    """ZoneEnvModel: the zone net and the layer that combines its pooled output with the x own features."""
    return dict(_zone_net_shapes(h, x, F), comb_w=(h, x + h), comb_b=(h,))


def _critic_shapes(h, x):
    return {"critic_w1": (h, x), "critic_b1": (h,), "critic_w2": (1, h), "critic_b2": (1,)}


def _gaussian_actor_shapes(h, x):
    return {"enc_w": (h, x), "enc_b": (h,), "mu_w": (2, h), "mu_b": (2,), "std_w": (2, h), "std_b": (2,)}


def _two_level_shapes(hi, lo):
    return dict({"hi_" + k: v for k, v in hi.items()}, **{"lo_" + k: v for k, v in lo.items()})


def mlp_tensor_shapes(h, F):
    """The shape of every zenv_mlp_weights tensor (both critic heads included) for hidden size h and zone rows of F
    features."""
    return dict(_enc_shapes(h, 8, F), **_gaussian_actor_shapes(h, h), **_critic_shapes(h, h),
                critic_sigma_w=(1, h), critic_sigma_b=(1,))


def hier_tensor_shapes(h, F):
    """The shape of every zenv_hier_weights tensor for hidden size h and zone rows of F features."""
    hi = dict(_enc_shapes(h, 8, F), actor_w1=(h, h + F), actor_b1=(h,), actor_w2=(1, h), actor_b2=(1,),
              **_critic_shapes(h, h))
    lo = dict(_enc_shapes(h, 10, F), **_gaussian_actor_shapes(h, h), **_critic_shapes(h, h))
    return _two_level_shapes(hi, lo)


def skill_tensor_shapes(h, S, F):
    """The shape of every zenv_skill_weights tensor for hidden size h, S skills and zone rows of F features."""
    hi = dict(_enc_shapes(h, 8, F), enc_w=(h, h), enc_b=(h,), logit_w=(S, h), logit_b=(S,), **_critic_shapes(h, h))
    lo = dict(_enc_shapes(h, 8 + S, F), **_gaussian_actor_shapes(h, h + S), **_critic_shapes(h, h + S))
    return _two_level_shapes(hi, lo)


def xy_tensor_shapes(h, F):
    """The shape of every zenv_xy_weights tensor for hidden size h and zone rows of F features."""
    hi = dict(_enc_shapes(h, 8, F), **_gaussian_actor_shapes(h, h), **_critic_shapes(h, h))
    lo = dict(_enc_shapes(h, 10, F), **_gaussian_actor_shapes(h, h), **_critic_shapes(h, h))
    return _two_level_shapes(hi, lo)


def option_tensor_shapes(h, S, F):
    """The shape of every zenv_option_weights tensor: ``skill_tensor_shapes`` with three rows in lo_mu_* / lo_std_*."""
    return dict(skill_tensor_shapes(h, S, F), lo_mu_w=(3, h), lo_mu_b=(3,), lo_std_w=(3, h), lo_std_b=(3,))


def inverse_tensor_shapes(h, S, F):
    """The shape of every zenv_skill_inverse_weights tensor for hidden size h, S skills and zone rows of F features."""
    return dict(_zone_net_shapes(h, 8, F), comb_w1=(h, 8 + h), comb_b1=(h,), comb_w2=(S, h), comb_b2=(S,))


def mlp_tensors_from_state_dict(sd):
    """ACModel.state_dict() (flat_model.py:24-52) -> the tensors load_mlp wants (numpy float32)."""
    names = dict(HIER_LO_KEYS)                                   # ZoneEnvModel + the Gaussian actor: the same keys
    if "critic.0.weight" in sd and "critic.2.weight" in sd:      # non-distributional critic, flat_model.py:43-47
        names.update(_HIER_CRITIC)
    elif "critic.0.weight" in sd and "critic_mu.weight" in sd:   # distributional_value=True, flat_model.py:35-41
        names.update({"critic_w1": "critic.0.weight", "critic_b1": "critic.0.bias",
                      "critic_w2": "critic_mu.weight", "critic_b2": "critic_mu.bias",
                      "critic_sigma_w": "critic_sigma.weight", "critic_sigma_b": "critic_sigma.bias"})
    return {k: _as_f32(sd[v]) for k, v in names.items()}


_DIST_CRITIC = {"critic_w1": "critic.0.weight", "critic_b1": "critic.0.bias",
                "critic_w2": "critic_mu.weight", "critic_b2": "critic_mu.bias",
                "critic_sigma_w": "critic_sigma.weight", "critic_sigma_b": "critic_sigma.bias"}


def ppo_state_dict_keys(distributional=False):
    """zenv_mlp_weights name -> ACModel state_dict key (flat_model.py:24-52) of every tensor the learner holds, in the
    arenas' order: 18 tensors, 20 with the distributional critic.  It is also ``ACModel.parameters()``' order, the
    order of torch Adam's state."""
    names = dict(HIER_LO_KEYS, **(_DIST_CRITIC if distributional else _HIER_CRITIC))
    order = nat.MLP_TENSORS + nat.MLP_CRITIC_TENSORS + (nat.MLP_SIGMA_TENSORS if distributional else ())
    return {name: names[name] for name in order}


def ppo_batch_indexes(num_frames, frames_per_proc, batch_num, rng):
    """The sample order of one epoch: _get_batches_starting_indexes (torch_ac/algos/ppo.py:157-183) for recurrence 1,
    before it is cut into batches.  A permutation of range(num_frames) from the caller's numpy Generator; on every odd
    call (batch_num) the indexes with (i + 1) % frames_per_proc == 0 are dropped and the shift is recurrence // 2 = 0
    -- the reference's quirk, kept."""
    indexes = rng.permutation(np.arange(0, num_frames, 1))
    if batch_num % 2 == 1:
        indexes = indexes[(indexes + 1) % frames_per_proc != 0]
        indexes = indexes + 0
    return np.ascontiguousarray(indexes, np.int32)


def hppo_state_dict_keys():
    """(hi, lo): zenv_hier_weights name -> state_dict key of every tensor the Zone-goals agent's two learners hold, in
    their arenas' order -- 16 tensors of HighPolicyValueModel, 18 of LoPolicyValueModel, critics included.  It is also
    each module's ``parameters()`` order, the order of torch Adam's state."""
    hi = dict(HIER_HI_KEYS, **_HIER_CRITIC)
    lo = dict(HIER_LO_KEYS, **_HIER_CRITIC)
    return ({name: hi[name[3:]] for name in nat.HIER_HI_TENSORS + nat.HIER_HI_CRITIC},
            {name: lo[name[3:]] for name in nat.HIER_LO_TENSORS + nat.HIER_LO_CRITIC})


def xyppo_state_dict_keys():
    """(hi, lo): zenv_xy_weights name -> state_dict key of every tensor the xy-goals agent's two learners hold, in their
    arenas' order -- 18 tensors each of HighPolicyValueModel and LoPolicyValueModel (xy-goals/src/
    hier_policy_value_models.py:19-72), critics included.  It is also each module's ``parameters()`` order, the order
    of torch Adam's state."""
    hi = dict(XY_HI_KEYS, **_HIER_CRITIC)
    lo = dict(XY_LO_KEYS, **_HIER_CRITIC)
    return ({name: hi[name[3:]] for name in nat.XY_HI_TENSORS + nat.XY_HI_CRITIC},
            {name: lo[name[3:]] for name in nat.XY_LO_TENSORS + nat.XY_LO_CRITIC})


def skppo_state_dict_keys():
    """(hi, lo): zenv_skill_weights name -> state_dict key of every tensor the fixed-length-skills agent's two learners
    hold, in their arenas' order -- 16 tensors of HighPolicyValueModel, 18 of LoPolicyValueModel (main/src/
    hier_policy_value_models.py:19-76), critics included.  It is also each module's ``parameters()`` order, the order
    of torch Adam's state."""
    hi = dict(SKILL_HI_KEYS, **_HIER_CRITIC)
    lo = dict(SKILL_LO_KEYS, **_HIER_CRITIC)
    return ({name: hi[name[3:]] for name in nat.SKILL_HI_TENSORS + nat.SKILL_HI_CRITIC},
            {name: lo[name[3:]] for name in nat.SKILL_LO_TENSORS + nat.SKILL_LO_CRITIC})


def opppo_state_dict_keys():
    """(hi, lo): zenv_option_weights name -> state_dict key of every tensor the Options agent's two learners hold, in
    their arenas' order -- 16 tensors of HighPolicyValueModel, 18 of LoPolicyValueModel (options/src/
    hier_policy_value_models.py), critics included; the names are the skill planner's, actor.mu_ / actor.std_ have three
    rows.  It is also each module's ``parameters()`` order, the order of torch Adam's state."""
    return skppo_state_dict_keys()


def diayn_state_dict_keys():
    """zenv_skill_inverse_weights name -> state_dict key of the 10 tensors DIAYN's inverse-model learner holds, in its
    arena's order: InverseModel's ``parameters()`` order (main/src/inverse_model.py), the order of torch Adam's state."""
    return {name: INVERSE_KEYS[name] for name in nat.SKILL_INVERSE_TENSORS}


def diayn_kept_samples(mask):
    """The sample indexes the inverse model trains on (main's _hier_policy_opt.py:193-199) from the collection's mask
    [N, T]: sample i = env * (T - 1) + f pairs the observation of frame f + 1 with the skill of frame f and is kept where
    mask[env, f + 1] is not 0.  Ascending int32: the reference's env-major order, what ``diayn_samples`` gives."""
    keep = np.asarray(mask)[:, 1:] != 0
    return np.flatnonzero(keep.reshape(-1)).astype(np.int32)


def hppo_batch_indexes(total, rng):
    """The sample order of one epoch of either level: _get_batches_starting_indexes_lo / _hi (zone-goals/src/torch_ac/
    algos/_hier_policy_opt.py:372-420) before it is cut into batches -- a plain permutation of range(total) from the
    caller's numpy Generator; no frame is dropped and nothing is shifted, unlike ``ppo_batch_indexes``."""
    return np.ascontiguousarray(rng.permutation(np.arange(0, total, 1)), np.int32)


def _two_level_tensors(hi_sd, lo_sd, hi_keys, lo_keys, sizes, want, describe):
    """The walk over a (hi_model_state, lo_model_state) pair: every key of hi_keys / lo_keys, the critics when present
    (critic.0 or critic.2), as numpy float32 under hi_<name> / lo_<name>.  sizes(out) reads the agent's sizes off the
    tensors, want(*sizes) is the shape table they must fit and describe.format(*sizes) names the sizes; a missing key
    or a misfit raises ValueError naming it."""
    out = {}
    for level, sd, keys in (("hi", hi_sd, hi_keys), ("lo", lo_sd, lo_keys)):
        names = dict(keys)
        if "critic.0.weight" in sd or "critic.2.weight" in sd:
            names.update(_HIER_CRITIC)
        for name, key in names.items():
            if key not in sd:
                raise ValueError(f"{level}_model_state has no {key!r} (needed for {level}_{name})")
            out[f"{level}_{name}"] = _as_f32(sd[key])
    n = sizes(out)
    shapes = want(*n)
    for name, a in out.items():
        if a.shape != shapes[name]:
            level, rest = name.split("_", 1)
            key = (hi_keys if level == "hi" else lo_keys).get(rest) or _HIER_CRITIC[rest]
            raise ValueError(f"{level}_model_state[{key!r}] has shape {tuple(a.shape)}, expected {shapes[name]} "
                             f"({describe.format(*n)})")
    return out


def _hier_sizes(out):
    """(h, F) of a Zone-goals checkpoint, -1 where the tensor that tells has the wrong rank."""
    h = out["hi_zone_b1"].shape[0] if out["hi_zone_b1"].ndim == 1 else -1
    F = out["hi_zone_w1"].shape[1] - 8 if out["hi_zone_w1"].ndim == 2 else -1
    return h, F


def _skill_sizes(out):
    """(h, S, F) of a skill-family checkpoint (actor.discrete_.0 is [S, h])."""
    logit = out["hi_logit_w"]
    h, S = (logit.shape[1], logit.shape[0]) if logit.ndim == 2 else (-1, -1)
    F = out["hi_zone_w1"].shape[1] - 8 if out["hi_zone_w1"].ndim == 2 else -1
    return h, S, F


def hier_tensors_from_state_dicts(hi_sd, lo_sd):
    """HighPolicyValueModel.state_dict() and LoPolicyValueModel.state_dict() -> the tensors ``ZoneVecEnv.load_hier``
    wants (numpy float32, names of ``_native.HIER_*``).  The critics are taken when present (critic.0 and critic.2
    both).  A missing key or a tensor whose shape does not fit the others raises ValueError naming it."""
    return _two_level_tensors(hi_sd, lo_sd, HIER_HI_KEYS, HIER_LO_KEYS, _hier_sizes, hier_tensor_shapes,
                              "hidden size {}, zone rows of {} features")


def xy_tensors_from_state_dicts(hi_sd, lo_sd):
    """HighPolicyValueModel.state_dict() and LoPolicyValueModel.state_dict() of the xy-goals agent (xy-goals/src/
    hier_policy_value_models.py) -> the tensors ``ZoneVecEnv.load_xy`` wants (numpy float32, names of ``_native.XY_*``).
    h and F come from the shapes; the critics are taken when present.  A Zone-goals checkpoint (an actor.0 / actor.2
    high level), a skill planner's or an Options agent's (actor.discrete_.0), a missing key or a tensor whose shape
    does not fit the others raises ValueError naming it."""
    if "actor.0.weight" in hi_sd or "actor.2.weight" in hi_sd:
        raise ValueError("hi_model_state has 'actor.0' / 'actor.2': a Zone-goals checkpoint (load it with "
                         "hier_tensors_from_state_dicts / load_hier), not an xy-goals agent's")
    if "actor.discrete_.0.weight" in hi_sd:
        raise ValueError("hi_model_state has 'actor.discrete_.0': a skill planner's or an Options agent's checkpoint "
                         "(load it with skill_tensors_from_state_dicts / load_skills or "
                         "option_tensors_from_state_dicts / load_options), not an xy-goals agent's")
    return _two_level_tensors(hi_sd, lo_sd, XY_HI_KEYS, XY_LO_KEYS, _hier_sizes, xy_tensor_shapes,
                              "hidden size {}, zone rows of {} features")


def option_tensors_from_state_dicts(hi_sd, lo_sd):
    """HighPolicyValueModel.state_dict() and LoPolicyValueModel.state_dict() of the variable-length Options agent
    (options/src/hier_policy_value_models.py) -> the tensors ``ZoneVecEnv.load_options`` wants (numpy float32, names of
    ``_native.SKILL_*``).  h, S and F come from the shapes; the critics are taken when present.  A skill planner's
    checkpoint (actor.mu_ / actor.std_ of two rows), a Zone-goals checkpoint, a missing key or a tensor whose shape
    does not fit the others raises ValueError naming it."""
    return _skill_family_tensors(hi_sd, lo_sd, 3)


def skill_tensors_from_state_dicts(hi_sd, lo_sd):
    """HighPolicyValueModel.state_dict() and LoPolicyValueModel.state_dict() of the fixed-length-skills agent -> the
    tensors ``ZoneVecEnv.load_skills`` wants (numpy float32, names of ``_native.SKILL_*``).  The hidden size h and the
    number of skills S come from the shapes (actor.discrete_.0 is [S, h]).  The critics are taken when present.  A
    Zone-goals checkpoint (the same hi_model_state / lo_model_state keys, an actor.0 / actor.2 high level), a missing
    key or a tensor whose shape does not fit the others raises ValueError naming it."""
    return _skill_family_tensors(hi_sd, lo_sd, 2)


def _skill_family_tensors(hi_sd, lo_sd, n_out):
    """n_out: the rows of the low level's actor.mu_ / actor.std_ -- 2: a skill planner's, 3: an Options agent's."""
    kind = "a skill planner's" if n_out == 2 else "an Options agent's"
    if "actor.0.weight" in hi_sd or "actor.2.weight" in hi_sd:
        raise ValueError("hi_model_state has 'actor.0' / 'actor.2': a Zone-goals checkpoint (load it with "
                         f"hier_tensors_from_state_dicts / load_hier), not {kind}")
    mu = lo_sd.get("actor.mu_.weight")
    if n_out == 3 and mu is not None and tuple(mu.shape)[:1] == (2,):
        raise ValueError("lo_model_state['actor.mu_.weight'] has 2 rows: a skill planner's checkpoint (load it with "
                         "skill_tensors_from_state_dicts / load_skills), not an Options agent's")
    if n_out == 2 and mu is not None and tuple(mu.shape)[:1] == (3,):
        raise ValueError("lo_model_state['actor.mu_.weight'] has 3 rows: an Options agent's checkpoint (load it with "
                         "option_tensors_from_state_dicts / load_options), not a skill planner's")
    return _two_level_tensors(hi_sd, lo_sd, SKILL_HI_KEYS, SKILL_LO_KEYS, _skill_sizes,
                              skill_tensor_shapes if n_out == 2 else option_tensor_shapes,
                              "hidden size {}, {} skills, zone rows of {} features")


def inverse_tensors_from_state_dict(state, n_skills):
    """InverseModel.state_dict() (main/src/inverse_model.py) -> the tensors ``ZoneVecEnv.load_skill_inverse`` wants
    (numpy float32, names of ``_native.SKILL_INVERSE_TENSORS``).  A dict with other keys (an ACModel, a policy's
    hi_model_state ...), a missing key, a tensor whose shape does not fit the others or a head of other than n_skills
    outputs raises ValueError naming it."""
    extra = sorted(k for k in state if k not in INVERSE_KEYS.values())
    if extra:
        raise ValueError(f"not an InverseModel state_dict: unexpected key {extra[0]!r}")
    out = {}
    for name, key in INVERSE_KEYS.items():
        if key not in state:
            raise ValueError(f"not an InverseModel state_dict: no {key!r}")
        out[name] = _as_f32(state[key])
    w1 = out["zone_w1"]
    h, F = (w1.shape[0], w1.shape[1] - 8) if w1.ndim == 2 else (-1, -1)
    want = inverse_tensor_shapes(h, int(n_skills), F)
    for name, a in out.items():
        if a.shape != want[name]:
            raise ValueError(f"InverseModel[{INVERSE_KEYS[name]!r}] has shape {tuple(a.shape)}, expected {want[name]} "
                             f"(hidden size {h}, {int(n_skills)} skills, zone rows of {F} features)")
    return out


def _check_collect_args(frames_per_proc, policy_seed, env_index0, discount, gae_lambda):
    """The rules every hierarchical collector shares: an integer T (not a bool), a discount and a lambda in [0, 1],
    non-negative 64-bit seeds.  Returns the normalised arguments."""
    if isinstance(frames_per_proc, bool) or int(frames_per_proc) != frames_per_proc:
        raise ValueError(f"frames_per_proc must be an integer, got {frames_per_proc!r}")
    for name, v in (("discount", discount), ("gae_lambda", gae_lambda)):
        if not (0.0 <= float(v) <= 1.0):
            raise ValueError(f"{name} must lie in [0, 1], got {v!r}")
    for name, v in (("policy_seed", policy_seed), ("env_index0", env_index0)):
        if int(v) != v or not (0 <= int(v) < 2 ** 64):
            raise ValueError(f"{name} must be an integer in [0, 2^64), got {v!r}")
    return int(frames_per_proc), int(policy_seed), int(env_index0), float(discount), float(gae_lambda)


def check_collect_hier_args(frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
    """What ``ZoneVecEnv.collect_hier`` checks before it calls into the library: T >= 2 frames (the low level hands
    out T - 1), a discount and a lambda in [0, 1], non-negative 64-bit seeds.  Returns the normalised arguments."""
    args = _check_collect_args(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
    if args[0] < 2:
        raise ValueError(f"frames_per_proc must be at least 2 (the low level hands out T - 1 frames), got {args[0]}")
    return args


def check_collect_option_args(frames_per_proc, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95):
    """What ``ZoneVecEnv.collect_options`` checks before it calls into the library: the rules of ``collect_hier`` -- T >= 2
    frames (the low level hands out T - 1), a discount and a lambda in [0, 1], non-negative 64-bit seeds.  Returns the
    normalised arguments."""
    return check_collect_hier_args(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)


def check_collect_skill_args(frames_per_proc, skill_len, policy_seed=1, env_index0=0, discount=0.99, gae_lambda=0.95,
                             diversity_coef=0.0, skill_prior_logits=None, n_skills=None, have_inverse=False):
    """What ``ZoneVecEnv.collect_skills`` checks before it calls into the library: T a positive multiple of skill_len
    (hrl_policy_planner.py:95), a discount and a lambda in [0, 1], a finite diversity_coef, non-negative 64-bit seeds;
    with an inverse model a finite prior of n_skills logits, without one diversity_coef = 0.  Returns the normalised
    arguments (the prior as a contiguous float32 array, or None)."""
    args = _check_collect_args(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
    T, L = args[0], int(skill_len)
    if T < 1 or L < 1 or T % L:
        raise ValueError(f"frames_per_proc must be a positive multiple of skill_len {L}, got {T}")
    if not np.isfinite(float(diversity_coef)):
        raise ValueError(f"diversity_coef must be finite, got {diversity_coef!r}")
    prior = None
    if have_inverse:
        if skill_prior_logits is None:
            raise ValueError("skill_prior_logits is needed with an inverse model (the diversity reward's prior)")
        prior = np.ascontiguousarray(_as_f32(skill_prior_logits)).reshape(-1)
        if n_skills is not None and prior.shape != (int(n_skills),):
            raise ValueError(f"skill_prior_logits must hold {int(n_skills)} logits, got shape {prior.shape}")
        if not np.all(np.isfinite(prior)):
            raise ValueError("skill_prior_logits must be finite")
    elif float(diversity_coef) != 0.0:
        raise ValueError("diversity_coef != 0 needs an inverse model (load_skill_inverse)")
    return args + (float(diversity_coef), prior)


def check_collect_xy_args(frames_per_proc, skill_len, policy_seed=0, env_index0=0, discount=0.99, gae_lambda=0.95):
    """What ``ZoneVecEnv.collect_xy`` checks before it calls into the library: T a positive multiple of skill_len
    (xy-goals' hrl_policy_planner.py:71-105 sizes its buffers by T // skill_len), a discount and a lambda in [0, 1],
    non-negative 64-bit seeds.  Returns the normalised arguments."""
    args = _check_collect_args(frames_per_proc, policy_seed, env_index0, discount, gae_lambda)
    T, L = args[0], int(skill_len)
    if T < 1 or L < 1 or T % L:
        raise ValueError(f"frames_per_proc must be a positive multiple of skill_len {L}, got {T}")
    return args


def _lo_rows(N, Z, F, T):
    """The per-frame buffers every collector fills, time-major [T, N, ...]: name -> (field id, shape, dtype)."""
    f32 = np.float32
    return {"obs": (nat.F_EXP_OBS, (T, N, 8), f32), "zone_obs": (nat.F_EXP_ZONE_OBS, (T, N, Z, F), f32),
            "action": (nat.F_EXP_ACTION, (T, N, 2), f32), "log_prob": (nat.F_EXP_LOG_PROB, (T, N, 2), f32),
            "value": (nat.F_EXP_VALUE, (T, N), f32), "reward": (nat.F_EXP_REWARD, (T, N), f32),
            "mask": (nat.F_EXP_MASK, (T, N), f32), "advantage": (nat.F_EXP_ADVANTAGE, (T, N), f32),
            "returnn": (nat.F_EXP_RETURN, (T, N), f32)}


def _hi_rows(Z, F, M):
    """The per-transition buffers every hierarchical collector fills, env-major [M, ...]."""
    f32 = np.float32
    return {"obs": (nat.F_HI_OBS, (M, 8), f32), "zone_obs": (nat.F_HI_ZONE_OBS, (M, Z, F), f32),
            "action": (nat.F_HI_ACTION, (M,), np.int32), "value": (nat.F_HI_VALUE, (M,), f32),
            "log_prob": (nat.F_HI_LOG_PROB, (M,), f32), "advantage": (nat.F_HI_ADVANTAGE, (M,), f32),
            "returnn": (nat.F_HI_RETURN, (M,), f32), "reward": (nat.F_HI_REWARD, (M,), f32),
            "mask": (nat.F_HI_MASK, (M,), f32)}


def hier_experience_layout(num_envs, num_zones, zone_feat, frames_per_proc, n_hi):
    """The buffers one ``collect_hier`` of T frames fills, as (lo, hi): name -> (field id, shape in memory, dtype).
    lo: time-major [T, N, ...] device buffers, handed out as [N, T-1, ...] views (the names of lo_exps in
    _hier_policy_opt.py:125-139, plus goal, reward (shaped), env_reward and mask).  hi: flat env-major [M, ...]
    (hi_exps, :142-161, plus each transition's reward and hi_mask), M = n_hi."""
    N, Z, F, T, M = int(num_envs), int(num_zones), int(zone_feat), int(frames_per_proc), int(n_hi)
    lo = dict(_lo_rows(N, Z, F, T), goal=(nat.F_LO_GOAL, (T, N, 2), np.float32),
              env_reward=(nat.F_LO_ENV_REWARD, (T, N), np.float32))
    hi = dict(_hi_rows(Z, F, M), action_mask=(nat.F_HI_ACTION_MASK, (M, Z), np.uint8))
    return lo, hi


def skill_experience_layout(num_envs, num_zones, zone_feat, frames_per_proc, skill_len):
    """The buffers one ``collect_skills`` of T frames fills, as (lo, hi): name -> (field id, shape in memory, dtype).
    lo: time-major [T, N, ...] device buffers, handed out as [N, T, ...] views (lo_exps of _hier_policy_opt.py:172-190:
    obs, zone_obs, skill, action, log_prob, value, advantage, returnn; plus reward = lo_reward, env_reward, diversity
    and mask).  hi: env-major [M, ...], M = N T / skill_len (hi_exps, :201-212, action = the skill; plus the window's
    reward and next_mask)."""
    N, Z, F, T, L = int(num_envs), int(num_zones), int(zone_feat), int(frames_per_proc), int(skill_len)
    lo = dict(_lo_rows(N, Z, F, T), skill=(nat.F_LO_SKILL, (T, N), np.int32),
              env_reward=(nat.F_LO_ENV_REWARD, (T, N), np.float32), diversity=(nat.F_LO_DIVERSITY, (T, N), np.float32))
    return lo, _hi_rows(Z, F, N * (T // L))


def option_experience_layout(num_envs, num_zones, zone_feat, frames_per_proc, n_hi):
    """The buffers one ``collect_options`` of T frames fills, as (lo, hi): name -> (field id, shape in memory, dtype).
    lo: time-major [T, N, ...] device buffers, handed out as [N, T-1, ...] views (lo_exps of options/src/torch_ac/algos/
    _hier_policy_opt.py:133-147: obs, zone_obs, skill, action, log_prob, value, advantage, returnn; plus reward =
    env_reward, mask and ended, the termination draw).  The reference's _action and lo_log_probs have three components:
    the first two are action / log_prob [T, N, 2], the third is term_action / term_log_prob [T, N], buffers of their
    own.  hi: flat env-major [M, ...] (hi_exps, :152-169, action = the skill; plus each transition's reward and
    hi_mask), M = n_hi."""
    N, Z, F, T, M = int(num_envs), int(num_zones), int(zone_feat), int(frames_per_proc), int(n_hi)
    f32 = np.float32
    lo = dict(_lo_rows(N, Z, F, T), skill=(nat.F_LO_SKILL, (T, N), np.int32),
              term_action=(nat.F_LO_TERM_ACTION, (T, N), f32), term_log_prob=(nat.F_LO_TERM_LOG_PROB, (T, N), f32),
              ended=(nat.F_LO_OPTION_ENDED, (T, N), np.uint8), env_reward=(nat.F_LO_ENV_REWARD, (T, N), f32))
    return lo, _hi_rows(Z, F, M)


def xy_experience_layout(num_envs, num_zones, zone_feat, frames_per_proc, skill_len):
    """The buffers one ``collect_xy`` of T frames fills, as (lo, hi): name -> (field id, shape in memory, dtype).
    lo: time-major [T, N, ...] device buffers, handed out as [N, T, ...] views (lo_exps of xy-goals/src/torch_ac/algos/
    _hier_policy_opt.py:145-158: obs, zone_obs, goal, action, log_prob, value, advantage, returnn; plus reward = the
    distance-to-goal reward, goal_dist, env_reward and mask).  hi: env-major [M, ...], M = N T / skill_len (hi_exps,
    :162-173: obs, zone_obs, goal, value, log_prob, advantage, returnn; plus the window's reward and next_mask).  The
    goal is continuous: there is no ``action`` among the high rows."""
    N, Z, F, T, L = int(num_envs), int(num_zones), int(zone_feat), int(frames_per_proc), int(skill_len)
    f32 = np.float32
    M = N * (T // L)
    lo = dict(_lo_rows(N, Z, F, T), goal=(nat.F_LO_GOAL, (T, N, 2), f32), goal_dist=(nat.F_LO_GOAL_DIST, (T, N), f32),
              env_reward=(nat.F_LO_ENV_REWARD, (T, N), f32))
    hi = {name: row for name, row in _hi_rows(Z, F, M).items() if name != "action"}
    hi["goal"] = (nat.F_HI_GOAL, (M, 2), f32)
    return lo, hi


def skill_num_frames(mask, skill_len):
    """logs['num_frames'] of _hier_policy_opt.py:104-124 from the recorded masks [T, N] (numpy or torch): every env's
    frames of a window up to and including its first done -- frame kL + i counts when mask[kL + 1 .. kL + i] are all
    1 (mask[t] = 1 - done of frame t - 1)."""
    T, N = mask.shape
    L = int(skill_len)
    if L == 1:
        return T * N
    m = mask.reshape(T // L, L, N)[:, 1:, :] != 0
    if not isinstance(m, np.ndarray):                           # torch
        return int(T // L * N + m.int().cumprod(dim=1).sum().item())
    return int(T // L * N + np.cumprod(m, axis=1).sum())


# The keys of the `logs` each collector's collect_experiences returns (main/src/torch_ac/algos/base.py:237-242; the
# four trees' _hier_policy_opt.py where they build `logs`), by the collector's name here.  ``ZoneVecEnv.episode_logs``
# adds ``env_per_episode`` to each.
_EPISODE_LOG_BASE = ("return_per_episode", "reshaped_return_per_episode", "num_frames_per_episode", "num_frames")
EPISODE_LOG_KEYS = {
    "collect": _EPISODE_LOG_BASE,
    "collect_hier": _EPISODE_LOG_BASE,
    "collect_options": _EPISODE_LOG_BASE,
    "collect_skills": _EPISODE_LOG_BASE + ("diversity_per_episode", "prediction_per_episode"),
    "collect_xy": _EPISODE_LOG_BASE + ("prediction_per_episode",),
}


def episode_log_columns(collector):
    """The ``_native.EPLOG_*`` columns of ``EPISODE_LOG_KEYS[collector]``, as the bit set zenv_episode_log reports."""
    return sum(1 << nat.EPLOG_KEYS.index(k) for k in EPISODE_LOG_KEYS[collector] if k != "num_frames")


def episode_log_keys(columns):
    """The per-episode keys of a zenv_episode_log column bit set, in column order."""
    return tuple(k for c, k in enumerate(nat.EPLOG_KEYS[:nat.EPLOG_ENV]) if columns >> c & 1)


def synthesize_stats(stats):
    """utils.synthesize (main/src/utils/other.py) from zenv_episode_log_stats' (count, sum, sum of squares about the
    mean, min, max): mean / std / min / max, std the population's as numpy.std."""
    count, total, ssq, lo, hi = (float(v) for v in stats)
    return {"mean": total / count, "std": (ssq / count) ** 0.5, "min": lo, "max": hi}


def episode_log_history(stats, num_frames, keys=("return_per_episode", "num_frames_per_episode")):
    """The flat entries a training loop keeps of one collection's logs, named as train_ppo.py / train_skill_planner.py
    name their columns: ``return_mean`` / ``_std`` / ``_min`` / ``_max`` and the same for ``num_frames_per_episode``
    (``num_frames_*``) and any further key (``diversity_*``) out of ``episode_log_stats()``, and ``num_frames``, the
    frames of the call."""
    out = {}
    for key in keys:
        name = {"num_frames_per_episode": "num_frames"}.get(key, key[:-len("_per_episode")])
        out.update({f"{name}_{k}": v for k, v in stats[key].items()})
    out["num_frames"] = int(num_frames)
    return out
