"""The reference's evaluation protocol (main/scripts/evaluate.py:22-25,47-78) on one device.

100 maps (env seeds 1000000..1000099) x 5 runs per map, undiscounted episodic return,
result layout ``{"return": [[r_run0..r_run4] for each map]}`` -- but all maps and runs are
stepped together as one batch of n_maps*n_runs envs instead of 500 sequential episodes.
``evaluate_zone_hrl`` does the same for zone-goals/scripts/evaluate_zone_hrl.py with the Zone-goals hierarchical agent,
``evaluate_hier`` for main/scripts/evaluate_hier.py with the fixed-length-skills agent, ``evaluate_options`` for
options/scripts/evaluate_hier.py with the variable-length Options agent, ``evaluate_xy_hrl`` for
xy-goals/scripts/evaluate_xy_hrl.py with the xy-goals agent.
"""
import pickle

import numpy as np

from . import _native as nat
from .vec_env import ZoneVecEnv, config_for_id

EVAL_SEED0 = 1000000     # evaluate.py:47


def load_model_state(model_dir):
    """``utils.get_model_state(model_dir)`` (main/src/utils/storage.py:36-52): the ``model_state`` entry of the
    ``status.pt`` a reference training run leaves in its model directory (train_ppo.py:201-208).  ``model_dir`` may also
    name the file itself.  The checkpoint holds only tensors and plain Python objects, so torch loads it without any of
    the reference's modules."""
    import os
    import torch
    path = model_dir if os.path.isfile(model_dir) else os.path.join(model_dir, "status.pt")
    status = torch.load(path, map_location="cpu", weights_only=True)
    if "model_state" not in status:
        raise KeyError(f"{path} has no 'model_state' (keys: {sorted(status)})")
    return status["model_state"]


def evaluate(env_id, policy, n_maps=100, n_runs_per_map=5, env_seed0=EVAL_SEED0, device=0,
             policy_seed=0, pkl_path=None, max_steps=None, argmax=False, precision="f32"):
    """policy: ZENV_POLICY_* (on-device scripted policy), a callable
    ``policy(obs (B,8) float32, zone_obs (B,Z,F) float32) -> actions (B,2)`` running on the host
    (e.g. the reference's ``Agent.get_actions`` behind a small adapter), an ACModel ``state_dict``
    (main/src/flat_model.py:24-52 names; what ``utils.Agent`` loads, main/src/utils/agent.py:15-28) or the path of
    a reference model directory / ``status.pt`` (``load_model_state``): the actor
    then runs on the device (``csrc/mlp_policy.hip``), ``dist.sample()`` per step as ``Agent.get_actions`` does
    (agent.py:41-44), or the mean with ``argmax=True``; ``precision`` "f32" (default: the reference's own arithmetic,
    actions within 1e-5 of its torch float32 modules), "f16x3" (within 3e-6 as well, a third of the time on batches of
    2 048 envs and more -- smaller ones run the float32 vector kernel either way) "bf16" (the MFMA kernels, 8x faster) or "f16" (the same kernels on
    float16 operands: within 1e-3, float16's range guarded).

    env_id: a registry id or a Config.  An id whose class is ``TSPOrderEnv`` ("PointTSP-v2", the results table's
    "Solver" row) is the task env of its config with ``enable_order()`` and ``order_rows()`` on: the network -- and a
    host policy -- sees the reference's (Z, 7) rows (main/envs/TSP_order_env.py:37-47), so the state_dict's
    ``zone_net_.0.weight`` is [h, 15].

    Returns ``{"return": [[...]], "length": [[...]], "goal_met": [[...]]}``."""
    base_id = order_base_id(env_id) if isinstance(env_id, str) else None
    cfg = config_for_id(base_id or env_id) if isinstance(env_id, str) else env_id
    if isinstance(policy, str):
        policy = load_model_state(policy)
    tensors = None
    if isinstance(policy, dict):
        from .vec_env import mlp_tensors_from_state_dict
        tensors = mlp_tensors_from_state_dict(policy)
        policy = nat.POLICY_MLP_MEAN if argmax else nat.POLICY_MLP_SAMPLE
    o = zo = None                          # a host policy's next input: the last step's observations

    def prepare(env):                      # routes ride in the bank: before it is built
        if base_id:
            env.enable_order()
            env.order_rows()

    def setup(env):
        nonlocal o, zo
        env.reset()
        if tensors is not None:
            env.load_mlp(tensors, precision=precision)
        if callable(policy):
            o, zo = env.step_results(None, copy=False)[:2]
            if base_id:
                zo = env.get(nat.F_ORDER_ROWS)

    def host_step(env):                    # one upload, one launch, one download, one synchronisation per step
        nonlocal o, zo
        o, zo, _, d, g, _ = env.step_results(np.asarray(policy(o, zo), np.float32), auto_reset=False, copy=False)
        if base_id:
            zo = env.get(nat.F_ORDER_ROWS)
        return d, g

    return _run_batched(cfg, n_maps, n_runs_per_map, env_seed0, device, max_steps, pkl_path, setup,
                        host_step if callable(policy) else _device_step(policy, policy_seed), prepare)


def order_base_id(env_id):
    """The registry id of the plain task env a solver-ordered id is built on -- same config, class ``TSPEnv`` --
    ("PointTSP-v2" -> "PointTSP-v0"), or None for an id whose class is not ``TSPOrderEnv`` and for a Config."""
    from .envs.registry import REGISTRY
    from .envs.zone_envs import TSPEnv, TSPOrderEnv
    if not isinstance(env_id, str):                          # a Config: the caller switches variants on himself
        return None
    cls, config = REGISTRY.get(env_id, (None, None))
    if cls is None or not issubclass(cls, TSPOrderEnv):
        return None
    for other, (c, conf) in REGISTRY.items():
        if c is TSPEnv and conf is config:
            return other
    raise RuntimeError(f"{env_id}: no plain TSP id with the same config")


def _device_step(policy, policy_seed):
    """step(env) of ``_run_batched`` for an on-device policy: pick the actions, step, fetch the flags."""
    def step(env):
        env.policy(int(policy), policy_seed=policy_seed)
        env.step(None, auto_reset=False)
        return env.step_results(None, copy=False)[3:5]
    return step


def _run_batched(cfg, n_maps, n_runs_per_map, env_seed0, device, max_steps, pkl_path, setup, step, prepare=None):
    """The protocol all evaluators share: one env per map and run (the maps of env seeds env_seed0 ..), every episode
    run once, to the horizon or until all are done.  setup(env) switches the variant on, resets and loads the agent;
    step(env) advances every env by one step without auto-reset and returns that step's (done, goal_met);
    prepare(env), when given, runs before the bank is built (a variant whose routes ride in it).  Returns
    ``{"return": [[...]], "length": [[...]], "goal_met": [[...]]}``, [map][run], and writes ``{"return": ...}`` to
    ``pkl_path`` as the reference's scripts do (evaluate.py:76-78)."""
    n = n_maps * n_runs_per_map
    env = ZoneVecEnv(cfg, n, device=device)
    try:
        if prepare is not None:
            prepare(env)
        env.build_bank(env_seed0, n_maps)
        env.schedule_sequential(first=np.repeat(np.arange(n_maps, dtype=np.int32), n_runs_per_map), stride=0)
        setup(env)
        goal = np.zeros(n, bool)
        for t in range(cfg.num_steps if max_steps is None else max_steps):
            d, g = step(env)
            goal |= g
            if d.all():                    # every episode finished (evaluate.py:64-72)
                break
        out = {
            "return": env.get(nat.F_LAST_RETURN).reshape(n_maps, n_runs_per_map).tolist(),
            "length": env.get(nat.F_LAST_LEN).reshape(n_maps, n_runs_per_map).tolist(),
            "goal_met": goal.reshape(n_maps, n_runs_per_map).tolist(),
        }
    finally:
        env.close()
    if pkl_path:
        with open(pkl_path, "wb") as f:
            pickle.dump({"return": out["return"]}, f)
    return out


# the goal-conditioned ids (zone-goals/envs/__init__.py) are the task envs of these ids with zenv_goal_enable on
HIER_BASE_IDS = {"PointTSP-v3": "PointTSP-v0", "PointTTSP-v3": "PointTTSP-v0", "ColourMatch-v3": "ColourMatch-v0"}


def load_hier_model_state(model):
    """``(utils.get_hi_model_state(model_dir), utils.get_lo_model_state(model_dir))`` (zone-goals/src/utils/
    storage.py:57-61): the ``hi_model_state`` / ``lo_model_state`` entries of a model directory's ``status.pt`` (or of
    that file named directly)."""
    import os
    import torch
    path = model if os.path.isfile(model) else os.path.join(model, "status.pt")
    status = torch.load(path, map_location="cpu", weights_only=True)
    for k in ("hi_model_state", "lo_model_state"):
        if k not in status:
            raise KeyError(f"{path} has no {k!r} (keys: {sorted(status)})")
    return status["hi_model_state"], status["lo_model_state"]


def evaluate_zone_hrl(env_id, model, n_maps=100, n_runs_per_map=5, env_seed0=EVAL_SEED0, policy_seed=0, argmax=False,
                      pkl_path=None, device=0, max_steps=None):
    """The protocol of zone-goals/scripts/evaluate_zone_hrl.py (100 maps x 5 runs, env seeds 1000000.., undiscounted
    return) with the Zone-goals hierarchical agent on the device, every map and run stepped together as one batch.
    Per step (:56-64): an env without a goal gets one from HighPolicyValueModel (a draw from Categorical over the
    available zones, or the argmax with ``argmax=True``), then LoPolicyValueModel's action (``dist.sample()``, or mu).

    env_id: "PointTSP-v3", "PointTTSP-v3", "ColourMatch-v3" (or any registry id / Config: goals are switched on);
    model: a model directory, its ``status.pt``, or a ``(hi_state_dict, lo_state_dict)`` pair.
    Returns ``{"return": [[...]], "length": [[...]], "goal_met": [[...]]}`` as ``evaluate`` does and writes
    ``{"return": ...}`` to ``pkl_path`` (evaluate_zone_hrl.py:44, :77-79)."""
    from .vec_env import hier_tensors_from_state_dicts
    if isinstance(env_id, str):
        cfg = config_for_id(HIER_BASE_IDS.get(env_id, env_id))
    else:
        cfg = env_id
    hi_sd, lo_sd = load_hier_model_state(model) if isinstance(model, str) else model
    tensors = hier_tensors_from_state_dicts(hi_sd, lo_sd)

    def setup(env):
        env.enable_goals()
        env.reset()
        env.load_hier(tensors)

    return _run_batched(cfg, n_maps, n_runs_per_map, env_seed0, device, max_steps, pkl_path, setup,
                        _device_step(nat.POLICY_HIER_MEAN if argmax else nat.POLICY_HIER_SAMPLE, policy_seed))


def evaluate_hier(env_id, model, n_maps=100, n_runs_per_map=5, n_skills=None, skill_len=200, policy_seed=0,
                  argmax=False, pkl_path=None, device=0, max_steps=None, env_seed0=EVAL_SEED0):
    """The protocol of main/scripts/evaluate_hier.py (100 maps x 5 runs, env seeds 1000000.., undiscounted return)
    with the fixed-length-skills agent on the device, every map and run stepped together as one batch.  Per step
    (:63-67): every ``skill_len`` steps from the episode's reset HighPolicyValueModel picks a skill (a draw from
    Categorical, or the argmax with ``argmax=True``), then LoPolicyValueModel acts under it (``dist.sample()``, or mu).

    env_id: a registry id ("PointTSP-v0" ...: make_fixed_env(hier=True) is the plain task env) or a Config;
    model: a model directory, its ``status.pt``, or a ``(hi_state_dict, lo_state_dict)`` pair; n_skills: checked
    against the checkpoint's when given (evaluate_hier.py builds HierAgent with 5).
    Returns ``{"return": [[...]], "length": [[...]], "goal_met": [[...]]}`` as ``evaluate`` does and writes
    ``{"return": ...}`` to ``pkl_path`` (evaluate_hier.py:45, :80-83)."""
    from .vec_env import skill_tensors_from_state_dicts
    cfg = config_for_id(env_id) if isinstance(env_id, str) else env_id
    hi_sd, lo_sd = load_hier_model_state(model) if isinstance(model, str) else model
    tensors = skill_tensors_from_state_dicts(hi_sd, lo_sd)
    S = tensors["hi_logit_w"].shape[0]
    if n_skills is not None and n_skills != S:
        raise ValueError(f"n_skills={n_skills}, but the checkpoint's high level has {S} skills")

    def setup(env):
        env.reset()
        env.load_skills(tensors, skill_len=skill_len)

    return _run_batched(cfg, n_maps, n_runs_per_map, env_seed0, device, max_steps, pkl_path, setup,
                        _device_step(nat.POLICY_SKILL_MEAN if argmax else nat.POLICY_SKILL_SAMPLE, policy_seed))


def evaluate_options(env_id, model, n_maps=100, n_runs_per_map=1, n_skills=None, policy_seed=0, argmax=False,
                     pkl_path=None, device=0, max_steps=None, env_seed0=EVAL_SEED0):
    """The protocol of options/scripts/evaluate_hier.py (100 maps x 1 run, env seeds 1000000.., undiscounted return)
    with the variable-length Options agent on the device, every map and run stepped together as one batch.  Per step
    (:63-75): an env without a skill -- the episode's first step, or the last option ended -- has HighPolicyValueModel
    pick one (a draw from Categorical, or the argmax with ``argmax=True``); LoPolicyValueModel acts under it
    (``dist.sample()``, or mu); the option ends with probability sigmoid(4 a_2 - 3), a_2 the sample's third component
    (with ``argmax=True``: iff that probability of mu_2 exceeds 0.5).

    env_id, model, n_skills: as ``evaluate_hier`` (the script builds HierAgent with 5 skills).
    Returns ``{"return": [[...]], "length": [[...]], "goal_met": [[...]], "terminations": [[...]]}`` -- terminations:
    how many options ended during the episode -- and writes ``{"return": ...}`` to ``pkl_path`` (:45, :88-90)."""
    from .vec_env import option_tensors_from_state_dicts
    cfg = config_for_id(env_id) if isinstance(env_id, str) else env_id
    hi_sd, lo_sd = load_hier_model_state(model) if isinstance(model, str) else model
    tensors = option_tensors_from_state_dicts(hi_sd, lo_sd)
    S = tensors["hi_logit_w"].shape[0]
    if n_skills is not None and n_skills != S:
        raise ValueError(f"n_skills={n_skills}, but the checkpoint's high level has {S} skills")
    policy = nat.POLICY_OPTION_MEAN if argmax else nat.POLICY_OPTION_SAMPLE
    ended = np.zeros(n_maps * n_runs_per_map, np.int64)

    def setup(env):
        env.reset()
        env.load_options(tensors)

    def step(env):
        nonlocal ended
        env.policy(policy, policy_seed=policy_seed)
        ended += env.get(nat.F_OPTION_ENDED)      # 0 for an env that has finished
        env.step(None, auto_reset=False)
        return env.step_results(None, copy=False)[3:5]

    out = _run_batched(cfg, n_maps, n_runs_per_map, env_seed0, device, max_steps, pkl_path, setup, step)
    out["terminations"] = ended.reshape(n_maps, n_runs_per_map).tolist()
    return out


def evaluate_xy_hrl(env_id, model, n_maps=100, n_runs_per_map=5, skill_len=200, policy_seed=0, argmax=False,
                    pkl_path=None, device=0, max_steps=None, env_seed0=EVAL_SEED0):
    """The protocol of xy-goals/scripts/evaluate_xy_hrl.py (100 maps x 5 runs, env seeds 1000000.., undiscounted
    return) with the xy-goals hierarchical agent on the device, every map and run stepped together as one batch.  Per
    step (:62-70): every ``skill_len`` steps from the episode's reset HighPolicyValueModel draws a goal in the plane
    from its Normal (or takes the mean with ``argmax=True``), then LoPolicyValueModel acts under it (``dist.sample()``,
    or mu).

    env_id: a registry id ("PointTSP-v0" ...: make_fixed_env(hier=True) is the plain task env) or a Config;
    model: a model directory, its ``status.pt``, or a ``(hi_state_dict, lo_state_dict)`` pair.
    Returns ``{"return": [[...]], "length": [[...]], "goal_met": [[...]]}`` as ``evaluate`` does and writes
    ``{"return": ...}`` to ``pkl_path`` (evaluate_xy_hrl.py:44, :79-81)."""
    from .vec_env import xy_tensors_from_state_dicts
    cfg = config_for_id(env_id) if isinstance(env_id, str) else env_id
    hi_sd, lo_sd = load_hier_model_state(model) if isinstance(model, str) else model
    tensors = xy_tensors_from_state_dicts(hi_sd, lo_sd)

    def setup(env):
        env.reset()
        env.load_xy(tensors, skill_len=skill_len)

    return _run_batched(cfg, n_maps, n_runs_per_map, env_seed0, device, max_steps, pkl_path, setup,
                        _device_step(nat.POLICY_XY_MEAN if argmax else nat.POLICY_XY_SAMPLE, policy_seed))
