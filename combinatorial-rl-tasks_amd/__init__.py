"""MI355X-native batched PointTSP / TimedTSP / ColourMatch env.step() path.

Layout of this package (only what the hot path needs):
  csrc/        HIP kernels (gfx950) + the C ABI of include/zenv.h + the host layout sampler
  _native.py   ctypes binding (no PyTorch, no CPU fallback)
  vec_env.py   ZoneVecEnv: N device-resident envs, struct-of-arrays results
  agents.py    the five agents' pure host functions: checkpoint -> tensors, tensor shapes, collector argument checks,
               experience layouts, the keys of each collector's episode logs (no shared library needed)
  envs/        host-side mirror of the reference interface (main/envs/*): registry ids,
               TSPEnv/TimedTSPEnv/ColourMatchEnv, FixedSeedsWrapper/ZoneWrapper, make_*_env
  penv.py      ParallelEnv-shaped vector env over one batched handle
  sharding.py  one-process-per-GPU env sharding + gather of episodic returns
"""
from ._native import (Config, ZenvError, E_ARG, E_HIP, E_STATE, E_LAYOUT, E_DONE, E_RANGE, TASK_TSP, TASK_TIMED_TSP, TASK_COLOUR_MATCH,
                      POLICY_UNIFORM, POLICY_GREEDY, POLICY_MLP_MEAN, POLICY_MLP_SAMPLE, POLICY_HIER_SAMPLE,
                      POLICY_HIER_MEAN, POLICY_SKILL_SAMPLE, POLICY_SKILL_MEAN, POLICY_OPTION_SAMPLE, POLICY_OPTION_MEAN,
                      POLICY_XY_SAMPLE, POLICY_XY_MEAN, F_OBS, F_ZONE_OBS, F_REWARD, F_DONE,
                      F_GOAL_MET, F_EP_RETURN, F_EP_LEN, F_LAST_RETURN, F_LAST_LEN, F_EPISODES,
                      F_VISIT_COUNT, F_SEED, F_ACTIONS, F_POLICY_MU, F_POLICY_STD, F_POLICY_VALUE,
                      F_SHAPED_REWARD, F_NEED_GOAL, F_AVAILABLE_GOALS, F_GOAL, F_ORDER_VAL, F_EXCEPTION, F_POLICY_VALUE_SIGMA,
                      F_HIER_LOGITS, F_HIER_VALUE, F_LO_GOAL, F_LO_ENV_REWARD, F_HI_OBS, F_HI_ZONE_OBS, F_HI_ACTION,
                      F_HI_ACTION_MASK, F_HI_VALUE, F_HI_LOG_PROB, F_HI_ADVANTAGE, F_HI_RETURN, F_HI_REWARD,
                      F_HI_MASK, F_HI_COUNT, F_SKILL, F_SKILL_AGE, F_SKILL_LOGITS, F_SKILL_VALUE, F_LO_SKILL,
                      F_LO_DIVERSITY, F_SKILL_BOOTSTRAP, F_OPTION_TERM_MU, F_OPTION_TERM_STD, F_OPTION_TERM_ACTION,
                      F_OPTION_TERM_PROB, F_OPTION_ENDED, F_LO_TERM_ACTION, F_LO_TERM_LOG_PROB, F_LO_OPTION_ENDED,
                      F_XY_GOAL, F_XY_GOAL_MU, F_XY_GOAL_STD, F_XY_VALUE, F_XY_GOAL_AGE, F_HI_GOAL, F_LO_GOAL_DIST,
                      F_XY_BOOTSTRAP_GOAL, F_PPO_STATS, PPO_PARAM, PPO_GRAD, PPO_EXP_AVG, PPO_EXP_AVG_SQ, PPO_STATS,
                      F_HPPO_LO_STATS, F_HPPO_HI_STATS, HPPO_LO, HPPO_HI, F_XYPPO_LO_STATS, F_XYPPO_HI_STATS, XYPPO_LO,
                      XYPPO_HI, F_SKPPO_LO_STATS, F_SKPPO_HI_STATS, SKPPO_LO, SKPPO_HI, F_OPPPO_LO_STATS,
                      F_OPPPO_HI_STATS, OPPPO_LO, OPPPO_HI, F_DIAYN_STATS, F_DIAYN_SAMPLES, F_ORDER_ROWS,
                      F_A2C_STATS, A2C_PARAM, A2C_GRAD, A2C_SQUARE_AVG, A2C_STATS,
                      RenderConfig, RENDER_CURRENT, RENDER_EXPERIENCE, DEVICE_RESTARTS, SAMPLE_STATUS_CAP,
                      SAMPLE_UNFINISHED, SAMPLE_SEED_RANGE, DET_OP_LOG, DET_OP_DIV, DET_OP_SQRT)
from .vec_env import (ZoneVecEnv, config_for_id, default_config, sample_layout, sample_layout_shared,
                      layout_thresholds, sample_layout_timed, det_ops,
                      fixed_seed_sequence, route_ranks, route_ranks_shared, zone_feat, hier_tensors_from_state_dicts,
                      hier_experience_layout, check_collect_hier_args, skill_tensors_from_state_dicts,
                      inverse_tensors_from_state_dict, skill_experience_layout, check_collect_skill_args,
                      skill_num_frames, option_tensor_shapes, option_tensors_from_state_dicts,
                      check_collect_option_args, option_experience_layout, xy_tensor_shapes,
                      xy_tensors_from_state_dicts, xy_experience_layout, check_collect_xy_args,
                      mlp_tensors_from_state_dict, ppo_state_dict_keys, ppo_batch_indexes, ppo_logs, a2c_logs,
                      hppo_state_dict_keys, hppo_batch_indexes, xyppo_state_dict_keys, skppo_state_dict_keys,
                      opppo_state_dict_keys, diayn_state_dict_keys, diayn_kept_samples,
                      EPISODE_LOG_KEYS, episode_log_columns, episode_log_keys, synthesize_stats)

__version__ = "0.1.0"
