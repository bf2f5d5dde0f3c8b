"""ctypes binding of libzenv_hip.so (include/zenv.h).  No PyTorch, no CPU fallback.

The library is built in-tree by ``build.py`` (hipcc, gfx950).  Importing this module fails
loudly when the shared object is missing; every compute call fails with ``ZenvError`` when
no MI355X is present.
"""
import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZENV_LIB_PATH") or os.path.join(_HERE, "lib", "libzenv_hip.so")   # env: diagnostic builds

MAX_ZONES = 32
OBS_DIM = 8

TASK_TSP, TASK_TIMED_TSP, TASK_COLOUR_MATCH = 0, 1, 2
POLICY_UNIFORM, POLICY_GREEDY, POLICY_MLP_MEAN, POLICY_MLP_SAMPLE = 0, 1, 2, 3
POLICY_HIER_SAMPLE, POLICY_HIER_MEAN = 4, 5     # the Zone-goals hierarchical agent (zenv_hier_load)
POLICY_SKILL_SAMPLE, POLICY_SKILL_MEAN = 6, 7   # the fixed-length-skills agent (zenv_skill_load)
POLICY_OPTION_SAMPLE, POLICY_OPTION_MEAN = 8, 9  # the variable-length Options agent (zenv_option_load)
POLICY_XY_SAMPLE, POLICY_XY_MEAN = 12, 13       # the xy-goals agent (zenv_xy_load); 10 and 11 stay unknown policies
MAX_SKILLS = 32
KERNEL_LANE_PER_ENV, KERNEL_WAVE_PER_ENV = 0, 1
HIP_STREAM_LEGACY = 1       # hipStreamLegacy: the null stream as an explicit handle (hip_runtime_api.h)
ROLLOUT_UNFUSED = 1
ROLLOUT_PER_STEP = 2
ROLLOUT_ASYNC = 4
ROLLOUT_CHUNK = 256
COMM_ID_BYTES = 128
ORDER_FRESH_FIRST_OBS = 1
CHUNK_NO_RESET, CHUNK_RESET_EVERY, CHUNK_RESET_LAST = 0, 1, 2

E_ARG, E_HIP, E_STATE, E_LAYOUT, E_DONE, E_RANGE = -1, -2, -3, -4, -5, -6

(F_OBS, F_ZONE_OBS, F_REWARD, F_DONE, F_GOAL_MET, F_EP_RETURN, F_EP_LEN, F_LAST_RETURN,
 F_LAST_LEN, F_EPISODES, F_VISIT_COUNT, F_SEED, F_ACTIONS, F_POLICY_MU, F_POLICY_STD, F_POLICY_VALUE,
 F_SHAPED_REWARD, F_NEED_GOAL, F_AVAILABLE_GOALS, F_GOAL,
 F_EXP_OBS, F_EXP_ZONE_OBS, F_EXP_ACTION, F_EXP_LOG_PROB, F_EXP_VALUE, F_EXP_REWARD, F_EXP_MASK,
 F_EXP_ADVANTAGE, F_EXP_RETURN, F_ORDER_VAL, F_EXCEPTION, F_POLICY_VALUE_SIGMA, F_ORDER_POS,
 F_CHUNK_REWARD, F_CHUNK_DONE, F_CHUNK_ACTIONS, F_HIER_LOGITS, F_HIER_VALUE,
 F_LO_GOAL, F_LO_ENV_REWARD, F_HI_OBS, F_HI_ZONE_OBS, F_HI_ACTION, F_HI_ACTION_MASK, F_HI_VALUE, F_HI_LOG_PROB,
 F_HI_ADVANTAGE, F_HI_RETURN, F_HI_REWARD, F_HI_MASK, F_HI_COUNT,
 F_SKILL, F_SKILL_AGE, F_SKILL_LOGITS, F_SKILL_VALUE,
 F_LO_SKILL, F_LO_DIVERSITY, F_SKILL_BOOTSTRAP,
 F_OPTION_TERM_MU, F_OPTION_TERM_STD, F_OPTION_TERM_ACTION, F_OPTION_TERM_PROB, F_OPTION_ENDED,
 F_LO_TERM_ACTION, F_LO_TERM_LOG_PROB, F_LO_OPTION_ENDED,
 F_XY_GOAL, F_XY_GOAL_MU, F_XY_GOAL_STD, F_XY_VALUE, F_XY_GOAL_AGE,
 F_HI_GOAL, F_LO_GOAL_DIST, F_XY_BOOTSTRAP_GOAL, F_PPO_STATS, F_HPPO_LO_STATS, F_HPPO_HI_STATS,
 F_XYPPO_LO_STATS, F_XYPPO_HI_STATS, F_SKPPO_LO_STATS, F_SKPPO_HI_STATS, F_OPPPO_LO_STATS,
 F_OPPPO_HI_STATS, F_DIAYN_STATS, F_DIAYN_SAMPLES, F_ORDER_ROWS, F_A2C_STATS) = range(87)
(RESULT_OBS, RESULT_REWARD, RESULT_DONE, RESULT_GOAL_MET, RESULT_EXCEPTION, RESULT_ZONE_OBS) = range(6)
N_RESULTS = 6


MLP_TENSORS = ("zone_w1", "zone_b1", "zone_w2", "zone_b2", "zone_w3", "zone_b3", "comb_w", "comb_b",
               "enc_w", "enc_b", "mu_w", "mu_b", "std_w", "std_b")
MLP_CRITIC_TENSORS = ("critic_w1", "critic_b1", "critic_w2", "critic_b2")   # optional, all or none
MLP_SIGMA_TENSORS = ("critic_sigma_w", "critic_sigma_b")   # optional: the distributional critic (critic_w2 = critic_mu)
MLP_BF16, MLP_F32, MLP_BF16X3, MLP_F16X3, MLP_F16 = 0, 1, 2, 3, 4


class MlpWeights(C.Structure):
    """struct zenv_mlp_weights (include/zenv.h): host float32 tensors in state_dict layout."""
    _fields_ = [("h_dim", C.c_int32), ("precision", C.c_int32)] + [
        (n, C.c_void_p) for n in MLP_TENSORS + MLP_CRITIC_TENSORS + MLP_SIGMA_TENSORS]


# struct zenv_hier_weights (include/zenv.h): hi_model_state / lo_model_state of the Zone-goals agent
HIER_HI_TENSORS = ("hi_zone_w1", "hi_zone_b1", "hi_zone_w2", "hi_zone_b2", "hi_zone_w3", "hi_zone_b3", "hi_comb_w",
                   "hi_comb_b", "hi_actor_w1", "hi_actor_b1", "hi_actor_w2", "hi_actor_b2")
HIER_HI_CRITIC = ("hi_critic_w1", "hi_critic_b1", "hi_critic_w2", "hi_critic_b2")    # optional, all or none
HIER_LO_TENSORS = ("lo_zone_w1", "lo_zone_b1", "lo_zone_w2", "lo_zone_b2", "lo_zone_w3", "lo_zone_b3", "lo_comb_w",
                   "lo_comb_b", "lo_enc_w", "lo_enc_b", "lo_mu_w", "lo_mu_b", "lo_std_w", "lo_std_b")
HIER_LO_CRITIC = ("lo_critic_w1", "lo_critic_b1", "lo_critic_w2", "lo_critic_b2")    # optional, all or none


class HierWeights(C.Structure):
    """struct zenv_hier_weights (include/zenv.h): host float32 tensors in state_dict layout."""
    _fields_ = [("h_dim", C.c_int32), ("precision", C.c_int32), ("zone_feat", C.c_int32), ("pad", C.c_int32)] + [
        (n, C.c_void_p) for n in HIER_HI_TENSORS + HIER_HI_CRITIC + HIER_LO_TENSORS + HIER_LO_CRITIC]


# struct zenv_skill_weights (include/zenv.h): hi_model_state / lo_model_state of the fixed-length-skills agent
SKILL_HI_TENSORS = ("hi_zone_w1", "hi_zone_b1", "hi_zone_w2", "hi_zone_b2", "hi_zone_w3", "hi_zone_b3", "hi_comb_w",
                    "hi_comb_b", "hi_enc_w", "hi_enc_b", "hi_logit_w", "hi_logit_b")
SKILL_HI_CRITIC = HIER_HI_CRITIC                                                     # optional, all or none
SKILL_LO_TENSORS = HIER_LO_TENSORS
SKILL_LO_CRITIC = HIER_LO_CRITIC                                                     # optional, all or none


class SkillWeights(C.Structure):
    """struct zenv_skill_weights (include/zenv.h): host float32 tensors in state_dict layout."""
    _fields_ = [("h_dim", C.c_int32), ("n_skills", C.c_int32), ("zone_feat", C.c_int32), ("precision", C.c_int32)] + [
        (n, C.c_void_p) for n in SKILL_HI_TENSORS + SKILL_HI_CRITIC + SKILL_LO_TENSORS + SKILL_LO_CRITIC]


class OptionWeights(C.Structure):
    """struct zenv_option_weights (include/zenv.h): zenv_skill_weights' members; lo_mu_* / lo_std_* have three rows."""
    _fields_ = list(SkillWeights._fields_)


# struct zenv_skill_inverse_weights (include/zenv.h): InverseModel, DIAYN's discriminator (main/src/inverse_model.py)
SKILL_INVERSE_TENSORS = ("zone_w1", "zone_b1", "zone_w2", "zone_b2", "zone_w3", "zone_b3", "comb_w1", "comb_b1",
                         "comb_w2", "comb_b2")


class SkillInverseWeights(C.Structure):
    """struct zenv_skill_inverse_weights (include/zenv.h): host float32 tensors in state_dict layout."""
    _fields_ = [("h_dim", C.c_int32), ("n_skills", C.c_int32), ("zone_feat", C.c_int32), ("precision", C.c_int32)] + [
        (n, C.c_void_p) for n in SKILL_INVERSE_TENSORS]


# struct zenv_xy_weights (include/zenv.h): hi_model_state / lo_model_state of the xy-goals agent -- the flat
# actor-critic's network above the Zone-goals low level
XY_HI_TENSORS = ("hi_zone_w1", "hi_zone_b1", "hi_zone_w2", "hi_zone_b2", "hi_zone_w3", "hi_zone_b3", "hi_comb_w",
                 "hi_comb_b", "hi_enc_w", "hi_enc_b", "hi_mu_w", "hi_mu_b", "hi_std_w", "hi_std_b")
XY_HI_CRITIC = HIER_HI_CRITIC                                                        # optional, all or none
XY_LO_TENSORS = HIER_LO_TENSORS
XY_LO_CRITIC = HIER_LO_CRITIC                                                        # optional, all or none


class XyWeights(C.Structure):
    """struct zenv_xy_weights (include/zenv.h): host float32 tensors in state_dict layout."""
    _fields_ = [("h_dim", C.c_int32), ("zone_feat", C.c_int32), ("precision", C.c_int32), ("pad", C.c_int32)] + [
        (n, C.c_void_p) for n in XY_HI_TENSORS + XY_HI_CRITIC + XY_LO_TENSORS + XY_LO_CRITIC]


PPO_PARAM, PPO_GRAD, PPO_EXP_AVG, PPO_EXP_AVG_SQ = 0, 1, 2, 3
PPO_STATS = ("entropy", "value", "value_std", "policy_loss", "value_loss", "grad_norm")   # ZENV_F_PPO_STATS' columns
HPPO_LO, HPPO_HI = 0, 1                                       # the `level` of the zenv_hppo_* functions
HPPO_STATS_FIELDS = (F_HPPO_LO_STATS, F_HPPO_HI_STATS)        # by level
XYPPO_LO, XYPPO_HI = 0, 1                                     # the `level` of the zenv_xyppo_* functions
XYPPO_STATS_FIELDS = (F_XYPPO_LO_STATS, F_XYPPO_HI_STATS)     # by level
SKPPO_LO, SKPPO_HI = 0, 1                                     # the `level` of the zenv_skppo_* functions
SKPPO_STATS_FIELDS = (F_SKPPO_LO_STATS, F_SKPPO_HI_STATS)     # by level
OPPPO_LO, OPPPO_HI = 0, 1                                     # the `level` of the zenv_opppo_* functions
OPPPO_STATS_FIELDS = (F_OPPPO_LO_STATS, F_OPPPO_HI_STATS)     # by level
DIAYN_STATS = ("loss", "", "", "", "", "grad_norm")           # ZENV_F_DIAYN_STATS' columns (1-4 are 0)


class PpoConfig(C.Structure):
    """struct zenv_ppo_config (include/zenv.h)."""
    _fields_ = [("lr", C.c_double), ("adam_eps", C.c_double), ("clip_eps", C.c_double), ("entropy_coef", C.c_double),
                ("value_loss_coef", C.c_double), ("max_grad_norm", C.c_double), ("max_batch", C.c_int32),
                ("distributional_value", C.c_int32)]


A2C_PARAM, A2C_GRAD, A2C_SQUARE_AVG = 0, 1, 2                 # the arenas of the zenv_a2c_* functions
A2C_STATS = ("entropy", "value", "policy_loss", "value_loss", "grad_norm")   # ZENV_F_A2C_STATS, a2c.py:85-91's order


class A2cConfig(C.Structure):
    """struct zenv_a2c_config (include/zenv.h)."""
    _fields_ = [("lr", C.c_double), ("rmsprop_alpha", C.c_double), ("rmsprop_eps", C.c_double),
                ("entropy_coef", C.c_double), ("value_loss_coef", C.c_double), ("max_grad_norm", C.c_double),
                ("max_batch", C.c_int32)]


RENDER_CURRENT, RENDER_EXPERIENCE = 0, 1                      # zenv_render_config.source
# layouts sampled on the device: ZENV_DEVICE_RESTARTS, ZENV_SAMPLE_STATUS_CAP, the codes of zenv_sample_status
DEVICE_RESTARTS, SAMPLE_STATUS_CAP = 256, 1024
SAMPLE_UNFINISHED, SAMPLE_SEED_RANGE = 1, 2
DET_OP_LOG, DET_OP_DIV, DET_OP_SQRT = 0, 1, 2   # zenv_det_ops


class RenderConfig(C.Structure):
    """struct zenv_render_config (include/zenv.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("source", C.c_int32), ("env", C.c_int32),
                ("view", C.c_float), ("robot_radius", C.c_float)]


# the columns of zenv_episode_log (ZENV_EPLOG_*) and the key each has in the reference's `logs`
(EPLOG_RETURN, EPLOG_RESHAPED_RETURN, EPLOG_NUM_FRAMES, EPLOG_DIVERSITY, EPLOG_PREDICTION, EPLOG_ENV) = range(6)
EPLOG_COUNT = 6
EPLOG_KEYS = ("return_per_episode", "reshaped_return_per_episode", "num_frames_per_episode", "diversity_per_episode",
              "prediction_per_episode", "env_per_episode")


class EpisodeLogInfo(C.Structure):
    """struct zenv_episode_log_info (include/zenv.h)."""
    _fields_ = [("kept", C.c_int64), ("done", C.c_int64), ("num_frames", C.c_int64), ("columns", C.c_int64)]


class ZenvError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"zenv error {code}: {message}")
        self.code = code


class Config(C.Structure):
    """Mirror of ``zenv_config`` (include/zenv.h)."""
    _fields_ = [
        ("task", C.c_int32), ("num_zones", C.c_int32), ("num_steps", C.c_int32),
        ("max_cd", C.c_int32), ("frameskip", C.c_int32), ("kernel", C.c_int32),
        ("zones_size", C.c_double), ("zones_keepout", C.c_double), ("robot_keepout", C.c_double),
        ("extent", C.c_double), ("placements_margin", C.c_double),
        ("time_saved_reward", C.c_double), ("beta_a", C.c_double), ("beta_b", C.c_double),
        ("timestep", C.c_double), ("mass", C.c_double), ("com_x", C.c_double),
        ("inertia_zz", C.c_double), ("damping", C.c_double * 3), ("gear", C.c_double),
        ("forcerange", C.c_double), ("vel_kv", C.c_double), ("reward_exception", C.c_double),
        ("n_zones_locations", C.c_int32), ("n_robot_locations", C.c_int32), ("robot_rot_fixed", C.c_int32),
        ("visited0", C.c_uint32), ("robot_rot", C.c_double), ("robot_location", C.c_double * 2),
        ("zones_locations", (C.c_double * 2) * MAX_ZONES),
    ]

    def copy(self):
        out = Config()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(Config))
        return out


# every symbol include/zenv.h declares: name -> (restype, argtypes)
_H = C.c_void_p


def _learner_prototypes(name, levels=False, updates=True):
    """What every learner family declares: zenv_<name>_check / _init over its weights and one settings struct per
    learner, the accessors of a learner's arenas and step count and (updates) the PPO update calls.  levels: a pair of
    learners, whose calls take `int level` behind the handle."""
    settings = [C.c_void_p] * (2 if levels else 1)
    h = [_H, C.c_int] if levels else [_H]
    out = {"check": [C.POINTER(Config), C.c_void_p] + settings, "init": [_H, C.c_void_p] + settings,
           "tensor": h + [C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)],
           "read": h + [C.c_int, C.c_int, C.c_void_p], "write": h + [C.c_int, C.c_int, C.c_void_p],
           "get_step": h + [C.POINTER(C.c_int64)], "set_step": h + [C.c_int64]}
    if updates:
        out.update({"minibatch": h + [C.c_void_p, C.c_int, C.c_int, C.c_int], "apply": h,
                    "epoch": h + [C.c_void_p, C.c_int, C.c_int, C.c_int]})
    return {f"zenv_{name}_{call}": (C.c_int, argtypes) for call, argtypes in out.items()}


_PROTOTYPES = {
    "zenv_last_error": (C.c_char_p, []),
    "zenv_version": (C.c_char_p, []),
    "zenv_device_count": (C.c_int, []),
    "zenv_build_flags": (C.c_char_p, []),
    "zenv_rollout_chunk": (C.c_int, []),
    "zenv_config_for_id": (C.c_int, [C.c_char_p, C.POINTER(Config)]),
    "zenv_default_config": (C.c_int, [C.c_int, C.c_int, C.POINTER(Config)]),
    "zenv_zone_feat": (C.c_int, [C.POINTER(Config)]),
    "zenv_config_size": (C.c_int, []),
    "zenv_sample_layout": (C.c_int, [C.POINTER(Config), C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_int32)]),
    "zenv_fixed_seed_sequence": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
    "zenv_create": (C.c_int, [C.POINTER(Config), C.c_int, C.c_int, C.POINTER(_H)]),
    "zenv_destroy": (C.c_int, [_H]),
    "zenv_num_envs": (C.c_int, [_H]),
    "zenv_get_config": (C.c_int, [_H, C.POINTER(Config)]),
    "zenv_bank_build": (C.c_int, [_H, C.c_int64, C.c_int, C.c_int]),
    "zenv_bank_build_seeds": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int]),
    "zenv_bank_set": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "zenv_bank_size": (C.c_int, [_H]),
    "zenv_bank_update": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "zenv_sample_layout_shared": (C.c_int, [C.POINTER(Config), C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(C.c_int32)]),
    "zenv_layout_thresholds": (C.c_int, [C.POINTER(Config), C.c_void_p, C.c_void_p]),
    "zenv_sample_layout_timed": (C.c_int, [C.POINTER(Config), C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(C.c_int32)]),
    "zenv_timed_layouts_device": (C.c_int, [_H, C.c_int]),
    "zenv_det_ops": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "zenv_bank_build_device": (C.c_int, [_H, C.c_int64, C.c_int]),
    "zenv_bank_build_seeds_device": (C.c_int, [_H, C.c_void_p, C.c_int]),
    "zenv_bank_update_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int]),
    "zenv_ring_stream": (C.c_int, [_H, C.c_void_p, C.c_int32]),
    "zenv_ring_refill": (C.c_int, [_H]),
    "zenv_sample_status": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int64)]),
    "zenv_bank_read": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "zenv_schedule_ring": (C.c_int, [_H, C.c_void_p, C.c_int32]),
    "zenv_schedule_sequential": (C.c_int, [_H, C.c_void_p, C.c_int32]),
    "zenv_schedule_fixed_seeds": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int64]),
    "zenv_reset": (C.c_int, [_H, C.c_void_p]),
    "zenv_step": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int]),
    "zenv_step_many": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "zenv_policy": (C.c_int, [_H, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]),
    "zenv_rollout": (C.c_int, [_H, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int,
                               C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zenv_set_rollout_slice": (C.c_int, [_H, C.c_int]),
    "zenv_collect": (C.c_int, [_H, C.c_int, C.c_uint64, C.c_uint64, C.c_float, C.c_float]),
    "zenv_collect_hier": (C.c_int, [_H, C.c_int, C.c_uint64, C.c_uint64, C.c_float, C.c_float,
                                    C.POINTER(C.c_int64)]),
    "zenv_order_enable": (C.c_int, [_H]),
    "zenv_order_configure": (C.c_int, [_H, C.c_int]),
    "zenv_route_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "zenv_route_ranks_shared": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "zenv_route_ranks_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "zenv_order_routes_device": (C.c_int, [_H, C.c_int]),
    "zenv_order_rows": (C.c_int, [_H, C.c_int]),
    "zenv_goal_enable": (C.c_int, [_H]),
    "zenv_set_goals": (C.c_int, [_H, C.c_void_p]),
    "zenv_solver_goals": (C.c_int, [_H, C.c_void_p]),
    "zenv_mlp_load": (C.c_int, [_H, C.c_void_p]),
    "zenv_mlp_forward": (C.c_int, [_H]),
    "zenv_hier_load": (C.c_int, [_H, C.c_void_p]),
    "zenv_hier_forward": (C.c_int, [_H]),
    "zenv_skill_load": (C.c_int, [_H, C.c_void_p]),
    "zenv_skill_configure": (C.c_int, [_H, C.c_int]),
    "zenv_set_skills": (C.c_int, [_H, C.c_void_p]),
    "zenv_skill_forward": (C.c_int, [_H]),
    "zenv_skill_inverse_load": (C.c_int, [_H, C.c_void_p]),
    "zenv_option_load": (C.c_int, [_H, C.c_void_p]),
    "zenv_option_forward": (C.c_int, [_H]),
    "zenv_xy_load": (C.c_int, [_H, C.c_void_p]),
    "zenv_set_xy_goals": (C.c_int, [_H, C.c_void_p, C.c_void_p]),
    "zenv_xy_forward": (C.c_int, [_H]),
    "zenv_collect_skill": (C.c_int, [_H, C.c_int, C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                     C.c_int]),
    "zenv_collect_option": (C.c_int, [_H, C.c_int, C.c_uint64, C.c_uint64, C.c_float, C.c_float,
                                      C.POINTER(C.c_int64)]),
    "zenv_collect_xy": (C.c_int, [_H, C.c_int, C.c_uint64, C.c_uint64, C.c_float, C.c_float]),
    **_learner_prototypes("ppo"),
    **_learner_prototypes("hppo", levels=True),
    **_learner_prototypes("xyppo", levels=True),
    **_learner_prototypes("skppo", levels=True),
    **_learner_prototypes("opppo", levels=True),
    **_learner_prototypes("diayn"),
    "zenv_diayn_samples": (C.c_int, [_H, C.POINTER(C.c_int64)]),
    "zenv_diayn_prior_init": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_double, C.c_double]),
    "zenv_diayn_prior_update": (C.c_int, [_H]),
    "zenv_diayn_prior_read": (C.c_int, [_H, C.c_void_p]),
    "zenv_diayn_prior_write": (C.c_int, [_H, C.c_void_p]),
    "zenv_get": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_int]),
    "zenv_get_rows": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "zenv_device_ptr": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p)]),
    "zenv_field_bytes": (C.c_int64, [_H, C.c_int]),
    "zenv_sync": (C.c_int, [_H]),
    "zenv_query": (C.c_int, [_H]),
    "zenv_host_alloc": (C.c_void_p, [C.c_int64]),
    "zenv_host_free": (C.c_int, [C.c_void_p]),
    "zenv_get_many": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "zenv_results_layout": (C.c_int64, [_H, C.POINTER(C.c_int64)]),
    "zenv_step_results": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p]),
    "zenv_host_io": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "zenv_step_host": (C.c_int, [_H, C.c_int]),
    "zenv_set_stream": (C.c_int, [_H, C.c_void_p]),
    "zenv_comm_unique_id": (C.c_int, [C.c_void_p]),
    "zenv_comm_init": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p]),
    "zenv_comm_destroy": (C.c_int, [_H]),
    "zenv_comm_info": (C.c_int, [_H, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]),
    "zenv_allgather": (C.c_int, [_H, C.c_int, C.c_void_p, C.c_int]),
    "zenv_comm_barrier": (C.c_int, [_H]),
    "zenv_comm_allreduce_max": (C.c_int, [_H, C.POINTER(C.c_double)]),
    "zenv_render_check": (C.c_int, [C.POINTER(Config), C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "zenv_render": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "zenv_episode_log": (C.c_int, [_H, C.POINTER(EpisodeLogInfo)]),
    "zenv_episode_log_tensor": (C.c_int, [_H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "zenv_episode_log_read": (C.c_int, [_H, C.c_int, C.c_void_p]),
    "zenv_episode_log_stats": (C.c_int, [_H, C.c_int, C.POINTER(C.c_double)]),
    "zenv_episode_log_reset": (C.c_int, [_H]),
    "zenv_probe_store_stream": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_float)]),
    "zenv_step_count": (C.c_int64, [_H]),
    "zenv_state_bytes": (C.c_int64, [_H]),
    "zenv_get_state": (C.c_int, [_H, C.c_void_p, C.c_int64]),
    "zenv_set_state": (C.c_int, [_H, C.c_void_p, C.c_int64]),
    "zenv_debug_state": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# The A2C learner's entry points (zenv_a2c_*), bound with the rest in lib().  They are kept in a table of their own: the
# stream class of every name in _PROTOTYPES is tabled in tests/stream_stall.py, theirs in tests/a2c_stream_classes.py.
_A2C_PROTOTYPES = {
    **_learner_prototypes("a2c", updates=False),
    "zenv_a2c_accumulate": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int]),
    "zenv_a2c_apply": (C.c_int, [_H]),
    "zenv_a2c_update": (C.c_int, [_H]),
}

_lib = None


def lib():
    """Load libzenv_hip.so once.  Raises ImportError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # If torch is (or will be) in this process its bundled libamdhip64 must be the one HIP
    # runtime: make sure it is loaded first so our DT_NEEDED resolves to the same copy.
    if "torch" in sys.modules:
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL if hasattr(C, "RTLD_GLOBAL") else 0)
    for name, (restype, argtypes) in {**_PROTOTYPES, **_A2C_PROTOTYPES}.items():
        fn = getattr(L, name)   # AttributeError if the ABI is incomplete
        fn.restype = restype
        fn.argtypes = argtypes
    if L.zenv_config_size() != C.sizeof(Config):
        raise ImportError("zenv_config layout mismatch between include/zenv.h and _native.Config")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = lib().zenv_last_error()
        raise ZenvError(rc, msg.decode() if msg else "")
    return rc


def exported_symbols():
    return sorted({**_PROTOTYPES, **_A2C_PROTOTYPES})
