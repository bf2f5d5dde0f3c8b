/*
 * zenv.h -- C ABI of the MI355X-native batched zone-env step path.
 *
 * Drop-in boundary for the env.step()/reset() hot path of
 * andrewli77/combinatorial-rl-tasks (paths below are relative to the reference root):
 *   main/envs/TSP_env.py, main/envs/TTSP_env.py, main/envs/colour_match_env.py,
 *   main/envs/zone_envs/ZoneEnvBase.py, main/envs/wrappers.py (FixedSeedsWrapper,
 *   ZoneWrapper), main/src/torch_ac/torch_utils/penv.py (ParallelEnv) and, beneath them,
 *   safety_gym Engine.step/reset + MuJoCo mj_step for xmls/point.xml (not vendored).
 *
 * Conventions: every entry point is extern "C", takes plain pointers and sizes, returns
 * 0 on success or a negative ZENV_E_* code (text from zenv_last_error()); no exception
 * crosses the boundary.  The caller owns every buffer it passes; the library owns the
 * handle and its device memory until zenv_destroy().  A handle is bound to one device and
 * one HIP stream and is not thread-safe.  zenv_step()/zenv_reset()/zenv_policy()/zenv_bank_update() are
 * asynchronous on the handle's stream; zenv_get*(), zenv_sync() and -- unless ZENV_ROLLOUT_ASYNC is set --
 * zenv_rollout() synchronise.
 *
 * Host buffers passed to an asynchronous call (the mask of zenv_reset, host actions of zenv_step / zenv_step_many, host
 * indices of the *_minibatch / *_epoch calls, host marks of zenv_render): pageable memory may be reused or freed as soon
 * as the call returns (such a call may wait for a busy stream); page-locked memory (zenv_host_alloc) is read when the
 * stream reaches the call and must stay untouched until then (zenv_sync, or zenv_query() == 1).  Device memory, or NULL
 * where the call takes it, keeps such a call asynchronous.  zenv_bank_update / zenv_bank_update_device copy their
 * arguments during the call; a second refill while the first one's copy is still queued waits for it.
 * The learners' *_get_step counts the Adam steps ENQUEUED so far; it does not wait for them.
 * tests/stream_stall.py classifies every entry point (asynchronous / synchronises / reads host memory / host only).
 *
 * There is no CPU fallback: every compute entry point fails with ZENV_E_HIP when no
 * gfx950 device is usable.
 */
#ifndef ZENV_H
#define ZENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZENV_MAX_ZONES 32
#define ZENV_OBS_DIM 8

/* tasks: envs/__init__.py:88-141 registry ids PointTSP-v0/v1, PointTTSP-v0/v1, ColourMatch-v0 */
enum { ZENV_TASK_TSP = 0, ZENV_TASK_TIMED_TSP = 1, ZENV_TASK_COLOUR_MATCH = 2 };

/* error codes */
enum {
    ZENV_OK = 0,
    ZENV_E_ARG = -1,        /* bad argument */
    ZENV_E_HIP = -2,        /* HIP runtime / no device */
    ZENV_E_STATE = -3,      /* call order (e.g. step before bank/reset) */
    ZENV_E_LAYOUT = -4,     /* ResamplingError: no layout in 10000 tries */
    ZENV_E_DONE = -5,       /* single-env semantics: 'Environment must be reset before stepping' */
    ZENV_E_RANGE = -6       /* ZENV_MLP_F16X3: a weight, input or activation of the network beyond float16's range */
};

/* zenv_get()/zenv_device_ptr() selectors */
enum {
    ZENV_F_OBS = 0,         /* float32 [N,8]   wrappers.py:136-142 'obs' = remaining,pos,dir,velp,velr */
    ZENV_F_ZONE_OBS = 1,    /* float32 [N,Z,F] wrappers.py:137 'zone_obs' */
    ZENV_F_REWARD = 2,      /* float32 [N] */
    ZENV_F_DONE = 3,        /* uint8   [N]     done flag returned by the last step */
    ZENV_F_GOAL_MET = 4,    /* uint8   [N]     info['goal_met'] (evaluate.py:65) */
    /* EP_RETURN / EP_LEN live inside the step kernels' records: zenv_get / zenv_device_ptr unpack them (stream-ordered),
     * and a device pointer of these two is a plain copy as of that call, not a live view */
    ZENV_F_EP_RETURN = 5,   /* float64 [N]     undiscounted return of the running episode */
    ZENV_F_EP_LEN = 6,      /* int32   [N]     steps of the running episode */
    ZENV_F_LAST_RETURN = 7, /* float64 [N]     return of the last finished episode (evaluate.py:62-72) */
    ZENV_F_LAST_LEN = 8,    /* int32   [N] */
    ZENV_F_EPISODES = 9,    /* int32   [N]     episodes finished so far */
    ZENV_F_VISIT_COUNT = 10,/* int32   [N]     visited zones (TSP/Timed) or goal_dist (ColourMatch) */
    ZENV_F_SEED = 11,       /* int64   [N]     env seed of the running episode */
    ZENV_F_ACTIONS = 12,    /* float32 [N,2]   internal action buffer (zenv_policy target) */
    ZENV_F_POLICY_MU = 13,  /* float32 [N,2]   mean of the actor's Normal (after zenv_mlp_forward) */
    ZENV_F_POLICY_STD = 14, /* float32 [N,2]   its standard deviation */
    ZENV_F_POLICY_VALUE = 15, /* float32 [N]   the critic's value (when critic weights were loaded) */
    /* goal-conditioned variant, after zenv_goal_enable(): */
    ZENV_F_SHAPED_REWARD = 16,   /* float64 [N] info['shaped_reward'] (TSP_next_city_env.py:60-66) */
    ZENV_F_NEED_GOAL = 17,       /* uint8   [N] info['need_next_goal'] / env.goal_zone is None (:69-75) */
    ZENV_F_AVAILABLE_GOALS = 18, /* uint32  [N] get_available_goals() as a bit mask, bit z = zone z unvisited */
    ZENV_F_GOAL = 19,            /* int32   [N] goal zone, -1 = none */
    /* experience buffers of the last zenv_collect(), time-major [T][N][...]; their [N][T] transposes, flattened, are
     * exps.* of base.py:125-128, :211-227 */
    ZENV_F_EXP_OBS = 20,         /* float32 [T,N,8]    every ZENV_F_EXP_* buffer is time-major (frame t of all envs is
                                  *                    contiguous); the observations are written in place by the step kernel */
    ZENV_F_EXP_ZONE_OBS = 21,    /* float32 [T,N,Z,F] */
    ZENV_F_EXP_ACTION = 22,      /* float32 [T,N,2] */
    ZENV_F_EXP_LOG_PROB = 23,    /* float32 [T,N,2]  Normal(mu, std).log_prob(action) */
    ZENV_F_EXP_VALUE = 24,       /* float32 [T,N] */
    ZENV_F_EXP_REWARD = 25,      /* float32 [T,N]    shaped_reward when the handle is goal-conditioned (:153-159) */
    ZENV_F_EXP_MASK = 26,        /* float32 [T,N]    1 - done of the previous step (:149-150) */
    ZENV_F_EXP_ADVANTAGE = 27,   /* float32 [T,N]    GAE (:190-196) */
    ZENV_F_EXP_RETURN = 28,      /* float32 [T,N]    value + advantage (:226) */
    ZENV_F_ORDER_VAL = 29,       /* float32 [N,Z]    TSPOrderEnv's 7th row feature 0.5^(position in the route), 0 when visited */
    ZENV_F_POLICY_VALUE_SIGMA = 31, /* float32 [N]   the distributional critic's sigma (flat_model.py:57-60) */
    ZENV_F_EXCEPTION = 30,       /* uint8   [N]      info['exception'] of the env's LAST FINISHED episode: 1 = it was ended by
                                  *                    Engine.step's MujocoException path (valid once done; see zenv_step) */
    ZENV_F_ORDER_POS = 32,       /* int8    [N,Z]    TSPOrderEnv's self.route: position of every zone in the remaining route, -1 =
                                  *                    not in it (visited) */
    /* time-major records of the last zenv_step_many(): every step of the chunk */
    ZENV_F_CHUNK_REWARD = 33,    /* float32 [K,N] */
    ZENV_F_CHUNK_DONE = 34,      /* uint8   [K,N] */
    ZENV_F_CHUNK_ACTIONS = 35,   /* float32 [K,N,2]  the device copy of the last chunk whose actions came from the host (a caller that
                                  *                    replays it passes zenv_device_ptr() of this field back, actions_on_device = 1);
                                  *                    K is that chunk's length, not the last call's.  0 bytes once a
                                  *                    device-action chunk has outgrown the buffer (its copy is gone) */
    /* Zone-goals hierarchical agent (zenv_hier_load): */
    ZENV_F_HIER_LOGITS = 36,     /* float32 [N,Z]    the high level's logit of every zone, -INFINITY where the zone is not an
                                  *                    available goal (hier_agent.py get_hi_action: logits[~available] = -inf);
                                  *                    unnormalised: actor.2's output, not Categorical's log-softmax */
    ZENV_F_HIER_VALUE = 37,      /* float32 [N]      the high level's critic value (0 without critic tensors); after
                                  *                    zenv_collect_hier: V_hi(obs_T), the high level's bootstrap value */
    /* Zone-goals experience of the last zenv_collect_hier().  The low level's other records are the ZENV_F_EXP_* buffers
     * (time-major [T][N]): obs, zone_obs, action, log_prob, value, reward (= info['shaped_reward']), mask, advantage and
     * return, the last two over frames 0 .. T-2 only (0 at frame T-1) */
    ZENV_F_LO_GOAL = 38,         /* float32 [T,N,2]  the low level's goal input (cur_goal): the goal zone's centre / 3 */
    ZENV_F_LO_ENV_REWARD = 39,   /* float32 [T,N]    the env reward of every frame (what hi_reward sums) */
    /* the closed high-level transitions, flat and env-major (env 0's in order, then env 1's ...): M rows */
    ZENV_F_HI_OBS = 40,          /* float32 [M,8]    the observation the goal was picked on */
    ZENV_F_HI_ZONE_OBS = 41,     /* float32 [M,Z,F] */
    ZENV_F_HI_ACTION = 42,       /* int32   [M]      the goal zone */
    ZENV_F_HI_ACTION_MASK = 43,  /* uint8   [M,Z]    the available goals when it was picked (1 = available) */
    ZENV_F_HI_VALUE = 44,        /* float32 [M]      the high critic's value */
    ZENV_F_HI_LOG_PROB = 45,     /* float32 [M]      log_prob(goal) of Categorical(masked logits): the log-softmax */
    ZENV_F_HI_ADVANTAGE = 46,    /* float32 [M] */
    ZENV_F_HI_RETURN = 47,       /* float32 [M]      value + advantage */
    ZENV_F_HI_REWARD = 48,       /* float32 [M]      the transition's reward: the env rewards from its pick to its close */
    ZENV_F_HI_MASK = 49,         /* float32 [M]      hi_mask: 0 when it closed because the episode ended, else 1 */
    ZENV_F_HI_COUNT = 50,        /* int32   [N]      rows of every env (closed transitions of the last call) */
    /* fixed-length-skills agent (zenv_skill_load).  zenv_reset and every auto-reset (zenv_step, zenv_step_many,
     * zenv_collect ...) clear the skill state; zenv_get / zenv_device_ptr bring it up to date (like ZENV_F_EP_LEN, a
     * device pointer of these two is a copy as of that call, not a live view) */
    ZENV_F_SKILL = 51,           /* int32   [N]      the env's current skill, -1 = none */
    ZENV_F_SKILL_AGE = 52,       /* int32   [N]      low-level steps taken under the current skill */
    ZENV_F_SKILL_LOGITS = 53,    /* float32 [N,S]    the high level's log-softmax: what Categorical(logits=log_softmax(x))
                                  *                    holds (main/src/policy_network.py:40-43) */
    ZENV_F_SKILL_VALUE = 54,     /* float32 [N]      the high level's critic value (0 without critic tensors) */
    /* fixed-length-skills experience of the last zenv_collect_skill() (before these three fields, ZENV_F_COUNT = 55).
     * Its other records reuse the Zone-goals fields: ZENV_F_EXP_* (the low level,
     * time-major [T][N], EXP_REWARD = reward + diversity_coef * diversity), ZENV_F_LO_ENV_REWARD (the env reward) and
     * the ZENV_F_HI_* rows (M = N * T / skill_len, env-major, ZENV_F_HI_ACTION = the skill; ZENV_F_HI_ACTION_MASK is not
     * written and has size 0) -- a skill handle is never goal-conditioned, so the two collections never share one */
    ZENV_F_LO_SKILL = 55,        /* int32   [T,N]    the skill the low level acted under at every frame */
    ZENV_F_LO_DIVERSITY = 56,    /* float32 [T,N]    DIAYN's diversity reward (0 everywhere without inverse weights) */
    ZENV_F_SKILL_BOOTSTRAP = 57, /* int32   [N]      s' ~ the high level at obs_T: the skill of next_lo_value */
    /* variable-length Options agent (zenv_option_load; before these five fields, ZENV_F_COUNT = 58): the third actor
     * output of the last zenv_policy(ZENV_POLICY_OPTION_*) / zenv_option_forward, 0 for an env that idled.  The agent
     * shares ZENV_F_SKILL / _SKILL_AGE / _SKILL_LOGITS / _SKILL_VALUE with the fixed-length-skills agent */
    ZENV_F_OPTION_TERM_MU = 58,     /* float32 [N]   mu_2 */
    ZENV_F_OPTION_TERM_STD = 59,    /* float32 [N]   std_2 */
    ZENV_F_OPTION_TERM_ACTION = 60, /* float32 [N]   a_2: the sampled (unclipped) third component, or mu_2 */
    ZENV_F_OPTION_TERM_PROB = 61,   /* float32 [N]   sigmoid(4 a_2 - 3) */
    ZENV_F_OPTION_ENDED = 62,       /* int32   [N]   1 = the env's option ended on the last policy call: it picks a new
                                     *               skill on the next.  Cleared wherever the skill state is (a reset,
                                     *               zenv_set_skills); brought up to date like ZENV_F_SKILL */
    /* Options experience of the last zenv_collect_option() (before these three fields, ZENV_F_COUNT = 63).  Its other
     * records reuse the fields above: ZENV_F_EXP_* (the low level, time-major [T][N], the first two action components;
     * EXP_REWARD = the env reward), ZENV_F_LO_SKILL, ZENV_F_LO_ENV_REWARD and the ZENV_F_HI_* rows with ZENV_F_HI_COUNT
     * (M closed transitions, env-major, ZENV_F_HI_ACTION = the skill; ZENV_F_HI_ACTION_MASK is not written and has
     * size 0) */
    ZENV_F_LO_TERM_ACTION = 63,     /* float32 [T,N] a_2, the third component of the low level's sample */
    ZENV_F_LO_TERM_LOG_PROB = 64,   /* float32 [T,N] Normal(mu_2, std_2).log_prob(a_2) */
    ZENV_F_LO_OPTION_ENDED = 65,    /* uint8   [T,N] the termination draw: 1 = the option ended after this frame */
    /* xy-goals hierarchical agent (zenv_xy_load; before these five fields, ZENV_F_COUNT = 66): 0 bytes before the load.
     * zenv_reset and every auto-reset clear the goal as they clear a skill; reading the goal or its age first brings
     * the state up to date (like ZENV_F_SKILL, a device pointer of the age is a copy as of that call) */
    ZENV_F_XY_GOAL = 66,            /* float32 [N,2] the env's current goal, meaningful where ZENV_F_XY_GOAL_AGE >= 0 */
    ZENV_F_XY_GOAL_MU = 67,         /* float32 [N,2] the high level's Normal: 2 (sigmoid(actor.mu_) - 0.5) */
    ZENV_F_XY_GOAL_STD = 68,        /* float32 [N,2] sigmoid(actor.std_) + 1e-3 */
    ZENV_F_XY_VALUE = 69,           /* float32 [N]   the high level's critic value (0 without critic tensors) */
    ZENV_F_XY_GOAL_AGE = 70,        /* int32   [N]   low-level steps taken under the current goal, -1 = no goal */
    /* xy-goals experience of the last zenv_collect_xy() (before these three fields, ZENV_F_COUNT = 71).  Its other
     * records reuse the fields above: ZENV_F_EXP_* (the low level, time-major [T][N], EXP_REWARD = the distance-to-goal
     * reward), ZENV_F_LO_GOAL (the goal the low level acted under), ZENV_F_LO_ENV_REWARD (the env reward) and the
     * ZENV_F_HI_* rows with ZENV_F_HI_COUNT (M = N * T / skill_len, env-major; the goal is continuous, so
     * ZENV_F_HI_ACTION and ZENV_F_HI_ACTION_MASK are not written and have size 0) */
    ZENV_F_HI_GOAL = 71,            /* float32 [M,2] the high level's recorded goal */
    ZENV_F_LO_GOAL_DIST = 72,       /* float32 [T,N] the distance of the goal from the robot (obs[1:3]) at every frame */
    ZENV_F_XY_BOOTSTRAP_GOAL = 73,  /* float32 [N,2] g' ~ the high level at obs_T: the goal of next_lo_value */
    /* the flat actor-critic's learner (zenv_ppo_init; before this field, ZENV_F_COUNT = 74): the statistics of the
     * minibatches of the last zenv_ppo_minibatch (one row) or zenv_ppo_epoch; 0 bytes before the first */
    ZENV_F_PPO_STATS = 74,          /* float32 [minibatches][6] entropy, value, value std (0 without the distributional
                                     *               critic), policy loss, value loss, gradient norm before the clip: the
                                     *               logs of ppo.py:93-100, :121 */
    /* the Zone-goals agent's two learners (zenv_hppo_init; before these two fields, ZENV_F_COUNT = 75): the statistics
     * of the minibatches of the level's last zenv_hppo_minibatch (one row) or zenv_hppo_epoch; 0 bytes before the first */
    ZENV_F_HPPO_LO_STATS = 75,      /* float32 [minibatches][6] the low level's: ZENV_F_PPO_STATS' columns, value std = 0 */
    ZENV_F_HPPO_HI_STATS = 76,      /* float32 [minibatches][6] the high level's, the same */
    /* the xy-goals agent's two learners (zenv_xyppo_init): the statistics of the minibatches of the level's last
     * zenv_xyppo_minibatch (one row) or zenv_xyppo_epoch; 0 bytes before the first.  Before these two fields,
     * ZENV_F_COUNT = 77
     */
    ZENV_F_XYPPO_LO_STATS = 77,     /* float32 [minibatches][6] the low level's: ZENV_F_PPO_STATS' columns, value std = 0 */
    ZENV_F_XYPPO_HI_STATS = 78,     /* float32 [minibatches][6] the high level's, the same */
    /* the fixed-length-skills agent's two learners (zenv_skppo_init): the statistics of the minibatches of the level's
     * last zenv_skppo_minibatch (one row) or zenv_skppo_epoch; 0 bytes before the first.  Before these two fields,
     * ZENV_F_COUNT = 79
     */
    ZENV_F_SKPPO_LO_STATS = 79,     /* float32 [minibatches][6] the low level's: ZENV_F_PPO_STATS' columns, value std = 0 */
    ZENV_F_SKPPO_HI_STATS = 80,     /* float32 [minibatches][6] the high level's, the same */
    /* the Options agent's two learners (zenv_opppo_init): the statistics of the minibatches of the level's last
     * zenv_opppo_minibatch (one row) or zenv_opppo_epoch; 0 bytes before the first.  Before these two fields,
     * ZENV_F_COUNT = 81
     */
    ZENV_F_OPPPO_LO_STATS = 81,     /* float32 [minibatches][6] the low level's: ZENV_F_PPO_STATS' columns, value std = 0 */
    ZENV_F_OPPPO_HI_STATS = 82,     /* float32 [minibatches][6] the high level's, the same */
    /* DIAYN's inverse-model learner (zenv_diayn_init): the statistics of the minibatches of its last
     * zenv_diayn_minibatch (one row) or zenv_diayn_epoch, and the kept sample indexes of the last zenv_diayn_samples; 0
     * bytes before the first.  Before these two fields,
     * ZENV_F_COUNT = 83
     */
    ZENV_F_DIAYN_STATS = 83,        /* float32 [minibatches][6] column 0 the cross-entropy loss, 5 the gradient norm, 1-4 = 0 */
    ZENV_F_DIAYN_SAMPLES = 84,      /* int32   [count]          the kept sample indexes, ascending (= env-major) */
    /* a solver-ordered handle's network rows (zenv_order_rows): 0 bytes while the switch is off.  Before this field,
     * ZENV_F_COUNT = 85
     */
    ZENV_F_ORDER_ROWS = 85,         /* float32 [N,Z,7]  TSPOrderEnv's observation rows (TSP_order_env.py:37-47): row z =
                                     * [ZENV_F_ZONE_OBS row z (6), ZENV_F_ORDER_VAL z], the exact bits of both as they stand
                                     * when the field is asked for */
    /* the flat actor-critic's A2C learner (zenv_a2c_init): the statistics of the last zenv_a2c_apply / zenv_a2c_update;
     * 0 bytes before the first.  Before this field,
     * ZENV_F_COUNT = 86
     */
    ZENV_F_A2C_STATS = 86,          /* float32 [5] the reference's log order: entropy, value, policy_loss, value_loss,
                                     * grad_norm (a2c.py:85-91), over all the frames accumulated */
    ZENV_F_COUNT = 87
};

/* scripted on-device action sources (the build's own; used by bench/tests) */
enum {
    ZENV_POLICY_UNIFORM = 0,
    ZENV_POLICY_GREEDY = 1,
    ZENV_POLICY_MLP_MEAN = 2,   /* a = mu of the loaded actor network (zenv_mlp_load) */
    ZENV_POLICY_MLP_SAMPLE = 3, /* a ~ Normal(mu, std), the reference's dist.sample() (utils/agent.py:41-44) */
    /* the Zone-goals hierarchical agent (zenv_hier_load; goal-conditioned handles only), see zenv_hier_forward */
    ZENV_POLICY_HIER_SAMPLE = 4, /* goal ~ Categorical(masked logits), a ~ Normal(mu, std): HierAgent.get_hi_action /
                                  * get_lo_action (zone-goals/src/utils/hier_agent.py) */
    ZENV_POLICY_HIER_MEAN = 5,   /* goal = argmax of the masked logits (ties: lowest zone), a = mu: deterministic */
    /* the fixed-length-skills agent (zenv_skill_load; plain task handles only), see zenv_skill_forward */
    ZENV_POLICY_SKILL_SAMPLE = 6, /* skill ~ Categorical(logits) every skill_len steps, a ~ Normal(mu, std): HierAgent.
                                   * get_hi_action / get_lo_action (main/src/utils/hier_agent.py) */
    ZENV_POLICY_SKILL_MEAN = 7,   /* skill = argmax (ties: lowest skill), a = mu: deterministic */
    /* the variable-length Options agent (zenv_option_load; plain task handles only), see zenv_option_forward */
    ZENV_POLICY_OPTION_SAMPLE = 8, /* skill ~ Categorical(logits) when the last option ended, (a, a_2) ~ Normal(mu, std),
                                    * the option ends with probability sigmoid(4 a_2 - 3) */
    ZENV_POLICY_OPTION_MEAN = 9,   /* skill = argmax, a = mu, the option ends iff sigmoid(4 mu_2 - 3) > 0.5 */
    /* (10 and 11 are not policies: they stay unknown, ZENV_E_ARG, whatever is loaded)
     * the xy-goals hierarchical agent (zenv_xy_load; plain task handles only), see zenv_xy_forward */
    ZENV_POLICY_XY_SAMPLE = 12,    /* goal ~ Normal(goal_mu, goal_std) every skill_len steps, a ~ Normal(mu, std):
                                    * HierAgent.get_hi_action / get_lo_action (xy-goals/src/utils/hier_agent.py) */
    ZENV_POLICY_XY_MEAN = 13       /* goal = goal_mu, a = mu: deterministic */
};

/* kernel layouts */
enum {
    ZENV_KERNEL_LANE_PER_ENV = 0,  /* SoA state, one lane per env, LDS-transposed obs tile */
    ZENV_KERNEL_WAVE_PER_ENV = 1   /* one wave64 per env, lane z owns zone z (north-star layout): same results,
                                    * ~10x the step time; kept selectable for comparison */
};

/* Replaces the config dicts of envs/__init__.py:7-50 merged into Engine.DEFAULT
 * (ZoneEnvBase.py:42-53) and the model constants of xmls/point.xml. */
typedef struct zenv_config {
    int32_t task;              /* ZENV_TASK_* */
    int32_t num_zones;         /* 'num_cities' */
    int32_t num_steps;         /* 'num_steps' */
    int32_t max_cd;            /* colour_match_env.py:16 */
    int32_t frameskip;         /* Engine frameskip_binom_n (p = 1.0) */
    int32_t kernel;            /* ZENV_KERNEL_* */
    double zones_size;         /* ZoneEnvBase.py:51 */
    double zones_keepout;      /* ZoneEnvBase.py:50 */
    double robot_keepout;
    double extent;             /* ZoneEnvBase.py:41 */
    double placements_margin;
    double time_saved_reward;  /* TSP_env.py:15 */
    double beta_a, beta_b;     /* TTSP_env.py:13 */
    double timestep;           /* point.xml <option timestep> */
    double mass, com_x, inertia_zz;
    double damping[3];
    double gear, forcerange, vel_kv;
    double reward_exception;   /* Engine.DEFAULT 'reward_exception' (-10.0): the reward of a step MuJoCo could not simulate */
    /* Fixed placements and a pre-coloured start: config_zone_fixed_1/_2 of envs/__init__.py:52-81 for TSPHardEnv
     * (TSP_hard_env.py:11-29, ids PointTSP-v4 / -v5).  [not vendored] Engine.placements_dict_from_object gives object i
     * with a fixed location (x, y) the placement box (x-k, y-k, x+k, y+k), k = keepout + 1e-9, which draw_placement
     * shrinks by the keepout again: the object lands within 1e-9 of (x, y) and still consumes two uniform draws. */
    int32_t n_zones_locations; /* 'zones_locations': the first n zones are fixed, the rest sampled as usual */
    int32_t n_robot_locations; /* 'robot_locations': 0 or 1 entry */
    int32_t robot_rot_fixed;   /* != 0: 'robot_rot' is given (no random_rot() draw for the robot) */
    uint32_t visited0;         /* 'zones_colours': bit z set = zone z starts visited (Yellow); TSP / TimedTSP only */
    double robot_rot;
    double robot_location[2];
    double zones_locations[ZENV_MAX_ZONES][2];
} zenv_config;

typedef struct zenv zenv_t;

/* ---- configuration / introspection (host only; usable without a GPU) ---- */
const char *zenv_last_error(void);
const char *zenv_version(void);
/* Benchmark integrity: the extra compiler switches this library was built with ("" = the shipped build; anything else
 * is a diagnostic variant, e.g. "-DZENV_EXP=1" compiles the row flush out) and the steps one persistent launch really
 * covers (ZENV_ROLLOUT_CHUNK unless the diagnostic environment variable ZENV_ROLLOUT_CHUNK_EXP shortened it).  bench.py
 * prints both and refuses to time a variant unless asked to. */
int zenv_device_count(void);                  /* usable HIP devices (0 without a GPU); does not create a context */
const char *zenv_build_flags(void);
int zenv_rollout_chunk(void);
/* env_id: "PointTSP-v0", "PointTSP-v1", "PointTSP-v4", "PointTSP-v5" (TSPHardEnv), "PointTTSP-v0", "PointTTSP-v1",
 * "ColourMatch-v0" (envs/__init__.py:88-141); unknown id -> ZENV_E_ARG (make_env.py:18 RuntimeError). */
int zenv_config_for_id(const char *env_id, zenv_config *out);
int zenv_default_config(int task, int num_zones, zenv_config *out);
int zenv_zone_feat(const zenv_config *cfg);   /* F: 6 (TSP) or 7 */
int zenv_config_size(void);                   /* sizeof(zenv_config): lets a binding check its mirror */

/* Host layout sampler = Engine.reset()'s random half for env.seed(seed); reset():
 * aux from RandomState(seed) (TTSP_env.py:19-21 tmax / colour_match_env.py:57-68 colours),
 * layout + robot_rot from RandomState(seed+1).  robot_xyrot[3], zone_xy[Z*2], aux[Z]. */
int zenv_sample_layout(const zenv_config *cfg, int64_t seed, double *robot_xyrot,
                       double *zone_xy, int32_t *aux, int32_t *restarts);
/* FixedSeedsWrapper.reset (wrappers.py:20-23): the seed sequence drawn by
 * np.random.default_rng(rng_seed).integers(min_seed, max_seed+1) -- PCG64 + SeedSequence. */
int zenv_fixed_seed_sequence(uint64_t rng_seed, int64_t min_seed, int64_t max_seed,
                             int count, int64_t *out);

/* ---- lifecycle ---- */
/* n_env: 1 .. the largest batch whose zone_obs [N][Z][F] stays below 2^29 floats (3.5 M envs at Z = 25; measured at 1 M:
 * the same 11.9 G env-steps/s); ZENV_E_ARG beyond it -- use several handles. */
int zenv_create(const zenv_config *cfg, int n_env, int device, zenv_t **out);
int zenv_destroy(zenv_t *h);
int zenv_num_envs(const zenv_t *h);
int zenv_get_config(const zenv_t *h, zenv_config *out);

/* ---- layout bank (pre-sampled episodes in HBM) ---- */
/* Sample layouts for env seeds seed_first .. seed_first+count-1 on n_threads host threads
 * and upload them.  Replaces the per-episode XML rebuild of Engine.reset(). */
int zenv_bank_build(zenv_t *h, int64_t seed_first, int count, int n_threads);
/* Same for an arbitrary list of env seeds (slot j <-> seeds[j]). */
int zenv_bank_build_seeds(zenv_t *h, const int64_t *seeds, int count, int n_threads);
/* Upload caller-provided layouts: robot_xyrot [S,3], zone_xy [S,Z,2], aux [S,Z] (may be NULL
 * for TSP), seeds [S]. */
int zenv_bank_set(zenv_t *h, const double *robot_xyrot, const double *zone_xy,
                  const int32_t *aux, const int64_t *seeds, int count);
int zenv_bank_size(const zenv_t *h);
/* Refill bank slots in place: slot slots[j] <- the layout of env seed seeds[j] (sampled here, on n_threads host
 * threads).  Stream-ordered: it lands behind every step already enqueued and before every later one.  With
 * zenv_schedule_ring this is Engine.reset's unbounded seed stream (_seed += 1 at every reset, [not vendored]
 * Engine.reset; make_env.py:20-35 make_test_env never runs out of maps): once env i has taken episode k from its ring,
 * the host puts episode k + depth into the slot that held it. */
int zenv_bank_update(zenv_t *h, const int32_t *slots, const int64_t *seeds, int count, int n_threads);

/* ---- layouts sampled on the device (K20) ----
 * The sampler of zenv_sample_layout, compiled a second time from ONE source (csrc/layout_sampler.hpp) for the host and
 * for gfx950: integer MT19937 and IEEE float64 add / mul / compare only, so both give the host sampler's bits.  On the
 * device one wave samples one env seed straight into its bank slot; only the seeds cross the bus.
 *
 * A device wave gives up after ZENV_DEVICE_RESTARTS restarts of the rejection sampler (the host's limit is the
 * reference's 10000) and reports the seed ZENV_SAMPLE_UNFINISHED; a seed outside [0, 2^32 - 2] (Engine.seed +
 * Engine.reset's `_seed += 1`) is reported ZENV_SAMPLE_SEED_RANGE.  In both cases the slot keeps what it held.  The
 * reports -- (slot, seed, code), all of them counted, the first ZENV_SAMPLE_STATUS_CAP listed -- wait on the device for
 * zenv_sample_status; the synchronous builders read them themselves.
 *
 * Every device-sampling call (zenv_bank_build_device, _build_seeds_device, zenv_bank_update_device, zenv_ring_stream,
 * zenv_ring_refill) answers ZENV_E_STATE on a TimedTSP handle -- its deadlines are int(beta * num_steps) with beta
 * through the host libm's log, which the device's math library does not reproduce bit for bit -- and on a
 * solver-ordered handle, whose bank rows need zenv_route_ranks.  Both stay on the host path -- unless a TimedTSP
 * handle opts in with zenv_timed_layouts_device (below), or a solver-ordered one with zenv_order_routes_device. */
#define ZENV_DEVICE_RESTARTS 256
#define ZENV_SAMPLE_STATUS_CAP 1024
enum { ZENV_SAMPLE_UNFINISHED = 1, ZENV_SAMPLE_SEED_RANGE = 2 };
/* zenv_sample_layout through the shared source, compiled for the host (10000 restarts): same arguments, same results,
 * usable without a GPU.  TimedTSP configs: ZENV_E_ARG. */
int zenv_sample_layout_shared(const zenv_config *cfg, int64_t seed, double *robot_xyrot,
                              double *zone_xy, int32_t *aux, int32_t *restarts);
/* ---- TimedTSP layouts on the device: an opt-in ----
 * The shared source draws the deadlines int(beta(beta_a, beta_b) * num_steps) through csrc/det_log.hpp: a faithfully
 * rounded log (error below 1 ulp) written once for x86 and gfx950, and IEEE division and square root.  Host and device
 * instantiations agree bit for bit; against numpy's stream (the host libm's log) a deadline can differ by one step where
 * beta * num_steps lands within a few ulps of an integer -- none does over the seeds the tests pin.  A caller who needs
 * numpy's stream by definition keeps zenv_sample_layout / zenv_bank_build*.
 *
 * zenv_sample_layout_timed: zenv_sample_layout_shared for TimedTSP configs (same arguments and seed rules; usable
 * without a GPU).  ZENV_E_ARG for another task, and unless beta_a > 1 and beta_b > 1 (numpy's other branch, Joehnk's
 * algorithm, is not implemented by either sampler). */
int zenv_sample_layout_timed(const zenv_config *cfg, int64_t seed, double *robot_xyrot,
                             double *zone_xy, int32_t *aux, int32_t *restarts);
/* While enabled, the five device-sampling calls accept this TimedTSP handle (goal-conditioned ones included): its bank is
 * then defined by zenv_sample_layout_timed.  What the device gives up on is finished by that sampler's host instantiation,
 * and zenv_bank_update on the handle samples with it too, so a bank never mixes the two definitions.  ZENV_E_ARG on a
 * handle of another task, and unless beta_a > 1 and beta_b > 1. */
int zenv_timed_layouts_device(zenv_t *h, int enable);
/* Test hook: out[i] = det_log(a[i]) / det_div(a[i], b[i]) / det_sqrt(a[i]) (host arrays of n; b only for ZENV_DET_OP_DIV),
 * computed by the host's compilation of csrc/det_log.hpp or, with on_device != 0, by the device's (needs a GPU). */
enum { ZENV_DET_OP_LOG = 0, ZENV_DET_OP_DIV = 1, ZENV_DET_OP_SQRT = 2 };
int zenv_det_ops(int op, const double *a, const double *b, double *out, int n, int on_device);
/* The keepout test of the shared source compares d^2 with a threshold instead of sqrt(d^2) with a distance.  rhs[2],
 * thr[2]: the two right-hand sides A a config has ([0] a zone against the robot, (robot_keepout + placements_margin) +
 * zones_keepout; [1] a zone against a zone) and for each the double T with  sqrt(s) < A <=> s < T.  Host only. */
int zenv_layout_thresholds(const zenv_config *cfg, double *rhs, double *thr);
/* zenv_bank_build / zenv_bank_build_seeds with the layouts sampled on the device.  Synchronous: the new bank is
 * sampled into fresh buffers, seeds the device left unfinished are finished by the host sampler (identical bits, or
 * ZENV_E_LAYOUT), an out-of-range seed is ZENV_E_ARG; on any error the previous bank stays in place.  The schedule is
 * treated as zenv_bank_build treats it. */
int zenv_bank_build_device(zenv_t *h, int64_t seed_first, int count);
int zenv_bank_build_seeds_device(zenv_t *h, const int64_t *seeds, int count);
/* zenv_bank_update with 12 bytes per layout over the bus.  Asynchronous and stream-ordered; slots the device could not
 * fill keep their contents and are reported by zenv_sample_status. */
int zenv_bank_update_device(zenv_t *h, const int32_t *slots, const int64_t *seeds, int count);
/* Engine.reset's unbounded seed stream without the host: builds an N x depth bank on the device (slot i*depth + j <-
 * seed0[i] + j, synchronous like zenv_bank_build_device), lays the ring schedule first[i] = i*depth over it and keeps
 * seed0 [N] on the device.  Episode k of env i is then the layout of env seed seed0[i] + k as long as
 * zenv_ring_refill runs at least once per `depth` episodes of an env (the ring guard of zenv_schedule_ring holds).  An
 * explicit zenv_reset takes a map from the ring as an auto-reset does and the guard does not count it, so refill after
 * it too. */
int zenv_ring_stream(zenv_t *h, const int64_t *seed0, int32_t depth);
/* Bring every ring back ahead of its env: slot first[i] + j must hold episode e_j, the smallest e >= the env's
 * episode index with e mod depth == j; the slots whose seed is not seed0[i] + e_j are listed on the device and sampled by
 * a launch that reads the list's length from device memory; the derived first rows are then recomputed for the whole
 * ring bank.  Asynchronous, stream-ordered, no host synchronisation, no host bookkeeping.  ZENV_E_STATE unless zenv_ring_stream made the current schedule. */
int zenv_ring_refill(zenv_t *h);
/* Synchronises, copies the device's failure list out (the first min(cap, ZENV_SAMPLE_STATUS_CAP) entries into slots /
 * seeds / codes [cap], any of which may be NULL) and clears it.  n_failed: every entry a sampling launch left
 * untouched since the last call; n_sampled_total: layouts the device has written since the handle was made. */
int zenv_sample_status(zenv_t *h, int32_t *slots, int64_t *seeds, int32_t *codes, int cap, int32_t *n_failed,
                       int64_t *n_sampled_total);
/* Synchronises and copies bank rows slot_first .. slot_first + count - 1 out (host memory; any may be NULL):
 * robot4 [count,4] (x, y, cos(rot/2), sin(rot/2)), zone_xy [count,Z,2], aux [count,Z], seeds [count], first12
 * [count,12] float32 (the derived rows: first observation, first greedy action, pad). */
int zenv_bank_read(zenv_t *h, int slot_first, int count, double *robot4, double *zone_xy, int32_t *aux,
                   int64_t *seeds, float *first12);

/* ---- episode schedule: which bank slot env i uses for its k-th episode ---- */
/* slot = (first[i] + k*stride) mod S; first == NULL -> i mod S. */
int zenv_schedule_sequential(zenv_t *h, const int32_t *first, int32_t stride);
/* Ring: env i owns the slots first[i] .. first[i] + depth - 1 and takes slot first[i] + (k mod depth) for its k-th
 * episode; the host keeps the ring ahead of the env with zenv_bank_update (or the device does, zenv_ring_stream /
 * zenv_ring_refill).  The ring is only refilled between
 * calls, so a call that could end more than `depth` episodes of an env is refused with ZENV_E_STATE (it could replay
 * maps): zenv_rollout with auto_reset and zenv_step_many(RESET_EVERY) beyond `depth` steps, zenv_collect and
 * zenv_collect_hier and zenv_collect_option beyond `depth` frames, zenv_collect_skill beyond `depth` windows. */
int zenv_schedule_ring(zenv_t *h, const int32_t *first, int32_t depth);
/* FixedSeedsWrapper semantics on device: env i draws seeds from its own PCG64 stream
 * default_rng(rng_seeds[i]).integers(min_seed, max_seed+1); the bank must hold
 * min_seed..max_seed in order (make_env.py:3-18,37-51). */
int zenv_schedule_fixed_seeds(zenv_t *h, const uint64_t *rng_seeds, int64_t min_seed,
                              int64_t max_seed);

/* ---- the hot path ---- */
/* ParallelEnv.reset (penv.py:46-50) / masked re-reset: mask uint8[N] host, NULL = all. */
int zenv_reset(zenv_t *h, const uint8_t *mask);
/* ParallelEnv.step / step_no_reset (penv.py:52-66): actions float32 [N,2]
 * (NULL = internal action buffer written by zenv_policy); auto_reset != 0 resets finished
 * envs in the same launch and returns the new episode's first observation with the terminal
 * reward/done/goal_met (penv.py:8-11).  With auto_reset == 0 a finished env is a masked
 * no-op: zero obs, reward 0, done 1 (WaitWrapper, wrappers.py:34-45); the first auto_reset != 0 step after that
 * brings it back -- reward 0, done 1 and the next episode's first observation -- as the worker's
 * `if done: obs = env.reset()` does after WaitWrapper's no-op (the fixed-length-skill loop,
 * torch_ac/algos/hier_base.py:179-183: skill_len - 1 step_no_reset calls, then one step).
 * Exception path ([not vendored] Engine.step: `except MujocoException: done = True; reward = reward_exception;
 * info['exception'] = True`): mujoco-py raises it when MuJoCo warns that qacc / qpos / qvel hold a NaN, an Inf or a
 * value beyond 1e10 (mj_checkAcc -> mjWARN_BADQACC, after which MuJoCo has reset the data to qpos0, qvel = 0).  With
 * the actuator forces clamped and a validated config the state stays finite, so the one trigger is a NaN action
 * (np.clip keeps a NaN): that step ends the episode with reward_exception, no goal test, joint state zeroed,
 * ZENV_F_EXCEPTION = 1.  The zone visit of that step's first set_mocaps() still counts (it ran before sim.step()). */
int zenv_step(zenv_t *h, const float *actions, int actions_on_device, int auto_reset);
/* An action chunk: n_steps steps of caller-supplied actions [n_steps][N][2] (host, or device memory of the handle's
 * device) -- the same results as n_steps zenv_step() calls, as ONE launch of the persistent kernel per
 * ZENV_ROLLOUT_CHUNK steps (env state in registers, a_{t+1} prefetched under step t; zone counts 5, 6, 10, 15, 20, 25 in
 * the lane layout -- other handles run the single-step launches).  Asynchronous on the handle's stream like zenv_step.
 *   ZENV_CHUNK_NO_RESET     n_steps x step_no_reset: a finished env idles as WaitWrapper's no-op (wrappers.py:34-45)
 *   ZENV_CHUNK_RESET_EVERY  n_steps x step (penv.py:52-59)
 *   ZENV_CHUNK_RESET_LAST   n_steps - 1 x step_no_reset, then one step: the fixed-length-skill loop of
 *                           main/src/torch_ac/algos/_hier_policy_opt.py:68-71 / hier_base.py:179-183 -- an env that
 *                           finishes inside the chunk waits (zero obs, reward 0, done) and comes back at the boundary
 * A NaN action takes Engine.step's exception branch as in zenv_step.  Afterwards obs / zone_obs / reward / done /
 * goal_met hold the LAST step's results; every step's reward and done flag is in ZENV_F_CHUNK_REWARD / _DONE
 * ([n_steps][N], valid until the next zenv_step_many).  The handle's action buffer (ZENV_F_ACTIONS, what zenv_step(NULL)
 * replays and snapshots keep) ends as after n_steps zenv_step calls: the last step's actions for host actions, with or
 * without zenv_host_io; untouched for device actions.  On a ring schedule RESET_EVERY is limited to `depth` steps
 * per call (ZENV_E_STATE beyond: the host refills the ring between calls). */
enum { ZENV_CHUNK_NO_RESET = 0, ZENV_CHUNK_RESET_EVERY = 1, ZENV_CHUNK_RESET_LAST = 2 };
int zenv_step_many(zenv_t *h, const float *actions, int actions_on_device, int n_steps, int reset_mode);
/* Scripted action source -> internal action buffer (or dst_device if non-NULL). */
int zenv_policy(zenv_t *h, int policy, uint64_t policy_seed, uint64_t env_index0,
                float *dst_device);
/* K closed-loop steps a_t = policy(obs_t, t); step(a_t) on the handle's stream, HIP-event
 * timed.  Default (flags 0): the persistent rollout kernel -- one launch advances every env by
 * up to ZENV_ROLLOUT_CHUNK steps with the env state in registers, publishing obs / zone_obs / reward / done /
 * goal_met to memory on every step (zone counts 5, 6, 10, 15, 20, 25; other counts use the next mode).
 * ZENV_ROLLOUT_PER_STEP: one step-kernel launch per step, the kernel of step t also emitting
 * a_{t+1} (fused action source).  ZENV_ROLLOUT_UNFUSED: per-step launches with the stand-alone
 * policy kernel before each.  Results are identical in all three.  ms_total: whole loop (events
 * on the stream); ms_step_kernel_avg (may be NULL): kernel time per step -- persistent: begin/end
 * events of every launch, summed, / steps; otherwise the mean over every event_stride-th
 * step-kernel dispatch. */
/* zenv_rollout() is SYNCHRONOUS by default: it returns when its last launch has finished (it reports their times).
 * ZENV_ROLLOUT_ASYNC: enqueue and return at once (ms_* come back as -1); the host overlaps its own work -- refilling
 * bank slots (zenv_bank_update), a policy update -- and collects with zenv_query() (1 = the stream is idle, 0 = still
 * running, < 0 error) or zenv_sync(). */
#define ZENV_ROLLOUT_UNFUSED 1
#define ZENV_ROLLOUT_PER_STEP 2
#define ZENV_ROLLOUT_ASYNC 4
#define ZENV_ROLLOUT_CHUNK 256   /* most steps one persistent launch covers */
int zenv_rollout(zenv_t *h, int steps, int policy, uint64_t policy_seed, uint64_t env_index0,
                 int auto_reset, int flags, int event_stride, float *ms_total,
                 float *ms_step_kernel_avg);
/* How many envs ONE persistent launch covers (default 65 536 = 1 024 tiles: the chip's 1 024 SIMDs each hold one env
 * wave and one stream wave; a larger batch is stepped slice by slice, every slice ZENV_ROLLOUT_CHUNK steps at a time).
 * A launch over more workgroups than are resident at once loses that placement -- one launch over 131 072 envs takes
 * 6.9 us per 65 536 env-steps against 5.3 for two launches over 65 536 each -- and a slice's per-step output (42 MB at
 * Z = 25) stays in the Infinity Cache while it is rewritten.  0: the whole batch in one launch.  Results do not
 * depend on it. */
int zenv_set_rollout_slice(zenv_t *h, int envs_per_launch);

/* ---- goal-conditioned variant: TSPNextCityEnv, main/envs/zone_envs/
 * TSP_next_city_env.py:41-109, and TimedTSPNextCityEnv, zone-goals/envs/TTSP_next_city_env.py:40-51, as the
 * vector calls of zone-goals/src/torch_ac/torch_utils/penv.py:76-99 (set_goal / needs_goal / available_goals).
 * ColourMatchNextCityEnv (zone-goals/envs/colour_match_next_city_env.py) likewise: any zone may be a goal, and
 * cycling a zone other than the goal costs 1.  After zenv_goal_enable() every env needs a goal (ZENV_F_NEED_GOAL = 1);
 * zenv_set_goals() takes int32 goals[N] from the host (-1 = leave that env alone) and fails with ZENV_E_ARG
 * when a goal zone is out of range or (TSP / TimedTSP) already visited (set_goal's assert, :86); every zenv_step() then also produces
 * shaped_reward = last_dist_to_goal - dist_to_goal (0 in the step that reaches the goal), need_next_goal
 * (goal reached, or episode over) and the available-goals mask.  zenv_rollout() is refused on such a handle;
 * the goal arrays are not part of zenv_get_state(). */
int zenv_goal_enable(zenv_t *h);
int zenv_set_goals(zenv_t *h, const int32_t *goals);
/* ColourMatchSolverEnv.solver_get_next_goal (zone-goals/envs/colour_match_solver_env.py:57-97, id ColourMatch-v2) for
 * every env of a goal-conditioned ColourMatch handle: the nearest zone that a cheapest recolouring plan has to cycle
 * (ties: lowest index) into goals[N] (host).  Feed the entries of the envs that need a goal to zenv_set_goals(). */
int zenv_solver_goals(zenv_t *h, int32_t *goals);

/* ---- solver-ordered variant: TSPOrderEnv, main/envs/TSP_order_env.py:13-113 (PointTSP-v2) ----
 * TSP handles only; call before building the bank.  The route of an episode is the bank's aux column (rank of
 * every zone in the visiting order): zenv_bank_build* fill it with zenv_route_ranks()'s tour (the solver's problem,
 * solved without OR-tools, which the reference calls at :49-50 and which is not available), zenv_bank_set takes the caller's.
 * Every zenv_step() then also yields info['shaped_reward'] (ZENV_F_SHAPED_REWARD, :63-72) and the order feature
 * of every zone (ZENV_F_ORDER_VAL, :37-47) -- the reference's (Z,7) row is [zone_obs row (6), order value].
 * Exclusive with zenv_goal_enable; zenv_rollout() is refused on such a handle (but see zenv_order_rows).
 * ZENV_F_ORDER_VAL belongs to the observation and follows it: the feature of the route as the step left it; on the
 * step that ends an episode without an auto-reset the terminal observation's; and ALL ZERO, like ZENV_F_OBS and
 * ZENV_F_ZONE_OBS, for an env that had finished before the step and was left alone (zenv_step with auto_reset 0:
 * WaitWrapper.step, main/envs/wrappers.py:34-50, returns a zero (Z,7) zone_obs, reward 0, done and an empty info, so
 * ZENV_F_SHAPED_REWARD is 0 as well) -- and with it column 6 of ZENV_F_ORDER_ROWS.  ZENV_F_ORDER_POS is state, not
 * observation: a waiting env keeps the route its last step left, which the next reset's first observation shows. */
int zenv_order_enable(zenv_t *h);
/* First observation of an episode.  Default (flags 0) = the reference's: TSPOrderEnv.reset() builds init_obs BEFORE
 * generate_route() (TSP_order_env.py:108-113), so the observation returned by reset() -- and by ParallelEnv's auto-reset,
 * penv.py:8-11 -- carries the order feature of the route the env object was left with: all zeros before the first
 * episode and after a finished one, the unvisited rest of the previous route (indexed by zone number, on the NEW map's
 * rows) after a time-limit end.  From the first step on the feature follows the new route; shaped_reward /
 * last_dist_to_goal use the new route from the start (:112).  ZENV_ORDER_FRESH_FIRST_OBS: the first observation
 * already shows the new episode's route (not what the reference does). */
#define ZENV_ORDER_FRESH_FIRST_OBS 1
int zenv_order_configure(zenv_t *h, int flags);
/* The built-in route of a layout (host only): rank[z] = position of zone z in the tour.  The problem is the one
 * TSP_Solver.get_optim_route (main/src/utils/TSP_Solver.py:24-62) hands to OR-tools -- closed tour from the robot, arc
 * cost int64(10 x distance), first solution PATH_CHEAPEST_ARC, greedy-descent local search (relocate, exchange, 2-opt,
 * or-opt) to a local optimum -- solved without the library: the same kind of tour, not its bit-exact route. */
int zenv_route_ranks(const double *robot_xy, const double *zone_xy, int num_zones, int32_t *rank);
/* ---- the tour on the device (K21) ----
 * zenv_route_ranks' tour -- the problem of TSP_Solver.get_optim_route (main/src/utils/TSP_Solver.py:24-62) that
 * TSPOrderEnv.generate_route asks for at main/envs/TSP_order_env.py:49-50 -- written once for the host and for gfx950
 * (csrc/route_solver.hpp): int64 arc costs from IEEE float64 arithmetic and a correctly rounded square root, integer
 * comparisons after that, and a first-improvement search whose scans evaluate 64 candidates of the host's order at a
 * time and take the first that improves.  Both instantiations give zenv_route_ranks' ranks, element for element.
 *
 * zenv_route_ranks_shared: the host instantiation, usable without a GPU (TSP_Solver.py:24-62, TSP_order_env.py:49-50).
 * robot_xy[2], zone_xy[num_zones][2] -> rank[num_zones]; moves_or_null[5]: the accepted moves per operator (or-opt of
 * chains 1, 2, 3, exchange, 2-opt).  ZENV_E_ARG for a null pointer, num_zones outside [1, ZENV_MAX_ZONES], a
 * non-finite coordinate or one beyond +-1e9 (inside that box the cast of 10 x distance to int64 is defined). */
int zenv_route_ranks_shared(const double *robot_xy, const double *zone_xy, int num_zones, int32_t *rank,
                            int32_t *moves_or_null);
/* The same tour of `count` layouts on the device, one wave64 per layout (TSP_Solver.py:24-62, TSP_order_env.py:49-50):
 * robot_xy[count][2], zone_xy[count][num_zones][2] -> rank[count][num_zones], moves_or_null[count][5], all host
 * pointers.  Synchronous, on the handle's stream; any handle, and num_zones is independent of the handle's.  The
 * argument checks are zenv_route_ranks_shared's; count < 0 is ZENV_E_ARG, count == 0 does nothing. */
int zenv_route_ranks_device(zenv_t *h, const double *robot_xy, const double *zone_xy, int count, int num_zones,
                            int32_t *rank, int32_t *moves_or_null);
/* While enabled, the five device-sampling calls (zenv_bank_build_device, zenv_bank_build_seeds_device,
 * zenv_bank_update_device, zenv_ring_stream, zenv_ring_refill) accept this solver-ordered handle: the wave that
 * samples a layout solves its tour (TSP_Solver.py:24-62, TSP_order_env.py:49-50) and writes the ranks as the row's aux
 * column; a slot the device gives up on gets the host sampler's layout and the shared tour's host instantiation.
 * Unlike zenv_timed_layouts_device the switch changes no value -- the rows equal zenv_bank_build's bit for bit.  It
 * exists because a row the device (re)fills always carries the built-in tour, never ranks a caller put there with
 * zenv_bank_set: a handle whose routes come from another solver must stay off.  ZENV_E_ARG on a handle that is not
 * solver-ordered (zenv_order_enable first). */
int zenv_order_routes_device(zenv_t *h, int enable);
/* ---- the flat agent on a solver-ordered handle (K22): the results table's "Solver" row ----
 * That agent is the flat actor-critic on TSPOrderEnv's (Z, 7) rows -- the six features of the zone row plus
 * 0.5^(position in the solver's route), TSP_order_env.py:37-47 -- trained on info['shaped_reward']
 * (main/src/torch_ac/algos/base.py:159-162).  While enabled, the handle's NETWORK ROW WIDTH is 7 instead of
 * zenv_zone_feat() = 6 and every flat-network path takes such rows:
 *   zenv_mlp_load          packs zone_net_.0.weight as [h][8 + 7] (the float16 range rule holds: the order value is in [0, 1]);
 *   zenv_mlp_forward, zenv_policy(ZENV_POLICY_MLP_MEAN / _SAMPLE)   evaluate the network on the rows of the current
 *                          observation, which one launch assembles first (ZENV_F_ORDER_ROWS holds them afterwards);
 *   zenv_rollout           accepts the handle with the two MLP policies: policy, step, order step per step, no persistent
 *                          kernel; scripted policies keep the refusal;
 *   zenv_collect           accepts the handle: ZENV_F_EXP_ZONE_OBS is [T,N,Z,7], ZENV_F_EXP_REWARD is
 *                          float32(shaped_reward) as on a goal-conditioned handle, and zenv_episode_log's return sums the
 *                          env reward, its reshaped return the shaped one (base.py:169-170);
 *   zenv_ppo_init / _minibatch / _apply / _epoch   train that network (zone_w1 [h][15]);
 *   zenv_render            ZENV_RENDER_EXPERIENCE reads the recorded rows at their stride of 7 (the order value is not
 *                          drawn: the frames are what a 6-wide record of the same observations gives).
 * ZENV_F_ZONE_OBS, the stepping calls and every value the env produces are unchanged, and a handle that never calls
 * this pays nothing: the rows are assembled only where a network is about to read them.
 * Toggling drops the loaded flat network, the flat learner and the experience buffers -- all three are sized by the
 * width -- and callers load them again.  ZENV_E_STATE unless zenv_order_enable came first. */
int zenv_order_rows(zenv_t *h, int enable);

/* ---- the reference's actor network on the device ----
 * ZoneEnvModel (main/src/env_model.py:48-79) + the actor of ACModel (flat_model.py:24-37,
 * policy_network.py:12-53, Box action space), evaluated on bf16 MFMA with float32 accumulation from
 * the handle's own obs / zone_obs buffers.  Pointers are host float32 tensors in the state_dict's
 * layout (row-major [out][in]); F = zenv_zone_feat(cfg).  h_dim <= 191 (the reference uses 185). */
enum {
    ZENV_MLP_BF16 = 0,  /* bf16 MFMA, float32 accumulation: ~20x faster, mu / std within 4e-2 of the reference's float32 */
    ZENV_MLP_F32 = 1,   /* float32 throughout (f32 MFMA / FMA): mu / std / value within 1e-5 of the reference's torch float32 --
                         * the mode in which evaluate() with a checkpoint reproduces the reference's arithmetic */
    ZENV_MLP_BF16X3 = 2, /* the two zone layers -- 96 % of the arithmetic -- as three bf16 products per k-step on hi / lo split
                         * operands (16 significant bits, float32's range), float32 accumulation, the per-env head on the
                         * float32 matrix instruction: within 2e-5 of torch float32 (measured: up to 1.1e-5) at a third of
                         * ZENV_MLP_F32's time */
    ZENV_MLP_F16X3 = 3, /* the same with float16 halves (22 significant bits: within 3e-6 of torch float32, float32's own
                         * rounding noise) on every layer -- the fastest of the float32-grade modes (0.30 of ZENV_MLP_F32).  float16's range applies to every
                         * operand: weights of 32 768 or more are refused by zenv_mlp_load (ZENV_E_RANGE); an input or
                         * activation that reaches 65 520 is caught on the device and reported as ZENV_E_RANGE by the next
                         * call that waits for it (zenv_get*, zenv_sync, zenv_rollout, zenv_step_results).
                         * Batches too small for the matrix kernel (< 2 048 envs) run the float32 vector kernel in both. */
    ZENV_MLP_F16 = 4    /* ZENV_MLP_BF16's two kernels with float16 operands (one product per k-step, float32 accumulation): 5 %
                         * slower than bf16 (the wider multipliers draw more power), 11 significant bits instead of 8 -- mu / std within 1e-3 of the reference's float32
                         * (bf16: within 4e-2 by contract, ~4e-3 measured).  float16's range is guaranteed, not assumed:
                         * zenv_mlp_load refuses weights of 65 504 or more and weights whose zone-layer activations could
                         * leave the range for observations up to 64 (a bound over the rows' absolute sums: ZENV_E_RANGE, use
                         * ZENV_MLP_BF16 or a split mode); the head kernel watches its own activations, and the zone kernel
                         * the observations' magnitude, at run time (ZENV_E_RANGE from the next call that waits). */
};
typedef struct zenv_mlp_weights {
    int32_t h_dim;
    int32_t precision;              /* ZENV_MLP_* */
    const float *zone_w1, *zone_b1; /* env_model.zone_net_.0  [h, 8+F], [h]   input = [obs, zone row] */
    const float *zone_w2, *zone_b2; /* env_model.zone_net_.2  [h, h],   [h] */
    const float *zone_w3, *zone_b3; /* env_model.zone_net_.4  [h, h],   [h] */
    const float *comb_w, *comb_b;   /* env_model.combine_net_ [h, 8+h], [h]   input = [obs, zone_emb] */
    const float *enc_w, *enc_b;     /* actor.enc_.0.0         [h, h],   [h] */
    const float *mu_w, *mu_b;       /* actor.mu_              [2, h],   [2] */
    const float *std_w, *std_b;     /* actor.std_             [2, h],   [2] */
    /* critic of flat_model.ACModel (:43-47, non-distributional): all four NULL = no value head */
    const float *critic_w1, *critic_b1; /* critic.0           [h, h],   [h] */
    const float *critic_w2, *critic_b2; /* critic.2           [1, h],   [1]   (distributional: critic_mu) */
    /* distributional critic (ACModel(distributional_value=True), flat_model.py:35-41,57-60): both non-NULL ->
     * value = critic_mu(relu(critic.0(x))) in ZENV_F_POLICY_VALUE and softplus_{beta=0.3}(critic_sigma(.)) + 1e-3 in
     * ZENV_F_POLICY_VALUE_SIGMA; collect_experiences uses the mean only (base.py:140-141,193-194) */
    const float *critic_sigma_w, *critic_sigma_b; /*         [1, h],   [1] */
} zenv_mlp_weights;
int zenv_mlp_load(zenv_t *h, const zenv_mlp_weights *w);
/* mu = 2 (sigmoid(mu_(x)) - 0.5), std = sigmoid(std_(x)) + 1e-3 of the current observations into
 * ZENV_F_POLICY_MU / ZENV_F_POLICY_STD (and value = critic(x) into ZENV_F_POLICY_VALUE).  zenv_policy() / zenv_rollout() with ZENV_POLICY_MLP_* call it
 * and turn it into actions (rollouts then run one launch sequence per step). */
int zenv_mlp_forward(zenv_t *h);

/* ---- the Zone-goals hierarchical agent on the device ----
 * HighPolicyValueModel and LoPolicyValueModel (zone-goals/src/hier_policy_value_models.py:19-86) with the per-step loop
 * of zone-goals/scripts/evaluate_zone_hrl.py:52-75: an env without a goal gets one from the high level (set_goal), then
 * the low level acts towards it.  Checkpoint: status.pt's hi_model_state / lo_model_state (zone-goals/src/utils/
 * storage.py:57-61).  h = hidden size (--hidden-size, 128 by default), F = zenv_zone_feat(cfg), goal_dim = 2.
 *   high:  emb = ZoneEnvModel(obs, zone_obs) (zone-goals/src/env_model.py:48-80); for every zone z
 *          logit_z = actor.2(relu(actor.0([emb, zone_obs[z]]))); value = critic.2(relu(critic.0(emb))).  One actor serves
 *          every zone, so the weights fit any zone count.
 *   low:   goal = zone_xy[goal] / 3 (float64, then float32: TSP_next_city_env.py:86-88, colour_match_next_city_env.py:
 *          143-145); emb = ZoneEnvGoalModel(obs, goal, zone_obs) (env_model.py:82-116: ZoneEnvModel on [obs, goal]);
 *          Normal(mu, std) = PolicyNetwork(emb) (policy_network.py:40-53); value = critic.2(relu(critic.0(emb))).
 * Host float32 tensors in the state_dict's layout (row-major [out][in]); each critic is optional (all four of it NULL =
 * no value output, 0 is written).  These weights are separate from zenv_mlp_load's: loading one leaves the other. */
typedef struct zenv_hier_weights {
    int32_t h_dim;                        /* 1 .. 191 */
    int32_t precision;                    /* ZENV_MLP_F32 only: the float32 vector-ALU kernels of hier_f32.hip */
    int32_t zone_feat;                    /* F the weights were built for (zone_net_.0 has 8 + F / 10 + F columns) */
    int32_t pad;
    /* hi_model_state (HighPolicyValueModel) */
    const float *hi_zone_w1, *hi_zone_b1; /* env_model.zone_net_.0  [h, 8+F], [h]   input = [obs, zone row] */
    const float *hi_zone_w2, *hi_zone_b2; /* env_model.zone_net_.2  [h, h],   [h] */
    const float *hi_zone_w3, *hi_zone_b3; /* env_model.zone_net_.4  [h, h],   [h] */
    const float *hi_comb_w, *hi_comb_b;   /* env_model.combine_net_ [h, 8+h], [h]   input = [obs, zone_emb] */
    const float *hi_actor_w1, *hi_actor_b1; /* actor.0              [h, h+F], [h]   input = [emb, zone row] */
    const float *hi_actor_w2, *hi_actor_b2; /* actor.2              [1, h],   [1] */
    const float *hi_critic_w1, *hi_critic_b1; /* critic.0           [h, h],   [h]   (optional) */
    const float *hi_critic_w2, *hi_critic_b2; /* critic.2           [1, h],   [1]   (optional) */
    /* lo_model_state (LoPolicyValueModel) */
    const float *lo_zone_w1, *lo_zone_b1; /* env_model.zone_net_.0  [h, 10+F], [h]  input = [obs, goal, zone row] */
    const float *lo_zone_w2, *lo_zone_b2; /* env_model.zone_net_.2  [h, h],   [h] */
    const float *lo_zone_w3, *lo_zone_b3; /* env_model.zone_net_.4  [h, h],   [h] */
    const float *lo_comb_w, *lo_comb_b;   /* env_model.combine_net_ [h, 10+h], [h]  input = [obs, goal, zone_emb] */
    const float *lo_enc_w, *lo_enc_b;     /* actor.enc_.0.0         [h, h],   [h] */
    const float *lo_mu_w, *lo_mu_b;       /* actor.mu_              [2, h],   [2] */
    const float *lo_std_w, *lo_std_b;     /* actor.std_             [2, h],   [2] */
    const float *lo_critic_w1, *lo_critic_b1; /* critic.0           [h, h],   [h]   (optional) */
    const float *lo_critic_w2, *lo_critic_b2; /* critic.2           [1, h],   [1]   (optional) */
} zenv_hier_weights;
/* ZENV_E_STATE on a handle without zenv_goal_enable(); ZENV_E_ARG for h_dim outside 1 .. 191, a zone_feat other than the
 * handle's F, a precision other than ZENV_MLP_F32, a null actor tensor or a critic given in part. */
int zenv_hier_load(zenv_t *h, const zenv_hier_weights *w);
/* Both networks on the current observations, every env:
 *   ZENV_F_HIER_LOGITS / ZENV_F_HIER_VALUE  the high level (masked with ZENV_F_AVAILABLE_GOALS)
 *   ZENV_F_POLICY_MU / _STD / _VALUE        the low level towards the env's current goal (ZENV_F_GOAL); an env without
 *                                           a goal gets 0 in all three.
 * zenv_policy(ZENV_POLICY_HIER_*) runs the same two networks as one step of evaluate_zone_hrl.py:56-64, on the device:
 * every env that needs a goal (ZENV_F_NEED_GOAL) and is not finished (left alone by step_no_reset) picks one among its
 * available zones -- through the path of zenv_set_goals (last_dist_to_goal, need flag, validity), so that the step that
 * follows equals zenv_set_goals(those goals) + zenv_step(those actions) -- then the low level writes the action of
 * every env (0 for an env without a goal, e.g. one with no available zone: not an error).  The high level is evaluated
 * only for the envs that pick: ZENV_F_HIER_LOGITS / _VALUE are refreshed for those.  Randomness: Philox keyed by
 * (policy_seed, env_index0 + env, zenv_step_count) with separate streams for the goal and the action draw.  No host
 * synchronisation.  zenv_rollout() / zenv_collect() do not take these policies; zenv_collect_hier() collects training
 * experience with them. */
int zenv_hier_forward(zenv_t *h);

/* ---- the fixed-length-skills agent on the device ----
 * HighPolicyValueModel and LoPolicyValueModel (main/src/hier_policy_value_models.py:19-76) with the per-step loop of
 * main/scripts/evaluate_hier.py:48-84: every skill_len steps counted from the episode's reset the high level picks one
 * of S skills, and every step the low level acts under the current one.  DIAYN ("Skills + Diversity") evaluates with
 * the same two networks.  Checkpoint: status.pt's hi_model_state / lo_model_state (main/scripts/train_skill_planner.py:
 * 152-163).  h = hidden size (--hidden-size, 128 by default), S = n_skills, F = zenv_zone_feat(cfg).
 *   high:  emb = ZoneEnvModel(obs, zone_obs) (main/src/env_model.py, the flat agent's encoder);
 *          logits = actor.discrete_.0(relu(actor.enc_.0.0(emb))), Categorical(logits=log_softmax(logits))
 *          (policy_network.py:40-43); value = critic.2(relu(critic.0(emb))).
 *   low:   onehot = one_hot(skill, S); emb = ZoneEnvSkillModel(obs, onehot, zone_obs) (env_model.py:81-117: zone_net_ on
 *          [obs, onehot, zone row], combine_net_ on [obs, onehot, zone_emb]); x = [emb, onehot];
 *          Normal(mu, std) = PolicyNetwork(x) (mu = 2 (sigmoid(mu_) - 0.5), std = sigmoid(std_) + 1e-3);
 *          value = critic.2(relu(critic.0(x))).
 * Host float32 tensors in the state_dict's layout (row-major [out][in]); each critic is optional (all four of it NULL =
 * no value output, 0 is written).  These weights are separate from zenv_mlp_load's and zenv_hier_load's: loading one
 * set leaves the others. */
typedef struct zenv_skill_weights {
    int32_t h_dim;                        /* 1 .. 191 */
    int32_t n_skills;                     /* S: 1 .. 32 */
    int32_t zone_feat;                    /* F the weights were built for (the handle's zenv_zone_feat) */
    int32_t precision;                    /* ZENV_MLP_F32 only: the float32 vector-ALU kernels of skill_f32.hip */
    /* hi_model_state (HighPolicyValueModel) */
    const float *hi_zone_w1, *hi_zone_b1; /* env_model.zone_net_.0  [h, 8+F],   [h]  input = [obs, zone row] */
    const float *hi_zone_w2, *hi_zone_b2; /* env_model.zone_net_.2  [h, h],     [h] */
    const float *hi_zone_w3, *hi_zone_b3; /* env_model.zone_net_.4  [h, h],     [h] */
    const float *hi_comb_w, *hi_comb_b;   /* env_model.combine_net_ [h, 8+h],   [h]  input = [obs, zone_emb] */
    const float *hi_enc_w, *hi_enc_b;     /* actor.enc_.0.0         [h, h],     [h]  input = emb */
    const float *hi_logit_w, *hi_logit_b; /* actor.discrete_.0      [S, h],     [S] */
    const float *hi_critic_w1, *hi_critic_b1; /* critic.0           [h, h],     [h]  (optional) */
    const float *hi_critic_w2, *hi_critic_b2; /* critic.2           [1, h],     [1]  (optional) */
    /* lo_model_state (LoPolicyValueModel) */
    const float *lo_zone_w1, *lo_zone_b1; /* env_model.zone_net_.0  [h, 8+S+F], [h]  input = [obs, onehot, zone row] */
    const float *lo_zone_w2, *lo_zone_b2; /* env_model.zone_net_.2  [h, h],     [h] */
    const float *lo_zone_w3, *lo_zone_b3; /* env_model.zone_net_.4  [h, h],     [h] */
    const float *lo_comb_w, *lo_comb_b;   /* env_model.combine_net_ [h, 8+S+h], [h]  input = [obs, onehot, zone_emb] */
    const float *lo_enc_w, *lo_enc_b;     /* actor.enc_.0.0         [h, h+S],   [h]  input = [emb, onehot] */
    const float *lo_mu_w, *lo_mu_b;       /* actor.mu_              [2, h],     [2] */
    const float *lo_std_w, *lo_std_b;     /* actor.std_             [2, h],     [2] */
    const float *lo_critic_w1, *lo_critic_b1; /* critic.0           [h, h+S],   [h]  input = [emb, onehot] (optional) */
    const float *lo_critic_w2, *lo_critic_b2; /* critic.2           [1, h],     [1]  (optional) */
} zenv_skill_weights;
/* ZENV_E_STATE on a goal-conditioned or solver-ordered handle; ZENV_E_ARG for h_dim outside 1 .. 191, n_skills outside
 * 1 .. 32, a zone_feat other than the handle's F, a precision other than ZENV_MLP_F32, a null actor tensor or a critic
 * given in part.  Loading allocates the per-env skill state (ZENV_F_SKILL = -1, ZENV_F_SKILL_AGE = 0 for every env). */
int zenv_skill_load(zenv_t *h, const zenv_skill_weights *w);
/* skill_len: the high level picks every skill_len steps (evaluate_hier.py:21).  200 until set; ZENV_E_ARG below 1. */
int zenv_skill_configure(zenv_t *h, int skill_len);
/* skills [N] from the host: env i gets skill skills[i] with its age restarting at 0; -1 leaves env i alone.
 * ZENV_E_ARG for a value outside -1 .. S-1 (nothing is changed then); ZENV_E_STATE before zenv_skill_load. */
int zenv_set_skills(zenv_t *h, const int32_t *skills);
/* Both networks on the current observations, every env:
 *   ZENV_F_SKILL_LOGITS / ZENV_F_SKILL_VALUE  the high level
 *   ZENV_F_POLICY_MU / _STD / _VALUE          the low level under the env's current skill (ZENV_F_SKILL); an env without
 *                                             one gets 0 in all three.
 * The skill state does not move.
 * zenv_policy(ZENV_POLICY_SKILL_*) runs the same two networks as one step of evaluate_hier.py:63-67, on the device:
 * every env whose skill is -1 or whose age has reached skill_len, and which is not finished (left alone by
 * step_no_reset), picks a skill (age 0) -- the high level is evaluated only for those, ZENV_F_SKILL_LOGITS / _VALUE are
 * refreshed for those -- then the low level writes the action of every env (0 for an env without a skill), and the age
 * of every unfinished env goes up by one.  With the reset clearing the state this is `i % skill_len == 0`, i counted
 * from the episode's reset.  Randomness: Philox keyed by (policy_seed, env_index0 + env, zenv_step_count) with separate
 * streams for the skill and the action draw.  No host synchronisation.  zenv_rollout() refuses these policies
 * (ZENV_E_ARG); zenv_collect() takes none (it runs the flat network). */
int zenv_skill_forward(zenv_t *h);

/* ---- the variable-length Options agent on the device ----
 * HighPolicyValueModel and LoPolicyValueModel of options/src/hier_policy_value_models.py with the per-step loop of
 * options/scripts/evaluate_hier.py:55-84.  The networks are the skill planner's above, except that the low level's
 * PolicyNetwork has action_dim + 1 = 3 outputs: the third component of its sample decides whether the skill ends.
 * There is no skill_len.  Checkpoint: status.pt's hi_model_state / lo_model_state.
 * The members, their shapes and their checks are zenv_skill_weights' (h 1 .. 191, S 1 .. 32, ZENV_MLP_F32 only, plain
 * task handles only, each critic optional), except for the four tensors marked below. */
typedef struct zenv_option_weights {
    int32_t h_dim;                        /* 1 .. 191 */
    int32_t n_skills;                     /* S: 1 .. 32 */
    int32_t zone_feat;                    /* F the weights were built for (the handle's zenv_zone_feat) */
    int32_t precision;                    /* ZENV_MLP_F32 only: the float32 vector-ALU kernels of option_f32.hip */
    /* hi_model_state (HighPolicyValueModel) */
    const float *hi_zone_w1, *hi_zone_b1; /* env_model.zone_net_.0  [h, 8+F],   [h] */
    const float *hi_zone_w2, *hi_zone_b2; /* env_model.zone_net_.2  [h, h],     [h] */
    const float *hi_zone_w3, *hi_zone_b3; /* env_model.zone_net_.4  [h, h],     [h] */
    const float *hi_comb_w, *hi_comb_b;   /* env_model.combine_net_ [h, 8+h],   [h] */
    const float *hi_enc_w, *hi_enc_b;     /* actor.enc_.0.0         [h, h],     [h] */
    const float *hi_logit_w, *hi_logit_b; /* actor.discrete_.0      [S, h],     [S] */
    const float *hi_critic_w1, *hi_critic_b1; /* critic.0           [h, h],     [h]  (optional) */
    const float *hi_critic_w2, *hi_critic_b2; /* critic.2           [1, h],     [1]  (optional) */
    /* lo_model_state (LoPolicyValueModel) */
    const float *lo_zone_w1, *lo_zone_b1; /* env_model.zone_net_.0  [h, 8+S+F], [h] */
    const float *lo_zone_w2, *lo_zone_b2; /* env_model.zone_net_.2  [h, h],     [h] */
    const float *lo_zone_w3, *lo_zone_b3; /* env_model.zone_net_.4  [h, h],     [h] */
    const float *lo_comb_w, *lo_comb_b;   /* env_model.combine_net_ [h, 8+S+h], [h] */
    const float *lo_enc_w, *lo_enc_b;     /* actor.enc_.0.0         [h, h+S],   [h] */
    const float *lo_mu_w, *lo_mu_b;       /* actor.mu_              [3, h],     [3]  rows 0-1: the action, row 2: a_2 */
    const float *lo_std_w, *lo_std_b;     /* actor.std_             [3, h],     [3] */
    const float *lo_critic_w1, *lo_critic_b1; /* critic.0           [h, h+S],   [h]  (optional) */
    const float *lo_critic_w2, *lo_critic_b2; /* critic.2           [1, h],     [1]  (optional) */
} zenv_option_weights;
/* The error codes of zenv_skill_load.  A handle holds ONE agent of the skill family: zenv_option_load drops loaded
 * skill weights (and inverse weights), zenv_skill_load drops loaded option weights; either resets the skill state
 * (ZENV_F_SKILL = -1, ZENV_F_SKILL_AGE = 0, ZENV_F_OPTION_ENDED = 0).  zenv_mlp_load's and zenv_hier_load's weights are
 * left alone.  zenv_set_skills works with either agent. */
int zenv_option_load(zenv_t *h, const zenv_option_weights *w);
/* Both networks on the current observations, every env, the state untouched (zenv_skill_forward's fields, the low level
 * under the env's current skill, zeros without one) plus ZENV_F_OPTION_TERM_MU / _STD, _TERM_ACTION = mu_2 and
 * _TERM_PROB = sigmoid(4 mu_2 - 3).
 * zenv_policy(ZENV_POLICY_OPTION_*) is one step of evaluate_hier.py:63-75 for every env, no host synchronisation:
 *  1. every unfinished env with ZENV_F_SKILL < 0 or ZENV_F_OPTION_ENDED = 1 picks a skill (age 0): the draw of
 *     ZENV_POLICY_SKILL_SAMPLE (same Philox stream, same inverse CDF), or the argmax (ties: lowest skill).  The high
 *     level runs for those envs only; ZENV_F_SKILL_LOGITS / _VALUE are refreshed for them.
 *  2. the low level of every unfinished env writes ZENV_F_POLICY_MU / _STD [N,2] (the first two components), _VALUE and
 *     the action [N,2]; SAMPLE draws the two exactly as the skill agent does (Box-Muller on words 0 and 1 of the Philox
 *     block with tag 0x4D4C50), and a_2 = mu_2 + std_2 sqrt(-2 ln u1') cos(2 pi u2') from words 2 and 3 of that block.
 *  3. prob = sigmoid(4 a_2 - 3) in float32.  SAMPLE: the option ends iff u < prob, u the uniform of word 0 of the block
 *     with tag 0x4F5054, keyed by (policy_seed, env_index0 + env, zenv_step_count) like the others.  MEAN: a_2 = mu_2,
 *     the option ends iff prob > 0.5.  The age goes up by one.
 * ZENV_F_SKILL keeps the skill the action was taken under; that the option ended is ZENV_F_OPTION_ENDED, consumed by the
 * next policy call.  A finished env (left alone by step_no_reset) idles: zeros in every output, nothing ends, its skill
 * and age stay.  zenv_rollout() refuses these policies (ZENV_E_ARG); with option weights loaded zenv_skill_forward,
 * zenv_collect_skill and ZENV_POLICY_SKILL_* answer ZENV_E_STATE as without skill weights, and so do
 * zenv_option_forward, zenv_collect_option and ZENV_POLICY_OPTION_* without option weights.  An auto-reset clears the
 * skill here (evaluate_hier.py starts every episode with cur_skill = None); inside zenv_collect_option it does not.
 * ZENV_OPTION_COMPACT=0 / 1 in the environment at zenv_option_load picks how step 1 finds its envs (diagnostic, same
 * results): 0 -- workgroup b owns envs 4 b .. 4 b + 3 and leaves when none picks (the default up to 4 096 envs); 1 -- a
 * list of the picking envs is compacted first and workgroup b owns entries 4 b .. 4 b + 3 of it (the default above). */
int zenv_option_forward(zenv_t *h);

/* DIAYN's discriminator, InverseModel (main/src/inverse_model.py): logits = combine_net(.2)(relu(combine_net(.0)(
 * [obs, zone_emb]))), zone_emb = mean over the zones of zone_net([obs, zone row]) -- the skill high level's encoder
 * followed by ReLU and an S-way head.  Host float32 tensors in the state_dict's layout; a struct of its own, so that
 * zenv_skill_weights keeps its size. */
typedef struct zenv_skill_inverse_weights {
    int32_t h_dim;                        /* must equal the loaded zenv_skill_weights' */
    int32_t n_skills;                     /* S, the same */
    int32_t zone_feat;                    /* F, the same */
    int32_t precision;                    /* ZENV_MLP_F32 only */
    const float *zone_w1, *zone_b1;       /* zone_net.0     [h, 8+F], [h]  input = [obs, zone row] */
    const float *zone_w2, *zone_b2;       /* zone_net.2     [h, h],   [h] */
    const float *zone_w3, *zone_b3;       /* zone_net.4     [h, h],   [h] */
    const float *comb_w1, *comb_b1;       /* combine_net.0  [h, 8+h], [h]  input = [obs, zone_emb] */
    const float *comb_w2, *comb_b2;       /* combine_net.2  [S, h],   [S] */
} zenv_skill_inverse_weights;
/* ZENV_E_STATE before zenv_skill_load; ZENV_E_ARG for a null tensor, a precision other than ZENV_MLP_F32, or an h_dim,
 * n_skills or zone_feat that differs from the loaded skill weights'.  A later zenv_skill_load of another shape drops
 * these weights. */
int zenv_skill_inverse_load(zenv_t *h, const zenv_skill_inverse_weights *w);

/* ---- the xy-goals hierarchical agent on the device ----
 * HighPolicyValueModel and LoPolicyValueModel of xy-goals/src/hier_policy_value_models.py:19-72 with the per-step loop
 * of xy-goals/scripts/evaluate_xy_hrl.py:48-81 (xy-goals/src/utils/hier_agent.py:38-50): every skill_len steps counted
 * from the episode's reset the high level draws a continuous goal in the plane, and every step the low level acts under
 * the current one.  The env is the plain task env: no goal zones, no shaped reward.  Checkpoint: status.pt's
 * hi_model_state / lo_model_state.  h = hidden size, F = zenv_zone_feat(cfg).
 *   high:  the flat actor-critic's network.  emb = ZoneEnvModel(obs, zone_obs); x = relu(actor.enc_.0.0(emb));
 *          goal_mu = 2 (sigmoid(actor.mu_(x)) - 0.5), goal_std = sigmoid(actor.std_(x)) + 1e-3;
 *          value = critic.2(relu(critic.0(emb))).
 *   low:   the Zone-goals low level (zenv_hier_weights' lo_* members) under another goal: emb = ZoneEnvGoalModel(obs,
 *          goal, zone_obs) on [obs, goal(2), zone row]; Normal(mu, std) = PolicyNetwork(emb); value = critic.2(relu(
 *          critic.0(emb))).  The goal is the high level's float32 sample as it stands: unclipped, not a zone centre,
 *          not divided by 3.
 * Host float32 tensors in the state_dict's layout (row-major [out][in]); each critic is optional (all four of it NULL =
 * no value output, 0 is written). */
typedef struct zenv_xy_weights {
    int32_t h_dim;                        /* 1 .. 191 */
    int32_t zone_feat;                    /* F the weights were built for (the handle's zenv_zone_feat) */
    int32_t precision;                    /* ZENV_MLP_F32 only: the float32 vector-ALU kernels of xy_f32.hip */
    int32_t pad;
    /* hi_model_state (HighPolicyValueModel) */
    const float *hi_zone_w1, *hi_zone_b1; /* env_model.zone_net_.0  [h, 8+F],  [h]  input = [obs, zone row] */
    const float *hi_zone_w2, *hi_zone_b2; /* env_model.zone_net_.2  [h, h],    [h] */
    const float *hi_zone_w3, *hi_zone_b3; /* env_model.zone_net_.4  [h, h],    [h] */
    const float *hi_comb_w, *hi_comb_b;   /* env_model.combine_net_ [h, 8+h],  [h]  input = [obs, zone_emb] */
    const float *hi_enc_w, *hi_enc_b;     /* actor.enc_.0.0         [h, h],    [h] */
    const float *hi_mu_w, *hi_mu_b;       /* actor.mu_              [2, h],    [2] */
    const float *hi_std_w, *hi_std_b;     /* actor.std_             [2, h],    [2] */
    const float *hi_critic_w1, *hi_critic_b1; /* critic.0           [h, h],    [h]  (optional) */
    const float *hi_critic_w2, *hi_critic_b2; /* critic.2           [1, h],    [1]  (optional) */
    /* lo_model_state (LoPolicyValueModel) */
    const float *lo_zone_w1, *lo_zone_b1; /* env_model.zone_net_.0  [h, 10+F], [h]  input = [obs, goal, zone row] */
    const float *lo_zone_w2, *lo_zone_b2; /* env_model.zone_net_.2  [h, h],    [h] */
    const float *lo_zone_w3, *lo_zone_b3; /* env_model.zone_net_.4  [h, h],    [h] */
    const float *lo_comb_w, *lo_comb_b;   /* env_model.combine_net_ [h, 10+h], [h]  input = [obs, goal, zone_emb] */
    const float *lo_enc_w, *lo_enc_b;     /* actor.enc_.0.0         [h, h],    [h] */
    const float *lo_mu_w, *lo_mu_b;       /* actor.mu_              [2, h],    [2] */
    const float *lo_std_w, *lo_std_b;     /* actor.std_             [2, h],    [2] */
    const float *lo_critic_w1, *lo_critic_b1; /* critic.0           [h, h],    [h]  (optional) */
    const float *lo_critic_w2, *lo_critic_b2; /* critic.2           [1, h],    [1]  (optional) */
} zenv_xy_weights;
/* The rules of zenv_skill_load: ZENV_E_STATE on a goal-conditioned or solver-ordered handle; ZENV_E_ARG for h_dim outside
 * 1 .. 191, a zone_feat other than the handle's F, a precision other than ZENV_MLP_F32, a null actor tensor or a critic
 * given in part.  Loading leaves every env without a goal (ZENV_F_XY_GOAL_AGE = -1).  The agent shares the per-env
 * clock with the skill family, so a handle holds ONE of the three: zenv_xy_load drops loaded skill, option and inverse
 * weights, zenv_skill_load and zenv_option_load drop these.  zenv_mlp_load's and zenv_hier_load's weights are left
 * alone.  The period is zenv_skill_configure's skill_len (200 until set). */
int zenv_xy_load(zenv_t *h, const zenv_xy_weights *w);
/* goals [N][2] from the host: env i with mask[i] != 0 (mask NULL = every env) gets goals[i] with its age restarting at
 * 0.  ZENV_E_ARG for a non-finite goal under the mask (nothing is changed then); ZENV_E_STATE before zenv_xy_load.  A
 * goal left over from an episode that has ended since is cleared first. */
int zenv_set_xy_goals(zenv_t *h, const float *goals, const uint8_t *mask);
/* Both networks on the current observations, every env:
 *   ZENV_F_XY_GOAL_MU / _GOAL_STD / ZENV_F_XY_VALUE  the high level
 *   ZENV_F_POLICY_MU / _STD / _VALUE                 the low level under the env's current goal (ZENV_F_XY_GOAL); an env
 *                                                    without one gets 0 in all three.
 * The state does not move.
 * zenv_policy(ZENV_POLICY_XY_*) runs the same two networks as one step of evaluate_xy_hrl.py:62-70, on the device, with
 * no host synchronisation:
 *  1. a goal left over from an episode that has ended since is cleared;
 *  2. every env without a goal or whose age has reached skill_len, and which is not finished (left alone by
 *     step_no_reset), gets a goal with age 0: SAMPLE goal_mu + goal_std * n, MEAN goal_mu.  The high level is
 *     evaluated, and ZENV_F_XY_GOAL_MU / _GOAL_STD / ZENV_F_XY_VALUE refreshed, for those envs only;
 *  3. the low level writes the action of every env with a goal: SAMPLE a ~ Normal(mu, std), MEAN mu (0 without a goal);
 *  4. the age of every unfinished env goes up by one.
 * With the reset clearing the state this is `i % skill_len == 0`, i counted from the episode's reset.  Randomness:
 * Philox4x32-10, counter (env_index0 + env, zenv_step_count, tag), key policy_seed.  The action draw is the other
 * agents' (tag 0x4D4C50, words 0-1); the goal draw is a stream of its own, tag 0x585947: n = sqrt(-2 ln u1) (cos, sin)(
 * 2 pi u2) on words 0 and 1, formed in float32 exactly as the action's.  The policies are numbered 12 and 13: 10 and 11
 * stay unknown policies.  zenv_rollout() refuses these policies (ZENV_E_ARG) and zenv_collect() takes none; before
 * zenv_xy_load they answer ZENV_E_STATE, and with these weights loaded so do zenv_skill_forward, zenv_option_forward,
 * zenv_set_skills, ZENV_POLICY_SKILL_* and ZENV_POLICY_OPTION_*. */
int zenv_xy_forward(zenv_t *h);

/* ---- one PPO rollout on the device: BaseAlgo.collect_experiences, main/src/torch_ac/algos/base.py:131-227 ----
 * T times: (dist, value) = acmodel(obs) [zenv_mlp_forward]; action = dist.sample(); record obs, action, value,
 * log_prob, mask; step the envs (auto-reset); record the reward.  Then next_value = value(obs_T) and the GAE
 * recursion.  Needs actor AND critic weights (zenv_mlp_load).  The buffers (ZENV_F_EXP_*) stay valid until the
 * next call with a different T or zenv_destroy; self.mask is carried from call to call like the reference's, across a
 * change of T too: frame 0's mask is 1 - done of the last frame of the previous call (1 before the first call).
 * zenv_reset does not touch it -- self.mask belongs to the algorithm, not to the envs, and the reference's
 * ParallelEnv.reset() leaves BaseAlgo.mask alone as well -- so after a zenv_reset between two calls frame 0 still
 * records the previous call's last 1 - done.  ZENV_E_ARG: frames_per_proc < 1, frames_per_proc x envs >= 2^31, a
 * non-finite discount or gae_lambda, or one outside [0, 1].  On a ring schedule (zenv_schedule_ring) T is limited to
 * the ring's depth: ZENV_E_STATE beyond. */
int zenv_collect(zenv_t *h, int frames_per_proc, uint64_t policy_seed, uint64_t env_index0, float discount,
                 float gae_lambda);

/* ---- the same for the Zone-goals agent: collect_experiences of HierPolicyAlgo,
 * zone-goals/src/torch_ac/algos/_hier_policy_opt.py:9-171 (zenv_hier_load with BOTH critics, goal-conditioned handle) ----
 * T frames, each: every env that needs a goal draws one (the launches of zenv_policy(ZENV_POLICY_HIER_SAMPLE)) and opens
 * a high-level transition -- obs, the goal, the available-goals mask, the high critic's value, log_prob(goal); the low
 * level acts and frame t is recorded (ZENV_F_EXP_*, ZENV_F_LO_GOAL: obs, goal, action, per-dimension log_prob, value,
 * mask = 1 - done of the previous step, carried from call to call); the envs step with auto-reset; the low level's reward
 * is info['shaped_reward'], the env reward goes into ZENV_F_LO_ENV_REWARD and into the env's hi_reward (float32 sum).  An
 * env whose need_next_goal is set closes its open transition: its reward is hi_reward, its hi_mask 0 if done else 1, and
 * hi_reward restarts at 0.  Then
 *   low level:  GAE over frames 0 .. T-2 with no bootstrap value (frame T-1 is only the next frame of T-2):
 *               delta = r_i + discount v_{i+1} m_{i+1} - v_i, adv_i = delta + discount gae_lambda adv_{i+1} m_{i+1}
 *   high level: per env over its closed transitions, NO discount (as the reference): delta = r + V_next m - V,
 *               adv = delta + gae_lambda adv_next m, m = the transition's hi_mask, V_next = the value of the env's
 *               next transition or, when no goal was picked after the last close, V_hi(obs_T); adv_next = 0 for the last.
 * The closed transitions are handed out (ZENV_F_HI_*, *n_hi = M); the open one and hi_reward stay on the device and are
 * the first transition of the next call.  Randomness: that of zenv_policy(ZENV_POLICY_HIER_SAMPLE), keyed by
 * (policy_seed, env_index0 + env, zenv_step_count): a call is bit-identical to T rounds of zenv_policy + zenv_step.  A
 * finished env draws nothing; an env with no available zone gets no goal and action 0 (the reference would assert).
 * One host synchronisation, at the end (to learn M).  ZENV_E_ARG: frames_per_proc < 2, frames_per_proc x envs >= 2^31,
 * a non-finite discount or gae_lambda, or one outside [0, 1] (as zenv_collect and zenv_collect_skill); ZENV_E_STATE: no goals, no
 * zenv_hier_load, a critic missing, zenv_host_io on, a solver-ordered handle, more frames than a ring schedule's depth.
 * zenv_reset ends the episodes it resets:
 * the open transition of such an env is dropped (no row ever refers to it) and its hi_reward restarts at 0, so the
 * first goal of the new episode opens the env's next transition. */
int zenv_collect_hier(zenv_t *h, int frames_per_proc, uint64_t policy_seed, uint64_t env_index0, float discount,
                      float gae_lambda, int64_t *n_hi);

/* ---- the same for the fixed-length-skills agent and DIAYN: collect_experiences of HierPolicyAlgo,
 * main/src/torch_ac/algos/_hier_policy_opt.py:9-233 (zenv_skill_load with BOTH critics, plain task handle) ----
 * T frames, T a multiple of L = skill_len (zenv_skill_configure), W = T / L windows.  At frames 0, L, 2L ... EVERY env
 * picks a skill: sample_hi != 0 draws it from the high level (the draw of zenv_policy(ZENV_POLICY_SKILL_SAMPLE)),
 * sample_hi = 0 draws randint(0, S) on a Philox stream of its own; either way row env * W + k of ZENV_F_HI_* records
 * the obs, the skill, the high critic's value and log_prob(skill).  Every frame the low level acts under the env's
 * skill and frame t is recorded (ZENV_F_EXP_*, ZENV_F_LO_SKILL; mask = 1 - done of the previous step, carried from call
 * to call); the envs step -- step_no_reset, except on a window's last frame, which auto-resets: an env whose episode
 * ends inside a window idles (zero obs, reward 0, done 1) and its frames are recorded all the same.  Then
 *   diversity_t = (log_softmax(inverse(obs_{t+1}))[skill_t] - log_softmax(skill_prior_logits)[skill_t]) * (1 - done_t)
 *   lo_reward_t = reward_t + diversity_coef * diversity_t  (ZENV_F_EXP_REWARD; reward_t in ZENV_F_LO_ENV_REWARD)
 * Bootstrap: V_hi(obs_T) into ZENV_F_SKILL_VALUE (the log-softmax into ZENV_F_SKILL_LOGITS), s' drawn from the high
 * level at obs_T on a stream of its own (ZENV_F_SKILL_BOOTSTRAP, also without sample_hi), next_lo_value = V_lo(obs_T,
 * s') into ZENV_F_POLICY_VALUE.
 *   low level:  GAE over all T frames with discount, bootstrapped by next_lo_value (the advantage / return fields)
 *   high level: per env over its W windows, NO discount: ZENV_F_HI_REWARD = the window's sum of env rewards,
 *               ZENV_F_HI_MASK = next_mask = ZENV_F_EXP_MASK of the next window's first frame (the carried mask for
 *               the last), delta = reward + V_next * next_mask - V, adv = delta + gae_lambda * adv_next * next_mask
 * ZENV_F_HI_COUNT = W for every env.  Afterwards ZENV_F_SKILL holds the last window's skill with ZENV_F_SKILL_AGE = L,
 * so the next zenv_policy(ZENV_POLICY_SKILL_*) picks at once.  Randomness: keyed by (policy_seed, env_index0 + env,
 * zenv_step_count); with sample_hi a call is bit-identical to T rounds of zenv_policy(ZENV_POLICY_SKILL_SAMPLE) +
 * zenv_step with auto_reset on each window's last frame only.  No host synchronisation.  skill_prior_logits: float32
 * [S] host memory, the learned skill prior (read during the call); it may be NULL without inverse weights.
 * ZENV_E_ARG: T < 1 or not a multiple of L, T x envs >= 2^31, a non-finite discount / gae_lambda / diversity_coef, a discount or
 * gae_lambda outside [0, 1], a null or non-finite prior while inverse weights are loaded, diversity_coef != 0 without
 * them.  ZENV_E_STATE: no zenv_skill_load, a critic missing, zenv_host_io on, a goal-conditioned or solver-ordered
 * handle, more windows (T / L) than a ring schedule's depth. */
int zenv_collect_skill(zenv_t *h, int frames_per_proc, uint64_t policy_seed, uint64_t env_index0, float discount,
                       float gae_lambda, float diversity_coef, const float *skill_prior_logits, int sample_hi);

/* ---- the same for the variable-length Options agent: collect_experiences of
 * options/src/torch_ac/algos/_hier_policy_opt.py:10-205 (zenv_option_load with BOTH critics, plain task handle) ----
 * T frames, each in this order:
 *  1. every unfinished env with ZENV_F_SKILL < 0 or ZENV_F_OPTION_ENDED = 1 picks a skill -- the launches of
 *     zenv_policy(ZENV_POLICY_OPTION_SAMPLE), in either ZENV_OPTION_COMPACT form -- and opens a high-level transition:
 *     the obs, the skill, the high critic's value and log_softmax(logits)[skill];
 *  2. the low level acts for every env and frame t is recorded: ZENV_F_EXP_* (obs, the action [T,N,2], its
 *     per-dimension log_prob [T,N,2], value, mask = 1 - done of the previous step, carried from call to call),
 *     ZENV_F_LO_SKILL (-1 for an env that idled), ZENV_F_LO_TERM_ACTION / _TERM_LOG_PROB (the third component of the
 *     reference's _action and lo_log_probs) and ZENV_F_LO_OPTION_ENDED (the termination draw);
 *  3. the envs step with auto-reset, on every frame; ZENV_F_EXP_REWARD and ZENV_F_LO_ENV_REWARD both hold the env
 *     reward, and hi_reward[env] += reward (a float32 sum);
 *  4. an env whose option ended closes its open transition with reward hi_reward and hi_mask = 0 if done else 1;
 *     hi_reward restarts at 0 whether or not a transition was open.
 * THE SKILL SURVIVES THE AUTO-RESET, as in the reference's training loop: cur_skills[j] is cleared by the termination
 * draw alone, so an option, its open transition and its hi_reward run across an episode boundary, and
 * ZENV_F_SKILL_AGE keeps counting.  This is the collector's rule only: zenv_policy(ZENV_POLICY_OPTION_*) keeps the
 * evaluation loop's (evaluate_hier.py starts every episode with cur_skill = None), where an auto-reset clears the
 * skill.  A call is therefore bit-identical to T rounds of zenv_policy(ZENV_POLICY_OPTION_SAMPLE) + zenv_step with
 * auto-reset in which zenv_set_skills puts back, after every step, the skill of each env that was done and whose
 * option did not end (up to ZENV_F_SKILL_AGE, which zenv_set_skills restarts).  Then
 *   bootstrap:  V_hi(obs_T) of every env into ZENV_F_SKILL_VALUE (the log-softmax into ZENV_F_SKILL_LOGITS); nothing
 *               is picked
 *   low level:  GAE with discount over frames 0 .. T-2 and no bootstrap value, as zenv_collect_hier; advantage and
 *               return of frame T-1 are 0
 *   high level: per env over the transitions closed in this call, NO discount: delta = r + V_next m - V,
 *               adv = delta + gae_lambda adv_next m, m = the transition's own hi_mask, V_next = the value of the env's
 *               next transition (which may be the one still open) or, when none was picked after the last close,
 *               V_hi(obs_T); adv_next = 0 for the last.
 * The closed transitions are handed out env-major (ZENV_F_HI_OBS / _ZONE_OBS / _ACTION / _VALUE / _LOG_PROB /
 * _ADVANTAGE / _RETURN / _REWARD / _MASK, ZENV_F_HI_COUNT, *n_hi = M; M = 0 is a valid result).  The open one and
 * hi_reward stay on the device and are the env's first transition of the next call: THE CARRY ASSUMES THAT THE HANDLE
 * IS NOT STEPPED BY OTHER MEANS BETWEEN TWO CALLS.  At the start of a call the skill state is brought up to date once,
 * as the policy does; an env that enters without a skill has its open transition dropped (and hi_reward 0).  A
 * termination without an open transition -- a skill planted by zenv_set_skills or picked by zenv_policy -- closes
 * nothing.  zenv_reset drops the open transition of the envs it resets and zeroes their hi_reward (their skill is
 * cleared as well); zenv_option_load and zenv_skill_load drop every open transition.  A finished env at frame 0 draws
 * nothing until the frame's auto-reset brings it back.  Randomness: exactly the policy's, Philox keyed by
 * (policy_seed, env_index0 + env, zenv_step_count) with the same tags.  One host synchronisation, to learn M.
 * ZENV_E_ARG: frames_per_proc < 2, frames_per_proc x envs >= 2^31, a non-finite discount or gae_lambda, or one
 * outside [0, 1].  ZENV_E_STATE: no option weights (loaded skill weights included), a critic missing, zenv_host_io on,
 * a goal-conditioned or solver-ordered handle, more frames than a ring schedule's depth. */
int zenv_collect_option(zenv_t *h, int frames_per_proc, uint64_t policy_seed, uint64_t env_index0, float discount,
                        float gae_lambda, int64_t *n_hi);

/* ---- the same for the xy-goals agent: collect_experiences of xy-goals/src/torch_ac/algos/_hier_policy_opt.py:10-192
 * (zenv_xy_load with BOTH critics, plain task handle) ----
 * T frames, T a multiple of L = skill_len (zenv_skill_configure), W = T / L windows.  At frames 0, L, 2L ... EVERY env
 * picks a goal, whatever it held before: goal_mu + goal_std * n, the draw of zenv_policy(ZENV_POLICY_XY_SAMPLE); row
 * env * W + k of the high-level rows records the obs (ZENV_F_HI_OBS / _ZONE_OBS), the goal (ZENV_F_HI_GOAL), the high
 * critic's value and Normal(goal_mu, goal_std).log_prob(goal) summed over the two dimensions (ZENV_F_HI_LOG_PROB).
 * Every frame the low level acts under the env's goal and frame t is recorded (ZENV_F_EXP_*, ZENV_F_LO_GOAL; mask = 1 -
 * done of the previous step, carried from call to call) with
 *   dist_t = sqrt((goal_x - obs_t[1])^2 + (goal_y - obs_t[2])^2)    (ZENV_F_LO_GOAL_DIST; float32, as torch rounds it)
 * on the observation the action is taken on; the envs step -- step_no_reset, except on a window's last frame, which
 * auto-resets: an env whose episode ends inside a window idles (zero obs, reward 0, done 1) and its frames are
 * evaluated and recorded all the same.  Then
 *   lo_reward_t = (dist_t - dist_{t+1}) * mask_{t+1} * ((t + 1) % L != 0)   (ZENV_F_EXP_REWARD; 0 at frame T - 1, where
 *                 the reference's factor is (T % L != 0) = 0); the env reward (ZENV_F_LO_ENV_REWARD) takes no part
 * Bootstrap: V_hi(obs_T) into ZENV_F_XY_VALUE (its Normal into ZENV_F_XY_GOAL_MU / _GOAL_STD), g' drawn from it on a
 * stream of its own (tag 0x585942; ZENV_F_XY_BOOTSTRAP_GOAL), next_lo_value = V_lo(obs_T, g') into
 * ZENV_F_POLICY_VALUE (ZENV_F_POLICY_MU / _STD: the low level under g').  The goal and its clock are left as the last
 * window left them.
 *   low level:  GAE over all T frames with discount, bootstrapped by next_lo_value (the advantage / return fields)
 *   high level: per env over its W windows, NO discount: ZENV_F_HI_REWARD = the window's sum of env rewards,
 *               ZENV_F_HI_MASK = next_mask = ZENV_F_EXP_MASK of the next window's first frame (the carried mask for
 *               the last), delta = reward + V_next * next_mask - V, adv = delta + gae_lambda * adv_next * next_mask
 * ZENV_F_HI_COUNT = W for every env.  Afterwards ZENV_F_XY_GOAL holds the last window's goal with ZENV_F_XY_GOAL_AGE =
 * L (-1 for an env the last frame reset), so the next zenv_policy(ZENV_POLICY_XY_*) picks at once.  Randomness: keyed
 * by (policy_seed, env_index0 + env, zenv_step_count); on a handle whose goals are not older than their episode's
 * windows (a fresh load) a call is bit-identical to T rounds of zenv_policy(ZENV_POLICY_XY_SAMPLE) + zenv_step with
 * auto_reset on each window's last frame only.  No host synchronisation.
 * ZENV_E_ARG: T < 1 or not a multiple of L, T x envs >= 2^31, a non-finite discount / gae_lambda or one outside
 * [0, 1].  ZENV_E_STATE: no zenv_xy_load (another agent's weights loaded included), a critic missing, zenv_host_io on,
 * a goal-conditioned or solver-ordered handle, more windows (T / L) than a ring schedule's depth. */
int zenv_collect_xy(zenv_t *h, int frames_per_proc, uint64_t policy_seed, uint64_t env_index0, float discount,
                    float gae_lambda);

/* ---- the flat actor-critic's PPO update on the device: update_parameters, main/src/torch_ac/algos/ppo.py:30-155 ----
 * Forward, loss, backward, gradient-norm clip and Adam of ACModel (flat_model.py:21-68, both critics) in float32, on
 * the samples of the handle's own ZENV_F_EXP_* buffers, recurrence 1.  Sample index i is env i / T, frame i % T: the
 * reference's [N][T] flattening (base.py:212-227); the kernels read the time-major buffers in place.  The learner's
 * parameters are separate from the acting network's: nothing here repacks zenv_mlp_load's images (read the parameters
 * back and load them to act with them).  Every reduction runs in a fixed order: the same call from the same state
 * gives the same bits.  The Zone-goals agent's two updates are zenv_hppo_* below, the xy-goals agent's two zenv_xyppo_*,
 * the fixed-length-skills agent's two zenv_skppo_*, the Options agent's two zenv_opppo_*; the updates of DIAYN's
 * inverse model and skill prior are zenv_diayn_*. */
typedef struct zenv_ppo_config {
    double lr, adam_eps;            /* torch.optim.Adam(lr, eps = adam_eps), betas 0.9 / 0.999 */
    double clip_eps, entropy_coef, value_loss_coef, max_grad_norm;
    int32_t max_batch;              /* the largest minibatch: sizes the activation workspace */
    int32_t distributional_value;   /* != 0: PPO-VD's critic (critic_mu, critic_sigma), value loss -log N(returnn) */
} zenv_ppo_config;
enum { ZENV_PPO_PARAM = 0, ZENV_PPO_GRAD = 1, ZENV_PPO_EXP_AVG = 2, ZENV_PPO_EXP_AVG_SQ = 3 };
/* The argument rules of zenv_ppo_init, on the host alone (cfg: the handle's config): ZENV_E_ARG for h_dim outside
 * 1 .. 191, a null actor tensor, a missing critic, critic_sigma_* without distributional_value or the reverse, a
 * negative or non-finite hyper-parameter, max_batch < 1, a workspace of 2^31 floats or more. */
int zenv_ppo_check(const zenv_config *cfg, const zenv_mlp_weights *init, const zenv_ppo_config *pc);
/* One device arena of float32 master parameters -- each tensor in the state_dict's row-major [out][in] layout, in
 * zenv_mlp_weights' member order (18 tensors, 20 with the distributional critic), each starting on a 256-byte
 * boundary with zeros between -- and arenas of the same shape for the gradients, exp_avg and exp_avg_sq; Adam's step
 * count starts at 0.  init->precision is not used.  A second call replaces the learner. */
int zenv_ppo_init(zenv_t *h, const zenv_mlp_weights *init, const zenv_ppo_config *pc);
/* The device pointer and element count of tensor `index` (member order) of arena `which` (ZENV_PPO_*): callers alias,
 * read and write them on the handle's stream (checkpoints, tests).  index = -1: the whole arena, padding included. */
int zenv_ppo_tensor(zenv_t *h, int which, int index, void **dev_ptr, int64_t *count);
/* The same tensor (index = -1: the whole arena) copied to / from host float32 memory, behind everything enqueued on
 * the handle's stream; both wait for the copy. */
int zenv_ppo_read(zenv_t *h, int which, int index, float *dst);
int zenv_ppo_write(zenv_t *h, int which, int index, const float *src);
int zenv_ppo_get_step(zenv_t *h, int64_t *step);
int zenv_ppo_set_step(zenv_t *h, int64_t step);
/* Forward, loss and backward on the samples idx[0 .. count) (host memory, or device memory of the handle's device):
 * the gradients are left in their arena, the six statistics in row 0 of ZENV_F_PPO_STATS; apply != 0 runs
 * zenv_ppo_apply behind it.  Asynchronous on the handle's stream.  ZENV_E_STATE without zenv_ppo_init or without
 * experience on the handle (zenv_collect); ZENV_E_ARG for count outside 1 .. max_batch and for a host index outside
 * [0, N T).  A device-resident index outside that range is never dereferenced: its sample is dropped (it adds nothing
 * to the loss; the means still divide by count) and the next call that waits for the device (zenv_get*, zenv_sync ...)
 * answers ZENV_E_ARG once. */
int zenv_ppo_minibatch(zenv_t *h, const int32_t *idx, int count, int idx_on_device, int apply);
/* clip_grad_norm_(max_grad_norm) and one step of torch's Adam on whatever the gradient arena holds (the arena itself
 * keeps the unclipped gradients). */
int zenv_ppo_apply(zenv_t *h);
/* The minibatches order[k B : (k + 1) B], B = batch_size, in sequence, the last one short: each forward, backward,
 * clip and Adam, with no host synchronisation; minibatch k's statistics in row k of ZENV_F_PPO_STATS. */
int zenv_ppo_epoch(zenv_t *h, const int32_t *order, int total, int batch_size, int on_device);

/* ---- the flat actor-critic's A2C update on the device: update_parameters, main/src/torch_ac/algos/a2c.py:21-93 ----
 * A2CAlgo for recurrence 1 on the network and the ZENV_F_EXP_* buffers of zenv_ppo_*, a learner of its own that a handle
 * may hold beside the PPO one: float32 master parameters, their gradients and RMSprop's square_avg.  A2C takes ONE step
 * on the loss averaged over all N T frames of a collection,
 *   loss = -mean(log_prob(a) advantage) - entropy_coef mean(entropy) + value_loss_coef mean((value - returnn)^2),
 * log_prob(a) summed over the action's two components (as ppo.py:73-76 sums them; a2c.py:53 as written multiplies
 * [B, 2] by [B] and raises for the two-component policy), the entropy's mean over frames x 2, no ratio, no clip.  N T is
 * usually far beyond an activation workspace, so the gradient is accumulated over chunks of at most max_batch frames:
 * every chunk's means divide by the update's total, chunk 0 overwrites the gradient arena and every later chunk adds
 * onto it, within a chunk in the fixed order of the PPO learner's partial sums and across chunks in the order of the
 * calls.  The statistics accumulate the same way and are finalised by the step.  The same calls from the same state
 * give the same bits. */
typedef struct zenv_a2c_config {
    double lr, rmsprop_alpha, rmsprop_eps;      /* torch.optim.RMSprop(lr, alpha, eps), momentum 0, not centered */
    double entropy_coef, value_loss_coef, max_grad_norm;
    int32_t max_batch;                          /* chunk size: sizes the activation workspace */
} zenv_a2c_config;
enum { ZENV_A2C_PARAM = 0, ZENV_A2C_GRAD = 1, ZENV_A2C_SQUARE_AVG = 2 };
/* zenv_ppo_check's rules on the host alone: ZENV_E_ARG for h_dim outside 1 .. 191, a null actor tensor, a missing critic,
 * a negative or non-finite hyper-parameter, max_batch < 1, a workspace of 2^31 floats or more -- and for critic_sigma_*
 * tensors: A2CAlgo has no distributional branch. */
int zenv_a2c_check(const zenv_config *cfg, const zenv_mlp_weights *init, const zenv_a2c_config *ac);
/* Three arenas in zenv_ppo_init's layout (18 tensors, zenv_mlp_weights' member order, 256-byte boundaries, zeros
 * between): parameters, gradients, square_avg; the step count starts at 0.  On a handle with zenv_order_rows on the
 * learner trains on the (Z, 7) rows.  A second call replaces the learner; zenv_ppo_* is not touched. */
int zenv_a2c_init(zenv_t *h, const zenv_mlp_weights *init, const zenv_a2c_config *ac);
/* as zenv_ppo_tensor / _read / _write / _get_step / _set_step, `which` one of ZENV_A2C_* */
int zenv_a2c_tensor(zenv_t *h, int which, int index, void **dev_ptr, int64_t *count);
int zenv_a2c_read(zenv_t *h, int which, int index, float *dst);
int zenv_a2c_write(zenv_t *h, int which, int index, const float *src);
int zenv_a2c_get_step(zenv_t *h, int64_t *step);
int zenv_a2c_set_step(zenv_t *h, int64_t step);
/* One chunk: forward, loss and backward on the samples idx[0 .. count) (host or device memory) of an update over
 * `total` frames.  first != 0 opens the update (the gradient arena and the running statistics are overwritten), first = 0
 * adds onto them.  Asynchronous on the handle's stream.  ZENV_E_STATE without zenv_a2c_init, without zenv_collect, or for
 * first = 0 with no update open; ZENV_E_ARG for count outside 1 .. max_batch, total < count, a total other than the open
 * update's, a host index outside [0, N T).  A device-resident index out of range is dropped and reported once, as
 * zenv_ppo_minibatch does. */
int zenv_a2c_accumulate(zenv_t *h, const int32_t *idx, int count, int idx_on_device, int64_t total, int first);
/* The gradient norm, clip_grad_norm_(max_grad_norm), one step of torch's RMSprop on whatever the gradient arena holds
 * (the arena keeps the unclipped gradient), step += 1, and the five statistics into ZENV_F_A2C_STATS. */
int zenv_a2c_apply(zenv_t *h);
/* All N T frames of the last zenv_collect in index order 0 .. N T - 1 (a2c.py:_get_starting_indexes, recurrence 1) in
 * chunks of max_batch, then zenv_a2c_apply; no host synchronisation (the first call of a size uploads the index list). */
int zenv_a2c_update(zenv_t *h);

/* ---- the Zone-goals agent's two PPO updates on the device: update_lo_parameters / update_hi_parameters,
 * zone-goals/src/torch_ac/algos/_hier_policy_opt.py:214-370 ----
 * Two learners beside the flat one, each with its own four arenas, Adam step count, workspace and statistics; `level`
 * 0 is the low level (LoPolicyValueModel), 1 the high level (HighPolicyValueModel).  They read the records of the last
 * zenv_collect_hier in place:
 *   low:   the flat learner's network on [obs, goal] (10 inputs), loss and Adam.  Sample index i is env i / (T-1), frame
 *          i % (T-1) of the ZENV_F_EXP_* buffers and ZENV_F_LO_GOAL: the reference's lo_exps hold T-1 frames per env
 *          (hrl_policy_planner.py:68); frame T-1 of any buffer is never read.
 *   high:  sample index i is row i of the ZENV_F_HI_* rows, i in [0, M).  Categorical over the goals of
 *          ZENV_F_HI_ACTION_MASK (logits[~mask] = -inf), log_prob and entropy of that distribution, the same clipped
 *          policy and value losses.
 * The reference takes the gradient norm and does not clip (:272, :349): max_grad_norm = +inf is accepted here and gives
 * a clip factor of exactly 1.  The arenas' order is zenv_hier_weights' member order, parameters() order of the modules:
 * 16 tensors for the high level (hi_zone_w1 .. hi_critic_b2), 18 for the low level (lo_zone_w1 .. lo_critic_b2).
 * Neither touches the acting agent's weights: read the parameters back and zenv_hier_load them to act with them. */
/* zenv_ppo_check's rules for either level, on the host alone: ZENV_E_ARG for h_dim outside 1 .. 191, a zone_feat other
 * than zenv_zone_feat(cfg), a null tensor, a missing critic at either level, distributional_value != 0, a negative or
 * non-finite hyper-parameter (max_grad_norm = +inf excepted), max_batch < 1, a workspace of 2^31 floats or more. */
int zenv_hppo_check(const zenv_config *cfg, const zenv_hier_weights *init, const zenv_ppo_config *lo,
                    const zenv_ppo_config *hi);
/* Both learners from one set of weights (init->precision is not used).  A second call replaces them. */
int zenv_hppo_init(zenv_t *h, const zenv_hier_weights *init, const zenv_ppo_config *lo, const zenv_ppo_config *hi);
/* The flat functions with the level after the handle; their semantics are the flat functions'.  ZENV_E_ARG for a level
 * other than 0 or 1; ZENV_E_STATE without zenv_hppo_init.  The update calls answer ZENV_E_STATE unless the handle's
 * ZENV_F_EXP_* / ZENV_F_LO_* / ZENV_F_HI_* buffers hold zenv_collect_hier's records (no collect yet, or another
 * collector ran last), and level 1 when that call closed no transition (M = 0).  Statistics: ZENV_F_HPPO_LO_STATS /
 * ZENV_F_HPPO_HI_STATS.  A device-resident index outside [0, N (T-1)) (low) or [0, M) (high), and a high-level row whose
 * recorded goal is outside [0, Z) or not among its available goals (a row without any included), is never
 * dereferenced past that check: the sample is dropped as zenv_ppo_minibatch drops one, it adds nothing to the loss or to
 * any gradient, and the next call that waits for the device answers ZENV_E_ARG once. */
int zenv_hppo_tensor(zenv_t *h, int level, int which, int index, void **dev_ptr, int64_t *count);
int zenv_hppo_read(zenv_t *h, int level, int which, int index, float *dst);
int zenv_hppo_write(zenv_t *h, int level, int which, int index, const float *src);
int zenv_hppo_get_step(zenv_t *h, int level, int64_t *step);
int zenv_hppo_set_step(zenv_t *h, int level, int64_t step);
int zenv_hppo_minibatch(zenv_t *h, int level, const int32_t *idx, int count, int idx_on_device, int apply);
int zenv_hppo_apply(zenv_t *h, int level);
int zenv_hppo_epoch(zenv_t *h, int level, const int32_t *order, int total, int batch_size, int on_device);

/* ---- the xy-goals agent's two PPO updates on the device: update_hi_parameters / update_lo_parameters,
 * xy-goals/src/torch_ac/algos/_hier_policy_opt.py:195-363 ----
 * Two more learners, each with its own four arenas, Adam step count, workspace and statistics; `level` 0 is the low
 * level (LoPolicyValueModel), 1 the high level (HighPolicyValueModel).  They read the records of the last
 * zenv_collect_xy in place:
 *   low:   the Zone-goals low level's network, loss and Adam on [obs, goal] (10 inputs).  Sample index i is env i / T,
 *          frame i % T of the ZENV_F_EXP_* buffers and ZENV_F_LO_GOAL: this agent's lo_exps hold ALL T frames per env
 *          (:147-158), frame T-1 included.
 *   high:  the flat actor-critic's network (8 inputs, Normal over two dimensions) on row i of the ZENV_F_HI_* rows,
 *          i in [0, M), M = N T / skill_len.  The action is the recorded goal (ZENV_F_HI_GOAL); ZENV_F_HI_LOG_PROB is
 *          one float per row, so the ratio is exp(log_prob(goal).sum(-1) - recorded); the entropy is
 *          entropy().sum(-1).mean(): summed over the two dimensions, then the mean over rows.  The clipped policy and
 *          value losses are the other learners'.
 * The reference takes the gradient norm and does not clip: max_grad_norm = +inf is accepted and gives a clip factor of
 * exactly 1.  The arenas' order is zenv_xy_weights' member order, parameters() order of the modules: 18 tensors for the
 * high level (hi_zone_w1 .. hi_critic_b2), 18 for the low level (lo_zone_w1 .. lo_critic_b2).  Neither touches the
 * acting agent's weights: read the parameters back and zenv_xy_load them to act with them. */
/* zenv_hppo_check's rules for either level, on the host alone: ZENV_E_ARG for h_dim outside 1 .. 191, a zone_feat other
 * than zenv_zone_feat(cfg), a null tensor, a missing critic at either level, distributional_value != 0, a negative or
 * non-finite hyper-parameter (max_grad_norm = +inf excepted), max_batch < 1, a workspace of 2^31 floats or more. */
int zenv_xyppo_check(const zenv_config *cfg, const zenv_xy_weights *init, const zenv_ppo_config *lo,
                     const zenv_ppo_config *hi);
/* Both learners from one set of weights (init->precision is not used).  A second call replaces them. */
int zenv_xyppo_init(zenv_t *h, const zenv_xy_weights *init, const zenv_ppo_config *lo, const zenv_ppo_config *hi);
/* The flat functions with the level after the handle; their semantics are the flat functions'.  ZENV_E_ARG for a level
 * other than 0 or 1; ZENV_E_STATE without zenv_xyppo_init.  The update calls answer ZENV_E_STATE unless the handle's
 * ZENV_F_EXP_* / ZENV_F_LO_* / ZENV_F_HI_* buffers hold a completed zenv_collect_xy's records (no collect yet, or another
 * collector ran last); zenv_hppo_* refuses these records in turn.  Statistics: ZENV_F_XYPPO_LO_STATS /
 * ZENV_F_XYPPO_HI_STATS.  A host index outside [0, N T) (low) or [0, M) (high) is ZENV_E_ARG; a device-resident one is
 * never dereferenced: the sample is dropped as zenv_ppo_minibatch drops one, it adds nothing to the loss or to any
 * gradient, and the next call that waits for the device answers ZENV_E_ARG once. */
int zenv_xyppo_tensor(zenv_t *h, int level, int which, int index, void **dev_ptr, int64_t *count);
int zenv_xyppo_read(zenv_t *h, int level, int which, int index, float *dst);
int zenv_xyppo_write(zenv_t *h, int level, int which, int index, const float *src);
int zenv_xyppo_get_step(zenv_t *h, int level, int64_t *step);
int zenv_xyppo_set_step(zenv_t *h, int level, int64_t step);
int zenv_xyppo_minibatch(zenv_t *h, int level, const int32_t *idx, int count, int idx_on_device, int apply);
int zenv_xyppo_apply(zenv_t *h, int level);
int zenv_xyppo_epoch(zenv_t *h, int level, const int32_t *order, int total, int batch_size, int on_device);

/* ---- the fixed-length-skills agent's two PPO updates on the device: update_lo_parameters / update_hi_parameters,
 * main/src/torch_ac/algos/_hier_policy_opt.py:265-419 ----
 * Two more learners, each with its own four arenas, Adam step count, workspace and statistics; `level` 0 is the low
 * level (LoPolicyValueModel), 1 the high level (HighPolicyValueModel), S = init->n_skills.  They read the records of the
 * last zenv_collect_skill in place (DIAYN collects with the same call; its inverse model's and skill prior's updates
 * are zenv_diayn_* below):
 *   low:   the flat learner's loss (a recorded log_prob per action component, the entropy's mean over both) on the
 *          network of [obs, onehot(skill)] (8 + S inputs) whose actor.enc_.0.0 and critic.0 read [emb, onehot].  Sample
 *          index i is env i / T, frame i % T of the ZENV_F_EXP_* buffers, all T frames; the skill is ZENV_F_LO_SKILL of
 *          that frame and the one-hot is formed from it on the fly.
 *   high:  the flat encoder and critic under logits = actor.discrete_.0(relu(actor.enc_.0.0(emb))),
 *          Categorical(logits = log_softmax(logits)) over the S skills, unmasked, on row i of the ZENV_F_HI_* rows,
 *          i in [0, M), M = N T / skill_len.  The action is the recorded skill (ZENV_F_HI_ACTION); ZENV_F_HI_LOG_PROB is
 *          one float per row; the entropy is the mean over rows.  The clipped policy and value losses are the other
 *          learners'.
 * The reference takes the gradient norm and does not clip: max_grad_norm = +inf is accepted and gives a clip factor of
 * exactly 1.  The arenas' order is zenv_skill_weights' member order, parameters() order of the modules: 16 tensors for
 * the high level (hi_zone_w1 .. hi_critic_b2), 18 for the low level (lo_zone_w1 .. lo_critic_b2).  Neither touches the
 * acting agent's weights: read the parameters back and zenv_skill_load them to act with them. */
/* zenv_hppo_check's rules for either level, on the host alone: ZENV_E_ARG for h_dim outside 1 .. 191, n_skills outside
 * 1 .. 32, a zone_feat other than zenv_zone_feat(cfg), a null tensor, a missing critic at either level,
 * distributional_value != 0, a negative or non-finite hyper-parameter (max_grad_norm = +inf excepted), max_batch < 1, a
 * workspace of 2^31 floats or more. */
int zenv_skppo_check(const zenv_config *cfg, const zenv_skill_weights *init, const zenv_ppo_config *lo,
                     const zenv_ppo_config *hi);
/* Both learners from one set of weights (init->precision is not used).  A second call replaces them. */
int zenv_skppo_init(zenv_t *h, const zenv_skill_weights *init, const zenv_ppo_config *lo, const zenv_ppo_config *hi);
/* The flat functions with the level after the handle; their semantics are the flat functions'.  ZENV_E_ARG for a level
 * other than 0 or 1; ZENV_E_STATE without zenv_skppo_init.  The update calls answer ZENV_E_STATE unless the handle's
 * ZENV_F_EXP_* / ZENV_F_LO_* / ZENV_F_HI_* buffers hold a completed zenv_collect_skill's records of an agent with S skills
 * (no collect yet, or another collector ran last); zenv_hppo_* and zenv_xyppo_* refuse these records in turn.
 * Statistics: ZENV_F_SKPPO_LO_STATS / ZENV_F_SKPPO_HI_STATS.  A host index outside [0, N T) (low) or [0, M) (high) is
 * ZENV_E_ARG; a device-resident one is never dereferenced: the sample is dropped as zenv_ppo_minibatch drops one, it adds
 * nothing to the loss or to any gradient, and the next call that waits for the device answers ZENV_E_ARG once.  A
 * recorded skill outside [0, S) -- a frame's ZENV_F_LO_SKILL or a row's ZENV_F_HI_ACTION -- drops its sample the same
 * way. */
int zenv_skppo_tensor(zenv_t *h, int level, int which, int index, void **dev_ptr, int64_t *count);
int zenv_skppo_read(zenv_t *h, int level, int which, int index, float *dst);
int zenv_skppo_write(zenv_t *h, int level, int which, int index, const float *src);
int zenv_skppo_get_step(zenv_t *h, int level, int64_t *step);
int zenv_skppo_set_step(zenv_t *h, int level, int64_t step);
int zenv_skppo_minibatch(zenv_t *h, int level, const int32_t *idx, int count, int idx_on_device, int apply);
int zenv_skppo_apply(zenv_t *h, int level);
int zenv_skppo_epoch(zenv_t *h, int level, const int32_t *order, int total, int batch_size, int on_device);

/* ---- the Options agent's two PPO updates on the device: update_lo_parameters / update_hi_parameters,
 * options/src/torch_ac/algos/_hier_policy_opt.py:208-381 ----
 * Two more learners, as zenv_skppo_*'s are; `level` 0 is the low level (LoPolicyValueModel), 1 the high level
 * (HighPolicyValueModel), S = init->n_skills.  They read the records of the last zenv_collect_option in place:
 *   low:   zenv_skppo_*'s low level with a third Gaussian component: actor.mu_ / actor.std_ are [3, h] / [3], the ratio is
 *          exp(sum over the three components of log_prob - recorded), the entropy's mean is over B x 3.  Components 0-1
 *          and their log_probs are ZENV_F_EXP_ACTION / ZENV_F_EXP_LOG_PROB [slot][2]; component 2, a_2, and its log_prob
 *          are ZENV_F_LO_TERM_ACTION / ZENV_F_LO_TERM_LOG_PROB [slot].  a_2 is a third action dimension and nothing more:
 *          the termination probability sigmoid(4 a_2 - 3) and the recorded draw play no part in the loss.  Sample index
 *          i is env i / (T - 1), frame i % (T - 1): frames 0 .. T-2 of every env, frame T-1 is never read.  The skill is
 *          ZENV_F_LO_SKILL of that frame.
 *   high:  zenv_skppo_*'s high level on row i of the ZENV_F_HI_* rows, i in [0, M), M the transitions the call closed.
 *          The action is the recorded skill (ZENV_F_HI_ACTION), ZENV_F_HI_LOG_PROB one float per row; no mask.
 * max_grad_norm = +inf is accepted.  The arenas' order is zenv_option_weights' member order, parameters() order of the
 * modules: 16 tensors for the high level, 18 for the low level (lo_mu_w / lo_std_w of 3 h, lo_mu_b / lo_std_b of 3
 * elements).  Neither touches the acting agent's weights: read the parameters back and zenv_option_load them to act with
 * them -- which drops the transitions the last collection left open. */
/* zenv_skppo_check's rules: ZENV_E_ARG for h_dim outside 1 .. 191, n_skills outside 1 .. 32, a zone_feat other than
 * zenv_zone_feat(cfg), a null tensor, a missing critic at either level, distributional_value != 0, a negative or
 * non-finite hyper-parameter (max_grad_norm = +inf excepted), max_batch < 1, a workspace of 2^31 floats or more. */
int zenv_opppo_check(const zenv_config *cfg, const zenv_option_weights *init, const zenv_ppo_config *lo,
                     const zenv_ppo_config *hi);
/* Both learners from one set of weights (init->precision is not used).  A second call replaces them; a failed one
 * leaves neither. */
int zenv_opppo_init(zenv_t *h, const zenv_option_weights *init, const zenv_ppo_config *lo, const zenv_ppo_config *hi);
/* The flat functions with the level after the handle.  ZENV_E_ARG for a level other than 0 or 1; ZENV_E_STATE without
 * zenv_opppo_init.  The update calls answer ZENV_E_STATE unless the handle's ZENV_F_EXP_* / ZENV_F_LO_* / ZENV_F_HI_*
 * buffers hold a completed zenv_collect_option's records with the experience's T and option weights with S skills are
 * loaded (no collect yet, another collector ran last, or zenv_skill_load replaced the weights); zenv_hppo_*, zenv_xyppo_*
 * and zenv_skppo_* refuse these records in turn.  The high level also answers ZENV_E_STATE when the last call closed no
 * transition (M = 0); the low level works then.  Statistics: ZENV_F_OPPPO_LO_STATS / ZENV_F_OPPPO_HI_STATS.  A host
 * index outside [0, N (T - 1)) (low) or [0, M) (high) is ZENV_E_ARG; a device-resident one is never dereferenced: the
 * sample is dropped as zenv_ppo_minibatch drops one, it adds nothing to the loss or to any gradient, the divisor stays
 * the minibatch's count, and the next call that waits for the device answers ZENV_E_ARG once.  A recorded skill outside
 * [0, S) -- a frame's ZENV_F_LO_SKILL or a row's ZENV_F_HI_ACTION -- drops its sample the same way; the -1 of a frame
 * on which the env idled is refused this way too. */
int zenv_opppo_tensor(zenv_t *h, int level, int which, int index, void **dev_ptr, int64_t *count);
int zenv_opppo_read(zenv_t *h, int level, int which, int index, float *dst);
int zenv_opppo_write(zenv_t *h, int level, int which, int index, const float *src);
int zenv_opppo_get_step(zenv_t *h, int level, int64_t *step);
int zenv_opppo_set_step(zenv_t *h, int level, int64_t step);
int zenv_opppo_minibatch(zenv_t *h, int level, const int32_t *idx, int count, int idx_on_device, int apply);
int zenv_opppo_apply(zenv_t *h, int level);
int zenv_opppo_epoch(zenv_t *h, int level, const int32_t *order, int total, int batch_size, int on_device);

/* ---- DIAYN's inverse model and learned skill prior on the device: update_inverse_parameters / update_skill_prior,
 * main/src/torch_ac/algos/_hier_policy_opt.py:421-464 ----
 * One more learner, with its own four arenas, Adam step count, workspace and statistics: InverseModel
 * (zenv_skill_inverse_weights' 10 tensors in member order: the flat encoder, a ReLU on combine_net.0, combine_net.2 as
 * an S-way head; no critic) under CrossEntropyLoss(logits, skill).mean(), Adam without a clip (max_grad_norm = +inf;
 * clip_eps, entropy_coef and value_loss_coef of zenv_ppo_config are checked and not used).  It reads the records of the
 * last zenv_collect_skill in place.  Sample index i in [0, N (T - 1)) is env i / (T - 1), frame f = i % (T - 1): the
 * observation and zone rows of frame f + 1 with the skill (ZENV_F_LO_SKILL) of frame f, kept where ZENV_F_EXP_MASK of
 * frame f + 1 is not 0 (_hier_policy_opt.py:193-199).  zenv_diayn_samples compacts the kept indexes on the device,
 * ascending -- the reference's env-major order -- into ZENV_F_DIAYN_SAMPLES, waits and returns their number: callers
 * permute [0, count), index the list with the permutation and pass the sample indexes to the update calls.  The list is
 * of the records it was taken from: the next collection empties it.  The learner never touches the acting
 * discriminator: read the parameters back and zenv_skill_inverse_load them.  Statistics: ZENV_F_DIAYN_STATS. */
/* On the host alone: ZENV_E_ARG for h_dim outside 1 .. 191, n_skills outside 1 .. 32, a zone_feat other than
 * zenv_zone_feat(cfg), a null tensor, a precision other than ZENV_MLP_F32, distributional_value != 0, a negative or
 * non-finite hyper-parameter (max_grad_norm = +inf excepted), max_batch < 1, a workspace of 2^31 floats or more. */
int zenv_diayn_check(const zenv_config *cfg, const zenv_skill_inverse_weights *init, const zenv_ppo_config *pc);
/* A second call replaces the learner; a failed one leaves none. */
int zenv_diayn_init(zenv_t *h, const zenv_skill_inverse_weights *init, const zenv_ppo_config *pc);
/* The flat functions; their semantics are the flat functions'.  ZENV_E_STATE without zenv_diayn_init.  The update calls
 * and zenv_diayn_samples answer ZENV_E_STATE unless the handle's buffers hold a completed zenv_collect_skill's records
 * (of an agent with the learner's S skills) of at least two frames -- zenv_collect_option's are refused -- and
 * zenv_diayn_minibatch / _epoch also when the collection kept no sample.  A host index outside [0, N (T - 1)) is
 * ZENV_E_ARG.  A device-resident index outside that range, a sample whose keep flag is 0 and a recorded skill outside
 * [0, S) are never trained on: the sample is dropped as zenv_ppo_minibatch drops one, it adds nothing to the loss or to
 * any gradient, and the next call that waits for the device answers ZENV_E_ARG once. */
int zenv_diayn_tensor(zenv_t *h, int which, int index, void **dev_ptr, int64_t *count);
int zenv_diayn_read(zenv_t *h, int which, int index, float *dst);
int zenv_diayn_write(zenv_t *h, int which, int index, const float *src);
int zenv_diayn_get_step(zenv_t *h, int64_t *step);
int zenv_diayn_set_step(zenv_t *h, int64_t step);
int zenv_diayn_samples(zenv_t *h, int64_t *count);
int zenv_diayn_minibatch(zenv_t *h, const int32_t *idx, int count, int idx_on_device, int apply);
int zenv_diayn_apply(zenv_t *h);
int zenv_diayn_epoch(zenv_t *h, const int32_t *order, int total, int batch_size, int on_device);
/* The learned skill prior: skill_logits [n_skills], Adam's moments and step count in the handle (host memory).
 * zenv_diayn_prior_update takes one Adam step (torch.optim.Adam(lr, eps = adam_eps); the reference: 1e-2, 1e-8) on the
 * mean cross-entropy of the logits against the M picks (ZENV_F_HI_ACTION) of the last zenv_collect_skill: the picks are
 * counted on the device, the gradient softmax(logits)_s - count_s / M is formed in double on the host.  A pick outside
 * [0, S) is not counted and the call answers ZENV_E_ARG.  ZENV_E_STATE without zenv_diayn_prior_init, without such
 * records (M = 0) or with records of an agent with another S.  What the next zenv_collect_skill takes as
 * skill_prior_logits is zenv_diayn_prior_read's. */
int zenv_diayn_prior_init(zenv_t *h, const float *logits, int n_skills, double lr, double adam_eps);
int zenv_diayn_prior_update(zenv_t *h);
int zenv_diayn_prior_read(zenv_t *h, float *logits);
int zenv_diayn_prior_write(zenv_t *h, const float *logits);

/* ---- results ---- */
int zenv_get(zenv_t *h, int field, void *dst, int dst_on_device);
/* The rows of envs [first_env, first_env + count) of an env-major field (obs, zone_obs, reward, counters ...; not the
 * time-major ZENV_F_EXP_* buffers) into host memory: what a caller that looks at a few envs of a multi-GB batch uses. */
int zenv_get_rows(zenv_t *h, int field, int first_env, int count, void *dst);
/* zero-copy for GPU consumers: the handle's own buffer, live -- except ZENV_F_EP_RETURN / _EP_LEN and ZENV_F_SKILL /
 * _SKILL_AGE, which are plain copies brought up to date by this call (stream-ordered): call it again for fresh values */
int zenv_device_ptr(zenv_t *h, int field, void **ptr);
int64_t zenv_field_bytes(const zenv_t *h, int field);
int zenv_sync(zenv_t *h);
int zenv_query(zenv_t *h);   /* non-blocking: 1 = everything enqueued on the handle's stream has finished, 0 = not yet */
/* Host-policy surface (a CPU-resident policy: actions up, observations down, every step): page-locked host
 * memory for the caller's buffers, so that zenv_step()'s action upload and zenv_get()'s downloads run as DMA
 * at PCIe rate instead of through a pageable bounce buffer.  zenv_get_many() enqueues several downloads and
 * synchronises once.  Free with zenv_host_free (any time before process exit). */
void *zenv_host_alloc(int64_t bytes);
int zenv_host_free(void *ptr);
int zenv_get_many(zenv_t *h, int n_fields, const int *fields, void *const *dst);
/* The per-step results a host policy reads back -- what one `worker` of the reference pickles into its Pipe after
 * env.step() (main/src/torch_ac/torch_utils/penv.py:8-12, 52-59) -- live in ONE device allocation, 256-byte aligned
 * pieces in ZENV_RESULT_* order, so that a step of a small batch (the reference trains with 16 envs,
 * scripts/train_ppo.py:29-30) costs one upload, one launch, one download and one synchronisation:
 * zenv_results_layout() returns the slab's size and the piece offsets (offsets may be NULL);
 * zenv_step_results() = zenv_step(actions on the host) + download of the whole slab into host_slab (page-locked
 * memory from zenv_host_alloc for DMA) + synchronise; actions == NULL only downloads (after zenv_reset). */
enum {
    ZENV_RESULT_OBS = 0,        /* float32 [N][8]            */
    ZENV_RESULT_REWARD = 1,     /* float32 [N]               */
    ZENV_RESULT_DONE = 2,       /* uint8   [N]               */
    ZENV_RESULT_GOAL_MET = 3,   /* uint8   [N]               */
    ZENV_RESULT_EXCEPTION = 4,  /* uint8   [N]               */
    ZENV_RESULT_ZONE_OBS = 5,   /* float32 [N][Z][F]         */
    ZENV_N_RESULTS = 6
};
int64_t zenv_results_layout(const zenv_t *h, int64_t *offsets /* [ZENV_N_RESULTS] or NULL */);
int zenv_step_results(zenv_t *h, const float *actions, int auto_reset, void *host_slab);

/* Host-resident I/O for small batches driven from the host (the reference's own shape: 16 worker envs and a policy on
 * the host, train_ppo.py:29-30 / penv.py:63-77).  enable = 1 moves the results slab (zenv_results_layout) and the action
 * buffer into page-locked host memory that the kernels write and read THEMSELVES over the bus: a step is then one kernel
 * launch and one wait -- no upload, no download (zenv_step_results: two copy enqueues that cost more than the kernel at
 * this size).  *results / *actions receive the two buffers (NULL when switched off); write the actions, call
 * zenv_step_host, read the results in place.  Every other entry point keeps working (zenv_get*, zenv_step_results,
 * snapshots), device-side readers of the observations (the network kernels) then read them over the bus: meant for
 * batches of a few hundred envs at most.  zenv_collect is refused while it is on.  enable = 0 moves everything back. */
int zenv_host_io(zenv_t *h, int enable, void **results, float **actions);
/* zenv_step with the actions already in the zenv_host_io buffer; returns when the results are in theirs. */
int zenv_step_host(zenv_t *h, int auto_reset);
/* Enqueue everything from now on onto the caller's HIP stream (hipStream_t passed as void*; NULL =
 * back to the handle's own stream; the null stream is named by hipStreamLegacy).  The handle first
 * drains the stream it was using.  This is how
 * a device-resident policy (base.py:139-145 without the .cpu().numpy() round trip) shares one
 * stream with the env: step, read the obs buffers of zenv_device_ptr(), compute actions, step. */
int zenv_set_stream(zenv_t *h, void *hip_stream);
int64_t zenv_step_count(const zenv_t *h);   /* batched steps executed so far */

/* ---- multi-GPU: env shards and the job's one collective ----
 * The path shards trivially: one process per GPU, rank r owns global envs [r*N, (r+1)*N), nothing is exchanged on the
 * step path.  After a rollout the per-env episodic figures are all-gathered over RCCL (xGMI) -- what replaces the
 * reference's per-env Pipe star, main/src/torch_ac/torch_utils/penv.py:26-40, at N > 1.  No PyTorch involved: librccl is
 * dlopen()ed by the first of these calls (a copy already in the process wins; ZENV_RCCL_PATH names another).
 *   zenv_comm_unique_id   rank 0: ncclGetUniqueId into id[ZENV_COMM_ID_BYTES]; the host hands it to every rank
 *                         (any side channel: a file, the launcher's store)
 *   zenv_comm_init        ncclCommInitRank on the handle's device; collective: every rank calls it
 *   zenv_allgather        field = one 4- or 8-byte figure per env (ZENV_F_LAST_RETURN, _EP_RETURN: float64 narrowed to
 *                         float32; ZENV_F_REWARD float32; ZENV_F_EPISODES, _LAST_LEN, _VISIT_COUNT, _EP_LEN int32) ->
 *                         dst [world * N] 4-byte elements ordered by global env index, on the handle's stream,
 *                         synchronised on return
 *   zenv_comm_barrier     the handle's stream drained on every rank (one-element all-reduce + synchronise)
 *   zenv_comm_allreduce_max  *value = max over ranks (the bench's max-over-ranks step time) */
#define ZENV_COMM_ID_BYTES 128
int zenv_comm_unique_id(void *id_out);
int zenv_comm_init(zenv_t *h, int rank, int world, const void *unique_id);
int zenv_comm_destroy(zenv_t *h);
int zenv_comm_info(const zenv_t *h, int *rank, int *world, const char **library);
int zenv_allgather(zenv_t *h, int field, void *dst, int dst_on_device);
int zenv_comm_barrier(zenv_t *h);
int zenv_comm_allreduce_max(zenv_t *h, double *value);

/* ---- rendering: observations and recorded experience as RGB frames (K18) ----
 * What the reference looks at through ZoneEnvBase.render (main/envs/zone_envs/ZoneEnvBase.py:243-336) and the loops of
 * scripts/visualize.py / visualize_hier.py.  Not MuJoCo's perspective camera: an exact orthographic, top-down drawing
 * of what the agent observes -- the zone rows (centre / 3, RGBA, the task's extra feature) and the robot's position and
 * heading (obs[1:3], obs[3:5]) -- in float32 by fixed rules, so that a frame is reproducible bit for bit.
 * dst: uint8 [count][height][width][3], RGB, row 0 at the top (+y); pixel (r, c) has its centre at
 * x = (c + 0.5) sx - view, y = view - (r + 0.5) sy with sx = 2 view / width, sy = 2 view / height, in observation
 * units (world / 3).  Painter's order, opaque: background (224, 224, 224); the zones in index order -- a disc of radius
 * zones_size / 3 in the row's colour, a row with alpha 0 (WaitWrapper's all-zero observation) skipped, an unvisited
 * TimedTSP zone (0, 1, 1) drawn as the reference fades it, (1 - t, max(0, t), max(0, t)) with t = row[6]
 * (TTSP_env.py:52-58); the image's mark, a ring from 1 to 1.35 zone radii in (255, 0, 255) around marks[i] (marks NULL
 * or a NaN component: none); the robot, a disc of radius robot_radius / 3 in (32, 32, 32) whose pixels more than 0.4
 * radii ahead of the centre along the heading are the nose (255, 255, 255).
 *   ZENV_RENDER_CURRENT     image i = env first + i, from the observation of the last reset / step (wherever the
 *                           handle published it: zenv_host_io's page-locked slab included)
 *   ZENV_RENDER_EXPERIENCE  image i = frame first + i of env `env` in the ZENV_F_EXP_* buffers of the last
 *                           collection (any of the five collectors): a film of one env's trajectory in one launch
 * zenv_render_check applies the rules that need no handle (ZENV_E_ARG: a null argument, a size outside 1 .. 4096, a
 * view that is not positive and finite, a robot_radius that is negative or not finite, an unknown source, count < 1,
 * first < 0, first + count beyond the envs (CURRENT), env outside [0, n_env) (EXPERIENCE), count * width * height * 3
 * >= 2^31).  zenv_render adds ZENV_E_STATE for a handle never reset (CURRENT) or without experience (EXPERIENCE) and
 * ZENV_E_ARG for first + count beyond the recorded frames.  marks: float32 [count][2], host or device memory.  With
 * dst in device memory the call is asynchronous on the handle's stream and dst may have any alignment; with a host
 * dst the frames are staged on the device, copied and waited for. */
enum { ZENV_RENDER_CURRENT = 0, ZENV_RENDER_EXPERIENCE = 1 };
typedef struct zenv_render_config {
    int32_t width, height;   /* 1 .. 4096 each */
    int32_t source;          /* ZENV_RENDER_CURRENT / ZENV_RENDER_EXPERIENCE */
    int32_t env;             /* ZENV_RENDER_EXPERIENCE: the env whose frames are drawn */
    float view;              /* half-width of the square shown, observation units; > 0, finite */
    float robot_radius;      /* world units; >= 0, finite */
} zenv_render_config;
int zenv_render_check(const zenv_config *cfg, const zenv_render_config *rc, int n_env, int first, int count);
int zenv_render(zenv_t *h, const zenv_render_config *rc, int first, int count, const float *marks,
                int marks_on_device, uint8_t *dst, int dst_on_device);

/* ---- the per-episode training logs of collect_experiences (K19) ----
 * The second value every collect_experiences of the reference returns: `logs` (main/src/torch_ac/algos/base.py:233-247,
 * main/src/torch_ac/algos/_hier_policy_opt.py:216-232 and the other trees' _hier_policy_opt.py at the same place),
 * computed on the device from the records the last collector left, in float32 and in the reference's order of
 * operations.  Per handle, zero at first and after zenv_episode_log_reset: the running sums log_episode_return,
 * _reshaped_return, _num_frames and _diversity [N] (base.py:101-103), and the tail, the last N entries of the lists
 * (N entries of 0, `[0] * num_procs`, base.py:106-108).  For frame t of the collection, done_t = 1 - mask[t + 1]
 * (1 - the mask carried into the next call for the last frame): the sums take += value (base.py:169-171), an env
 * whose episode is done appends an entry -- the frames in order, the envs ascending inside a frame, as `for i, done_ in
 * enumerate(done)` does (base.py:173-178) -- and the sums are multiplied by 1 - done_t (base.py:180-182).
 *   collector                  return +=              reshaped +=         an entry when          num_frames
 *   zenv_collect               env reward             ZENV_F_EXP_REWARD   done_t                 T N
 *   zenv_collect_hier/_option  ZENV_F_LO_ENV_REWARD   the same            done_t                 T N
 *   zenv_collect_skill / _xy   ZENV_F_LO_ENV_REWARD   the same            done_t and the env is  the active envs of
 *                                                                         active in its window   every frame, summed
 * An env is active from every frame t with t % skill_len == 0 until its first done_t of the window
 * (_hier_policy_opt.py:29-31, 112-116); an idle env keeps counting frames into its sum, which the mask zeroes again.
 * zenv_collect_skill also sums ZENV_F_LO_DIVERSITY, the diversity reward without diversity_coef (:109); the prediction
 * column of the skills and xy-goals agents is never added to and stays 0.
 * The result is the last max(D, N) entries of (tail + the D new entries) (base.py:235-240); the tail becomes the last N
 * of the same list (:245-247).  Beside the reference's columns every entry carries the env that produced it (-1 for the
 * initial zero entries).
 *
 * zenv_episode_log: once after a collection; it synchronises the stream once, to size the result.  ZENV_E_ARG on a
 * null argument; ZENV_E_STATE when no collection has run or this collection's log was already taken (every collector
 * re-arms it).  info.columns: the ZENV_EPLOG_* columns the collector's `logs` has, as bits (1 << column).
 * zenv_episode_log_tensor: the device pointer of a column of the last result and its length (float32; int32 for
 * ZENV_EPLOG_ENV), valid until the next zenv_episode_log.  zenv_episode_log_read copies a column to host memory.
 * zenv_episode_log_stats: out = count, sum, the sum of squares about the mean (sum / count), min, max of a float
 * column, reduced in float64 by a fixed tree.  All three: ZENV_E_STATE before the first zenv_episode_log, ZENV_E_ARG for an
 * unknown column (the env column has no statistics) or a null argument.
 * zenv_episode_log_reset zeroes the sums and the tail, as a fresh algo object. */
enum {
    ZENV_EPLOG_RETURN = 0,            /* return_per_episode */
    ZENV_EPLOG_RESHAPED_RETURN = 1,   /* reshaped_return_per_episode */
    ZENV_EPLOG_NUM_FRAMES = 2,        /* num_frames_per_episode */
    ZENV_EPLOG_DIVERSITY = 3,         /* diversity_per_episode (zenv_collect_skill) */
    ZENV_EPLOG_PREDICTION = 4,        /* prediction_per_episode (zenv_collect_skill, zenv_collect_xy) */
    ZENV_EPLOG_ENV = 5,               /* the env of every entry, int32 */
    ZENV_EPLOG_COUNT = 6
};
typedef struct zenv_episode_log_info {
    int64_t kept;          /* entries of the result: max(done, N) */
    int64_t done;          /* D: entries this collection appended (log_done_counter) */
    int64_t num_frames;    /* logs["num_frames"] */
    int64_t columns;       /* bit (1 << ZENV_EPLOG_*) for every column the collector's logs define */
} zenv_episode_log_info;
int zenv_episode_log(zenv_t *h, zenv_episode_log_info *out);
int zenv_episode_log_tensor(zenv_t *h, int column, void **ptr, int64_t *count);
int zenv_episode_log_read(zenv_t *h, int column, void *dst);
int zenv_episode_log_stats(zenv_t *h, int column, double out[5]);
int zenv_episode_log_reset(zenv_t *h);

/* Measurement utility (bench.py `store_stream_ceiling`; not part of the env path): n_tiles waves each rewrite their
 * own contiguous tile_bytes (a multiple of 16, >= 1024) `steps` times with 1 KiB dwordx4 bursts under cache_policy
 * (0 plain, 2 non-temporal, 16 sc1 = write-through) -- the row stream of the step kernels with the env taken away.
 * us_per_step = best of `reps` timed launches (dispatch begin/end events) / steps, after one untimed launch. */
int zenv_probe_store_stream(int device, int64_t n_tiles, int tile_bytes, int steps, int cache_policy, int reps,
                            float *us_per_step);

/* ---- state snapshot (tests / checkpointing; the reference never checkpoints env state) ---- */
int64_t zenv_state_bytes(const zenv_t *h);
int zenv_get_state(zenv_t *h, void *dst, int64_t bytes);
int zenv_set_state(zenv_t *h, const void *src, int64_t bytes);
/* Per-env dynamic state for parity tests: qpos[N,3], qvel[N,3] float64; zone_state int32 [N,Z]
 * (visited 0/1, or colour 0..2); cooldown int32 [N,Z]; steps int32 [N]. Any may be NULL. */
int zenv_debug_state(zenv_t *h, double *qpos, double *qvel, int32_t *zone_state,
                     int32_t *cooldown, int32_t *steps);

#ifdef __cplusplus
}
#endif
#endif /* ZENV_H */
