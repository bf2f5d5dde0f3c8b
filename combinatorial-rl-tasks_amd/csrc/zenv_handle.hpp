// zenv_handle.hpp -- the handle behind zenv_t and the helpers every translation unit of the C ABI uses (zenv_api.cpp:
// the environment; zenv_agents.cpp: the networks, the per-step policies, the collectors; zenv_train.cpp: the learners;
// zenv_episode_log.cpp: the collectors' per-episode logs).
// Internal: not installed.
#pragma once
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is dlopen()ed by the first zenv_comm_* call

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/zenv.h"
#include "dev_params.hpp"
#include "kernels.hpp"
#include "hier_f32.hpp"
#include "option_f32.hpp"
#include "skill_f32.hpp"
#include "xy_f32.hpp"
#include "mlp_policy.hpp"
#include "episode_log.hpp"
#include "layout_sample.hpp"
#include "order_rows.hpp"

using namespace zenvk;

#define ZENV_INTERNAL __attribute__((visibility("hidden")))

// sets the calling thread's zenv_last_error() text and returns `code` (zenv_api.cpp)
ZENV_INTERNAL int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(ZENV_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                        __FILE__, __LINE__);                                                  \
    } while (0)

struct Alloc {
    void **slot;
    size_t bytes;
    bool is_state;   // part of zenv_get_state/zenv_set_state
    int64_t slab_off = -1;   // >= 0: lives at this offset of the handle's results slab (one hipMalloc, one download)
};

struct PpoState;   // zenv_train.cpp
// A handle's learner slots.  The first ten follow the ZENV_F_PPO_STATS .. ZENV_F_DIAYN_STATS fields, so a statistics
// field's slot is its distance from ZENV_F_PPO_STATS; a pair's high level is the slot behind its low level.
enum LearnerSlot {
    L_FLAT = 0,                     // zenv_ppo_*
    L_HIER_LO, L_HIER_HI,           // zenv_hppo_*
    L_XY_LO, L_XY_HI,               // zenv_xyppo_*
    L_SKILL_LO, L_SKILL_HI,         // zenv_skppo_*
    L_OPTION_LO, L_OPTION_HI,       // zenv_opppo_*
    L_DIAYN,                        // zenv_diayn_*: the inverse model
    L_A2C,                          // zenv_a2c_*: the flat actor-critic's other learner (ZENV_F_A2C_STATS)
    N_LEARNERS
};
static_assert(ZENV_F_PPO_STATS + L_HIER_LO == ZENV_F_HPPO_LO_STATS && ZENV_F_PPO_STATS + L_HIER_HI == ZENV_F_HPPO_HI_STATS &&
              ZENV_F_PPO_STATS + L_XY_LO == ZENV_F_XYPPO_LO_STATS && ZENV_F_PPO_STATS + L_XY_HI == ZENV_F_XYPPO_HI_STATS &&
              ZENV_F_PPO_STATS + L_SKILL_LO == ZENV_F_SKPPO_LO_STATS && ZENV_F_PPO_STATS + L_SKILL_HI == ZENV_F_SKPPO_HI_STATS &&
              ZENV_F_PPO_STATS + L_OPTION_LO == ZENV_F_OPPPO_LO_STATS && ZENV_F_PPO_STATS + L_OPTION_HI == ZENV_F_OPPPO_HI_STATS &&
              ZENV_F_PPO_STATS + L_DIAYN == ZENV_F_DIAYN_STATS, "LearnerSlot follows the statistics fields");

struct zenv {
    zenv_config cfg{};
    int n_env = 0;
    int device = 0;
    hipStream_t stream = nullptr;       // the stream work is enqueued on
    hipStream_t own_stream = nullptr;   // created with the handle; `stream` unless zenv_set_stream
    DevParams p{};
    DevParams *d_self = nullptr;     // device copy of p (DevParams::self): the persistent kernel reads cold fields from it
    DevParams self_shadow{};         // what d_self holds
    bool self_valid = false;
    std::vector<Alloc> allocs;
    // The per-step results (obs, reward, done, goal_met, exception, zone_obs) share ONE allocation, 256-byte aligned
    // pieces in that order, so that a host policy fetches them with one copy (zenv_step_results).
    void *results_slab = nullptr;
    // zenv_host_io(): results slab + action buffer in page-locked host memory that the kernels write / read directly
    void *host_io_slab = nullptr;
    float *host_io_actions = nullptr, *dev_actions = nullptr;
    int64_t results_off[ZENV_N_RESULTS] = {};
    int64_t results_bytes = 0;
    void *bank_mem[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };   // robot, zone, aux, seed, derived first rows
    uint8_t *d_mask = nullptr;
    bool bank_ready = false;
    bool sched_ready = false;
    bool was_reset = false;
    int64_t step_count = 0;
    // What the internal action buffer holds when a fused rollout left a_{step_count} behind: the next rollout with
    // the same action source continues from it instead of launching the policy kernel again.
    struct {
        bool valid = false;
        int policy = -1;
        uint64_t seed = 0, index0 = 0;
        int64_t step = -1;
    } act_tag;
    std::vector<hipEvent_t> events;
    int rollout_slice_tiles = 1024;   // 64-env tiles per persistent launch (zenv_set_rollout_slice): one per wave slot pair
    // actor network (zenv_mlp_load)
    void *mlp_mem = nullptr;
    MlpImages mlp{};
    void *mlp_pooled = nullptr;
    float *mlp_mu = nullptr, *mlp_std = nullptr, *mlp_value = nullptr, *mlp_value_sigma = nullptr;
    int *mlp_range_flag = nullptr;      // pinned host word, see mlp_range_check()
    void *mlp_f32_mem = nullptr;        // float32 path (ZENV_MLP_F32): transposed float32 weights
    MlpF32 mlp_f32{};
    bool mlp_ready = false;
    // Zone-goals hierarchical agent (zenv_hier_load): float32 weights, the high level's outputs
    void *hier_mem = nullptr;
    HierF32 hier{};
    bool hier_ready = false;
    float *hier_logits = nullptr, *hier_value = nullptr;
    // fixed-length-skills agent (zenv_skill_load): float32 weights, the per-env skill state, the high level's outputs
    void *skill_mem = nullptr;
    SkillF32 skill{};
    bool skill_ready = false;
    int skill_len = 200;                // evaluate_hier.py:21
    int skill_n = 0;                    // S the outputs are allocated for
    SkillState sst{};
    void *sst_mem = nullptr;
    float *skill_logits = nullptr, *skill_value = nullptr;
    // variable-length Options agent (zenv_option_load): it takes the place of the skill agent on the handle -- its
    // weights live in skill_mem / skill, the state in sst -- plus the picking envs' list and the third output's fields
    bool option_ready = false;
    int option_compact = 0;
    void *opt_mem = nullptr;
    OptionList olist{};
    OptionTerm oterm{};
    // xy-goals agent (zenv_xy_load): it shares the per-env clock (sst, skill_len) with the skill family -- skill 0 = the
    // env has a goal -- and takes their place on the handle; its own: float32 weights, one allocation (xy_state_mem) for
    // the goal, its staging and mask (zenv_set_xy_goals), the high level's outputs and the published age
    void *xy_mem = nullptr;
    XyF32 xy{};
    bool xy_ready = false;
    void *xy_state_mem = nullptr;
    float2 *xy_goal = nullptr, *xy_goal_in = nullptr;
    float *xy_goal_mu = nullptr, *xy_goal_std = nullptr, *xy_value = nullptr;
    int32_t *xy_age = nullptr;
    uint8_t *xy_mask = nullptr;
    // zenv_collect_xy: the per-frame records of one call (T frames, W windows) beside the ZENV_F_EXP_* buffers -- the
    // low level's goal, its distance and the env reward [T][N]; the high level's goal of every row [N * W]; the
    // bootstrap goal and the row count [N]
    struct {
        int T = 0, W = 0;
        float2 *lo_goal = nullptr, *hi_goal = nullptr, *boot = nullptr;
        float *dist = nullptr, *env_reward = nullptr;
        int32_t *count = nullptr;
    } xc;
    void *xc_mem = nullptr;
    // zenv_collect_option: the per-frame records of one call (T frames) that have no place in hframes -- the skill the
    // low level acted under, a_2 with its log_prob and the termination draw, [T][N] each
    struct {
        int T = 0;
        int32_t *lo_skill = nullptr;
        float *term_action = nullptr, *term_log_prob = nullptr;
        uint8_t *ended = nullptr;
    } oc;
    void *oc_mem = nullptr;
    // DIAYN's discriminator (zenv_skill_inverse_load) and the per-frame records of zenv_collect_skill (T frames):
    // lo_skill, diversity, env_reward [T][N]; the bootstrap skill and the row count [N]
    void *skinv_mem = nullptr;
    SkillInvF32 skinv{};
    bool skinv_ready = false;
    struct {
        int T = 0;
        int32_t *lo_skill = nullptr, *boot = nullptr, *count = nullptr;
        float *diversity = nullptr, *env_reward = nullptr;
    } sk;
    void *sk_mem = nullptr;
    // the learners (zenv_*_init), by LearnerSlot: arenas, workspace, the optimiser's step count.  DIAYN's never touches
    // the acting discriminator (skinv)
    PpoState *learner[N_LEARNERS] = {};
    // zenv_diayn_samples: the kept sample indexes of the last zenv_collect_skill (ZENV_F_DIAYN_SAMPLES), capacity
    // diayn_cap, and the compaction's block counts behind them in the same allocation; diayn_kept < 0: not taken since
    // the last collection (every collector resets it)
    void *diayn_mem = nullptr;
    int32_t *diayn_list = nullptr, *diayn_blocks = nullptr;
    int64_t diayn_cap = 0, diayn_kept = -1;
    // the learned skill prior (zenv_diayn_prior_init): logits, Adam's moments and step count on the host; the device
    // histogram [32 counters, the compaction's total] and its page-locked flag (a pick outside [0, S))
    struct {
        bool ready = false;
        int S = 0;
        double lr = 0.0, adam_eps = 0.0;
        int64_t step = 0;
        float logits[32] = {}, exp_avg[32] = {}, exp_avg_sq[32] = {};
    } prior;
    int32_t *diayn_counts = nullptr;
    int *diayn_flag = nullptr;
    // goal-conditioned variant (zenv_goal_enable)
    bool goal_enabled = false;
    bool order_enabled = false;   // solver-ordered variant (zenv_order_enable)
    // zenv_order_rows: the flat network, its collector and its learner take the reference's (Z, 7) rows -- net_feat, the
    // handle's network row width, is p.F + 1 while on and p.F otherwise (DevParams knows nothing of it: the step kernels
    // keep their 6-wide rows); order_rows: ZENV_F_ORDER_ROWS [N][Z][7], assembled by k_order_rows before a network reads it
    int net_feat = 0;
    float *order_rows = nullptr;
    OrderWait order_wait{};       // WaitWrapper's zero order column for envs left alone by zenv_step(auto_reset 0), order_rows.hpp
    int32_t *goal_in = nullptr, *goal_bad = nullptr;
    // experience buffers (zenv_collect)
    ExpBuffers exp{};
    void *exp_mem = nullptr;
    bool exp_hier = false;              // the ZENV_F_EXP_* buffers hold zenv_collect_hier's frames (any other collector clears it)
    bool exp_xy = false;                // ... zenv_collect_xy's, the same
    bool exp_skill = false;             // ... zenv_collect_skill's, the same
    bool exp_option = false;            // ... zenv_collect_option's, the same
    // zenv_collect_hier: the per-frame records of one call (T), the state that lives from call to call, the flat
    // high-level output (capacity hi_cap rows, hi_m of them written by the last call)
    HierFrames hframes{};
    void *hframes_mem = nullptr;
    HierCarry hcarry{};
    void *hcarry_mem = nullptr;
    HierOut hout{};
    void *hout_mem = nullptr;
    int64_t hi_cap = 0, hi_m = 0;
    int hi_kind = 0;                    // whose rows and per-frame records the ZENV_F_HI_* / ZENV_F_LO_* fields hold:
                                        // 0 zenv_collect_hier's, 1 zenv_collect_skill's, 2 zenv_collect_option's,
                                        // 3 zenv_collect_xy's
    int32_t *hi_total_host = nullptr;   // page-locked word M is read back into
    // staging of zenv_bank_update (page-locked host image + its device copy)
    void *refill_host = nullptr, *refill_dev = nullptr;
    size_t refill_cap = 0;
    hipEvent_t refill_done = nullptr;
    bool refill_busy = false;
    // device layout sampling (zenv_layout.cpp): the status block and the stale-list count in one allocation; the slot /
    // seed lists the kernels walk (capacity list_cap entries); the page-locked image zenv_bank_update_device stages its
    // 12 bytes per layout in; a streamed ring's first seeds [N] and whether zenv_ring_stream made the current schedule
    struct {
        void *mem = nullptr;
        SampleStatus *status = nullptr;
        uint32_t *count = nullptr;
        double *zones_locations = nullptr;   // device copy of cfg.zones_locations (the same allocation)
        void *list_mem = nullptr;
        int32_t *list_slots = nullptr;
        int64_t *list_seeds = nullptr;
        size_t list_cap = 0;
        void *stage_host = nullptr;
        size_t stage_cap = 0;
        hipEvent_t stage_done = nullptr;
        bool stage_busy = false;
        int64_t *ring_seed0 = nullptr;
        bool ring_streamed = false;
        bool timed_device = false;           // zenv_timed_layouts_device: TimedTSP layouts with det_log's deadlines
        bool order_device = false;           // zenv_order_routes_device: solver-ordered rows with the tour solved on the device (K21)
    } ls;
    // the sharded job's communicator (zenv_comm_init): RCCL over xGMI
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    void *comm_send = nullptr, *comm_recv = nullptr;   // [N] and [world * N] 4-byte elements
    double *comm_scalar = nullptr;                      // device scratch of the barrier / max-reduce
    // zenv_step_many: the chunk's actions on the device (when they came from the host) and its time-major records
    void *chunk_mem = nullptr;
    size_t chunk_cap = 0;           // steps * envs the allocation holds
    float *chunk_actions = nullptr, *chunk_reward = nullptr;
    uint8_t *chunk_done = nullptr;
    int chunk_steps = 0;            // steps of the last zenv_step_many (extent of ZENV_F_CHUNK_REWARD / _DONE)
    int chunk_host_steps = 0;       // steps of the last host-action chunk while chunk_actions holds it, else 0
    // ZENV_F_EP_RETURN / ZENV_F_EP_LEN as plain arrays: the values live in the HotA records, unpacked by refresh_field()
    double *pub_ep_return = nullptr;
    int32_t *pub_steps = nullptr;
    // zenv_episode_log (zenv_episode_log.cpp): the reference's `logs` of the last collection.  source: which collector
    // armed it (0 none / taken; 1 zenv_collect, 2 _hier, 3 _skill, 4 _option, 5 _xy), every collector sets it on
    // success and ensure_exp clears it.  state_mem: the four running sums [N] and the two tails (ping-pong, `cur` the
    // live one); res_mem: the result's columns, capacity `cap` entries; ws_mem: the (frame, wave) counts, the scan's
    // levels and totals (D, the active frames); the reduction's partial results lie behind the result.  flat_reward: the env reward
    // [T][N] of zenv_collect on a goal-conditioned handle, whose ZENV_F_EXP_REWARD holds the shaped one
    struct {
        int source = 0;
        void *state_mem = nullptr, *res_mem = nullptr, *ws_mem = nullptr;
        float *carry[4] = {};
        EpLogList tail[2] = {}, res{};
        int cur = 0;
        int64_t cap = 0, ws_counts = 0;
        int32_t *counts = nullptr, *active = nullptr, *levels = nullptr, *totals = nullptr;
        double *stat_ws = nullptr, *stat_fin = nullptr;
        int64_t kept = -1, done = 0, num_frames = 0, columns = 0;
        float *flat_reward = nullptr;
        int flat_T = 0;
    } eplog;
    // zenv_render: the device copies of a host caller's marks and of the frames on their way to host memory
    void *render_marks = nullptr, *render_stage = nullptr;
    size_t render_marks_cap = 0, render_stage_cap = 0;
};

ZENV_INTERNAL int use_device(const zenv *h);
// the width of the rows the flat network reads, records and trains on (zenv_order_rows)
inline int net_row_feat(const zenv *h) { return h->net_feat ? h->net_feat : h->p.F; }

// ---- zenv_agents.cpp, as far as the stepping paths of zenv_api.cpp call it
inline bool policy_known(int policy) { return policy >= ZENV_POLICY_UNIFORM && policy <= ZENV_POLICY_MLP_SAMPLE; }
inline bool policy_is_mlp(int policy) { return policy == ZENV_POLICY_MLP_MEAN || policy == ZENV_POLICY_MLP_SAMPLE; }
// a_t = pi(obs_t, t) into pol.out, for every kind of action source
// (rows: where a handle with zenv_order_rows on assembles the rows the network reads, null = ZENV_F_ORDER_ROWS)
ZENV_INTERNAL int run_policy(zenv *h, const StepPolicy &pol, const MlpRecord *rec = nullptr, float *rows = nullptr);
// the flat network, the flat learner and the experience buffers go: all three are sized by the network row width
ZENV_INTERNAL int drop_flat_network(zenv *h);
// the refusal of a call whose auto-resets could outrun a ring schedule
ZENV_INTERNAL int ring_guard(const zenv *h, int steps, int auto_reset_every_step);
// ZENV_E_RANGE once the float16 network kernels have flagged an operand out of range
ZENV_INTERNAL int mlp_range_check(zenv *h);

// ---- zenv_api.cpp, as far as zenv_layout.cpp calls it
ZENV_INTERNAL int validate_config(const zenv_config &c);
// Make the five freshly filled device buffers (robot, zone, aux, seed, room for the derived rows) of S slots the
// handle's bank: frees the old one, derives the first rows, treats the schedule as every bank upload does.
ZENV_INTERNAL int adopt_bank(zenv *h, void *const fresh[5], size_t S);

// ---- zenv_layout.cpp
ZENV_INTERNAL void layout_free(zenv *h);

// ---- zenv_episode_log.cpp
ZENV_INTERNAL void eplog_free(zenv *h);
// room for the env reward of T frames beside the shaped one (zenv_collect on a goal-conditioned handle)
ZENV_INTERNAL int eplog_flat_reward(zenv *h, int T);

// ---- zenv_train.cpp
ZENV_INTERNAL void ppo_free(zenv *h);
// the flat learners alone, PPO's and A2C's (zenv_order_rows: they are sized by the network row width)
ZENV_INTERNAL void ppo_free_flat(zenv *h);
// ZENV_E_ARG once an update has met (and dropped) a device-resident index out of range; mlp_range_check() asks
ZENV_INTERNAL int ppo_index_check(zenv *h);
// the statistics field of a LearnerSlot: the buffer and the bytes the last update call of that learner filled
// (ZENV_F_A2C_STATS: five floats once zenv_a2c_apply / zenv_a2c_update has run)
ZENV_INTERNAL void *ppo_stats(const zenv *h, int slot, int64_t *bytes);
