// hier_f32.hpp -- the Zone-goals hierarchical agent on the device (zone-goals/src/hier_policy_value_models.py,
// zone-goals/src/utils/hier_agent.py): HighPolicyValueModel picks the next goal zone, LoPolicyValueModel drives the
// robot to it.  float32 throughout (hier_f32.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "../../include/zenv.h"
#include "dev_params.hpp"
#include "mlp_policy.hpp"

namespace zenvk {

// One ZoneEnvModel (XIN = 8: [obs]) or ZoneEnvGoalModel (XIN = 10: [obs, goal]) encoder.  Every matrix TRANSPOSED
// ([in][kMlpHP], consecutive threads = consecutive output features) and zero-padded to kMlpHP columns; device pointers.
// zone_net_.0 and combine_net_ are split by input columns: the per-env part x = [obs(, goal)] and the rest.
struct HierEnc {
    const float *w1x, *w1z, *b1;   // zone_net_.0   [XIN][HP] (obs, goal columns), [8][HP] (zone row columns), [HP]
    const float *w2t, *b2;         // zone_net_.2   [HP][HP], [HP]
    const float *w3t, *b3;         // zone_net_.4
    const float *wcx, *wce, *bc;   // combine_net_  [XIN][HP] (obs, goal columns), [HP][HP] (zone embedding), [HP]
};
struct HierF32 {
    int h, hi_critic, lo_critic, pad;
    HierEnc hi, lo;
    // high level: actor.0 split into its embedding columns and its zone-row columns; actor.2 as one row + bias
    const float *hae, *haz, *hab;  // actor.0   [HP][HP], [8][HP], [HP]
    const float *ha2;              // actor.2   [HP + 1]: weight, bias last
    const float *hv1t, *hv1b;      // critic.0  [HP][HP], [HP]
    const float *hv2;              // critic.2  [HP + 1]
    // low level: PolicyNetwork + critic
    const float *encw, *encb;      // actor.enc_.0.0 [HP][HP], [HP]
    const float *heads;            // [4][HP + 1]: mu_ rows 0-1, std_ rows 2-3, bias last
    const float *lv1t, *lv1b;      // critic.0  [HP][HP], [HP]
    const float *lv2;              // critic.2  [HP + 1]
};

constexpr int kHierOffs = 33;      // the pointers of HierF32, from hi.w1x on
static_assert(sizeof(HierF32) == 4 * sizeof(int) + kHierOffs * sizeof(const float *), "HierF32 layout");

// Host packer: the float32 state_dict tensors of zenv_hier_weights -> one buffer; offs[] = offsets in floats of the
// pointers of HierF32 in declaration order, 0 for an absent critic (the image starts with 4 floats of padding, so that
// no tensor sits at offset 0).  hier_f32_at() binds such an image to its device address.
size_t pack_hier_f32(const zenv_hier_weights &w, int F, std::vector<float> &out, size_t offs[kHierOffs]);
HierF32 hier_f32_at(const zenv_hier_weights &w, const float *base, const size_t offs[kHierOffs]);

// What the high-level kernel does besides the logits / value: nothing (mode < 0: every env is evaluated), or pick a
// goal for every env that needs one and is not finished -- argmax (0) or a draw from Categorical(logits) (1), keyed by
// (seed, global env, step) on a Philox stream of its own -- into new_goal[N] (-1 = leave the env alone), the buffer
// launch_goal_set reads.  In modes 0 / 1 only the envs that pick are evaluated and written.  Mode -2: the critic only,
// every env (the bootstrap value V_hi(obs_T) of zenv_collect_hier); the logits are not written.
struct HierPick {
    int mode;
    uint32_t step_index;
    uint64_t seed, env_index0;
    int32_t *new_goal;
};
// What zenv_collect_hier records at frame t (hier_collect.hip), time-major [T][N]; t < 0: nothing.
//   high level, for every env that picks: its goal, the critic's value, Categorical(masked logits).log_prob(goal) and
//   the available-goals mask; open[env] = 1 (a high-level transition is open)
//   low level: lo_goal [T][N][2] = the goal input of every env (zone_xy / 3 of its last goal, 0 before the first);
//   the rest of frame t goes through MlpAction::rec (head_outputs), also for an env without a goal (zeros)
struct HierRecord {
    int t, N;
    int32_t *goal;
    float *value, *log_prob;
    uint32_t *avail;
    uint8_t *open;
    float *lo_goal;
};
inline HierRecord no_hier_record() { return HierRecord{ -1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr }; }
hipError_t launch_hier_high(const HierF32 &w, const DevParams &p, float *logits, float *value, const HierPick &pick,
                            hipStream_t s, const HierRecord &rec = no_hier_record());
// Low level for every env with a goal (p.goal >= 0): mu / std / value, and the action as MlpAction asks (mode 0: mu,
// 1: Normal(mu, std) sample).  An env without a goal gets mu = std = value = 0 (and action 0).
hipError_t launch_hier_low(const HierF32 &w, const DevParams &p, float *mu, float *stdv, float *value,
                           const MlpAction &act, hipStream_t s, const HierRecord &rec = no_hier_record());

// ---- zenv_collect_hier's bookkeeping (hier_collect.hip): the high level's semi-Markov transitions
// Per-env state that lives from call to call, [N]: hi_reward (the open transition's float32 reward so far), open, and
// the carry slot -- the transition left open by an earlier call: obs, zone_obs, goal, avail, value, log_prob.
struct HierCarry {
    float *hi_reward;
    uint8_t *open;
    float *obs, *zone_obs;          // [N][8], [N][Z*F]
    int32_t *goal;
    uint32_t *avail;
    float *value, *log_prob;
    int64_t *src;                   // [N] scratch: the exp slot (t * N + env) the carry is refilled from, -1 = keep
};
// Per-frame records of one call, time-major [T][N], plus the per-env count of closed transitions.
struct HierFrames {
    int T;
    int32_t *pick_goal;             // -1: no pick at this frame
    float *pick_value, *pick_log_prob;
    uint32_t *pick_avail;
    float *close_reward;            // the closed transition's reward
    uint8_t *close_flag;            // 0 none, 1 closed with hi_mask 1 (goal reached), 2 closed with hi_mask 0 (done)
    float *lo_goal;                 // [T][N][2]
    float *env_reward;              // [T][N]
    int32_t *count, *offset;        // [N]
    int32_t *total;                 // [1]: M
};
// The flat env-major output [M, ...] (hi_exps)
struct HierOut {
    float *obs, *zone_obs;          // [M][8], [M][Z*F]
    int32_t *action;
    uint8_t *action_mask;           // [M][Z]
    float *value, *log_prob, *advantage, *returnn;
    float *reward, *mask;           // the transition's reward and hi_mask (not part of hi_exps; what its GAE used)
    uint32_t *avail;                // [M] scratch
    int64_t *src;                   // [M] scratch: exp slot (t * N + env) of the row's observation, < 0: carry of env -1 - src
};
// after the step of frame t: env reward, hi_reward, and the close of the open transition of every env that needs a goal
hipError_t launch_hier_close(const DevParams &p, const HierFrames &f, const HierCarry &c, int t, hipStream_t s);
// zenv_reset of the envs in mask (null = all): drop their open transition, hi_reward = 0
hipError_t launch_hier_reset(const HierCarry &c, const uint8_t *mask, int N, hipStream_t s);
// exclusive prefix sum of f.count into f.offset, the sum into f.total (one workgroup)
hipError_t launch_hier_count_scan(const HierFrames &f, int N, hipStream_t s);
// per env, backward over the frames: the high-level GAE, the small fields of its rows, the new carry (value, goal ...)
hipError_t launch_hier_gae(const HierFrames &f, const HierCarry &c, const HierOut &o, int N, const float *v_final,
                           float gae_lambda, hipStream_t s);
// the rows' obs / zone_obs / action_mask (M rows; a null o.action_mask is left out), then the carry slot's obs of every env whose open transition began
// in this call
hipError_t launch_hier_gather(const HierOut &o, const HierCarry &c, const float *exp_obs, const float *exp_zone_obs,
                              int64_t M, int N, int Z, int F, hipStream_t s);
hipError_t launch_hier_carry(const HierCarry &c, const float *exp_obs, const float *exp_zone_obs, int N, int ZF,
                             hipStream_t s);

}  // namespace zenvk
