// xy_f32.hpp -- the xy-goals hierarchical agent on the device (xy-goals/src/hier_policy_value_models.py:19-72,
// xy-goals/scripts/evaluate_xy_hrl.py:48-81): every skill_len steps HighPolicyValueModel draws a continuous goal in
// [-1, 1]^2 from its own Normal, LoPolicyValueModel acts under it.  float32 throughout (xy_f32.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "../../include/zenv.h"
#include "dev_params.hpp"
#include "hier_f32.hpp"
#include "mlp_policy.hpp"
#include "skill_f32.hpp"

namespace zenvk {

// Every matrix TRANSPOSED ([in][kMlpHP]) and zero-padded to kMlpHP columns, device pointers (the layout of HierF32).
// The high level is the flat actor-critic's network (ZoneEnvModel, XIN = 8, then PolicyNetwork's Gaussian heads), the
// low level the Zone-goals low level (ZoneEnvGoalModel, XIN = 10: [obs, goal]).
struct XyF32 {
    int h, hi_critic, lo_critic, pad;
    HierEnc hi, lo;
    // high level: PolicyNetwork(emb, Box(-1, 1, (2,)), hiddens=[h]) + critic
    const float *hencw, *hencb;    // actor.enc_.0.0  [HP][HP], [HP]
    const float *hheads;           // [4][HP + 1]: mu_ rows 0-1, std_ rows 2-3, bias last
    const float *hv1t, *hv1b;      // critic.0        [HP][HP], [HP]
    const float *hv2;              // critic.2        [HP + 1]
    // low level: PolicyNetwork + critic
    const float *encw, *encb;      // actor.enc_.0.0  [HP][HP], [HP]
    const float *heads;            // [4][HP + 1]
    const float *lv1t, *lv1b;      // critic.0        [HP][HP], [HP]
    const float *lv2;              // critic.2        [HP + 1]
};
constexpr int kXyPtrs = 32;        // the pointers of XyF32, from hi.w1x on
static_assert(sizeof(XyF32) == 4 * sizeof(int) + kXyPtrs * sizeof(const float *), "XyF32 layout");

// Host packer: the float32 state_dict tensors of zenv_xy_weights -> one buffer; offs[] = offsets in floats of the
// pointers of XyF32 in declaration order, 0 for an absent critic.  xy_f32_at() binds such an image to its device address.
size_t pack_xy_f32(const zenv_xy_weights &w, int F, std::vector<float> &out, size_t offs[kXyPtrs]);
XyF32 xy_f32_at(const zenv_xy_weights &w, const float *base, const size_t offs[kXyPtrs]);

// The agent's per-env state is the skill family's SkillState -- skill 0 = the env has a goal, -1 = none; age = low-level
// steps under it; epi as there, so that k_skill_sync and the reset paths clear a goal as they clear a skill -- with the
// goal itself beside it: goal [N] (meaningful where skill >= 0).
// What zenv_collect_xy (xy_collect.hip) records besides the kernels' outputs, at frame t of T, N envs:
//   high level, at the first frame of window k (of W = T / L): row env * W + k of the env-major hi rows -- the obs and
//   zone_obs the goal was picked on, the goal, the critic's value, Normal(goal_mu, goal_std).log_prob(goal).sum(-1)
//   low level, every frame: the goal it acted under into lo_goal [T][N] and its distance from the robot (obs[1:3])
//   into lo_dist [T][N]; the rest goes through MlpAction::rec
struct XyRecord {
    int t, N, W, k;
    float *hi_obs, *hi_zone_obs;       // [N * W][8], [N * W][Z * F]
    float2 *hi_goal;                   // [N * W]
    float *hi_value, *hi_log_prob;     // [N * W]
    float2 *lo_goal;                   // [T][N]
    float *lo_dist;                    // [T][N]
};
// What the high-level kernel does besides goal_mu / goal_std / value: mode < 0 -- nothing, every env is evaluated; 0 / 1
// -- every env without a goal or whose age has reached skill_len, and which is not finished, gets one: goal_mu (0) or
// goal_mu + goal_std * n (1), n a Box-Muller pair keyed by (seed, global env, step) on a Philox stream of its own; only
// those envs are evaluated and written.  zenv_collect_xy adds: every = 1 -- every env picks (a window's first frame);
// mode 2 -- every env is evaluated and draws g' on a second stream into boot[N], the goal and its clock are not touched
// (the bootstrap goal).  For the low level, every = 1 evaluates every env whatever its clock says (under boot).
struct XyPick {
    int mode, skill_len;
    uint32_t step_index;
    uint64_t seed, env_index0;
    int every;
    float2 *boot;
    XyRecord rec;                       // null pointers: nothing is recorded
};
hipError_t launch_xy_high(const XyF32 &w, const DevParams &p, const SkillState &st, float2 *goal, float *goal_mu,
                          float *goal_std, float *value, const XyPick &pick, hipStream_t s);
// Low level for every env with a goal (every: for every env): mu / std / value under goal[env] as it stands, and the
// action as MlpAction asks; then, when it acts (act.mode >= 0), the age of every unfinished env with a goal goes up by
// one.  An env without a goal gets mu = std = value = 0 (and action 0).
hipError_t launch_xy_low(const XyF32 &w, const DevParams &p, const SkillState &st, const float2 *goal, float *mu,
                         float *stdv, float *value, const MlpAction &act, hipStream_t s, const XyRecord *rec = nullptr,
                         int every = 0);
// zenv_set_xy_goals: in [N] -> goal, skill 0, age 0 for every env in mask (null = all)
hipError_t launch_xy_set(const DevParams &p, const SkillState &st, float2 *goal, const float2 *in, const uint8_t *mask,
                         hipStream_t s);
// ZENV_F_XY_GOAL_AGE: age_out[env] = the env's age, -1 without a goal
hipError_t launch_xy_age(const DevParams &p, const SkillState &st, int32_t *age_out, hipStream_t s);

// ---- zenv_collect_xy (xy_collect.hip)
// After the frames, the low level's distance-to-goal reward, elementwise over [T][N]:
// reward[t] = (dist[t] - dist[t + 1]) * mask[t + 1] * ((t + 1) % L != 0), 0 at frame T - 1
hipError_t launch_xy_lo_reward(float *reward, const float *dist, const float *mask, int T, int L, int N, hipStream_t s);

}  // namespace zenvk
