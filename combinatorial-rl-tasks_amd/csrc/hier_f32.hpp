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

// Host packer: the float32 state_dict tensors of zenv_hier_weights -> one buffer; offs[] = offsets in floats of the
// pointers of HierF32 in declaration order (HierF32 fields from `hi.w1x` on), 0 for an absent critic.
constexpr int kHierOffs = 33;
size_t pack_hier_f32(const zenv_hier_weights &w, int F, std::vector<float> &out, size_t offs[kHierOffs]);

// What the high-level kernel does besides the logits / value: nothing (mode < 0: every env is evaluated), or pick a
// goal for every env that needs one and is not finished -- argmax (0) or a draw from Categorical(logits) (1), keyed by
// (seed, global env, step) on a Philox stream of its own -- into new_goal[N] (-1 = leave the env alone), the buffer
// launch_goal_set reads.  In modes 0 / 1 only the envs that pick are evaluated and written.
struct HierPick {
    int mode;
    uint32_t step_index;
    uint64_t seed, env_index0;
    int32_t *new_goal;
};
hipError_t launch_hier_high(const HierF32 &w, const DevParams &p, float *logits, float *value, const HierPick &pick,
                            hipStream_t s);
// Low level for every env with a goal (p.goal >= 0): mu / std / value, and the action as MlpAction asks (mode 0: mu,
// 1: Normal(mu, std) sample).  An env without a goal gets mu = std = value = 0 (and action 0).
hipError_t launch_hier_low(const HierF32 &w, const DevParams &p, float *mu, float *stdv, float *value,
                           const MlpAction &act, hipStream_t s);

}  // namespace zenvk
