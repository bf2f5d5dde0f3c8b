// skill_f32.hpp -- the fixed-length-skills agent on the device (main/src/hier_policy_value_models.py:19-76,
// main/scripts/evaluate_hier.py:48-84): HighPolicyValueModel picks one of S skills every skill_len steps,
// LoPolicyValueModel acts under it.  float32 throughout (skill_f32.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "../../include/zenv.h"
#include "dev_params.hpp"
#include "hier_f32.hpp"
#include "mlp_policy.hpp"

namespace zenvk {

constexpr int kMaxSkills = 32;

// Every matrix TRANSPOSED ([in][kMlpHP]) and zero-padded to kMlpHP columns, device pointers (the layout of HierF32).
// Both encoders are ZoneEnvModel-shaped (XIN = 8: obs); the low level's one-hot skill enters as one column per env of
// zone_net_.0, combine_net_, actor.enc_.0.0 and critic.0 ([S][HP] each).
struct SkillF32 {
    int h, S, hi_critic, lo_critic;
    HierEnc hi, lo;
    const float *lo_w1s, *lo_wcs;  // skill columns of the low level's zone_net_.0 / combine_net_  [S][HP]
    // high level: PolicyNetwork(emb, Discrete(S), hiddens=[h]) + critic
    const float *hencw, *hencb;    // actor.enc_.0.0     [HP][HP], [HP]
    const float *hdisc;            // actor.discrete_.0  [S][HP + 1]: one row per skill, bias last
    const float *hv1t, *hv1b;      // critic.0           [HP][HP], [HP]
    const float *hv2;              // critic.2           [HP + 1]
    // low level: PolicyNetwork([emb, onehot], Box) + critic on [emb, onehot]
    const float *encw, *encs, *encb;  // actor.enc_.0.0  [HP][HP] (emb columns), [S][HP] (skill columns), [HP]
    const float *heads;               // [4][HP + 1]: mu_ rows 0-1, std_ rows 2-3, bias last
    const float *lv1t, *lv1s, *lv1b;  // critic.0        [HP][HP], [S][HP], [HP]
    const float *lv2;                 // critic.2        [HP + 1]
};
constexpr int kSkillPtrs = 36;     // the pointers of SkillF32, from hi.w1x on
static_assert(sizeof(SkillF32) == 4 * sizeof(int) + kSkillPtrs * sizeof(const float *), "SkillF32 layout");

// Host packer: the float32 state_dict tensors of zenv_skill_weights -> one buffer; offs[] = offsets in floats of the
// pointers of SkillF32 in declaration order, 0 for an absent critic (the image starts with 4 floats of padding, so that
// no tensor sits at offset 0).  skill_f32_at() binds such an image to its device address.
size_t pack_skill_f32(const zenv_skill_weights &w, int F, std::vector<float> &out, size_t offs[kSkillPtrs]);
SkillF32 skill_f32_at(const zenv_skill_weights &w, const float *base, const size_t offs[kSkillPtrs]);

// The per-env skill state, [N] each: skill (-1 = none), age (low-level steps under it), epi (the episode index,
// Sched::episode_idx, the skill belongs to: an env whose episode index moved on was reset since, its skill is stale)
struct SkillState {
    int32_t *skill, *age, *epi;
    int32_t *in;                   // [N] staging of zenv_set_skills
};
// What the high-level kernel does besides the logits / value: mode < 0 -- nothing, every env is evaluated; 0 / 1 --
// every env that needs a skill (skill < 0 or age >= skill_len) and is not finished picks one, argmax (0) or a draw from
// Categorical(logits) (1) keyed by (seed, global env, step) on a Philox stream of its own; only those envs are
// evaluated and written.
struct SkillPick {
    int mode, skill_len;
    uint32_t step_index;
    uint64_t seed, env_index0;
};
hipError_t launch_skill_high(const SkillF32 &w, const DevParams &p, const SkillState &st, float *logits, float *value,
                             const SkillPick &pick, hipStream_t s);
// Low level for every env with a skill: mu / std / value, and the action as MlpAction asks (mode 0: mu, 1: Normal(mu,
// std) sample); then, when it acts (act.mode >= 0), the age of every unfinished env with a skill goes up by one.  An env
// without a skill gets mu = std = value = 0 (and action 0).
hipError_t launch_skill_low(const SkillF32 &w, const DevParams &p, const SkillState &st, float *mu, float *stdv,
                            float *value, const MlpAction &act, hipStream_t s);
// Clear (skill -1, age 0) every env whose episode index moved on, and with force also those in mask (null = all).
hipError_t launch_skill_sync(const DevParams &p, const SkillState &st, const uint8_t *mask, int force, hipStream_t s);
// st.in -> skill, age 0 for every env whose entry is >= 0
hipError_t launch_skill_set(const DevParams &p, const SkillState &st, hipStream_t s);

}  // namespace zenvk
