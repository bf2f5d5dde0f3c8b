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
// no tensor sits at offset 0).  skill_f32_at() binds such an image to its device address.  n_out: the rows of
// lo_mu_w / lo_std_w, 2 (the action) or 3 (the Options agent's, option_f32.hpp: `heads` is then [6][HP + 1]).
size_t pack_skill_f32(const zenv_skill_weights &w, int F, std::vector<float> &out, size_t offs[kSkillPtrs],
                      int n_out = 2);
SkillF32 skill_f32_at(const zenv_skill_weights &w, const float *base, const size_t offs[kSkillPtrs]);

// The per-env skill state, [N] each: skill (-1 = none), age (low-level steps under it), epi (the episode index,
// Sched::episode_idx, the skill belongs to: an env whose episode index moved on was reset since, its skill is stale)
struct SkillState {
    int32_t *skill, *age, *epi;
    int32_t *in;                   // [N] staging of zenv_set_skills
    int32_t *ended;                // [N] the Options agent's flag (option_f32.hpp): 1 = the skill's option ended on the
                                   // last policy call, the env picks on the next; cleared wherever the skill is
};
// What zenv_collect_skill (skill_collect.hip) records besides the kernels' outputs, at frame t of T, N envs:
//   high level, at the first frame of window k (of W = T / L): row env * W + k of the env-major hi rows -- the obs and
//   zone_obs the skill was picked on, the skill, the critic's value, log_softmax(x)[skill]
//   low level, every frame: the env's skill into lo_skill [T][N] (-1: none); the rest goes through MlpAction::rec
struct SkillRecord {
    int t, N, W, k;
    float *hi_obs, *hi_zone_obs;       // [N * W][8], [N * W][Z * F]
    int32_t *hi_skill;
    float *hi_value, *hi_log_prob;     // [N * W]
    int32_t *lo_skill;                 // [T][N]
};
// What the high-level kernel does besides the logits / value: mode < 0 -- nothing, every env is evaluated; 0 / 1 --
// every env that needs a skill (skill < 0 or age >= skill_len) and is not finished picks one, argmax (0) or a draw from
// Categorical(logits) (1) keyed by (seed, global env, step) on a Philox stream of its own; only those envs are
// evaluated and written.  zenv_collect_skill adds: every = 1 -- every env picks (a window's first frame); mode 2 --
// randint(0, S), a stream of its own; mode 3 -- every env is evaluated and draws s' from Categorical(logits) on a third
// stream into boot[N], the skill state is not touched (the bootstrap skill).
struct SkillPick {
    int mode, skill_len;
    uint32_t step_index;
    uint64_t seed, env_index0;
    int every;
    int32_t *boot;
    SkillRecord rec;                    // null pointers: nothing is recorded
};
hipError_t launch_skill_high(const SkillF32 &w, const DevParams &p, const SkillState &st, float *logits, float *value,
                             const SkillPick &pick, hipStream_t s);
// Low level for every env with a skill: mu / std / value, and the action as MlpAction asks (mode 0: mu, 1: Normal(mu,
// std) sample); then, when it acts (act.mode >= 0), the age of every unfinished env with a skill goes up by one.  An env
// without a skill gets mu = std = value = 0 (and action 0).
hipError_t launch_skill_low(const SkillF32 &w, const DevParams &p, const SkillState &st, float *mu, float *stdv,
                            float *value, const MlpAction &act, hipStream_t s, const SkillRecord *rec = nullptr);
// Clear (skill -1, age 0, not ended) every env whose episode index moved on, and with force also those in mask (null = all).
hipError_t launch_skill_sync(const DevParams &p, const SkillState &st, const uint8_t *mask, int force, hipStream_t s);
// st.in -> skill, age 0, not ended for every env whose entry is >= 0
hipError_t launch_skill_set(const DevParams &p, const SkillState &st, hipStream_t s);

// ---- zenv_collect_skill (skill_collect.hip)
// InverseModel (main/src/inverse_model.py): the ZoneEnvModel encoder (combine_net.0 as its combine layer), ReLU, then
// combine_net.2 -> S logits.  Layout of SkillF32.
struct SkillInvF32 {
    int h, S;
    HierEnc enc;
    const float *head;                 // combine_net.2 [S][HP + 1]: one row per skill, bias last
};
constexpr int kSkillInvPtrs = 11;      // enc (10) + head
size_t pack_skill_inverse_f32(const zenv_skill_inverse_weights &w, int F, std::vector<float> &out,
                              size_t offs[kSkillInvPtrs]);
SkillInvF32 skill_inverse_f32_at(const zenv_skill_inverse_weights &w, const float *base,
                                 const size_t offs[kSkillInvPtrs]);
// One frame's diversity reward, after the step of frame t (p.obs = obs_{t+1}, p.reward / p.done_out its results):
// diversity[t][env] = (log_softmax(inverse(obs_{t+1}))[skill] - prior[skill]) * (1 - done), 0 for a finished env or
// without a network (net = 0); exp_reward[t][env] = reward + coef * diversity (a separate multiply and add).
struct SkillDiv {
    int t, N, net;
    float coef;
    const int32_t *skill;              // lo_skill [T][N]
    float *diversity, *exp_reward;     // [T][N]
    float prior[kMaxSkills];           // log_softmax(skill_prior_logits)
};
hipError_t launch_skill_inverse(const SkillInvF32 &w, const DevParams &p, const SkillDiv &d, hipStream_t s);
// The high level's GAE per env over its W = T / L windows (no discount): reward = the window's sum of env_reward,
// next_mask = mask[(k + 1) L] (cur_mask for the last window), V_next = value of window k + 1 (v_final for the last);
// writes advantage, returnn, reward, mask of rows env * W + k (value read from o.value) and count[env] = W.
hipError_t launch_skill_hi_gae(const HierOut &o, int T, int L, int N, const float *env_reward, const float *mask,
                               const float *cur_mask, const float *v_final, float gae_lambda, int32_t *count,
                               hipStream_t s);

}  // namespace zenvk
