// option_f32.hpp -- the variable-length Options agent on the device (options/src/hier_policy_value_models.py,
// options/scripts/evaluate_hier.py:55-84): the skill planner's two networks with a third actor output whose sample
// decides, after every low-level action, whether the skill ends.  float32 throughout (option_f32.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "skill_f32.hpp"

namespace zenvk {

// The weights are a SkillF32 whose `heads` is [6][HP + 1]: mu_ rows 0-2, std_ rows 3-5 (pack_skill_f32 with n_out = 3).
// The per-env state is the skill family's SkillState; its `ended` flag is what this agent adds.

// The Philox stream of the termination draw (the skill draw uses 0x534B4C, the action draw 0x4D4C50, whose words 2 and
// 3 give the third action component's normal)
constexpr uint32_t kOptionTermTag = 0x4F5054u;

// The envs that pick on this call, compacted: list[0 .. *count - 1] in no particular order.  launch_option_list fills
// it, launch_option_low (when it acts) leaves *count = 0 for the next call.
struct OptionList {
    int32_t *list;                     // [N]
    int32_t *count;                    // [1]
};
// mode < 0: every env is evaluated, nothing is picked (zenv_option_forward).  0 / 1: every unfinished env without a
// skill or whose option ended picks one (age 0) -- argmax (0), or a draw from Categorical(logits) (1), the draw of
// SkillPick mode 1 -- and only those are evaluated and written.  compact = 0: workgroup b owns envs 4 b .. 4 b + 3 and
// leaves when none of them picks; 1: it owns entries 4 b .. 4 b + 3 of the list and leaves when they lie beyond *count.
// Measured: the list wins by a fifth at 65 536 envs and loses the cost of its launch at 500.  The
// default is the list once the high level's N / 4 workgroups no longer all fit on the device at once (256 CUs x 4
// workgroups of 35 KB LDS): below that a workgroup that stays costs no time, above it costs a slot.
constexpr int kOptionCompactMinEnvs = 4096;
struct OptionPick {
    int mode, compact;
    uint32_t step_index;
    uint64_t seed, env_index0;
};
// What zenv_collect_option records at frame t besides the kernels' outputs, time-major [T][N] (null pick_skill:
// nothing is recorded, and every other output is what it is without a record):
//   high level, for every env that picks: the skill, the critic's value and log_softmax(logits)[skill] into the
//   HierFrames pick fields (the skill in the goal field), open[env] = 1 (HierCarry: a high-level transition is open)
//   low level, every env: the skill it acted under (-1: it idled), a_2, Normal(mu_2, std_2).log_prob(a_2) and the
//   termination draw; the rest of frame t goes through MlpAction::rec (head_outputs / idle_outputs)
struct OptionRecord {
    int t, N;
    int32_t *pick_skill;
    float *pick_value, *pick_log_prob;
    uint8_t *open;
    int32_t *lo_skill;
    float *term_action, *term_log_prob;
    uint8_t *ended;
};
hipError_t launch_option_list(const DevParams &p, const SkillState &st, const OptionList &ol, hipStream_t s);
hipError_t launch_option_high(const SkillF32 &w, const DevParams &p, const SkillState &st, const OptionList &ol,
                              float *logits, float *value, const OptionPick &pick, hipStream_t s,
                              const OptionRecord &rec = OptionRecord{});
// The third component's outputs, [N] each: mu_2, std_2, a_2 (the sample, or mu_2), prob = sigmoid(4 a_2 - 3)
struct OptionTerm {
    float *mu, *stdv, *action, *prob;
};
// Low level for every env with a skill (when it acts, act.mode >= 0: every UNFINISHED env with one): mu / std [N][2],
// value, the action as MlpAction asks, the OptionTerm fields; when it acts also st.ended (mode 1: u < prob on the
// kOptionTermTag stream, mode 0: prob > 0.5) and age + 1.  Every other env gets zeros everywhere (ended = 0).
hipError_t launch_option_low(const SkillF32 &w, const DevParams &p, const SkillState &st, const OptionList &ol,
                             float *mu, float *stdv, float *value, const OptionTerm &term, const MlpAction &act,
                             hipStream_t s, const OptionRecord &rec = OptionRecord{});

// ---- zenv_collect_option (option_collect.hip): the high level's transitions are semi-Markov like the Zone-goals
// agent's, so the bookkeeping is hier_collect.hip's (HierFrames / HierCarry / HierOut, the skill in the goal field);
// what differs is when a transition closes and that the skill outlives an auto-reset.
// Once per call, after launch_skill_sync: an env that enters without a skill has no open transition (hi_reward 0).
hipError_t launch_option_enter(const SkillState &st, const HierCarry &c, int N, hipStream_t s);
// After the step of frame t (_hier_policy_opt.py:62-75): env reward, hi_reward, and for every env whose option ended
// the close of its open transition (reward hi_reward, hi_mask 0 if done else 1; hi_reward restarts at 0 either way).
// Every env that holds a skill takes the env's current episode index into SkillState::epi, unless its option ended on
// the step that ended its episode: the skill, its open transition and hi_reward run across the auto-reset
// (cur_skills[j] is cleared by the termination draw alone, :74).
hipError_t launch_option_close(const DevParams &p, const SkillState &st, const HierFrames &f, const HierCarry &c, int t,
                               hipStream_t s);

}  // namespace zenvk
