// option_collect.hip -- what zenv_collect_option adds to the Options agent's kernels (option_f32.hip) and to the
// semi-Markov bookkeeping of hier_collect.hip: collect_experiences of options/src/torch_ac/algos/_hier_policy_opt.py:
// 10-205, gfx950.
//
// A high-level transition opens when an env picks a skill (k_option_high records the pick at frame t) and closes when
// the termination draw of a later frame ends the option (k_option_close, after that frame's step).  The records, the
// count scan, the per-env backward GAE, the gather and the carry slot are hier_collect.hip's, with the skill in the
// goal field.  Two things are this agent's own:
//   * the close is decided by SkillState::ended, not by the env, and a termination without an open transition (a skill
//     planted by zenv_set_skills or picked by zenv_policy) closes nothing;
//   * the skill survives an auto-reset (cur_skills[j] is cleared by the termination draw alone, :74): k_option_close
//     moves SkillState::epi of every env that holds a skill to the env's current episode index, so that k_skill_sync
//     never finds it stale -- except where the option ended on the very step that ended the episode.  The step kernels
//     are untouched.
#include <hip/hip_runtime.h>

#include "option_f32.hpp"

namespace zenvk {
namespace {

__global__ __launch_bounds__(256) void k_option_enter(SkillState st, HierCarry c, int N)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N || st.skill[env] >= 0) return;
    c.open[env] = 0;
    c.hi_reward[env] = 0.f;
}

__global__ __launch_bounds__(256) void k_option_close(DevParams p, SkillState st, HierFrames f, HierCarry c, int t)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.N) return;
    const size_t slot = (size_t)t * p.N + env;
    const float r = p.reward[env];
    f.env_reward[slot] = r;
    float hr = c.hi_reward[env] + r;                           // self.hi_reward += self.rewards[i] (float32)
    const bool ended = st.ended[env] != 0, done = p.done_out[env] != 0;
    if (ended) {                                               // torch.rand(()) < termination_prob[j] (:68)
        if (c.open[env]) {
            f.close_reward[slot] = hr;
            f.close_flag[slot] = done ? 2 : 1;                  // self.hi_mask[j] = 0 if done[j] else 1
            f.count[env] += 1;
            c.open[env] = 0;
        }
        hr = 0.f;
    }
    // the skill goes on in the env's next episode; one that ended together with its episode is left behind (the env
    // picks either way, and k_skill_sync finds it as it finds any skill after a reset)
    if (st.skill[env] >= 0 && !(ended && done)) st.epi[env] = p.sched[env].episode_idx;
    c.hi_reward[env] = hr;
}

}  // namespace

hipError_t launch_option_enter(const SkillState &st, const HierCarry &c, int N, hipStream_t s)
{
    hipLaunchKernelGGL(k_option_enter, dim3((N + 255) / 256), dim3(256), 0, s, st, c, N);
    return hipGetLastError();
}

hipError_t launch_option_close(const DevParams &p, const SkillState &st, const HierFrames &f, const HierCarry &c, int t,
                               hipStream_t s)
{
    hipLaunchKernelGGL(k_option_close, dim3((p.N + 255) / 256), dim3(256), 0, s, p, st, f, c, t);
    return hipGetLastError();
}

}  // namespace zenvk
