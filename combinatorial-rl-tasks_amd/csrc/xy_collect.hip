// xy_collect.hip -- what zenv_collect_xy adds to the xy-goals agent's two networks (xy_f32.hip): collect_experiences of
// the xy-goals agent (xy-goals/src/torch_ac/algos/_hier_policy_opt.py:10-192), gfx950.
//
//  * k_xy_lo_reward -- after the frames: the low level's reward of :128-131, the progress towards the goal over one
//    step, from the distances k_xy_f32<1> recorded at every frame.  The env reward takes no part in it.
// The two GAE recursions are the other collectors': k_exp_gae (the low level, :123-134) and k_skill_hi_gae (the high
// level per env over its T / L regular windows, :111-120, no discount).
#include <hip/hip_runtime.h>

#include "xy_f32.hpp"

namespace zenvk {
namespace {

// lo_reward = (dist[t] - dist[t + 1]) * next_mask * ((t + 1) % L != 0): torch's float32 operations in their order
// (no FMA).  Frame T - 1 is written as 0: T is a multiple of L, so the reference multiplies its difference to
// next_lo_dist_to_goal by (T % L != 0) = 0 -- that distance, of obs_T to the bootstrap goal, is therefore not computed.
__global__ __launch_bounds__(256) void k_xy_lo_reward(float *__restrict__ reward, const float *__restrict__ dist,
                                                      const float *__restrict__ mask, int T, int L, int N)
{
    const size_t total = (size_t)T * N;
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= total) return;
    const int t = (int)(slot / (size_t)N);
    float r = 0.f;
    if (t + 1 < T) {
        const float in_window = (t + 1) % L != 0 ? 1.f : 0.f;
        r = __fmul_rn(__fsub_rn(dist[slot], dist[slot + N]), __fmul_rn(mask[slot + N], in_window));
    }
    reward[slot] = r;
}

}  // namespace

hipError_t launch_xy_lo_reward(float *reward, const float *dist, const float *mask, int T, int L, int N, hipStream_t s)
{
    const size_t total = (size_t)T * N;
    hipLaunchKernelGGL(k_xy_lo_reward, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reward, dist, mask, T, L, N);
    return hipGetLastError();
}

}  // namespace zenvk
