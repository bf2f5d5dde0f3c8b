// skill_collect.hip -- what zenv_collect_skill adds to the skill agent's two networks (skill_f32.hip): collect_experiences
// of the fixed-length-skills agent and DIAYN (main/src/torch_ac/algos/_hier_policy_opt.py:9-233), gfx950.
//
//  * k_skill_inverse_f32 -- after the step of every frame: InverseModel (main/src/inverse_model.py) on obs_{t+1}, the
//    encoder of hier_enc.hpp (the workgroup layout of skill_f32.hip: 192 threads = hidden features, EB = 4 envs), ReLU,
//    one length-h dot product per (env, skill) thread, then the diversity reward of :83-88 and the low level's reward
//    of :91.  A workgroup whose envs are all done (diversity 0) skips the network.
//  * k_skill_hi_gae -- after the frames: the high level's GAE (:142-151, no discount) per env over its T / L windows.
//    The windows are regular, so the env-major rows are addressed directly: no scan, no gather (the picks wrote their
//    obs, skill, value and log_prob into those rows already).
#include <hip/hip_runtime.h>

#include <cmath>

#include "hier_enc.hpp"
#include "skill_f32.hpp"

namespace zenvk {
namespace {

using namespace hf32;

constexpr int SR = kMaxSkills;      // per env: S logit rows

__device__ __forceinline__ void div_out(const SkillDiv &d, const DevParams &p, int env, float div)
{
    const size_t slot = (size_t)d.t * d.N + env;
    d.diversity[slot] = div;
    // lo_reward = reward + diversity_coef * diversity: rounded as torch's two float32 operations (no FMA)
    d.exp_reward[slot] = __fadd_rn(p.reward[env], __fmul_rn(d.coef, div));
}

__global__ __launch_bounds__(HP) void k_skill_inverse_f32(SkillInvF32 w, DevParams p, SkillDiv d)
{
    __shared__ __align__(16) float x0[ZF * RP];
    __shared__ __align__(16) float y1[HP * RP];
    __shared__ float xin[EB * XP];
    __shared__ float peb[EB * HP];
    __shared__ float va[EB * HP];
    __shared__ float vb[EB * HP];
    __shared__ float lg[EB * SR];
    __shared__ int on[EB];
    const int j = threadIdx.x;
    const int h = w.h, S = w.S;
    const bool live = j < h;
    const int env0 = blockIdx.x * EB;
    const int n_env = min(EB, p.N - env0);

    if (j < EB) on[j] = d.net && j < n_env && !p.done_out[env0 + j];     // * ~done: a finished env's reward is 0
    __syncthreads();
    if (!(on[0] | on[1] | on[2] | on[3])) {
        if (j < n_env) div_out(d, p, env0 + j, 0.f);
        return;
    }
    if (j < EB * XP) {
        const int e = j / XP, k = j % XP;
        xin[j] = e < n_env && k < 8 ? p.obs[(size_t)(env0 + e) * 8 + k] : 0.f;
    }
    __syncthreads();
    encode_envs<8>(w.enc, p, xin, nullptr, nullptr, nullptr, env0, n_env, h, j, x0, y1, peb, va, vb);
    // combine_net.1: ReLU of the embedding (vb) -> va
#pragma unroll
    for (int e = 0; e < EB; ++e) va[e * HP + j] = live ? fmaxf(vb[e * HP + j], 0.f) : 0.f;
    __syncthreads();
    // combine_net.2: one thread per (env, skill)
    if (j < EB * SR) {
        const int e = j / SR, r = j - e * SR;
        float s = 0.f;
        if (r < S) {
            const float *row = w.head + (size_t)r * (HP + 1);
            s = row[HP];
            for (int k = 0; k < h; ++k) s = __builtin_fmaf(row[k], va[e * HP + k], s);
        }
        lg[j] = s;
    }
    __syncthreads();
    if (j < n_env) {
        const int env = env0 + j;
        float div = 0.f;
        if (on[j]) {
            const float *L = lg + j * SR;
            const int sk = d.skill[(size_t)d.t * d.N + env];
            float m = L[0];
            for (int s = 1; s < S; ++s) m = fmaxf(m, L[s]);
            float sum = 0.f;
            for (int s = 0; s < S; ++s) sum += expf(L[s] - m);
            if (sk >= 0 && sk < S) div = ((L[sk] - m) - logf(sum)) - d.prior[sk];
        }
        div_out(d, p, env, div);
    }
}

// _hier_policy_opt.py:142-151 for one env, windows in reverse
__global__ __launch_bounds__(256) void k_skill_hi_gae(HierOut o, int T, int L, int N, const float *__restrict__ env_reward,
                                                      const float *__restrict__ mask, const float *__restrict__ cur_mask,
                                                      const float *__restrict__ v_final, float lambda,
                                                      int32_t *__restrict__ count)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    const int W = T / L;
    float vn = v_final[env], an = 0.f;
    for (int k = W - 1; k >= 0; --k) {
        float r = 0.f;                                          // hi_rewards = rewards of the window, summed
        for (int i = k * L; i < (k + 1) * L; ++i) r += env_reward[(size_t)i * N + env];
        const float m = k + 1 < W ? mask[(size_t)(k + 1) * L * N + env] : cur_mask[env];
        const size_t row = (size_t)env * W + k;
        const float v = o.value[row];
        const float delta = r + vn * m - v;
        const float adv = delta + lambda * an * m;
        o.advantage[row] = adv;
        o.returnn[row] = v + adv;
        o.reward[row] = r;
        o.mask[row] = m;
        vn = v;
        an = adv;
    }
    count[env] = W;
}

}  // namespace

hipError_t launch_skill_inverse(const SkillInvF32 &w, const DevParams &p, const SkillDiv &d, hipStream_t s)
{
    hipLaunchKernelGGL(k_skill_inverse_f32, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, d);
    return hipGetLastError();
}

hipError_t launch_skill_hi_gae(const HierOut &o, int T, int L, int N, const float *env_reward, const float *mask,
                               const float *cur_mask, const float *v_final, float gae_lambda, int32_t *count,
                               hipStream_t s)
{
    hipLaunchKernelGGL(k_skill_hi_gae, dim3((N + 255) / 256), dim3(256), 0, s, o, T, L, N, env_reward, mask, cur_mask,
                       v_final, gae_lambda, count);
    return hipGetLastError();
}

}  // namespace zenvk
