// xy_f32.hip -- the xy-goals hierarchical agent (xy-goals/src/hier_policy_value_models.py:19-72) in float32, gfx950.
//
// Two launches of one kernel template on the vector ALU, with the building blocks and the workgroup layout of
// hier_f32.hip (hier_enc.hpp: 192 threads = hidden features, EB = 4 envs per workgroup):
//  * k_xy_f32<0> -- HighPolicyValueModel, the flat actor-critic's network: emb = ZoneEnvModel(obs, zone_obs); x = relu(
//    actor.enc_.0.0(emb)); goal_mu = 2 (sigmoid(actor.mu_(x)) - 0.5), goal_std = sigmoid(actor.std_(x)) + 1e-3; value =
//    critic.2(relu(critic.0(emb))).  When it picks, the goal (goal_mu, or goal_mu + goal_std * n) goes into the agent's
//    float2 goal buffer, and a workgroup none of whose envs picks leaves at once: the high level costs what the envs
//    that pick cost (one in skill_len steps).
//  * k_xy_f32<1> -- LoPolicyValueModel, the Zone-goals low level under another goal: ZoneEnvGoalModel's [obs, goal] is
//    the same for every zone row of an env, so it folds into a per-env bias of zone_net_.0 and a per-env term of
//    combine_net_ (k_hier_f32<1>); the goal is the float2 buffer's as it stands -- the high level's float32 sample,
//    unclipped.  Then PolicyNetwork's mu_ / std_, the Normal sample of mlp_head_out.hpp, and the goal's age.
// Only the summation order differs from torch's: within 1e-5 of the reference's float32 modules.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "f32_packer.hpp"
#include "skill_net.hpp"
#include "xy_f32.hpp"

namespace zenvk {
namespace {

using namespace hf32;

// the goal draw's Philox stream (the action draw of mlp_head_out.hpp uses the tag 0x4D4C50, the Zone-goals goal draw
// 0x48474C, the skill draw 0x534B4C)
constexpr uint32_t kXyGoalTag = 0x585947u;

// goal = mu + std * n, n the Box-Muller pair of words 0 and 1 of the goal stream's block: the arithmetic of mlp_action
__device__ __forceinline__ float2 xy_goal_draw(const XyPick &pick, int env, float2 m, float2 sd)
{
    const PhiloxWords c = philox_words(pick.seed, pick.env_index0 + (uint64_t)env, pick.step_index, kXyGoalTag);
    const float u1 = u01(c.w[0]), u2 = u01(c.w[1]);
    const float rad = sqrtf(-2.0f * logf(u1));
    return make_float2(m.x + sd.x * rad * cosf(6.283185307179586f * u2), m.y + sd.y * rad * sinf(6.283185307179586f * u2));
}

// LEVEL 0: HighPolicyValueModel -> out0 = goal_mu [N][2], out1 = goal_std [N][2], out2 = value [N] (+ the goal pick)
// LEVEL 1: LoPolicyValueModel   -> out0 = mu [N][2], out1 = std [N][2], out2 = value [N] (+ the action, the age)
template <int LEVEL>
__global__ __launch_bounds__(HP) void k_xy_f32(XyF32 w, DevParams p, SkillState st, float2 *__restrict__ goal,
                                               float *__restrict__ out0, float *__restrict__ out1,
                                               float *__restrict__ out2, XyPick pick, MlpAction act)
{
    constexpr int XIN = LEVEL ? 10 : 8;                 // [obs] or [obs, goal]
    __shared__ __align__(16) float x0[ZF * RP];         // zone rows of the pass       [k][row]
    __shared__ __align__(16) float y1[HP * RP];         // activations of the pass     [k][row]
    __shared__ float xin[EB * XP];                      // per-env input
    __shared__ float peb[EB * HP];
    __shared__ float va[EB * HP];
    __shared__ float vb[EB * HP];
    __shared__ float hd[EB * 8];
    __shared__ int on[EB];
    const int j = threadIdx.x;
    const int h = w.h;
    const bool live = j < h;                             // padded features stay exactly 0
    const int env0 = blockIdx.x * EB;
    const int n_env = min(EB, p.N - env0);
    const bool has_critic = LEVEL ? w.lo_critic : w.hi_critic;

    // ---- which envs are evaluated: high -- all (forward) or those that get a goal; low -- those with a goal
    if (j < EB) {
        int a = 0;
        if (j < n_env) {
            const int env = env0 + j;
            if (LEVEL == 0)
                a = pick.mode < 0 ||
                    ((st.skill[env] < 0 || st.age[env] >= pick.skill_len) && !p.sched[env].done_state);
            else
                a = st.skill[env] >= 0;
        }
        on[j] = a;
    }
    __syncthreads();
    if (!(on[0] | on[1] | on[2] | on[3])) {
        if (LEVEL == 1 && j < n_env) idle_outputs(env0 + j, out0, out1, out2, act);
        return;
    }
    if (j < EB * XP) {
        const int e = j / XP, k = j % XP;
        float v = 0.f;
        if (e < n_env) {
            const int env = env0 + e;
            if (k < 8) {
                v = p.obs[(size_t)env * 8 + k];
            } else if (LEVEL == 1 && k < 10 && on[e]) {
                const float2 g = goal[env];
                v = k == 8 ? g.x : g.y;
            }
        }
        xin[j] = v;
    }
    __syncthreads();
    encode_envs<XIN>(LEVEL ? w.lo : w.hi, p, xin, nullptr, nullptr, nullptr, env0, n_env, h, j, x0, y1, peb, va, vb);

    // ---- vb = emb: relu(actor.enc_.0.0(emb)) -> va, relu(critic.0(emb)) -> peb (0 without a critic)
    {
        float t[EB], hv[EB];
#pragma unroll
        for (int e = 0; e < EB; ++e) hv[e] = 0.f;
        if (has_critic) matvec(hv, LEVEL ? w.lv1t : w.hv1t, LEVEL ? w.lv1b : w.hv1b, vb, HP, h, j);
        matvec(t, LEVEL ? w.encw : w.hencw, LEVEL ? w.encb : w.hencb, vb, HP, h, j);
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            va[e * HP + j] = live ? fmaxf(t[e], 0.f) : 0.f;
            peb[e * HP + j] = live ? fmaxf(hv[e], 0.f) : 0.f;
        }
        __syncthreads();
    }

    // ---- mu_, std_ on va, critic.2 on peb: one thread per (env, row)
    if (j < EB * 8) {
        const int e = j >> 3, row = j & 7;
        float s = 0.f;
        if (row < 4) s = dot_row((LEVEL ? w.heads : w.hheads) + (size_t)row * (HP + 1), va + e * HP, h);
        else if (row == 4 && has_critic) s = dot_row(LEVEL ? w.lv2 : w.hv2, peb + e * HP, h);
        hd[j] = s;
    }
    __syncthreads();
    if (j >= n_env) return;
    const int env = env0 + j;
    const float *o = hd + 8 * j;
    if (LEVEL == 0) {
        if (!on[j]) return;
        // PolicyNetwork's Normal, as head_outputs forms the low level's
        const float2 m = make_float2(2.0f * (sigmoidf_(o[0]) - 0.5f), 2.0f * (sigmoidf_(o[1]) - 0.5f));
        const float2 sd = make_float2(sigmoidf_(o[2]) + 1e-3f, sigmoidf_(o[3]) + 1e-3f);
        reinterpret_cast<float2 *>(out0)[env] = m;
        reinterpret_cast<float2 *>(out1)[env] = sd;
        out2[env] = o[4];
        if (pick.mode >= 0) {
            goal[env] = pick.mode == 1 ? xy_goal_draw(pick, env, m, sd) : m;
            st.skill[env] = 0;
            st.age[env] = 0;
        }
        return;
    }
    if (on[j]) {
        out2[env] = o[4];
        head_outputs(env, o[0], o[1], o[2], o[3], o[4], out0, out1, act);
        if (act.mode >= 0 && !p.sched[env].done_state) st.age[env] += 1;
    } else {
        idle_outputs(env, out0, out1, out2, act);
    }
}

__global__ __launch_bounds__(256) void k_xy_set(DevParams p, SkillState st, float2 *__restrict__ goal,
                                                const float2 *__restrict__ in, const uint8_t *__restrict__ mask)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.N || (mask && !mask[env])) return;
    goal[env] = in[env];
    st.skill[env] = 0;
    st.age[env] = 0;
    st.ended[env] = 0;
}

__global__ __launch_bounds__(256) void k_xy_age(DevParams p, SkillState st, int32_t *__restrict__ age_out)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.N) return;
    age_out[env] = st.skill[env] >= 0 ? st.age[env] : -1;
}

}  // namespace

size_t pack_xy_f32(const zenv_xy_weights &w, int F, std::vector<float> &out, size_t offs[kXyPtrs])
{
    const int h = w.h_dim;
    Packer pk(out, h);
    int i = 0;
    pk.enc(offs, i, w.hi_zone_w1, w.hi_zone_b1, w.hi_zone_w2, w.hi_zone_b2, w.hi_zone_w3, w.hi_zone_b3, w.hi_comb_w,
           w.hi_comb_b, F, 8, 0);
    pk.enc(offs, i, w.lo_zone_w1, w.lo_zone_b1, w.lo_zone_w2, w.lo_zone_b2, w.lo_zone_w3, w.lo_zone_b3, w.lo_comb_w,
           w.lo_comb_b, F, 10, 0);
    const bool hc = w.hi_critic_w1 != nullptr, lc = w.lo_critic_w1 != nullptr;
    offs[i++] = pk.cols(w.hi_enc_w, h, 0, h, HP);
    offs[i++] = pk.bias(w.hi_enc_b);
    offs[i++] = pk.head_rows(w.hi_mu_w, w.hi_mu_b, w.hi_std_w, w.hi_std_b, 2);
    offs[i++] = hc ? pk.cols(w.hi_critic_w1, h, 0, h, HP) : 0;
    offs[i++] = hc ? pk.bias(w.hi_critic_b1) : 0;
    offs[i++] = hc ? pk.rows(w.hi_critic_w2, w.hi_critic_b2, 1) : 0;
    offs[i++] = pk.cols(w.lo_enc_w, h, 0, h, HP);
    offs[i++] = pk.bias(w.lo_enc_b);
    offs[i++] = pk.head_rows(w.lo_mu_w, w.lo_mu_b, w.lo_std_w, w.lo_std_b, 2);
    offs[i++] = lc ? pk.cols(w.lo_critic_w1, h, 0, h, HP) : 0;
    offs[i++] = lc ? pk.bias(w.lo_critic_b1) : 0;
    offs[i++] = lc ? pk.rows(w.lo_critic_w2, w.lo_critic_b2, 1) : 0;
    return out.size();
}

XyF32 xy_f32_at(const zenv_xy_weights &w, const float *base, const size_t offs[kXyPtrs])
{
    XyF32 s{};
    s.h = w.h_dim;
    s.hi_critic = w.hi_critic_w1 ? 1 : 0;
    s.lo_critic = w.lo_critic_w1 ? 1 : 0;
    bind_pointers(s, offsetof(XyF32, hi), base, offs, kXyPtrs);
    return s;
}

hipError_t launch_xy_high(const XyF32 &w, const DevParams &p, const SkillState &st, float2 *goal, float *goal_mu,
                          float *goal_std, float *value, const XyPick &pick, hipStream_t s)
{
    hipLaunchKernelGGL(k_xy_f32<0>, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, st, goal, goal_mu, goal_std, value,
                       pick, no_mlp_action());
    return hipGetLastError();
}

hipError_t launch_xy_low(const XyF32 &w, const DevParams &p, const SkillState &st, const float2 *goal, float *mu,
                         float *stdv, float *value, const MlpAction &act, hipStream_t s)
{
    const XyPick none{ -1, 0, 0u, 0ull, 0ull };
    hipLaunchKernelGGL(k_xy_f32<1>, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, st, const_cast<float2 *>(goal), mu,
                       stdv, value, none, act);
    return hipGetLastError();
}

hipError_t launch_xy_set(const DevParams &p, const SkillState &st, float2 *goal, const float2 *in, const uint8_t *mask,
                         hipStream_t s)
{
    hipLaunchKernelGGL(k_xy_set, dim3((p.N + 255) / 256), dim3(256), 0, s, p, st, goal, in, mask);
    return hipGetLastError();
}

hipError_t launch_xy_age(const DevParams &p, const SkillState &st, int32_t *age_out, hipStream_t s)
{
    hipLaunchKernelGGL(k_xy_age, dim3((p.N + 255) / 256), dim3(256), 0, s, p, st, age_out);
    return hipGetLastError();
}

}  // namespace zenvk
