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
// Inside zenv_collect_xy (xy_collect.hip) both epilogues also record: the high level the pick's row (obs, zone_obs, goal,
// value, log_prob summed over the goal's dimensions) and, in a bootstrap mode of its own, g'; the low level the goal it
// acted under and its distance from the robot.  Without an XyRecord the outputs are what they are without the collector.
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
// 0x48474C, the skill draws 0x534B4C / 0x534B55 / 0x534B42, the Options agent's termination 0x4F5054); the bootstrap goal
// g' of zenv_collect_xy has a stream of its own, so that it is not the first pick of the next call
constexpr uint32_t kXyGoalTag = 0x585947u;
constexpr uint32_t kXyBootTag = 0x585942u;

// goal = mu + std * n, n the Box-Muller pair of words 0 and 1 of the goal stream's block: the arithmetic of mlp_action
__device__ __forceinline__ float2 xy_goal_draw(const XyPick &pick, int env, float2 m, float2 sd, uint32_t tag)
{
    const PhiloxWords c = philox_words(pick.seed, pick.env_index0 + (uint64_t)env, pick.step_index, tag);
    const float u1 = u01(c.w[0]), u2 = u01(c.w[1]);
    const float rad = sqrtf(-2.0f * logf(u1));
    return make_float2(m.x + sd.x * rad * cosf(6.283185307179586f * u2), m.y + sd.y * rad * sinf(6.283185307179586f * u2));
}

// inside zenv_collect_xy, frame t of the low level: the goal it acted under and its distance from the robot, obs[1:3] of
// the observation the action is taken on -- torch's float32 pow(pow(goal - xy, 2).sum(-1), 0.5) bit for bit (no FMA)
__device__ __forceinline__ void xy_record_goal(const XyRecord &xr, int env, float2 g, float x, float y)
{
    const size_t slot = (size_t)xr.t * xr.N + env;
    const float dx = __fsub_rn(g.x, x), dy = __fsub_rn(g.y, y);
    xr.lo_goal[slot] = g;
    // the root through float64: HIP's __fsqrt_rn is the hardware's approximate root here (1 ulp off now and then), while
    // a float64 root of a float32, rounded back to float32, is the correctly rounded float32 root (53 >= 2 * 24 + 2 bits)
    xr.lo_dist[slot] = (float)sqrt((double)__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
}

// an env without a goal: idle_outputs, and inside zenv_collect_xy goal 0 at distance 0 for frame t
__device__ __forceinline__ void xy_idle(int env, float *__restrict__ mu, float *__restrict__ stdv,
                                        float *__restrict__ value, const MlpAction &act, const XyRecord &xr)
{
    idle_outputs(env, mu, stdv, value, act);
    if (act.mode >= 0 && xr.lo_goal) {
        const size_t slot = (size_t)xr.t * xr.N + env;
        xr.lo_goal[slot] = make_float2(0.f, 0.f);
        xr.lo_dist[slot] = 0.f;
    }
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
                a = pick.mode < 0 || pick.mode == 2 || pick.every ||
                    ((st.skill[env] < 0 || st.age[env] >= pick.skill_len) && !p.sched[env].done_state);
            else
                a = pick.every || st.skill[env] >= 0;
        }
        on[j] = a;
    }
    __syncthreads();
    if (!(on[0] | on[1] | on[2] | on[3])) {
        if (LEVEL == 1 && j < n_env) xy_idle(env0 + j, out0, out1, out2, act, pick.rec);
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
    if (LEVEL == 0 && pick.rec.hi_obs) {
        // zenv_collect_xy: the obs and zone_obs every picking env picks on, into its row env * W + k
        const XyRecord &xr = pick.rec;
        const int ZFn = p.Z * p.F;
        for (int i = j; i < EB * (8 + ZFn); i += HP) {
            const int e = i / (8 + ZFn), k = i - e * (8 + ZFn);
            if (e >= n_env || !on[e]) continue;
            const size_t env = (size_t)(env0 + e), row = env * xr.W + xr.k;
            if (k < 8) xr.hi_obs[row * 8 + k] = p.obs[env * 8 + k];
            else xr.hi_zone_obs[row * ZFn + (k - 8)] = p.zone_obs[env * ZFn + (k - 8)];
        }
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
        if (pick.mode == 2) {                             // the bootstrap goal: the state stays as it is
            pick.boot[env] = xy_goal_draw(pick, env, m, sd, kXyBootTag);
        } else if (pick.mode >= 0) {
            const float2 g = pick.mode == 1 ? xy_goal_draw(pick, env, m, sd, kXyGoalTag) : m;
            goal[env] = g;
            st.skill[env] = 0;
            st.age[env] = 0;
            const XyRecord &xr = pick.rec;
            if (xr.hi_goal) {                             // zenv_collect_xy: the pick's row
                const size_t row = (size_t)env * xr.W + xr.k;
                xr.hi_goal[row] = g;
                xr.hi_value[row] = o[4];
                // Normal(goal_mu, goal_std).log_prob(goal).sum(-1), each term as head_outputs forms the action's
                const float z0 = (g.x - m.x) / sd.x, z1 = (g.y - m.y) / sd.y;
                xr.hi_log_prob[row] = (-0.5f * z0 * z0 - logf(sd.x) - 0.91893853320467274178f) +
                                      (-0.5f * z1 * z1 - logf(sd.y) - 0.91893853320467274178f);
            }
        }
        return;
    }
    if (on[j]) {
        out2[env] = o[4];
        head_outputs(env, o[0], o[1], o[2], o[3], o[4], out0, out1, act);
        if (act.mode >= 0 && !p.sched[env].done_state) st.age[env] += 1;
        if (act.mode >= 0 && pick.rec.lo_goal) {
            const float *x = xin + j * XP;                // [obs, goal] of this env
            xy_record_goal(pick.rec, env, make_float2(x[8], x[9]), x[1], x[2]);
        }
    } else {
        xy_idle(env, out0, out1, out2, act, pick.rec);
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
                         float *stdv, float *value, const MlpAction &act, hipStream_t s, const XyRecord *rec, int every)
{
    XyPick none{ -1, 0, 0u, 0ull, 0ull, every, nullptr, XyRecord{} };
    if (rec) none.rec = *rec;
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
