// option_f32.hip -- the variable-length Options agent (options/src/hier_policy_value_models.py) in float32, gfx950.
//
// The networks are the skill planner's (skill_f32.hip) with a third row in the actor's mu_ / std_, on the same building
// blocks and workgroup layout (hier_enc.hpp: 192 threads = hidden features, EB = 4 envs per workgroup; skill_net.hpp).
// What differs is the control flow of a step (options/scripts/evaluate_hier.py:63-75):
//  * k_option_low -- LoPolicyValueModel with the termination epilogue: after the two action components the same thread
//    forms the third one, prob = sigmoid(4 a_2 - 3), the termination draw and the ended flag.
//  * k_option_high -- HighPolicyValueModel for the envs that pick: a scattered few per cent on every step.  Either
//    workgroup b looks at envs 4 b .. 4 b + 3 and leaves when none picks (a workgroup that stays pays for four), or
//    k_option_list first compacts the picking envs into a list (wave ballot, one atomic per wave) and workgroup b takes
//    entries 4 b .. 4 b + 3 of it.  An env's result does not depend on its workgroup neighbours, so the order of the
//    list changes no value.
// Inside zenv_collect_option both kernels also record frame t (OptionRecord; option_collect.hip has the rest).
#include <hip/hip_runtime.h>

#include "option_f32.hpp"
#include "skill_net.hpp"

namespace zenvk {
namespace {

using namespace hf32;

__device__ __forceinline__ bool option_picks(const DevParams &p, const SkillState &st, int env)
{
    return !p.sched[env].done_state && (st.skill[env] < 0 || st.ended[env] != 0);
}

__global__ __launch_bounds__(256) void k_option_list(DevParams p, SkillState st, OptionList ol)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    const bool pick = env < p.N && option_picks(p, st, env);
    const unsigned long long vote = __ballot(pick);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && vote) base = atomicAdd(ol.count, __popcll(vote));
    base = __shfl(base, 0);
    const int at = base + __popcll(vote & ((1ull << lane) - 1ull));
    if (pick && at < p.N) ol.list[at] = env;
}

// out0 = log-softmax logits [N][S], out1 = value [N] (+ the skill pick)
__global__ __launch_bounds__(HP) void k_option_high(SkillF32 w, DevParams p, SkillState st, OptionList ol,
                                                    float *__restrict__ out0, float *__restrict__ out1, OptionPick pick,
                                                    OptionRecord rec)
{
    __shared__ __align__(16) float x0[ZF * RP];         // zone rows of the pass       [k][row]
    __shared__ __align__(16) float y1[HP * RP];         // activations of the pass     [k][row]
    __shared__ float xin[EB * XP];                      // per-env input: obs
    __shared__ float peb[EB * HP];
    __shared__ float va[EB * HP];
    __shared__ float vb[EB * HP];
    __shared__ float lg[EB * SR];
    __shared__ int on[EB];
    __shared__ int envs[EB];                            // the workgroup's envs
    const int j = threadIdx.x;
    const int h = w.h, S = w.S;
    const int slot0 = blockIdx.x * EB;
    const int n_all = pick.compact ? min(*ol.count, p.N) : p.N;
    if (slot0 >= n_all) return;
    const int n_env = min(EB, n_all - slot0);

    if (j < EB) {
        int a = 0, env = 0;
        if (j < n_env) {
            env = pick.compact ? ol.list[slot0 + j] : slot0 + j;
            a = pick.mode < 0 || pick.compact || option_picks(p, st, env);
        }
        on[j] = a;
        envs[j] = env;
    }
    __syncthreads();
    if (!(on[0] | on[1] | on[2] | on[3])) return;
    if (j < EB * XP) {
        const int e = j / XP, k = j % XP;
        xin[j] = e < n_env && k < 8 ? p.obs[(size_t)envs[e] * 8 + k] : 0.f;
    }
    __syncthreads();
    encode_envs<8>(w.hi, p, xin, nullptr, nullptr, nullptr, 0, n_env, h, j, x0, y1, peb, va, vb, envs);
    skill_hidden<0>(w, w.hi_critic, nullptr, h, j, va, vb, peb);
    skill_logit_rows(w, w.hi_critic, h, j, va, peb, lg);
    if (j < n_env && on[j]) {
        const int env = envs[j];
        const float *L = lg + j * SR;
        out1[env] = L[kMaxSkills];
        const Categorical cat = categorical(L, S, out0 + (size_t)env * S);
        if (pick.mode < 0) return;
        int g = cat.best;
        if (pick.mode == 1)                              // the stream of ZENV_POLICY_SKILL_SAMPLE
            g = categorical_draw(L, S, cat,
                                 philox_uniform(pick.seed, pick.env_index0 + (uint64_t)env, pick.step_index, 0x534B4Cu));
        st.skill[env] = g;
        st.age[env] = 0;
        if (!rec.pick_skill) return;
        const size_t slot = (size_t)rec.t * rec.N + env;   // the pick opens a high-level transition (:36-40)
        rec.pick_skill[slot] = g;
        rec.pick_value[slot] = L[kMaxSkills];
        rec.pick_log_prob[slot] = (L[g] - cat.m) - cat.lse;
        rec.open[env] = 1;
    }
}

// out0 = mu [N][2], out1 = std [N][2], out2 = value [N], term (+ the action, the ended flag, the age)
__global__ __launch_bounds__(HP) void k_option_low(SkillF32 w, DevParams p, SkillState st, OptionList ol,
                                                   float *__restrict__ out0, float *__restrict__ out1,
                                                   float *__restrict__ out2, OptionTerm term, MlpAction act,
                                                   OptionRecord rec)
{
    __shared__ __align__(16) float x0[ZF * RP];
    __shared__ __align__(16) float y1[HP * RP];
    __shared__ float xin[EB * XP];
    __shared__ float peb[EB * HP];
    __shared__ float va[EB * HP];
    __shared__ float vb[EB * HP];
    __shared__ float lg[EB * 8];                        // per env: mu_ rows 0-2, std_ rows 3-5, the critic (row 6)
    __shared__ int sel[EB];                             // the env's skill column (-1: the env idles)
    const int j = threadIdx.x;
    const int h = w.h;
    const int env0 = blockIdx.x * EB;
    const int n_env = min(EB, p.N - env0);
    const bool acts = act.mode >= 0;
    if (acts && blockIdx.x == 0 && j == 0) *ol.count = 0;    // this call's list is used up

    if (j < EB) {
        int s = -1;
        if (j < n_env && !(acts && p.sched[env0 + j].done_state)) s = st.skill[env0 + j];
        sel[j] = s;
    }
    __syncthreads();
    const bool any = (sel[0] & sel[1] & sel[2] & sel[3]) >= 0;      // some env acts: the AND of values >= -1 is -1 only when all are
    if (any) {
        if (j < EB * XP) {
            const int e = j / XP, k = j % XP;
            xin[j] = e < n_env && k < 8 ? p.obs[(size_t)(env0 + e) * 8 + k] : 0.f;
        }
        __syncthreads();
        encode_envs<8>(w.lo, p, xin, w.lo_w1s, w.lo_wcs, sel, env0, n_env, h, j, x0, y1, peb, va, vb);
        skill_hidden<1>(w, w.lo_critic, sel, h, j, va, vb, peb);
        if (j < EB * 8) {
            const int e = j >> 3, row = j & 7;
            float s = 0.f;
            if (row < 6) s = dot_row(w.heads + (size_t)row * (HP + 1), va + e * HP, h);
            else if (row == 6 && w.lo_critic) s = dot_row(w.lv2, peb + e * HP, h);
            lg[j] = s;
        }
        __syncthreads();
    }
    if (j >= n_env) return;
    const int env = env0 + j;
    const size_t slot = (size_t)rec.t * rec.N + env;
    if (sel[j] < 0) {
        idle_outputs(env, out0, out1, out2, act);
        term.mu[env] = term.stdv[env] = term.action[env] = term.prob[env] = 0.f;
        if (acts) st.ended[env] = 0;
        if (acts && rec.lo_skill) {
            rec.lo_skill[slot] = -1;
            rec.term_action[slot] = rec.term_log_prob[slot] = 0.f;
            rec.ended[slot] = 0;
        }
        return;
    }
    const float *o = lg + 8 * j;
    out2[env] = o[6];
    head_outputs(env, o[0], o[1], o[3], o[4], o[6], out0, out1, act);
    // ---- the third component: its sample decides whether the option ends (evaluate_hier.py:68, :73)
    const float m2 = 2.0f * (sigmoidf_(o[2]) - 0.5f), sd2 = sigmoidf_(o[5]) + 1e-3f;
    const uint64_t g = act.env_index0 + (uint64_t)env;
    float a2 = m2;
    if (act.mode == 1) {
        // words 2 and 3 of the action draw's Philox block (mlp_action took 0 and 1)
        const PhiloxWords c = philox_words(act.seed, g, act.step_index, 0x4D4C50u);
        const float u1 = u01(c.w[2]), u2 = u01(c.w[3]);
        a2 = m2 + sd2 * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
    }
    const float prob = sigmoidf_(4.0f * a2 - 3.0f);
    term.mu[env] = m2;
    term.stdv[env] = sd2;
    term.action[env] = a2;
    term.prob[env] = prob;
    if (!acts) return;
    const bool ended = act.mode == 1 ? philox_uniform(act.seed, g, act.step_index, kOptionTermTag) < prob : prob > 0.5f;
    st.ended[env] = ended;
    st.age[env] += 1;
    if (!rec.lo_skill) return;
    rec.lo_skill[slot] = sel[j];
    rec.term_action[slot] = a2;
    const float z2 = (a2 - m2) / sd2;                    // Normal(mu_2, std_2).log_prob(a_2), as head_outputs forms the other two
    rec.term_log_prob[slot] = -0.5f * z2 * z2 - logf(sd2) - 0.91893853320467274178f;
    rec.ended[slot] = ended;
}

}  // namespace

hipError_t launch_option_list(const DevParams &p, const SkillState &st, const OptionList &ol, hipStream_t s)
{
    hipLaunchKernelGGL(k_option_list, dim3((p.N + 255) / 256), dim3(256), 0, s, p, st, ol);
    return hipGetLastError();
}

hipError_t launch_option_high(const SkillF32 &w, const DevParams &p, const SkillState &st, const OptionList &ol,
                              float *logits, float *value, const OptionPick &pick, hipStream_t s, const OptionRecord &rec)
{
    hipLaunchKernelGGL(k_option_high, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, st, ol, logits, value, pick, rec);
    return hipGetLastError();
}

hipError_t launch_option_low(const SkillF32 &w, const DevParams &p, const SkillState &st, const OptionList &ol,
                             float *mu, float *stdv, float *value, const OptionTerm &term, const MlpAction &act,
                             hipStream_t s, const OptionRecord &rec)
{
    hipLaunchKernelGGL(k_option_low, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, st, ol, mu, stdv, value, term, act,
                       rec);
    return hipGetLastError();
}

}  // namespace zenvk
