// skill_f32.hip -- the fixed-length-skills agent (main/src/hier_policy_value_models.py:19-76) in float32, gfx950.
//
// Two launches of one kernel template on the vector ALU, with the building blocks and the workgroup layout of
// hier_f32.hip (hier_enc.hpp: 192 threads = hidden features, EB = 4 envs per workgroup):
//  * k_skill_f32<0> -- HighPolicyValueModel.  emb = ZoneEnvModel(obs, zone_obs) (the flat agent's encoder); logits =
//    actor.discrete_.0(relu(actor.enc_.0.0(emb))), one length-h dot product per (env, skill) thread; Categorical(logits=
//    log_softmax(x)); value = critic.2(relu(critic.0(emb))).  When it picks, a workgroup none of whose envs needs a
//    skill leaves at once: the high level costs what the envs that pick cost (one in skill_len steps).
//  * k_skill_f32<1> -- LoPolicyValueModel.  The one-hot skill of ZoneEnvSkillModel's [obs, onehot] and of the heads'
//    [emb, onehot] input selects one weight column: a per-env bias in zone_net_.0, combine_net_, actor.enc_.0.0 and
//    critic.0, so the per-zone part has the flat network's shape.  Then PolicyNetwork's mu_ / std_ and the Normal sample
//    of mlp_head_out.hpp, and the skill's age.
// Only the summation order differs from torch's: within 1e-5 of the reference's float32 modules.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>

#include "f32_packer.hpp"
#include "skill_net.hpp"

namespace zenvk {
namespace {

using namespace hf32;

// one uniform in (0, 1) of the skill draw: Philox4x32-10 keyed by (seed, global env, step), a stream of its own (the
// action draw of mlp_head_out.hpp uses the tag 0x4D4C50, the Zone-goals goal draw 0x48474C).  zenv_collect_skill's
// randint(0, S) draws on the tag 0x534B55 and its bootstrap skill s' on 0x534B42.
__device__ __forceinline__ float skill_uniform(const SkillPick &pick, int env)
{
    const uint32_t tag = pick.mode == 2 ? 0x534B55u : pick.mode == 3 ? 0x534B42u : 0x534B4Cu;
    return philox_uniform(pick.seed, pick.env_index0 + (uint64_t)env, pick.step_index, tag);
}

// an env without a skill: idle_outputs, and inside zenv_collect_skill skill -1 for frame t
__device__ __forceinline__ void skill_idle(int env, float *__restrict__ mu, float *__restrict__ stdv,
                                           float *__restrict__ value, const MlpAction &act, const SkillRecord &sr)
{
    idle_outputs(env, mu, stdv, value, act);
    if (act.mode >= 0 && sr.lo_skill) sr.lo_skill[(size_t)sr.t * sr.N + env] = -1;
}

// LEVEL 0: HighPolicyValueModel -> out0 = log-softmax logits [N][S], out1 = value [N] (+ the skill pick)
// LEVEL 1: LoPolicyValueModel   -> out0 = mu [N][2], out1 = std [N][2], out2 = value [N] (+ the action, the age)
template <int LEVEL>
__global__ __launch_bounds__(HP) void k_skill_f32(SkillF32 w, DevParams p, SkillState st, float *__restrict__ out0,
                                                  float *__restrict__ out1, float *__restrict__ out2, SkillPick pick,
                                                  MlpAction act)
{
    __shared__ __align__(16) float x0[ZF * RP];         // zone rows of the pass       [k][row]
    __shared__ __align__(16) float y1[HP * RP];         // activations of the pass     [k][row]
    __shared__ float xin[EB * XP];                      // per-env input: obs
    __shared__ float peb[EB * HP];
    __shared__ float va[EB * HP];
    __shared__ float vb[EB * HP];
    __shared__ float lg[EB * SR];
    __shared__ int on[EB];
    __shared__ int sel[EB];                             // the low level's skill column (-1: none)
    const int j = threadIdx.x;
    const int h = w.h, S = w.S;
    const int env0 = blockIdx.x * EB;
    const int n_env = min(EB, p.N - env0);
    const bool has_critic = LEVEL ? w.lo_critic : w.hi_critic;

    // ---- which envs are evaluated: high -- all (forward) or those that pick a skill; low -- those with a skill
    if (j < EB) {
        int a = 0, s = -1;
        if (j < n_env) {
            const int env = env0 + j;
            if (LEVEL == 0) {
                const int sk = st.skill[env];
                a = pick.mode < 0 || pick.mode == 3 || pick.every ||
                    ((sk < 0 || st.age[env] >= pick.skill_len) && !p.sched[env].done_state);
            } else {
                s = st.skill[env];
                a = s >= 0;
            }
        }
        on[j] = a;
        sel[j] = s;
    }
    __syncthreads();
    if (!(on[0] | on[1] | on[2] | on[3])) {
        if (LEVEL == 1 && j < n_env) skill_idle(env0 + j, out0, out1, out2, act, pick.rec);
        return;
    }
    if (j < EB * XP) {
        const int e = j / XP, k = j % XP;
        xin[j] = e < n_env && k < 8 ? p.obs[(size_t)(env0 + e) * 8 + k] : 0.f;
    }
    if (LEVEL == 0 && pick.rec.hi_obs) {
        // zenv_collect_skill: the obs and zone_obs every picking env picks on, into its row env * W + k
        const SkillRecord &sr = pick.rec;
        const int ZFn = p.Z * p.F;
        for (int i = j; i < EB * (8 + ZFn); i += HP) {
            const int e = i / (8 + ZFn), k = i - e * (8 + ZFn);
            if (e >= n_env || !on[e]) continue;
            const size_t env = (size_t)(env0 + e), row = env * sr.W + sr.k;
            if (k < 8) sr.hi_obs[row * 8 + k] = p.obs[env * 8 + k];
            else sr.hi_zone_obs[row * ZFn + (k - 8)] = p.zone_obs[env * ZFn + (k - 8)];
        }
    }
    __syncthreads();
    if (LEVEL == 0)
        encode_envs<8>(w.hi, p, xin, nullptr, nullptr, nullptr, env0, n_env, h, j, x0, y1, peb, va, vb);
    else
        encode_envs<8>(w.lo, p, xin, w.lo_w1s, w.lo_wcs, sel, env0, n_env, h, j, x0, y1, peb, va, vb);

    // ---- vb = emb: a = relu(actor.enc_.0.0(.)) -> va, relu(critic.0(.)) -> peb (the low level adds the skill column)
    skill_hidden<LEVEL>(w, has_critic, sel, h, j, va, vb, peb);

    if (LEVEL == 0) {
        skill_logit_rows(w, has_critic, h, j, va, peb, lg);
        if (j < n_env && on[j]) {
            const int env = env0 + j;
            const float *L = lg + j * SR;
            out1[env] = L[kMaxSkills];
            const Categorical cat = categorical(L, S, out0 + (size_t)env * S);
            if (pick.mode >= 0) {
                int g = cat.best;
                if (pick.mode == 1 || pick.mode == 3) {
                    g = categorical_draw(L, S, cat, skill_uniform(pick, env));
                } else if (pick.mode == 2) {              // randint(0, S); the top uniform is exactly 1.0
                    g = min((int)(skill_uniform(pick, env) * (float)S), S - 1);
                }
                if (pick.mode == 3) {
                    pick.boot[env] = g;
                } else {
                    st.skill[env] = g;
                    st.age[env] = 0;
                }
                const SkillRecord &sr = pick.rec;
                if (sr.hi_skill) {                        // zenv_collect_skill: the pick's row
                    const size_t row = (size_t)env * sr.W + sr.k;
                    sr.hi_skill[row] = g;
                    sr.hi_value[row] = L[kMaxSkills];
                    sr.hi_log_prob[row] = (L[g] - cat.m) - cat.lse;
                }
            }
        }
        return;
    }

    // ---- low level: mu_, std_ on va, critic.2 on peb
    if (j < EB * 8) {
        const int e = j >> 3, row = j & 7;
        float s = 0.f;
        if (row < 4) s = dot_row(w.heads + (size_t)row * (HP + 1), va + e * HP, h);
        else if (row == 4 && has_critic) s = dot_row(w.lv2, peb + e * HP, h);
        lg[j] = s;
    }
    __syncthreads();
    if (j < n_env) {
        const int env = env0 + j;
        if (on[j]) {
            const float *o = lg + 8 * j;
            out2[env] = o[4];
            head_outputs(env, o[0], o[1], o[2], o[3], o[4], out0, out1, act);
            if (act.mode >= 0 && !p.sched[env].done_state) st.age[env] += 1;
            if (act.mode >= 0 && pick.rec.lo_skill) pick.rec.lo_skill[(size_t)pick.rec.t * pick.rec.N + env] = sel[j];
        } else {
            skill_idle(env, out0, out1, out2, act, pick.rec);
        }
    }
}

__global__ __launch_bounds__(256) void k_skill_sync(DevParams p, SkillState st, const uint8_t *__restrict__ mask,
                                                    int force)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.N) return;
    const int32_t k = p.sched[env].episode_idx;
    if (st.epi[env] != k || (force && (!mask || mask[env]))) {
        st.skill[env] = -1;
        st.age[env] = 0;
        st.ended[env] = 0;
        st.epi[env] = k;
    }
}

__global__ __launch_bounds__(256) void k_skill_set(DevParams p, SkillState st)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.N) return;
    const int32_t s = st.in[env];
    if (s < 0) return;
    st.skill[env] = s;
    st.age[env] = 0;
    st.ended[env] = 0;
}

}  // namespace

size_t pack_skill_f32(const zenv_skill_weights &w, int F, std::vector<float> &out, size_t offs[kSkillPtrs], int n_out)
{
    const int h = w.h_dim, S = w.n_skills;
    Packer pk(out, h);
    int i = 0;
    pk.enc(offs, i, w.hi_zone_w1, w.hi_zone_b1, w.hi_zone_w2, w.hi_zone_b2, w.hi_zone_w3, w.hi_zone_b3, w.hi_comb_w,
           w.hi_comb_b, F, 8, 0);
    pk.enc(offs, i, w.lo_zone_w1, w.lo_zone_b1, w.lo_zone_w2, w.lo_zone_b2, w.lo_zone_w3, w.lo_zone_b3, w.lo_comb_w,
           w.lo_comb_b, F, 8, S);
    offs[i++] = pk.cols(w.lo_zone_w1, 8 + S + F, 8, S, S);  // the skill columns
    offs[i++] = pk.cols(w.lo_comb_w, 8 + S + h, 8, S, S);
    offs[i++] = pk.cols(w.hi_enc_w, h, 0, h, HP);
    offs[i++] = pk.bias(w.hi_enc_b);
    offs[i++] = pk.rows(w.hi_logit_w, w.hi_logit_b, S);
    const bool hc = w.hi_critic_w1 != nullptr, lc = w.lo_critic_w1 != nullptr;
    offs[i++] = hc ? pk.cols(w.hi_critic_w1, h, 0, h, HP) : 0;
    offs[i++] = hc ? pk.bias(w.hi_critic_b1) : 0;
    offs[i++] = hc ? pk.rows(w.hi_critic_w2, w.hi_critic_b2, 1) : 0;
    offs[i++] = pk.cols(w.lo_enc_w, h + S, 0, h, HP);
    offs[i++] = pk.cols(w.lo_enc_w, h + S, h, S, S);
    offs[i++] = pk.bias(w.lo_enc_b);
    offs[i++] = pk.head_rows(w.lo_mu_w, w.lo_mu_b, w.lo_std_w, w.lo_std_b, n_out);
    offs[i++] = lc ? pk.cols(w.lo_critic_w1, h + S, 0, h, HP) : 0;
    offs[i++] = lc ? pk.cols(w.lo_critic_w1, h + S, h, S, S) : 0;
    offs[i++] = lc ? pk.bias(w.lo_critic_b1) : 0;
    offs[i++] = lc ? pk.rows(w.lo_critic_w2, w.lo_critic_b2, 1) : 0;
    return out.size();
}

size_t pack_skill_inverse_f32(const zenv_skill_inverse_weights &w, int F, std::vector<float> &out,
                              size_t offs[kSkillInvPtrs])
{
    Packer pk(out, w.h_dim);
    int i = 0;
    pk.enc(offs, i, w.zone_w1, w.zone_b1, w.zone_w2, w.zone_b2, w.zone_w3, w.zone_b3, w.comb_w1, w.comb_b1, F, 8, 0);
    offs[i++] = pk.rows(w.comb_w2, w.comb_b2, w.n_skills);
    return out.size();
}

SkillInvF32 skill_inverse_f32_at(const zenv_skill_inverse_weights &w, const float *base,
                                 const size_t offs[kSkillInvPtrs])
{
    SkillInvF32 s{};
    s.h = w.h_dim;
    s.S = w.n_skills;
    static_assert(offsetof(SkillInvF32, head) == offsetof(SkillInvF32, enc) + sizeof(HierEnc), "SkillInvF32 layout");
    bind_pointers(s, offsetof(SkillInvF32, enc), base, offs, kSkillInvPtrs);
    return s;
}

SkillF32 skill_f32_at(const zenv_skill_weights &w, const float *base, const size_t offs[kSkillPtrs])
{
    SkillF32 s{};
    s.h = w.h_dim;
    s.S = w.n_skills;
    s.hi_critic = w.hi_critic_w1 ? 1 : 0;
    s.lo_critic = w.lo_critic_w1 ? 1 : 0;
    bind_pointers(s, offsetof(SkillF32, hi), base, offs, kSkillPtrs);
    return s;
}

hipError_t launch_skill_high(const SkillF32 &w, const DevParams &p, const SkillState &st, float *logits, float *value,
                             const SkillPick &pick, hipStream_t s)
{
    hipLaunchKernelGGL(k_skill_f32<0>, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, st, logits, value, nullptr, pick,
                       no_mlp_action());
    return hipGetLastError();
}

hipError_t launch_skill_low(const SkillF32 &w, const DevParams &p, const SkillState &st, float *mu, float *stdv,
                            float *value, const MlpAction &act, hipStream_t s, const SkillRecord *rec)
{
    SkillPick none{ -1, 0, 0u, 0ull, 0ull, 0, nullptr, SkillRecord{} };
    if (rec) none.rec = *rec;
    hipLaunchKernelGGL(k_skill_f32<1>, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, st, mu, stdv, value, none, act);
    return hipGetLastError();
}

hipError_t launch_skill_sync(const DevParams &p, const SkillState &st, const uint8_t *mask, int force, hipStream_t s)
{
    hipLaunchKernelGGL(k_skill_sync, dim3((p.N + 255) / 256), dim3(256), 0, s, p, st, mask, force);
    return hipGetLastError();
}

hipError_t launch_skill_set(const DevParams &p, const SkillState &st, hipStream_t s)
{
    hipLaunchKernelGGL(k_skill_set, dim3((p.N + 255) / 256), dim3(256), 0, s, p, st);
    return hipGetLastError();
}

}  // namespace zenvk
