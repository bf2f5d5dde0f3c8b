// hier_f32.hip -- the Zone-goals hierarchical agent (zone-goals/src/hier_policy_value_models.py:19-86) in float32, gfx950.
//
// Two launches of one kernel template, both on the vector ALU in the layout of mlp_f32.hip's k_mlp_f32: a workgroup of
// kMlpHP = 192 threads owns EB = 4 consecutive envs, thread j owns hidden feature j, input rows sit in LDS ([k][row]: the
// same address in every lane = a broadcast), the weights are read transposed ([k][j]) from L2.
//
//  * k_hier_f32<0> -- HighPolicyValueModel.  emb = ZoneEnvModel(obs, zone_obs); actor.0 = [W_e | W_z] on [emb, zone row]
//    splits into W_e emb + b (once per env) + W_z row_z (Z times, F columns), so every logit costs h * F FMAs plus a
//    length-h dot product with actor.2 (a 6-way split reduction over LDS).  The same kernel masks the unavailable zones
//    and picks the goal (argmax, or the inverse CDF of softmax(masked logits) on one Philox uniform) into the buffer
//    launch_goal_set reads.  When it picks, a workgroup none of whose envs needs a goal writes -1 and leaves: the high
//    level costs what the envs that pick cost (goals change every few hundred steps).
//  * k_hier_f32<1> -- LoPolicyValueModel.  ZoneEnvGoalModel's [obs, goal] is the same for every zone row of an env:
//    W_x [obs, goal] + b folds into a per-env bias of zone_net_.0 (and the [obs, goal] columns of combine_net_ into a
//    per-env term), so the per-zone part has the flat network's shape, F columns.  Then PolicyNetwork's enc_ / mu_ /
//    std_ and the Normal sample of mlp_head_out.hpp.
// Only the summation order differs from torch's (and the mean over the zone rows is taken before zone_net_'s third,
// activation-free layer, with which it commutes): within 1e-5 of the reference's float32 modules.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "f32_packer.hpp"
#include "hier_enc.hpp"
#include "hier_f32.hpp"
#include "mlp_head_out.hpp"

namespace zenvk {
namespace {

using namespace hf32;

// zenv_collect_hier: the low level's goal input of frame t, cur_goal of _hier_policy_opt.py -- the last goal's centre / 3
// (goal_xy survives the goal's clearing and the auto-reset), 0 before the first goal
__device__ __forceinline__ void lo_record_goal(const DevParams &p, const HierRecord &rec, int env)
{
    if (!rec.lo_goal) return;
    const double2 zz = p.goal_xy[env];
    reinterpret_cast<float2 *>(rec.lo_goal)[(size_t)rec.t * rec.N + env] =
        make_float2((float)(zz.x / 3.0), (float)(zz.y / 3.0));
}

// the goal draw's Philox stream (the action draw of mlp_head_out.hpp uses the tag 0x4D4C50)
constexpr uint32_t kGoalTag = 0x48474Cu;

// LEVEL 0: HighPolicyValueModel -> out0 = logits [N][Z], out1 = value [N] (+ the goal pick)
// LEVEL 1: LoPolicyValueModel   -> out0 = mu [N][2], out1 = std [N][2], out2 = value [N] (+ the action)
template <int LEVEL>
__global__ __launch_bounds__(HP) void k_hier_f32(HierF32 w, DevParams p, float *__restrict__ out0, float *__restrict__ out1,
                                                 float *__restrict__ out2, HierPick pick, MlpAction act, HierRecord rec)
{
    constexpr int XIN = LEVEL ? 10 : 8;                 // [obs] or [obs, goal]
    __shared__ __align__(16) float x0[ZF * RP];         // zone rows of the pass       [k][row]
    __shared__ __align__(16) float y1[HP * RP];         // activations of the pass     [k][row]
    __shared__ float xin[EB * XP];                      // per-env input
    __shared__ float peb[EB * HP];                      // per-env bias of the zone-row layer
    __shared__ float va[EB * HP];
    __shared__ float vb[EB * HP];
    __shared__ float red[NQ * RP];
    __shared__ float lg[EB * ZENV_MAX_ZONES];
    __shared__ float hd[EB * 8];
    __shared__ int on[EB];
    const int j = threadIdx.x;
    const int h = w.h, Z = p.Z, F = p.F;
    const bool live = j < h;                             // padded features stay exactly 0
    const int env0 = blockIdx.x * EB;
    const int n_env = min(EB, p.N - env0);
    const HierEnc &E = LEVEL ? w.lo : w.hi;
    const bool has_critic = LEVEL ? w.lo_critic : w.hi_critic;

    // ---- which envs are evaluated: high -- all (forward) or those that pick a goal; low -- those with a goal
    if (j < EB) {
        int a = 0;
        if (j < n_env) {
            const int env = env0 + j;
            if (LEVEL == 0) a = pick.mode < 0 || (p.need_goal[env] && !p.sched[env].done_state);
            else a = p.goal[env] >= 0;
        }
        on[j] = a;
    }
    __syncthreads();
    if (!(on[0] | on[1] | on[2] | on[3])) {
        if (j < n_env) {
            if (LEVEL == 0) {
                if (pick.mode >= 0) pick.new_goal[env0 + j] = -1;
            } else {
                idle_outputs(env0 + j, out0, out1, out2, act);
                lo_record_goal(p, rec, env0 + j);
            }
        }
        return;
    }
    if (j < EB * XP) {
        const int e = j / XP, k = j % XP;
        float v = 0.f;
        if (e < n_env) {
            const int env = env0 + e;
            if (k < 8) {
                v = p.obs[(size_t)env * 8 + k];
            } else if (LEVEL == 1 && k < 10 && p.goal[env] >= 0) {
                // get_goal(): the goal zone's centre / 3 in float64, then float32 (TSP_next_city_env.py:86-88)
                const double2 zz = p.goal_xy[env];
                v = (float)((k == 8 ? zz.x : zz.y) / 3.0);
            }
        }
        xin[j] = v;
    }
    __syncthreads();
    encode_envs<XIN>(E, p, xin, nullptr, nullptr, nullptr, env0, n_env, h, j, x0, y1, peb, va, vb);
    const int n_rows = n_env * Z;
    float t[EB];
    float hv[EB];                                                           // critic.0(emb)
#pragma unroll
    for (int e = 0; e < EB; ++e) hv[e] = 0.f;
    if (has_critic) matvec(hv, LEVEL ? w.lv1t : w.hv1t, LEVEL ? w.lv1b : w.hv1b, vb, HP, h, j);

    if (LEVEL == 0 && pick.mode == -2) {                  // the critic only: value = critic.2(relu(critic.0(emb)))
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EB; ++e) va[e * HP + j] = live ? fmaxf(hv[e], 0.f) : 0.f;
        __syncthreads();
        if (j < n_env) {
            float s = 0.f;
            if (has_critic) {
                s = w.hv2[HP];
                for (int k = 0; k < h; ++k) s = __builtin_fmaf(w.hv2[k], va[j * HP + k], s);
            }
            out1[env0 + j] = s;
        }
        return;
    }
    if (LEVEL == 0) {
        // ---- actor.0 = W_e emb + b (per env) + W_z zone row (per zone); logit = actor.2(relu(.))
        matvec(t, w.hae, w.hab, vb, HP, h, j);
        __syncthreads();                                  // every thread is past its zone_part reads of peb
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            peb[e * HP + j] = live ? t[e] : 0.f;
            va[e * HP + j] = live ? fmaxf(hv[e], 0.f) : 0.f;
        }
        const float a2 = live ? w.ha2[j] : 0.f;
        for (int r0 = 0; r0 < n_rows; r0 += RP) {
            __syncthreads();
            load_rows(x0, p.zone_obs, env0, r0, n_rows, Z, F, j);
            __syncthreads();
            float acc[RP];
            zone_part(acc, peb, w.haz, x0, r0, Z, F, j);
            store_rows(y1, acc, a2, live, j);            // actor.2's products, summed over the features next
            __syncthreads();
            {
                const int r = j % RP, q = j / RP;
                float s = 0.f;
                for (int k = q * RP; k < q * RP + RP; ++k) s += y1[k * RP + r];
                red[q * RP + r] = s;
            }
            __syncthreads();
            if (j < RP && r0 + j < n_rows) {
                float s = red[j];
#pragma unroll
                for (int q = 1; q < NQ; ++q) s += red[q * RP + j];
                const int row = r0 + j, e = row / Z;
                lg[e * ZENV_MAX_ZONES + (row - e * Z)] = s + w.ha2[HP];
            }
        }
        __syncthreads();
        if (j < n_env && on[j]) {
            const int env = env0 + j;
            if (has_critic) {                             // critic.2(relu(critic.0(emb)))
                float s = w.hv2[HP];
                for (int k = 0; k < h; ++k) s = __builtin_fmaf(w.hv2[k], va[j * HP + k], s);
                out1[env] = s;
            } else {
                out1[env] = 0.f;
            }
            // get_hi_action: logits[~available_goals] = -inf, then Categorical(logits)
            const uint32_t avail = p.available[env];
            const float *L = lg + j * ZENV_MAX_ZONES;
            float m = -INFINITY;
            int best = -1;
            for (int z = 0; z < Z; ++z) {
                const float l = ((avail >> z) & 1u) ? L[z] : -INFINITY;
                out0[(size_t)env * Z + z] = l;
                if (l > m) {                              // strict: ties go to the lowest zone
                    m = l;
                    best = z;
                }
            }
            if (pick.mode >= 0) {
                int g = best;                             // -1: no available zone, the env gets no goal
                float s = 0.f;                            // sum of exp(l - max) over the available zones
                if (best >= 0 && (pick.mode == 1 || rec.goal)) {
                    for (int z = 0; z < Z; ++z)
                        if ((avail >> z) & 1u) s += expf(L[z] - m);
                }
                if (pick.mode == 1 && best >= 0) {
                    // inverse CDF of softmax over the available zones, in zone order
                    const float u = philox_uniform(pick.seed, pick.env_index0 + (uint64_t)env, pick.step_index, kGoalTag);
                    const float thr = u * s;
                    float c = 0.f;
                    for (int z = 0; z < Z; ++z) {
                        if (!((avail >> z) & 1u)) continue;
                        c += expf(L[z] - m);
                        g = z;                            // the last available zone takes what rounding leaves over
                        if (c > thr) break;
                    }
                }
                pick.new_goal[env] = g;
                if (rec.goal && g >= 0) {
                    // zenv_collect_hier: a high-level transition opens -- Categorical(masked logits).log_prob(goal) is
                    // the log-softmax over the available zones
                    const size_t slot = (size_t)rec.t * rec.N + env;
                    rec.goal[slot] = g;
                    rec.value[slot] = out1[env];
                    rec.log_prob[slot] = (L[g] - m) - logf(s);
                    rec.avail[slot] = avail;
                    rec.open[env] = 1;
                }
            }
        } else if (j < n_env && pick.mode >= 0) {
            pick.new_goal[env0 + j] = -1;
        }
        return;
    }

    // ---- low level: a = relu(actor.enc_(emb)); mu_, std_ on a; critic.2 on relu(critic.0(emb))
    matvec(t, w.encw, w.encb, vb, HP, h, j);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EB; ++e) {
        va[e * HP + j] = live ? fmaxf(t[e], 0.f) : 0.f;
        peb[e * HP + j] = live ? fmaxf(hv[e], 0.f) : 0.f;
    }
    __syncthreads();
    if (j < EB * 8) {
        const int e = j >> 3, row = j & 7;
        float s = 0.f;
        if (row < 4 || (row == 4 && has_critic)) {
            const float *wr = row < 4 ? w.heads + (size_t)row * (HP + 1) : w.lv2;
            const float *x = row < 4 ? va + e * HP : peb + e * HP;
            s = wr[HP];
            for (int k = 0; k < h; ++k) s = __builtin_fmaf(wr[k], x[k], s);
        }
        hd[j] = s;
    }
    __syncthreads();
    if (j < n_env) {
        const int env = env0 + j;
        if (on[j]) {
            const float *o = hd + 8 * j;
            out2[env] = o[4];
            head_outputs(env, o[0], o[1], o[2], o[3], o[4], out0, out1, act);
        } else {
            idle_outputs(env, out0, out1, out2, act);
        }
        lo_record_goal(p, rec, env);
    }
}

}  // namespace

size_t pack_hier_f32(const zenv_hier_weights &w, int F, std::vector<float> &out, size_t offs[kHierOffs])
{
    const int h = w.h_dim;
    Packer pk(out, h);
    int i = 0;
    pk.enc(offs, i, w.hi_zone_w1, w.hi_zone_b1, w.hi_zone_w2, w.hi_zone_b2, w.hi_zone_w3, w.hi_zone_b3, w.hi_comb_w,
           w.hi_comb_b, F, 8, 0);
    pk.enc(offs, i, w.lo_zone_w1, w.lo_zone_b1, w.lo_zone_w2, w.lo_zone_b2, w.lo_zone_w3, w.lo_zone_b3, w.lo_comb_w,
           w.lo_comb_b, F, 10, 0);
    offs[i++] = pk.cols(w.hi_actor_w1, h + F, 0, h, HP);    // actor.0: emb columns
    offs[i++] = pk.cols(w.hi_actor_w1, h + F, h, F, ZF);    //          zone-row columns
    offs[i++] = pk.bias(w.hi_actor_b1);
    offs[i++] = pk.rows(w.hi_actor_w2, w.hi_actor_b2, 1);
    const bool hc = w.hi_critic_w1 != nullptr, lc = w.lo_critic_w1 != nullptr;
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

HierF32 hier_f32_at(const zenv_hier_weights &w, const float *base, const size_t offs[kHierOffs])
{
    HierF32 s{};
    s.h = w.h_dim;
    s.hi_critic = w.hi_critic_w1 ? 1 : 0;
    s.lo_critic = w.lo_critic_w1 ? 1 : 0;
    bind_pointers(s, offsetof(HierF32, hi), base, offs, kHierOffs);
    return s;
}

hipError_t launch_hier_high(const HierF32 &w, const DevParams &p, float *logits, float *value, const HierPick &pick,
                            hipStream_t s, const HierRecord &rec)
{
    hipLaunchKernelGGL(k_hier_f32<0>, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, logits, value, nullptr, pick,
                       no_mlp_action(), rec);
    return hipGetLastError();
}

hipError_t launch_hier_low(const HierF32 &w, const DevParams &p, float *mu, float *stdv, float *value,
                           const MlpAction &act, hipStream_t s, const HierRecord &rec)
{
    const HierPick none{ -1, 0u, 0ull, 0ull, nullptr };
    hipLaunchKernelGGL(k_hier_f32<1>, dim3((p.N + EB - 1) / EB), dim3(HP), 0, s, w, p, mu, stdv, value, none, act, rec);
    return hipGetLastError();
}

}  // namespace zenvk
