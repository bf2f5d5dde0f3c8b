// skill_net.hpp -- what the kernels of the skill family share after the encoder (skill_f32.hip: fixed-length skills,
// option_f32.hip: variable-length Options): the hidden layers of actor and critic on the embedding, the dot-product rows
// of the heads, Categorical(logits=log_softmax(x)) with its inverse-CDF draw.
#pragma once
#include <hip/hip_runtime.h>

#include "hier_enc.hpp"
#include "mlp_head_out.hpp"
#include "skill_f32.hpp"

namespace zenvk {
namespace hf32 {

constexpr int SR = kMaxSkills + 1;    // per env: S logit rows, then the critic (row kMaxSkills)

// sum_k w[k] x[k] + w[HP] over the h features (a row of the [.][HP + 1] layout)
__device__ __forceinline__ float dot_row(const float *__restrict__ w, const float *__restrict__ x, int h)
{
    float s = w[HP];
    for (int k = 0; k < h; ++k) s = __builtin_fmaf(w[k], x[k], s);
    return s;
}

// vb = emb (encode_envs ended with a barrier: nobody reads va / peb any more): relu(actor.enc_.0.0(.)) -> va,
// relu(critic.0(.)) -> peb (0 without a critic); the low level (LEVEL 1) adds the skill column sel[e] of both.  Ends
// with a barrier.
template <int LEVEL>
__device__ __forceinline__ void skill_hidden(const SkillF32 &w, bool has_critic, const int *sel, int h, int j,
                                             float *__restrict__ va, float *__restrict__ vb, float *__restrict__ peb)
{
    const bool live = j < h;
    float t[EB], hv[EB];
#pragma unroll
    for (int e = 0; e < EB; ++e) hv[e] = 0.f;
    if (has_critic) {
        matvec(hv, LEVEL ? w.lv1t : w.hv1t, LEVEL ? w.lv1b : w.hv1b, vb, HP, h, j);
        if (LEVEL == 1) add_column(hv, w.lv1s, sel, j);
    }
    matvec(t, LEVEL ? w.encw : w.hencw, LEVEL ? w.encb : w.hencb, vb, HP, h, j);
    if (LEVEL == 1) add_column(t, w.encs, sel, j);
#pragma unroll
    for (int e = 0; e < EB; ++e) {
        va[e * HP + j] = live ? fmaxf(t[e], 0.f) : 0.f;
        peb[e * HP + j] = live ? fmaxf(hv[e], 0.f) : 0.f;
    }
    __syncthreads();
}

// the high level's rows of the workgroup, one thread per (env, row): the S logits on va, then the critic on peb -> lg
// [EB][SR]; ends with a barrier
__device__ __forceinline__ void skill_logit_rows(const SkillF32 &w, bool has_critic, int h, int j,
                                                 const float *__restrict__ va, const float *__restrict__ peb,
                                                 float *__restrict__ lg)
{
    if (j < EB * SR) {
        const int e = j / SR, r = j - e * SR;
        float s = 0.f;
        if (r < w.S) s = dot_row(w.hdisc + (size_t)r * (HP + 1), va + e * HP, h);
        else if (r == kMaxSkills && has_critic) s = dot_row(w.hv2, peb + e * HP, h);
        lg[j] = s;
    }
    __syncthreads();
}

// Categorical(logits=log_softmax(x)) of one env: x - max - log(sum exp(x - max)) into out[S]
struct Categorical {
    float m, sum, lse;
    int best;                                         // the argmax; ties go to the lowest index
};
__device__ __forceinline__ Categorical categorical(const float *__restrict__ L, int S, float *__restrict__ out)
{
    Categorical c;
    c.m = L[0];
    c.best = 0;
    for (int s = 1; s < S; ++s)
        if (L[s] > c.m) {                             // strict: ties go to the lowest skill
            c.m = L[s];
            c.best = s;
        }
    c.sum = 0.f;
    for (int s = 0; s < S; ++s) c.sum += expf(L[s] - c.m);
    c.lse = logf(c.sum);
    for (int s = 0; s < S; ++s) out[s] = (L[s] - c.m) - c.lse;
    return c;
}
// inverse CDF of softmax(x) on one uniform u, in index order
__device__ __forceinline__ int categorical_draw(const float *__restrict__ L, int S, const Categorical &c, float u)
{
    const float thr = u * c.sum;
    float acc = 0.f;
    int g = c.best;
    for (int s = 0; s < S; ++s) {
        acc += expf(L[s] - c.m);
        g = s;                                        // the last index takes what rounding leaves over
        if (acc > thr) break;
    }
    return g;
}

}  // namespace hf32
}  // namespace zenvk
