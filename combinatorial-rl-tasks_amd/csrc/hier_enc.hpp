// hier_enc.hpp -- the float32 vector-ALU building blocks of the hierarchical agents' networks (hier_f32.hip: Zone-goals,
// skill_f32.hip: fixed-length skills), in the layout of mlp_f32.hip's k_mlp_f32: a workgroup of kMlpHP = 192 threads owns
// EB = 4 consecutive envs, thread j owns hidden feature j, input rows sit in LDS ([k][row]: the same address in every
// lane = a broadcast), the weights are read transposed ([k][j]) from L2.
#pragma once
#include <hip/hip_runtime.h>

#include "hier_f32.hpp"

namespace zenvk {
namespace hf32 {

constexpr int HP = kMlpHP;     // 192 threads = hidden features (padded)
constexpr int RP = 32;         // rows (zone rows of consecutive envs) per pass
constexpr int EB = 4;          // envs per workgroup
constexpr int XP = 12;         // per-env input [obs (8), goal (2)], padded
constexpr int ZF = 8;          // zone row (F <= 7), padded
constexpr int NQ = HP / RP;    // 6 partial sums per logit

// acc[r] += w * x[k][r] for the RP rows of one pass
__device__ __forceinline__ void fma_rows(float (&acc)[RP], float w, const float *__restrict__ xk)
{
    const float4 *x4 = reinterpret_cast<const float4 *>(xk);
#pragma unroll
    for (int q = 0; q < RP / 4; ++q) {
        const float4 v = x4[q];
        acc[4 * q + 0] = __builtin_fmaf(w, v.x, acc[4 * q + 0]);
        acc[4 * q + 1] = __builtin_fmaf(w, v.y, acc[4 * q + 1]);
        acc[4 * q + 2] = __builtin_fmaf(w, v.z, acc[4 * q + 2]);
        acc[4 * q + 3] = __builtin_fmaf(w, v.w, acc[4 * q + 3]);
    }
}

// out[e] (+)= sum_k wt[k][j] * x[e][k] for the EB env vectors in LDS (x: [EB][stride]); b: bias, or null = accumulate
__device__ __forceinline__ void matvec(float (&out)[EB], const float *__restrict__ wt, const float *__restrict__ b,
                                       const float *__restrict__ x, int stride, int n_in, int j)
{
    if (b) {
#pragma unroll
        for (int e = 0; e < EB; ++e) out[e] = b[j];
    }
    for (int k = 0; k < n_in; ++k) {
        const float w = wt[(size_t)k * HP + j];
#pragma unroll
        for (int e = 0; e < EB; ++e) out[e] = __builtin_fmaf(w, x[e * stride + k], out[e]);
    }
}

// zone rows r0 .. r0 + RP - 1 of the workgroup's envs (row = e * Z + z) -> x0 [ZF][RP], zeros beyond; the envs are
// env0 + e, or envs[e] where a list is given
__device__ __forceinline__ void load_rows(float *__restrict__ x0, const float *__restrict__ zone_obs, int env0, int r0,
                                          int n_rows, int Z, int F, int j, const int *envs = nullptr)
{
    for (int i = j; i < ZF * RP; i += HP) {
        const int k = i / RP, r = i % RP, row = r0 + r;
        float v = 0.f;
        if (row < n_rows && k < F) {
            const int e = row / Z, z = row - e * Z;
            v = zone_obs[((size_t)(envs ? envs[e] : env0 + e) * Z + z) * F + k];
        }
        x0[k * RP + r] = v;
    }
}

// acc[r] = bias[e(row)][j] + sum_k wz[k][j] row[k]
__device__ __forceinline__ void zone_part(float (&acc)[RP], const float *__restrict__ peb, const float *__restrict__ wz,
                                          const float *__restrict__ x0, int r0, int Z, int F, int j)
{
#pragma unroll
    for (int r = 0; r < RP; ++r) {
        const int e = min((r0 + r) / Z, EB - 1);
        acc[r] = peb[e * HP + j];
    }
    for (int k = 0; k < F; ++k) fma_rows(acc, wz[(size_t)k * HP + j], x0 + k * RP);
}

__device__ __forceinline__ void store_rows(float *__restrict__ y, const float (&acc)[RP], float scale, bool live, int j)
{
#pragma unroll
    for (int q = 0; q < RP / 4; ++q)
        reinterpret_cast<float4 *>(y + j * RP)[q] =
            live ? make_float4(scale * fmaxf(acc[4 * q], 0.f), scale * fmaxf(acc[4 * q + 1], 0.f),
                               scale * fmaxf(acc[4 * q + 2], 0.f), scale * fmaxf(acc[4 * q + 3], 0.f))
                 : make_float4(0.f, 0.f, 0.f, 0.f);
}

// t[e] += col[sel[e]][j]: a one-hot input of env e is one selected column of the weight (transposed: [n][HP]);
// sel[e] < 0 adds nothing
__device__ __forceinline__ void add_column(float (&t)[EB], const float *__restrict__ col, const int *sel, int j)
{
#pragma unroll
    for (int e = 0; e < EB; ++e)
        if (sel[e] >= 0) t[e] += col[(size_t)sel[e] * HP + j];
}

// ZoneEnvModel / ZoneEnvGoalModel / ZoneEnvSkillModel on the workgroup's envs env0 .. env0 + n_env - 1, or the n_env envs
// envs[0 ..] (LDS) where a list is given -- xin, sel and the outputs stay per workgroup slot e either way: the per-env input
// x (XIN columns of xin [EB][XP], LDS) is the same for every zone row of an env, so W_x x + b of zone_net_.0 is a per-env
// bias (peb) and the per-zone part has the flat network's shape, F columns.  A one-hot input (the skill) enters the same
// way, as the column sel[e] of col1 (zone_net_.0) and colc (combine_net_); col1 = colc = null: none.
// -> emb in vb [EB][HP] (0 in the padded features), followed by a barrier.  x0, y1, peb, va: the caller's LDS scratch.
template <int XIN>
__device__ __forceinline__ void encode_envs(const HierEnc &E, const DevParams &p, const float *__restrict__ xin,
                                            const float *__restrict__ col1, const float *__restrict__ colc,
                                            const int *sel, int env0, int n_env, int h, int j, float *__restrict__ x0,
                                            float *__restrict__ y1, float *__restrict__ peb, float *__restrict__ va,
                                            float *__restrict__ vb, const int *envs = nullptr)
{
    const int Z = p.Z, F = p.F;
    const bool live = j < h;                             // padded features stay exactly 0
    float t[EB];
    matvec(t, E.w1x, E.b1, xin, XP, XIN, j);            // zone_net_.0 on [obs(, goal)] + bias: the same for every row
    if (col1) add_column(t, col1, sel, j);               // ... + the one-hot's column
#pragma unroll
    for (int e = 0; e < EB; ++e) peb[e * HP + j] = t[e];

    // ---- zone_net_.0 (zone-row columns), ReLU, zone_net_.2, ReLU on every row; rows summed per env
    const int n_rows = n_env * Z;
    float psum[EB];
#pragma unroll
    for (int e = 0; e < EB; ++e) psum[e] = 0.f;
    const float b2 = E.b2[j];
    for (int r0 = 0; r0 < n_rows; r0 += RP) {
        __syncthreads();                                  // the previous pass is done with x0 / y1 (and peb is written)
        load_rows(x0, p.zone_obs, env0, r0, n_rows, Z, F, j, envs);
        __syncthreads();
        float acc[RP];
        zone_part(acc, peb, E.w1z, x0, r0, Z, F, j);
        store_rows(y1, acc, 1.f, live, j);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RP; ++r) acc[r] = b2;
        for (int k = 0; k < h; ++k) fma_rows(acc, E.w2t[(size_t)k * HP + j], y1 + k * RP);
#pragma unroll
        for (int r = 0; r < RP; ++r) {
            const int row = r0 + r;
            const int e = row / Z;
            const float v = fmaxf(acc[r], 0.f);
#pragma unroll
            for (int ee = 0; ee < EB; ++ee)
                if (row < n_rows && e == ee) psum[ee] += v;
        }
    }

    // ---- per env: zone_emb = zone_net_.4(mean); emb = combine_net_([obs(, goal), zone_emb])
    __syncthreads();
    const float inv_z = 1.0f / (float)Z;
#pragma unroll
    for (int e = 0; e < EB; ++e) vb[e * HP + j] = live ? psum[e] * inv_z : 0.f;
    __syncthreads();
    matvec(t, E.w3t, E.b3, vb, HP, h, j);
#pragma unroll
    for (int e = 0; e < EB; ++e) va[e * HP + j] = live ? t[e] : 0.f;
    __syncthreads();
    matvec(t, E.wce, E.bc, va, HP, h, j);
    matvec(t, E.wcx, nullptr, xin, XP, XIN, j);
    if (colc) add_column(t, colc, sel, j);
#pragma unroll
    for (int e = 0; e < EB; ++e) vb[e * HP + j] = live ? t[e] : 0.f;        // emb
    __syncthreads();
}

}  // namespace hf32
}  // namespace zenvk
