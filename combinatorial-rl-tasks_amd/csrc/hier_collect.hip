// hier_collect.hip -- the bookkeeping of zenv_collect_hier: collect_experiences of the Zone-goals agent
// (zone-goals/src/torch_ac/algos/_hier_policy_opt.py:9-171) besides its two networks, gfx950.
//
// The high level's transitions are semi-Markov: an env opens one when it picks a goal (k_hier_f32<0> records the pick
// at frame t) and closes it when the env asks for the next goal (k_hier_close, after the step of the frame that
// reached the goal or ended the episode).  Their number per env varies, so nothing is laid out during the frames: the
// picks and closes sit in time-major [T][N] records (whole lines per frame), the observations stay where the step
// kernel wrote them (the EXP_OBS slots of zenv_collect) and a transition refers to them by slot.  After the frames:
//   k_hier_count_scan  exclusive prefix sum of the per-env close counts -> row offsets and M (one workgroup, 16-byte
//                      coalesced tiles)
//   k_hier_gae         per env, backward over the frames: the high-level GAE (no discount, lambda only, as the
//                      reference) and the small fields of the env's rows; the new carry
//   k_hier_gather      the rows' obs / zone_obs / action mask, env-major [M, ...]: one contiguous dword stream per field
//                      (a Z*F row, 150 floats at Z = 25, is not a whole number of 16-byte pieces)
//   k_hier_carry       the carry slot of every env whose open transition began in this call: its observation, which
//                      the next call's rows read (the exp slots are overwritten by then)
// All of them are bandwidth-bound and small next to the low-level network.
#include <hip/hip_runtime.h>

#include "hier_f32.hpp"

namespace zenvk {
namespace {

__global__ __launch_bounds__(256) void k_hier_close(DevParams p, HierFrames f, HierCarry c, int t)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= p.N) return;
    const size_t slot = (size_t)t * p.N + env;
    const float r = p.reward[env];
    f.env_reward[slot] = r;
    float hr = c.hi_reward[env] + r;                           // self.hi_reward += self.rewards[i] (float32)
    if (p.need_goal[env]) {                                    // info['need_next_goal']
        if (c.open[env]) {
            f.close_reward[slot] = hr;
            f.close_flag[slot] = p.done_out[env] ? 2 : 1;       // self.hi_mask[j] = 0 if done[j] else 1
            f.count[env] += 1;
            c.open[env] = 0;
        }
        hr = 0.f;
    }
    c.hi_reward[env] = hr;
}

constexpr int SCAN_T = 1024;
constexpr int SCAN_W = SCAN_T / 64;    // waves

// exclusive prefix sum of count[N] -> offset[N], total.  Tiles of 4 * SCAN_T counts: thread i reads the 16 bytes at
// 4 i (consecutive lanes, consecutive addresses), scans them, then a wave scan (DPP shuffles) and a scan of the wave
// sums; a running carry joins the tiles.
__global__ __launch_bounds__(SCAN_T) void k_hier_count_scan(HierFrames f, int N)
{
    __shared__ int wsum[SCAN_W];
    __shared__ int tile_total;
    const int i = threadIdx.x, lane = i & 63, w = i >> 6;
    int carry = 0;
    for (int base = 0; base < N; base += 4 * SCAN_T) {
        const int at = base + 4 * i;
        int v[4] = { 0, 0, 0, 0 };
        if (at + 3 < N) {                                     // count / offset are 256-byte aligned, `at` a multiple of 4
            const int4 q = *reinterpret_cast<const int4 *>(f.count + at);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int k = 0; k < 4; ++k)
                if (at + k < N) v[k] = f.count[at + k];
        }
        const int s = v[0] + v[1] + v[2] + v[3];
        int x = s;                                            // inclusive scan over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        if (w == 0) {                                         // inclusive scan of the wave sums
            int y = lane < SCAN_W ? wsum[lane] : 0;
            for (int d = 1; d < SCAN_W; d <<= 1) {
                const int z = __shfl_up(y, d, 64);
                if (lane >= d) y += z;
            }
            if (lane < SCAN_W) wsum[lane] = y;
            if (lane == SCAN_W - 1) tile_total = y;
        }
        __syncthreads();
        int e = carry + (w ? wsum[w - 1] : 0) + x - s;        // exclusive prefix of this thread's first count
        int o[4];
        for (int k = 0; k < 4; ++k) {
            o[k] = e;
            e += v[k];
        }
        if (at + 3 < N) {
            *reinterpret_cast<int4 *>(f.offset + at) = make_int4(o[0], o[1], o[2], o[3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (at + k < N) f.offset[at + k] = o[k];
        }
        carry += tile_total;
        __syncthreads();                                      // wsum / tile_total are rewritten by the next tile
    }
    if (i == 0) *f.total = carry;
}

// zenv_reset: the open transition of a reset env belongs to the episode that ended -- it is dropped, and hi_reward
// restarts at 0 (the new episode's first pick opens the next transition)
__global__ __launch_bounds__(256) void k_hier_reset(HierCarry c, const uint8_t *__restrict__ mask, int N)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N || (mask && !mask[env])) return;
    c.open[env] = 0;
    c.hi_reward[env] = 0.f;
}

// _hier_policy_opt.py:99-107 for one env: for its closed transitions k in reverse order
//   delta = r_k + V_next * m_k - V_k,  adv_k = delta + lambda * adv_next * m_k
// V_next: the value of the env's next transition (the one still open, if a goal was picked after the last close), else
// V_hi(obs_T); adv_next = 0 for the last one.  m_k is the hi_mask recorded when k closed.  Rows offset .. offset+count-1.
__global__ __launch_bounds__(256) void k_hier_gae(HierFrames f, HierCarry c, HierOut o, int N,
                                                  const float *__restrict__ v_final, float lambda)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    const int base = f.offset[env];
    int idx = f.count[env];
    float vn = v_final[env], an = 0.f, pr = 0.f, pm = 0.f;
    bool pending = false, seen = false;
    int64_t carry_src = -1;                                    // the new carry, written once the old one is consumed
    int c_goal = 0;
    uint32_t c_avail = 0;
    float c_value = 0.f, c_log_prob = 0.f;
    for (int t = f.T - 1; t >= 0; --t) {
        const size_t slot = (size_t)t * N + env;               // time-major: the threads of a wave read one line
        const uint8_t fl = f.close_flag[slot];
        if (fl) {
            pending = true;
            pr = f.close_reward[slot];
            pm = fl == 1 ? 1.f : 0.f;
        }
        const int g = f.pick_goal[slot];
        if (g < 0) continue;
        const float v = f.pick_value[slot];
        if (pending) {
            if (idx > 0) {
                const float adv = pr + vn * pm - v + lambda * an * pm;
                const int row = base + --idx;
                o.action[row] = g;
                o.avail[row] = f.pick_avail[slot];
                o.value[row] = v;
                o.log_prob[row] = f.pick_log_prob[slot];
                o.advantage[row] = adv;
                o.returnn[row] = v + adv;
                o.reward[row] = pr;
                o.mask[row] = pm;
                o.src[row] = (int64_t)slot;
                an = adv;
            }
            pending = false;
        } else if (!seen) {                                    // picked, not closed yet: the next call's carry
            carry_src = (int64_t)slot;
            c_goal = g;
            c_avail = f.pick_avail[slot];
            c_value = v;
            c_log_prob = f.pick_log_prob[slot];
        }
        vn = v;
        seen = true;
    }
    if (pending && idx > 0) {                                  // the transition an earlier call left open
        const float v = c.value[env];
        const float adv = pr + vn * pm - v + lambda * an * pm;
        const int row = base + --idx;
        o.action[row] = c.goal[env];
        o.avail[row] = c.avail[env];
        o.value[row] = v;
        o.log_prob[row] = c.log_prob[env];
        o.advantage[row] = adv;
        o.returnn[row] = v + adv;
        o.reward[row] = pr;
        o.mask[row] = pm;
        o.src[row] = -1 - (int64_t)env;
    }
    if (carry_src >= 0) {
        c.goal[env] = c_goal;
        c.avail[env] = c_avail;
        c.value[env] = c_value;
        c.log_prob[env] = c_log_prob;
    }
    c.src[env] = carry_src;
}

constexpr int RB = 32;   // rows per workgroup of the copies

// rows m0 .. m0 + RB - 1: dst[m][k] = (source row of m)[k], k < W -- consecutive threads, consecutive addresses
__device__ __forceinline__ void copy_rows(float *__restrict__ dst, const int64_t *src_row, const float *__restrict__ exp,
                                          const float *__restrict__ carry, int64_t m0, int n_rows, int W)
{
    for (int i = (int)threadIdx.x; i < n_rows * W; i += (int)blockDim.x) {
        const int r = i / W, k = i - r * W;
        const int64_t s = src_row[r];
        if (s == INT64_MIN) continue;
        const float *from = s >= 0 ? exp + (size_t)s * W : carry + (size_t)(-1 - s) * W;
        dst[(size_t)(m0 + r) * W + k] = from[k];
    }
}

__global__ __launch_bounds__(256) void k_hier_gather(HierOut o, HierCarry c, const float *__restrict__ exp_obs,
                                                     const float *__restrict__ exp_zone_obs, int64_t M, int Z, int ZF)
{
    __shared__ int64_t src[RB];
    __shared__ uint32_t av[RB];
    const int64_t m0 = (int64_t)blockIdx.x * RB;
    const int n_rows = (int)min((int64_t)RB, M - m0);
    if ((int)threadIdx.x < n_rows) {
        src[threadIdx.x] = o.src[m0 + threadIdx.x];
        av[threadIdx.x] = o.avail[m0 + threadIdx.x];
    }
    __syncthreads();
    copy_rows(o.obs, src, exp_obs, c.obs, m0, n_rows, 8);
    copy_rows(o.zone_obs, src, exp_zone_obs, c.zone_obs, m0, n_rows, ZF);
    if (!o.action_mask) return;                                              // zenv_collect_option: skills have no mask
    for (int i = (int)threadIdx.x; i < n_rows * Z; i += (int)blockDim.x) {   // hi_action_masks: available_goals as bool [Z]
        const int r = i / Z, z = i - r * Z;
        o.action_mask[(size_t)(m0 + r) * Z + z] = (uint8_t)((av[r] >> z) & 1u);
    }
}

__global__ __launch_bounds__(256) void k_hier_carry(HierCarry c, const float *__restrict__ exp_obs,
                                                    const float *__restrict__ exp_zone_obs, int N, int ZF)
{
    __shared__ int64_t src[RB];
    const int64_t e0 = (int64_t)blockIdx.x * RB;
    const int n_rows = (int)min((int64_t)RB, (int64_t)N - e0);
    if ((int)threadIdx.x < n_rows) {
        const int64_t s = c.src[e0 + threadIdx.x];
        src[threadIdx.x] = s >= 0 ? s : INT64_MIN;             // INT64_MIN: keep this env's carry
    }
    __syncthreads();
    copy_rows(c.obs, src, exp_obs, nullptr, e0, n_rows, 8);
    copy_rows(c.zone_obs, src, exp_zone_obs, nullptr, e0, n_rows, ZF);
}

}  // namespace

hipError_t launch_hier_close(const DevParams &p, const HierFrames &f, const HierCarry &c, int t, hipStream_t s)
{
    hipLaunchKernelGGL(k_hier_close, dim3((p.N + 255) / 256), dim3(256), 0, s, p, f, c, t);
    return hipGetLastError();
}

hipError_t launch_hier_count_scan(const HierFrames &f, int N, hipStream_t s)
{
    hipLaunchKernelGGL(k_hier_count_scan, dim3(1), dim3(SCAN_T), 0, s, f, N);
    return hipGetLastError();
}

hipError_t launch_hier_reset(const HierCarry &c, const uint8_t *mask, int N, hipStream_t s)
{
    hipLaunchKernelGGL(k_hier_reset, dim3((N + 255) / 256), dim3(256), 0, s, c, mask, N);
    return hipGetLastError();
}

hipError_t launch_hier_gae(const HierFrames &f, const HierCarry &c, const HierOut &o, int N, const float *v_final,
                           float gae_lambda, hipStream_t s)
{
    hipLaunchKernelGGL(k_hier_gae, dim3((N + 255) / 256), dim3(256), 0, s, f, c, o, N, v_final, gae_lambda);
    return hipGetLastError();
}

hipError_t launch_hier_gather(const HierOut &o, const HierCarry &c, const float *exp_obs, const float *exp_zone_obs,
                              int64_t M, int N, int Z, int F, hipStream_t s)
{
    (void)N;
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_hier_gather, dim3((unsigned)((M + RB - 1) / RB)), dim3(256), 0, s, o, c, exp_obs, exp_zone_obs,
                       M, Z, Z * F);
    return hipGetLastError();
}

hipError_t launch_hier_carry(const HierCarry &c, const float *exp_obs, const float *exp_zone_obs, int N, int ZF,
                             hipStream_t s)
{
    hipLaunchKernelGGL(k_hier_carry, dim3((N + RB - 1) / RB), dim3(256), 0, s, c, exp_obs, exp_zone_obs, N, ZF);
    return hipGetLastError();
}

}  // namespace zenvk
