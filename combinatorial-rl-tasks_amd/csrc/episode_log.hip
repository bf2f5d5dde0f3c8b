// episode_log.hip -- the reference's per-episode training logs from the collectors' records, gfx950.
//
// collect_experiences keeps four running float32 sums per env, appends an entry to its lists whenever an env's episode
// ends (main/src/torch_ac/algos/base.py:167-182; the skills / xy-goals loops only while the env is still active in its
// window, main/src/torch_ac/algos/_hier_policy_opt.py:105-128) and multiplies the sums by the new mask.  The entries are
// appended frame by frame and env-ascending inside a frame.  Here:
//
//  * k_eplog_walk<false> -- one thread per env walks its T frames (the [T][N] reads are coalesced across the wave);
//    a ballot per frame gives the wave's number of entries, one count per (frame, wave), frame-major.
//  * k_eplog_scan_block / _add -- the exclusive scan of those counts, kEpLogScan counts per workgroup, the block sums
//    scanned by the same kernels one level up: the position of every (frame, wave)'s first entry, and D.
//  * k_eplog_walk<true>  -- the same walk with the sums: an env that appends writes its entry at its wave's position plus
//    its rank in the ballot, and the carry is advanced.  No staging area, no atomic: every position is computed.
//  * k_eplog_copy -- the old tail's share of the result, and the new tail out of the result.
//  * k_eplog_stat -- sum / min / max of a column in float64: a fixed tree, 4 values per thread pairwise, 256 threads
//    through LDS, the workgroups' partial results by the same kernel one level up; then the squares about the mean.
#include <hip/hip_runtime.h>

#include <cmath>

#include "episode_log.hpp"

namespace zenvk {
namespace {

__device__ __forceinline__ int lanes_below(unsigned long long bits)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bits >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bits, 0u));
}

template <bool kScatter>
__global__ __launch_bounds__(256) void k_eplog_walk(EpLogWalk k, int32_t *__restrict__ counts,
                                                    int32_t *__restrict__ active, EpLogList out, int64_t base)
{
    const int env = blockIdx.x * 256 + threadIdx.x;       // a wave = 64 consecutive envs; no lane leaves before the end
    const bool in = env < k.N;
    const int W = (k.N + 63) >> 6, w = env >> 6;
    const bool lead = (threadIdx.x & 63) == 0 && w < W;
    float r = 0.f, s = 0.f, f = 0.f, d = 0.f;
    if (kScatter && in) r = k.carry[0][env], s = k.carry[1][env], f = k.carry[2][env], d = k.carry[3][env];
    bool act = true;
    for (int t = 0; t < k.T; ++t) {
        if (k.L > 0 && t % k.L == 0) act = true;          // proc_active = [True] * num_procs (:29-31)
        const size_t at = (size_t)t * k.N + env;
        float m = 1.f;
        if (in) m = t + 1 < k.T ? k.mask[at + k.N] : k.cur_mask[env];
        if (kScatter && in) {
            r = __fadd_rn(r, k.ret[at]);
            s = __fadd_rn(s, k.resh[at]);
            f = __fadd_rn(f, 1.f);
            if (k.div) d = __fadd_rn(d, k.div[at]);
        }
        const bool done = in && (1.f - m) != 0.f;
        const bool ev = done && act;                      // `if done_` (base.py:174), `and self.proc_active[i]` (:115)
        const unsigned long long bits = __ballot(ev);
        if (!kScatter) {
            const unsigned long long on = __ballot(in && act);       // frame_counter += sum(proc_active) (:112)
            if (lead) {
                counts[(size_t)t * W + w] = __popcll(bits);
                if (active) active[(size_t)t * W + w] = __popcll(on);
            }
        } else if (ev) {
            const int64_t pos = base + counts[(size_t)t * W + w] + lanes_below(bits);
            out.col[0][pos] = r;
            out.col[1][pos] = s;
            out.col[2][pos] = f;
            out.col[3][pos] = d;
            out.col[4][pos] = 0.f;                        // log_episode_prediction is never added to
            out.env[pos] = env;
        }
        if (done && k.L > 0) act = false;                 // until the next window; without windows every done counts
        if (kScatter) r = __fmul_rn(r, m), s = __fmul_rn(s, m), f = __fmul_rn(f, m), d = __fmul_rn(d, m);
    }
    if (kScatter && in) k.carry[0][env] = r, k.carry[1][env] = s, k.carry[2][env] = f, k.carry[3][env] = d;
}

// a[b * 256 .. b * 256 + 255] becomes its own exclusive scan, sums[b] the block's total
__global__ __launch_bounds__(kEpLogScan) void k_eplog_scan_block(int32_t *__restrict__ a, int64_t n,
                                                                 int32_t *__restrict__ sums)
{
    __shared__ int sh[2 * kEpLogScan];
    const int j = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kEpLogScan + j;
    const int c = i < n ? a[i] : 0;
    int *src = sh, *dst = sh + kEpLogScan;
    src[j] = c;
    __syncthreads();
    for (int step = 1; step < kEpLogScan; step <<= 1) {
        dst[j] = src[j] + (j >= step ? src[j - step] : 0);
        __syncthreads();
        int *x = src;
        src = dst;
        dst = x;
    }
    if (i < n) a[i] = src[j] - c;
    if (j == kEpLogScan - 1) sums[blockIdx.x] = src[j];
}

__global__ __launch_bounds__(kEpLogScan) void k_eplog_scan_add(int32_t *__restrict__ a, int64_t n,
                                                               const int32_t *__restrict__ sums)
{
    const int64_t i = (int64_t)blockIdx.x * kEpLogScan + threadIdx.x;
    if (i < n) a[i] += sums[blockIdx.x];
}

__global__ __launch_bounds__(256) void k_eplog_copy(EpLogList dst, int64_t dst0, EpLogList src, int64_t src0, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < kEpLogCols; ++c) dst.col[c][dst0 + i] = src.col[c][src0 + i];
    dst.env[dst0 + i] = src.env[src0 + i];
}

// One level of the tree over n values: x (float32, the first level; `about` non-null: the square of x - about[0] /
// n_all) or the partial results (ps, pmn, pmx) of the level below.  Workgroup b writes os[b], omn[b], omx[b].
__global__ __launch_bounds__(256) void k_eplog_stat(const float *__restrict__ x, const double *__restrict__ ps,
                                                    const double *__restrict__ pmn, const double *__restrict__ pmx,
                                                    int64_t n, const double *__restrict__ about, int64_t n_all,
                                                    double *__restrict__ os, double *__restrict__ omn,
                                                    double *__restrict__ omx)
{
    __shared__ double sh_s[256], sh_mn[256], sh_mx[256];
    const int j = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * kEpLogStat + 4 * (int64_t)j;
    const double mean = about ? about[0] / (double)n_all : 0.0;
    double v[4], mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = first + q;
        v[q] = 0.0;
        if (i < n) {
            double lo, hi;
            if (x) {
                double u = (double)x[i];
                if (about) u = (u - mean) * (u - mean);
                v[q] = lo = hi = u;
            } else {
                v[q] = ps[i], lo = pmn[i], hi = pmx[i];
            }
            mn = fmin(mn, lo);
            mx = fmax(mx, hi);
        }
    }
    sh_s[j] = (v[0] + v[1]) + (v[2] + v[3]);
    sh_mn[j] = mn;
    sh_mx[j] = mx;
    __syncthreads();
    for (int step = 1; step < 256; step <<= 1) {          // neighbours first: the tree of a pairwise sum
        if ((j & (2 * step - 1)) == 0) {
            sh_s[j] += sh_s[j + step];
            sh_mn[j] = fmin(sh_mn[j], sh_mn[j + step]);
            sh_mx[j] = fmax(sh_mx[j], sh_mx[j + step]);
        }
        __syncthreads();
    }
    if (j == 0) os[blockIdx.x] = sh_s[0], omn[blockIdx.x] = sh_mn[0], omx[blockIdx.x] = sh_mx[0];
}

inline int64_t blocks_of(int64_t n, int per) { return (n + per - 1) / per; }

}  // namespace

hipError_t launch_eplog_count(const EpLogWalk &k, int32_t *counts, int32_t *active, hipStream_t s)
{
    hipLaunchKernelGGL(k_eplog_walk<false>, dim3((k.N + 255) / 256), dim3(256), 0, s, k, counts, active, EpLogList{}, 0);
    return hipGetLastError();
}

int64_t eplog_scan_levels(int64_t n)
{
    int64_t total = 0;
    do {
        n = blocks_of(n, kEpLogScan);
        total += n;
    } while (n > 1);
    return total;
}

hipError_t launch_eplog_scan(int32_t *a, int64_t n, int32_t *levels, int32_t *total, hipStream_t s)
{
    const int64_t nb = blocks_of(n, kEpLogScan);
    if (nb == 1) {
        hipLaunchKernelGGL(k_eplog_scan_block, dim3(1), dim3(kEpLogScan), 0, s, a, n, total);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_eplog_scan_block, dim3((unsigned)nb), dim3(kEpLogScan), 0, s, a, n, levels);
    if (hipError_t e = launch_eplog_scan(levels, nb, levels + nb, total, s)) return e;
    hipLaunchKernelGGL(k_eplog_scan_add, dim3((unsigned)nb), dim3(kEpLogScan), 0, s, a, n, levels);
    return hipGetLastError();
}

hipError_t launch_eplog_scatter(const EpLogWalk &k, const int32_t *offsets, const EpLogList &out, int64_t base,
                                hipStream_t s)
{
    hipLaunchKernelGGL(k_eplog_walk<true>, dim3((k.N + 255) / 256), dim3(256), 0, s, k, const_cast<int32_t *>(offsets),
                       nullptr, out, base);
    return hipGetLastError();
}

hipError_t launch_eplog_copy(const EpLogList &dst, int64_t dst0, const EpLogList &src, int64_t src0, int64_t n,
                             hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_eplog_copy, dim3((unsigned)blocks_of(n, 256)), dim3(256), 0, s, dst, dst0, src, src0, n);
    return hipGetLastError();
}

int64_t eplog_stat_ws(int64_t n)
{
    int64_t total = 0;
    do {
        n = blocks_of(n, kEpLogStat);
        total += 3 * n;
    } while (n > 1);
    return total;
}

hipError_t launch_eplog_stats(const float *x, int64_t n, double *ws, double *fin, hipStream_t s)
{
    for (int pass = 0; pass < 2; ++pass) {
        const float *x32 = x;
        const double *ps = nullptr, *pmn = nullptr, *pmx = nullptr;
        double *at = ws;
        for (int64_t m = n;;) {
            const int64_t nb = blocks_of(m, kEpLogStat);
            double *o = nb == 1 ? fin + 3 * pass : at;
            hipLaunchKernelGGL(k_eplog_stat, dim3((unsigned)nb), dim3(256), 0, s, x32, ps, pmn, pmx, m,
                               x32 && pass ? fin : nullptr, n, o, o + nb, o + 2 * nb);
            if (hipError_t e = hipGetLastError()) return e;
            if (nb == 1) break;
            x32 = nullptr, ps = o, pmn = o + nb, pmx = o + 2 * nb;
            at += 3 * nb;
            m = nb;
        }
    }
    return hipSuccess;
}

}  // namespace zenvk
