// episode_log.hpp -- the `logs` of the reference's collect_experiences as a post-pass over the collectors' records
// (episode_log.hip): the five trees' logging loops (main/src/torch_ac/algos/base.py:167-182, 233-247;
// main/src/torch_ac/algos/_hier_policy_opt.py:105-128, 216-232 and the other trees' _hier_policy_opt.py at the same
// place).  Internal: not installed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace zenvk {

constexpr int kEpLogCols = 5;          // return, reshaped return, num_frames, diversity, prediction
constexpr int kEpLogScan = 256;        // counts one workgroup of the scan takes
constexpr int kEpLogStat = 1024;       // values one workgroup of the reduction takes

// One collection's records, time-major, and the state the reference carries from call to call.
struct EpLogWalk {
    int T, N;
    int L;                          // window length of the skills / xy-goals collectors, 0: no windows (always active)
    const float *ret;               // [T][N] the env reward
    const float *resh;              // [T][N] what the reshaped return sums
    const float *div;               // [T][N] the unscaled diversity reward, or null (the column stays 0)
    const float *mask;              // [T][N] self.masks: done_t = 1 - mask[t + 1]
    const float *cur_mask;          // [N]    self.mask after the call: done_{T-1} = 1 - cur_mask
    float *carry[4];                // [N] each: log_episode_return, _reshaped_return, _num_frames, _diversity
};

// A list of entries: the columns and the env that produced each entry.
struct EpLogList {
    float *col[kEpLogCols];
    int32_t *env;
};

// counts[t * W + w] = entries that wave w (envs 64 w .. 64 w + 63) appends in frame t, W = ceil(N / 64);
// active[t * W + w] = its envs that are active in frame t (L > 0 only).  The carry is read, not written.
hipError_t launch_eplog_count(const EpLogWalk &k, int32_t *counts, int32_t *active, hipStream_t s);
// In place: a[i] becomes the sum of a[0 .. i - 1], *total the sum of all n.  `levels` holds the block sums of every
// level of the hierarchy: eplog_scan_levels(n) counts.
int64_t eplog_scan_levels(int64_t n);
hipError_t launch_eplog_scan(int32_t *a, int64_t n, int32_t *levels, int32_t *total, hipStream_t s);
// The walk again: entry number offsets[t * W + w] + (its rank inside the wave) goes to out[base + that]; the carry is
// advanced over the T frames.
hipError_t launch_eplog_scatter(const EpLogWalk &k, const int32_t *offsets, const EpLogList &out, int64_t base,
                                hipStream_t s);
// dst[dst0 + i] = src[src0 + i] for i < n, every column and the env
hipError_t launch_eplog_copy(const EpLogList &dst, int64_t dst0, const EpLogList &src, int64_t src0, int64_t n,
                             hipStream_t s);
// fin[0 .. 2] = sum, min, max of x[0 .. n - 1] in float64; then fin[3] = the sum of (x - fin[0] / n)^2.  A fixed tree:
// kEpLogStat values per workgroup and level.  `ws` holds eplog_stat_ws(n) doubles.
int64_t eplog_stat_ws(int64_t n);
hipError_t launch_eplog_stats(const float *x, int64_t n, double *ws, double *fin, hipStream_t s);

}  // namespace zenvk
