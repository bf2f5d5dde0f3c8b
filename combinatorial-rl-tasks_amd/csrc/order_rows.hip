// order_rows.hip -- K22: the (Z, 7) rows of TSPOrderEnv (main/envs/TSP_order_env.py:37-47) for the flat network, gfx950.
//
// The output is indexed by FLOAT, not by row: a 28-byte row per lane would store 7 dwords at a 28-byte lane stride,
// seven partial passes over every cache line.  Here a lane owns four consecutive output floats and stores them as one
// 16-byte piece, so a wave's store instruction covers 1 KiB of contiguous destination; the (at most two) rows a piece
// touches are gathered with scalar loads that consecutive lanes serve from the same cache lines (the inputs are 6/7
// and 1/7 of the output's bytes and are read once).  A frame slot of the experience buffers starts wherever
// t * N * Z * 7 floats lands, so the 16-byte grid is laid from the first aligned float of dst: lane 0 of the launch
// writes the up-to-three floats before it, the last piece is cut at the end.  Nothing depends on Z or N.
#include <hip/hip_runtime.h>

#include "order_rows.hpp"

namespace zenvk {

namespace {

__device__ __forceinline__ float order_rows_elem(const float *__restrict__ zone_obs, const float *__restrict__ order_val,
                                                 int64_t row, int col)
{
    return col < kOrderRowIn ? zone_obs[row * kOrderRowIn + col] : order_val[row];
}

__global__ __launch_bounds__(256) void k_order_rows(const float *__restrict__ zone_obs,
                                                    const float *__restrict__ order_val, float *__restrict__ dst,
                                                    int64_t total, int lead)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0)
        for (int i = 0; i < lead; ++i)      // lead <= 3 < 7: row 0 (and lead <= total, see the launcher)
            dst[i] = order_rows_elem(zone_obs, order_val, 0, i);
    const int64_t i0 = lead + 4 * g;
    if (i0 >= total) return;
    int64_t row = i0 / kOrderRowOut;
    int col = (int)(i0 - row * kOrderRowOut);
    float v[4];
    const int n = total - i0 < 4 ? (int)(total - i0) : 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = k < n ? order_rows_elem(zone_obs, order_val, row, col) : 0.f;
        if (++col == kOrderRowOut) col = 0, ++row;
    }
    if (n == 4) {
        *reinterpret_cast<float4 *>(dst + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < n) dst[i0 + k] = v[k];
    }
}

// One lane per env, like K7 (order_rows.hpp: OrderWait).
__global__ __launch_bounds__(256) void k_order_wait(const uint8_t *__restrict__ done_out, const Sched *__restrict__ sched,
                                                    uint8_t *__restrict__ seen, float *__restrict__ order_val,
                                                    double *__restrict__ shaped, int n, int zones)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n) return;
    const bool left_alone = done_out[env] != 0 && sched[env].done_state != 0;
    if (!left_alone) {
        seen[env] = 0;
    } else if (!seen[env]) {
        seen[env] = 1;                                  // the finishing step: its observation is the real one
    } else {
        float *val = order_val + (size_t)env * zones;
        for (int z = 0; z < zones; ++z) val[z] = 0.f;
        shaped[env] = 0.0;
    }
}

__global__ __launch_bounds__(256) void k_order_wait_clear(uint8_t *__restrict__ seen, const uint8_t *__restrict__ mask, int n)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env < n && mask[env]) seen[env] = 0;
}

}  // namespace

hipError_t order_wait_after_step(OrderWait &w, const DevParams &p, int auto_reset, hipStream_t s)
{
    if (!w.seen) return hipErrorInvalidValue;
    if (auto_reset) {
        if (!w.live) return hipSuccess;
        w.live = false;                                 // every waiting env came back with this step
        return hipMemsetAsync(w.seen, 0, (size_t)p.N, s);
    }
    w.live = true;
    hipLaunchKernelGGL(k_order_wait, dim3((p.N + 255) / 256), dim3(256), 0, s, p.done_out, p.sched, w.seen, p.order_val,
                       p.shaped, p.N, p.Z);
    return hipGetLastError();
}

hipError_t order_wait_after_reset(OrderWait &w, const DevParams &p, const uint8_t *mask, hipStream_t s)
{
    if (!w.seen) return hipErrorInvalidValue;
    if (!w.live) return hipSuccess;
    if (!mask) {
        w.live = false;
        return hipMemsetAsync(w.seen, 0, (size_t)p.N, s);
    }
    hipLaunchKernelGGL(k_order_wait_clear, dim3((p.N + 255) / 256), dim3(256), 0, s, w.seen, mask, p.N);
    return hipGetLastError();
}

hipError_t launch_order_rows(const float *zone_obs, const float *order_val, float *dst, int64_t rows, hipStream_t s)
{
    const int64_t total = rows * kOrderRowOut;
    if (total <= 0) return hipSuccess;
    // floats up to the first 16-byte boundary of dst (dst is a float pointer: 4-byte aligned)
    const int to_boundary = (int)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / 4);
    const int lead = (int)(total < to_boundary ? total : to_boundary);
    const int64_t pieces = (total - lead + 3) / 4;
    const int64_t blocks = pieces > 0 ? (pieces + 255) / 256 : 1;
    hipLaunchKernelGGL(k_order_rows, dim3((unsigned)blocks), dim3(256), 0, s, zone_obs, order_val, dst, total, lead);
    return hipGetLastError();
}

}  // namespace zenvk
