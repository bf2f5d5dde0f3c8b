// order_rows.hpp -- K22 (order_rows.hip): the solver-ordered handles' network rows.  TSPOrderEnv's observation row is
// (Z, 7): the six features of the task's zone row plus 0.5^(position in the solver's route)
// (main/envs/TSP_order_env.py:37-47).  The step kernels keep writing the 6-wide rows and k_order_step the order
// value; this kernel puts the two together where a network is about to read them.  Internal: not installed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace zenvk {

constexpr int kOrderRowIn = 6;                  // zenv_zone_feat() of a TSP config
constexpr int kOrderRowOut = kOrderRowIn + 1;   // the network row width of such a handle (zenv_order_rows)

// dst[r][0..5] = zone_obs[r][0..5], dst[r][6] = order_val[r] for the `rows` = N * Z zone rows: bit copies.
// dst must be 16-byte aligned (the handle's allocations and the experience buffers' frame slots are).
hipError_t launch_order_rows(const float *zone_obs, const float *order_val, float *dst, int64_t rows, hipStream_t s);

}  // namespace zenvk
