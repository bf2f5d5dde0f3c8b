// order_rows.hpp -- K22 (order_rows.hip): the solver-ordered handles' network rows.  TSPOrderEnv's observation row is
// (Z, 7): the six features of the task's zone row plus 0.5^(position in the solver's route)
// (main/envs/TSP_order_env.py:37-47).  The step kernels keep writing the 6-wide rows and k_order_step the order
// value; this kernel puts the two together where a network is about to read them.  Internal: not installed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "dev_params.hpp"

namespace zenvk {

constexpr int kOrderRowIn = 6;                  // zenv_zone_feat() of a TSP config
constexpr int kOrderRowOut = kOrderRowIn + 1;   // the network row width of such a handle (zenv_order_rows)

// dst[r][0..5] = zone_obs[r][0..5], dst[r][6] = order_val[r] for the `rows` = N * Z zone rows: bit copies.
// dst must be 16-byte aligned (the handle's allocations and the experience buffers' frame slots are).
hipError_t launch_order_rows(const float *zone_obs, const float *order_val, float *dst, int64_t rows, hipStream_t s);

// WaitWrapper on a solver-ordered handle (main/envs/wrappers.py:34-50): an env that had finished BEFORE a step and was
// left alone (zenv_step with auto_reset 0) answers with an all-zero observation -- the order column of the (Z, 7) rows
// with it -- reward 0, done and an empty info.  k_order_step (K7) sees only the state after the step kernel, where the
// finishing step (the real terminal observation and its feature) and the waits behind it look alike, and emits the
// leftover route's feature on both.  `seen` [N] remembers that an env's finishing step has passed: k_order_wait, behind
// k_order_step on every step without auto-reset, sets it there and on every later such step writes zeros to the env's
// order_val row and 0 to its shaped reward.  order_pos is left alone: the leftover route is what the next reset's first
// observation shows.  An auto-reset step revives every waiting env and a reset the envs of its mask: both clear `seen`.
// `live` keeps all of this off the handles that never step without auto-reset.
struct OrderWait {
    uint8_t *seen = nullptr;    // [N], zeroed by zenv_order_enable
    bool live = false;          // a step without auto-reset has run since `seen` was last all zero
};
hipError_t order_wait_after_step(OrderWait &w, const DevParams &p, int auto_reset, hipStream_t s);    // behind launch_order_step
hipError_t order_wait_after_reset(OrderWait &w, const DevParams &p, const uint8_t *mask, hipStream_t s);   // behind launch_order_reset

}  // namespace zenvk
