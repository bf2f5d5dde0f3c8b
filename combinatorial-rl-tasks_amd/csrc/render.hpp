// render.hpp -- host-callable launcher of the top-down rasteriser in render.hip (K18).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace zenvk {

// Image i is drawn from obs + i * obs_stride (8 floats) and zone_obs + i * zone_stride (Z rows of F floats) into
// dst + i * H * W * 3.  Strides are in floats: 8 / Z * F for consecutive envs, N * 8 / N * Z * F for consecutive
// frames of one env in the time-major experience buffers.  count * H * W * 3 < 2^31 (zenv_render_check).
struct RenderParams {
    const float *obs;
    const float *zone_obs;
    const float *marks;      // [count][2] or null; a NaN component = no mark for that image
    uint8_t *dst;            // any alignment
    int64_t obs_stride, zone_stride;
    int32_t count, W, H, Z, F;
    int32_t timed;           // != 0: TimedTSP rows, an unvisited zone fades with row[6]
    float view, sx, sy;      // half-width shown; pixel pitch (2 * view) / W, (2 * view) / H
    float rz, rr;            // zone radius, robot radius (observation units)
};
hipError_t launch_render(const RenderParams &rp, hipStream_t s);

}  // namespace zenvk
