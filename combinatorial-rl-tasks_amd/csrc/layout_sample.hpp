// layout_sample.hpp -- K20 (layout_sample.hip): Engine.reset()'s random half sampled on the device, straight into bank
// slots, and the ring schedule's stale-slot list.  See DESIGN.md 4 (K20).
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "dev_params.hpp"
#include "layout_sampler.hpp"

namespace zenvk {

// What the sampling kernels leave for the host (zenv_sample_status): every entry that was NOT written into its slot
// is counted in n_failed, the first ZENV_SAMPLE_STATUS_CAP of them are listed.
struct SampleStatus {
    uint32_t n_failed;
    uint32_t pad_;
    unsigned long long n_sampled;          // layouts written since the handle was made
    int32_t slots[ZENV_SAMPLE_STATUS_CAP];
    int32_t codes[ZENV_SAMPLE_STATUS_CAP];
    int64_t seeds[ZENV_SAMPLE_STATUS_CAP];
};

struct LayoutSampleArgs {
    SamplerCfg c;
    double *bank_robot, *bank_zone;        // the bank the rows go into (not necessarily the handle's current one)
    int32_t *bank_aux;
    int64_t *bank_seed;
    int32_t bank_size;
    int32_t count;                         // entries, when count_dev is null
    const uint32_t *count_dev;             // else: the count a previous kernel left in device memory
    const int32_t *slots;                  // entry e -> slot slots[e]; null: slot e
    const int64_t *seeds;                  // entry e -> env seed seeds[e]
    SampleStatus *status;
};

// One wave per entry, grid-stride over the list: `grid` blocks of 64 threads.  order (TSP configs): the ORDER
// instantiation -- the wave that sampled a layout also solves its tour (K21, route_solver.hpp) and the aux column it
// writes is the tour's ranks.
hipError_t launch_layout_sample(const LayoutSampleArgs &a, int grid, hipStream_t s, bool order = false);

// K21 over caller-supplied layouts (device pointers): robot [count][2], zones [count][Z][2] -> rank [count][Z] and, unless
// null, moves [count][5] (accepted moves per operator: or-opt 1, 2, 3, exchange, 2-opt).  One wave per layout,
// grid-stride; 1 <= Z <= ZENV_MAX_ZONES, every coordinate finite and within +-1e9 (the caller checks).
hipError_t launch_route_ranks(const double *robot, const double *zones, int count, int Z, int32_t *rank, int32_t *moves,
                              int grid, hipStream_t s);

// zenv_det_ops on the device: out[i] = det_log(a[i]) / det_div(a[i], b[i]) / det_sqrt(a[i]) (device pointers; b only
// for DET_OP_DIV), compiled from det_log.hpp as the sampling kernel is.
enum { DET_OP_LOG = 0, DET_OP_DIV = 1, DET_OP_SQRT = 2 };   // == ZENV_DET_OP_*
hipError_t launch_det_ops(int op, const double *a, const double *b, double *out, int n, hipStream_t s);

// The slots of a streamed ring that do not hold the episode they must (zenv_ring_refill): for env i and ring position
// j the slot slot_first[i] + j must hold episode e_j = the smallest e >= episode_idx[i] with e mod depth == j, i.e.
// bank_seed == seed0[i] + e_j; the others are appended to (list_slots, list_seeds), *count of them (zeroed by the
// caller; at most N * depth).
hipError_t launch_ring_stale(const DevParams &p, const int64_t *seed0, int32_t *list_slots, int64_t *list_seeds,
                             uint32_t *count, hipStream_t s);

}  // namespace zenvk
