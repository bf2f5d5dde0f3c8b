// layout_sample.hip -- K20: Engine.reset()'s random half on gfx950 (see layout_sampler.hpp for the arithmetic, which
// is the host's, and DESIGN.md 4 for the choice of mapping).
//
// One wave64 per env seed.  The generator's 624 words live in LDS (2 496 B per wave, so LDS never limits occupancy:
// the 32-waves-per-CU cap does); the twist runs 64 words at a time, every draw is a broadcast ds_read of one word that
// all lanes temper alike; placed object j (0 = the robot, 1 .. Z = the zones) sits in lane j's registers, so the
// keepout test of a candidate against everything placed is one compare per lane and one ballot.  Control flow is
// wave-uniform throughout: rejection loops of different seeds never share a wave, so they do not diverge.
// TimedTSP: every lane evaluates the same serial deadline draw (beta -> gamma -> gauss, det_log.hpp), lane z + 1 keeps
// zone z's deadline.
//
// K21: the solver-ordered handles' tour (route_solver.hpp, the host's route_ranks bit for bit) by one wave64 per layout.
// The int64 cost matrix (row stride route_stride(n): odd, a column read is conflict-free), the nodes' coordinates and
// the tour live in dynamic LDS sized by the layout's zone count (2 496 B at 15 zones, 9 372 B at 32), so a 15-zone
// bank still runs 32 waves per CU.  A scan evaluates 64 candidates of the host's order per step, one per lane; a ballot
// and its lowest set bit pick the host's move; the lanes permute the tour together.  Reached two ways: the ORDER
// instantiation of k_layout_sample (the wave that sampled a layout solves it and writes the ranks as the bank's aux
// column) and k_route_ranks over caller-supplied layouts.
#include <hip/hip_runtime.h>

#include "layout_sample.hpp"
#include "route_solver.hpp"

namespace zenvk {
namespace {

constexpr int kWave = 64;

struct WaveLanes {
    static constexpr int kLanes = kWave;
    uint32_t *mt;      // LDS, 624 words
    int ln;
    double x, y;       // the object this lane holds
    int32_t aux;       // lane z + 1: zone z's aux value
    __device__ __forceinline__ int lane() const { return ln; }
    // a block is one wave: the barrier costs nothing, the fence orders the wave's LDS stores before its LDS loads
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ bool any(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0ull; }
    __device__ __forceinline__ uint32_t word(int i) const { return mt[i]; }
    __device__ __forceinline__ void set_word(int i, uint32_t v) { mt[i] = v; }
    __device__ __forceinline__ double px(int) const { return x; }      // asked for by lane j only (kLanes > Z)
    __device__ __forceinline__ double py(int) const { return y; }
    __device__ __forceinline__ void place(int j, double xx, double yy)
    {
        if (ln == j) { x = xx; y = yy; }
    }
    __device__ __forceinline__ void set_aux(int z, int32_t v)
    {
        if (ln == z + 1) aux = v;
    }
};
static_assert(ZENV_MAX_ZONES + 1 <= kWave, "one lane per placed object");

// The route solver's wave: [cost int64 n x stride | x double n | y double n | tour int32 n] in dynamic LDS
// (route_lds_bytes), the ranks straight into global memory.
struct WaveRouteLanes {
    static constexpr int kLanes = kWave;
    int64_t *cost;
    double *xs, *ys;
    int32_t *tr;
    int32_t *rank;     // global: this layout's [Z] ranks
    int stride, ln;
    int32_t held;      // a permutation's staged value: tour position `ln`
    bool held_live;
    __device__ __forceinline__ WaveRouteLanes(int64_t *lds, int n, int lane, int32_t *rank_out)
        : cost(lds), xs(reinterpret_cast<double *>(lds + n * route_stride(n))), ys(xs + n),
          tr(reinterpret_cast<int32_t *>(ys + n)), rank(rank_out), stride(route_stride(n)), ln(lane), held(0), held_live(false)
    {
    }
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ uint64_t ballot(bool b) const { return __builtin_amdgcn_ballot_w64(b); }
    __device__ __forceinline__ double x(int a) const { return xs[a]; }
    __device__ __forceinline__ double y(int a) const { return ys[a]; }
    __device__ __forceinline__ int64_t d(int a, int b) const { return cost[a * stride + b]; }
    __device__ __forceinline__ void set_d(int a, int b, int64_t v) { cost[a * stride + b] = v; }
    __device__ __forceinline__ int tour(int i) const { return tr[i]; }
    __device__ __forceinline__ void set_tour(int i, int v) { tr[i] = v; }
    __device__ __forceinline__ void stage(int, int v, bool live) { held = v; held_live = live; }   // kLanes >= n: k == ln
    __device__ __forceinline__ void commit(int) { if (held_live) tr[ln] = held; }
    __device__ __forceinline__ void set_rank(int z, int v) { rank[z] = v; }
    __device__ __forceinline__ void set_xy(int a, double xx, double yy) { xs[a] = xx; ys[a] = yy; }
};
static_assert(kRouteMaxNodes <= kWave, "a permutation is one position per lane");

__device__ __forceinline__ int64_t *route_lds()
{
    extern __shared__ int64_t route_lds_mem[];
    return route_lds_mem;
}

template <int TASK, bool ORDER = false>
__global__ __launch_bounds__(kWave) void k_layout_sample(LayoutSampleArgs a)
{
    static_assert(!ORDER || TASK == ZENV_TASK_TSP, "the solver-ordered variant is a PointTSP variant");
    __shared__ uint32_t mt[624];
    const int lane = threadIdx.x, Z = a.c.Z;
    const uint32_t n = a.count_dev ? *a.count_dev : (uint32_t)a.count;
    uint32_t written = 0;
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const int slot = a.slots ? a.slots[e] : (int)e;
        const int64_t seed = a.seeds[e];
        if (slot < 0 || slot >= a.bank_size) continue;      // the host checked its lists; a device-made list is in range
        WaveLanes st;
        st.mt = mt;
        st.ln = lane;
        st.x = st.y = 0.0;
        st.aux = 0;
        double rot = 0.0;
        int32_t restarts = 0;
        int code = SAMPLE_SEED_RANGE;                        // Engine.seed: 'Seed must be between 0 and 2**32 - 1'
        if (seed >= 0 && seed + 1 <= 0xFFFFFFFFll)
            code = sample_layout_shared(a.c, TASK == ZENV_TASK_COLOUR_MATCH, TASK == ZENV_TASK_TIMED_TSP, (uint32_t)seed,
                                        kSamplerDeviceAttempts, st, rot, restarts);
        if (code == SAMPLE_OK) {
            if (lane == 0) {
                double s, c;
                det_sincos_inl(rot / 2, s, c);               // world.py rot2quat: [cos(rot/2), 0, 0, sin(rot/2)]
                double2 *br = reinterpret_cast<double2 *>(a.bank_robot + 4 * (size_t)slot);
                br[0] = make_double2(st.x, st.y);
                br[1] = make_double2(c, s);
                a.bank_seed[slot] = seed;
            } else if (lane <= Z) {
                const size_t bi = (size_t)slot * Z + (lane - 1);
                reinterpret_cast<double2 *>(a.bank_zone)[bi] = make_double2(st.x, st.y);
                if constexpr (!ORDER) a.bank_aux[bi] = st.aux;
            }
            if constexpr (ORDER) {
                // lane j holds node j's centre: the aux column is the tour's ranks (TSP_order_env.py:49-50)
                WaveRouteLanes rt(route_lds(), Z + 1, lane, a.bank_aux + (size_t)slot * Z);
                if (lane <= Z) rt.set_xy(lane, st.x, st.y);
                rt.sync();
                int32_t moves[ROUTE_N_OPS];
                route_solve_shared(Z, rt, moves);
            }
            written++;
        } else if (lane == 0) {
            // the slot stays as it was; the host hears of it (zenv_sample_status)
            const uint32_t i = atomicAdd(&a.status->n_failed, 1u);
            if (i < (uint32_t)ZENV_SAMPLE_STATUS_CAP) {
                a.status->slots[i] = slot;
                a.status->codes[i] = code;
                a.status->seeds[i] = seed;
            }
        }
        __syncthreads();                                     // the next entry's seeding stores behind this one's loads
    }
    if (lane == 0 && written) atomicAdd(&a.status->n_sampled, (unsigned long long)written);
}

__global__ __launch_bounds__(256) void k_ring_stale(DevParams p, const int64_t *__restrict__ seed0,
                                                    int32_t *__restrict__ list_slots, int64_t *__restrict__ list_seeds,
                                                    uint32_t *__restrict__ count)
{
    const int depth = p.sched_stride;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)p.N * depth) return;
    const int env = (int)(t / depth), j = (int)(t % depth);
    const int k = p.sched[env].episode_idx;                  // episodes started so far = the next episode's index
    const int ahead = (j - k % depth + depth) % depth;       // e_j = k + ahead: the smallest e >= k with e mod depth == j
    const int slot = p.slot_first[env] + j;
    if (slot < 0 || slot >= p.bank_size) return;
    const int64_t want = seed0[env] + (int64_t)k + ahead;
    if (p.bank_seed[slot] != want) {
        const uint32_t i = atomicAdd(count, 1u);             // at most N * depth entries: the lists' size
        list_slots[i] = slot;
        list_seeds[i] = want;
    }
}

// K21 over caller-supplied layouts: robot [count][2], zones [count][Z][2] -> rank [count][Z], moves [count][5] (or null)
__global__ __launch_bounds__(kWave) void k_route_ranks(const double *__restrict__ robot, const double *__restrict__ zones,
                                                       int count, int Z, int32_t *__restrict__ rank,
                                                       int32_t *__restrict__ moves_out)
{
    const int lane = threadIdx.x;
    for (int e = blockIdx.x; e < count; e += gridDim.x) {
        WaveRouteLanes rt(route_lds(), Z + 1, lane, rank + (size_t)e * Z);
        if (lane == 0) rt.set_xy(0, robot[2 * (size_t)e], robot[2 * (size_t)e + 1]);
        else if (lane <= Z) rt.set_xy(lane, zones[((size_t)e * Z + (lane - 1)) * 2], zones[((size_t)e * Z + (lane - 1)) * 2 + 1]);
        rt.sync();
        int32_t moves[ROUTE_N_OPS];
        route_solve_shared(Z, rt, moves);
        if (moves_out && lane == 0)
            for (int k = 0; k < ROUTE_N_OPS; ++k) moves_out[(size_t)e * ROUTE_N_OPS + k] = moves[k];
        __syncthreads();                                     // the next layout's stores behind this one's loads
    }
}

// zenv_det_ops: det_log / det_div / det_sqrt as the device compiles them, one element per thread
__global__ __launch_bounds__(256) void k_det_ops(int op, const double *__restrict__ a, const double *__restrict__ b,
                                                 double *__restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = op == DET_OP_LOG ? det_log(a[i]) : op == DET_OP_DIV ? det_div(a[i], b[i]) : det_sqrt(a[i]);
}

}  // namespace

hipError_t launch_det_ops(int op, const double *a, const double *b, double *out, int n, hipStream_t s)
{
    if (n < 1) return hipSuccess;
    hipLaunchKernelGGL(k_det_ops, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, op, a, b, out, n);
    return hipGetLastError();
}

size_t route_lds_bytes(int Z)
{
    const size_t n = (size_t)Z + 1;
    return n * route_stride((int)n) * sizeof(int64_t) + 2 * n * sizeof(double) + n * sizeof(int32_t);
}

hipError_t launch_route_ranks(const double *robot, const double *zones, int count, int Z, int32_t *rank, int32_t *moves,
                              int grid, hipStream_t s)
{
    if (grid < 1 || count < 1) return hipSuccess;
    hipLaunchKernelGGL(k_route_ranks, dim3(grid), dim3(kWave), route_lds_bytes(Z), s, robot, zones, count, Z, rank, moves);
    return hipGetLastError();
}

hipError_t launch_layout_sample(const LayoutSampleArgs &a, int grid, hipStream_t s, bool order)
{
    if (grid < 1) return hipSuccess;
    if (order) {
        if (a.c.task != ZENV_TASK_TSP) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_layout_sample<ZENV_TASK_TSP, true>), dim3(grid), dim3(kWave), route_lds_bytes(a.c.Z), s, a);
    } else if (a.c.task == ZENV_TASK_COLOUR_MATCH)
        hipLaunchKernelGGL(k_layout_sample<ZENV_TASK_COLOUR_MATCH>, dim3(grid), dim3(kWave), 0, s, a);
    else if (a.c.task == ZENV_TASK_TIMED_TSP)
        hipLaunchKernelGGL(k_layout_sample<ZENV_TASK_TIMED_TSP>, dim3(grid), dim3(kWave), 0, s, a);
    else
        hipLaunchKernelGGL(k_layout_sample<ZENV_TASK_TSP>, dim3(grid), dim3(kWave), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ring_stale(const DevParams &p, const int64_t *seed0, int32_t *list_slots, int64_t *list_seeds,
                             uint32_t *count, hipStream_t s)
{
    const long long n = (long long)p.N * p.sched_stride;
    hipLaunchKernelGGL(k_ring_stale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, seed0, list_slots, list_seeds,
                       count);
    return hipGetLastError();
}

}  // namespace zenvk
