// zenv_layout.cpp -- layouts sampled on the device (K20): the host instantiation of the shared sampler
// (zenv_sample_layout_shared, usable without a GPU), the synchronous device builders, the stream-ordered refills and
// the streamed ring.  Host-side plumbing only; the kernels are layout_sample.hip and k_bank_derive.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "host_sampler.hpp"
#include "layout_sample.hpp"
#include "route_solver.hpp"
#include "zenv_handle.hpp"

namespace zenvk {

double keepout_threshold(double A)
{
    if (!(A > 0.0)) return 0.0;                      // sqrt(s) < A never holds; neither does s < 0
    double t = A * A;
    while (t > 0.0 && std::sqrt(std::nextafter(t, 0.0)) >= A) t = std::nextafter(t, 0.0);
    while (std::sqrt(t) < A) t = std::nextafter(t, INFINITY);
    return t;                                        // the smallest double whose sqrt is >= A
}

SamplerCfg make_sampler_cfg(const zenv_config &cfg)
{
    SamplerCfg c{};
    c.task = cfg.task;
    c.Z = cfg.num_zones;
    c.n_zones_locations = cfg.n_zones_locations;
    c.n_robot_locations = cfg.n_robot_locations;
    c.robot_rot_fixed = cfg.robot_rot_fixed;
    c.extent = cfg.extent;
    c.robot_keepout = cfg.robot_keepout;
    c.zones_keepout = cfg.zones_keepout;
    c.robot_rot = cfg.robot_rot;
    c.num_steps = cfg.num_steps;
    c.beta_a = cfg.beta_a;
    c.beta_b = cfg.beta_b;
    // host_sampler.cpp: placed[j].keepout + cfg.placements_margin + keepout, left to right
    c.t_robot_zone = keepout_threshold((cfg.robot_keepout + cfg.placements_margin) + cfg.zones_keepout);
    c.t_zone_zone = keepout_threshold((cfg.zones_keepout + cfg.placements_margin) + cfg.zones_keepout);
    std::memcpy(c.robot_location, cfg.robot_location, sizeof(c.robot_location));
    c.zones_locations = &cfg.zones_locations[0][0];      // the caller's config outlives the SamplerCfg
    return c;
}

int sample_layout_shared_host(const zenv_config &cfg, int64_t seed, Layout &out)
{
    const int Z = cfg.num_zones;
    std::memset(&out, 0, sizeof(out));
    const SamplerCfg c = make_sampler_cfg(cfg);
    HostLanes st;
    std::memset(st.aux, 0, sizeof(st.aux));
    const int code = sample_layout_shared(c, cfg.task == ZENV_TASK_COLOUR_MATCH, cfg.task == ZENV_TASK_TIMED_TSP,
                                          (uint32_t)seed, kSamplerHostAttempts, st, out.robot_rot, out.restarts);
    if (code != SAMPLE_OK) return ZENV_E_LAYOUT;
    out.robot_x = st.x[0];
    out.robot_y = st.y[0];
    for (int z = 0; z < Z; ++z) {
        out.zone_xy[z][0] = st.x[z + 1];
        out.zone_xy[z][1] = st.y[z + 1];
        out.aux[z] = st.aux[z];
    }
    return 0;
}

}  // namespace zenvk

namespace {

constexpr int kMaxGrid = 256 * 32;     // one wave per block: what 256 CUs hold at 32 waves each

bool seed_in_range(int64_t seed) { return seed >= 0 && seed + 1 <= 0xFFFFFFFFll; }

int device_sampling_allowed(const zenv *h)
{
    if (h->cfg.task == ZENV_TASK_TIMED_TSP && !h->ls.timed_device)
        return fail(ZENV_E_STATE, "TimedTSP layouts are sampled on the host: the deadlines are int(beta * num_steps) with beta "
                                  "through the host libm's log, which the device's math library does not reproduce bit for bit "
                                  "(zenv_timed_layouts_device switches the handle to the shared det_log's deadlines)");
    if (h->order_enabled && !h->ls.order_device)
        return fail(ZENV_E_STATE, "solver-ordered layouts are sampled on the host: their bank rows carry zenv_route_ranks' route "
                                  "(zenv_order_routes_device lets the device solve that tour for the rows it samples)");
    return ZENV_OK;
}

// the ORDER instantiation of the sampling kernel: the handle is solver-ordered and has opted in
bool device_routes(const zenv *h) { return h->order_enabled && h->ls.order_device; }

// The host instantiation of the shared tour (route_solver.hpp): rank[Z] and, unless null, moves[5].
void route_ranks_shared_host(const double *robot_xy, const double *zone_xy, int Z, int32_t *rank, int32_t *moves_or_null)
{
    HostRouteLanes rt;
    rt.n = Z + 1;
    rt.rank = rank;
    rt.xs[0] = robot_xy[0];
    rt.ys[0] = robot_xy[1];
    for (int z = 0; z < Z; ++z) {
        rt.xs[z + 1] = zone_xy[2 * z];
        rt.ys[z + 1] = zone_xy[2 * z + 1];
    }
    int32_t moves[ROUTE_N_OPS];
    route_solve_shared(Z, rt, moves);
    if (moves_or_null) std::memcpy(moves_or_null, moves, sizeof(moves));
}

// the argument checks the two new route calls share (count layouts)
int route_args_ok(const double *robot_xy, const double *zone_xy, int64_t count, int num_zones, const int32_t *rank)
{
    if (!robot_xy || !zone_xy || !rank) return fail(ZENV_E_ARG, "null argument");
    if (num_zones < 1 || num_zones > ZENV_MAX_ZONES) return fail(ZENV_E_ARG, "num_zones outside [1,%d]", ZENV_MAX_ZONES);
    for (int64_t i = 0; i < count * 2; ++i)
        if (!route_coord_ok(robot_xy[i])) return fail(ZENV_E_ARG, "robot coordinate %g: not finite or beyond +-1e9", robot_xy[i]);
    for (int64_t i = 0; i < count * num_zones * 2; ++i)
        if (!route_coord_ok(zone_xy[i])) return fail(ZENV_E_ARG, "zone coordinate %g: not finite or beyond +-1e9", zone_xy[i]);
    return ZENV_OK;
}

int ensure_status(zenv *h)
{
    if (h->ls.mem) return ZENV_OK;
    // [status | the stale list's count, padded to 16 bytes | the config's fixed zone locations]
    const size_t bytes = sizeof(SampleStatus) + 16 + sizeof(h->cfg.zones_locations);
    HIP_TRY(hipMalloc(&h->ls.mem, bytes));
    HIP_TRY(hipMemset(h->ls.mem, 0, bytes));
    h->ls.status = static_cast<SampleStatus *>(h->ls.mem);
    h->ls.count = reinterpret_cast<uint32_t *>(static_cast<char *>(h->ls.mem) + sizeof(SampleStatus));
    h->ls.zones_locations = reinterpret_cast<double *>(static_cast<char *>(h->ls.mem) + sizeof(SampleStatus) + 16);
    HIP_TRY(hipMemcpy(h->ls.zones_locations, h->cfg.zones_locations, sizeof(h->cfg.zones_locations), hipMemcpyHostToDevice));
    return ZENV_OK;
}

// room for `n` (slot, seed) entries on the device; growing waits for the launches that read the old lists
int ensure_lists(zenv *h, size_t n)
{
    if (h->ls.list_cap >= n) return ZENV_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->ls.list_mem) (void)hipFree(h->ls.list_mem);
    h->ls.list_mem = nullptr;
    h->ls.list_cap = 0;
    const size_t cap = std::max(n, (size_t)1024);
    HIP_TRY(hipMalloc(&h->ls.list_mem, cap * (sizeof(int64_t) + sizeof(int32_t))));
    h->ls.list_seeds = static_cast<int64_t *>(h->ls.list_mem);
    h->ls.list_slots = reinterpret_cast<int32_t *>(h->ls.list_seeds + cap);
    h->ls.list_cap = cap;
    return ZENV_OK;
}

LayoutSampleArgs sample_args(const zenv *h, void *const bank[4], int32_t bank_size)
{
    LayoutSampleArgs a{};
    a.c = make_sampler_cfg(h->cfg);
    a.c.zones_locations = h->ls.zones_locations;
    a.bank_robot = static_cast<double *>(bank[0]);
    a.bank_zone = static_cast<double *>(bank[1]);
    a.bank_aux = static_cast<int32_t *>(bank[2]);
    a.bank_seed = static_cast<int64_t *>(bank[3]);
    a.bank_size = bank_size;
    a.status = h->ls.status;
    return a;
}

struct Failures {
    uint32_t n = 0;
    std::vector<int32_t> slots, codes;
    std::vector<int64_t> seeds;
};

// Synchronises; reads the failure list (the listed part) and, with `clear`, empties it.  total: n_sampled.
int take_status(zenv *h, Failures &f, unsigned long long *total, bool clear = true)
{
    HIP_TRY(hipStreamSynchronize(h->stream));
    struct { uint32_t n_failed, pad; unsigned long long n_sampled; } head;
    HIP_TRY(hipMemcpy(&head, h->ls.status, sizeof(head), hipMemcpyDeviceToHost));
    f.n = head.n_failed;
    if (total) *total = head.n_sampled;
    const size_t listed = clear ? std::min<size_t>(head.n_failed, ZENV_SAMPLE_STATUS_CAP) : 0;
    f.slots.resize(listed);
    f.codes.resize(listed);
    f.seeds.resize(listed);
    if (listed) {
        HIP_TRY(hipMemcpy(f.slots.data(), h->ls.status->slots, listed * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(f.codes.data(), h->ls.status->codes, listed * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(f.seeds.data(), h->ls.status->seeds, listed * sizeof(int64_t), hipMemcpyDeviceToHost));
        // n_failed (and its pad); n_sampled runs on.  The handle's stream is hipStreamNonBlocking: a null-stream memset
        // would not be ordered before later launches on it, so the clear goes on the handle's stream itself
        HIP_TRY(hipMemsetAsync(h->ls.status, 0, 8, h->stream));
    }
    return ZENV_OK;
}

// The synchronous builders: `count` seeds -> a fresh bank, sampled on the device, finished by the host where the
// device gave up.  On any error the handle's bank is untouched.
int build_on_device(zenv *h, const int64_t *seed_list, int count)
{
    int rc = device_sampling_allowed(h);
    if (rc) return rc;
    rc = use_device(h);
    if (rc) return rc;
    for (int i = 0; i < count; ++i)
        if (!seed_in_range(seed_list[i])) return fail(ZENV_E_ARG, "Seed must be between 0 and 2**32 - 1");
    rc = ensure_status(h);
    if (rc) return rc;
    const size_t S = (size_t)count, Z = (size_t)h->cfg.num_zones;
    rc = ensure_lists(h, S);
    if (rc) return rc;
    // failures of earlier asynchronous refills stay the caller's to collect: this call must start from an empty list
    Failures before;
    rc = take_status(h, before, nullptr, false);
    if (rc) return rc;
    if (before.n)
        return fail(ZENV_E_STATE, "%u unfinished device refills are waiting: call zenv_sample_status first", before.n);
    const size_t bytes[5] = { S * 4 * sizeof(double), S * Z * 2 * sizeof(double), S * Z * sizeof(int32_t),
                              S * sizeof(int64_t), S * 3 * sizeof(float4) };
    void *fresh[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    auto drop = [&fresh]() {
        for (void *m : fresh)
            if (m) (void)hipFree(m);
    };
    hipError_t err = hipSuccess;
    for (int i = 0; i < 5 && err == hipSuccess; ++i) err = hipMalloc(&fresh[i], bytes[i]);
    if (err == hipSuccess) err = hipMemcpy(h->ls.list_seeds, seed_list, S * sizeof(int64_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        LayoutSampleArgs a = sample_args(h, fresh, (int32_t)S);
        a.count = count;
        a.seeds = h->ls.list_seeds;
        err = launch_layout_sample(a, std::min(count, kMaxGrid), h->stream, device_routes(h));
    }
    if (err != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        drop();
        return fail(ZENV_E_HIP, "sampling the layout bank: %s", hipGetErrorString(err));
    }
    Failures f;
    rc = take_status(h, f, nullptr);
    if (rc) {
        drop();
        return rc;
    }
    // the device gave up on these after ZENV_DEVICE_RESTARTS restarts (or they did not fit the list): the host sampler
    // yields the same bits, or the reference's ResamplingError.  A report beyond the listed ones names no slot, so
    // every slot is looked at then (more than ZENV_SAMPLE_STATUS_CAP failures: not a config anyone trains on).
    std::vector<int32_t> redo(f.slots);
    if (f.n > f.slots.size()) {
        redo.resize(S);
        for (size_t i = 0; i < S; ++i) redo[i] = (int32_t)i;
    }
    for (int32_t slot : redo) {
        Layout L;
        // a TimedTSP bank is defined by the shared sampler's det_log: its host instantiation finishes it, not libm's
        if (h->ls.timed_device ? sample_layout_shared_host(h->cfg, seed_list[slot], L) : sample_layout(h->cfg, seed_list[slot], L)) {
            drop();
            return fail(ZENV_E_LAYOUT, "Failed to sample layout of objects (seed %lld)", (long long)seed_list[slot]);
        }
        // a solver-ordered row's aux column is the tour of its layout, not the sampler's (empty) column
        if (device_routes(h)) {
            const double robot_xy[2] = { L.robot_x, L.robot_y };
            route_ranks_shared_host(robot_xy, &L.zone_xy[0][0], (int)Z, L.aux, nullptr);
        }
        double s, c;
        det_sincos(L.robot_rot / 2, s, c);
        const double robot4[4] = { L.robot_x, L.robot_y, c, s };
        err = hipMemcpy(static_cast<double *>(fresh[0]) + 4 * (size_t)slot, robot4, sizeof(robot4), hipMemcpyHostToDevice);
        if (err == hipSuccess)
            err = hipMemcpy(static_cast<double *>(fresh[1]) + 2 * Z * (size_t)slot, L.zone_xy, 2 * Z * sizeof(double),
                            hipMemcpyHostToDevice);
        if (err == hipSuccess)
            err = hipMemcpy(static_cast<int32_t *>(fresh[2]) + Z * (size_t)slot, L.aux, Z * sizeof(int32_t), hipMemcpyHostToDevice);
        if (err == hipSuccess)
            err = hipMemcpy(static_cast<int64_t *>(fresh[3]) + slot, &seed_list[slot], sizeof(int64_t), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            drop();
            return fail(ZENV_E_HIP, "finishing the layout bank: %s", hipGetErrorString(err));
        }
    }
    return adopt_bank(h, fresh, S);
}

}  // namespace

namespace {

// numpy's beta takes Joehnk's algorithm (pow / exp) unless both parameters exceed 1; the samplers have the other branch
int beta_branch_ok(const zenv_config &cfg)
{
    if (!(cfg.beta_a > 1.0) || !(cfg.beta_b > 1.0))
        return fail(ZENV_E_ARG, "beta_a = %g, beta_b = %g: the deadline draw implements numpy's beta for a > 1 and b > 1 only",
                    cfg.beta_a, cfg.beta_b);
    return ZENV_OK;
}

// zenv_sample_layout's outputs from the shared sampler's host instantiation
int shared_host_out(const zenv_config &cfg, int64_t seed, double *robot_xyrot, double *zone_xy, int32_t *aux, int32_t *restarts)
{
    if (!seed_in_range(seed)) return fail(ZENV_E_ARG, "Seed must be between 0 and 2**32 - 1");
    Layout L;
    const int rc = sample_layout_shared_host(cfg, seed, L);
    if (restarts) *restarts = L.restarts;
    if (rc) return fail(ZENV_E_LAYOUT, "Failed to sample layout of objects (seed %lld)", (long long)seed);
    if (robot_xyrot) {
        robot_xyrot[0] = L.robot_x;
        robot_xyrot[1] = L.robot_y;
        robot_xyrot[2] = L.robot_rot;
    }
    for (int z = 0; z < cfg.num_zones; ++z) {
        if (zone_xy) {
            zone_xy[2 * z] = L.zone_xy[z][0];
            zone_xy[2 * z + 1] = L.zone_xy[z][1];
        }
        if (aux) aux[z] = L.aux[z];
    }
    return ZENV_OK;
}

}  // namespace

void layout_free(zenv *h)
{
    if (h->ls.mem) (void)hipFree(h->ls.mem);
    if (h->ls.list_mem) (void)hipFree(h->ls.list_mem);
    if (h->ls.stage_host) (void)hipHostFree(h->ls.stage_host);
    if (h->ls.stage_done) (void)hipEventDestroy(h->ls.stage_done);
    if (h->ls.ring_seed0) (void)hipFree(h->ls.ring_seed0);
    h->ls = {};
}

extern "C" int zenv_layout_thresholds(const zenv_config *cfg, double *rhs, double *thr)
{
    if (!cfg || !rhs || !thr) return fail(ZENV_E_ARG, "null argument");
    int rc = validate_config(*cfg);
    if (rc) return rc;
    rhs[0] = (cfg->robot_keepout + cfg->placements_margin) + cfg->zones_keepout;
    rhs[1] = (cfg->zones_keepout + cfg->placements_margin) + cfg->zones_keepout;
    const SamplerCfg c = make_sampler_cfg(*cfg);
    thr[0] = c.t_robot_zone;
    thr[1] = c.t_zone_zone;
    return ZENV_OK;
}

extern "C" int zenv_sample_layout_shared(const zenv_config *cfg, int64_t seed, double *robot_xyrot, double *zone_xy,
                                         int32_t *aux, int32_t *restarts)
{
    if (!cfg) return fail(ZENV_E_ARG, "null config");
    int rc = validate_config(*cfg);
    if (rc) return rc;
    if (cfg->task == ZENV_TASK_TIMED_TSP)
        return fail(ZENV_E_ARG, "the shared sampler does not draw TimedTSP deadlines (host libm's log): use zenv_sample_layout, "
                                "or zenv_sample_layout_timed for the shared det_log's deadlines");
    return shared_host_out(*cfg, seed, robot_xyrot, zone_xy, aux, restarts);
}

extern "C" int zenv_sample_layout_timed(const zenv_config *cfg, int64_t seed, double *robot_xyrot, double *zone_xy,
                                        int32_t *aux, int32_t *restarts)
{
    if (!cfg) return fail(ZENV_E_ARG, "null config");
    int rc = validate_config(*cfg);
    if (rc) return rc;
    if (cfg->task != ZENV_TASK_TIMED_TSP) return fail(ZENV_E_ARG, "zenv_sample_layout_timed samples TimedTSP configs");
    rc = beta_branch_ok(*cfg);
    if (rc) return rc;
    return shared_host_out(*cfg, seed, robot_xyrot, zone_xy, aux, restarts);
}

extern "C" int zenv_timed_layouts_device(zenv_t *h, int enable)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (h->cfg.task != ZENV_TASK_TIMED_TSP)
        return fail(ZENV_E_ARG, "zenv_timed_layouts_device is for TimedTSP handles: the other tasks' layouts need no switch");
    int rc = beta_branch_ok(h->cfg);
    if (rc) return rc;
    h->ls.timed_device = enable != 0;
    return ZENV_OK;
}

extern "C" int zenv_order_routes_device(zenv_t *h, int enable)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->order_enabled)
        return fail(ZENV_E_ARG, "zenv_order_routes_device is for solver-ordered handles (zenv_order_enable): the other "
                                "handles' layouts need no switch");
    h->ls.order_device = enable != 0;
    return ZENV_OK;
}

extern "C" int zenv_route_ranks_shared(const double *robot_xy, const double *zone_xy, int num_zones, int32_t *rank,
                                       int32_t *moves_or_null)
{
    int rc = route_args_ok(robot_xy, zone_xy, 1, num_zones, rank);
    if (rc) return rc;
    route_ranks_shared_host(robot_xy, zone_xy, num_zones, rank, moves_or_null);
    return ZENV_OK;
}

extern "C" int zenv_route_ranks_device(zenv_t *h, const double *robot_xy, const double *zone_xy, int count, int num_zones,
                                       int32_t *rank, int32_t *moves_or_null)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (count < 0) return fail(ZENV_E_ARG, "count must be >= 0");
    int rc = route_args_ok(robot_xy, zone_xy, count, num_zones, rank);
    if (rc) return rc;
    if (count == 0) return ZENV_OK;
    rc = use_device(h);
    if (rc) return rc;
    // [robot | zones | moves | rank] in one allocation: the doubles first
    const size_t n = (size_t)count, Z = (size_t)num_zones;
    const size_t b_robot = n * 2 * sizeof(double), b_zone = n * Z * 2 * sizeof(double);
    const size_t b_moves = n * ROUTE_N_OPS * sizeof(int32_t), b_rank = n * Z * sizeof(int32_t);
    char *d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), b_robot + b_zone + b_moves + b_rank));
    double *d_robot = reinterpret_cast<double *>(d), *d_zone = reinterpret_cast<double *>(d + b_robot);
    int32_t *d_moves = reinterpret_cast<int32_t *>(d + b_robot + b_zone), *d_rank = d_moves + n * ROUTE_N_OPS;
    hipError_t err = hipMemcpyAsync(d_robot, robot_xy, b_robot, hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(d_zone, zone_xy, b_zone, hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess)
        err = launch_route_ranks(d_robot, d_zone, count, num_zones, d_rank, moves_or_null ? d_moves : nullptr,
                                 std::min(count, kMaxGrid), h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(rank, d_rank, b_rank, hipMemcpyDeviceToHost, h->stream);
    if (err == hipSuccess && moves_or_null) err = hipMemcpyAsync(moves_or_null, d_moves, b_moves, hipMemcpyDeviceToHost, h->stream);
    const hipError_t done = hipStreamSynchronize(h->stream);
    (void)hipFree(d);
    if (err == hipSuccess) err = done;
    if (err != hipSuccess) return fail(ZENV_E_HIP, "zenv_route_ranks_device: %s", hipGetErrorString(err));
    return ZENV_OK;
}

extern "C" int zenv_det_ops(int op, const double *a, const double *b, double *out, int n, int on_device)
{
    if (op != DET_OP_LOG && op != DET_OP_DIV && op != DET_OP_SQRT) return fail(ZENV_E_ARG, "unknown det op %d", op);
    if (n < 0) return fail(ZENV_E_ARG, "n must be >= 0");
    if (n == 0) return ZENV_OK;
    if (!a || !out || (op == DET_OP_DIV && !b)) return fail(ZENV_E_ARG, "null argument");
    if (!on_device) {
        for (int i = 0; i < n; ++i)
            out[i] = op == DET_OP_LOG ? det_log(a[i]) : op == DET_OP_DIV ? det_div(a[i], b[i]) : det_sqrt(a[i]);
        return ZENV_OK;
    }
    const size_t bytes = (size_t)n * sizeof(double);
    double *d = nullptr;                                 // [a | b | out]
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), 3 * bytes));
    hipError_t err = hipMemcpy(d, a, bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess && op == DET_OP_DIV) err = hipMemcpy(d + n, b, bytes, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_det_ops(op, d, d + n, d + 2 * (size_t)n, n, nullptr);
    if (err == hipSuccess) err = hipMemcpy(out, d + 2 * (size_t)n, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (err != hipSuccess) return fail(ZENV_E_HIP, "zenv_det_ops: %s", hipGetErrorString(err));
    return ZENV_OK;
}

extern "C" int zenv_bank_build_seeds_device(zenv_t *h, const int64_t *seed_list, int count)
{
    if (!h || !seed_list) return fail(ZENV_E_ARG, "null argument");
    if (count < 1) return fail(ZENV_E_ARG, "count must be >= 1");
    return build_on_device(h, seed_list, count);
}

extern "C" int zenv_bank_build_device(zenv_t *h, int64_t seed_first, int count)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (count < 1) return fail(ZENV_E_ARG, "count must be >= 1");
    std::vector<int64_t> seeds(count);
    for (int i = 0; i < count; ++i) seeds[i] = seed_first + i;
    return build_on_device(h, seeds.data(), count);
}

extern "C" int zenv_bank_update_device(zenv_t *h, const int32_t *slots, const int64_t *seed_list, int count)
{
    if (!h || !slots || !seed_list) return fail(ZENV_E_ARG, "null argument");
    int rc = device_sampling_allowed(h);
    if (rc) return rc;
    if (!h->bank_ready) return fail(ZENV_E_STATE, "build or set the layout bank first");
    if (count < 0) return fail(ZENV_E_ARG, "count must be >= 0");
    if (count == 0) return ZENV_OK;
    for (int i = 0; i < count; ++i)
        if (slots[i] < 0 || slots[i] >= h->p.bank_size)
            return fail(ZENV_E_ARG, "slot %d outside the bank [0,%d)", slots[i], h->p.bank_size);
    rc = use_device(h);
    if (rc) return rc;
    rc = ensure_status(h);
    if (rc) return rc;
    const size_t n = (size_t)count;
    rc = ensure_lists(h, std::max(n, (size_t)h->p.bank_size));
    if (rc) return rc;
    // 12 bytes per layout: [seeds int64 x n | slots int32 x n] in page-locked memory, two copies behind the stream's work
    const size_t need = n * (sizeof(int64_t) + sizeof(int32_t));
    if (h->ls.stage_cap < need) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (h->ls.stage_host) (void)hipHostFree(h->ls.stage_host);
        h->ls.stage_host = nullptr;
        h->ls.stage_cap = 0;
        const size_t cap = std::max(need * 2, (size_t)1 << 14);
        HIP_TRY(hipHostMalloc(&h->ls.stage_host, cap, hipHostMallocDefault));
        h->ls.stage_cap = cap;
    } else if (h->ls.stage_busy) {
        HIP_TRY(hipEventSynchronize(h->ls.stage_done));      // the previous refill's copies still read the image
    }
    char *hb = static_cast<char *>(h->ls.stage_host);
    std::memcpy(hb, seed_list, n * sizeof(int64_t));
    std::memcpy(hb + n * sizeof(int64_t), slots, n * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(h->ls.list_seeds, hb, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ls.list_slots, hb + n * sizeof(int64_t), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (!h->ls.stage_done) HIP_TRY(hipEventCreateWithFlags(&h->ls.stage_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->ls.stage_done, h->stream));
    h->ls.stage_busy = true;
    LayoutSampleArgs a = sample_args(h, h->bank_mem, h->p.bank_size);
    a.count = count;
    a.slots = h->ls.list_slots;
    a.seeds = h->ls.list_seeds;
    HIP_TRY(launch_layout_sample(a, std::min(count, kMaxGrid), h->stream, device_routes(h)));
    // a slot the sampler left alone derives to the rows it already has
    HIP_TRY(launch_bank_derive(h->p, h->ls.list_slots, count, h->stream));
    return ZENV_OK;
}

extern "C" int zenv_ring_stream(zenv_t *h, const int64_t *seed0, int32_t depth)
{
    if (!h || !seed0) return fail(ZENV_E_ARG, "null argument");
    int rc = device_sampling_allowed(h);
    if (rc) return rc;
    if (depth < 1) return fail(ZENV_E_ARG, "ring depth must be >= 1");
    const int64_t S = (int64_t)h->n_env * depth;
    if (S > 0x7FFFFFFFll) return fail(ZENV_E_ARG, "num_envs * depth = %lld slots: beyond 2^31 - 1", (long long)S);
    std::vector<int64_t> seeds((size_t)S);
    std::vector<int32_t> first(h->n_env);
    for (int i = 0; i < h->n_env; ++i) {
        first[i] = i * depth;
        for (int j = 0; j < depth; ++j) seeds[(size_t)i * depth + j] = seed0[i] + j;
    }
    rc = build_on_device(h, seeds.data(), (int)S);
    if (rc) return rc;
    if (!h->ls.ring_seed0) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->ls.ring_seed0), (size_t)h->n_env * sizeof(int64_t)));
    HIP_TRY(hipMemcpy(h->ls.ring_seed0, seed0, (size_t)h->n_env * sizeof(int64_t), hipMemcpyHostToDevice));
    rc = zenv_schedule_ring(h, first.data(), depth);
    if (rc) return rc;
    h->ls.ring_streamed = true;
    return ZENV_OK;
}

extern "C" int zenv_ring_refill(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    int rc = device_sampling_allowed(h);
    if (rc) return rc;
    if (!h->ls.ring_streamed || !h->bank_ready || !h->sched_ready || h->p.sched_mode != SCHED_RING)
        return fail(ZENV_E_STATE, "zenv_ring_refill needs the schedule zenv_ring_stream made (another schedule or bank has "
                                  "replaced it, or none was made)");
    rc = use_device(h);
    if (rc) return rc;
    const int grid = std::min(h->p.bank_size, kMaxGrid);
    HIP_TRY(hipMemsetAsync(h->ls.count, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(launch_ring_stale(h->p, h->ls.ring_seed0, h->ls.list_slots, h->ls.list_seeds, h->ls.count, h->stream));
    LayoutSampleArgs a = sample_args(h, h->bank_mem, h->p.bank_size);
    a.count_dev = h->ls.count;
    a.slots = h->ls.list_slots;
    a.seeds = h->ls.list_seeds;
    HIP_TRY(launch_layout_sample(a, grid, h->stream, device_routes(h)));
    // The derived rows: k_bank_derive takes its slot count from the launch, and how many slots were stale only the
    // device knows, so the pass covers the whole ring bank (rows of untouched slots derive to what they hold).  A
    // variant that walks the device-made list has to sit beside the device functions it shares with the step kernels,
    // in kernels.hip, whose committed PMC record (profiles/traffic.json) is keyed to that file: it comes with the next
    // profiling pass.
    HIP_TRY(launch_bank_derive(h->p, nullptr, h->p.bank_size, h->stream));
    return ZENV_OK;
}

extern "C" int zenv_sample_status(zenv_t *h, int32_t *slots, int64_t *seeds, int32_t *codes, int cap, int32_t *n_failed,
                                  int64_t *n_sampled_total)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (cap < 0) return fail(ZENV_E_ARG, "cap must be >= 0");
    int rc = use_device(h);
    if (rc) return rc;
    rc = ensure_status(h);
    if (rc) return rc;
    Failures f;
    unsigned long long total = 0;
    rc = take_status(h, f, &total);
    if (rc) return rc;
    const size_t n = std::min<size_t>(f.slots.size(), (size_t)cap);
    if (slots) std::memcpy(slots, f.slots.data(), n * sizeof(int32_t));
    if (seeds) std::memcpy(seeds, f.seeds.data(), n * sizeof(int64_t));
    if (codes) std::memcpy(codes, f.codes.data(), n * sizeof(int32_t));
    if (n_failed) *n_failed = (int32_t)std::min<uint32_t>(f.n, 0x7FFFFFFFu);
    if (n_sampled_total) *n_sampled_total = (int64_t)total;
    return ZENV_OK;
}

extern "C" int zenv_bank_read(zenv_t *h, int slot_first, int count, double *robot4, double *zone_xy, int32_t *aux,
                              int64_t *seeds, float *first12)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->bank_ready) return fail(ZENV_E_STATE, "build or set the layout bank first");
    if (count < 0 || slot_first < 0 || (int64_t)slot_first + count > h->p.bank_size)
        return fail(ZENV_E_ARG, "slots [%d, %lld) outside the bank [0,%d)", slot_first, (long long)slot_first + count, h->p.bank_size);
    int rc = use_device(h);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (count == 0) return ZENV_OK;
    const size_t Z = (size_t)h->cfg.num_zones, s0 = (size_t)slot_first, n = (size_t)count;
    if (robot4) HIP_TRY(hipMemcpy(robot4, h->p.bank_robot + 4 * s0, n * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (zone_xy) HIP_TRY(hipMemcpy(zone_xy, h->p.bank_zone + 2 * Z * s0, n * 2 * Z * sizeof(double), hipMemcpyDeviceToHost));
    if (aux) HIP_TRY(hipMemcpy(aux, h->p.bank_aux + Z * s0, n * Z * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (seeds) HIP_TRY(hipMemcpy(seeds, h->p.bank_seed + s0, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (first12) HIP_TRY(hipMemcpy(first12, h->p.bank_first + 3 * s0, n * 3 * sizeof(float4), hipMemcpyDeviceToHost));
    return ZENV_OK;
}
