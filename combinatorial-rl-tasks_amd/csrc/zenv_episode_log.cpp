// zenv_episode_log.cpp -- the C ABI of the per-episode training logs (include/zenv.h, K19): the `logs` every
// collect_experiences of the reference returns, from the records the last collector left on the device.  The kernels:
// episode_log.hip.  The collectors (zenv_agents.cpp) arm h->eplog.source.
#include <algorithm>

#include "zenv_handle.hpp"

namespace {

constexpr int64_t kAll = (1 << ZENV_EPLOG_RETURN) | (1 << ZENV_EPLOG_RESHAPED_RETURN) | (1 << ZENV_EPLOG_NUM_FRAMES);

inline size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// one allocation: `cols` float columns and the env column of `n` entries each, `lists` times
int alloc_lists(void **mem, EpLogList *lists, int n_lists, int64_t n, size_t extra_floats, float **extra)
{
    const size_t piece = pad256((size_t)n * 4);
    const size_t bytes = piece * (size_t)(kEpLogCols + 1) * n_lists + pad256(extra_floats * 4);
    HIP_TRY(hipMalloc(mem, bytes));
    char *at = static_cast<char *>(*mem);
    for (int l = 0; l < n_lists; ++l) {
        for (int c = 0; c < kEpLogCols; ++c, at += piece) lists[l].col[c] = reinterpret_cast<float *>(at);
        lists[l].env = reinterpret_cast<int32_t *>(at);
        at += piece;
    }
    if (extra) *extra = reinterpret_cast<float *>(at);
    return ZENV_OK;
}

// the sums and the tail as a fresh algo object has them: zeros, and N entries of 0 (env -1)
int zero_state(zenv *h)
{
    auto &e = h->eplog;
    const size_t N = (size_t)h->n_env;
    for (float *c : e.carry) HIP_TRY(hipMemsetAsync(c, 0, N * 4, h->stream));
    e.cur = 0;
    for (int c = 0; c < kEpLogCols; ++c) HIP_TRY(hipMemsetAsync(e.tail[0].col[c], 0, N * 4, h->stream));
    HIP_TRY(hipMemsetAsync(e.tail[0].env, 0xFF, N * 4, h->stream));
    return ZENV_OK;
}

int ensure_state(zenv *h)
{
    auto &e = h->eplog;
    if (e.state_mem) return ZENV_OK;
    const size_t N = (size_t)h->n_env, piece = pad256(N * 4) / 4;
    float *carry = nullptr;
    if (int rc = alloc_lists(&e.state_mem, e.tail, 2, (int64_t)N, 4 * piece, &carry)) return rc;
    for (int c = 0; c < 4; ++c) e.carry[c] = carry + c * piece;
    return zero_state(h);
}

// the result's columns for `keep` entries (grown by half again, never shrunk) and the reduction's workspace beside
int ensure_result(zenv *h, int64_t keep)
{
    auto &e = h->eplog;
    if (keep <= e.cap) return ZENV_OK;
    const int64_t cap = std::max<int64_t>(keep, e.cap + e.cap / 2);
    if (e.res_mem) HIP_TRY(hipFree(e.res_mem));
    e.res_mem = nullptr;
    e.cap = 0;
    float *ws = nullptr;
    const size_t ws_doubles = (size_t)eplog_stat_ws(cap) + 8;
    if (int rc = alloc_lists(&e.res_mem, &e.res, 1, cap, ws_doubles * 2, &ws)) return rc;
    e.stat_fin = reinterpret_cast<double *>(ws);
    e.stat_ws = e.stat_fin + 8;
    e.cap = cap;
    return ZENV_OK;
}

// the (frame, wave) counts of T frames, the active counts, the scan's levels, the two totals
int ensure_counts(zenv *h, int64_t M)
{
    auto &e = h->eplog;
    if (M <= e.ws_counts) return ZENV_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (e.ws_mem) HIP_TRY(hipFree(e.ws_mem));
    e.ws_mem = nullptr;
    e.ws_counts = 0;
    const size_t piece = pad256((size_t)M * 4), lev = pad256((size_t)eplog_scan_levels(M) * 4);
    HIP_TRY(hipMalloc(&e.ws_mem, 2 * piece + lev + 256));
    char *at = static_cast<char *>(e.ws_mem);
    e.counts = reinterpret_cast<int32_t *>(at);
    e.active = reinterpret_cast<int32_t *>(at + piece);
    e.levels = reinterpret_cast<int32_t *>(at + 2 * piece);
    e.totals = reinterpret_cast<int32_t *>(at + 2 * piece + lev);
    e.ws_counts = M;
    return ZENV_OK;
}

int column_ready(zenv *h, int column, bool with_env)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (column < 0 || column >= (with_env ? ZENV_EPLOG_COUNT : ZENV_EPLOG_ENV))
        return fail(ZENV_E_ARG, "column %d is not a ZENV_EPLOG_* column%s", column, with_env ? "" : " with statistics");
    if (h->eplog.kept < 0) return fail(ZENV_E_STATE, "zenv_episode_log first");
    return use_device(h);
}

void *column_ptr(zenv *h, int column)
{
    return column == ZENV_EPLOG_ENV ? (void *)h->eplog.res.env : (void *)h->eplog.res.col[column];
}

}  // namespace

void eplog_free(zenv *h)
{
    auto &e = h->eplog;
    for (void *m : { e.state_mem, e.res_mem, e.ws_mem, (void *)e.flat_reward })
        if (m) (void)hipFree(m);
    e = {};
}

int eplog_flat_reward(zenv *h, int T)
{
    auto &e = h->eplog;
    if (e.flat_reward && e.flat_T == T) return ZENV_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (e.flat_reward) HIP_TRY(hipFree(e.flat_reward));
    e.flat_reward = nullptr;
    HIP_TRY(hipMalloc((void **)&e.flat_reward, (size_t)T * h->n_env * 4));
    e.flat_T = T;
    return ZENV_OK;
}

extern "C" int zenv_episode_log(zenv_t *h, zenv_episode_log_info *out)
{
    if (!h || !out) return fail(ZENV_E_ARG, "null argument");
    auto &e = h->eplog;
    if (!e.source || !h->exp_mem)
        return fail(ZENV_E_STATE, "zenv_episode_log follows a collection, once (no collection has run, the last one "
                                  "failed, or its log was already taken)");
    if (int rc = use_device(h)) return rc;
    if (int rc = ensure_state(h)) return rc;
    const int T = h->exp.T, N = h->n_env;
    EpLogWalk k{};
    k.T = T, k.N = N;
    k.mask = h->exp.mask, k.cur_mask = h->exp.cur_mask;
    for (int c = 0; c < 4; ++c) k.carry[c] = e.carry[c];
    int64_t columns = kAll;
    switch (e.source) {
    case 1:     // base.py:169-170: the env reward, self.rewards[i] (the shaped reward where the env reports one)
        k.resh = h->exp.reward;
        k.ret = h->goal_enabled || h->order_enabled ? e.flat_reward : h->exp.reward;
        break;
    case 2:     // zone-goals / options _hier_policy_opt.py: both sums take the env reward
    case 4:
        k.ret = k.resh = h->hframes.env_reward;
        break;
    case 3:     // main _hier_policy_opt.py:107-112
        k.ret = k.resh = h->sk.env_reward;
        k.div = h->sk.diversity;
        k.L = h->skill_len;
        columns |= (1 << ZENV_EPLOG_DIVERSITY) | (1 << ZENV_EPLOG_PREDICTION);
        break;
    default:    // xy-goals _hier_policy_opt.py
        k.ret = k.resh = h->xc.env_reward;
        k.L = h->skill_len;
        columns |= 1 << ZENV_EPLOG_PREDICTION;
        break;
    }
    if (!k.ret || !k.resh) return fail(ZENV_E_STATE, "the last collection left no reward record");
    const int64_t W = ((int64_t)N + 63) / 64, M = W * T;
    if (int rc = ensure_counts(h, M)) return rc;
    e.source = 0;                         // taken, however the call ends
    e.kept = -1;
    HIP_TRY(launch_eplog_count(k, e.counts, k.L > 0 ? e.active : nullptr, h->stream));
    HIP_TRY(launch_eplog_scan(e.counts, M, e.levels, e.totals, h->stream));
    if (k.L > 0) HIP_TRY(launch_eplog_scan(e.active, M, e.levels, e.totals + 1, h->stream));
    // D (and the active frames) to the host: the one synchronisation of the call
    int32_t totals[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(totals, e.totals, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int64_t D = totals[0], keep = std::max<int64_t>(D, N), head = keep - D;
    if (int rc = ensure_result(h, keep)) return rc;
    // the result = the last `keep` of (tail + new): the tail's last N - D entries when D < N, then the new entries
    const EpLogList &old_tail = e.tail[e.cur], &new_tail = e.tail[e.cur ^ 1];
    HIP_TRY(launch_eplog_copy(e.res, 0, old_tail, N - head, head, h->stream));
    HIP_TRY(launch_eplog_scatter(k, e.counts, e.res, head, h->stream));
    HIP_TRY(launch_eplog_copy(new_tail, 0, e.res, keep - N, N, h->stream));
    e.cur ^= 1;
    e.kept = keep;
    e.done = D;
    e.num_frames = k.L > 0 ? (int64_t)totals[1] : (int64_t)T * N;
    e.columns = columns;
    out->kept = e.kept, out->done = e.done, out->num_frames = e.num_frames, out->columns = e.columns;
    return ZENV_OK;
}

extern "C" int zenv_episode_log_tensor(zenv_t *h, int column, void **ptr, int64_t *count)
{
    if (!ptr || !count) return fail(ZENV_E_ARG, "null argument");
    if (int rc = column_ready(h, column, true)) return rc;
    *ptr = column_ptr(h, column);
    *count = h->eplog.kept;
    return ZENV_OK;
}

extern "C" int zenv_episode_log_read(zenv_t *h, int column, void *dst)
{
    if (!dst) return fail(ZENV_E_ARG, "null argument");
    if (int rc = column_ready(h, column, true)) return rc;
    HIP_TRY(hipMemcpyAsync(dst, column_ptr(h, column), (size_t)h->eplog.kept * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ZENV_OK;
}

extern "C" int zenv_episode_log_stats(zenv_t *h, int column, double out[5])
{
    if (!out) return fail(ZENV_E_ARG, "null argument");
    if (int rc = column_ready(h, column, false)) return rc;
    auto &e = h->eplog;
    HIP_TRY(launch_eplog_stats(e.res.col[column], e.kept, e.stat_ws, e.stat_fin, h->stream));
    double fin[6];
    HIP_TRY(hipMemcpyAsync(fin, e.stat_fin, sizeof fin, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    out[0] = (double)e.kept, out[1] = fin[0], out[2] = fin[3], out[3] = fin[1], out[4] = fin[2];
    return ZENV_OK;
}

extern "C" int zenv_episode_log_reset(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (int rc = use_device(h)) return rc;
    if (!h->eplog.state_mem) return ZENV_OK;       // nothing carried yet: already as a fresh object
    return zero_state(h);
}
