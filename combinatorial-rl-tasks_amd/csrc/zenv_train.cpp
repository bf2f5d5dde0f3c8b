// zenv_train.cpp -- the learner behind the C ABI of include/zenv.h: the flat actor-critic's PPO update on the handle's own
// experience buffers (zenv_ppo_*).  The kernels: ppo_update.hip.  The networks that act and collect: zenv_agents.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ppo_update.hpp"
#include "zenv_handle.hpp"

struct PpoState {
    PpoNet net{};
    void *arena_mem = nullptr;      // param | grad | exp_avg | exp_avg_sq
    void *ws_mem = nullptr;         // weight images, activations, partials
    int64_t step = 0;               // Adam's step count
    double lr = 0.0;
    int32_t *idx = nullptr;         // host indices, uploaded
    size_t idx_cap = 0;
    float *stats = nullptr;         // ZENV_F_PPO_STATS [stats_cap][6]
    int stats_cap = 0, stats_rows = 0;
};

namespace {

// element counts of the 20 tensors for hidden size h and zone rows of F features, zenv_mlp_weights' member order
void tensor_counts(int h, int F, int64_t (&count)[PPO_MAX_TENSORS])
{
    const int64_t hh = (int64_t)h * h;
    const int64_t c[PPO_MAX_TENSORS] = { (int64_t)h * (8 + F), h, hh, h, hh, h, (int64_t)h * (8 + h), h, hh, h, 2 * h, 2,
                                         2 * h, 2, hh, h, h, 1, h, 1 };
    std::copy(c, c + PPO_MAX_TENSORS, count);
}

void tensor_list(const zenv_mlp_weights *w, const float *(&t)[PPO_MAX_TENSORS])
{
    const float *l[PPO_MAX_TENSORS] = { w->zone_w1, w->zone_b1, w->zone_w2, w->zone_b2, w->zone_w3, w->zone_b3, w->comb_w,
                                        w->comb_b, w->enc_w, w->enc_b, w->mu_w, w->mu_b, w->std_w, w->std_b, w->critic_w1,
                                        w->critic_b1, w->critic_w2, w->critic_b2, w->critic_sigma_w, w->critic_sigma_b };
    std::copy(l, l + PPO_MAX_TENSORS, t);
}

struct Layout {
    int HP, KC, rp, bp;
    int64_t chunks;
    // floats of every workspace piece, in carving order
    int64_t img[PPO_N_IMAGES], a1, p, ci, pre, ss, partial;
    int64_t total;
};

Layout layout_for(int h, int Z, int max_batch)
{
    Layout l{};
    l.HP = (h + 32) / 32 * 32;          // h <= 191: at least one padded column, the constant's
    l.KC = l.HP + 8;
    const int64_t rp = ((int64_t)max_batch * Z + 31) / 32 * 32, bp = ((int64_t)max_batch + 31) / 32 * 32;
    l.rp = (int)std::min<int64_t>(rp, INT32_MAX);
    l.bp = (int)std::min<int64_t>(bp, INT32_MAX);
    l.chunks = (rp + kPpoChunk - 1) / kPpoChunk;
    const int64_t HP = l.HP, KC = l.KC;
    for (int i = 0; i < PPO_N_IMAGES; ++i) l.img[i] = HP * HP;
    l.img[PPO_I_W1] = HP * 16;
    l.img[PPO_I_WC] = HP * KC;
    l.img[PPO_I_HA] = l.img[PPO_I_HV] = 32 * HP;
    l.img[PPO_T_HA] = l.img[PPO_T_HV] = HP * 32;
    l.a1 = rp * HP;
    l.p = bp * HP;
    l.ci = bp * KC;
    l.pre = bp * 32;
    l.ss = bp * 8;
    l.partial = l.chunks * HP * (HP + 32);
    l.total = 2 * l.a1 + 4 * l.p + l.ci + 2 * l.pre + l.ss + l.partial;
    for (int i = 0; i < PPO_N_IMAGES; ++i) l.total += l.img[i];
    return l;
}

bool bad_hyper(double v) { return !std::isfinite(v) || v < 0.0; }

}  // namespace

extern "C" int zenv_ppo_check(const zenv_config *cfg, const zenv_mlp_weights *w, const zenv_ppo_config *pc)
{
    if (!cfg || !w || !pc) return fail(ZENV_E_ARG, "null argument");
    if (w->h_dim < 1 || w->h_dim > 191) return fail(ZENV_E_ARG, "h_dim %d outside [1, 191]", w->h_dim);
    if (cfg->num_zones < 1 || cfg->num_zones > ZENV_MAX_ZONES)
        return fail(ZENV_E_ARG, "num_zones %d outside [1, %d]", cfg->num_zones, ZENV_MAX_ZONES);
    const float *t[PPO_MAX_TENSORS];
    tensor_list(w, t);
    for (int i = 0; i < PPO_CRITIC_W1; ++i)
        if (!t[i]) return fail(ZENV_E_ARG, "zenv_mlp_weights has a null tensor");
    for (int i = PPO_CRITIC_W1; i <= PPO_CRITIC_B2; ++i)
        if (!t[i]) return fail(ZENV_E_ARG, "the update needs the critic: critic_w1 / _b1 / _w2 / _b2");
    const int n_sigma = (w->critic_sigma_w != nullptr) + (w->critic_sigma_b != nullptr);
    if (pc->distributional_value && n_sigma != 2)
        return fail(ZENV_E_ARG, "distributional_value needs critic_sigma_w and critic_sigma_b");
    if (!pc->distributional_value && n_sigma != 0)
        return fail(ZENV_E_ARG, "critic_sigma_* given without distributional_value");
    for (double v : { pc->lr, pc->adam_eps, pc->clip_eps, pc->entropy_coef, pc->value_loss_coef, pc->max_grad_norm })
        if (bad_hyper(v)) return fail(ZENV_E_ARG, "a hyper-parameter is negative or not finite (%g)", v);
    if (pc->max_batch < 1) return fail(ZENV_E_ARG, "max_batch must be >= 1");
    const Layout l = layout_for(w->h_dim, cfg->num_zones, pc->max_batch);
    if (l.total >= ((int64_t)1 << 31))
        return fail(ZENV_E_ARG, "max_batch %d x %d zones needs a workspace of %lld floats, the limit is 2^31: use smaller "
                    "minibatches", pc->max_batch, cfg->num_zones, (long long)l.total);
    return ZENV_OK;
}

void ppo_free(zenv *h)
{
    PpoState *s = h->ppo;
    if (!s) return;
    for (void *m : { s->arena_mem, s->ws_mem, (void *)s->idx, (void *)s->stats })
        if (m) (void)hipFree(m);
    if (s->net.bad_index) (void)hipHostFree(s->net.bad_index);
    delete s;
    h->ppo = nullptr;
}

int ppo_index_check(zenv *h)
{
    if (!h->ppo || !h->ppo->net.bad_index || !*(volatile int *)h->ppo->net.bad_index) return ZENV_OK;
    *(volatile int *)h->ppo->net.bad_index = 0;
    return fail(ZENV_E_ARG, "a device-resident minibatch index lay outside [0, envs x frames): its sample was dropped and "
                            "the update since the last synchronising call is invalid");
}

void *ppo_stats(const zenv *h, int64_t *bytes)
{
    *bytes = h->ppo ? (int64_t)h->ppo->stats_rows * kPpoStats * 4 : 0;
    return h->ppo ? h->ppo->stats : nullptr;
}

extern "C" int zenv_ppo_init(zenv_t *h, const zenv_mlp_weights *w, const zenv_ppo_config *pc)
{
    if (!h || !w || !pc) return fail(ZENV_E_ARG, "null argument");
    if (int rc = zenv_ppo_check(&h->cfg, w, pc)) return rc;
    if (int rc = use_device(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    ppo_free(h);
    PpoState *s = new PpoState();
    h->ppo = s;
    PpoNet &n = s->net;
    const Layout l = layout_for(w->h_dim, h->p.Z, pc->max_batch);
    n.h = w->h_dim, n.HP = l.HP, n.F = h->p.F, n.Z = h->p.Z, n.K1 = 8 + h->p.F, n.KC = l.KC;
    n.dist = pc->distributional_value ? 1 : 0;
    n.n_tensors = n.dist ? 20 : 18;
    n.max_batch = pc->max_batch;
    s->lr = pc->lr;
    n.hyper = PpoHyper{ (float)pc->lr, (float)pc->adam_eps, (float)pc->clip_eps, (float)pc->entropy_coef,
                        (float)pc->value_loss_coef, (float)pc->max_grad_norm };
    tensor_counts(n.h, n.F, n.count);
    int64_t at = 0;
    for (int i = 0; i < PPO_MAX_TENSORS; ++i) {         // every tensor starts on a 256-byte boundary
        n.off[i] = at;
        if (i < n.n_tensors) at += (n.count[i] + 63) / 64 * 64;
        else n.count[i] = 0;
    }
    n.arena = at;
    // ---- the four arenas
    std::vector<float> host((size_t)n.arena, 0.f);
    const float *t[PPO_MAX_TENSORS];
    tensor_list(w, t);
    for (int i = 0; i < n.n_tensors; ++i) std::memcpy(host.data() + n.off[i], t[i], (size_t)n.count[i] * sizeof(float));
    const size_t arena_bytes = (size_t)n.arena * sizeof(float);
    HIP_TRY(hipMalloc(&s->arena_mem, 4 * arena_bytes));
    n.param = static_cast<float *>(s->arena_mem);
    n.grad = n.param + n.arena, n.exp_avg = n.grad + n.arena, n.exp_avg_sq = n.exp_avg + n.arena;
    HIP_TRY(hipMemset(s->arena_mem, 0, 4 * arena_bytes));
    HIP_TRY(hipMemcpy(n.param, host.data(), arena_bytes, hipMemcpyHostToDevice));
    // ---- the workspace, carved in layout_for's order; every piece a multiple of 32 floats
    const int norm_parts = (int)((n.arena + kPpoNormBlock - 1) / kPpoNormBlock);
    const size_t ws_bytes = (size_t)l.total * sizeof(float) + (size_t)(norm_parts + 1) * sizeof(double) + 256;
    HIP_TRY(hipMalloc(&s->ws_mem, ws_bytes));
    HIP_TRY(hipMemset(s->ws_mem, 0, ws_bytes));
    float *f = static_cast<float *>(s->ws_mem);
    auto take = [&f](int64_t count) { float *p = f; f += count; return p; };
    for (int i = 0; i < PPO_N_IMAGES; ++i) n.img[i] = take(l.img[i]);
    n.A1 = take(l.a1), n.A2 = take(l.a1);
    n.P = take(l.p), n.C = take(l.p), n.Ha = take(l.p), n.Hc = take(l.p);
    n.CI = take(l.ci);
    n.PRE = take(l.pre), n.DH = take(l.pre);
    n.SS = take(l.ss);
    n.partial = take(l.partial);
    n.norm_partial = reinterpret_cast<double *>(f);      // l.total is a multiple of 8 floats: 8-byte aligned
    n.scalars = reinterpret_cast<float *>(n.norm_partial + norm_parts + 1);
    HIP_TRY(hipHostMalloc((void **)&n.bad_index, sizeof(int), hipHostMallocDefault));
    *n.bad_index = 0;
    s->stats_cap = 64;
    HIP_TRY(hipMalloc((void **)&s->stats, (size_t)s->stats_cap * kPpoStats * sizeof(float)));
    HIP_TRY(hipMemset(s->stats, 0, (size_t)s->stats_cap * kPpoStats * sizeof(float)));
    return ZENV_OK;
}

extern "C" int zenv_ppo_tensor(zenv_t *h, int which, int index, void **dev_ptr, int64_t *count)
{
    if (!h || !dev_ptr || !count) return fail(ZENV_E_ARG, "null argument");
    if (!h->ppo) return fail(ZENV_E_STATE, "zenv_ppo_init first");
    const PpoNet &n = h->ppo->net;
    if (which < ZENV_PPO_PARAM || which > ZENV_PPO_EXP_AVG_SQ) return fail(ZENV_E_ARG, "unknown arena %d", which);
    if (index < -1 || index >= n.n_tensors) return fail(ZENV_E_ARG, "tensor index %d outside [-1, %d)", index, n.n_tensors);
    float *base = n.param + (int64_t)which * n.arena;
    *dev_ptr = index < 0 ? base : base + n.off[index];
    *count = index < 0 ? n.arena : n.count[index];
    return ZENV_OK;
}

// a tensor (or, index = -1, a whole arena) to or from host memory, behind everything enqueued; both wait for the copy
static int ppo_copy(zenv_t *h, int which, int index, void *host, bool to_host)
{
    if (!host) return fail(ZENV_E_ARG, "null argument");
    void *dev = nullptr;
    int64_t count = 0;
    if (int rc = zenv_ppo_tensor(h, which, index, &dev, &count)) return rc;
    if (int rc = use_device(h)) return rc;
    if (to_host) HIP_TRY(hipMemcpyAsync(host, dev, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream));
    else HIP_TRY(hipMemcpyAsync(dev, host, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return mlp_range_check(h);
}

extern "C" int zenv_ppo_read(zenv_t *h, int which, int index, float *dst) { return ppo_copy(h, which, index, dst, true); }

extern "C" int zenv_ppo_write(zenv_t *h, int which, int index, const float *src)
{
    return ppo_copy(h, which, index, const_cast<float *>(src), false);
}

extern "C" int zenv_ppo_get_step(zenv_t *h, int64_t *step)
{
    if (!h || !step) return fail(ZENV_E_ARG, "null argument");
    if (!h->ppo) return fail(ZENV_E_STATE, "zenv_ppo_init first");
    *step = h->ppo->step;
    return ZENV_OK;
}

extern "C" int zenv_ppo_set_step(zenv_t *h, int64_t step)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->ppo) return fail(ZENV_E_STATE, "zenv_ppo_init first");
    if (step < 0) return fail(ZENV_E_ARG, "the step count must be >= 0");
    h->ppo->step = step;
    return ZENV_OK;
}

namespace {

// the checks every update call shares; *idx_dev: the indices on the device
int ppo_indices(zenv *h, const int32_t *idx, int total, int on_device, const int32_t **idx_dev)
{
    PpoState *s = h->ppo;
    if (!h->exp_mem) return fail(ZENV_E_STATE, "zenv_collect first: the handle holds no experience");
    if (int rc = use_device(h)) return rc;
    if (on_device) {
        *idx_dev = idx;
        return ZENV_OK;
    }
    const int64_t frames = (int64_t)h->n_env * h->exp.T;
    for (int i = 0; i < total; ++i)
        if (idx[i] < 0 || idx[i] >= frames)
            return fail(ZENV_E_ARG, "index %d (at %d) outside [0, %lld)", idx[i], i, (long long)frames);
    if (s->idx_cap < (size_t)total) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (s->idx) HIP_TRY(hipFree(s->idx));
        s->idx = nullptr, s->idx_cap = 0;
        HIP_TRY(hipMalloc((void **)&s->idx, (size_t)total * sizeof(int32_t)));
        s->idx_cap = (size_t)total;
    }
    HIP_TRY(hipMemcpyAsync(s->idx, idx, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    *idx_dev = s->idx;
    return ZENV_OK;
}

int ppo_stats_rows(zenv *h, int rows)
{
    PpoState *s = h->ppo;
    if (rows > s->stats_cap) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipFree(s->stats));
        s->stats = nullptr, s->stats_cap = 0, s->stats_rows = 0;
        HIP_TRY(hipMalloc((void **)&s->stats, (size_t)rows * kPpoStats * sizeof(float)));
        s->stats_cap = rows;
    }
    s->stats_rows = rows;
    return ZENV_OK;
}

PpoExp exp_of(const zenv *h)
{
    const ExpBuffers &x = h->exp;
    return PpoExp{ x.obs, x.zone_obs, x.action, x.log_prob, x.value, x.advantage, x.returnn, h->n_env, x.T };
}

int ppo_step(zenv *h)
{
    PpoState *s = h->ppo;
    s->step += 1;
    // torch.optim.Adam forms these in Python floats: step_size = lr / (1 - beta1^t), sqrt(1 - beta2^t)
    const double bc1 = 1.0 - std::pow(0.9, (double)s->step), bc2 = 1.0 - std::pow(0.999, (double)s->step);
    HIP_TRY(launch_ppo_apply(s->net, (float)(s->lr / bc1), (float)std::sqrt(bc2), h->stream));
    return ZENV_OK;
}

}  // namespace

extern "C" int zenv_ppo_minibatch(zenv_t *h, const int32_t *idx, int count, int idx_on_device, int apply)
{
    if (!h || !idx) return fail(ZENV_E_ARG, "null argument");
    if (!h->ppo) return fail(ZENV_E_STATE, "zenv_ppo_init first");
    if (count < 1 || count > h->ppo->net.max_batch)
        return fail(ZENV_E_ARG, "count %d outside [1, max_batch = %d]", count, h->ppo->net.max_batch);
    const int32_t *idx_dev = nullptr;
    if (int rc = ppo_indices(h, idx, count, idx_on_device, &idx_dev)) return rc;
    if (int rc = ppo_stats_rows(h, 1)) return rc;
    HIP_TRY(launch_ppo_minibatch(h->ppo->net, exp_of(h), idx_dev, count, h->ppo->stats, h->stream));
    return apply ? ppo_step(h) : ZENV_OK;
}

extern "C" int zenv_ppo_apply(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->ppo) return fail(ZENV_E_STATE, "zenv_ppo_init first");
    if (int rc = use_device(h)) return rc;
    return ppo_step(h);
}

extern "C" int zenv_ppo_epoch(zenv_t *h, const int32_t *order, int total, int batch_size, int on_device)
{
    if (!h || !order) return fail(ZENV_E_ARG, "null argument");
    if (!h->ppo) return fail(ZENV_E_STATE, "zenv_ppo_init first");
    if (total < 1) return fail(ZENV_E_ARG, "total must be >= 1");
    if (batch_size < 1 || batch_size > h->ppo->net.max_batch)
        return fail(ZENV_E_ARG, "batch_size %d outside [1, max_batch = %d]", batch_size, h->ppo->net.max_batch);
    const int32_t *idx_dev = nullptr;
    if (int rc = ppo_indices(h, order, total, on_device, &idx_dev)) return rc;
    const int n_mb = (total + batch_size - 1) / batch_size;
    if (int rc = ppo_stats_rows(h, n_mb)) return rc;
    for (int k = 0; k < n_mb; ++k) {
        const int lo = k * batch_size, count = std::min(batch_size, total - lo);
        HIP_TRY(launch_ppo_minibatch(h->ppo->net, exp_of(h), idx_dev + lo, count, h->ppo->stats + (size_t)k * kPpoStats,
                                     h->stream));
        if (int rc = ppo_step(h)) return rc;
    }
    return ZENV_OK;
}
