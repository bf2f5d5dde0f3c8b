// zenv_agents.cpp -- the networks behind the C ABI of include/zenv.h: the loaders, forwards and per-step policies of the
// flat actor and of the Zone-goals, fixed-length-skills / DIAYN, Options and xy-goals agents, and the five collectors
// (zenv_collect, zenv_collect_hier, zenv_collect_skill, zenv_collect_option, zenv_collect_xy).  The handle and the environment's own calls: zenv_api.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "zenv_handle.hpp"

namespace {

// the actor tensors of a two-level agent all there, each critic as its four tensors or not at all
int check_tensors(std::initializer_list<const float *> actor, std::initializer_list<const float *> hi_critic,
                  std::initializer_list<const float *> lo_critic)
{
    for (const float *t : actor)
        if (!t) return fail(ZENV_E_ARG, "the weights have a null actor tensor");
    for (const auto &critic : { hi_critic, lo_critic }) {
        const size_t n = critic.size() - (size_t)std::count(critic.begin(), critic.end(), nullptr);
        if (n != 0 && n != critic.size()) return fail(ZENV_E_ARG, "give all four tensors of a critic or none");
    }
    return ZENV_OK;
}

// A new weight image in place of `mem`: the stream drained (a kernel in flight may read the old one), the old one freed
// (the size changes with the critics), the new one uploaded
int replace_image(zenv *h, void *&mem, const void *src, size_t bytes)
{
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (mem) HIP_TRY(hipFree(mem));
    mem = nullptr;
    HIP_TRY(hipMalloc(&mem, bytes));
    HIP_TRY(hipMemcpy(mem, src, bytes, hipMemcpyHostToDevice));
    return ZENV_OK;
}

// ZENV_F_POLICY_MU / _STD / _VALUE: the flat network and every agent's low level write them, whichever loads first
// allocates them
int ensure_policy_outputs(zenv *h)
{
    const size_t N = (size_t)h->n_env;
    if (!h->mlp_value) HIP_TRY(hipMalloc((void **)&h->mlp_value, N * sizeof(float)));
    if (!h->mlp_mu) HIP_TRY(hipMalloc((void **)&h->mlp_mu, N * 2 * sizeof(float)));
    if (!h->mlp_std) HIP_TRY(hipMalloc((void **)&h->mlp_std, N * 2 * sizeof(float)));
    return ZENV_OK;
}

// One device allocation carved into 256-byte aligned pieces, in the order they are asked for: piece() notes where each
// pointer will land, alloc() sizes the allocation from the pieces and sets the pointers.
class Carver {
    std::vector<std::pair<void **, size_t>> pieces_;     // (the pointer to set, its offset)
    size_t total_ = 0;
    bool overflow_ = false;

public:
    template <typename T>
    void piece(T *&slot, size_t count)
    {
        if (count > (SIZE_MAX - 255 - total_) / sizeof(T)) overflow_ = true;
        pieces_.push_back({ reinterpret_cast<void **>(&slot), total_ });
        total_ += (count * sizeof(T) + 255) & ~(size_t)255;
    }
    size_t bytes() const { return total_; }
    int alloc(void **mem, const char *what)
    {
        if (overflow_) return fail(ZENV_E_HIP, "%s layout overflow", what);
        HIP_TRY(hipMalloc(mem, total_));
        for (const auto &p : pieces_) *p.first = static_cast<char *>(*mem) + p.second;
        return ZENV_OK;
    }
};

}  // namespace

// ZENV_MLP_F16X3: the network kernel sets *mlp_range_flag (pinned host memory) when one of its operands left float16's
// range; every entry point that waits for the device looks at it once the stream has drained
int mlp_range_check(zenv *h)
{
    if (int rc = ppo_index_check(h)) return rc;
    if (!h->mlp_range_flag || !*(volatile int *)h->mlp_range_flag) return ZENV_OK;
    *(volatile int *)h->mlp_range_flag = 0;
    return fail(ZENV_E_RANGE, "an input or activation of the network reached 65 520, beyond float16 (ZENV_MLP_F16: or an "
                              "observation beyond 64): the actions since the last synchronising call are invalid -- load these "
                              "weights with ZENV_MLP_BF16, ZENV_MLP_BF16X3 or ZENV_MLP_F32");
}

// ============================================================================ actor network
extern "C" int zenv_mlp_load(zenv_t *h, const zenv_mlp_weights *w)
{
    if (!h || !w) return fail(ZENV_E_ARG, "null argument");
    for (const float *t : { w->zone_w1, w->zone_b1, w->zone_w2, w->zone_b2, w->zone_w3, w->zone_b3, w->comb_w, w->comb_b,
                            w->enc_w, w->enc_b, w->mu_w, w->mu_b, w->std_w, w->std_b })
        if (!t) return fail(ZENV_E_ARG, "zenv_mlp_weights has a null tensor");
    const int n_critic = (w->critic_w1 != nullptr) + (w->critic_b1 != nullptr) + (w->critic_w2 != nullptr) +
                         (w->critic_b2 != nullptr);
    if (n_critic != 0 && n_critic != 4) return fail(ZENV_E_ARG, "give all four critic tensors or none");
    const int n_sigma = (w->critic_sigma_w != nullptr) + (w->critic_sigma_b != nullptr);
    if (n_sigma == 1 || (n_sigma == 2 && n_critic == 0))
        return fail(ZENV_E_ARG, "the distributional critic needs critic.0, critic_mu (as critic_w2 / _b2) and critic_sigma");
    if (w->precision < ZENV_MLP_BF16 || w->precision > ZENV_MLP_F16)
        return fail(ZENV_E_ARG, "unknown zenv_mlp_weights.precision %d", w->precision);
    const bool f16 = w->precision == ZENV_MLP_F16;
    if ((f16 || w->precision == ZENV_MLP_F16X3) && w->h_dim >= 1 && w->h_dim < kMlpHP) {
        // ZENV_MLP_F16, single float16 operands: (i) every weight must be a finite float16 (zone_net_.4 and combine_net_
        // are looked at below, folded); (ii) the zone layers' activations are bounded here, over the rows' absolute sums,
        // for observations up to kMlpF16ObsBound and zone rows up to 2 (positions / 3, flags, timers: bounded by
        // construction) -- the zone kernel has no cycles to spare for watching them; the head kernel watches its own.
        // ZENV_MLP_F16X3, float16 halves: a weight of 65 520 or more would be inf on the device.
        const int hd = w->h_dim, F = net_row_feat(h);     // (zenv_order_rows: the order value lies in [0, 1], inside the rows' bound of 2)
        const struct { const float *t; size_t n; const char *name; bool folded; } all[] = {
            { w->zone_w1, (size_t)hd * (8 + F), "zone_net_.0.weight", 0 }, { w->zone_b1, (size_t)hd, "zone_net_.0.bias", 0 },
            { w->zone_w2, (size_t)hd * hd, "zone_net_.2.weight", 0 },      { w->zone_b2, (size_t)hd, "zone_net_.2.bias", 0 },
            { w->zone_w3, (size_t)hd * hd, "zone_net_.4.weight", 1 },      { w->zone_b3, (size_t)hd, "zone_net_.4.bias", 1 },
            { w->comb_w, (size_t)hd * (8 + hd), "combine_net_.weight", 1 }, { w->comb_b, (size_t)hd, "combine_net_.bias", 1 },
            { w->enc_w, (size_t)hd * hd, "actor.enc_.0.0.weight", 0 },     { w->enc_b, (size_t)hd, "actor.enc_.0.0.bias", 0 },
            { w->mu_w, (size_t)2 * hd, "actor.mu_.weight", 0 },            { w->mu_b, 2, "actor.mu_.bias", 0 },
            { w->std_w, (size_t)2 * hd, "actor.std_.weight", 0 },          { w->std_b, 2, "actor.std_.bias", 0 },
            { w->critic_w1, (size_t)hd * hd, "critic.0.weight", 0 },       { w->critic_b1, (size_t)hd, "critic.0.bias", 0 },
            { w->critic_w2, (size_t)hd, "critic.2.weight", 0 },            { w->critic_b2, 1, "critic.2.bias", 0 },
            { w->critic_sigma_w, (size_t)hd, "critic_sigma.weight", 0 },   { w->critic_sigma_b, 1, "critic_sigma.bias", 0 } };
        const float limit = f16 ? 65504.0f : 32768.0f;
        for (const auto &a : all)
            for (size_t i = 0; a.t && !(f16 && a.folded) && i < a.n; ++i)
                if (!(std::fabs(a.t[i]) < limit))
                    return f16 ? fail(ZENV_E_RANGE, "%s[%zu] = %g is not a finite float16: use ZENV_MLP_BF16 or a split mode",
                                      a.name, i, (double)a.t[i])
                               : fail(ZENV_E_RANGE, "%s[%zu] = %g: ZENV_MLP_F16X3 keeps weights as float16 pairs (|w| < 32 768); "
                                                    "use ZENV_MLP_BF16X3 or ZENV_MLP_F32", a.name, i, (double)a.t[i]);
        double a1 = 0.0, s2 = 0.0, b2 = 0.0;                   // (ii), ZENV_MLP_F16 only
        for (int r = 0; f16 && r < hd; ++r) {
            double v = std::fabs((double)w->zone_b1[r]), s = 0.0;
            for (int k = 0; k < 8 + F; ++k)
                v += std::fabs((double)w->zone_w1[(size_t)r * (8 + F) + k]) * (k < 8 ? (double)kMlpF16ObsBound : 2.0);
            a1 = std::max(a1, v);
            for (int k = 0; k < hd; ++k) s += std::fabs((double)w->zone_w2[(size_t)r * hd + k]);
            s2 = std::max(s2, s);
            b2 = std::max(b2, std::fabs((double)w->zone_b2[r]));
        }
        if (!(a1 < 65504.0) || !(s2 * a1 + b2 < 65504.0))
            return fail(ZENV_E_RANGE, "zone_net_'s activations are bounded by %.3g / %.3g for observations up to %g: beyond "
                                      "float16 -- use ZENV_MLP_BF16 or a split mode for these weights",
                        a1, s2 * a1 + b2, (double)kMlpF16ObsBound);
    }
    std::vector<uint16_t> img;
    size_t offs[8];
    if (pack_images(*w, net_row_feat(h), img, offs, w->precision == ZENV_MLP_F16) != 0)
        return fail(ZENV_E_ARG, "h_dim %d outside [1, %d]", w->h_dim, kMlpHP - 1);
    if (w->precision == ZENV_MLP_F16)        // zone_net_.4 folded into combine_net_: a product that can leave the range
        for (size_t i = 0; i < img.size(); ++i)
            if ((img[i] & 0x7C00u) == 0x7C00u)
                return fail(ZENV_E_RANGE, "combine_net_ folded over zone_net_.4 leaves float16's range: use ZENV_MLP_BF16 or "
                                          "a split mode for these weights");
    std::vector<float> f32;         // the float32-grade modes' images (packed before the handle is touched: it can refuse)
    size_t fo[30];
    const bool f32_grade = w->precision != ZENV_MLP_BF16 && w->precision != ZENV_MLP_F16;
    if (f32_grade) {
        pack_f32(*w, net_row_feat(h), f32, fo);
        if (w->precision == ZENV_MLP_F16X3) {
            // the float16 images start at fo[24] (zone_net_.2): combine_net_ arrives with zone_net_.4 folded in, a product of
            // two in-range matrices that need not be in range itself
            const uint16_t *hw = reinterpret_cast<const uint16_t *>(f32.data() + fo[24]);
            const size_t n16 = (f32.size() - fo[24]) * 2;
            for (size_t i = 0; i < n16; ++i)
                if ((hw[i] & 0x7C00u) == 0x7C00u)
                    return fail(ZENV_E_RANGE, "combine_net_ folded over zone_net_.4 leaves float16's range: use ZENV_MLP_BF16X3 "
                                              "or ZENV_MLP_F32 for these weights");
        }
    }
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env;
    h->mlp_ready = false;
    if (int rc = replace_image(h, h->mlp_mem, img.data(), img.size() * 2)) return rc;
    if (h->mlp_f32_mem) HIP_TRY(hipFree(h->mlp_f32_mem));
    h->mlp_f32_mem = nullptr;
    if (int rc = ensure_policy_outputs(h)) return rc;
    HIP_TRY(hipMemsetAsync(h->mlp_value, 0, N * sizeof(float), h->stream));
    if (!h->mlp_value_sigma) HIP_TRY(hipMalloc((void **)&h->mlp_value_sigma, N * sizeof(float)));
    HIP_TRY(hipMemsetAsync(h->mlp_value_sigma, 0, N * sizeof(float), h->stream));
    if (!h->mlp_pooled) HIP_TRY(hipMalloc(&h->mlp_pooled, N * kMlpHP * sizeof(uint16_t)));
    const char *base = static_cast<const char *>(h->mlp_mem);
    h->mlp = MlpImages{ base + offs[0], base + offs[1], base + offs[2], base + offs[3], base + offs[4], base + offs[5],
                        n_critic ? base + offs[6] : nullptr, n_critic ? base + offs[7] : nullptr, nullptr,
                        n_sigma == 2 ? 1 : 0, 0, nullptr };
    if (w->precision != ZENV_MLP_BF16 && !h->mlp_range_flag) {
        HIP_TRY(hipHostMalloc((void **)&h->mlp_range_flag, sizeof(int), hipHostMallocDefault));
        *h->mlp_range_flag = 0;
    }
    if (w->precision == ZENV_MLP_F16) {
        h->mlp.elem_f16 = 1;
        h->mlp.range_flag = h->mlp_range_flag;
    }
    if (f32_grade) {
        // (diagnostic: ZENV_MLP_F32_VALU=1 runs the network on the vector ALU, k_mlp_f32, instead of the f32 MFMA)
        // ZENV_MLP_F32_MFMA=1 the MFMA kernel whatever the batch; default: by batch size, see launch_mlp_forward_f32)
        const int on_mfma = std::getenv("ZENV_MLP_F32_VALU") ? 0 : std::getenv("ZENV_MLP_F32_MFMA") ? 2 : 1;
        if (int rc = replace_image(h, h->mlp_f32_mem, f32.data(), f32.size() * sizeof(float))) return rc;
        const float *fb = static_cast<const float *>(h->mlp_f32_mem);
        h->mlp_f32 = MlpF32{ w->h_dim, n_sigma == 2 ? 1 : 0, n_critic ? 1 : 0, 0,
                             fb + fo[0], fb + fo[1], fb + fo[2], fb + fo[3], fb + fo[4], fb + fo[5], fb + fo[6],
                             fb + fo[7], fb + fo[8], fb + fo[9], n_critic ? fb + fo[10] : nullptr,
                             n_critic ? fb + fo[11] : nullptr, fb + fo[12], fb + fo[13], fb + fo[14], fb + fo[15], fb + fo[16], fb + fo[17], fb + fo[18],
                             n_critic ? fb + fo[19] : nullptr, n_critic ? fb + fo[20] : nullptr, on_mfma,
                             w->precision == ZENV_MLP_BF16X3 ? 1 : w->precision == ZENV_MLP_F16X3 ? 2 : 0,
                             fb + fo[21], fb + fo[22], fb + fo[23], fb + fo[24], fb + fo[25],
                             n_critic ? fb + fo[26] : nullptr, fb + fo[27], fb + fo[28], n_critic ? fb + fo[29] : nullptr,
                             h->mlp_range_flag };
        h->mlp.f32 = &h->mlp_f32;
    }
    h->mlp_ready = true;
    return ZENV_OK;
}

// The zone rows the flat network reads: the observation's own, or with zenv_order_rows on the (Z, 7) rows that
// k_order_rows (K22) assembles into `dst` (null: ZENV_F_ORDER_ROWS) from the handle's 6-wide rows and the order value as
// they stand.  Launched here, where a network is about to read them: a caller that never asks a network pays nothing.
static int network_rows(zenv *h, float *dst, const float **rows)
{
    *rows = h->p.zone_obs;
    if (!h->net_feat) return ZENV_OK;
    if (!dst) dst = h->order_rows;
    HIP_TRY(launch_order_rows(h->p.zone_obs, h->p.order_val, dst, (int64_t)h->n_env * h->p.Z, h->stream));
    *rows = dst;
    return ZENV_OK;
}

// the flat network on the current observation: `act` says what the head kernel does with (mu, std)
static int flat_forward(zenv *h, const MlpAction &act, float *rows_dst = nullptr)
{
    const float *rows = nullptr;
    if (int rc = network_rows(h, rows_dst, &rows)) return rc;
    HIP_TRY(launch_mlp_forward(h->mlp, h->n_env, h->p.Z, net_row_feat(h), h->p.obs, rows, h->mlp_pooled, h->mlp_mu,
                               h->mlp_std, h->mlp_value, h->mlp_value_sigma, act, h->stream));
    return ZENV_OK;
}

extern "C" int zenv_mlp_forward(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->mlp_ready) return fail(ZENV_E_STATE, "zenv_mlp_load first");
    if (!h->was_reset) return fail(ZENV_E_STATE, "reset before asking for actions");
    if (int rc = use_device(h)) return rc;
    return flat_forward(h, no_mlp_action());
}

// zenv_order_rows toggled: what is sized by the network row width goes, and callers load it again
int drop_flat_network(zenv *h)
{
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->mlp_ready = false;
    for (void **m : { &h->mlp_mem, &h->mlp_f32_mem, &h->exp_mem })
        if (*m) {
            HIP_TRY(hipFree(*m));
            *m = nullptr;
        }
    h->mlp = MlpImages{};
    h->exp = ExpBuffers{};
    h->exp_hier = h->exp_xy = h->exp_skill = h->exp_option = false;
    h->diayn_kept = -1;
    h->eplog.source = 0;
    ppo_free_flat(h);
    return ZENV_OK;
}

// ============================================================================ Zone-goals hierarchical agent
extern "C" int zenv_hier_load(zenv_t *h, const zenv_hier_weights *w)
{
    if (!h || !w) return fail(ZENV_E_ARG, "null argument");
    if (!h->goal_enabled) return fail(ZENV_E_STATE, "the hierarchical agent sets goals: zenv_goal_enable first");
    if (w->h_dim < 1 || w->h_dim >= kMlpHP) return fail(ZENV_E_ARG, "h_dim %d outside 1 .. %d", w->h_dim, kMlpHP - 1);
    if (w->precision != ZENV_MLP_F32)
        return fail(ZENV_E_ARG, "zenv_hier_weights.precision %d: only ZENV_MLP_F32 is built", w->precision);
    if (w->zone_feat != h->p.F)
        return fail(ZENV_E_ARG, "the weights take zone rows of %d features, this handle's have %d", w->zone_feat, h->p.F);
    int rc = check_tensors({ w->hi_zone_w1, w->hi_zone_b1, w->hi_zone_w2, w->hi_zone_b2, w->hi_zone_w3, w->hi_zone_b3,
                             w->hi_comb_w, w->hi_comb_b, w->hi_actor_w1, w->hi_actor_b1, w->hi_actor_w2, w->hi_actor_b2,
                             w->lo_zone_w1, w->lo_zone_b1, w->lo_zone_w2, w->lo_zone_b2, w->lo_zone_w3, w->lo_zone_b3,
                             w->lo_comb_w, w->lo_comb_b, w->lo_enc_w, w->lo_enc_b, w->lo_mu_w, w->lo_mu_b, w->lo_std_w,
                             w->lo_std_b },
                           { w->hi_critic_w1, w->hi_critic_b1, w->hi_critic_w2, w->hi_critic_b2 },
                           { w->lo_critic_w1, w->lo_critic_b1, w->lo_critic_w2, w->lo_critic_b2 });
    if (rc) return rc;
    std::vector<float> img;
    size_t o[kHierOffs];
    pack_hier_f32(*w, h->p.F, img, o);
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env;
    h->hier_ready = false;
    if (int rc = replace_image(h, h->hier_mem, img.data(), img.size() * sizeof(float))) return rc;
    if (int rc = ensure_policy_outputs(h)) return rc;
    if (!h->hier_logits) HIP_TRY(hipMalloc((void **)&h->hier_logits, N * h->p.Z * sizeof(float)));
    if (!h->hier_value) HIP_TRY(hipMalloc((void **)&h->hier_value, N * sizeof(float)));
    HIP_TRY(hipMemsetAsync(h->hier_logits, 0, N * h->p.Z * sizeof(float), h->stream));
    HIP_TRY(hipMemsetAsync(h->hier_value, 0, N * sizeof(float), h->stream));
    h->hier = hier_f32_at(*w, static_cast<const float *>(h->hier_mem), o);
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->hier_ready = true;
    return ZENV_OK;
}

extern "C" int zenv_hier_forward(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->hier_ready) return fail(ZENV_E_STATE, "zenv_hier_load first");
    if (!h->was_reset) return fail(ZENV_E_STATE, "reset before asking for actions");
    if (int rc = use_device(h)) return rc;
    const HierPick none{ -1, 0u, 0ull, 0ull, nullptr };
    HIP_TRY(launch_hier_high(h->hier, h->p, h->hier_logits, h->hier_value, none, h->stream));
    HIP_TRY(launch_hier_low(h->hier, h->p, h->mlp_mu, h->mlp_std, h->mlp_value, no_mlp_action(), h->stream));
    return ZENV_OK;
}

// one step of evaluate_zone_hrl.py:56-64: goals for the envs that need one (through launch_goal_set, the path of
// zenv_set_goals), then the low level's action of every env into `out`
static int run_hier_policy(zenv_t *h, int policy, uint32_t step_index, uint64_t seed, uint64_t env_index0, float *out)
{
    if (!h->hier_ready) return fail(ZENV_E_STATE, "zenv_hier_load first");
    const int mode = policy == ZENV_POLICY_HIER_SAMPLE ? 1 : 0;
    const HierPick pick{ mode, step_index, seed, env_index0, h->goal_in };
    HIP_TRY(launch_hier_high(h->hier, h->p, h->hier_logits, h->hier_value, pick, h->stream));
    HIP_TRY(launch_goal_set(h->p, h->goal_in, h->goal_bad, h->stream));
    const MlpAction act{ mode, step_index, seed, env_index0, out, MlpRecord{} };
    HIP_TRY(launch_hier_low(h->hier, h->p, h->mlp_mu, h->mlp_std, h->mlp_value, act, h->stream));
    return ZENV_OK;
}

// ============================================================================ fixed-length-skills agent
// zenv_skill_load (n_out = 2) and zenv_option_load (n_out = 3: the rows of lo_mu_w / lo_std_w)
static int load_skill_family(zenv_t *h, const zenv_skill_weights *w, int n_out)
{
    if (h->goal_enabled || h->order_enabled)
        return fail(ZENV_E_STATE, "the skill agent steps a plain task handle, not a goal-conditioned / solver-ordered one");
    if (w->h_dim < 1 || w->h_dim >= kMlpHP) return fail(ZENV_E_ARG, "h_dim %d outside 1 .. %d", w->h_dim, kMlpHP - 1);
    if (w->n_skills < 1 || w->n_skills > kMaxSkills)
        return fail(ZENV_E_ARG, "n_skills %d outside 1 .. %d", w->n_skills, kMaxSkills);
    if (w->precision != ZENV_MLP_F32)
        return fail(ZENV_E_ARG, "zenv_skill_weights.precision %d: only ZENV_MLP_F32 is built", w->precision);
    if (w->zone_feat != h->p.F)
        return fail(ZENV_E_ARG, "the weights take zone rows of %d features, this handle's have %d", w->zone_feat, h->p.F);
    int rc = check_tensors({ w->hi_zone_w1, w->hi_zone_b1, w->hi_zone_w2, w->hi_zone_b2, w->hi_zone_w3, w->hi_zone_b3,
                             w->hi_comb_w, w->hi_comb_b, w->hi_enc_w, w->hi_enc_b, w->hi_logit_w, w->hi_logit_b,
                             w->lo_zone_w1, w->lo_zone_b1, w->lo_zone_w2, w->lo_zone_b2, w->lo_zone_w3, w->lo_zone_b3,
                             w->lo_comb_w, w->lo_comb_b, w->lo_enc_w, w->lo_enc_b, w->lo_mu_w, w->lo_mu_b, w->lo_std_w,
                             w->lo_std_b },
                           { w->hi_critic_w1, w->hi_critic_b1, w->hi_critic_w2, w->hi_critic_b2 },
                           { w->lo_critic_w1, w->lo_critic_b1, w->lo_critic_w2, w->lo_critic_b2 });
    if (rc) return rc;
    std::vector<float> img;
    size_t o[kSkillPtrs];
    pack_skill_f32(*w, h->p.F, img, o, n_out);
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env, S = (size_t)w->n_skills;
    h->skill_ready = h->option_ready = h->xy_ready = false;     // a handle holds one agent on the skill state's clock
    if (int rc = replace_image(h, h->skill_mem, img.data(), img.size() * sizeof(float))) return rc;
    if (int rc = ensure_policy_outputs(h)) return rc;
    if (h->skill_logits && h->skill_n != (int)S) {
        HIP_TRY(hipFree(h->skill_logits));
        h->skill_logits = nullptr;
    }
    if (!h->skill_logits) HIP_TRY(hipMalloc((void **)&h->skill_logits, N * S * sizeof(float)));
    h->skill_n = (int)S;
    if (!h->skill_value) HIP_TRY(hipMalloc((void **)&h->skill_value, N * sizeof(float)));
    if (!h->sst_mem) {
        HIP_TRY(hipMalloc(&h->sst_mem, 5 * N * sizeof(int32_t)));
        int32_t *m = static_cast<int32_t *>(h->sst_mem);
        h->sst = SkillState{ m, m + N, m + 2 * N, m + 3 * N, m + 4 * N };
    }
    if (n_out == 3 && !h->opt_mem) {
        HIP_TRY(hipMalloc(&h->opt_mem, (5 * N + 1) * 4));
        float *m = static_cast<float *>(h->opt_mem);
        h->oterm = OptionTerm{ m, m + N, m + 2 * N, m + 3 * N };
        h->olist.list = reinterpret_cast<int32_t *>(m + 4 * N);
        h->olist.count = h->olist.list + N;
    }
    if (h->opt_mem) HIP_TRY(hipMemsetAsync(h->opt_mem, 0, (5 * N + 1) * 4, h->stream));
    HIP_TRY(hipMemsetAsync(h->skill_logits, 0, N * S * sizeof(float), h->stream));
    HIP_TRY(hipMemsetAsync(h->skill_value, 0, N * sizeof(float), h->stream));
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 1, h->stream));     // every env: no skill (the new S may be smaller)
    // ... and with the skills go the high-level transitions zenv_collect_option left open
    if (h->hcarry_mem) HIP_TRY(launch_hier_reset(h->hcarry, nullptr, h->n_env, h->stream));
    h->skill = skill_f32_at(*w, static_cast<const float *>(h->skill_mem), o);
    HIP_TRY(hipStreamSynchronize(h->stream));
    (n_out == 3 ? h->option_ready : h->skill_ready) = true;
    if (n_out == 3 || (h->skinv_ready && (h->skinv.h != w->h_dim || h->skinv.S != w->n_skills))) h->skinv_ready = false;
    return ZENV_OK;
}

extern "C" int zenv_skill_load(zenv_t *h, const zenv_skill_weights *w)
{
    if (!h || !w) return fail(ZENV_E_ARG, "null argument");
    return load_skill_family(h, w, 2);
}

extern "C" int zenv_skill_inverse_load(zenv_t *h, const zenv_skill_inverse_weights *w)
{
    if (!h || !w) return fail(ZENV_E_ARG, "null argument");
    if (!h->skill_ready) return fail(ZENV_E_STATE, "zenv_skill_load first (the inverse model takes its shapes)");
    if (w->h_dim != h->skill.h || w->n_skills != h->skill.S || w->zone_feat != h->p.F)
        return fail(ZENV_E_ARG, "inverse model h_dim %d, n_skills %d, zone_feat %d: the skill weights have %d, %d, %d",
                    w->h_dim, w->n_skills, w->zone_feat, h->skill.h, h->skill.S, h->p.F);
    if (w->precision != ZENV_MLP_F32)
        return fail(ZENV_E_ARG, "zenv_skill_inverse_weights.precision %d: only ZENV_MLP_F32 is built", w->precision);
    for (const float *t : { w->zone_w1, w->zone_b1, w->zone_w2, w->zone_b2, w->zone_w3, w->zone_b3, w->comb_w1,
                            w->comb_b1, w->comb_w2, w->comb_b2 })
        if (!t) return fail(ZENV_E_ARG, "zenv_skill_inverse_weights has a null tensor");
    std::vector<float> img;
    size_t o[kSkillInvPtrs];
    pack_skill_inverse_f32(*w, h->p.F, img, o);
    if (int rc = use_device(h)) return rc;
    h->skinv_ready = false;
    if (int rc = replace_image(h, h->skinv_mem, img.data(), img.size() * sizeof(float))) return rc;
    h->skinv = skill_inverse_f32_at(*w, static_cast<const float *>(h->skinv_mem), o);
    h->skinv_ready = true;
    return ZENV_OK;
}

extern "C" int zenv_skill_configure(zenv_t *h, int skill_len)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (skill_len < 1) return fail(ZENV_E_ARG, "skill_len %d: must be >= 1", skill_len);
    h->skill_len = skill_len;
    return ZENV_OK;
}

extern "C" int zenv_set_skills(zenv_t *h, const int32_t *skills)
{
    if (!h || !skills) return fail(ZENV_E_ARG, "null argument");
    if (!h->skill_ready && !h->option_ready) return fail(ZENV_E_STATE, "zenv_skill_load or zenv_option_load first");
    for (int i = 0; i < h->n_env; ++i)
        if (skills[i] < -1 || skills[i] >= h->skill_n)
            return fail(ZENV_E_ARG, "env %d: skill %d outside -1 .. %d", i, skills[i], h->skill_n - 1);
    if (int rc = use_device(h)) return rc;
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    HIP_TRY(hipMemcpyAsync(h->sst.in, skills, sizeof(int32_t) * (size_t)h->n_env, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_skill_set(h->p, h->sst, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));      // `skills` is the caller's (pageable) memory
    return ZENV_OK;
}

extern "C" int zenv_skill_forward(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->skill_ready) return fail(ZENV_E_STATE, "zenv_skill_load first");
    if (!h->was_reset) return fail(ZENV_E_STATE, "reset before asking for actions");
    if (int rc = use_device(h)) return rc;
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    const SkillPick none{ -1, h->skill_len, 0u, 0ull, 0ull, 0, nullptr, SkillRecord{} };
    HIP_TRY(launch_skill_high(h->skill, h->p, h->sst, h->skill_logits, h->skill_value, none, h->stream));
    HIP_TRY(launch_skill_low(h->skill, h->p, h->sst, h->mlp_mu, h->mlp_std, h->mlp_value, no_mlp_action(), h->stream));
    return ZENV_OK;
}

// one step of evaluate_hier.py:63-67: a skill for the envs whose skill ran out (or that have none), then the low level's
// action of every env into `out`
static int run_skill_policy(zenv_t *h, int policy, uint32_t step_index, uint64_t seed, uint64_t env_index0, float *out)
{
    if (!h->skill_ready) return fail(ZENV_E_STATE, "zenv_skill_load first");
    const int mode = policy == ZENV_POLICY_SKILL_SAMPLE ? 1 : 0;
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    const SkillPick pick{ mode, h->skill_len, step_index, seed, env_index0, 0, nullptr, SkillRecord{} };
    HIP_TRY(launch_skill_high(h->skill, h->p, h->sst, h->skill_logits, h->skill_value, pick, h->stream));
    const MlpAction act{ mode, step_index, seed, env_index0, out, MlpRecord{} };
    HIP_TRY(launch_skill_low(h->skill, h->p, h->sst, h->mlp_mu, h->mlp_std, h->mlp_value, act, h->stream));
    return ZENV_OK;
}

// ============================================================================ variable-length Options agent
extern "C" int zenv_option_load(zenv_t *h, const zenv_option_weights *w)
{
    if (!h || !w) return fail(ZENV_E_ARG, "null argument");
    // the same members in the same order: only the rows of lo_mu_* / lo_std_* differ
    static_assert(sizeof(zenv_option_weights) == sizeof(zenv_skill_weights), "zenv_option_weights layout");
    zenv_skill_weights sw;
    std::memcpy(&sw, w, sizeof sw);
    if (int rc = load_skill_family(h, &sw, 3)) return rc;
    // diagnostic: how the high level finds the envs that pick; the results are the same
    const char *e = std::getenv("ZENV_OPTION_COMPACT");
    h->option_compact = e ? std::atoi(e) != 0 : h->n_env > kOptionCompactMinEnvs;
    return ZENV_OK;
}

extern "C" int zenv_option_forward(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->option_ready) return fail(ZENV_E_STATE, "zenv_option_load first");
    if (!h->was_reset) return fail(ZENV_E_STATE, "reset before asking for actions");
    if (int rc = use_device(h)) return rc;
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    const OptionPick none{ -1, 0, 0u, 0ull, 0ull };
    HIP_TRY(launch_option_high(h->skill, h->p, h->sst, h->olist, h->skill_logits, h->skill_value, none, h->stream));
    HIP_TRY(launch_option_low(h->skill, h->p, h->sst, h->olist, h->mlp_mu, h->mlp_std, h->mlp_value, h->oterm,
                              no_mlp_action(), h->stream));
    return ZENV_OK;
}

// one step of options/scripts/evaluate_hier.py:63-75: a skill for the envs that have none or whose option ended, then
// the low level's action of every env into `out` and the termination draw
static int run_option_policy(zenv_t *h, int policy, uint32_t step_index, uint64_t seed, uint64_t env_index0, float *out)
{
    if (!h->option_ready) return fail(ZENV_E_STATE, "zenv_option_load first");
    const int mode = policy == ZENV_POLICY_OPTION_SAMPLE ? 1 : 0;
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    const OptionPick pick{ mode, h->option_compact, step_index, seed, env_index0 };
    if (pick.compact) HIP_TRY(launch_option_list(h->p, h->sst, h->olist, h->stream));
    HIP_TRY(launch_option_high(h->skill, h->p, h->sst, h->olist, h->skill_logits, h->skill_value, pick, h->stream));
    const MlpAction act{ mode, step_index, seed, env_index0, out, MlpRecord{} };
    HIP_TRY(launch_option_low(h->skill, h->p, h->sst, h->olist, h->mlp_mu, h->mlp_std, h->mlp_value, h->oterm, act,
                              h->stream));
    return ZENV_OK;
}

// ============================================================================ xy-goals hierarchical agent
extern "C" int zenv_xy_load(zenv_t *h, const zenv_xy_weights *w)
{
    if (!h || !w) return fail(ZENV_E_ARG, "null argument");
    if (h->goal_enabled || h->order_enabled)
        return fail(ZENV_E_STATE, "the xy-goals agent steps a plain task handle, not a goal-conditioned / solver-ordered one");
    if (w->h_dim < 1 || w->h_dim >= kMlpHP) return fail(ZENV_E_ARG, "h_dim %d outside 1 .. %d", w->h_dim, kMlpHP - 1);
    if (w->precision != ZENV_MLP_F32)
        return fail(ZENV_E_ARG, "zenv_xy_weights.precision %d: only ZENV_MLP_F32 is built", w->precision);
    if (w->zone_feat != h->p.F)
        return fail(ZENV_E_ARG, "the weights take zone rows of %d features, this handle's have %d", w->zone_feat, h->p.F);
    int rc = check_tensors({ w->hi_zone_w1, w->hi_zone_b1, w->hi_zone_w2, w->hi_zone_b2, w->hi_zone_w3, w->hi_zone_b3,
                             w->hi_comb_w, w->hi_comb_b, w->hi_enc_w, w->hi_enc_b, w->hi_mu_w, w->hi_mu_b, w->hi_std_w,
                             w->hi_std_b, w->lo_zone_w1, w->lo_zone_b1, w->lo_zone_w2, w->lo_zone_b2, w->lo_zone_w3,
                             w->lo_zone_b3, w->lo_comb_w, w->lo_comb_b, w->lo_enc_w, w->lo_enc_b, w->lo_mu_w, w->lo_mu_b,
                             w->lo_std_w, w->lo_std_b },
                           { w->hi_critic_w1, w->hi_critic_b1, w->hi_critic_w2, w->hi_critic_b2 },
                           { w->lo_critic_w1, w->lo_critic_b1, w->lo_critic_w2, w->lo_critic_b2 });
    if (rc) return rc;
    std::vector<float> img;
    size_t o[kXyPtrs];
    pack_xy_f32(*w, h->p.F, img, o);
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env;
    // the skill state's clock has one owner: the skill planner, the Options agent or this one
    h->skill_ready = h->option_ready = h->skinv_ready = h->xy_ready = false;
    if (int rc = replace_image(h, h->xy_mem, img.data(), img.size() * sizeof(float))) return rc;
    if (int rc = ensure_policy_outputs(h)) return rc;
    if (!h->sst_mem) {
        HIP_TRY(hipMalloc(&h->sst_mem, 5 * N * sizeof(int32_t)));
        int32_t *m = static_cast<int32_t *>(h->sst_mem);
        h->sst = SkillState{ m, m + N, m + 2 * N, m + 3 * N, m + 4 * N };
    }
    Carver cv;
    if (!h->xy_state_mem) {
        cv.piece(h->xy_goal, N);
        cv.piece(h->xy_goal_in, N);
        cv.piece(h->xy_goal_mu, N * 2);
        cv.piece(h->xy_goal_std, N * 2);
        cv.piece(h->xy_value, N);
        cv.piece(h->xy_age, N);
        cv.piece(h->xy_mask, N);
        if (int rc = cv.alloc(&h->xy_state_mem, "xy-goals state")) return rc;
        HIP_TRY(hipMemsetAsync(h->xy_state_mem, 0, cv.bytes(), h->stream));
    } else {
        HIP_TRY(hipMemsetAsync(h->xy_goal, 0, N * sizeof(float2), h->stream));
        HIP_TRY(hipMemsetAsync(h->xy_goal_mu, 0, N * 2 * sizeof(float), h->stream));
        HIP_TRY(hipMemsetAsync(h->xy_goal_std, 0, N * 2 * sizeof(float), h->stream));
        HIP_TRY(hipMemsetAsync(h->xy_value, 0, N * sizeof(float), h->stream));
    }
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 1, h->stream));     // every env: no goal
    // ... and with the skills go the high-level transitions zenv_collect_option left open
    if (h->hcarry_mem) HIP_TRY(launch_hier_reset(h->hcarry, nullptr, h->n_env, h->stream));
    h->xy = xy_f32_at(*w, static_cast<const float *>(h->xy_mem), o);
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->xy_ready = true;
    return ZENV_OK;
}

extern "C" int zenv_set_xy_goals(zenv_t *h, const float *goals, const uint8_t *mask)
{
    if (!h || !goals) return fail(ZENV_E_ARG, "null argument");
    if (!h->xy_ready) return fail(ZENV_E_STATE, "zenv_xy_load first");
    for (int i = 0; i < h->n_env; ++i)
        if ((!mask || mask[i]) && !(std::isfinite(goals[2 * i]) && std::isfinite(goals[2 * i + 1])))
            return fail(ZENV_E_ARG, "env %d: goal (%g, %g) is not finite", i, (double)goals[2 * i], (double)goals[2 * i + 1]);
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env;
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    HIP_TRY(hipMemcpyAsync(h->xy_goal_in, goals, N * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    if (mask) HIP_TRY(hipMemcpyAsync(h->xy_mask, mask, N, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_xy_set(h->p, h->sst, h->xy_goal, h->xy_goal_in, mask ? h->xy_mask : nullptr, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));      // `goals` and `mask` are the caller's (pageable) memory
    return ZENV_OK;
}

extern "C" int zenv_xy_forward(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->xy_ready) return fail(ZENV_E_STATE, "zenv_xy_load first");
    if (!h->was_reset) return fail(ZENV_E_STATE, "reset before asking for actions");
    if (int rc = use_device(h)) return rc;
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    const XyPick none{ -1, h->skill_len, 0u, 0ull, 0ull, 0, nullptr, XyRecord{} };
    HIP_TRY(launch_xy_high(h->xy, h->p, h->sst, h->xy_goal, h->xy_goal_mu, h->xy_goal_std, h->xy_value, none, h->stream));
    HIP_TRY(launch_xy_low(h->xy, h->p, h->sst, h->xy_goal, h->mlp_mu, h->mlp_std, h->mlp_value, no_mlp_action(),
                          h->stream));
    return ZENV_OK;
}

// one step of evaluate_xy_hrl.py:62-70: a goal for the envs whose goal ran out (or that have none), then the low level's
// action of every env into `out`
static int run_xy_policy(zenv_t *h, int policy, uint32_t step_index, uint64_t seed, uint64_t env_index0, float *out)
{
    if (!h->xy_ready) return fail(ZENV_E_STATE, "zenv_xy_load first");
    const int mode = policy == ZENV_POLICY_XY_SAMPLE ? 1 : 0;
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    const XyPick pick{ mode, h->skill_len, step_index, seed, env_index0, 0, nullptr, XyRecord{} };
    HIP_TRY(launch_xy_high(h->xy, h->p, h->sst, h->xy_goal, h->xy_goal_mu, h->xy_goal_std, h->xy_value, pick, h->stream));
    const MlpAction act{ mode, step_index, seed, env_index0, out, MlpRecord{} };
    HIP_TRY(launch_xy_low(h->xy, h->p, h->sst, h->xy_goal, h->mlp_mu, h->mlp_std, h->mlp_value, act, h->stream));
    return ZENV_OK;
}

// a_t = pi(obs_t, t) into pol.out, for every kind of action source
int run_policy(zenv *h, const StepPolicy &pol, const MlpRecord *rec, float *rows)
{
    if (!policy_is_mlp(pol.policy)) {
        HIP_TRY(launch_policy(h->p, pol, h->stream));
        return ZENV_OK;
    }
    if (!h->mlp_ready) return fail(ZENV_E_STATE, "zenv_mlp_load first");
    // the head kernel also turns (mu, std) into the action
    const MlpAction act{ pol.policy == ZENV_POLICY_MLP_SAMPLE ? 1 : 0, pol.step_index, pol.seed, pol.env_index0, pol.out,
                         rec ? *rec : MlpRecord{} };
    return flat_forward(h, act, rows);
}

// A ring schedule is only as deep as its `depth` slots per env, and only the HOST refills them (zenv_bank_update), between
// calls: an env ends at most one episode per auto-resetting step, so a call of up to `depth` such steps cannot outrun
// its ring; a longer one could wrap onto maps it has already played -- silently.  Refused instead.  `steps` counts the
// call's auto-resets per env: its steps, frames, or skill windows (zenv_collect_skill resets on a window's last frame).
int ring_guard(const zenv *h, int steps, int auto_reset_every_step)
{
    if (h->p.sched_mode == SCHED_RING && auto_reset_every_step && steps > h->p.sched_stride)
        return fail(ZENV_E_STATE, "a ring schedule of depth %d is refilled by the host between calls: %d auto-resetting "
                    "steps in one call could replay maps (use calls of at most `depth` steps with zenv_bank_update in "
                    "between, a deeper ring, or a sequential schedule)", h->p.sched_stride, steps);
    return ZENV_OK;
}

// ============================================================================ experience collection
// the collectors' discount and gae_lambda: finite and in [0, 1] (a NaN would turn every advantage into NaN)
static int gae_args(float discount, float gae_lambda)
{
    if (!std::isfinite(discount) || !std::isfinite(gae_lambda))
        return fail(ZENV_E_ARG, "discount %g and gae_lambda %g must be finite", discount, gae_lambda);
    if (discount < 0.f || discount > 1.f || gae_lambda < 0.f || gae_lambda > 1.f)
        return fail(ZENV_E_ARG, "discount %g and gae_lambda %g must lie in [0, 1]", discount, gae_lambda);
    return ZENV_OK;
}

// What the collectors ask before anything else: a handle that was reset and keeps its results on the device,
// T x N frames that fit the kernels' 32-bit slots, sane GAE factors, and no more auto-resets (`resets` per env) than a
// ring schedule is deep
static int collect_ready(const zenv *h, const char *who, int T, int resets, float discount, float gae_lambda)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if ((int64_t)T * h->n_env > INT32_MAX) return fail(ZENV_E_ARG, "frames_per_proc x envs must stay below 2^31");
    if (int ra = gae_args(discount, gae_lambda)) return ra;
    if (!h->was_reset) return fail(ZENV_E_STATE, "Environment must be reset before stepping");
    if (h->host_io_slab) return fail(ZENV_E_STATE, "%s records on the device: switch zenv_host_io off first", who);
    return ring_guard(h, resets, 1);
}

namespace {

// The collectors record the observations where they are produced: the policy of frame t reads slot t of the
// ZENV_F_EXP_* buffers, the step kernel of frame t writes obs_{t+1} into slot t + 1 (the last one into the handle's own
// buffers again).  Whatever way the call returns, the handle gets its own buffers back.
//
// A handle with zenv_order_rows on records 7-wide rows, which the step kernel cannot write: it keeps writing the handle's
// own 6-wide buffer, and k_order_rows fills slot t (rows(t)) when the policy of frame t is about to read it.  `obs`
// keeps its aliasing.
class FrameObs {
    zenv *h_;
    float *obs_, *zone_obs_;     // the handle's own
    size_t n_obs_, n_zone_;      // floats per frame
    bool assembled_;             // the zone rows of a slot are assembled (zenv_order_rows), not written in place
    void point_at(float *obs, float *zone_obs) const { h_->p.obs = obs, h_->p.zone_obs = assembled_ ? zone_obs_ : zone_obs; }

public:
    explicit FrameObs(zenv *h)
        : h_(h), obs_(h->p.obs), zone_obs_(h->p.zone_obs), n_obs_((size_t)h->n_env * 8),
          n_zone_((size_t)h->n_env * h->p.Z * net_row_feat(h)), assembled_(h->net_feat != 0) {}
    FrameObs(const FrameObs &) = delete;
    ~FrameObs() { point_at(obs_, zone_obs_); }
    int begin() const            // obs_0 into slot 0
    {
        HIP_TRY(hipMemcpyAsync(h_->exp.obs, obs_, n_obs_ * 4, hipMemcpyDeviceToDevice, h_->stream));
        if (!assembled_)
            HIP_TRY(hipMemcpyAsync(h_->exp.zone_obs, zone_obs_, n_zone_ * 4, hipMemcpyDeviceToDevice, h_->stream));
        return ZENV_OK;
    }
    // where the policy of frame t has its rows assembled; null: they are already in place
    float *rows(int t) const { return assembled_ ? h_->exp.zone_obs + t * n_zone_ : nullptr; }
    void read(int t) const { point_at(h_->exp.obs + t * n_obs_, h_->exp.zone_obs + t * n_zone_); }
    void write_next(int t, int T) const { t + 1 < T ? read(t + 1) : point_at(obs_, zone_obs_); }
};

}  // namespace

// the ZENV_F_EXP_* buffers for T frames (every collector's); self.mask survives a change of T
static int ensure_exp(zenv_t *h, int T)
{
    const size_t N = (size_t)h->n_env, ZF = (size_t)h->p.Z * net_row_feat(h);
    h->exp_hier = false;        // zenv_collect_hier sets it once its records are complete
    h->exp_xy = false;          // zenv_collect_xy, the same
    h->exp_skill = false;       // zenv_collect_skill, the same
    h->exp_option = false;      // zenv_collect_option, the same
    h->diayn_kept = -1;         // zenv_diayn_samples' list was of the records this call overwrites
    h->eplog.source = 0;        // zenv_episode_log: every collector arms it once its records are complete
    if (!h->exp_mem || h->exp.T != T) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        std::vector<float> keep_mask;
        if (h->exp_mem) {       // self.mask survives a change of T
            keep_mask.resize(N);
            HIP_TRY(hipMemcpy(keep_mask.data(), h->exp.cur_mask, N * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipFree(h->exp_mem));
            h->exp_mem = nullptr;
        }
        const size_t per_slot = 8 + ZF + 2 + 2 + 5;            // floats per (env, t)
        const size_t total = N * (size_t)T * per_slot + N;
        HIP_TRY(hipMalloc(&h->exp_mem, total * sizeof(float)));
        float *f = static_cast<float *>(h->exp_mem);
        ExpBuffers &x = h->exp;
        x.T = T;
        x.obs = f;            f += N * T * 8;
        x.zone_obs = f;       f += N * T * ZF;
        x.action = f;         f += N * T * 2;
        x.log_prob = f;       f += N * T * 2;
        x.value = f;          f += N * T;
        x.reward = f;         f += N * T;
        x.mask = f;           f += N * T;
        x.advantage = f;      f += N * T;
        x.returnn = f;        f += N * T;
        x.cur_mask = f;
        if (keep_mask.empty()) keep_mask.assign(N, 1.0f);      // base.py:96 self.mask = ones
        HIP_TRY(hipMemcpy(x.cur_mask, keep_mask.data(), N * 4, hipMemcpyHostToDevice));
    }
    return ZENV_OK;
}

extern "C" int zenv_collect(zenv_t *h, int T, uint64_t policy_seed, uint64_t env_index0, float discount, float gae_lambda)
{
    if (T < 1) return fail(ZENV_E_ARG, "frames_per_proc must be positive");
    if (int rc = collect_ready(h, "zenv_collect", T, T, discount, gae_lambda)) return rc;     // every frame auto-resets
    if (!h->mlp_ready || !h->mlp.wv1) return fail(ZENV_E_STATE, "zenv_mlp_load with actor and critic weights first");
    if (h->order_enabled && !h->net_feat)
        return fail(ZENV_E_STATE, "solver-ordered envs are stepped with zenv_step (their order feature is not part of "
                                  "the network input this call evaluates: zenv_order_rows makes it one)");
    if (int rc = use_device(h)) return rc;
    h->act_tag.valid = false;
    if (int rc = ensure_exp(h, T)) return rc;
    // the envs that report info['shaped_reward'] train on it (base.py:159-162); the env reward goes beside it
    const bool shaped = h->goal_enabled || h->order_enabled;
    if (shaped)
        if (int rc = eplog_flat_reward(h, T)) return rc;
    const FrameObs frames(h);
    if (int rc = frames.begin()) return rc;
    for (int t = 0; t < T; ++t) {
        frames.read(t);
        StepPolicy pol{ ZENV_POLICY_MLP_SAMPLE, (uint32_t)h->step_count, policy_seed, env_index0, h->p.actions };
        // dist, value = acmodel(obs); action = dist.sample(); the head kernel also records frame t (and the reward
        // of frame t-1, still in the env's reward / done buffers)
        const MlpRecord rec{ h->exp.action, h->exp.log_prob, h->exp.value, h->exp.mask, h->exp.reward, h->exp.cur_mask,
                             h->p.reward, shaped ? h->p.shaped : nullptr, h->p.done_out, T, t, h->n_env };
        if (int rc = run_policy(h, pol, &rec, frames.rows(t))) return rc;
        frames.write_next(t, T);
        HIP_TRY(launch_step(h->p, h->p.actions, 1, no_policy(), h->stream));     // ParallelEnv.step: auto-reset
        if (h->goal_enabled) HIP_TRY(launch_goal_step(h->p, h->stream));
        if (h->order_enabled) {
            HIP_TRY(launch_order_step(h->p, h->stream));
            HIP_TRY(order_wait_after_step(h->order_wait, h->p, 1, h->stream));
        }
        if (shaped) {
            // the env reward beside the shaped one the record keeps: zenv_episode_log's return (base.py:169)
            HIP_TRY(hipMemcpyAsync(h->eplog.flat_reward + (size_t)t * h->n_env, h->p.reward, (size_t)h->n_env * 4,
                                   hipMemcpyDeviceToDevice, h->stream));
        }
        h->step_count += 1;
    }
    HIP_TRY(launch_exp_reward(h->exp, h->n_env, T - 1, h->p.reward, shaped ? h->p.shaped : nullptr,
                              h->p.done_out, h->stream));
    // next_value = value(obs_T) (:177-187), then the GAE recursion
    if (int rc = flat_forward(h, no_mlp_action())) return rc;
    HIP_TRY(launch_exp_gae(h->exp, h->n_env, h->mlp_value, discount, gae_lambda, h->stream));
    h->eplog.source = 1;
    return ZENV_OK;
}

// ---- zenv_collect_hier: collect_experiences of the Zone-goals agent (zone-goals/src/torch_ac/algos/_hier_policy_opt.py)
// the per-frame records for T frames; the state carried from call to call is allocated (and zeroed) once.
// zenv_collect_option shares them and has no goal input to record (with_goal = false)
static int ensure_hier_collect(zenv_t *h, int T, bool with_goal = true)
{
    const size_t N = (size_t)h->n_env, ZF = (size_t)h->p.Z * h->p.F;
    if (!h->hcarry_mem) {
        HierCarry &c = h->hcarry;
        Carver cv;
        cv.piece(c.src, N);
        cv.piece(c.obs, N * 8);
        cv.piece(c.zone_obs, N * ZF);
        cv.piece(c.hi_reward, N);
        cv.piece(c.value, N);
        cv.piece(c.log_prob, N);
        cv.piece(c.goal, N);
        cv.piece(c.avail, N);
        cv.piece(c.open, N);
        if (int rc = cv.alloc(&h->hcarry_mem, "carry")) return rc;
        HIP_TRY(hipMemsetAsync(h->hcarry_mem, 0, cv.bytes(), h->stream));
    }
    if (!h->hi_total_host) HIP_TRY(hipHostMalloc((void **)&h->hi_total_host, 4, hipHostMallocDefault));
    if (h->hframes_mem && h->hframes.T == T) return ZENV_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->hframes_mem) HIP_TRY(hipFree(h->hframes_mem));
    h->hframes_mem = nullptr;
    const size_t TN = (size_t)T * N;
    HierFrames &f = h->hframes;
    Carver cv;
    cv.piece(f.lo_goal, with_goal ? TN * 2 : 0);
    cv.piece(f.pick_goal, TN);
    cv.piece(f.pick_value, TN);
    cv.piece(f.pick_log_prob, TN);
    cv.piece(f.pick_avail, TN);
    cv.piece(f.close_reward, TN);
    cv.piece(f.env_reward, TN);
    cv.piece(f.count, N);
    cv.piece(f.offset, N);
    cv.piece(f.total, 1);
    cv.piece(f.close_flag, TN);
    if (int rc = cv.alloc(&h->hframes_mem, "frame record")) return rc;
    if (!with_goal) f.lo_goal = nullptr;                          // ZENV_F_LO_GOAL: 0 bytes
    f.T = T;
    HIP_TRY(hipMemsetAsync(h->hframes_mem, 0, cv.bytes(), h->stream));
    return ZENV_OK;
}

// room for M rows of the flat high-level output (grown by half again, never shrunk)
static int ensure_hier_out(zenv_t *h, int64_t M)
{
    if (M <= h->hi_cap) return ZENV_OK;
    const int64_t cap = std::max<int64_t>(M, h->hi_cap + h->hi_cap / 2);
    const size_t Z = (size_t)h->p.Z, ZF = Z * h->p.F, R = (size_t)cap;
    if (h->hout_mem) HIP_TRY(hipFree(h->hout_mem));
    h->hout_mem = nullptr;
    h->hi_cap = 0;
    HierOut &o = h->hout;
    Carver cv;
    cv.piece(o.src, R);
    cv.piece(o.obs, R * 8);
    cv.piece(o.zone_obs, R * ZF);
    cv.piece(o.action, R);
    cv.piece(o.value, R);
    cv.piece(o.log_prob, R);
    cv.piece(o.advantage, R);
    cv.piece(o.returnn, R);
    cv.piece(o.reward, R);
    cv.piece(o.mask, R);
    cv.piece(o.avail, R);
    cv.piece(o.action_mask, R * Z);
    if (int rc = cv.alloc(&h->hout_mem, "output")) return rc;
    h->hi_cap = cap;
    return ZENV_OK;
}

extern "C" int zenv_collect_hier(zenv_t *h, int T, uint64_t policy_seed, uint64_t env_index0, float discount,
                                 float gae_lambda, int64_t *n_hi)
{
    if (T < 2) return fail(ZENV_E_ARG, "frames_per_proc must be at least 2 (the low level hands out T - 1 frames)");
    int rc = collect_ready(h, "zenv_collect_hier", T, T, discount, gae_lambda);     // every frame auto-resets
    if (rc) return rc;
    if (h->order_enabled)
        return fail(ZENV_E_STATE, "zenv_collect_hier runs the goal-conditioned agent: this handle is solver-ordered");
    if (!h->goal_enabled) return fail(ZENV_E_STATE, "zenv_collect_hier needs a goal-conditioned handle: zenv_goal_enable first");
    if (!h->hier_ready) return fail(ZENV_E_STATE, "zenv_hier_load first");
    if (!h->hier.hi_critic || !h->hier.lo_critic)
        return fail(ZENV_E_STATE, "zenv_collect_hier needs both critics (zenv_hier_load with hi_critic_* and lo_critic_*)");
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env, ZF = (size_t)h->p.Z * h->p.F;
    h->act_tag.valid = false;
    h->hi_kind = 0;
    if (int rc = ensure_exp(h, T)) return rc;
    if (int rc = ensure_hier_collect(h, T)) return rc;
    const HierFrames &f = h->hframes;
    const HierCarry &c = h->hcarry;
    HIP_TRY(hipMemsetAsync(f.pick_goal, 0xFF, (size_t)T * N * 4, h->stream));     // -1: no pick
    HIP_TRY(hipMemsetAsync(f.close_flag, 0, (size_t)T * N, h->stream));
    HIP_TRY(hipMemsetAsync(f.count, 0, N * 4, h->stream));
    const FrameObs frames(h);
    if (int rc = frames.begin()) return rc;
    for (int t = 0; t < T; ++t) {
        frames.read(t);
        const uint32_t step_index = (uint32_t)h->step_count;
        const HierRecord hrec{ t, h->n_env, f.pick_goal, f.pick_value, f.pick_log_prob, f.pick_avail, c.open, f.lo_goal };
        // :14-46 goals for the envs that need one (zenv_policy(ZENV_POLICY_HIER_SAMPLE)'s launches), the pick recorded
        const HierPick pick{ 1, step_index, policy_seed, env_index0, h->goal_in };
        HIP_TRY(launch_hier_high(h->hier, h->p, h->hier_logits, h->hier_value, pick, h->stream, hrec));
        HIP_TRY(launch_goal_set(h->p, h->goal_in, h->goal_bad, h->stream));
        // :48-64 the low level's action; frame t recorded (and the shaped reward / mask of frame t-1)
        const MlpRecord rec{ h->exp.action, h->exp.log_prob, h->exp.value, h->exp.mask, h->exp.reward, h->exp.cur_mask,
                             h->p.reward, h->p.shaped, h->p.done_out, T, t, h->n_env };
        const MlpAction act{ 1, step_index, policy_seed, env_index0, h->p.actions, rec };
        HIP_TRY(launch_hier_low(h->hier, h->p, h->mlp_mu, h->mlp_std, h->mlp_value, act, h->stream, hrec));
        frames.write_next(t, T);
        HIP_TRY(launch_step(h->p, h->p.actions, 1, no_policy(), h->stream));     // ParallelEnv.step: auto-reset
        HIP_TRY(launch_goal_step(h->p, h->stream));
        HIP_TRY(launch_hier_close(h->p, f, c, t, h->stream));                     // :66-76
        h->step_count += 1;
    }
    HIP_TRY(launch_exp_reward(h->exp, h->n_env, T - 1, h->p.reward, h->p.shaped, h->p.done_out, h->stream));
    // next_hi_val = V_hi(obs_T) (:93-95), into ZENV_F_HIER_VALUE
    const HierPick value_only{ -2, 0u, 0ull, 0ull, nullptr };
    HIP_TRY(launch_hier_high(h->hier, h->p, h->hier_logits, h->hier_value, value_only, h->stream));
    // :109-116 the low level over frames 0 .. T-2, no bootstrap: frame T-1 is only the "next" frame of T-2
    ExpBuffers lo = h->exp;
    lo.T = T - 1;
    lo.cur_mask = h->exp.mask + (size_t)(T - 1) * N;
    HIP_TRY(launch_exp_gae(lo, h->n_env, h->exp.value + (size_t)(T - 1) * N, discount, gae_lambda, h->stream));
    HIP_TRY(hipMemsetAsync(h->exp.advantage + (size_t)(T - 1) * N, 0, N * 4, h->stream));
    HIP_TRY(hipMemsetAsync(h->exp.returnn + (size_t)(T - 1) * N, 0, N * 4, h->stream));
    // the high level's rows: offsets, then M to the host (the one synchronisation of the call)
    HIP_TRY(launch_hier_count_scan(f, h->n_env, h->stream));
    HIP_TRY(hipMemcpyAsync(h->hi_total_host, f.total, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int64_t M = *h->hi_total_host;
    h->hi_m = 0;
    if (int rc = ensure_hier_out(h, M)) return rc;
    HIP_TRY(launch_hier_gae(f, c, h->hout, h->n_env, h->hier_value, gae_lambda, h->stream));
    HIP_TRY(launch_hier_gather(h->hout, c, h->exp.obs, h->exp.zone_obs, M, h->n_env, h->p.Z, h->p.F, h->stream));
    HIP_TRY(launch_hier_carry(c, h->exp.obs, h->exp.zone_obs, h->n_env, (int)ZF, h->stream));
    h->hi_m = M;
    h->exp_hier = true;
    h->eplog.source = 2;
    if (n_hi) *n_hi = M;
    return ZENV_OK;
}


// ---- zenv_collect_skill: collect_experiences of the fixed-length-skills agent and DIAYN (main/src/torch_ac/algos/
// _hier_policy_opt.py:9-233).  The per-frame records for T frames (the ZENV_F_EXP_* buffers aside)
static int ensure_skill_collect(zenv_t *h, int T)
{
    if (h->sk_mem && h->sk.T == T) return ZENV_OK;
    const size_t N = (size_t)h->n_env, TN = (size_t)T * N;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->sk_mem) HIP_TRY(hipFree(h->sk_mem));
    h->sk_mem = nullptr;
    Carver cv;
    cv.piece(h->sk.lo_skill, TN);
    cv.piece(h->sk.diversity, TN);
    cv.piece(h->sk.env_reward, TN);
    cv.piece(h->sk.boot, N);
    cv.piece(h->sk.count, N);
    if (int rc = cv.alloc(&h->sk_mem, "skill record")) return rc;
    HIP_TRY(hipMemsetAsync(h->sk_mem, 0, cv.bytes(), h->stream));
    h->sk.T = T;
    return ZENV_OK;
}

extern "C" int zenv_collect_skill(zenv_t *h, int T, uint64_t policy_seed, uint64_t env_index0, float discount,
                                  float gae_lambda, float diversity_coef, const float *skill_prior_logits, int sample_hi)
{
    const int L = h ? h->skill_len : 1;
    int rc = collect_ready(h, "zenv_collect_skill", T, T / L, discount, gae_lambda);   // a window's last frame resets
    if (rc) return rc;
    if (h->order_enabled || h->goal_enabled)
        return fail(ZENV_E_STATE, "zenv_collect_skill steps a plain task handle, not a goal-conditioned / solver-ordered one");
    if (!h->skill_ready) return fail(ZENV_E_STATE, "zenv_skill_load first");
    if (!h->skill.hi_critic || !h->skill.lo_critic)
        return fail(ZENV_E_STATE, "zenv_collect_skill needs both critics (zenv_skill_load with hi_critic_* and lo_critic_*)");
    const int S = h->skill.S;
    if (T < 1 || T % L != 0)
        return fail(ZENV_E_ARG, "frames_per_proc %d must be a positive multiple of skill_len %d", T, L);
    if (!std::isfinite(diversity_coef)) return fail(ZENV_E_ARG, "diversity_coef must be finite");
    if (diversity_coef != 0.f && !h->skinv_ready)
        return fail(ZENV_E_ARG, "diversity_coef %g without an inverse model (zenv_skill_inverse_load)", diversity_coef);
    SkillDiv div{};
    div.N = h->n_env;
    div.net = h->skinv_ready ? 1 : 0;
    div.coef = diversity_coef;
    if (h->skinv_ready) {
        if (!skill_prior_logits) return fail(ZENV_E_ARG, "skill_prior_logits is null (an inverse model is loaded)");
        double m = -INFINITY;
        for (int s = 0; s < S; ++s) {
            if (!std::isfinite(skill_prior_logits[s])) return fail(ZENV_E_ARG, "skill_prior_logits[%d] is not finite", s);
            m = std::max(m, (double)skill_prior_logits[s]);
        }
        double sum = 0.0;                                        // log_softmax(self.skill_logits, dim=0), once per call
        for (int s = 0; s < S; ++s) sum += std::exp((double)skill_prior_logits[s] - m);
        for (int s = 0; s < S; ++s) div.prior[s] = (float)((double)skill_prior_logits[s] - m - std::log(sum));
    }
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env;
    const int W = T / L;
    h->act_tag.valid = false;
    if (int rc = ensure_exp(h, T)) return rc;
    if (int rc = ensure_skill_collect(h, T)) return rc;
    h->hi_m = 0;
    h->hi_kind = 1;
    if (int rc = ensure_hier_out(h, (int64_t)N * W)) return rc;
    h->hi_m = (int64_t)N * W;
    const HierOut &o = h->hout;
    div.skill = h->sk.lo_skill;
    div.diversity = h->sk.diversity;
    div.exp_reward = h->exp.reward;
    const FrameObs frames(h);
    if (int rc = frames.begin()) return rc;
    for (int t = 0; t < T; ++t) {
        frames.read(t);
        const uint32_t step_index = (uint32_t)h->step_count;
        SkillRecord sr{ t, h->n_env, W, t / L, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
        if (t % L == 0) {
            // :28-45 every env picks (hi_dist.sample() or randint), the pick recorded in row env * W + t / L
            HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
            SkillPick pick{ sample_hi ? 1 : 2, L, step_index, policy_seed, env_index0, 1, nullptr, sr };
            pick.rec.hi_obs = o.obs;
            pick.rec.hi_zone_obs = o.zone_obs;
            pick.rec.hi_skill = o.action;
            pick.rec.hi_value = o.value;
            pick.rec.hi_log_prob = o.log_prob;
            HIP_TRY(launch_skill_high(h->skill, h->p, h->sst, h->skill_logits, h->skill_value, pick, h->stream));
        }
        // :60-64 the low level's action; frame t recorded (and the env reward / mask of frame t-1)
        const MlpRecord rec{ h->exp.action, h->exp.log_prob, h->exp.value, h->exp.mask, h->sk.env_reward,
                             h->exp.cur_mask, h->p.reward, nullptr, h->p.done_out, T, t, h->n_env };
        const MlpAction act{ 1, step_index, policy_seed, env_index0, h->p.actions, rec };
        sr.lo_skill = h->sk.lo_skill;
        HIP_TRY(launch_skill_low(h->skill, h->p, h->sst, h->mlp_mu, h->mlp_std, h->mlp_value, act, h->stream, &sr));
        frames.write_next(t, T);
        // :68-71 step_no_reset inside a window, step on its last frame
        HIP_TRY(launch_step(h->p, h->p.actions, (t + 1) % L == 0 ? 1 : 0, no_policy(), h->stream));
        // :74-91 the diversity reward on obs_{t+1} and the low level's reward
        div.t = t;
        HIP_TRY(launch_skill_inverse(h->skinv, h->p, div, h->stream));
        h->step_count += 1;
    }
    {   // the env reward of frame T-1 and self.lo_mask = 1 - done
        ExpBuffers last = h->exp;
        last.reward = h->sk.env_reward;
        HIP_TRY(launch_exp_reward(last, h->n_env, T - 1, h->p.reward, nullptr, h->p.done_out, h->stream));
    }
    // :131-139 next_hi_value = V_hi(obs_T); s' ~ hi_dist(obs_T) on a stream of its own; next_lo_value = V_lo(obs_T, s')
    const SkillPick boot{ 3, L, (uint32_t)h->step_count, policy_seed, env_index0, 1, h->sk.boot, SkillRecord{} };
    HIP_TRY(launch_skill_high(h->skill, h->p, h->sst, h->skill_logits, h->skill_value, boot, h->stream));
    SkillState sb = h->sst;
    sb.skill = h->sk.boot;
    HIP_TRY(launch_skill_low(h->skill, h->p, sb, h->mlp_mu, h->mlp_std, h->mlp_value, no_mlp_action(), h->stream));
    // :154-161 the low level over all T frames; :142-151 the high level per env over its windows
    HIP_TRY(launch_exp_gae(h->exp, h->n_env, h->mlp_value, discount, gae_lambda, h->stream));
    HIP_TRY(launch_skill_hi_gae(o, T, L, h->n_env, h->sk.env_reward, h->exp.mask, h->exp.cur_mask, h->skill_value,
                                gae_lambda, h->sk.count, h->stream));
    h->exp_skill = true;
    h->eplog.source = 3;
    return ZENV_OK;
}

// ---- zenv_collect_xy: collect_experiences of the xy-goals agent (xy-goals/src/torch_ac/algos/_hier_policy_opt.py:
// 10-192).  The per-frame records for T frames in W windows (the ZENV_F_EXP_* buffers aside)
static int ensure_xy_collect(zenv_t *h, int T, int W)
{
    if (h->xc_mem && h->xc.T == T && h->xc.W == W) return ZENV_OK;
    const size_t N = (size_t)h->n_env, TN = (size_t)T * N;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->xc_mem) HIP_TRY(hipFree(h->xc_mem));
    h->xc_mem = nullptr;
    Carver cv;
    cv.piece(h->xc.lo_goal, TN);
    cv.piece(h->xc.dist, TN);
    cv.piece(h->xc.env_reward, TN);
    cv.piece(h->xc.hi_goal, N * (size_t)W);
    cv.piece(h->xc.boot, N);
    cv.piece(h->xc.count, N);
    if (int rc = cv.alloc(&h->xc_mem, "xy-goals record")) return rc;
    HIP_TRY(hipMemsetAsync(h->xc_mem, 0, cv.bytes(), h->stream));
    h->xc.T = T;
    h->xc.W = W;
    return ZENV_OK;
}

extern "C" int zenv_collect_xy(zenv_t *h, int T, uint64_t policy_seed, uint64_t env_index0, float discount,
                               float gae_lambda)
{
    const int L = h ? h->skill_len : 1;
    int rc = collect_ready(h, "zenv_collect_xy", T, T / L, discount, gae_lambda);     // a window's last frame resets
    if (rc) return rc;
    if (h->order_enabled || h->goal_enabled)
        return fail(ZENV_E_STATE, "zenv_collect_xy steps a plain task handle, not a goal-conditioned / solver-ordered one");
    if (!h->xy_ready) return fail(ZENV_E_STATE, "zenv_xy_load first");
    if (!h->xy.hi_critic || !h->xy.lo_critic)
        return fail(ZENV_E_STATE, "zenv_collect_xy needs both critics (zenv_xy_load with hi_critic_* and lo_critic_*)");
    if (T < 1 || T % L != 0)
        return fail(ZENV_E_ARG, "frames_per_proc %d must be a positive multiple of skill_len %d", T, L);
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env;
    const int W = T / L;
    h->act_tag.valid = false;
    if (int rc = ensure_exp(h, T)) return rc;
    if (int rc = ensure_xy_collect(h, T, W)) return rc;
    h->hi_m = 0;
    h->hi_kind = 3;
    if (int rc = ensure_hier_out(h, (int64_t)N * W)) return rc;
    h->hi_m = (int64_t)N * W;
    const HierOut &o = h->hout;
    const FrameObs frames(h);
    if (int rc = frames.begin()) return rc;
    for (int t = 0; t < T; ++t) {
        frames.read(t);
        const uint32_t step_index = (uint32_t)h->step_count;
        XyRecord xr{ t, h->n_env, W, t / L, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
        if (t % L == 0) {
            // :29-42 every env picks, whatever it held (goal ~ hi_dist), the pick recorded in row env * W + t / L
            HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
            XyPick pick{ 1, L, step_index, policy_seed, env_index0, 1, nullptr, xr };
            pick.rec.hi_obs = o.obs;
            pick.rec.hi_zone_obs = o.zone_obs;
            pick.rec.hi_goal = h->xc.hi_goal;
            pick.rec.hi_value = o.value;
            pick.rec.hi_log_prob = o.log_prob;
            HIP_TRY(launch_xy_high(h->xy, h->p, h->sst, h->xy_goal, h->xy_goal_mu, h->xy_goal_std, h->xy_value, pick,
                                   h->stream));
        }
        // :45-72 the low level's action under the goal; frame t recorded with its goal and distance (and the env
        // reward / mask of frame t-1)
        const MlpRecord rec{ h->exp.action, h->exp.log_prob, h->exp.value, h->exp.mask, h->xc.env_reward,
                             h->exp.cur_mask, h->p.reward, nullptr, h->p.done_out, T, t, h->n_env };
        const MlpAction act{ 1, step_index, policy_seed, env_index0, h->p.actions, rec };
        xr.lo_goal = h->xc.lo_goal;
        xr.lo_dist = h->xc.dist;
        HIP_TRY(launch_xy_low(h->xy, h->p, h->sst, h->xy_goal, h->mlp_mu, h->mlp_std, h->mlp_value, act, h->stream, &xr));
        frames.write_next(t, T);
        // :51-54 step_no_reset inside a window, step on its last frame
        HIP_TRY(launch_step(h->p, h->p.actions, (t + 1) % L == 0 ? 1 : 0, no_policy(), h->stream));
        h->step_count += 1;
    }
    {   // the env reward of frame T-1 and self.lo_mask = 1 - done
        ExpBuffers last = h->exp;
        last.reward = h->xc.env_reward;
        HIP_TRY(launch_exp_reward(last, h->n_env, T - 1, h->p.reward, nullptr, h->p.done_out, h->stream));
    }
    // :98-105 next_hi_value = V_hi(obs_T); g' ~ hi_dist(obs_T) on a stream of its own; next_lo_value = V_lo(obs_T, g')
    const XyPick boot{ 2, L, (uint32_t)h->step_count, policy_seed, env_index0, 1, h->xc.boot, XyRecord{} };
    HIP_TRY(launch_xy_high(h->xy, h->p, h->sst, h->xy_goal, h->xy_goal_mu, h->xy_goal_std, h->xy_value, boot, h->stream));
    HIP_TRY(launch_xy_low(h->xy, h->p, h->sst, h->xc.boot, h->mlp_mu, h->mlp_std, h->mlp_value, no_mlp_action(),
                          h->stream, nullptr, 1));
    // :128-131 the low level's reward from the recorded distances, :123-134 its GAE over all T frames; :111-120 the
    // high level per env over its windows
    HIP_TRY(launch_xy_lo_reward(h->exp.reward, h->xc.dist, h->exp.mask, T, L, h->n_env, h->stream));
    HIP_TRY(launch_exp_gae(h->exp, h->n_env, h->mlp_value, discount, gae_lambda, h->stream));
    HIP_TRY(launch_skill_hi_gae(o, T, L, h->n_env, h->xc.env_reward, h->exp.mask, h->exp.cur_mask, h->xy_value,
                                gae_lambda, h->xc.count, h->stream));
    h->exp_xy = true;
    h->eplog.source = 5;
    return ZENV_OK;
}

// ---- zenv_collect_option: collect_experiences of the Options agent (options/src/torch_ac/algos/_hier_policy_opt.py:
// 10-205).  The per-frame records for T frames that zenv_collect_hier's (ensure_hier_collect) have no place for
static int ensure_option_collect(zenv_t *h, int T)
{
    if (h->oc_mem && h->oc.T == T) return ZENV_OK;
    const size_t TN = (size_t)T * h->n_env;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->oc_mem) HIP_TRY(hipFree(h->oc_mem));
    h->oc_mem = nullptr;
    Carver cv;
    cv.piece(h->oc.lo_skill, TN);
    cv.piece(h->oc.term_action, TN);
    cv.piece(h->oc.term_log_prob, TN);
    cv.piece(h->oc.ended, TN);
    if (int rc = cv.alloc(&h->oc_mem, "option record")) return rc;
    HIP_TRY(hipMemsetAsync(h->oc_mem, 0, cv.bytes(), h->stream));
    h->oc.T = T;
    return ZENV_OK;
}

extern "C" int zenv_collect_option(zenv_t *h, int T, uint64_t policy_seed, uint64_t env_index0, float discount,
                                   float gae_lambda, int64_t *n_hi)
{
    if (T < 2) return fail(ZENV_E_ARG, "frames_per_proc must be at least 2 (the low level hands out T - 1 frames)");
    int rc = collect_ready(h, "zenv_collect_option", T, T, discount, gae_lambda);   // every frame auto-resets
    if (rc) return rc;
    if (h->order_enabled || h->goal_enabled)
        return fail(ZENV_E_STATE, "zenv_collect_option steps a plain task handle, not a goal-conditioned / solver-ordered one");
    if (!h->option_ready) return fail(ZENV_E_STATE, "zenv_option_load first");
    if (!h->skill.hi_critic || !h->skill.lo_critic)
        return fail(ZENV_E_STATE, "zenv_collect_option needs both critics (zenv_option_load with hi_critic_* and lo_critic_*)");
    if (int rc = use_device(h)) return rc;
    const size_t N = (size_t)h->n_env, ZF = (size_t)h->p.Z * h->p.F;
    h->act_tag.valid = false;
    h->hi_m = 0;
    h->hi_kind = 2;
    if (int rc = ensure_exp(h, T)) return rc;
    if (int rc = ensure_hier_collect(h, T, false)) return rc;
    if (int rc = ensure_option_collect(h, T)) return rc;
    const HierFrames &f = h->hframes;
    const HierCarry &c = h->hcarry;
    HIP_TRY(hipMemsetAsync(f.pick_goal, 0xFF, (size_t)T * N * 4, h->stream));     // -1: no pick
    HIP_TRY(hipMemsetAsync(f.close_flag, 0, (size_t)T * N, h->stream));
    HIP_TRY(hipMemsetAsync(f.count, 0, N * 4, h->stream));
    // the skill state as the policy would find it; an env that enters without a skill has no transition open
    HIP_TRY(launch_skill_sync(h->p, h->sst, nullptr, 0, h->stream));
    HIP_TRY(launch_option_enter(h->sst, c, h->n_env, h->stream));
    const FrameObs frames(h);
    if (int rc = frames.begin()) return rc;
    for (int t = 0; t < T; ++t) {
        frames.read(t);
        const uint32_t step_index = (uint32_t)h->step_count;
        const OptionRecord orec{ t, h->n_env, f.pick_goal, f.pick_value, f.pick_log_prob, c.open, h->oc.lo_skill,
                                 h->oc.term_action, h->oc.term_log_prob, h->oc.ended };
        // :17-40 a skill for the envs without one (zenv_policy(ZENV_POLICY_OPTION_SAMPLE)'s launches), the pick recorded
        const OptionPick pick{ 1, h->option_compact, step_index, policy_seed, env_index0 };
        if (pick.compact) HIP_TRY(launch_option_list(h->p, h->sst, h->olist, h->stream));
        HIP_TRY(launch_option_high(h->skill, h->p, h->sst, h->olist, h->skill_logits, h->skill_value, pick, h->stream,
                                   orec));
        // :42-63 the low level's action and the termination draw; frame t recorded (and reward / mask of frame t-1)
        const MlpRecord rec{ h->exp.action, h->exp.log_prob, h->exp.value, h->exp.mask, h->exp.reward, h->exp.cur_mask,
                             h->p.reward, nullptr, h->p.done_out, T, t, h->n_env };
        const MlpAction act{ 1, step_index, policy_seed, env_index0, h->p.actions, rec };
        HIP_TRY(launch_option_low(h->skill, h->p, h->sst, h->olist, h->mlp_mu, h->mlp_std, h->mlp_value, h->oterm, act,
                                  h->stream, orec));
        frames.write_next(t, T);
        HIP_TRY(launch_step(h->p, h->p.actions, 1, no_policy(), h->stream));      // self.env.step (:50): auto-reset
        HIP_TRY(launch_option_close(h->p, h->sst, f, c, t, h->stream));           // :65-75, and the skill's episode index
        h->step_count += 1;
    }
    HIP_TRY(launch_exp_reward(h->exp, h->n_env, T - 1, h->p.reward, nullptr, h->p.done_out, h->stream));
    // next_hi_val = V_hi(obs_T) (:95-97) of every env, into ZENV_F_SKILL_VALUE; nothing is picked
    const OptionPick value_only{ -1, 0, 0u, 0ull, 0ull };
    HIP_TRY(launch_option_high(h->skill, h->p, h->sst, h->olist, h->skill_logits, h->skill_value, value_only, h->stream));
    // :111-118 the low level over frames 0 .. T-2, no bootstrap: frame T-1 is only the "next" frame of T-2
    ExpBuffers lo = h->exp;
    lo.T = T - 1;
    lo.cur_mask = h->exp.mask + (size_t)(T - 1) * N;
    HIP_TRY(launch_exp_gae(lo, h->n_env, h->exp.value + (size_t)(T - 1) * N, discount, gae_lambda, h->stream));
    HIP_TRY(hipMemsetAsync(h->exp.advantage + (size_t)(T - 1) * N, 0, N * 4, h->stream));
    HIP_TRY(hipMemsetAsync(h->exp.returnn + (size_t)(T - 1) * N, 0, N * 4, h->stream));
    // :100-108 the high level's rows: offsets, then M to the host (the one synchronisation of the call)
    HIP_TRY(launch_hier_count_scan(f, h->n_env, h->stream));
    HIP_TRY(hipMemcpyAsync(h->hi_total_host, f.total, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int64_t M = *h->hi_total_host;
    if (int rc = ensure_hier_out(h, M)) return rc;
    HierOut rows = h->hout;
    rows.action_mask = nullptr;                                  // every skill is always available: no mask
    HIP_TRY(launch_hier_gae(f, c, rows, h->n_env, h->skill_value, gae_lambda, h->stream));
    HIP_TRY(launch_hier_gather(rows, c, h->exp.obs, h->exp.zone_obs, M, h->n_env, h->p.Z, h->p.F, h->stream));
    HIP_TRY(launch_hier_carry(c, h->exp.obs, h->exp.zone_obs, h->n_env, (int)ZF, h->stream));
    h->hi_m = M;
    h->exp_option = true;
    h->eplog.source = 4;
    if (n_hi) *n_hi = M;
    return ZENV_OK;
}

extern "C" int zenv_policy(zenv_t *h, int policy, uint64_t policy_seed, uint64_t env_index0, float *dst_device)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    if (!h->was_reset) return fail(ZENV_E_STATE, "reset before asking for actions");
    const bool hier = policy == ZENV_POLICY_HIER_SAMPLE || policy == ZENV_POLICY_HIER_MEAN;
    const bool skill = policy == ZENV_POLICY_SKILL_SAMPLE || policy == ZENV_POLICY_SKILL_MEAN;
    const bool option = policy == ZENV_POLICY_OPTION_SAMPLE || policy == ZENV_POLICY_OPTION_MEAN;
    const bool xy = policy == ZENV_POLICY_XY_SAMPLE || policy == ZENV_POLICY_XY_MEAN;
    if (!policy_known(policy) && !hier && !skill && !option && !xy) return fail(ZENV_E_ARG, "unknown policy %d", policy);
    if (int rc = use_device(h)) return rc;
    const StepPolicy pol{ policy, (uint32_t)h->step_count, policy_seed, env_index0,
                          dst_device ? dst_device : h->p.actions };
    h->act_tag.valid = false;
    if (hier) return run_hier_policy(h, policy, pol.step_index, policy_seed, env_index0, pol.out);
    if (skill) return run_skill_policy(h, policy, pol.step_index, policy_seed, env_index0, pol.out);
    if (option) return run_option_policy(h, policy, pol.step_index, policy_seed, env_index0, pol.out);
    if (xy) return run_xy_policy(h, policy, pol.step_index, policy_seed, env_index0, pol.out);
    return run_policy(h, pol);
}
