// zenv_train.cpp -- the learners behind the C ABI of include/zenv.h: the flat actor-critic's PPO update on the handle's own
// experience buffers (zenv_ppo_*) and the Zone-goals agent's two (zenv_hppo_*, level 0 = low, 1 = high) on the records
// of zenv_collect_hier, the xy-goals agent's two (zenv_xyppo_*, the same levels) on the records of zenv_collect_xy, and
// the fixed-length-skills agent's two (zenv_skppo_*) on the records of zenv_collect_skill, and the Options agent's two
// (zenv_opppo_*) on the records of zenv_collect_option, and DIAYN's inverse model's (zenv_diayn_*, no level) on the
// records of zenv_collect_skill, with the kept-sample list and the learned skill prior's step beside it; and the flat
// actor-critic's A2C update (zenv_a2c_*) on the same buffers as zenv_ppo_*, a learner of its own beside it.
// One PpoState each, the same code.  The kernels: ppo_update.hip.  The networks that act and collect: zenv_agents.cpp.
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
    float *stats = nullptr;         // ZENV_F_PPO_STATS / ZENV_F_HPPO_*_STATS / ZENV_F_XYPPO_*_STATS / ZENV_F_SKPPO_*_STATS /
                                    // ZENV_F_OPPPO_*_STATS
                                    // [stats_cap][6]
    int stats_cap = 0, stats_rows = 0;
    // the A2C learner (zenv_a2c_*): square_avg lies in the exp_avg arena, the fourth arena is not used
    double rms_alpha = 0.0, rms_eps = 0.0;
    int64_t acc_total = 0;          // the frames the open accumulation's means divide by; 0: none since the init
    int32_t *iota = nullptr;        // zenv_a2c_update: the indexes 0 .. iota_n on the device
    int64_t iota_n = 0;
};

namespace {

// which network a learner trains: the width of its per-sample input, its head and what the head's loss is taken of
struct NetKind {
    int XD, head, loss;
    int S = 0;                      // the fixed-length-skills and Options agents' learners: the number of skills
    int NA = 2;                     // the Gaussian head's action components: 3 for the Options agent's low level
    int a2c = 0;                    // the flat network under the A2C learner: the head's five deltas also lie in DZ
    // XD + F + 1 <= 16 / 18 columns, rounded up to 8; the skills agent's low level: 8 + S + F + 1 <= 48 of them
    int w1c(int F) const { return S && XD > 8 ? (XD + F + 1 + 7) / 8 * 8 : XD == 8 ? 16 : 24; }
    // the skills agent's low level: actor.enc_.0.0 and critic.0 read [emb, onehot], S columns more
    int tail() const { return S && XD > 8 ? S : 0; }
    // the flat actor-critic's learner; every other one belongs to a hierarchical agent
    bool flat() const { return XD == 8 && head == PPO_HEAD_GAUSSIAN && loss == PPO_LOSS_ACTION; }
};
constexpr NetKind kFlat{ 8, PPO_HEAD_GAUSSIAN, PPO_LOSS_ACTION }, kHierLo{ 10, PPO_HEAD_GAUSSIAN, PPO_LOSS_ACTION },
    kHierHi{ 8, PPO_HEAD_ZONES, PPO_LOSS_ACTION };
// the xy-goals agent: its low level is the Zone-goals low level, its high level the flat network under the joint loss
constexpr NetKind kXyLo = kHierLo, kXyHi{ 8, PPO_HEAD_GAUSSIAN, PPO_LOSS_JOINT_GOAL };
// the fixed-length-skills agent: the Gaussian network on [obs, onehot(skill)], and the flat encoder under a Categorical
NetKind sk_lo(int S) { return NetKind{ 8 + S, PPO_HEAD_GAUSSIAN, PPO_LOSS_ACTION, S }; }
NetKind sk_hi(int S) { return NetKind{ 8, PPO_HEAD_SKILLS, PPO_LOSS_ACTION, S }; }
// the Options agent: the skills agent's high level as it stands (sk_hi), its low level with a third action component
NetKind op_lo(int S) { return NetKind{ 8 + S, PPO_HEAD_GAUSSIAN, PPO_LOSS_ACTION, S, 3 }; }
// DIAYN's inverse model: the flat encoder with a ReLU on it under an S-way head, no enc_ layer and no critic
NetKind inv_kind(int S) { return NetKind{ 8, PPO_HEAD_INVERSE, PPO_LOSS_ACTION, S }; }
// the flat network under A2C's loss (zenv_a2c_*)
constexpr NetKind kA2c{ 8, PPO_HEAD_GAUSSIAN, PPO_LOSS_ACTION, 0, 2, 1 };

// element counts of the tensors for hidden size h and zone rows of F features: zenv_mlp_weights' member order (20; the
// Zone-goals low level's 18 with XD = 10; the skills agent's low level's 18 with XD = 8 + S and [h, h + S] in
// actor.enc_.0.0 and critic.0; the Options agent's the same with [3, h] / [3] in actor.mu_ / actor.std_), or the 16 of
// zenv_hier_weights' hi_* members, or the 16 of zenv_skill_weights' / zenv_option_weights'
void tensor_counts(int h, int F, NetKind k, int64_t (&count)[PPO_MAX_TENSORS])
{
    const int64_t hh = (int64_t)h * h, X = k.XD, he = (int64_t)h * (h + k.tail()), S = k.S, A = k.NA;
    const int64_t c[PPO_MAX_TENSORS] = { h * (X + F), h, hh, h, hh, h, h * (X + h), h, he, h, A * h, A,
                                         A * h, A, he, h, h, 1, h, 1 };
    const int64_t z[PPO_MAX_TENSORS] = { h * (X + F), h, hh, h, hh, h, h * (X + h), h, (int64_t)h * (h + F), h, h, 1,
                                         hh, h, h, 1, 0, 0, 0, 0 };
    const int64_t d[PPO_MAX_TENSORS] = { h * (X + F), h, hh, h, hh, h, h * (X + h), h, hh, h, S * h, S,
                                         hh, h, h, 1, 0, 0, 0, 0 };
    // zenv_skill_inverse_weights' 10: the encoder's eight, combine_net.2 [S, h] / [S]
    const int64_t v[PPO_MAX_TENSORS] = { h * (X + F), h, hh, h, hh, h, h * (X + h), h, S * h, S };
    const int64_t *src = k.head == PPO_HEAD_ZONES ? z : k.head == PPO_HEAD_SKILLS ? d : k.head == PPO_HEAD_INVERSE ? v : c;
    std::copy(src, src + PPO_MAX_TENSORS, count);
}

void tensor_list(const zenv_mlp_weights *w, const float *(&t)[PPO_MAX_TENSORS])
{
    const float *l[PPO_MAX_TENSORS] = { w->zone_w1, w->zone_b1, w->zone_w2, w->zone_b2, w->zone_w3, w->zone_b3, w->comb_w,
                                        w->comb_b, w->enc_w, w->enc_b, w->mu_w, w->mu_b, w->std_w, w->std_b, w->critic_w1,
                                        w->critic_b1, w->critic_w2, w->critic_b2, w->critic_sigma_w, w->critic_sigma_b };
    std::copy(l, l + PPO_MAX_TENSORS, t);
}

struct Layout {
    int HP, KC, LDC, rp, bp;
    int64_t chunks;
    // floats of every workspace piece, in carving order
    int64_t img[PPO_N_IMAGES], a1, p, hd, c, ci, pre, ss, partial, u, l, dz;
    int64_t total;
};

Layout layout_for(int h, int Z, int F, int max_batch, NetKind k)
{
    Layout l{};
    l.HP = (h + 32) / 32 * 32;          // h <= 191: at least one padded column, the constant's
    l.KC = l.HP + (k.XD + 7) / 8 * 8;
    l.LDC = k.tail() ? l.HP + 32 : l.HP;
    const int64_t rp = ((int64_t)max_batch * Z + 31) / 32 * 32, bp = ((int64_t)max_batch + 31) / 32 * 32;
    l.rp = (int)std::min<int64_t>(rp, INT32_MAX);
    l.bp = (int)std::min<int64_t>(bp, INT32_MAX);
    l.chunks = (rp + kPpoChunk - 1) / kPpoChunk;
    const int64_t HP = l.HP, KC = l.KC;
    for (int i = 0; i < PPO_N_IMAGES; ++i) l.img[i] = HP * HP;
    l.img[PPO_I_W1] = HP * k.w1c(F);
    l.img[PPO_I_WC] = HP * KC;
    l.img[PPO_I_WE] = l.img[PPO_I_WV] = HP * l.LDC;
    l.img[PPO_I_HA] = l.img[PPO_I_HV] = 32 * HP;
    l.img[PPO_T_HA] = l.img[PPO_T_HV] = HP * 32;
    // DIAYN's inverse model has no enc_ layer and no critic: no image of theirs, no Ha / Hc, no PRE / DH
    const bool inverse = k.head == PPO_HEAD_INVERSE;
    if (inverse)
        for (int i : { PPO_I_WE, PPO_I_WV, PPO_I_HV, PPO_T_WE, PPO_T_WV, PPO_T_HV }) l.img[i] = 0;
    l.a1 = rp * HP;
    l.p = bp * HP;
    l.hd = inverse ? 0 : bp * HP;
    l.c = bp * l.LDC;
    l.ci = bp * KC;
    l.pre = inverse ? 0 : bp * 32;
    l.ss = bp * 8;
    // the widest product of the learner: a partial is [HP][its columns rounded up to 32]; HP + 32 covers every product
    // but combine_net_'s, whose KC columns pass HP + 32 once the own ones pass 32 (the skills agent, S > 24)
    l.partial = l.chunks * HP * std::max<int64_t>(HP + 32, (KC + 31) / 32 * 32);
    if (k.head == PPO_HEAD_ZONES) l.u = rp * HP, l.l = rp * 32;
    if (k.head == PPO_HEAD_SKILLS || inverse) l.l = bp * 32;       // the S logits of a sample, their deltas
    // DZ, in floats: a double per zone row (the per-zone head), or 2 NA + 1 per sample (the skills and Options agents' low
    // level), or S per sample (the inverse model), or five per sample (the A2C learner)
    l.dz = k.tail() ? bp * 2 * (2 * k.NA + 1) : inverse ? bp * 2 * k.S : k.a2c ? bp * 2 * 5 : l.l / 16;
    l.total = 2 * l.a1 + l.p + 2 * l.hd + l.c + l.ci + 2 * l.pre + l.ss + l.partial + l.u + 2 * l.l + l.dz;
    for (int i = 0; i < PPO_N_IMAGES; ++i) l.total += l.img[i];
    return l;
}

bool bad_hyper(double v) { return !std::isfinite(v) || v < 0.0; }

// the rules every learner's tensors and settings follow (t: the learner's tensors in arena order)
int learner_check(const zenv_config *cfg, int h_dim, const float *const *t, NetKind k, const zenv_ppo_config *pc,
                  const char *who)
{
    if (h_dim < 1 || h_dim > 191) return fail(ZENV_E_ARG, "%sh_dim %d outside [1, 191]", who, h_dim);
    if (cfg->num_zones < 1 || cfg->num_zones > ZENV_MAX_ZONES)
        return fail(ZENV_E_ARG, "num_zones %d outside [1, %d]", cfg->num_zones, ZENV_MAX_ZONES);
    const bool inverse = k.head == PPO_HEAD_INVERSE;    // ten tensors, no critic
    const int critic = inverse ? PPO_INV_TENSORS : k.head != PPO_HEAD_GAUSSIAN ? PPO_CRITIC_W1 - 2 : PPO_CRITIC_W1;
    for (int i = 0; i < critic; ++i)
        if (!t[i]) return fail(ZENV_E_ARG, "%sa tensor of the weights is null", who);
    for (int i = critic; i < critic + (inverse ? 0 : 4); ++i)
        if (!t[i]) return fail(ZENV_E_ARG, "%sthe update needs the critic: critic_w1 / _b1 / _w2 / _b2", who);
    const bool hier = !k.flat();
    if (hier && pc->distributional_value)
        return fail(ZENV_E_ARG, "%sdistributional_value must be 0: the hierarchical agents' critics are plain", who);
    for (double v : { pc->lr, pc->adam_eps, pc->clip_eps, pc->entropy_coef, pc->value_loss_coef })
        if (bad_hyper(v)) return fail(ZENV_E_ARG, "%sa hyper-parameter is negative or not finite (%g)", who, v);
    // the hierarchical agents' references take the norm and do not clip: +inf stands for that
    if (bad_hyper(pc->max_grad_norm) && !(hier && pc->max_grad_norm == INFINITY))
        return fail(ZENV_E_ARG, "%sa hyper-parameter is negative or not finite (%g)", who, pc->max_grad_norm);
    if (pc->max_batch < 1) return fail(ZENV_E_ARG, "%smax_batch must be >= 1", who);
    const Layout l = layout_for(h_dim, cfg->num_zones, zenv_zone_feat(cfg), pc->max_batch, k);
    if (l.total >= ((int64_t)1 << 31))
        return fail(ZENV_E_ARG, "%smax_batch %d x %d zones needs a workspace of %lld floats, the limit is 2^31: use smaller "
                    "minibatches", who, pc->max_batch, cfg->num_zones, (long long)l.total);
    return ZENV_OK;
}

// the low level's tensors: zenv_hier_weights, zenv_xy_weights, zenv_skill_weights and zenv_option_weights name them alike
template <class W>
void lo_tensor_list(const W *w, const float *(&t)[PPO_MAX_TENSORS])
{
    const float *l[PPO_MAX_TENSORS] = { w->lo_zone_w1, w->lo_zone_b1, w->lo_zone_w2, w->lo_zone_b2, w->lo_zone_w3,
                                        w->lo_zone_b3, w->lo_comb_w, w->lo_comb_b, w->lo_enc_w, w->lo_enc_b, w->lo_mu_w,
                                        w->lo_mu_b, w->lo_std_w, w->lo_std_b, w->lo_critic_w1, w->lo_critic_b1,
                                        w->lo_critic_w2, w->lo_critic_b2, nullptr, nullptr };
    std::copy(l, l + PPO_MAX_TENSORS, t);
}

// the high level's, once per naming: the Zone-goals agent's per-zone actor, ...
void hi_tensor_list(const zenv_hier_weights *w, const float *(&t)[PPO_MAX_TENSORS])
{
    const float *u[PPO_MAX_TENSORS] = { w->hi_zone_w1, w->hi_zone_b1, w->hi_zone_w2, w->hi_zone_b2, w->hi_zone_w3,
                                        w->hi_zone_b3, w->hi_comb_w, w->hi_comb_b, w->hi_actor_w1, w->hi_actor_b1,
                                        w->hi_actor_w2, w->hi_actor_b2, w->hi_critic_w1, w->hi_critic_b1, w->hi_critic_w2,
                                        w->hi_critic_b2, nullptr, nullptr, nullptr, nullptr };
    std::copy(u, u + PPO_MAX_TENSORS, t);
}

// ... the xy-goals agent's flat network, ...
void hi_tensor_list(const zenv_xy_weights *w, const float *(&t)[PPO_MAX_TENSORS])
{
    const float *u[PPO_MAX_TENSORS] = { w->hi_zone_w1, w->hi_zone_b1, w->hi_zone_w2, w->hi_zone_b2, w->hi_zone_w3,
                                        w->hi_zone_b3, w->hi_comb_w, w->hi_comb_b, w->hi_enc_w, w->hi_enc_b, w->hi_mu_w,
                                        w->hi_mu_b, w->hi_std_w, w->hi_std_b, w->hi_critic_w1, w->hi_critic_b1,
                                        w->hi_critic_w2, w->hi_critic_b2, nullptr, nullptr };
    std::copy(u, u + PPO_MAX_TENSORS, t);
}

// ... and the skill head of zenv_skill_weights and zenv_option_weights, the same members
template <class W>
void hi_tensor_list(const W *w, const float *(&t)[PPO_MAX_TENSORS])
{
    const float *u[PPO_MAX_TENSORS] = { w->hi_zone_w1, w->hi_zone_b1, w->hi_zone_w2, w->hi_zone_b2, w->hi_zone_w3,
                                        w->hi_zone_b3, w->hi_comb_w, w->hi_comb_b, w->hi_enc_w, w->hi_enc_b,
                                        w->hi_logit_w, w->hi_logit_b, w->hi_critic_w1, w->hi_critic_b1, w->hi_critic_w2,
                                        w->hi_critic_b2, nullptr, nullptr, nullptr, nullptr };
    std::copy(u, u + PPO_MAX_TENSORS, t);
}

// the number of skills the weights are of; the goal agents have none
template <class W>
int skills_of(const W *w) { return w->n_skills; }
int skills_of(const zenv_hier_weights *) { return 0; }
int skills_of(const zenv_xy_weights *) { return 0; }

// ---- the learner families: what the entry points zenv_<name>_* have in common
enum { AGENT_FLAT = 0, AGENT_HIER, AGENT_XY, AGENT_SKILL, AGENT_OPTION, AGENT_DIAYN, AGENT_A2C, N_AGENTS };

struct Family {
    const char *name;               // "zenv_<name>_init first"
    int first;                      // its LearnerSlot; with levels: the low level's, the high level's is the next
    bool levels;                    // a pair: the entry points take level 0 (low) or 1 (high)
    bool skills;                    // its weights carry n_skills
    bool net_rows;                  // trains on the rows the flat network reads (net_row_feat), not the handle's p.F
    int arenas;                     // the arenas `which` may name: Adam's four, RMSprop's three
    NetKind (*kind[2])(int S);      // the network of each level (the one of a family without levels in [0])
};
const Family kFamily[N_AGENTS] = {
    { "ppo", L_FLAT, false, false, true, 4, { [](int) { return kFlat; }, nullptr } },
    { "hppo", L_HIER_LO, true, false, false, 4, { [](int) { return kHierLo; }, [](int) { return kHierHi; } } },
    { "xyppo", L_XY_LO, true, false, false, 4, { [](int) { return kXyLo; }, [](int) { return kXyHi; } } },
    { "skppo", L_SKILL_LO, true, true, false, 4, { sk_lo, sk_hi } },
    { "opppo", L_OPTION_LO, true, true, false, 4, { op_lo, sk_hi } },
    { "diayn", L_DIAYN, false, true, false, 4, { inv_kind, nullptr } },
    { "a2c", L_A2C, false, false, true, 3, { [](int) { return kA2c; }, nullptr } },
};
static_assert(ZENV_PPO_PARAM == 0 && ZENV_PPO_EXP_AVG_SQ == 3 && ZENV_A2C_PARAM == 0 && ZENV_A2C_SQUARE_AVG == 2,
              "Family::arenas");

int check_skills(int n_skills)
{
    if (n_skills < 1 || n_skills > kMaxSkills) return fail(ZENV_E_ARG, "n_skills %d outside [1, %d]", n_skills, kMaxSkills);
    return ZENV_OK;
}

int check_zone_feat(const zenv_config *cfg, int zone_feat)
{
    if (zone_feat != zenv_zone_feat(cfg))
        return fail(ZENV_E_ARG, "zone_feat %d: the handle's zone rows have %d features", zone_feat, zenv_zone_feat(cfg));
    return ZENV_OK;
}

// zenv_hppo_check / _xyppo_ / _skppo_ / _opppo_: the two levels of a pair's weights
template <class W>
int pair_check(int agent, const zenv_config *cfg, const W *w, const zenv_ppo_config *lo, const zenv_ppo_config *hi)
{
    if (!cfg || !w || !lo || !hi) return fail(ZENV_E_ARG, "null argument");
    const Family &f = kFamily[agent];
    if (f.skills)
        if (int rc = check_skills(skills_of(w))) return rc;
    if (int rc = check_zone_feat(cfg, w->zone_feat)) return rc;
    const float *tl[PPO_MAX_TENSORS], *th[PPO_MAX_TENSORS];
    lo_tensor_list(w, tl);
    hi_tensor_list(w, th);
    if (int rc = learner_check(cfg, w->h_dim, tl, f.kind[0](skills_of(w)), lo, "low level: ")) return rc;
    return learner_check(cfg, w->h_dim, th, f.kind[1](skills_of(w)), hi, "high level: ");
}

}  // namespace

extern "C" int zenv_ppo_check(const zenv_config *cfg, const zenv_mlp_weights *w, const zenv_ppo_config *pc)
{
    if (!cfg || !w || !pc) return fail(ZENV_E_ARG, "null argument");
    const float *t[PPO_MAX_TENSORS];
    tensor_list(w, t);
    if (int rc = learner_check(cfg, w->h_dim, t, kFlat, pc, "")) return rc;
    const int n_sigma = (w->critic_sigma_w != nullptr) + (w->critic_sigma_b != nullptr);
    if (pc->distributional_value && n_sigma != 2)
        return fail(ZENV_E_ARG, "distributional_value needs critic_sigma_w and critic_sigma_b");
    if (!pc->distributional_value && n_sigma != 0)
        return fail(ZENV_E_ARG, "critic_sigma_* given without distributional_value");
    return ZENV_OK;
}

extern "C" int zenv_hppo_check(const zenv_config *cfg, const zenv_hier_weights *w, const zenv_ppo_config *lo,
                               const zenv_ppo_config *hi)
{
    return pair_check(AGENT_HIER, cfg, w, lo, hi);
}

extern "C" int zenv_xyppo_check(const zenv_config *cfg, const zenv_xy_weights *w, const zenv_ppo_config *lo,
                                const zenv_ppo_config *hi)
{
    return pair_check(AGENT_XY, cfg, w, lo, hi);
}

extern "C" int zenv_skppo_check(const zenv_config *cfg, const zenv_skill_weights *w, const zenv_ppo_config *lo,
                                const zenv_ppo_config *hi)
{
    return pair_check(AGENT_SKILL, cfg, w, lo, hi);
}

extern "C" int zenv_opppo_check(const zenv_config *cfg, const zenv_option_weights *w, const zenv_ppo_config *lo,
                                const zenv_ppo_config *hi)
{
    return pair_check(AGENT_OPTION, cfg, w, lo, hi);
}

static void inverse_tensor_list(const zenv_skill_inverse_weights *w, const float *(&t)[PPO_MAX_TENSORS])
{
    const float *l[PPO_MAX_TENSORS] = { w->zone_w1, w->zone_b1, w->zone_w2, w->zone_b2, w->zone_w3, w->zone_b3,
                                        w->comb_w1, w->comb_b1, w->comb_w2, w->comb_b2 };
    std::copy(l, l + PPO_MAX_TENSORS, t);
}

extern "C" int zenv_diayn_check(const zenv_config *cfg, const zenv_skill_inverse_weights *w, const zenv_ppo_config *pc)
{
    if (!cfg || !w || !pc) return fail(ZENV_E_ARG, "null argument");
    if (int rc = check_skills(w->n_skills)) return rc;
    if (int rc = check_zone_feat(cfg, w->zone_feat)) return rc;
    if (w->precision != ZENV_MLP_F32) return fail(ZENV_E_ARG, "precision %d: the inverse model is float32 only", w->precision);
    const float *t[PPO_MAX_TENSORS];
    inverse_tensor_list(w, t);
    return learner_check(cfg, w->h_dim, t, inv_kind(w->n_skills), pc, "inverse model: ");
}

static void learner_free(PpoState *&s)
{
    if (!s) return;
    for (void *m : { s->arena_mem, s->ws_mem, (void *)s->idx, (void *)s->stats, (void *)s->iota })
        if (m) (void)hipFree(m);
    if (s->net.bad_index) (void)hipHostFree(s->net.bad_index);
    delete s;
    s = nullptr;
}

void ppo_free_flat(zenv *h)
{
    for (const Family &f : kFamily)
        if (f.net_rows) learner_free(h->learner[f.first]);
}

void ppo_free(zenv *h)
{
    for (PpoState *&s : h->learner) learner_free(s);
    if (h->diayn_mem) (void)hipFree(h->diayn_mem);
    if (h->diayn_counts) (void)hipFree(h->diayn_counts);
    if (h->diayn_flag) (void)hipHostFree(h->diayn_flag);
    h->diayn_mem = nullptr, h->diayn_list = h->diayn_blocks = h->diayn_counts = nullptr, h->diayn_flag = nullptr;
    h->diayn_cap = 0, h->diayn_kept = -1;
    h->prior.ready = false;
}

int ppo_index_check(zenv *h)
{
    bool bad = false;
    for (PpoState *s : h->learner)
        if (s && s->net.bad_index && *(volatile int *)s->net.bad_index) {
            *(volatile int *)s->net.bad_index = 0;
            bad = true;
        }
    if (h->diayn_flag && *(volatile int *)h->diayn_flag) {      // the skill prior's histogram met a pick outside [0, S)
        *(volatile int *)h->diayn_flag = 0;
        bad = true;
    }
    if (!bad) return ZENV_OK;
    return fail(ZENV_E_ARG, "a device-resident minibatch index lay outside [0, envs x frames), or a recorded goal was "
                            "not among its row's available goals, or a recorded skill lay outside [0, n_skills), or the inverse model's sample was one the collection did not keep: the sample was dropped and the update since the last "
                            "synchronising call is invalid");
}

void *ppo_stats(const zenv *h, int slot, int64_t *bytes)
{
    const PpoState *s = h->learner[slot];
    *bytes = s ? (int64_t)s->stats_rows * (slot == L_A2C ? kA2cStats : kPpoStats) * 4 : 0;
    return s ? s->stats : nullptr;
}

// a learner of kind k in the family's slot of `level` (replacing what is there) from the tensors t in arena order;
// checked by the caller
static int learner_create(zenv *h, int agent, int level, int h_dim, const float *const *t, NetKind k,
                          const zenv_ppo_config *pc)
{
    if (int rc = use_device(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    PpoState *&slot = h->learner[kFamily[agent].first + level];
    learner_free(slot);
    PpoState *s = new PpoState();
    slot = s;
    PpoNet &n = s->net;
    // the flat learners train on the rows the flat network reads (zenv_order_rows: 7 wide on a solver-ordered handle)
    const int F = kFamily[agent].net_rows ? net_row_feat(h) : h->p.F;
    const Layout l = layout_for(h_dim, h->p.Z, F, pc->max_batch, k);
    n.h = h_dim, n.HP = l.HP, n.F = F, n.Z = h->p.Z, n.K1 = k.XD + F, n.KC = l.KC;
    n.XD = k.XD, n.W1C = k.w1c(F), n.head = k.head, n.loss = k.loss, n.S = k.S, n.NA = k.NA, n.LDC = l.LDC;
    const bool inverse = k.head == PPO_HEAD_INVERSE;    // no critic: cr names a tensor that exists and is never read
    n.cr = inverse ? 0 : k.head != PPO_HEAD_GAUSSIAN ? PPO_CRITIC_W1 - 2 : PPO_CRITIC_W1;
    n.split_reduce = k.flat() ? 0 : 1;                  // the hierarchical agents' learners
    n.dist = pc->distributional_value ? 1 : 0;
    n.n_tensors = inverse ? PPO_INV_TENSORS : k.head != PPO_HEAD_GAUSSIAN ? 16 : n.dist ? 20 : 18;
    n.max_batch = pc->max_batch;
    s->lr = pc->lr;
    n.hyper = PpoHyper{ (float)pc->lr, (float)pc->adam_eps, (float)pc->clip_eps, (float)pc->entropy_coef,
                        (float)pc->value_loss_coef, (float)pc->max_grad_norm };
    tensor_counts(n.h, n.F, k, n.count);
    int64_t at = 0;
    for (int i = 0; i < PPO_MAX_TENSORS; ++i) {         // every tensor starts on a 256-byte boundary
        n.off[i] = at;
        if (i < n.n_tensors) at += (n.count[i] + 63) / 64 * 64;
        else n.count[i] = 0;
    }
    n.arena = at;
    // ---- the four arenas
    std::vector<float> host((size_t)n.arena, 0.f);
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
    n.P = take(l.p), n.C = take(l.c), n.Ha = take(l.hd), n.Hc = take(l.hd);
    n.CI = take(l.ci);
    n.PRE = take(l.pre), n.DH = take(l.pre);
    n.SS = take(l.ss);
    n.partial = take(l.partial);
    n.U = take(l.u), n.L = take(l.l), n.DL = take(l.l);
    n.DZ = reinterpret_cast<double *>(take(l.dz));          // doubles; every piece before it is a multiple of 32 floats
    n.norm_partial = reinterpret_cast<double *>(f);      // l.total is a multiple of 8 floats: 8-byte aligned
    n.scalars = reinterpret_cast<float *>(n.norm_partial + norm_parts + 1);
    n.run_sums = reinterpret_cast<double *>(n.scalars + 8);      // four doubles within the 256 bytes behind the partials
    HIP_TRY(hipHostMalloc((void **)&n.bad_index, sizeof(int), hipHostMallocDefault));
    *n.bad_index = 0;
    s->stats_cap = 64;
    HIP_TRY(hipMalloc((void **)&s->stats, (size_t)s->stats_cap * kPpoStats * sizeof(float)));
    HIP_TRY(hipMemset(s->stats, 0, (size_t)s->stats_cap * kPpoStats * sizeof(float)));
    return ZENV_OK;
}

extern "C" int zenv_ppo_init(zenv_t *h, const zenv_mlp_weights *w, const zenv_ppo_config *pc)
{
    if (!h || !w || !pc) return fail(ZENV_E_ARG, "null argument");
    if (int rc = zenv_ppo_check(&h->cfg, w, pc)) return rc;
    const float *t[PPO_MAX_TENSORS];
    tensor_list(w, t);
    return learner_create(h, AGENT_FLAT, 0, w->h_dim, t, kFlat, pc);
}

// zenv_hppo_init / _xyppo_ / _skppo_ / _opppo_: both learners of a pair, or neither
template <class W>
static int pair_init(int agent, zenv *h, const W *w, const zenv_ppo_config *lo, const zenv_ppo_config *hi)
{
    if (!h || !w || !lo || !hi) return fail(ZENV_E_ARG, "null argument");
    if (int rc = pair_check(agent, &h->cfg, w, lo, hi)) return rc;
    const Family &f = kFamily[agent];
    const float *tl[PPO_MAX_TENSORS], *th[PPO_MAX_TENSORS];
    lo_tensor_list(w, tl);
    hi_tensor_list(w, th);
    int rc = learner_create(h, agent, 0, w->h_dim, tl, f.kind[0](skills_of(w)), lo);
    if (!rc) rc = learner_create(h, agent, 1, w->h_dim, th, f.kind[1](skills_of(w)), hi);
    if (rc) {                   // no half-pair: a failed init leaves the handle without either learner
        learner_free(h->learner[f.first]);
        learner_free(h->learner[f.first + 1]);
    }
    return rc;
}

extern "C" int zenv_hppo_init(zenv_t *h, const zenv_hier_weights *w, const zenv_ppo_config *lo, const zenv_ppo_config *hi)
{
    return pair_init(AGENT_HIER, h, w, lo, hi);
}

extern "C" int zenv_xyppo_init(zenv_t *h, const zenv_xy_weights *w, const zenv_ppo_config *lo, const zenv_ppo_config *hi)
{
    return pair_init(AGENT_XY, h, w, lo, hi);
}

extern "C" int zenv_skppo_init(zenv_t *h, const zenv_skill_weights *w, const zenv_ppo_config *lo, const zenv_ppo_config *hi)
{
    return pair_init(AGENT_SKILL, h, w, lo, hi);
}

extern "C" int zenv_opppo_init(zenv_t *h, const zenv_option_weights *w, const zenv_ppo_config *lo,
                               const zenv_ppo_config *hi)
{
    return pair_init(AGENT_OPTION, h, w, lo, hi);
}

extern "C" int zenv_diayn_init(zenv_t *h, const zenv_skill_inverse_weights *w, const zenv_ppo_config *pc)
{
    if (!h || !w || !pc) return fail(ZENV_E_ARG, "null argument");
    if (int rc = zenv_diayn_check(&h->cfg, w, pc)) return rc;
    const float *t[PPO_MAX_TENSORS];
    inverse_tensor_list(w, t);
    const int rc = learner_create(h, AGENT_DIAYN, 0, w->h_dim, t, inv_kind(w->n_skills), pc);
    if (rc) learner_free(h->learner[L_DIAYN]);      // no half-built learner
    return rc;
}

namespace {

// What an entry point works on: a family's learner (of a pair: level 0 or 1, else -1) with the experience it reads.
struct Learner {
    PpoState *s = nullptr;
    int level = -1;
    int agent = AGENT_FLAT;
};

int find_learner(zenv *h, int level, int agent, Learner &out)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    const Family &f = kFamily[agent];
    if (!f.levels) level = 0;
    if (level != 0 && level != 1) return fail(ZENV_E_ARG, "level %d: 0 is the low level, 1 the high level", level);
    PpoState *s = h->learner[f.first + level];
    if (!s) return fail(ZENV_E_STATE, "zenv_%s_init first", f.name);
    out = Learner{ s, f.levels ? level : -1, agent };
    return ZENV_OK;
}

int learner_tensor(const Learner &l, int which, int index, void **dev_ptr, int64_t *count)
{
    if (!dev_ptr || !count) return fail(ZENV_E_ARG, "null argument");
    const PpoNet &n = l.s->net;
    if (which < 0 || which >= kFamily[l.agent].arenas) return fail(ZENV_E_ARG, "unknown arena %d", which);
    if (index < -1 || index >= n.n_tensors) return fail(ZENV_E_ARG, "tensor index %d outside [-1, %d)", index, n.n_tensors);
    float *base = n.param + (int64_t)which * n.arena;
    *dev_ptr = index < 0 ? base : base + n.off[index];
    *count = index < 0 ? n.arena : n.count[index];
    return ZENV_OK;
}

// a tensor (or, index = -1, a whole arena) to or from host memory, behind everything enqueued; both wait for the copy
int learner_copy(zenv *h, const Learner &l, int which, int index, void *host, bool to_host)
{
    if (!host) return fail(ZENV_E_ARG, "null argument");
    void *dev = nullptr;
    int64_t count = 0;
    if (int rc = learner_tensor(l, which, index, &dev, &count)) return rc;
    if (int rc = use_device(h)) return rc;
    if (to_host) HIP_TRY(hipMemcpyAsync(host, dev, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream));
    else HIP_TRY(hipMemcpyAsync(dev, host, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return mlp_range_check(h);
}

int learner_set_step(const Learner &l, int64_t step)
{
    if (step < 0) return fail(ZENV_E_ARG, "the step count must be >= 0");
    l.s->step = step;
    return ZENV_OK;
}

// the records the handle holds are zenv_collect_skill's.  exp_skill says so by itself -- the collector sets it once its
// buffers of exp.T frames are complete and every collector's start clears it -- the other terms are its consequences
bool skill_records(const zenv *h)
{
    return h->exp_mem && h->exp_skill && h->hi_kind == 1 && h->sk_mem && h->sk.T == h->exp.T && h->hi_m >= 1;
}

int need_skill_records(const zenv *h)
{
    if (!skill_records(h))
        return fail(ZENV_E_STATE, "zenv_collect_skill first: the ZENV_F_EXP_* / ZENV_F_LO_* / ZENV_F_HI_* buffers do "
                                  "not hold its records");
    return ZENV_OK;
}

// the records are of an agent with the learner's number of skills (ready: that agent is loaded)
int need_learner_skills(const zenv *h, bool ready, const Learner &l)
{
    if (!ready || h->skill.S != l.s->net.S)
        return fail(ZENV_E_STATE, "the records are of an agent with another number of skills than the learner's %d",
                    l.s->net.S);
    return ZENV_OK;
}

// what DIAYN's two updates read: a completed zenv_collect_skill of at least two frames
int diayn_records(const zenv *h)
{
    if (int rc = need_skill_records(h)) return rc;
    if (h->exp.T < 2)
        return fail(ZENV_E_STATE, "a collection of one frame has no (next observation, skill) pair for the inverse model");
    return ZENV_OK;
}

// The kept samples of the handle's records into diayn_list (k_inv_count / _scan / _scatter), their number into
// diayn_kept; waits for the device.
int diayn_compact(zenv *h)
{
    if (int rc = diayn_records(h)) return rc;
    if (int rc = use_device(h)) return rc;
    const int64_t samples = (int64_t)h->n_env * (h->exp.T - 1);
    const int64_t blocks = (samples + kInvBlock - 1) / kInvBlock;
    if (h->diayn_cap < samples) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (h->diayn_mem) HIP_TRY(hipFree(h->diayn_mem));
        h->diayn_mem = nullptr, h->diayn_list = h->diayn_blocks = nullptr, h->diayn_cap = 0, h->diayn_kept = -1;
        HIP_TRY(hipMalloc(&h->diayn_mem, (size_t)(samples + blocks + 2) * sizeof(int32_t)));
        h->diayn_list = static_cast<int32_t *>(h->diayn_mem);
        h->diayn_blocks = h->diayn_list + samples;      // [blocks + 1], then the total
        h->diayn_cap = samples;
    }
    h->diayn_kept = -1;
    int32_t *total = h->diayn_blocks + (h->diayn_cap + kInvBlock - 1) / kInvBlock + 1;
    HIP_TRY(launch_inv_compact(h->exp.mask, h->n_env, h->exp.T, h->diayn_blocks, h->diayn_list, total, h->stream));
    int32_t kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, total, sizeof(kept), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->diayn_kept = kept;
    return ZENV_OK;
}

// minibatch / epoch: ZENV_E_STATE when the collection kept no sample (the list is taken here if it was not yet)
int diayn_any_kept(zenv *h)
{
    if (h->diayn_kept < 0)
        if (int rc = diayn_compact(h)) return rc;
    if (h->diayn_kept == 0) return fail(ZENV_E_STATE, "the last zenv_collect_skill kept no sample for the inverse model");
    return ZENV_OK;
}

// the experience the learner gathers from, and how many sample indexes it has; ZENV_E_STATE when the handle holds none
// of the learner's kind
int learner_exp(const zenv *h, const Learner &l, PpoExp &x, int64_t &samples)
{
    const ExpBuffers &e = h->exp;
    const HierOut &o = h->hout;
    // T frames of every env, the flat collector's columns; what else a low level reads of a frame is set by its case
    auto frames = [&](int T) {
        x = PpoExp{ e.obs, e.zone_obs, e.action, e.log_prob, e.value, e.advantage, e.returnn, h->n_env, T, nullptr, nullptr,
                    nullptr };
        samples = (int64_t)h->n_env * T;
    };
    // the M dense env-major rows of a high level, the pick as the action, one log_prob per row
    auto rows = [&]() {
        x = PpoExp{ o.obs, o.zone_obs, nullptr, o.log_prob, o.value, o.advantage, o.returnn, (int)h->hi_m, 1, nullptr, o.action,
                    nullptr };
        samples = h->hi_m;
    };
    const bool high = l.level == 1;
    switch (l.agent) {
    case AGENT_DIAYN:
        if (int rc = diayn_records(h)) return rc;
        if (int rc = need_learner_skills(h, h->skill_ready, l)) return rc;
        // the pairs (obs of frame f + 1, skill of frame f), f in 0 .. T-2, where the mask of frame f + 1 is not 0
        // (_hier_policy_opt.py:193-199)
        frames(e.T - 1);
        x.action = x.log_prob = x.value = x.advantage = x.returnn = nullptr;
        x.skill = h->sk.lo_skill, x.obs_shift = 1, x.keep = e.mask;
        return ZENV_OK;
    case AGENT_XY:
        if (!h->exp_mem || !h->exp_xy || h->hi_kind != 3 || !h->xc_mem || h->xc.T != e.T)
            return fail(ZENV_E_STATE, "zenv_collect_xy first: the ZENV_F_EXP_* / ZENV_F_LO_* / ZENV_F_HI_* buffers do not "
                                      "hold its records");
        if (!high) {            // ALL T frames of every env (_hier_policy_opt.py:147-158), the goal the frame was acted under
            frames(e.T);
            x.goal = reinterpret_cast<const float *>(h->xc.lo_goal);
        } else {                // the windows, M = N W: the goal is the action
            rows();
            x.action = reinterpret_cast<const float *>(h->xc.hi_goal), x.hi_action = nullptr;
        }
        return ZENV_OK;
    case AGENT_SKILL:
        if (int rc = need_skill_records(h)) return rc;
        if (int rc = need_learner_skills(h, h->skill_ready, l)) return rc;
        if (!high) {            // ALL T frames of every env (_hier_policy_opt.py:188-199), the skill the frame was acted under
            frames(e.T);
            x.skill = h->sk.lo_skill;
        } else {                // the windows, M = N T / skill_len
            rows();
        }
        return ZENV_OK;
    case AGENT_OPTION:
        if (!h->exp_mem || !h->exp_option || h->hi_kind != 2 || !h->oc_mem || h->oc.T != e.T)
            return fail(ZENV_E_STATE, "zenv_collect_option first: the ZENV_F_EXP_* / ZENV_F_LO_* / ZENV_F_HI_* buffers do "
                                      "not hold its records");
        if (int rc = need_learner_skills(h, h->option_ready, l)) return rc;
        if (!high) {            // frames 0 .. T-2 of every env (_hier_policy_opt.py:111-118); a_2's records are the oc ones
            frames(e.T - 1);
            x.skill = h->oc.lo_skill, x.term_action = h->oc.term_action, x.term_log_prob = h->oc.term_log_prob;
            return ZENV_OK;
        }
        if (h->hi_m < 1) return fail(ZENV_E_STATE, "the last zenv_collect_option closed no high-level transition (M = 0)");
        rows();                 // the closed transitions
        return ZENV_OK;
    case AGENT_HIER:
        if (!h->exp_mem || !h->exp_hier || h->hi_kind != 0 || !h->hframes.lo_goal)
            return fail(ZENV_E_STATE, "zenv_collect_hier first: the ZENV_F_EXP_* / ZENV_F_LO_* / ZENV_F_HI_* buffers do not "
                                      "hold its records");
        if (!high) {            // frames 0 .. T-2 of every env (hrl_policy_planner.py:68)
            frames(e.T - 1);
            x.goal = h->hframes.lo_goal;
            return ZENV_OK;
        }
        if (h->hi_m < 1) return fail(ZENV_E_STATE, "the last zenv_collect_hier closed no high-level transition (M = 0)");
        rows();                 // the closed transitions, with the goals available at each pick
        x.hi_mask = o.action_mask;
        return ZENV_OK;
    default:                    // AGENT_FLAT, AGENT_A2C: every frame of the flat collector
        if (!h->exp_mem) return fail(ZENV_E_STATE, "zenv_collect first: the handle holds no experience");
        frames(e.T);
        return ZENV_OK;
    }
}

// the checks every update call shares; *idx_dev: the indices on the device
int learner_indices(zenv *h, PpoState *s, const int32_t *idx, int total, int on_device, int64_t samples,
                    const int32_t **idx_dev)
{
    if (int rc = use_device(h)) return rc;
    if (on_device) {
        *idx_dev = idx;
        return ZENV_OK;
    }
    for (int i = 0; i < total; ++i)
        if (idx[i] < 0 || idx[i] >= samples)
            return fail(ZENV_E_ARG, "index %d (at %d) outside [0, %lld)", idx[i], i, (long long)samples);
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

int learner_stats_rows(zenv *h, PpoState *s, int rows)
{
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

int learner_step(zenv *h, PpoState *s)
{
    s->step += 1;
    // torch.optim.Adam forms these in Python floats: step_size = lr / (1 - beta1^t), sqrt(1 - beta2^t)
    const double bc1 = 1.0 - std::pow(0.9, (double)s->step), bc2 = 1.0 - std::pow(0.999, (double)s->step);
    HIP_TRY(launch_ppo_apply(s->net, (float)(s->lr / bc1), (float)std::sqrt(bc2), h->stream));
    return ZENV_OK;
}

int learner_minibatch(zenv *h, const Learner &l, const int32_t *idx, int count, int idx_on_device, int apply)
{
    if (!idx) return fail(ZENV_E_ARG, "null argument");
    PpoState *s = l.s;
    if (count < 1 || count > s->net.max_batch)
        return fail(ZENV_E_ARG, "count %d outside [1, max_batch = %d]", count, s->net.max_batch);
    PpoExp x{};
    int64_t samples = 0;
    if (int rc = learner_exp(h, l, x, samples)) return rc;
    const int32_t *idx_dev = nullptr;
    if (int rc = learner_indices(h, s, idx, count, idx_on_device, samples, &idx_dev)) return rc;
    if (int rc = learner_stats_rows(h, s, 1)) return rc;
    HIP_TRY(launch_ppo_minibatch(s->net, x, idx_dev, count, s->stats, h->stream));
    return apply ? learner_step(h, s) : ZENV_OK;
}

int learner_apply(zenv *h, const Learner &l)
{
    if (int rc = use_device(h)) return rc;
    return learner_step(h, l.s);
}

int learner_epoch(zenv *h, const Learner &l, const int32_t *order, int total, int batch_size, int on_device)
{
    if (!order) return fail(ZENV_E_ARG, "null argument");
    PpoState *s = l.s;
    if (total < 1) return fail(ZENV_E_ARG, "total must be >= 1");
    if (batch_size < 1 || batch_size > s->net.max_batch)
        return fail(ZENV_E_ARG, "batch_size %d outside [1, max_batch = %d]", batch_size, s->net.max_batch);
    PpoExp x{};
    int64_t samples = 0;
    if (int rc = learner_exp(h, l, x, samples)) return rc;
    const int32_t *idx_dev = nullptr;
    if (int rc = learner_indices(h, s, order, total, on_device, samples, &idx_dev)) return rc;
    const int n_mb = (total + batch_size - 1) / batch_size;
    if (int rc = learner_stats_rows(h, s, n_mb)) return rc;
    for (int k = 0; k < n_mb; ++k) {
        const int lo = k * batch_size, count = std::min(batch_size, total - lo);
        HIP_TRY(launch_ppo_minibatch(s->net, x, idx_dev + lo, count, s->stats + (size_t)k * kPpoStats, h->stream));
        if (int rc = learner_step(h, s)) return rc;
    }
    return ZENV_OK;
}

}  // namespace

// every entry point: find the learner, then the shared body
#define LEARNER(h, level, agent)                                  \
    Learner l;                                                    \
    if (int rc = find_learner(h, level, agent, l)) return rc

// The entry points of a family come in two shapes: LEARNER_ABI_LEVELS for a pair, whose functions take `int level`
// behind the handle, and LEARNER_ABI for a family of one learner.  Both are the five accessors and the three PPO update
// calls below with LV (the parameter) and lv (its value) filled in.  The order of the argument checks is part of the ABI.
#define LEVEL_PARAM , int level

#define LEARNER_ACCESSORS(name, agent, LV, lv)                                                                    \
    extern "C" int zenv_##name##_tensor(zenv_t *h LV, int which, int index, void **dev_ptr, int64_t *count)      \
    {                                                                                                             \
        if (!h || !dev_ptr || !count) return fail(ZENV_E_ARG, "null argument");                                   \
        LEARNER(h, lv, agent);                                                                                    \
        return learner_tensor(l, which, index, dev_ptr, count);                                                   \
    }                                                                                                             \
    extern "C" int zenv_##name##_read(zenv_t *h LV, int which, int index, float *dst)                            \
    {                                                                                                             \
        if (!dst) return fail(ZENV_E_ARG, "null argument");                                                       \
        LEARNER(h, lv, agent);                                                                                    \
        return learner_copy(h, l, which, index, dst, true);                                                       \
    }                                                                                                             \
    extern "C" int zenv_##name##_write(zenv_t *h LV, int which, int index, const float *src)                     \
    {                                                                                                             \
        if (!src) return fail(ZENV_E_ARG, "null argument");                                                       \
        LEARNER(h, lv, agent);                                                                                    \
        return learner_copy(h, l, which, index, const_cast<float *>(src), false);                                 \
    }                                                                                                             \
    extern "C" int zenv_##name##_get_step(zenv_t *h LV, int64_t *step)                                           \
    {                                                                                                             \
        if (!h || !step) return fail(ZENV_E_ARG, "null argument");                                                \
        LEARNER(h, lv, agent);                                                                                    \
        *step = l.s->step;                                                                                        \
        return ZENV_OK;                                                                                           \
    }                                                                                                             \
    extern "C" int zenv_##name##_set_step(zenv_t *h LV, int64_t step)                                            \
    {                                                                                                             \
        LEARNER(h, lv, agent);                                                                                    \
        return learner_set_step(l, step);                                                                         \
    }

// READY: what zenv_<name>_minibatch and _epoch do between the lookup and the body (DIAYN: the kept-sample list)
#define LEARNER_UPDATES(name, agent, LV, lv, READY)                                                               \
    extern "C" int zenv_##name##_minibatch(zenv_t *h LV, const int32_t *idx, int count, int idx_on_device, int apply) \
    {                                                                                                             \
        if (!h || !idx) return fail(ZENV_E_ARG, "null argument");                                                 \
        LEARNER(h, lv, agent);                                                                                    \
        READY;                                                                                                    \
        return learner_minibatch(h, l, idx, count, idx_on_device, apply);                                         \
    }                                                                                                             \
    extern "C" int zenv_##name##_apply(zenv_t *h LV)                                                             \
    {                                                                                                             \
        LEARNER(h, lv, agent);                                                                                    \
        return learner_apply(h, l);                                                                               \
    }                                                                                                             \
    extern "C" int zenv_##name##_epoch(zenv_t *h LV, const int32_t *order, int total, int batch_size, int on_device) \
    {                                                                                                             \
        if (!h || !order) return fail(ZENV_E_ARG, "null argument");                                               \
        LEARNER(h, lv, agent);                                                                                    \
        READY;                                                                                                    \
        return learner_epoch(h, l, order, total, batch_size, on_device);                                          \
    }

#define LEARNER_ABI(name, agent, READY) LEARNER_ACCESSORS(name, agent, , 0) LEARNER_UPDATES(name, agent, , 0, READY)
#define LEARNER_ABI_LEVELS(name, agent) \
    LEARNER_ACCESSORS(name, agent, LEVEL_PARAM, level) LEARNER_UPDATES(name, agent, LEVEL_PARAM, level, )

LEARNER_ABI(ppo, AGENT_FLAT, )
LEARNER_ABI_LEVELS(hppo, AGENT_HIER)
LEARNER_ABI_LEVELS(xyppo, AGENT_XY)
LEARNER_ABI_LEVELS(skppo, AGENT_SKILL)
LEARNER_ABI_LEVELS(opppo, AGENT_OPTION)
// DIAYN: the inverse model's learner (one: no level) and, below, the kept samples and the learned skill prior
LEARNER_ABI(diayn, AGENT_DIAYN, if (int rc = diayn_any_kept(h)) return rc)

extern "C" int zenv_diayn_samples(zenv_t *h, int64_t *count)
{
    if (!h || !count) return fail(ZENV_E_ARG, "null argument");
    if (int rc = diayn_compact(h)) return rc;
    *count = h->diayn_kept;
    return mlp_range_check(h);
}

extern "C" int zenv_diayn_prior_init(zenv_t *h, const float *logits, int n_skills, double lr, double adam_eps)
{
    if (!h || !logits) return fail(ZENV_E_ARG, "null argument");
    if (int rc = check_skills(n_skills)) return rc;
    for (double v : { lr, adam_eps })
        if (bad_hyper(v)) return fail(ZENV_E_ARG, "a hyper-parameter is negative or not finite (%g)", v);
    for (int s = 0; s < n_skills; ++s)
        if (!std::isfinite(logits[s])) return fail(ZENV_E_ARG, "logits[%d] is not finite", s);
    if (int rc = use_device(h)) return rc;
    if (!h->diayn_counts) HIP_TRY(hipMalloc((void **)&h->diayn_counts, 32 * sizeof(int32_t)));
    if (!h->diayn_flag) {
        HIP_TRY(hipHostMalloc((void **)&h->diayn_flag, sizeof(int), hipHostMallocDefault));
        *h->diayn_flag = 0;
    }
    auto &p = h->prior;
    p = {};
    p.S = n_skills, p.lr = lr, p.adam_eps = adam_eps;
    std::copy(logits, logits + n_skills, p.logits);
    p.ready = true;
    return ZENV_OK;
}

// update_skill_prior (_hier_policy_opt.py:449-464): one Adam step on the mean cross-entropy of the logits against the
// M picks of the last zenv_collect_skill.  d loss / d logit_s = softmax(logits)_s - count_s / M, formed in double from
// the device histogram and rounded to float32; the step in float32 as k_ppo_adam forms it.
extern "C" int zenv_diayn_prior_update(zenv_t *h)
{
    if (!h) return fail(ZENV_E_ARG, "null handle");
    auto &p = h->prior;
    if (!p.ready) return fail(ZENV_E_STATE, "zenv_diayn_prior_init first");
    if (!skill_records(h))
        return fail(ZENV_E_STATE, "zenv_collect_skill first: the ZENV_F_HI_* rows do not hold its picks (M = 0)");
    if (!h->skill_ready || h->skill.S != p.S)
        return fail(ZENV_E_STATE, "the records are of an agent with another number of skills than the prior's %d", p.S);
    if (int rc = use_device(h)) return rc;
    const int S = p.S;
    HIP_TRY(launch_prior_hist(h->hout.action, h->hi_m, S, h->diayn_counts, h->diayn_flag, h->stream));
    int32_t counts[32];
    HIP_TRY(hipMemcpyAsync(counts, h->diayn_counts, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    double m = (double)p.logits[0];
    for (int s = 1; s < S; ++s) m = std::max(m, (double)p.logits[s]);
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += std::exp((double)p.logits[s] - m);
    const double lse = m + std::log(sum);
    p.step += 1;
    const double bc1 = 1.0 - std::pow(0.9, (double)p.step), bc2 = 1.0 - std::pow(0.999, (double)p.step);
    const float step_size = (float)(p.lr / bc1), bc2_sqrt = (float)std::sqrt(bc2), eps = (float)p.adam_eps;
    const float b2 = 0.999f, w1 = (float)(1.0 - 0.9), w2 = (float)(1.0 - 0.999);
    for (int s = 0; s < S; ++s) {
        // S = 1: the softmax is exactly 1 and, with every pick counted, the gradient exactly 0
        const float gr = (float)(std::exp((double)p.logits[s] - lse) - (double)counts[s] / (double)h->hi_m);
        float mo = p.exp_avg[s], v = p.exp_avg_sq[s];
        mo = mo + w1 * (gr - mo);
        v = v * b2 + (w2 * gr) * gr;
        const float denom = std::sqrt(v) / bc2_sqrt + eps;
        p.logits[s] = p.logits[s] + ((-step_size) * mo) / denom;
        p.exp_avg[s] = mo, p.exp_avg_sq[s] = v;
    }
    return mlp_range_check(h);
}

extern "C" int zenv_diayn_prior_read(zenv_t *h, float *logits)
{
    if (!h || !logits) return fail(ZENV_E_ARG, "null argument");
    if (!h->prior.ready) return fail(ZENV_E_STATE, "zenv_diayn_prior_init first");
    std::copy(h->prior.logits, h->prior.logits + h->prior.S, logits);
    return ZENV_OK;
}

extern "C" int zenv_diayn_prior_write(zenv_t *h, const float *logits)
{
    if (!h || !logits) return fail(ZENV_E_ARG, "null argument");
    if (!h->prior.ready) return fail(ZENV_E_STATE, "zenv_diayn_prior_init first");
    for (int s = 0; s < h->prior.S; ++s)
        if (!std::isfinite(logits[s])) return fail(ZENV_E_ARG, "logits[%d] is not finite", s);
    std::copy(logits, logits + h->prior.S, h->prior.logits);
    return ZENV_OK;
}

// ============================================================================ the flat actor-critic's A2C update
// update_parameters of main/src/torch_ac/algos/a2c.py:21-93 for recurrence 1: one RMSprop step on the gradient of the
// loss averaged over ALL frames of a collection, taken chunk by chunk through the workspace (launch_a2c_accumulate).
namespace {

// the learner's settings as the shared checks and learner_create take them; rmsprop_eps rides in adam_eps
zenv_ppo_config a2c_as_ppo(const zenv_a2c_config *ac)
{
    zenv_ppo_config pc{};
    pc.lr = ac->lr, pc.adam_eps = ac->rmsprop_eps, pc.clip_eps = 0.0, pc.entropy_coef = ac->entropy_coef;
    pc.value_loss_coef = ac->value_loss_coef, pc.max_grad_norm = ac->max_grad_norm, pc.max_batch = ac->max_batch;
    pc.distributional_value = 0;
    return pc;
}

// one chunk behind what is enqueued; idx_dev: count indexes on the device
int a2c_chunk(zenv *h, PpoState *s, const PpoExp &x, const int32_t *idx_dev, int count, int64_t total, int first)
{
    if (first) s->acc_total = total;
    HIP_TRY(launch_a2c_accumulate(s->net, x, idx_dev, count, total, first, h->stream));
    return ZENV_OK;
}

int a2c_step(zenv *h, PpoState *s)
{
    if (int rc = learner_stats_rows(h, s, 1)) return rc;
    s->step += 1;
    HIP_TRY(launch_a2c_apply(s->net, (float)s->lr, (float)s->rms_alpha, (float)(1.0 - s->rms_alpha), (float)s->rms_eps,
                             std::max<int64_t>(s->acc_total, 1), s->stats, h->stream));
    return ZENV_OK;
}

}  // namespace

extern "C" int zenv_a2c_check(const zenv_config *cfg, const zenv_mlp_weights *w, const zenv_a2c_config *ac)
{
    if (!cfg || !w || !ac) return fail(ZENV_E_ARG, "null argument");
    if (bad_hyper(ac->rmsprop_alpha))
        return fail(ZENV_E_ARG, "a hyper-parameter is negative or not finite (%g)", ac->rmsprop_alpha);
    const zenv_ppo_config pc = a2c_as_ppo(ac);
    const float *t[PPO_MAX_TENSORS];
    tensor_list(w, t);
    if (int rc = learner_check(cfg, w->h_dim, t, kA2c, &pc, "")) return rc;
    if (w->critic_sigma_w || w->critic_sigma_b)
        return fail(ZENV_E_ARG, "critic_sigma_* given: A2CAlgo has no distributional critic");
    return ZENV_OK;
}

extern "C" int zenv_a2c_init(zenv_t *h, const zenv_mlp_weights *w, const zenv_a2c_config *ac)
{
    if (!h || !w || !ac) return fail(ZENV_E_ARG, "null argument");
    if (int rc = zenv_a2c_check(&h->cfg, w, ac)) return rc;
    const zenv_ppo_config pc = a2c_as_ppo(ac);
    const float *t[PPO_MAX_TENSORS];
    tensor_list(w, t);
    PpoState *&s = h->learner[L_A2C];
    const int rc = learner_create(h, AGENT_A2C, 0, w->h_dim, t, kA2c, &pc);
    if (rc) {
        learner_free(s);                // no half-built learner
        return rc;
    }
    s->rms_alpha = ac->rmsprop_alpha, s->rms_eps = ac->rmsprop_eps;
    return ZENV_OK;
}

LEARNER_ACCESSORS(a2c, AGENT_A2C, , 0)

extern "C" int zenv_a2c_accumulate(zenv_t *h, const int32_t *idx, int count, int idx_on_device, int64_t total, int first)
{
    if (!h || !idx) return fail(ZENV_E_ARG, "null argument");
    LEARNER(h, 0, AGENT_A2C);
    PpoState *s = l.s;
    if (count < 1 || count > s->net.max_batch)
        return fail(ZENV_E_ARG, "count %d outside [1, max_batch = %d]", count, s->net.max_batch);
    if (total < count) return fail(ZENV_E_ARG, "total %lld is less than the chunk's count %d", (long long)total, count);
    if (!first && s->acc_total == 0)
        return fail(ZENV_E_STATE, "no accumulation is open: the update's first chunk takes first != 0");
    if (!first && total != s->acc_total)
        return fail(ZENV_E_ARG, "total %lld differs from the first chunk's %lld", (long long)total, (long long)s->acc_total);
    PpoExp x{};
    int64_t samples = 0;
    if (int rc = learner_exp(h, l, x, samples)) return rc;
    const int32_t *idx_dev = nullptr;
    if (int rc = learner_indices(h, s, idx, count, idx_on_device, samples, &idx_dev)) return rc;
    return a2c_chunk(h, s, x, idx_dev, count, total, first ? 1 : 0);
}

extern "C" int zenv_a2c_apply(zenv_t *h)
{
    LEARNER(h, 0, AGENT_A2C);
    if (int rc = use_device(h)) return rc;
    return a2c_step(h, l.s);
}

extern "C" int zenv_a2c_update(zenv_t *h)
{
    LEARNER(h, 0, AGENT_A2C);
    PpoState *s = l.s;
    PpoExp x{};
    int64_t samples = 0;
    if (int rc = learner_exp(h, l, x, samples)) return rc;
    if (int rc = use_device(h)) return rc;
    if (s->iota_n < samples) {          // once per size: the index order 0 .. N T - 1 (a2c.py:_get_starting_indexes)
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (s->iota) HIP_TRY(hipFree(s->iota));
        s->iota = nullptr, s->iota_n = 0;
        std::vector<int32_t> host((size_t)samples);
        for (int64_t i = 0; i < samples; ++i) host[(size_t)i] = (int32_t)i;
        HIP_TRY(hipMalloc((void **)&s->iota, (size_t)samples * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(s->iota, host.data(), (size_t)samples * sizeof(int32_t), hipMemcpyHostToDevice));
        s->iota_n = samples;
    }
    const int64_t B = s->net.max_batch;
    for (int64_t lo = 0; lo < samples; lo += B) {
        const int count = (int)std::min<int64_t>(B, samples - lo);
        if (int rc = a2c_chunk(h, s, x, s->iota + lo, count, samples, lo == 0)) return rc;
    }
    return a2c_step(h, s);
}
