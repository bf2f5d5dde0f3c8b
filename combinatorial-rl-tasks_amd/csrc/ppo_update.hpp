// ppo_update.hpp -- the PPO updates on the device (ppo_update.hip): the flat actor-critic's, the Zone-goals agent's two
// levels', the xy-goals agent's two levels', the fixed-length-skills agent's two levels' and the Options agent's two
// levels'; and the flat actor-critic's A2C update (launch_a2c_*).  What zenv_train.cpp hands to the launches.  Internal:
// not installed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace zenvk {

// the tensors of the parameter arena, in zenv_mlp_weights' member order (the Zone-goals low level: the same 18 with
// [obs, goal] where the flat network has obs)
enum {
    PPO_ZONE_W1 = 0, PPO_ZONE_B1, PPO_ZONE_W2, PPO_ZONE_B2, PPO_ZONE_W3, PPO_ZONE_B3, PPO_COMB_W, PPO_COMB_B,
    PPO_ENC_W, PPO_ENC_B, PPO_MU_W, PPO_MU_B, PPO_STD_W, PPO_STD_B, PPO_CRITIC_W1, PPO_CRITIC_B1, PPO_CRITIC_W2,
    PPO_CRITIC_B2, PPO_SIGMA_W, PPO_SIGMA_B, PPO_MAX_TENSORS
};
// The Zone-goals high level's 16 tensors, zenv_hier_weights' hi_* member order: the encoder's eight as above, then
// actor.0 / actor.2 where the Gaussian actor has enc_ / mu_, then the critic two places earlier (PpoNet::cr)
enum { PPO_ACTOR_W1 = PPO_ENC_W, PPO_ACTOR_B1 = PPO_ENC_B, PPO_ACTOR_W2 = PPO_MU_W, PPO_ACTOR_B2 = PPO_MU_B };
// The fixed-length-skills agent's high level has the same 16 places: actor.enc_.0.0 [h, h] / actor.discrete_.0 [S, h]
// where the Zone-goals one has actor.0 / actor.2 (PPO_HEAD_SKILLS).  Its low level is the Gaussian network on
// [obs, onehot(skill)] (XD = 8 + S) whose actor.enc_.0.0 and critic.0 read [emb, onehot]: [h, h + S] (PpoNet::S).
enum { PPO_HEAD_GAUSSIAN = 0, PPO_HEAD_ZONES = 1, PPO_HEAD_SKILLS = 2, PPO_HEAD_INVERSE = 3 };
// DIAYN's discriminator (InverseModel, zenv_skill_inverse_weights' member order: 10 tensors): the encoder's eight as
// above with a ReLU after combine_net.0, then combine_net.2 [S, h] / [S] straight on it -- no enc_ layer, no critic
// (PPO_HEAD_INVERSE).  Its head uses the image slots PPO_I_HA / PPO_T_HA.
enum { PPO_INV_W2 = PPO_ENC_W, PPO_INV_B2 = PPO_ENC_B, PPO_INV_TENSORS = 10 };
// what the Gaussian head's loss is taken of: the flat learner's action with a recorded log_prob per component
// (k_ppo_loss), or the xy-goals high level's goal with one recorded log_prob per row (k_xyppo_hi_loss)
enum { PPO_LOSS_ACTION = 0, PPO_LOSS_JOINT_GOAL = 1 };
// the padded weight images k_ppo_prep rebuilds from the arena before every minibatch (I_*: [out][in] with the bias in
// column h, the A operand of a forward product; T_*: the transpose, the A operand of a backward-data product)
enum {
    PPO_I_W1 = 0, PPO_I_W2, PPO_I_W3, PPO_I_WC, PPO_I_WE, PPO_I_WV, PPO_I_HA, PPO_I_HV,
    PPO_T_W2, PPO_T_W3, PPO_T_WC, PPO_T_WE, PPO_T_WV, PPO_T_HA, PPO_T_HV, PPO_N_IMAGES
};
constexpr int kPpoChunk = 256;      // rows one wave reduces into one partial of a weight gradient
constexpr int kPpoStats = 6;        // entropy, value, value std, policy loss, value loss, gradient norm
constexpr int kA2cStats = 5;        // the A2C learner's: entropy, value, policy loss, value loss, gradient norm
constexpr int kPpoNormBlock = 4096; // arena elements per partial of the gradient norm
constexpr int kPpoReduceSplit = 16; // k_ppo_reduce_split: segments of the chunk range, one thread each
constexpr int kInvBlock = 1024;     // k_inv_count / k_inv_scatter: sample indexes per block (256 threads x 4 consecutive)
constexpr int kInvScan = 64;        // k_inv_scan: block counts per tile of the exclusive scan (one wave)

struct PpoHyper {
    float lr, adam_eps, clip_eps, entropy_coef, value_loss_coef, max_grad_norm;
};

struct PpoNet {
    int h, HP, F, Z, K1, KC, dist, n_tensors;
    int XD;                  // the per-sample input's width: 8 (obs), 10 ([obs, goal]) or 8 + S ([obs, onehot(skill)]);
                             // K1 = XD + F
    int W1C;                 // columns of zone_net_.0's image and gathered input: XD + F + 1 rounded up to 8; the last is
                             // the constant that carries the bias.  KC = HP + XD rounded up to 8
    int S;                   // the fixed-length-skills and Options agents' learners: the number of skills (1 .. 32); 0 for
                             // every other
    int NA;                  // the Gaussian head's action components: 2, or 3 for the Options agent's low level, whose
                             // third, a_2, decides whether the option ends.  PRE / DH hold mu in columns 0 .. NA, std in
                             // NA .. 2 NA and the value in 2 NA (4 under every other head)
    int LDC;                 // the leading dimension of C and of the images of actor.enc_.0.0 and critic.0: HP, or HP + 32
                             // for the skills agent's low level, whose columns HP .. HP + S hold onehot(skill)
    int head;                // PPO_HEAD_GAUSSIAN: enc_, mu_, std_;  PPO_HEAD_ZONES: actor.0 / actor.2 over [emb, zone row];
                             // PPO_HEAD_SKILLS: enc_, discrete_ (a Categorical over S skills)
    int loss;                // PPO_LOSS_ACTION, or PPO_LOSS_JOINT_GOAL: the xy-goals high level (PPO_HEAD_GAUSSIAN only)
    int cr;                  // the arena index of critic.0.weight: PPO_CRITIC_W1, or two less under PPO_HEAD_ZONES
    int split_reduce;        // the partials of a weight gradient are added by kPpoReduceSplit threads per element
                             // (k_ppo_reduce_split); 0 for the flat learner, whose sums keep their one chain and bits
    int accumulate;          // launch_a2c_accumulate's chunks after the first: a weight gradient's partials are added onto
                             // the gradient arena (k_ppo_reduce<true>); 0 in every other launch, which overwrites it
    int64_t off[PPO_MAX_TENSORS], count[PPO_MAX_TENSORS];   // floats, within an arena
    int64_t arena;                                          // floats of one arena (a multiple of 64)
    float *param, *grad, *exp_avg, *exp_avg_sq;
    float *img[PPO_N_IMAGES];
    // activation workspace for max_batch samples; the backward pass overwrites every activation with its delta
    int max_batch;
    float *A1, *A2;          // [rows][HP], rows = samples x Z rounded up to 32
    float *P, *C, *Ha, *Hc;  // [samples][HP] (C: [samples][LDC]), samples rounded up to 32
    float *CI;               // [samples][KC]: zone_net_.4's output (HP columns), then the XD own features
    float *PRE, *DH;         // [samples][32]: the six (NA = 3: seven) head pre-activations, their deltas
    // PPO_HEAD_ZONES only: relu(actor.0) of every zone row [rows][HP], the logits and their deltas [rows][32] (column 0)
    // PPO_HEAD_SKILLS: L, DL are the S logits of a sample and their deltas [samples][32]; the value stays in PRE / DH
    // PPO_HEAD_INVERSE: L, DL the same; Ha, Hc, PRE, DH and the images of enc_ and the critic are not allocated
    float *U, *L, *DL;
    double *DZ;              // [rows]: the logits' deltas as k_hppo_loss forms them, before they are rounded into DL;
                             // the skills / Options agents' low level: [samples][2 NA + 1], the head's deltas before they
                             // are rounded; PPO_HEAD_INVERSE: [samples][S], the logits' deltas the same way
    float *SS;               // [samples][8]: the per-sample terms of the statistics
    float *partial;          // the per-chunk partials of one weight gradient
    double *norm_partial;    // [arena / kPpoNormBlock + 1]
    float *scalars;          // [0] the gradient norm of the last launch_ppo_norm
    double *run_sums;        // [4] the A2C learner's running sums over the chunks of an update: entropy, value, policy loss,
                             // value loss (k_a2c_stats), finalised once by launch_a2c_apply
    int *bad_index;          // page-locked host word: a device index outside [0, N T), or a recorded goal or skill
                             // outside its range, was met (and dropped)
    PpoHyper hyper;
};

// The experience a minibatch is gathered from.  Sample index i is env i / T, frame i % T, and lies at slot
// frame * N + env: the handle's time-major buffers with T the frames an env hands out (all of them; one less for the
// Zone-goals low level, whose last frame is never read), or dense rows with N = the rows and T = 1.
// PPO_LOSS_JOINT_GOAL: action is the recorded goal [slot][2] and log_prob one float per slot, the sum over both
// dimensions.
struct PpoExp {
    const float *obs, *zone_obs, *action, *log_prob, *value, *advantage, *returnn;
    int N, T;
    const float *goal;              // [slot][2], XD = 10 only
    const int32_t *hi_action;       // PPO_HEAD_ZONES: the recorded goal [slot] and the goals available at the pick;
    const uint8_t *hi_mask;         // [slot][Z].  PPO_HEAD_SKILLS: the recorded skill [slot], no mask
    const int32_t *skill = nullptr; // [slot]: the skill a frame was acted under (XD = 8 + S only)
    // NA = 3: the third action component and its recorded log_prob [slot]; components 0-1 stay in action / log_prob [slot][2]
    const float *term_action = nullptr, *term_log_prob = nullptr;
    // PPO_HEAD_INVERSE: sample i (env i / T, frame f = i % T, T = the collection's frames - 1) reads its observation and
    // zone rows at frame f + obs_shift, its skill at frame f, and is dropped where keep [slot of frame f + obs_shift]
    // is 0.  Every other learner: 0 and null.
    int obs_shift = 0;
    const float *keep = nullptr;
};

// forward, loss and backward of the samples idx[0 .. count) (device memory): gradients into net.grad, the six
// statistics into stats (device memory)
hipError_t launch_ppo_minibatch(const PpoNet &net, const PpoExp &exp, const int32_t *idx, int count, float *stats,
                                hipStream_t stream);
// the clip and Adam step on net.grad; step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t), formed on the
// host in double as torch forms them
hipError_t launch_ppo_apply(const PpoNet &net, float step_size, float bc2_sqrt, hipStream_t stream);

// ---- the flat actor-critic's A2C update (main/src/torch_ac/algos/a2c.py:21-93, recurrence 1): ONE gradient of the loss
// averaged over `total` frames, which may be many times max_batch.  A chunk of count <= max_batch samples runs the
// forward and backward passes of launch_ppo_minibatch under k_a2c_loss, whose means divide by `total`: the chunk's
// gradient is its share of the whole.  first != 0 overwrites the gradient arena and the running sums of the statistics,
// every later chunk adds onto them -- within a chunk in the partials' order, across chunks in the order of the calls.
// net.hyper's adam_eps and clip_eps are not read.
hipError_t launch_a2c_accumulate(const PpoNet &net, const PpoExp &exp, const int32_t *idx, int count, int64_t total,
                                 int first, hipStream_t stream);
// The gradient norm, clip_grad_norm_ and torch.optim.RMSprop's step (momentum 0, not centered, no weight decay) on
// net.grad, the square average in net.exp_avg; the five statistics of the `total` frames accumulated into stats (device
// memory).  one_minus_alpha = (float)(1.0 - alpha) as torch forms it in double.
hipError_t launch_a2c_apply(const PpoNet &net, float lr, float alpha, float one_minus_alpha, float eps, int64_t total,
                            float *stats, hipStream_t stream);

// DIAYN's kept samples: list[0 .. *total) = the sample indexes i in [0, N (T - 1)), ascending, whose keep flag
// mask[(i % (T - 1) + 1) N + i / (T - 1)] is not 0 (mask: [T][N]).  block_count: [blocks + 1] ints, blocks =
// ceil(N (T - 1) / kInvBlock); total: one int (device memory).
hipError_t launch_inv_compact(const float *mask, int N, int T, int32_t *block_count, int32_t *list, int32_t *total,
                              hipStream_t stream);
// counts[s] += the rows of action[0 .. M) that equal s, s in [0, S); a row outside [0, S) is dropped and sets *bad.
// counts is zeroed first.
hipError_t launch_prior_hist(const int32_t *action, int64_t M, int S, int32_t *counts, int *bad, hipStream_t stream);

}  // namespace zenvk
