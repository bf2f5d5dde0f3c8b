// ppo_update.hip -- one PPO minibatch of the flat actor-critic in float32, gfx950: forward, loss, backward, gradient-norm
// clip and Adam (update_parameters, main/src/torch_ac/algos/ppo.py:30-155, recurrence 1) on the network of
// mlp_f32.hip -- ZoneEnvModel (main/src/env_model.py:48-79), PolicyNetwork's Box branch (policy_network.py:39-52) and
// both critics of ACModel (flat_model.py:21-68).  The same launches serve the Zone-goals agent's two learners
// (zone-goals/src/torch_ac/algos/_hier_policy_opt.py:214-370): the low level is this network on [obs, goal] (XD = 10
// where the flat one has 8), the high level this encoder and critic under a per-zone head (PPO_HEAD_ZONES, below).
// And the xy-goals agent's two (xy-goals/src/torch_ac/algos/_hier_policy_opt.py:195-363): its low level is the
// Zone-goals low level on all T frames of an env, its high level the flat network on the dense rows of its windows with
// the loss of k_xyppo_hi_loss.
// And the fixed-length-skills agent's two (main/src/torch_ac/algos/_hier_policy_opt.py:265-419): its low level is the
// Gaussian network on [obs, onehot(skill)] (XD = 8 + S; the one-hot is formed from the recorded skill wherever a product
// reads it and is never stored per zone row), with actor.enc_.0.0 and critic.0 reading [emb, onehot] from an embedding
// buffer 32 columns wider (PpoNet::LDC); its high level is the flat encoder and critic under a Categorical over the S
// skills (PPO_HEAD_SKILLS, k_skppo_hi_loss).
// And the Options agent's two (options/src/torch_ac/algos/_hier_policy_opt.py:208-381): its high level is the skills
// agent's on the rows of the transitions a collection closed, its low level the skills agent's with a third Gaussian
// component (PpoNet::NA = 3) on frames 0 .. T-2, the third component's records read from buffers of their own.
// And DIAYN's discriminator (update_inverse_parameters, main/src/torch_ac/algos/_hier_policy_opt.py:421-447): the flat
// encoder with a ReLU after combine_net.0 under an S-way cross-entropy head (PPO_HEAD_INVERSE, k_inv_loss) on the pairs
// (observation of frame f + 1, skill of frame f) the collection kept (k_inv_count / _scan / _scatter); and the histogram
// of the recorded picks for the learned skill prior's step (k_prior_hist).
// And the flat actor-critic's A2C update (update_parameters, main/src/torch_ac/algos/a2c.py:21-93, recurrence 1): the
// flat network's launches, chunk by chunk, under a loss whose means divide by the frames of the WHOLE update (k_a2c_loss),
// the chunks' weight gradients added onto the arena in a fixed order (k_ppo_reduce<true>, k_a2c_head_bias), the
// statistics carried as running sums (k_a2c_stats), and one clip and RMSprop step behind them (k_a2c_rmsprop).
//
// Every layer is a product on v_mfma_f32_32x32x2_f32, forward and backward, in one of two shapes:
//
//  * k_ppo_nt   Y[row][f] = sum_k W[f][k] X[row][k].  A 32 x 32 result has its row (a zone row or a sample) on the lane
//    and 16 features in the registers.  Both operands are k-contiguous in memory, so lane (r, half) reads one float4 of
//    its weight row and one of its activation row per four MFMAs; the k index a lane half feeds to MFMA t of a group is
//    8 q + 4 half + t for both operands, a permutation of the reduction that leaves the sum what it is.  The forward
//    layers use the padded weights [out][in], the backward-data products their transposes.
//  * k_ppo_tn   dW[n][k] = sum_row dY[row][n] X[row][k].  The reduction runs over rows, both operands are read as
//    they lie (32 consecutive floats of two rows per MFMA).  A wave reduces kPpoChunk rows into a partial of its own;
//    k_ppo_reduce adds the partials of an element in chunk order, in double.  No atomics: the same call from the same
//    state gives the same bits.
//
// Activations are row-major [row][HP], HP = h rounded up to 32 (h <= 191, so a padded column is always free).  Column
// h of every activation is the constant 1 of a valid row: the biases ride in column h of the padded weights, and the
// bias gradients come out as column h of the weight gradients.  Rows past the minibatch are all zero, constant
// included, so they add nothing to any gradient.  The minibatch is gathered by index straight from the time-major
// experience buffers (zone_net_.0's input has no copy); an index outside [0, N T) is never dereferenced: its rows
// read as zero, its sample takes no part in the loss, and a flag tells the host.
//
// The weights the products read are padded images of the parameter arena, rebuilt by k_ppo_prep before every
// minibatch (0.9 MB); the arenas themselves stay in the state_dict's unpadded layout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "ppo_update.hpp"

namespace zenvk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Gather {
    const float *obs, *zone_obs;
    const int32_t *idx;
    int count, N, T, Z, F;
    const float *goal;      // [slot][2]: columns 8-9 of the per-sample input when XD = 10
    int XD, W1C;
    const int32_t *skill;   // [slot]: columns 8 .. 8 + S of the per-sample input are onehot(skill) (S > 0; else null)
    int S;
    // DIAYN's inverse model: the observation's frame is the sample's plus `shift` (the skill stays the sample's frame's),
    // and a sample whose keep flag [the observation's slot] is 0 is dropped.  0 and null for every other learner.
    int shift;
    const float *keep;
};

// where a zone row of the minibatch lies in the experience buffers
struct RowRef {
    bool ok;
    size_t slot;     // frame * N + env
    int z;
    int sk;          // the frame's skill (Gather::skill), checked
};

// sk: the frame's recorded skill where the learner has one (g.skill); one outside [0, S) drops the sample as an index
// out of range does
__device__ __forceinline__ bool sample_slot(const Gather &g, int b, size_t &slot, int &sk)
{
    if (b >= g.count) return false;
    const int i = g.idx[b];
    if (i < 0 || i >= g.N * g.T) return false;       // N T < 2^31: zenv_collect refuses more
    const int env = i / g.T, t = i - env * g.T;      // exps.* flattens [N][T] (base.py:212-227)
    slot = (size_t)(t + g.shift) * g.N + env;
    if (g.skill) {
        sk = g.skill[(size_t)t * g.N + env];
        if (sk < 0 || sk >= g.S) return false;
    }
    if (g.keep && g.keep[slot] == 0.f) return false;
    return true;
}
__device__ __forceinline__ bool sample_slot(const Gather &g, int b, size_t &slot)
{
    int sk = -1;
    return sample_slot(g, b, slot, sk);
}

__device__ __forceinline__ RowRef row_ref(const Gather &g, int row)
{
    RowRef r;
    const int b = row / g.Z;
    r.z = row - b * g.Z;
    r.slot = 0;
    r.sk = -1;
    r.ok = sample_slot(g, b, r.slot, r.sk);
    return r;
}

// zone_net_.0's input [obs (8), goal or onehot(skill) (XD - 8), zone row (F), 0 ..., 1]: the last of the W1C columns (15
// for XD = 8, 23 for XD = 10) is the constant that carries the bias
__device__ __forceinline__ float x0_elem(const Gather &g, const RowRef &r, int k)
{
    if (!r.ok) return 0.f;
    if (k < 8) return g.obs[r.slot * 8 + k];
    if (k < g.XD) return g.skill ? (k - 8 == r.sk ? 1.f : 0.f) : g.goal[r.slot * 2 + (k - 8)];
    if (k < g.XD + g.F) return g.zone_obs[(r.slot * g.Z + r.z) * g.F + (k - g.XD)];
    return k == g.W1C - 1 ? 1.f : 0.f;
}

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

enum { NT_STORE = 0, NT_RELU = 1, NT_MASK = 2, NT_ADD = 3 };

// torch.relu: a NaN stays a NaN (fmaxf(x, 0) would answer 0, and a minibatch on NaN observations would report finite
// losses where the reference reports NaN)
__device__ __forceinline__ float reluf(float x) { return x < 0.f ? 0.f : x; }

// D[row][f] (op)= sum_k A[f][k] B[row][k]; grid = row tiles, block = (64, feature tiles).  A: [32 x tiles][lda], B:
// [32 x row tiles][ldb] or the gathered input, K a multiple of 8.  NT_MASK keeps the product where D held a positive
// activation (the ReLU's derivative) and writes 0 elsewhere; NT_ADD adds to D.
template <int MODE, bool GATHER>
__global__ __launch_bounds__(448) void k_ppo_nt(const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb,
                                                int K, float *D, int ldd, Gather g)
{
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int row = blockIdx.x * 32 + r, f0 = threadIdx.y * 32;
    const float *ap = A + (size_t)(f0 + r) * lda + 4 * hh;
    // eight accumulators, one per MFMA of two groups: chains of K / 16 steps (K / 8 fused multiply-adds) instead of
    // one of K / 2 -- float32's rounding grows with the chain -- and no MFMA waits for the one before it
    f32x16 acc8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc8[u][i] = 0.f;
    const RowRef ref = GATHER ? row_ref(g, row) : RowRef{ false, 0, 0, -1 };
    const float *bp = GATHER ? nullptr : B + (size_t)row * ldb + 4 * hh;
    auto load_b = [&](int q) {
        if (GATHER) {
            const int k = 8 * q + 4 * hh;
            return make_float4(x0_elem(g, ref, k), x0_elem(g, ref, k + 1), x0_elem(g, ref, k + 2), x0_elem(g, ref, k + 3));
        }
        return *reinterpret_cast<const float4 *>(bp + 8 * q);
    };
    const int groups = K / 8;
    int q = 0;
    for (; q + 1 < groups; q += 2) {
        const float4 a0 = *reinterpret_cast<const float4 *>(ap + 8 * q), a1 = *reinterpret_cast<const float4 *>(ap + 8 * q + 8);
        const float4 b0 = load_b(q), b1 = load_b(q + 1);
        acc8[0] = mfma32(a0.x, b0.x, acc8[0]);
        acc8[1] = mfma32(a0.y, b0.y, acc8[1]);
        acc8[2] = mfma32(a0.z, b0.z, acc8[2]);
        acc8[3] = mfma32(a0.w, b0.w, acc8[3]);
        acc8[4] = mfma32(a1.x, b1.x, acc8[4]);
        acc8[5] = mfma32(a1.y, b1.y, acc8[5]);
        acc8[6] = mfma32(a1.z, b1.z, acc8[6]);
        acc8[7] = mfma32(a1.w, b1.w, acc8[7]);
    }
    if (q < groups) {                       // combine_net_'s K = HP + 8: an odd number of groups
        const float4 a0 = *reinterpret_cast<const float4 *>(ap + 8 * q);
        const float4 b0 = load_b(q);
        acc8[0] = mfma32(a0.x, b0.x, acc8[0]);
        acc8[1] = mfma32(a0.y, b0.y, acc8[1]);
        acc8[2] = mfma32(a0.z, b0.z, acc8[2]);
        acc8[3] = mfma32(a0.w, b0.w, acc8[3]);
    }
    const f32x16 acc = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) + ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));
    // register i of lane (r, hh) is feature f0 + (i & 3) + 8 (i >> 2) + 4 hh of row r: four float4 stores
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 *dp = reinterpret_cast<float4 *>(D + (size_t)row * ldd + f0 + 8 * q + 4 * hh);
        float4 v = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
        if (MODE == NT_RELU) v = make_float4(reluf(v.x), reluf(v.y), reluf(v.z), reluf(v.w));
        if (MODE == NT_MASK) {
            const float4 o = *dp;
            v = make_float4(o.x > 0.f ? v.x : 0.f, o.y > 0.f ? v.y : 0.f, o.z > 0.f ? v.z : 0.f, o.w > 0.f ? v.w : 0.f);
        }
        if (MODE == NT_ADD) {
            const float4 o = *dp;
            v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
        }
        *dp = v;
    }
}

// part[chunk][n][k] = sum over the chunk's rows of A[row][n] B[row][k]; grid = (chunks, n tiles), block = (64, k
// tiles).  `rows` is a multiple of 32, so both lane halves make the same number of steps, a multiple of 8.  Columns of B from nB on
// read as 0; GATHER: B is zone_net_.0's gathered input (W1C columns).
template <bool GATHER>
__global__ __launch_bounds__(448) void k_ppo_tn(const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb,
                                                int nB, int rows, float *__restrict__ part, Gather g)
{
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int i0 = blockIdx.y * 32, j0 = threadIdx.y * 32;
    const int row_begin = blockIdx.x * kPpoChunk, row_end = min(rows, row_begin + kPpoChunk);
    const bool col = j0 + r < nB;
    // eight accumulators taking the row pairs in turn (a chunk's rows are a multiple of 32): chains of 16 steps
    f32x16 part8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) part8[u][i] = 0.f;
    for (int row0 = row_begin + hh; row0 < row_end; row0 += 16) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = row0 + 2 * u;
            const float a = A[(size_t)row * lda + i0 + r];
            float b = 0.f;
            if (col) b = GATHER ? x0_elem(g, row_ref(g, row), j0 + r) : B[(size_t)row * ldb + j0 + r];
            part8[u] = mfma32(a, b, part8[u]);
        }
    }
    const f32x16 acc = ((part8[0] + part8[1]) + (part8[2] + part8[3])) + ((part8[4] + part8[5]) + (part8[6] + part8[7]));
    const int m_rows = gridDim.y * 32, ldp = blockDim.y * 32;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = i0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
        part[((size_t)blockIdx.x * m_rows + n) * ldp + j0 + r] = acc[i];
    }
}

// dst[r][dst_col0 + c] = sum over chunks of part[chunk][src_row0 + r][src_col0 + c], in chunk order, in double.
// ADD (the A2C learner's chunks after the first): the sum is added onto what dst holds -- the chain of an element runs on
// from the chunks of the earlier launches -- and rounded once.
template <bool ADD>
__global__ void k_ppo_reduce(const float *__restrict__ part, int chunks, int m_rows, int ldp, int src_row0, int src_col0,
                             float *__restrict__ dst, int dst_ld, int dst_col0, int rows, int cols)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * cols) return;
    const int r = e / cols, c = e - r * cols;
    const float *p = part + (size_t)(src_row0 + r) * ldp + src_col0 + c;
    double s = 0.0;
    for (int ch = 0; ch < chunks; ++ch) s += (double)p[(size_t)ch * m_rows * ldp];
    float *d = dst + (size_t)r * dst_ld + dst_col0 + c;
    *d = ADD ? (float)((double)*d + s) : (float)s;
}

// The same sum with kPpoReduceSplit threads per element: thread (segment, element) adds the partials of its
// contiguous share of the chunks in chunk order in double, the element's first thread then adds the segments in order.
// One chain per element leaves most of the device idle and waiting on memory when a minibatch has hundreds of
// partials (960 for zone_net_.2 at 16 384 samples x 15 zones); the order is still fixed.  Block = 32 elements x
// kPpoReduceSplit segments: a wave half reads 32 consecutive floats.
__global__ __launch_bounds__(32 * kPpoReduceSplit) void k_ppo_reduce_split(
    const float *__restrict__ part, int chunks, int m_rows, int ldp, int src_row0, int src_col0, float *__restrict__ dst,
    int dst_ld, int dst_col0, int rows, int cols)
{
    __shared__ double sh[kPpoReduceSplit][32];
    const int lane = threadIdx.x & 31, seg = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + lane;
    const bool live = e < rows * cols;
    const int r = live ? e / cols : 0, c = live ? e - r * cols : 0;
    const int per = (chunks + kPpoReduceSplit - 1) / kPpoReduceSplit;
    const int ch0 = seg * per, ch1 = min(chunks, ch0 + per);
    double s = 0.0;
    if (live) {
        const float *p = part + (size_t)(src_row0 + r) * ldp + src_col0 + c;
        for (int ch = ch0; ch < ch1; ++ch) s += (double)p[(size_t)ch * m_rows * ldp];
    }
    sh[seg][lane] = s;
    __syncthreads();
    if (seg == 0 && live) {
        double t = sh[0][lane];
#pragma unroll
        for (int k = 1; k < kPpoReduceSplit; ++k) t += sh[k][lane];
        dst[(size_t)r * dst_ld + dst_col0 + c] = (float)t;
    }
}

// ---- the padded weight images
__device__ __forceinline__ float img_square(const float *w, const float *b, int h, int r, int c, bool one, int ld)
{
    if (r < h) return c < h ? w[(size_t)r * ld + c] : c == h ? b[r] : 0.f;
    return one && r == h && c == h ? 1.f : 0.f;
}
__device__ __forceinline__ float img_square(const float *w, const float *b, int h, int r, int c, bool one)
{
    return img_square(w, b, h, r, c, one, h);
}
__device__ __forceinline__ float img_transposed(const float *w, int ld, int col0, int h, int r, int c)
{
    return r < h && c < h ? w[(size_t)c * ld + col0 + r] : 0.f;
}

__global__ void k_ppo_prep(PpoNet n)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x, which = blockIdx.y;
    const int h = n.h, HP = n.HP;
    // DIAYN's inverse model has no enc_ layer and no critic: their images are not allocated.  Its head, combine_net.2,
    // is the skills agent's actor.discrete_.0 in another place of the arena.
    const bool inverse = n.head == PPO_HEAD_INVERSE;
    if (inverse && (which == PPO_I_WE || which == PPO_I_WV || which == PPO_I_HV || which == PPO_T_WE || which == PPO_T_WV ||
                    which == PPO_T_HV))
        return;
    const int ld = which == PPO_I_W1 ? n.W1C : which == PPO_I_WC ? n.KC : (which == PPO_T_HA || which == PPO_T_HV) ? 32
                   : (which == PPO_I_WE || which == PPO_I_WV) ? n.LDC : HP;
    const int n_rows = (which == PPO_I_HA || which == PPO_I_HV) ? 32 : HP;
    if (e >= n_rows * ld) return;
    const int r = e / ld, c = e - r * ld;
    auto T = [&](int t) { return n.param + n.off[t]; };
    const int XD = n.XD, kb = n.W1C - 1;
    const bool zones = n.head == PPO_HEAD_ZONES, skills = n.head == PPO_HEAD_SKILLS || inverse;
    const int hw = inverse ? PPO_INV_W2 : PPO_ACTOR_W2, hb = inverse ? PPO_INV_B2 : PPO_ACTOR_B2;    // the S-way head
    // the skills agent's low level: actor.enc_.0.0 and critic.0 are [h][h + S] over [emb, onehot]; the onehot's columns
    // lie at HP .. HP + S of their images
    const int tail = n.LDC > HP ? n.S : 0;
    // the Gaussian head's columns: NA of mu, NA of std, then the value (the distributional critic's sigma: 5, NA = 2)
    const int NA = n.NA, vr = 2 * NA;
    // the critic's four tensors
    const float *cw1 = T(n.cr), *cb1 = T(n.cr + 1), *cw2 = T(n.cr + 2), *cb2 = T(n.cr + 3);
    float v = 0.f;
    switch (which) {
    case PPO_I_W1:
        if (r < h) v = c < n.K1 ? T(PPO_ZONE_W1)[(size_t)r * n.K1 + c] : c == kb ? T(PPO_ZONE_B1)[r] : 0.f;
        else v = r == h && c == kb ? 1.f : 0.f;
        break;
    case PPO_I_W2: v = img_square(T(PPO_ZONE_W2), T(PPO_ZONE_B2), h, r, c, false); break;
    case PPO_I_W3: v = img_square(T(PPO_ZONE_W3), T(PPO_ZONE_B3), h, r, c, true); break;
    case PPO_I_WC:
        if (r < h) {
            const float *w = T(PPO_COMB_W) + (size_t)r * (XD + h);     // combine_net_'s input is [obs (, goal), zone_emb]
            v = c < h ? w[XD + c] : c == h ? T(PPO_COMB_B)[r] : (c >= HP && c < HP + XD) ? w[c - HP] : 0.f;
        } else {
            v = r == h && c == h ? 1.f : 0.f;
        }
        break;
    // PPO_HEAD_ZONES: actor.0.weight = [W_e | W_z], [h][h + F]; this is W_e with actor.0's bias
    case PPO_I_WE:
        if (c >= HP) v = r < h && c - HP < tail ? T(PPO_ENC_W)[(size_t)r * (h + tail) + h + (c - HP)] : 0.f;
        else v = img_square(T(PPO_ENC_W), T(PPO_ENC_B), h, r, c, true, zones ? h + n.F : h + tail);
        break;
    case PPO_I_WV:
        if (c >= HP) v = r < h && c - HP < tail ? cw1[(size_t)r * (h + tail) + h + (c - HP)] : 0.f;
        else v = img_square(cw1, cb1, h, r, c, true, h + tail);
        break;
    case PPO_I_HA:
        if (zones) {                                  // row 0: actor.2
            if (r == 0 && c <= h) v = c < h ? T(PPO_ACTOR_W2)[c] : T(PPO_ACTOR_B2)[0];
        } else if (skills) {                          // rows 0 .. S: actor.discrete_.0
            if (r < n.S && c <= h) v = c < h ? T(hw)[(size_t)r * h + c] : T(hb)[r];
        } else if (r < 2 * NA && c <= h) {            // rows 0 .. NA: actor.mu_, NA .. 2 NA: actor.std_
            const float *w = T(r < NA ? PPO_MU_W : PPO_STD_W), *b = T(r < NA ? PPO_MU_B : PPO_STD_B);
            const int o = r < NA ? r : r - NA;
            v = c < h ? w[(size_t)o * h + c] : b[o];
        }
        break;
    case PPO_I_HV:                                    // row 2 NA: critic.2 (4 under the other two heads)
        if (c <= h && (r == vr || (r == 5 && n.dist))) {
            const float *w = r == vr ? cw2 : T(PPO_SIGMA_W), *b = r == vr ? cb2 : T(PPO_SIGMA_B);
            v = c < h ? w[c] : b[0];
        }
        break;
    case PPO_T_W2: v = img_transposed(T(PPO_ZONE_W2), h, 0, h, r, c); break;
    case PPO_T_W3: v = img_transposed(T(PPO_ZONE_W3), h, 0, h, r, c); break;
    case PPO_T_WC: v = img_transposed(T(PPO_COMB_W), XD + h, XD, h, r, c); break;
    case PPO_T_WE: v = img_transposed(T(PPO_ENC_W), zones ? h + n.F : h + tail, 0, h, r, c); break;
    case PPO_T_WV: v = img_transposed(cw1, h + tail, 0, h, r, c); break;
    case PPO_T_HA:
        if (zones) {
            if (r < h && c == 0) v = T(PPO_ACTOR_W2)[r];
        } else if (skills) {
            if (r < h && c < n.S) v = T(hw)[(size_t)c * h + r];
        } else if (r < h && c < 2 * NA) v = T(c < NA ? PPO_MU_W : PPO_STD_W)[(size_t)(c < NA ? c : c - NA) * h + r];
        break;
    case PPO_T_HV:
        if (r < h && (c == vr || (c == 5 && n.dist))) v = (c == vr ? cw2 : T(PPO_SIGMA_W))[r];
        break;
    default: break;
    }
    n.img[which][e] = v;
}

// ---- the per-sample pieces between the products
// P = the mean of a sample's zone rows (its column h: the constant), the XD own columns of combine_net_'s input; rows from
// `count` on are zero.  Thread (b, f), f < KC.
__global__ void k_ppo_pool(PpoNet n, Gather g, int bp)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= bp * n.KC) return;
    const int b = e / n.KC, f = e - b * n.KC;
    size_t slot = 0;
    int sk = -1;
    const bool ok = sample_slot(g, b, slot, sk);
    if (f == 0 && b < g.count && !ok) *n.bad_index = 1;
    if (f >= n.HP) {
        const int k = f - n.HP;
        float v = 0.f;
        if (ok && k < 8) v = g.obs[slot * 8 + k];
        else if (ok && k < g.XD) v = g.skill ? (k - 8 == sk ? 1.f : 0.f) : g.goal[slot * 2 + (k - 8)];
        n.CI[(size_t)b * n.KC + f] = v;
        return;
    }
    float v = 0.f;
    if (ok && f < n.h) {
        const float *a = n.A2 + (size_t)b * g.Z * n.HP + f;
        float s = 0.f;
        for (int z = 0; z < g.Z; ++z) s += a[(size_t)z * n.HP];
        v = s / (float)g.Z;                       // .sum(dim=1) / n_zones (env_model.py:77)
    } else if (ok && f == n.h) {
        v = 1.f;
    }
    n.P[(size_t)b * n.HP + f] = v;
}

// dZ2[row][f] = dP[sample][f] / Z where relu(zone_net_.2) was positive, in place over A2
__global__ void k_ppo_spread(PpoNet n, int Z, int rows)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int quads = n.HP / 4;
    if (e >= rows * quads) return;
    const int row = e / quads, q = e - row * quads;
    float4 *ap = reinterpret_cast<float4 *>(n.A2 + (size_t)row * n.HP) + q;
    const float4 a = *ap;
    const float4 d = reinterpret_cast<const float4 *>(n.P + (size_t)(row / Z) * n.HP)[q];
    const float fz = (float)Z;
    *ap = make_float4(a.x > 0.f ? d.x / fz : 0.f, a.y > 0.f ? d.y / fz : 0.f, a.z > 0.f ? d.z / fz : 0.f,
                      a.w > 0.f ? d.w / fz : 0.f);
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// torch.clamp, torch.min and torch.max hand a NaN on where fminf / fmaxf drop it: a NaN ratio or value gives a NaN loss,
// as in the reference
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : x > hi ? hi : x; }

// PPO's clipped surrogate of one sample (ppo.py:76-79): returns -min(surr1, surr2); g_lp = d loss / d log_prob(a), the
// mean's 1 / count included.  dlp = log_prob(a) - the recorded log_prob.
__device__ __forceinline__ float clipped_policy(float dlp, float adv, float clip_eps, float inv_b, float &g_lp)
{
    const float ratio = expf(dlp);
    const float lo = 1.0f - clip_eps, hi = 1.0f + clip_eps;
    const float surr1 = ratio * adv, surr2 = clampf(ratio, lo, hi) * adv;
    // d min(surr1, surr2) / d ratio: adv on the unclipped branch, adv inside the clamp's range, 0 outside
    const float through = surr1 <= surr2 ? 1.0f : (ratio >= lo && ratio <= hi) ? 1.0f : 0.f;
    g_lp = -adv * inv_b * through * ratio;
    return -(surr1 <= surr2 ? surr1 : surr2);
}

// the clipped value loss of one sample (ppo.py:83-86): returns max(s1, s2); dval = d loss / d v with the coefficient
// and the mean's 1 / count
__device__ __forceinline__ float clipped_value(float v, float old, float ret, const PpoHyper &hy, float inv_b, float &dval)
{
    const float dv = v - old;
    const float vc = old + clampf(dv, -hy.clip_eps, hy.clip_eps);
    const float s1 = (v - ret) * (v - ret), s2 = (vc - ret) * (vc - ret);
    const bool inside = dv >= -hy.clip_eps && dv <= hy.clip_eps;
    const float dl = s1 >= s2 ? 2.0f * (v - ret) : inside ? 2.0f * (vc - ret) : 0.f;
    dval = hy.value_loss_coef * inv_b * dl;
    return s1 >= s2 ? s1 : s2;
}

// The loss of one sample (ppo.py:70-89) and its derivative with respect to the six head pre-activations
// (PRE: mu_ 0-1, std_ 2-3, critic.2 / critic_mu 4, critic_sigma 5), scaled by the means' 1 / count.
__global__ void k_ppo_loss(PpoNet n, PpoExp x, Gather g, int bp)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bp) return;
    float d[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, ss[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    size_t slot = 0;
    if (sample_slot(g, b, slot)) {
        const float *pre = n.PRE + (size_t)b * 32;
        const PpoHyper &hy = n.hyper;
        const float inv_b = 1.0f / (float)g.count;
        const float adv = x.advantage[slot], ret = x.returnn[slot];
        float mu[2], sd[2], smu[2], ssd[2], diff[2], dlp = 0.f, ent = 0.f;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            smu[o] = sigmoidf(pre[o]);
            ssd[o] = sigmoidf(pre[2 + o]);
            mu[o] = 2.0f * (smu[o] - 0.5f);                   // policy_network.py:46-47
            sd[o] = ssd[o] + 1e-3f;
            diff[o] = x.action[slot * 2 + o] - mu[o];
            // Normal.log_prob: -(a - mu)^2 / (2 var) - log(std) - log(sqrt(2 pi))
            const float lp = -(diff[o] * diff[o]) / (2.0f * (sd[o] * sd[o])) - logf(sd[o]) - 0.9189385332046727f;
            dlp += lp - x.log_prob[slot * 2 + o];
            ent += 0.5f + 0.9189385332046727f + logf(sd[o]);  // Normal.entropy
        }
        float g_lp;                                           // d loss / d log_prob(a_o), the same for both o
        const float ploss = clipped_policy(dlp, adv, hy.clip_eps, inv_b, g_lp);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const float var = sd[o] * sd[o];
            const float g_mu = g_lp * (diff[o] / var);
            const float g_sd = g_lp * ((diff[o] * diff[o]) / (var * sd[o]) - 1.0f / sd[o])
                               - hy.entropy_coef * (0.5f * inv_b) / sd[o];          // the entropy's mean is over B x 2
            d[o] = g_mu * 2.0f * smu[o] * (1.0f - smu[o]);
            d[2 + o] = g_sd * ssd[o] * (1.0f - ssd[o]);
        }
        const float v = pre[4];
        float vloss, vsig = 0.f;
        if (n.dist) {
            const float bx = 0.3f * pre[5];                   // Softplus(beta = 0.3), threshold 20 (flat_model.py:28,62)
            const float sp = bx > 20.0f ? pre[5] : log1pf(expf(bx)) / 0.3f;
            const float dsp = bx > 20.0f ? 1.0f : sigmoidf(bx);
            vsig = sp + 1e-3f;
            const float dr = ret - v, var = vsig * vsig;
            vloss = (dr * dr) / (2.0f * var) + logf(vsig) + 0.9189385332046727f;    // -Normal(v, sigma).log_prob(returnn)
            const float w = hy.value_loss_coef * inv_b;
            d[4] = w * (-dr / var);
            d[5] = w * (-(dr * dr) / (var * vsig) + 1.0f / vsig) * dsp;
        } else {
            vloss = clipped_value(v, x.value[slot], ret, hy, inv_b, d[4]);
        }
        ss[0] = ent;
        ss[1] = v;
        ss[2] = vsig;
        ss[3] = ploss;
        ss[4] = vloss;
    }
    float *dh = n.DH + (size_t)b * 32;
#pragma unroll
    for (int i = 0; i < 32; ++i) dh[i] = i < 6 ? d[i] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) n.SS[(size_t)b * 8 + i] = ss[i];
}

// The loss of one row of the xy-goals agent's high level (xy-goals/src/torch_ac/algos/_hier_policy_opt.py:288-363) and
// its derivative with respect to the head pre-activations (PRE: mu_ 0-1, std_ 2-3, critic.2 4).  The network is the flat
// one; the "action" is the recorded goal x.action [slot][2], and three things differ from k_ppo_loss:
//   * x.log_prob holds ONE float per row, the recorded log_prob already summed over the goal's two dimensions:
//     dlp = (lp_0 + lp_1) - log_prob[slot];
//   * the entropy is summed over the two dimensions before the mean over rows (k_ppo_stats divides by count, not by
//     2 count), so d loss / d std_o carries entropy_coef / (count std_o) where the flat loss has half of it;
//   * the value loss is always the clipped one: the agent has no distributional critic.
__global__ void k_xyppo_hi_loss(PpoNet n, PpoExp x, Gather g, int bp)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bp) return;
    float d[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, ss[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    size_t slot = 0;
    if (sample_slot(g, b, slot)) {
        const float *pre = n.PRE + (size_t)b * 32;
        const PpoHyper &hy = n.hyper;
        const float inv_b = 1.0f / (float)g.count;
        float sd[2], smu[2], ssd[2], diff[2], lp[2], ent = 0.f;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            smu[o] = sigmoidf(pre[o]);
            ssd[o] = sigmoidf(pre[2 + o]);
            const float mu = 2.0f * (smu[o] - 0.5f);          // policy_network.py:46-47
            sd[o] = ssd[o] + 1e-3f;
            diff[o] = x.action[slot * 2 + o] - mu;
            lp[o] = -(diff[o] * diff[o]) / (2.0f * (sd[o] * sd[o])) - logf(sd[o]) - 0.9189385332046727f;
            ent += 0.5f + 0.9189385332046727f + logf(sd[o]);  // Normal.entropy, .sum(dim=-1)
        }
        float g_lp;                                           // d loss / d log_prob(goal_o), the same for both o
        const float ploss = clipped_policy((lp[0] + lp[1]) - x.log_prob[slot], x.advantage[slot], hy.clip_eps, inv_b, g_lp);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const float var = sd[o] * sd[o];
            const float g_mu = g_lp * (diff[o] / var);
            const float g_sd = g_lp * ((diff[o] * diff[o]) / (var * sd[o]) - 1.0f / sd[o]) - hy.entropy_coef * inv_b / sd[o];
            d[o] = g_mu * 2.0f * smu[o] * (1.0f - smu[o]);
            d[2 + o] = g_sd * ssd[o] * (1.0f - ssd[o]);
        }
        const float v = pre[4];
        ss[0] = ent;
        ss[1] = v;
        ss[3] = ploss;
        ss[4] = clipped_value(v, x.value[slot], x.returnn[slot], hy, inv_b, d[4]);
    }
    float *dh = n.DH + (size_t)b * 32;
#pragma unroll
    for (int i = 0; i < 32; ++i) dh[i] = i < 6 ? d[i] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) n.SS[(size_t)b * 8 + i] = ss[i];
}

// d loss / d logit of one category of a Categorical(logits) whose log-probability is lp (p = exp(lp)) and entropy H:
// g_lp (1[this is the recorded one] - p) from the policy loss, ec p (lp + H) from the entropy's term -ec H.  In double.
__device__ __forceinline__ double categorical_dlogit(float g_lp, double ec, double lp, double H, bool recorded)
{
    const double p = exp(lp);
    return (double)g_lp * ((recorded ? 1.0 : 0.0) - p) + ec * p * (lp + H);
}

// ---- PPO_HEAD_ZONES: the Zone-goals high level's actor (zone-goals/src/hier_policy_value_models.py:19-56), one logit
// per zone from actor.2(relu(actor.0([emb, zone row]))).  With actor.0.weight = [W_e | W_z] the emb part E = W_e emb + b
// is taken once per sample (k_ppo_nt, into Ha; its column h is the constant 1) and
//   U[row][f] = relu(E[sample][f] + sum_k W_z[f][k] zone row[k]),   k in zone-feature order.
// Column h of U stays the constant of a valid row; rows of a dropped sample and rows past the minibatch are zero.
__global__ void k_hppo_head(PpoNet n, Gather g, int rows)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * n.HP) return;
    const int row = e / n.HP, f = e - row * n.HP;
    const RowRef r = row_ref(g, row);
    float v = 0.f;
    if (r.ok && f <= n.h) {
        float s = 0.f;
        if (f < n.h) {
            const float *w = n.param + n.off[PPO_ACTOR_W1] + (size_t)f * (n.h + g.F) + n.h;
            const float *zr = g.zone_obs + (r.slot * g.Z + r.z) * g.F;
            for (int k = 0; k < g.F; ++k) s += w[k] * zr[k];
        }
        v = reluf(n.Ha[(size_t)(row / g.Z) * n.HP + f] + s);
    }
    n.U[(size_t)row * n.HP + f] = v;
}

// The loss of one high-level sample (_hier_policy_opt.py:315-334) and its derivatives: Categorical over the goals that
// were available at the pick (logits[~mask] = -inf).  With p the masked softmax, H = -sum p log p the entropy and g_lp
// as in k_ppo_loss,   d loss / d logit_z = g_lp (1[z = a] - p_z) + (entropy_coef / count) p_z (log p_z + H),
// 0 for an unavailable z.  A recorded goal outside [0, Z) or marked unavailable (a row without an available goal has
// one) drops the sample like an index out of range.  One thread per sample; L, DL: [rows][32], column 0.
// The softmax and the derivatives are formed in double (Z <= 32 terms per sample) and rounded once.  A row's derivatives
// sum to zero -- a shift common to its logits changes nothing -- so actor.2.bias' gradient is 0 for every input; any sum
// of the deltas holds nothing but their rounding (1e-17 even before they are rounded to float32, where float64 autograd
// gives exactly 0 for two zones), so k_ppo_stats writes the 0 itself.
__global__ void k_hppo_loss(PpoNet n, PpoExp x, Gather g, int bp, int rows)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bp) return;
    const int Z = g.Z;
    float d_value = 0.f, ss[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    float g_lp = 0.f;
    double lse = 0.0, H = 0.0, ec = 0.0;
    size_t slot = 0;
    bool ok = sample_slot(g, b, slot);
    int a = -1;
    const uint8_t *mk = nullptr;
    const float *lg = n.L + (size_t)b * Z * 32;
    if (ok) {
        a = x.hi_action[slot];
        mk = x.hi_mask + slot * Z;
        if (a < 0 || a >= Z || !mk[a]) {
            ok = false;
            *n.bad_index = 1;
        }
    }
    if (ok) {
        const PpoHyper &hy = n.hyper;
        const float inv_b = 1.0f / (float)g.count;
        double m = (double)lg[(size_t)a * 32];
        for (int z = 0; z < Z; ++z)
            if (mk[z]) m = fmax(m, (double)lg[(size_t)z * 32]);
        double sum = 0.0;
        for (int z = 0; z < Z; ++z)
            if (mk[z]) sum += exp((double)lg[(size_t)z * 32] - m);
        lse = m + log(sum);
        for (int z = 0; z < Z; ++z)
            if (mk[z]) {
                const double lp = (double)lg[(size_t)z * 32] - lse;
                H -= exp(lp) * lp;
            }
        const float lp_a = (float)((double)lg[(size_t)a * 32] - lse);
        const float ploss = clipped_policy(lp_a - x.log_prob[slot], x.advantage[slot], hy.clip_eps, inv_b, g_lp);
        const float v = n.PRE[(size_t)b * 32 + 4];
        const float vloss = clipped_value(v, x.value[slot], x.returnn[slot], hy, inv_b, d_value);
        ec = (double)hy.entropy_coef * (double)inv_b;
        ss[0] = (float)H;
        ss[1] = v;
        ss[3] = ploss;
        ss[4] = vloss;
    }
    for (int z = 0; z < Z; ++z) {
        const size_t row = (size_t)b * Z + z;
        if (row >= (size_t)rows) break;
        double dz = 0.0;
        if (ok && mk[z]) {
            dz = categorical_dlogit(g_lp, ec, (double)lg[(size_t)z * 32] - lse, H, z == a);
        }
        n.DZ[row] = dz;
        float4 *dl = reinterpret_cast<float4 *>(n.DL + row * 32);
        dl[0] = make_float4((float)dz, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 1; i < 8; ++i) dl[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float *dh = n.DH + (size_t)b * 32;
#pragma unroll
    for (int i = 0; i < 32; ++i) dh[i] = i == 4 ? d_value : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) n.SS[(size_t)b * 8 + i] = ss[i];
}

// S[sample][f] = the sum over the sample's zone rows of actor.0's delta dU[row][f] = [U > 0] actor.2[f] dlogit[row]: the
// delta of E, into Ha.  A unit that is active on every zone row of a sample sees the sum of the row's dlogit, which is
// zero: added up in float32 from the rounded deltas it came out as 1e-9 of noise, and Adam (eps 1e-8) turned that into
// steps of a tenth of lr on rows of W_e whose gradient is zero.  So the sum runs over the unrounded deltas, in z order,
// in double, times actor.2[f], rounded once.  U still holds the activations here.
__global__ void k_hppo_sum(PpoNet n, int Z, int bp, int rows)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= bp * n.HP) return;
    const int b = e / n.HP, f = e - b * n.HP;
    double s = 0.0;
    if (f < n.h) {
        for (int z = 0; z < Z; ++z) {
            const size_t row = (size_t)b * Z + z;
            if (row >= (size_t)rows) break;
            if (n.U[row * n.HP + f] > 0.f) s += n.DZ[row];
        }
        s *= (double)n.param[n.off[PPO_ACTOR_W2] + f];
    }
    n.Ha[(size_t)b * n.HP + f] = (float)s;
}

// ---- PPO_HEAD_SKILLS: the fixed-length-skills agent's high level (main/src/hier_policy_value_models.py:19-43):
// logits = actor.discrete_.0(relu(actor.enc_.0.0(emb))), Categorical(logits = log_softmax(logits)), unmasked.
// The loss of one row (_hier_policy_opt.py:345-419) and its derivatives with respect to the S logits (L, DL: [samples]
// [32], columns 0 .. S) and the value (PRE / DH, column 4): k_hppo_loss' with every skill available and the logits of
// a row side by side.  The log-softmax, the entropy and the derivatives are formed in double and rounded once.  With
// S = 1 the one probability is exactly 1 and every derivative exactly 0, as float64 autograd gives it.  A recorded
// skill outside [0, S) drops the row like an index out of range.  One thread per row.
__global__ void k_skppo_hi_loss(PpoNet n, PpoExp x, Gather g, int bp)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bp) return;
    const int S = n.S;
    float d_value = 0.f, ss[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    float g_lp = 0.f;
    double lse = 0.0, H = 0.0, ec = 0.0;
    size_t slot = 0;
    bool ok = sample_slot(g, b, slot);
    int a = -1;
    const float *lg = n.L + (size_t)b * 32;
    if (ok) {
        a = x.hi_action[slot];
        if (a < 0 || a >= S) {
            ok = false;
            *n.bad_index = 1;
        }
    }
    if (ok) {
        const PpoHyper &hy = n.hyper;
        const float inv_b = 1.0f / (float)g.count;
        double m = (double)lg[a];
        for (int s = 0; s < S; ++s) m = fmax(m, (double)lg[s]);
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += exp((double)lg[s] - m);
        lse = m + log(sum);
        for (int s = 0; s < S; ++s) {
            const double lp = (double)lg[s] - lse;
            H -= exp(lp) * lp;
        }
        const float lp_a = (float)((double)lg[a] - lse);
        const float ploss = clipped_policy(lp_a - x.log_prob[slot], x.advantage[slot], hy.clip_eps, inv_b, g_lp);
        const float v = n.PRE[(size_t)b * 32 + 4];
        const float vloss = clipped_value(v, x.value[slot], x.returnn[slot], hy, inv_b, d_value);
        ec = (double)hy.entropy_coef * (double)inv_b;
        ss[0] = (float)H;
        ss[1] = v;
        ss[3] = ploss;
        ss[4] = vloss;
    }
    float *dl = n.DL + (size_t)b * 32, *dh = n.DH + (size_t)b * 32;
    for (int s = 0; s < 32; ++s)
        dl[s] = ok && s < S ? (float)categorical_dlogit(g_lp, ec, (double)lg[s] - lse, H, s == a) : 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) dh[i] = i == 4 ? d_value : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) n.SS[(size_t)b * 8 + i] = ss[i];
}

// The loss of one sample of the skills agent's low level: k_ppo_loss' loss with the plain critic -- a recorded log_prob
// per action component, the entropy's mean over count x 2 -- formed in double from the float32 pre-activations and
// rounded once, as the high level's is.  In float32 the head's own arithmetic (sigmoid, log_prob, ratio and the products
// of the derivative) is the largest part of the error of the gradients of actor.mu_.bias and actor.std_.bias, two sums
// over the minibatch that cancel to a tenth of their terms: 1e-8 .. 7e-8 at 96 samples, where float32 torch has
// 5e-9 .. 8e-8 and the rounding of the pre-activations adds 1e-9 (DESIGN K15).  The 2 NA + 1 deltas also go to DZ
// [samples][2 NA + 1] before they are rounded: k_skppo_head_bias adds them up for the three head biases.  The flat
// learner's k_ppo_loss stays as it is, and with it the bits of every other learner.
__device__ __forceinline__ double sigmoidd(double x) { return 1.0 / (1.0 + exp(-x)); }

// NA: the action's components, 2 (the skills agent) or 3 (the Options agent, whose third component a_2 is recorded in
// buffers of its own: PpoExp::term_action / term_log_prob [slot]).  The ratio is over all NA components, the entropy's
// mean over count x NA; the head's columns are mu 0 .. NA, std NA .. 2 NA, the value 2 NA.  The NA = 2 instantiation is
// K15's kernel operation for operation.
template <int NA>
__global__ void k_skppo_lo_loss(PpoNet n, PpoExp x, Gather g, int bp)
{
    constexpr int ND = 2 * NA + 1;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bp) return;
    float d[ND], ss[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    double dd[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) d[i] = 0.f, dd[i] = 0.0;
    size_t slot = 0;
    if (sample_slot(g, b, slot)) {
        const float *pre = n.PRE + (size_t)b * 32;
        const PpoHyper &hy = n.hyper;
        const double inv_b = 1.0 / (double)g.count, eps = (double)hy.clip_eps;
        const double adv = (double)x.advantage[slot], ret = (double)x.returnn[slot];
        const double half_log_2pi = 0.9189385332046727;
        // the entropy's mean is over B x NA
        const double ent_w = NA == 2 ? 0.5 * inv_b : inv_b / (double)NA;
        double sd[NA], smu[NA], ssd[NA], diff[NA], dlp = 0.0, ent = 0.0;
#pragma unroll
        for (int o = 0; o < NA; ++o) {
            smu[o] = sigmoidd((double)pre[o]);
            ssd[o] = sigmoidd((double)pre[NA + o]);
            const double mu = 2.0 * (smu[o] - 0.5);               // policy_network.py:46-47
            sd[o] = ssd[o] + 1e-3;
            const float a = o < 2 ? x.action[slot * 2 + o] : x.term_action[slot];
            const float old_lp = o < 2 ? x.log_prob[slot * 2 + o] : x.term_log_prob[slot];
            diff[o] = (double)a - mu;
            const double lp = -(diff[o] * diff[o]) / (2.0 * (sd[o] * sd[o])) - log(sd[o]) - half_log_2pi;
            dlp += lp - (double)old_lp;
            ent += 0.5 + half_log_2pi + log(sd[o]);                // Normal.entropy
        }
        // clipped_policy and clipped_value in double: comparisons, so that a NaN ratio or value gives a NaN loss
        const double ratio = exp(dlp), lo = 1.0 - eps, hi = 1.0 + eps;
        const double surr1 = ratio * adv, surr2 = (ratio < lo ? lo : ratio > hi ? hi : ratio) * adv;
        const double through = surr1 <= surr2 ? 1.0 : (ratio >= lo && ratio <= hi) ? 1.0 : 0.0;
        const double g_lp = -adv * inv_b * through * ratio;
#pragma unroll
        for (int o = 0; o < NA; ++o) {
            const double var = sd[o] * sd[o];
            const double g_mu = g_lp * (diff[o] / var);
            const double g_sd = g_lp * ((diff[o] * diff[o]) / (var * sd[o]) - 1.0 / sd[o])
                                - (double)hy.entropy_coef * ent_w / sd[o];
            dd[o] = g_mu * 2.0 * smu[o] * (1.0 - smu[o]);
            dd[NA + o] = g_sd * ssd[o] * (1.0 - ssd[o]);
        }
        const double v = (double)pre[2 * NA], old = (double)x.value[slot], dv = v - old;
        const double vc = old + (dv < -eps ? -eps : dv > eps ? eps : dv);
        const double s1 = (v - ret) * (v - ret), s2 = (vc - ret) * (vc - ret);
        const bool inside = dv >= -eps && dv <= eps;
        const double dl = s1 >= s2 ? 2.0 * (v - ret) : inside ? 2.0 * (vc - ret) : 0.0;
        dd[2 * NA] = (double)hy.value_loss_coef * inv_b * dl;
#pragma unroll
        for (int i = 0; i < ND; ++i) d[i] = (float)dd[i];
        ss[0] = (float)ent;
        ss[1] = pre[2 * NA];
        ss[3] = (float)(-(surr1 <= surr2 ? surr1 : surr2));
        ss[4] = (float)(s1 >= s2 ? s1 : s2);
    }
#pragma unroll
    for (int i = 0; i < ND; ++i) n.DZ[(size_t)b * ND + i] = dd[i];
    float *dh = n.DH + (size_t)b * 32;
#pragma unroll
    for (int i = 0; i < 32; ++i) dh[i] = i < ND ? d[i] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) n.SS[(size_t)b * 8 + i] = ss[i];
}

// The skills agent's low level: onehot(skill) of every sample into columns HP .. HP + 32 of C, beside the embedding that
// combine_net_ writes into columns 0 .. HP: the input [emb, onehot] of actor.enc_.0.0 and critic.0.  Rows of a dropped
// sample and rows past the minibatch are zero.  Thread (b, k), k < 32.
__global__ void k_skppo_onehot(PpoNet n, Gather g, int bp)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= bp * 32) return;
    const int b = e >> 5, k = e & 31;
    size_t slot = 0;
    int sk = -1;
    const bool ok = sample_slot(g, b, slot, sk);
    n.C[(size_t)b * n.LDC + n.HP + k] = ok && k == sk ? 1.f : 0.f;
}

// a block's fixed-order sum: every thread's double, then a tree over LDS
__device__ __forceinline__ double block_sum_256(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double out = sh[0];
    __syncthreads();
    return out;
}

// The skills agent's low level: the gradients of actor.mu_.bias, actor.std_.bias and critic.2.bias are the sums of the
// head's deltas over the minibatch.  As column h of a float32 product the sum of deltas that are each of order 1 where the
// policy's std is small, and cancel, carried 1e-7 of rounding into gradients of 0.1; so the sums run over the unrounded
// deltas (DZ, k_skppo_lo_loss), in double, in a fixed order, and are rounded once.  Block c of 256 threads: delta c of
// the 2 NA + 1 (NA mu, NA std, critic.2.bias).
__global__ __launch_bounds__(256) void k_skppo_head_bias(PpoNet n, int bp)
{
    __shared__ double sh[256];
    const int c = blockIdx.x;
    double s = 0.0;
    const int NA = n.NA, ND = 2 * NA + 1;
    for (int b = threadIdx.x; b < bp; b += 256) s += n.DZ[(size_t)b * ND + c];
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) {
        float *dst = c < NA ? n.grad + n.off[PPO_MU_B] + c : c < 2 * NA ? n.grad + n.off[PPO_STD_B] + (c - NA)
                                                                        : n.grad + n.off[n.cr + 3];
        *dst = (float)s;
    }
}

// ---- PPO_HEAD_INVERSE: DIAYN's discriminator (main/src/inverse_model.py), logits = combine_net.2(relu(combine_net.0(
// [obs, zone_emb]))), trained by update_inverse_parameters (main/src/torch_ac/algos/_hier_policy_opt.py:421-447):
// CrossEntropyLoss(logits, skill).mean().  The loss of one sample and its derivative with respect to the S logits (L,
// DL: [samples][32], columns 0 .. S): with p = softmax(logits), loss = -log p[skill] and d loss / d logit_s =
// (p_s - 1[s = skill]) / count.  The log-softmax and the derivatives are formed in double and rounded once into DL; the
// unrounded ones go to DZ [samples][S] for k_inv_head_bias.  With S = 1 the one probability is exactly 1: the loss and
// every derivative are exactly 0.  The skill is the one of the sample's own frame, the observation the next frame's
// (Gather::shift); a sample that sample_slot drops -- index, skill or keep flag -- adds nothing.  SS column 0: the loss;
// columns 1-4 stay 0 (k_ppo_stats turns them into the statistics row).  One thread per sample, rows up to bp written.
__global__ void k_inv_loss(PpoNet n, Gather g, int bp)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bp) return;
    const int S = n.S;
    size_t slot = 0;
    int a = -1;
    const bool ok = sample_slot(g, b, slot, a);
    const float *lg = n.L + (size_t)b * 32;
    double lse = 0.0, inv_b = 0.0;
    float loss = 0.f;
    if (ok) {
        inv_b = 1.0 / (double)g.count;
        double m = (double)lg[a];
        for (int s = 0; s < S; ++s) {
            const double v = (double)lg[s];
            m = v > m ? v : m;
        }
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += exp((double)lg[s] - m);
        lse = m + log(sum);
        loss = (float)(lse - (double)lg[a]);
    }
    float *dl = n.DL + (size_t)b * 32;
    for (int s = 0; s < 32; ++s) {
        double dz = 0.0;
        if (ok && s < S) dz = (exp((double)lg[s] - lse) - (s == a ? 1.0 : 0.0)) * inv_b;
        if (s < S) n.DZ[(size_t)b * S + s] = dz;
        dl[s] = (float)dz;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) n.SS[(size_t)b * 8 + i] = i == 0 ? loss : 0.f;
}

// combine_net.2.bias' gradient: the sum over the minibatch of the logits' deltas.  A column's deltas cancel -- p_s over
// every sample against the 1 of the samples of skill s -- so, as k_skppo_head_bias does, the sum runs over the unrounded
// deltas (DZ), in double, in a fixed order, and is rounded once.  Block s of 256 threads: skill s.
__global__ __launch_bounds__(256) void k_inv_head_bias(PpoNet n, int bp)
{
    __shared__ double sh[256];
    const int c = blockIdx.x, S = n.S;
    double s = 0.0;
    for (int b = threadIdx.x; b < bp; b += 256) s += n.DZ[(size_t)b * S + c];
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) n.grad[n.off[PPO_INV_B2] + c] = (float)s;
}

// ---- DIAYN's kept samples (_hier_policy_opt.py:193-199): the sample indexes i in [0, N (T - 1)) whose keep flag --
// the mask of frame i % (T - 1) + 1 of env i / (T - 1) -- is not 0, ascending, which is the reference's env-major
// order.  Three launches: a count per block of kInvBlock indexes, an exclusive scan of the counts, and a scatter in
// which thread t of a block writes its four consecutive indexes behind those of threads 0 .. t - 1.  Every position
// is a sum of integer counts of lower indexes: no atomics, and nothing depends on the order blocks or waves run in.
__device__ __forceinline__ bool inv_kept(const float *mask, int N, int T1, int64_t total, int64_t i)
{
    if (i >= total) return false;
    const int env = (int)(i / T1), f = (int)(i - (int64_t)env * T1);
    return mask[(size_t)(f + 1) * N + env] != 0.f;
}

// the kept ones among a thread's four indexes (bit k: index first + k), and the exclusive sum of the counts of the
// block's threads before it; *block_total: the block's count.  256 threads.
__device__ __forceinline__ int inv_thread_prefix(const float *mask, int N, int T1, int64_t total, unsigned &bits,
                                                 int *sh, int &block_total)
{
    const int64_t first = (int64_t)blockIdx.x * kInvBlock + 4 * (int64_t)threadIdx.x;
    bits = 0;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (inv_kept(mask, N, T1, total, first + k)) bits |= 1u << k, ++c;
    // an inclusive scan over the 256 counts (Hillis-Steele, two buffers)
    int *src = sh, *dst = sh + 256;
    src[threadIdx.x] = c;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        dst[threadIdx.x] = src[threadIdx.x] + ((int)threadIdx.x >= d ? src[threadIdx.x - d] : 0);
        __syncthreads();
        int *t = src;
        src = dst;
        dst = t;
    }
    block_total = src[255];
    return src[threadIdx.x] - c;
}

__global__ __launch_bounds__(256) void k_inv_count(const float *__restrict__ mask, int N, int T1, int64_t total,
                                                   int32_t *__restrict__ block_count)
{
    __shared__ int sh[512];
    unsigned bits;
    int block_total;
    (void)inv_thread_prefix(mask, N, T1, total, bits, sh, block_total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = block_total;
}

// block_count[b] becomes the sum of the counts of blocks 0 .. b - 1, block_count[blocks] and *total the sum of all.  One
// wave: tiles of kInvScan counts in turn, an inclusive scan across the lanes, the tiles before as a carry.
__global__ __launch_bounds__(kInvScan) void k_inv_scan(int32_t *block_count, int blocks, int32_t *total)
{
    const int lane = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < blocks; b0 += kInvScan) {
        const int c = b0 + lane < blocks ? block_count[b0 + lane] : 0;
        int v = c;
#pragma unroll
        for (int d = 1; d < kInvScan; d <<= 1) {
            const int u = __shfl_up(v, d, kInvScan);
            if (lane >= d) v += u;
        }
        if (b0 + lane < blocks) block_count[b0 + lane] = carry + v - c;
        carry += __shfl(v, kInvScan - 1, kInvScan);
    }
    if (lane == 0) {
        block_count[blocks] = carry;
        *total = carry;
    }
}

__global__ __launch_bounds__(256) void k_inv_scatter(const float *__restrict__ mask, int N, int T1, int64_t total,
                                                     const int32_t *__restrict__ block_offset, int32_t *__restrict__ list)
{
    __shared__ int sh[512];
    unsigned bits;
    int block_total;
    int at = block_offset[blockIdx.x] + inv_thread_prefix(mask, N, T1, total, bits, sh, block_total);
    const int64_t first = (int64_t)blockIdx.x * kInvBlock + 4 * (int64_t)threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (bits & (1u << k)) list[at++] = (int32_t)(first + k);
}

// ---- the learned skill prior (update_skill_prior, _hier_policy_opt.py:449-464): the histogram of the M recorded picks.
// Integer counters in LDS, then one integer add per skill and block to the global counters: integer sums do not depend
// on their order.  A pick outside [0, S) is dropped and flagged.
__global__ __launch_bounds__(256) void k_prior_hist(const int32_t *__restrict__ action, int64_t M, int S,
                                                    int32_t *__restrict__ counts, int *bad)
{
    __shared__ int sh[32];
    if (threadIdx.x < 32) sh[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int a = action[i];
        if (a >= 0 && a < S) atomicAdd(&sh[a], 1);
        else *bad = 1;
    }
    __syncthreads();
    if ((int)threadIdx.x < S && sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], sh[threadIdx.x]);
}

// stats[0..4] = the minibatch means of the per-sample terms; one block of 256 threads, thread i adds samples i, i + 256 ...
// ent_terms: the entropy's mean is over count x 2 (the Options agent's low level: 3) action components, or over count
// categoricals or rows whose two components' entropies are already summed (k_xyppo_hi_loss).  zero_grad (or null):
// a gradient that is 0 for every input -- PPO_HEAD_ZONES: actor.2.bias', see k_hppo_loss
__global__ __launch_bounds__(256) void k_ppo_stats(const float *__restrict__ SS, int count, double ent_terms,
                                                   float *__restrict__ stats, float *__restrict__ zero_grad)
{
    __shared__ double sh[256];
    if (zero_grad && threadIdx.x == 0) *zero_grad = 0.f;
    for (int k = 0; k < 5; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < count; b += 256) s += (double)SS[(size_t)b * 8 + k];
        s = block_sum_256(s, sh);
        if (threadIdx.x == 0) stats[k] = (float)(s / (k == 0 ? ent_terms * count : (double)count));
    }
}

// the gradient norm: a partial per kPpoNormBlock elements, then their sum in order
__global__ __launch_bounds__(256) void k_ppo_sumsq(const float *__restrict__ grad, int64_t n, double *__restrict__ part)
{
    __shared__ double sh[256];
    const int64_t base = (int64_t)blockIdx.x * kPpoNormBlock;
    double s = 0.0;
    for (int i = threadIdx.x; i < kPpoNormBlock; i += 256) {
        const int64_t e = base + i;
        if (e < n) {
            const double v = (double)grad[e];
            s += v * v;
        }
    }
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ void k_ppo_norm(const double *__restrict__ part, int n_parts, float *__restrict__ norm, float *__restrict__ stat)
{
    double s = 0.0;
    for (int i = 0; i < n_parts; ++i) s += part[i];
    const float v = (float)sqrt(s);
    *norm = v;
    if (stat) *stat = v;
}

// clip_grad_norm_ and torch.optim.Adam's single-tensor step (betas 0.9 / 0.999, no weight decay, no amsgrad); the
// arenas' padding holds zeros and stays zero
__global__ void k_ppo_adam(PpoNet n, float step_size, float bc2_sqrt)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n.arena) return;
    const float clip = fminf(n.hyper.max_grad_norm / (n.scalars[0] + 1e-6f), 1.0f);
    const float gr = n.grad[e] * clip;
    const float b2 = 0.999f;
    const float w1 = (float)(1.0 - 0.9), w2 = (float)(1.0 - 0.999);
    float m = n.exp_avg[e], v = n.exp_avg_sq[e];
    m = m + w1 * (gr - m);                        // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + (w2 * gr) * gr;                  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + n.hyper.adam_eps;
    n.param[e] = n.param[e] + ((-step_size) * m) / denom;        // param.addcdiv_(exp_avg, denom, value = -step_size)
    n.exp_avg[e] = m;
    n.exp_avg_sq[e] = v;
}

// ---- the A2C learner's statistics and step
// The A2C loss of one sample of a chunk (main/src/torch_ac/algos/a2c.py:51-57) and its derivative with respect to the
// head pre-activations (PRE: mu_ 0-1, std_ 2-3, critic.2 4), the head taken as k_ppo_loss takes it:
//   loss = -mean(log_prob(a) advantage) - entropy_coef mean(entropy) + value_loss_coef mean((value - returnn)^2)
// with log_prob(a) summed over the action's two components (as ppo.py:73-76 sums them), the entropy's mean over samples x 2,
// no ratio, no clip, no recorded log_prob and no value clipping.  Every mean divides by `total`, the frames of the whole
// update, not by the chunk's count: the chunk's deltas are its share of the update's.
// Formed in double from the float32 pre-activations and rounded once, as k_skppo_lo_loss forms its loss and for its
// reason: the gradients of actor.mu_.bias, actor.std_.bias and critic.2.bias are sums over the frames that cancel, and
// float32 arithmetic in the head put 8.8 x 2^-24 of its scale into actor.mu_.bias' at 33 frames (DESIGN K23).  The five unrounded deltas go to DZ
// [samples][5] for k_a2c_head_bias.
__global__ void k_a2c_loss(PpoNet n, PpoExp x, Gather g, int bp, double inv_total)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bp) return;
    float ss[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    double dd[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    size_t slot = 0;
    if (sample_slot(g, b, slot)) {
        const float *pre = n.PRE + (size_t)b * 32;
        const PpoHyper &hy = n.hyper;
        const double adv = (double)x.advantage[slot], ret = (double)x.returnn[slot];
        const double half_log_2pi = 0.9189385332046727;
        double sd[2], smu[2], ssd[2], diff[2], lp = 0.0, ent = 0.0;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            smu[o] = sigmoidd((double)pre[o]);
            ssd[o] = sigmoidd((double)pre[2 + o]);
            const double mu = 2.0 * (smu[o] - 0.5);               // policy_network.py:46-47
            sd[o] = ssd[o] + 1e-3;
            diff[o] = (double)x.action[slot * 2 + o] - mu;
            // Normal.log_prob: -(a - mu)^2 / (2 var) - log(std) - log(sqrt(2 pi))
            lp += -(diff[o] * diff[o]) / (2.0 * (sd[o] * sd[o])) - log(sd[o]) - half_log_2pi;
            ent += 0.5 + half_log_2pi + log(sd[o]);                // Normal.entropy
        }
        const double g_lp = -adv * inv_total;                     // d loss / d log_prob(a_o), the same for both o
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const double var = sd[o] * sd[o];
            const double g_mu = g_lp * (diff[o] / var);
            const double g_sd = g_lp * ((diff[o] * diff[o]) / (var * sd[o]) - 1.0 / sd[o])
                                - (double)hy.entropy_coef * (0.5 * inv_total) / sd[o];   // the mean is over total x 2
            dd[o] = g_mu * 2.0 * smu[o] * (1.0 - smu[o]);
            dd[2 + o] = g_sd * ssd[o] * (1.0 - ssd[o]);
        }
        const double v = (double)pre[4];
        dd[4] = (double)hy.value_loss_coef * inv_total * (2.0 * (v - ret));
        ss[0] = (float)ent;
        ss[1] = pre[4];
        ss[3] = (float)(-(lp * adv));
        ss[4] = (float)((v - ret) * (v - ret));
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) n.DZ[(size_t)b * 5 + i] = dd[i];
    float *dh = n.DH + (size_t)b * 32;
#pragma unroll
    for (int i = 0; i < 32; ++i) dh[i] = i < 5 ? (float)dd[i] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) n.SS[(size_t)b * 8 + i] = ss[i];
}

// The gradients of actor.mu_.bias, actor.std_.bias and critic.2.bias: the chunk's sums of the unrounded deltas (DZ), in
// double, in block_sum_256's order; the first chunk's is rounded into the arena, a later chunk's added onto what the arena
// holds and rounded once.  Block c of 256 threads: delta c of the five.
__global__ __launch_bounds__(256) void k_a2c_head_bias(PpoNet n, int bp, int first)
{
    __shared__ double sh[256];
    const int c = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < bp; b += 256) s += n.DZ[(size_t)b * 5 + c];
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) {
        float *dst = c < 2 ? n.grad + n.off[PPO_MU_B] + c : c < 4 ? n.grad + n.off[PPO_STD_B] + (c - 2)
                                                                  : n.grad + n.off[n.cr + 3];
        *dst = first ? (float)s : (float)((double)*dst + s);
    }
}

// sums[0 .. 4) (+)= the chunk's sums of the per-sample terms (SS columns 0, 1, 3, 4: entropy, value, policy loss, value
// loss), in double: k_ppo_stats' sums carried from chunk to chunk instead of divided.  One block of 256 threads; the first
// chunk overwrites.  The order within a chunk is block_sum_256's, across chunks that of the launches.
__global__ __launch_bounds__(256) void k_a2c_stats(const float *__restrict__ SS, int count, int first, double *__restrict__ sums)
{
    __shared__ double sh[256];
    for (int k = 0; k < 4; ++k) {
        const int col = k < 2 ? k : k + 1;
        double s = 0.0;
        for (int b = threadIdx.x; b < count; b += 256) s += (double)SS[(size_t)b * 8 + col];
        s = block_sum_256(s, sh);
        if (threadIdx.x == 0) sums[k] = first ? s : sums[k] + s;
    }
}

// stats[0 .. 4) = the means over the update's `total` frames (the entropy's over total x 2 components); stats[4], the
// gradient norm, is k_ppo_norm's
__global__ void k_a2c_finish(const double *__restrict__ sums, double total, float *__restrict__ stats)
{
    const int k = threadIdx.x;
    if (k < 4) stats[k] = (float)(sums[k] / (k == 0 ? 2.0 * total : total));
}

// clip_grad_norm_ and torch.optim.RMSprop's single-tensor step with momentum 0, not centered, no weight decay:
//   square_avg.mul_(alpha).addcmul_(grad, grad, value = 1 - alpha);  avg = square_avg.sqrt().add_(eps);
//   param.addcdiv_(grad, avg, value = -lr)
// (eps is added after the square root).  Four elements per thread and step through 16-byte loads and stores, grid-stride
// over the arena (a multiple of 64 floats).  The padding holds zeros and stays zero: 0 / (0 + eps).  The gradient arena
// is read only: it keeps the unclipped gradient.
__global__ __launch_bounds__(256) void k_a2c_rmsprop(PpoNet n, float lr, float alpha, float one_minus_alpha, float eps)
{
    const float clip = fminf(n.hyper.max_grad_norm / (n.scalars[0] + 1e-6f), 1.0f);
    const int64_t quads = n.arena / 4, stride = (int64_t)gridDim.x * blockDim.x;
    float4 *param = reinterpret_cast<float4 *>(n.param), *sq = reinterpret_cast<float4 *>(n.exp_avg);
    const float4 *grad = reinterpret_cast<const float4 *>(n.grad);
    auto step = [&](float &p, float &v, float gr) {
        gr *= clip;
        v = v * alpha + (one_minus_alpha * gr) * gr;
        const float avg = sqrtf(v) + eps;
        p = p + ((-lr) * gr) / avg;
    };
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
        float4 p = param[q], v = sq[q];
        const float4 gr = grad[q];
        step(p.x, v.x, gr.x);
        step(p.y, v.y, gr.y);
        step(p.z, v.z, gr.z);
        step(p.w, v.w, gr.w);
        param[q] = p;
        sq[q] = v;
    }
}

Gather no_gather() { return Gather{ nullptr, nullptr, nullptr, 0, 1, 1, 1, 0, nullptr, 8, 16, nullptr, 0, 0, nullptr }; }

template <int MODE>
void nt(const float *A, int lda, const float *B, int ldb, int K, float *D, int ldd, int rows, int m_tiles,
        hipStream_t s)
{
    hipLaunchKernelGGL((k_ppo_nt<MODE, false>), dim3(rows / 32), dim3(64, m_tiles), 0, s, A, lda, B, ldb, K, D, ldd,
                       no_gather());
}

void tn(const float *A, int lda, int m_tiles, const float *B, int ldb, int nB, int rows, float *part, hipStream_t s)
{
    const int chunks = (rows + kPpoChunk - 1) / kPpoChunk;
    hipLaunchKernelGGL((k_ppo_tn<false>), dim3(chunks, m_tiles), dim3(64, (nB + 31) / 32), 0, s, A, lda, B, ldb, nB, rows,
                       part, no_gather());
}

// one piece of a weight gradient out of the partials of the last tn(): rows x cols from (src_row0, src_col0)
void reduce(const PpoNet &n, int rows_reduced, int m_tiles, int nB, int src_row0, int src_col0, int tensor, int dst_ld,
            int dst_col0, int rows, int cols, hipStream_t s)
{
    const int chunks = (rows_reduced + kPpoChunk - 1) / kPpoChunk;
    const int total = rows * cols;
    if (n.split_reduce && chunks > kPpoReduceSplit) {
        hipLaunchKernelGGL(k_ppo_reduce_split, dim3((total + 31) / 32), dim3(32 * kPpoReduceSplit), 0, s, n.partial, chunks,
                           m_tiles * 32, ((nB + 31) / 32) * 32, src_row0, src_col0, n.grad + n.off[tensor], dst_ld, dst_col0,
                           rows, cols);
        return;
    }
    if (n.accumulate) {
        hipLaunchKernelGGL(k_ppo_reduce<true>, dim3((total + 255) / 256), dim3(256), 0, s, n.partial, chunks, m_tiles * 32,
                           ((nB + 31) / 32) * 32, src_row0, src_col0, n.grad + n.off[tensor], dst_ld, dst_col0, rows, cols);
        return;
    }
    hipLaunchKernelGGL(k_ppo_reduce<false>, dim3((total + 255) / 256), dim3(256), 0, s, n.partial, chunks, m_tiles * 32,
                       ((nB + 31) / 32) * 32, src_row0, src_col0, n.grad + n.off[tensor], dst_ld, dst_col0, rows, cols);
}

void launch_norm(const PpoNet &n, float *stat, hipStream_t s)
{
    const int parts = (int)((n.arena + kPpoNormBlock - 1) / kPpoNormBlock);
    hipLaunchKernelGGL(k_ppo_sumsq, dim3(parts), dim3(256), 0, s, n.grad, n.arena, n.norm_partial);
    hipLaunchKernelGGL(k_ppo_norm, dim3(1), dim3(1), 0, s, n.norm_partial, parts, n.scalars, stat);
}

// the two heads between the encoder's forward and backward passes: C holds the embedding going in, its delta coming out
// the A2C learner's chunk (launch_a2c_accumulate); null for every PPO learner
struct A2cPass {
    int64_t total;
    int first;
};

void gaussian_head(const PpoNet &n, const PpoExp &x, const Gather &g, int bp, float *stats, hipStream_t s,
                   const A2cPass *a2c = nullptr)
{
    const int h = n.h, HP = n.HP, NT = HP / 32, cr = n.cr, LDC = n.LDC;
    // the skills agent's low level: C is [emb | onehot(skill)] and actor.enc_.0.0 / critic.0 are [h][h + S]
    const int tail = LDC > HP ? n.S : 0, ldw = h + tail;
    const int NA = n.NA;        // the action's components: mu in columns 0 .. NA of PRE / DH, std NA .. 2 NA, the value 2 NA
    float *const *I = n.img;
    if (tail) hipLaunchKernelGGL(k_skppo_onehot, dim3((bp * 32 + 255) / 256), dim3(256), 0, s, n, g, bp);
    nt<NT_RELU>(I[PPO_I_WE], LDC, n.C, LDC, LDC, n.Ha, HP, bp, NT, s);                    // relu(actor.enc_)
    nt<NT_RELU>(I[PPO_I_WV], LDC, n.C, LDC, LDC, n.Hc, HP, bp, NT, s);                    // relu(critic.0)
    nt<NT_STORE>(I[PPO_I_HA], HP, n.Ha, HP, HP, n.PRE, 32, bp, 1, s);                     // mu_, std_
    nt<NT_ADD>(I[PPO_I_HV], HP, n.Hc, HP, HP, n.PRE, 32, bp, 1, s);                       // critic.2 / critic_mu, critic_sigma
    if (a2c) {                                                // no ratio, the means over the whole update's frames
        hipLaunchKernelGGL(k_a2c_loss, dim3((bp + 63) / 64), dim3(64), 0, s, n, x, g, bp, 1.0 / (double)a2c->total);
        hipLaunchKernelGGL(k_a2c_stats, dim3(1), dim3(256), 0, s, n.SS, g.count, a2c->first, n.run_sums);
    } else if (n.loss == PPO_LOSS_JOINT_GOAL) {               // the entropy's mean is over the rows alone
        hipLaunchKernelGGL(k_xyppo_hi_loss, dim3((bp + 63) / 64), dim3(64), 0, s, n, x, g, bp);
        hipLaunchKernelGGL(k_ppo_stats, dim3(1), dim3(256), 0, s, n.SS, g.count, 1.0, stats, (float *)nullptr);
    } else {
        if (tail && NA == 3) hipLaunchKernelGGL(k_skppo_lo_loss<3>, dim3((bp + 63) / 64), dim3(64), 0, s, n, x, g, bp);
        else if (tail) hipLaunchKernelGGL(k_skppo_lo_loss<2>, dim3((bp + 63) / 64), dim3(64), 0, s, n, x, g, bp);
        else hipLaunchKernelGGL(k_ppo_loss, dim3((bp + 63) / 64), dim3(64), 0, s, n, x, g, bp);
        hipLaunchKernelGGL(k_ppo_stats, dim3(1), dim3(256), 0, s, n.SS, g.count, (double)NA, stats, (float *)nullptr);
    }
    // ---- backward: every weight gradient is taken before its layer's activations are overwritten by deltas
    tn(n.DH, 32, 1, n.Ha, HP, HP, bp, n.partial, s);
    reduce(n, bp, 1, HP, 0, 0, PPO_MU_W, h, 0, NA, h, s);
    const bool col_bias = !tail && !a2c;       // the three head biases as column h of the products (else: from DZ)
    if (col_bias) reduce(n, bp, 1, HP, 0, h, PPO_MU_B, 1, 0, NA, 1, s);
    reduce(n, bp, 1, HP, NA, 0, PPO_STD_W, h, 0, NA, h, s);
    if (col_bias) reduce(n, bp, 1, HP, NA, h, PPO_STD_B, 1, 0, NA, 1, s);
    tn(n.DH, 32, 1, n.Hc, HP, HP, bp, n.partial, s);
    reduce(n, bp, 1, HP, 2 * NA, 0, cr + 2, h, 0, 1, h, s);
    if (col_bias) reduce(n, bp, 1, HP, 2 * NA, h, cr + 3, 1, 0, 1, 1, s);
    else if (a2c) hipLaunchKernelGGL(k_a2c_head_bias, dim3(5), dim3(256), 0, s, n, bp, a2c->first);
    else hipLaunchKernelGGL(k_skppo_head_bias, dim3(2 * NA + 1), dim3(256), 0, s, n, bp); // the three head biases
    if (n.dist) {
        reduce(n, bp, 1, HP, 5, 0, PPO_SIGMA_W, h, 0, 1, h, s);
        reduce(n, bp, 1, HP, 5, h, PPO_SIGMA_B, 1, 0, 1, 1, s);
    }
    nt<NT_MASK>(I[PPO_T_HA], 32, n.DH, 32, 32, n.Ha, HP, bp, NT, s);                      // delta of actor.enc_
    nt<NT_MASK>(I[PPO_T_HV], 32, n.DH, 32, 32, n.Hc, HP, bp, NT, s);                      // delta of critic.0
    tn(n.Ha, HP, NT, n.C, LDC, LDC, bp, n.partial, s);
    reduce(n, bp, NT, LDC, 0, 0, PPO_ENC_W, ldw, 0, h, h, s);
    if (tail) reduce(n, bp, NT, LDC, 0, HP, PPO_ENC_W, ldw, h, h, tail, s);               // the onehot's columns
    reduce(n, bp, NT, LDC, 0, h, PPO_ENC_B, 1, 0, h, 1, s);
    tn(n.Hc, HP, NT, n.C, LDC, LDC, bp, n.partial, s);
    reduce(n, bp, NT, LDC, 0, 0, cr, ldw, 0, h, h, s);
    if (tail) reduce(n, bp, NT, LDC, 0, HP, cr, ldw, h, h, tail, s);
    reduce(n, bp, NT, LDC, 0, h, cr + 1, 1, 0, h, 1, s);
    // the onehot has no delta: the embedding's comes from the first h columns of both weights
    nt<NT_STORE>(I[PPO_T_WE], HP, n.Ha, HP, HP, n.C, LDC, bp, NT, s);                     // delta of the embedding ...
    nt<NT_ADD>(I[PPO_T_WV], HP, n.Hc, HP, HP, n.C, LDC, bp, NT, s);                       // ... from both heads
}

// PPO_HEAD_SKILLS: gaussian_head with the S logits of actor.discrete_.0 in L / DL where it has mu_ and std_ in PRE / DH
void skill_head(const PpoNet &n, const PpoExp &x, const Gather &g, int bp, float *stats, hipStream_t s)
{
    const int h = n.h, HP = n.HP, NT = HP / 32, cr = n.cr, S = n.S;
    float *const *I = n.img;
    nt<NT_RELU>(I[PPO_I_WE], HP, n.C, HP, HP, n.Ha, HP, bp, NT, s);                       // relu(actor.enc_)
    nt<NT_RELU>(I[PPO_I_WV], HP, n.C, HP, HP, n.Hc, HP, bp, NT, s);                       // relu(critic.0)
    nt<NT_STORE>(I[PPO_I_HA], HP, n.Ha, HP, HP, n.L, 32, bp, 1, s);                       // actor.discrete_.0: S logits
    nt<NT_STORE>(I[PPO_I_HV], HP, n.Hc, HP, HP, n.PRE, 32, bp, 1, s);                     // critic.2
    hipLaunchKernelGGL(k_skppo_hi_loss, dim3((bp + 63) / 64), dim3(64), 0, s, n, x, g, bp);
    hipLaunchKernelGGL(k_ppo_stats, dim3(1), dim3(256), 0, s, n.SS, g.count, 1.0, stats, (float *)nullptr);
    // ---- backward
    tn(n.DL, 32, 1, n.Ha, HP, HP, bp, n.partial, s);
    reduce(n, bp, 1, HP, 0, 0, PPO_ACTOR_W2, h, 0, S, h, s);
    reduce(n, bp, 1, HP, 0, h, PPO_ACTOR_B2, 1, 0, S, 1, s);
    tn(n.DH, 32, 1, n.Hc, HP, HP, bp, n.partial, s);
    reduce(n, bp, 1, HP, 4, 0, cr + 2, h, 0, 1, h, s);
    reduce(n, bp, 1, HP, 4, h, cr + 3, 1, 0, 1, 1, s);
    nt<NT_MASK>(I[PPO_T_HA], 32, n.DL, 32, 32, n.Ha, HP, bp, NT, s);                      // delta of actor.enc_
    nt<NT_MASK>(I[PPO_T_HV], 32, n.DH, 32, 32, n.Hc, HP, bp, NT, s);                      // delta of critic.0
    tn(n.Ha, HP, NT, n.C, HP, HP, bp, n.partial, s);
    reduce(n, bp, NT, HP, 0, 0, PPO_ENC_W, h, 0, h, h, s);
    reduce(n, bp, NT, HP, 0, h, PPO_ENC_B, 1, 0, h, 1, s);
    tn(n.Hc, HP, NT, n.C, HP, HP, bp, n.partial, s);
    reduce(n, bp, NT, HP, 0, 0, cr, h, 0, h, h, s);
    reduce(n, bp, NT, HP, 0, h, cr + 1, 1, 0, h, 1, s);
    nt<NT_STORE>(I[PPO_T_WE], HP, n.Ha, HP, HP, n.C, HP, bp, NT, s);                      // delta of the embedding ...
    nt<NT_ADD>(I[PPO_T_WV], HP, n.Hc, HP, HP, n.C, HP, bp, NT, s);                        // ... from actor and critic
}

// PPO_HEAD_INVERSE: C holds relu(combine_net.0) going in, combine_net.0's delta coming out
void inverse_head(const PpoNet &n, const Gather &g, int bp, float *stats, hipStream_t s)
{
    const int h = n.h, HP = n.HP, NT = HP / 32, S = n.S;
    float *const *I = n.img;
    nt<NT_STORE>(I[PPO_I_HA], HP, n.C, HP, HP, n.L, 32, bp, 1, s);                        // combine_net.2: S logits
    hipLaunchKernelGGL(k_inv_loss, dim3((bp + 63) / 64), dim3(64), 0, s, n, g, bp);
    hipLaunchKernelGGL(k_ppo_stats, dim3(1), dim3(256), 0, s, n.SS, g.count, 1.0, stats, (float *)nullptr);
    // ---- backward
    tn(n.DL, 32, 1, n.C, HP, HP, bp, n.partial, s);
    reduce(n, bp, 1, HP, 0, 0, PPO_INV_W2, h, 0, S, h, s);
    hipLaunchKernelGGL(k_inv_head_bias, dim3(S), dim3(256), 0, s, n, bp);                 // combine_net.2.bias
    nt<NT_MASK>(I[PPO_T_HA], 32, n.DL, 32, 32, n.C, HP, bp, NT, s);                       // delta of combine_net.0
}

void zone_head(const PpoNet &n, const PpoExp &x, const Gather &g, int rp, int bp, float *stats, hipStream_t s)
{
    const int h = n.h, HP = n.HP, NT = HP / 32, cr = n.cr, F = n.F;
    const int chunks = (rp + kPpoChunk - 1) / kPpoChunk;
    float *const *I = n.img;
    nt<NT_STORE>(I[PPO_I_WE], HP, n.C, HP, HP, n.Ha, HP, bp, NT, s);                      // E = W_e emb + b
    nt<NT_RELU>(I[PPO_I_WV], HP, n.C, HP, HP, n.Hc, HP, bp, NT, s);                       // relu(critic.0)
    hipLaunchKernelGGL(k_hppo_head, dim3((unsigned)(((int64_t)rp * HP + 255) / 256)), dim3(256), 0, s, n, g, rp);
    nt<NT_STORE>(I[PPO_I_HA], HP, n.U, HP, HP, n.L, 32, rp, 1, s);                        // actor.2: a logit per zone row
    nt<NT_STORE>(I[PPO_I_HV], HP, n.Hc, HP, HP, n.PRE, 32, bp, 1, s);                     // critic.2
    hipLaunchKernelGGL(k_hppo_loss, dim3((bp + 63) / 64), dim3(64), 0, s, n, x, g, bp, rp);
    hipLaunchKernelGGL(k_ppo_stats, dim3(1), dim3(256), 0, s, n.SS, g.count, 1.0, stats,
                       n.grad + n.off[PPO_ACTOR_B2]);               // and actor.2.bias' gradient
    // ---- backward
    tn(n.DL, 32, 1, n.U, HP, HP, rp, n.partial, s);
    reduce(n, rp, 1, HP, 0, 0, PPO_ACTOR_W2, h, 0, 1, h, s);
    tn(n.DH, 32, 1, n.Hc, HP, HP, bp, n.partial, s);
    reduce(n, bp, 1, HP, 4, 0, cr + 2, h, 0, 1, h, s);
    reduce(n, bp, 1, HP, 4, h, cr + 3, 1, 0, 1, 1, s);
    hipLaunchKernelGGL(k_hppo_sum, dim3((bp * HP + 255) / 256), dim3(256), 0, s, n, n.Z, bp, rp);   // S, the delta of E
    nt<NT_MASK>(I[PPO_T_HA], 32, n.DL, 32, 32, n.U, HP, rp, NT, s);                       // dU, the delta of actor.0
    nt<NT_MASK>(I[PPO_T_HV], 32, n.DH, 32, 32, n.Hc, HP, bp, NT, s);                      // delta of critic.0
    // d W_z = sum over the zone rows of dU x the row's zone features: columns XD .. XD + F of the gathered input
    hipLaunchKernelGGL((k_ppo_tn<true>), dim3(chunks, NT), dim3(64, (n.W1C + 31) / 32), 0, s, n.U, HP, nullptr, 0, n.W1C, rp,
                       n.partial, g);
    reduce(n, rp, NT, n.W1C, 0, n.XD, PPO_ACTOR_W1, h + F, h, h, F, s);
    tn(n.Ha, HP, NT, n.C, HP, HP, bp, n.partial, s);                                      // d W_e and actor.0's bias
    reduce(n, bp, NT, HP, 0, 0, PPO_ACTOR_W1, h + F, 0, h, h, s);
    reduce(n, bp, NT, HP, 0, h, PPO_ACTOR_B1, 1, 0, h, 1, s);
    tn(n.Hc, HP, NT, n.C, HP, HP, bp, n.partial, s);
    reduce(n, bp, NT, HP, 0, 0, cr, h, 0, h, h, s);
    reduce(n, bp, NT, HP, 0, h, cr + 1, 1, 0, h, 1, s);
    nt<NT_STORE>(I[PPO_T_WE], HP, n.Ha, HP, HP, n.C, HP, bp, NT, s);                      // delta of the embedding ...
    nt<NT_ADD>(I[PPO_T_WV], HP, n.Hc, HP, HP, n.C, HP, bp, NT, s);                        // ... from actor and critic
}

}  // namespace

// forward, loss and backward of one minibatch; a2c: the A2C learner's chunk, which leaves the norm to its apply
static hipError_t minibatch(const PpoNet &n, const PpoExp &x, const int32_t *idx, int count, float *stats, hipStream_t s,
                            const A2cPass *a2c)
{
    const int h = n.h, HP = n.HP, KC = n.KC, NT = HP / 32, XD = n.XD, W1C = n.W1C, LDC = n.LDC;
    const int rp = (count * n.Z + 31) / 32 * 32, bp = (count + 31) / 32 * 32;
    const Gather g{ x.obs, x.zone_obs, idx, count, x.N, x.T, n.Z, n.F, x.goal, XD, W1C, x.skill, x.skill ? n.S : 0,
                    x.obs_shift, x.keep };
    float *const *I = n.img;
    // the widest image: combine_net_'s [HP][KC], or actor.enc_.0.0's [HP][LDC] (zone_net_.0's W1C <= 48 <= KC)
    const int wide = KC > LDC ? KC : LDC;
    hipLaunchKernelGGL(k_ppo_prep, dim3((HP * wide + 255) / 256, PPO_N_IMAGES), dim3(256), 0, s, n);
    // ---- forward
    hipLaunchKernelGGL((k_ppo_nt<NT_RELU, true>), dim3(rp / 32), dim3(64, NT), 0, s, I[PPO_I_W1], W1C, nullptr, 0, W1C,
                       n.A1, HP, g);                                                      // relu(zone_net_.0)
    nt<NT_RELU>(I[PPO_I_W2], HP, n.A1, HP, HP, n.A2, HP, rp, NT, s);                      // relu(zone_net_.2)
    hipLaunchKernelGGL(k_ppo_pool, dim3((bp * KC + 255) / 256), dim3(256), 0, s, n, g, bp);
    nt<NT_STORE>(I[PPO_I_W3], HP, n.P, HP, HP, n.CI, KC, bp, NT, s);                      // zone_net_.4 of the mean
    if (n.head == PPO_HEAD_INVERSE) {
        nt<NT_RELU>(I[PPO_I_WC], KC, n.CI, KC, KC, n.C, LDC, bp, NT, s);                  // relu(combine_net.0)
        inverse_head(n, g, bp, stats, s);
    } else {
        nt<NT_STORE>(I[PPO_I_WC], KC, n.CI, KC, KC, n.C, LDC, bp, NT, s);                 // combine_net_
        if (n.head == PPO_HEAD_ZONES) zone_head(n, x, g, rp, bp, stats, s);
        else if (n.head == PPO_HEAD_SKILLS) skill_head(n, x, g, bp, stats, s);
        else gaussian_head(n, x, g, bp, stats, s, a2c);
    }
    // ---- the encoder's backward pass, from the embedding's delta in C
    if ((KC + 31) / 32 <= 7) {
        tn(n.C, LDC, NT, n.CI, KC, KC, bp, n.partial, s);
        reduce(n, bp, NT, KC, 0, 0, PPO_COMB_W, XD + h, XD, h, h, s);
        reduce(n, bp, NT, KC, 0, HP, PPO_COMB_W, XD + h, 0, h, XD, s);
        reduce(n, bp, NT, KC, 0, h, PPO_COMB_B, 1, 0, h, 1, s);
    } else {
        // HP = 192 with more than 32 own columns: eight k tiles would be 512 threads where k_ppo_tn is built for 448.
        // The product is taken in two by columns, zone_emb's HP and the own ones; an element's sum is what it would be.
        tn(n.C, LDC, NT, n.CI, KC, HP, bp, n.partial, s);
        reduce(n, bp, NT, HP, 0, 0, PPO_COMB_W, XD + h, XD, h, h, s);
        reduce(n, bp, NT, HP, 0, h, PPO_COMB_B, 1, 0, h, 1, s);
        tn(n.C, LDC, NT, n.CI + HP, KC, KC - HP, bp, n.partial, s);
        reduce(n, bp, NT, KC - HP, 0, 0, PPO_COMB_W, XD + h, 0, h, XD, s);
    }
    nt<NT_STORE>(I[PPO_T_WC], HP, n.C, LDC, HP, n.CI, KC, bp, NT, s);                     // delta of zone_net_.4's output
    tn(n.CI, KC, NT, n.P, HP, HP, bp, n.partial, s);
    reduce(n, bp, NT, HP, 0, 0, PPO_ZONE_W3, h, 0, h, h, s);
    reduce(n, bp, NT, HP, 0, h, PPO_ZONE_B3, 1, 0, h, 1, s);
    nt<NT_STORE>(I[PPO_T_W3], HP, n.CI, KC, HP, n.P, HP, bp, NT, s);                      // delta of the mean
    hipLaunchKernelGGL(k_ppo_spread, dim3((rp * (HP / 4) + 255) / 256), dim3(256), 0, s, n, n.Z, rp);
    tn(n.A2, HP, NT, n.A1, HP, HP, rp, n.partial, s);
    reduce(n, rp, NT, HP, 0, 0, PPO_ZONE_W2, h, 0, h, h, s);
    reduce(n, rp, NT, HP, 0, h, PPO_ZONE_B2, 1, 0, h, 1, s);
    nt<NT_MASK>(I[PPO_T_W2], HP, n.A2, HP, HP, n.A1, HP, rp, NT, s);                      // delta of zone_net_.0
    {
        const int chunks = (rp + kPpoChunk - 1) / kPpoChunk;
        hipLaunchKernelGGL((k_ppo_tn<true>), dim3(chunks, NT), dim3(64, (W1C + 31) / 32), 0, s, n.A1, HP, nullptr, 0, W1C,
                           rp, n.partial, g);
    }
    reduce(n, rp, NT, W1C, 0, 0, PPO_ZONE_W1, n.K1, 0, h, n.K1, s);
    reduce(n, rp, NT, W1C, 0, W1C - 1, PPO_ZONE_B1, 1, 0, h, 1, s);
    if (!a2c) launch_norm(n, stats + 5, s);
    return hipGetLastError();
}

hipError_t launch_ppo_minibatch(const PpoNet &n, const PpoExp &x, const int32_t *idx, int count, float *stats,
                                hipStream_t s)
{
    return minibatch(n, x, idx, count, stats, s, nullptr);
}

hipError_t launch_a2c_accumulate(const PpoNet &net, const PpoExp &x, const int32_t *idx, int count, int64_t total,
                                 int first, hipStream_t s)
{
    PpoNet n = net;
    n.accumulate = first ? 0 : 1;
    const A2cPass pass{ total, first };
    return minibatch(n, x, idx, count, nullptr, s, &pass);
}

hipError_t launch_a2c_apply(const PpoNet &n, float lr, float alpha, float one_minus_alpha, float eps, int64_t total,
                            float *stats, hipStream_t s)
{
    launch_norm(n, stats + 4, s);
    hipLaunchKernelGGL(k_a2c_finish, dim3(1), dim3(64), 0, s, n.run_sums, (double)total, stats);
    const int64_t quads = n.arena / 4;
    const unsigned blocks = (unsigned)std::min<int64_t>((quads + 255) / 256, 1024);
    hipLaunchKernelGGL(k_a2c_rmsprop, dim3(blocks), dim3(256), 0, s, n, lr, alpha, one_minus_alpha, eps);
    return hipGetLastError();
}

hipError_t launch_ppo_apply(const PpoNet &n, float step_size, float bc2_sqrt, hipStream_t s)
{
    launch_norm(n, nullptr, s);
    hipLaunchKernelGGL(k_ppo_adam, dim3((unsigned)((n.arena + 255) / 256)), dim3(256), 0, s, n, step_size, bc2_sqrt);
    return hipGetLastError();
}

hipError_t launch_inv_compact(const float *mask, int N, int T, int32_t *block_count, int32_t *list, int32_t *total,
                              hipStream_t s)
{
    const int64_t samples = (int64_t)N * (T - 1);
    const int blocks = (int)((samples + kInvBlock - 1) / kInvBlock);
    hipLaunchKernelGGL(k_inv_count, dim3(blocks), dim3(256), 0, s, mask, N, T - 1, samples, block_count);
    hipLaunchKernelGGL(k_inv_scan, dim3(1), dim3(kInvScan), 0, s, block_count, blocks, total);
    hipLaunchKernelGGL(k_inv_scatter, dim3(blocks), dim3(256), 0, s, mask, N, T - 1, samples, block_count, list);
    return hipGetLastError();
}

hipError_t launch_prior_hist(const int32_t *action, int64_t M, int S, int32_t *counts, int *bad, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(counts, 0, 32 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    const int blocks = (int)std::min<int64_t>((M + 255) / 256, 1024);
    hipLaunchKernelGGL(k_prior_hist, dim3(blocks), dim3(256), 0, s, action, M, S, counts, bad);
    return hipGetLastError();
}

}  // namespace zenvk
