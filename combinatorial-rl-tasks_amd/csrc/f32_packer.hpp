// f32_packer.hpp -- the host packer of the float32 agents' weight images (zenv_hier_load, zenv_skill_load,
// zenv_option_load, zenv_skill_inverse_load): every tensor transposed and zero-padded as the kernels of hier_enc.hpp
// read it, at a 16-byte aligned offset in floats, none at offset 0 (0 = absent: the image starts with 4 zero floats).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

#include "hier_enc.hpp"

namespace zenvk {
namespace hf32 {

struct Packer {
    std::vector<float> &out;
    int h;
    explicit Packer(std::vector<float> &o, int h_) : out(o), h(h_) { out.assign(4, 0.f); }
    size_t put(size_t n)                                     // n zero floats, 16-byte aligned start
    {
        const size_t at = (out.size() + 3) & ~(size_t)3;
        out.resize(at + n, 0.f);
        return at;
    }
    // columns col0 .. col0 + n_cols - 1 of W [h][in_stride], transposed -> [rows][HP] (rows >= n_cols, zero-padded)
    size_t cols(const float *W, int in_stride, int col0, int n_cols, int rows)
    {
        const size_t at = put((size_t)rows * HP);
        for (int o = 0; o < h; ++o)
            for (int k = 0; k < n_cols; ++k) out[at + (size_t)k * HP + o] = W[(size_t)o * in_stride + col0 + k];
        return at;
    }
    size_t bias(const float *b)
    {
        const size_t at = put(HP);
        for (int o = 0; o < h; ++o) out[at + o] = b[o];
        return at;
    }
    // n output rows of W [n][h] + b [n] -> [n][HP + 1], bias last
    size_t rows(const float *W, const float *b, int n)
    {
        const size_t at = put((size_t)n * (HP + 1));
        fill_rows(at, W, b, n);
        return at;
    }
    // PolicyNetwork's heads as one block [2 n][HP + 1]: the n rows of mu_, then those of std_
    size_t head_rows(const float *mu_w, const float *mu_b, const float *std_w, const float *std_b, int n)
    {
        const size_t at = put(2 * (size_t)n * (HP + 1));
        fill_rows(at, mu_w, mu_b, n);
        fill_rows(at + (size_t)n * (HP + 1), std_w, std_b, n);
        return at;
    }
    // One encoder, the ten pointers of HierEnc into offs[i ...]: zone_net_.0 on [x, (onehot,) zone row] and
    // combine_net_ on [x, (onehot,) zone_emb], split by input columns.  xin: the width of the per-env input x (8: obs,
    // 10: [obs, goal]); xs: the one-hot columns after it, skipped here (the skill family packs them on their own)
    void enc(size_t *offs, int &i, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
             const float *b3, const float *wc, const float *bc, int F, int xin, int xs)
    {
        offs[i++] = cols(w1, xin + xs + F, 0, xin, xin);
        offs[i++] = cols(w1, xin + xs + F, xin + xs, F, ZF);
        offs[i++] = bias(b1);
        offs[i++] = cols(w2, h, 0, h, HP);
        offs[i++] = bias(b2);
        offs[i++] = cols(w3, h, 0, h, HP);
        offs[i++] = bias(b3);
        offs[i++] = cols(wc, xin + xs + h, 0, xin, xin);
        offs[i++] = cols(wc, xin + xs + h, xin + xs, h, HP);
        offs[i++] = bias(bc);
    }

private:
    void fill_rows(size_t at, const float *W, const float *b, int n)
    {
        for (int r = 0; r < n; ++r) {
            for (int k = 0; k < h; ++k) out[at + (size_t)r * (HP + 1) + k] = W[(size_t)r * h + k];
            out[at + (size_t)r * (HP + 1) + HP] = b[r];
        }
    }
};

// Bind a packed image to its device address: the n pointers of a weight struct from `first` on, in declaration order
// (the struct's static_assert: nothing else sits between them); offset 0 = absent = null
template <typename Net>
void bind_pointers(Net &net, size_t first, const float *base, const size_t *offs, int n)
{
    for (int i = 0; i < n; ++i) {
        const float *p = offs[i] ? base + offs[i] : nullptr;
        std::memcpy(reinterpret_cast<char *>(&net) + first + (size_t)i * sizeof p, &p, sizeof p);
    }
}

}  // namespace hf32
}  // namespace zenvk
