// render.hip -- K18: a top-down, orthographic rasteriser over the observation buffers (DESIGN.md 4 "K18"), gfx950.
//
// What the reference shows with ZoneEnvBase.render (ZoneEnvBase.py:243-336, MuJoCo's camera) is drawn here from what
// the agent observes: the zone rows (centre / 3, RGBA, the task's extra feature) and the robot's position and heading.
// Output: uint8 [count][H][W][3], RGB, row 0 at the top (+y).  All arithmetic is float32 in the order DESIGN.md gives
// (the build's -ffp-contract=off keeps every product and sum rounded on its own), so a frame is reproducible bit for
// bit by the same rules in numpy (tests/render_ref.py).
//
// Shape: the kernel is a byte stream with a few dozen flops per byte.  One workgroup draws up to 16 KiB of ONE image:
// its zone centres and colours are converted once into LDS, then every lane produces 16 consecutive bytes -- five and a
// third pixels -- and stores them with one global_store_dwordx4.  A wave's 1 KiB covers a few pixel rows, so lane z of
// the wave first tests zone z against those rows and the ballot is the (wave-uniform) list of zones the lanes walk;
// the mark and the robot are skipped by the whole wave in the same way.
// dst may have any alignment: per image, the bytes before the first and after the last 16-byte boundary are stored one
// by one by the image's first workgroup.
#include <hip/hip_runtime.h>

#include "render.hpp"

namespace zenvk {
namespace {

constexpr int kBlock = 256;
constexpr int kChunksPerBlock = 1024;      // 16-byte chunks per workgroup
constexpr int kMaxZones = 32;

constexpr uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | g << 8 | b << 16; }
constexpr uint32_t kBackground = rgb(224, 224, 224);
constexpr uint32_t kMark = rgb(255, 0, 255);
constexpr uint32_t kBody = rgb(32, 32, 32);
constexpr uint32_t kNose = rgb(255, 255, 255);

struct Scene {
    float zx[kMaxZones], zy[kMaxZones];    // NaN: the row is not drawn
    uint32_t zc[kMaxZones];
    float rx, ry, dir_x, dir_y, mx, my;    // robot; mark (NaN: none)
};

__device__ inline uint32_t to_byte(float c)
{
    c = fminf(fmaxf(c, 0.0f), 1.0f);       // (a NaN component becomes 0)
    return (uint32_t)(uint8_t)floorf(c * 255.0f + 0.5f);
}

// the constants every pixel test uses, from the two radii
struct Radii {
    float z2, ring2, r2, nose;
};
__device__ inline Radii radii(const RenderParams &rp)
{
    const float outer = 1.35f * rp.rz;
    return Radii{ rp.rz * rp.rz, outer * outer, rp.rr * rp.rr, 0.4f * rp.rr };
}

__device__ inline void pixel_centre(const RenderParams &rp, int r, int c, float &x, float &y)
{
    x = ((float)c + 0.5f) * rp.sx - rp.view;
    y = rp.view - ((float)r + 0.5f) * rp.sy;
}

// the mark's ring over whatever the zones left in col
__device__ inline uint32_t over_mark(const Scene &sc, const Radii &rd, float x, float y, uint32_t col)
{
    const float dx = x - sc.mx, dy = y - sc.my;
    const float d2 = dx * dx + dy * dy;
    return rd.z2 < d2 && d2 <= rd.ring2 ? kMark : col;
}

// the robot over everything else
__device__ inline uint32_t over_robot(const Scene &sc, const Radii &rd, float x, float y, uint32_t col)
{
    const float dx = x - sc.rx, dy = y - sc.ry;
    const float d2 = dx * dx + dy * dy;
    if (d2 <= rd.r2) col = dx * sc.dir_x + dy * sc.dir_y > rd.nose ? kNose : kBody;
    return col;
}

// can a disc of radius `reach` (slack included) around height cy touch a pixel row between y_bot and y_top?  False for a NaN
__device__ inline bool near_rows(float cy, float y_top, float y_bot, float reach)
{
    return cy - y_top <= reach && y_bot - cy <= reach;
}

// one pixel against every zone: the few bytes outside the 16-byte chunks
__device__ inline uint32_t shade_one(const Scene &sc, const Radii &rd, int Z, float x, float y)
{
    uint32_t col = kBackground;
    for (int z = 0; z < Z; ++z) {
        const float dx = x - sc.zx[z], dy = y - sc.zy[z];
        const float d2 = dx * dx + dy * dy;
        if (d2 <= rd.z2) col = sc.zc[z];
    }
    return over_robot(sc, rd, x, y, over_mark(sc, rd, x, y, col));
}

__global__ __launch_bounds__(kBlock) void k_render(RenderParams rp)
{
    __shared__ Scene sc;
    const int img = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int W = rp.W, Z = rp.Z;
    const int bytes = rp.H * W * 3;
    uint8_t *out = rp.dst + (int64_t)img * bytes;

    if (tid < Z) {
        const float *row = rp.zone_obs + (int64_t)img * rp.zone_stride + (int64_t)tid * rp.F;
        float cx = __builtin_nanf(""), cy = cx;
        uint32_t col = 0;
        if (row[5] != 0.0f) {               // alpha 0: WaitWrapper's all-zero observation
            cx = row[0];
            cy = row[1];
            float r = row[2], g = row[3], b = row[4];
            if (rp.timed && r == 0.0f && g == 1.0f && b == 1.0f) {      // unvisited: fades as its deadline nears
                const float t = row[6];
                r = 1.0f - t;
                g = b = fmaxf(0.0f, t);
            }
            col = rgb(to_byte(r), to_byte(g), to_byte(b));
        }
        sc.zx[tid] = cx;
        sc.zy[tid] = cy;
        sc.zc[tid] = col;
    } else if (tid == 64) {
        const float *o = rp.obs + (int64_t)img * rp.obs_stride;
        sc.rx = o[1];
        sc.ry = o[2];
        sc.dir_x = o[3];
        sc.dir_y = o[4];
    } else if (tid == 128) {
        const float nan = __builtin_nanf("");
        sc.mx = rp.marks ? rp.marks[2 * (int64_t)img] : nan;
        sc.my = rp.marks ? rp.marks[2 * (int64_t)img + 1] : nan;
    }
    __syncthreads();

    const Radii rd = radii(rp);
    const int head = min(bytes, (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u));
    const int n_chunks = (bytes - head) / 16;
    const int tail = bytes - head - 16 * n_chunks;

    if (blockIdx.y == 0) {                  // the unaligned ends, byte by byte (at most 15 each)
        int b = -1;
        if (tid < head) b = tid;
        else if (tid >= 32 && tid < 32 + tail) b = head + 16 * n_chunks + (tid - 32);
        if (b >= 0) {
            const int p = b / 3, r = p / W;
            float x, y;
            pixel_centre(rp, r, p - r * W, x, y);
            out[b] = (uint8_t)(shade_one(sc, rd, Z, x, y) >> (8 * (b - 3 * p)));
        }
    }

    const int lane = tid & 63;
    const int k_block = (int)blockIdx.y * kChunksPerBlock;
    for (int it = 0; it < kChunksPerBlock / kBlock; ++it) {
        const int k_wave = k_block + it * kBlock + (tid - lane);        // wave-uniform
        if (k_wave >= n_chunks) break;
        // the zones that can reach the pixel rows of this wave's chunks: |cy - y| <= rad for some row, with a pixel of slack
        const int k_last = min(k_wave + 63, n_chunks - 1);
        const int row_first = ((head + 16 * k_wave) / 3) / W, row_last = ((head + 16 * k_last + 15) / 3) / W;
        const float y_top = rp.view - ((float)row_first + 0.5f) * rp.sy, y_bot = rp.view - ((float)row_last + 0.5f) * rp.sy;
        // (a pixel inside a disc has |dy| <= rad but for float32 rounding: 1 % and a whole pixel pitch cover that)
        const float zy = sc.zy[lane & (kMaxZones - 1)];
        const unsigned long long zones_near = __ballot(lane < Z && near_rows(zy, y_top, y_bot, 1.01f * rp.rz + rp.sy));
        const bool mark_near = __builtin_amdgcn_readfirstlane(near_rows(sc.my, y_top, y_bot, 1.37f * rp.rz + rp.sy));
        const bool robot_near = __builtin_amdgcn_readfirstlane(near_rows(sc.ry, y_top, y_bot, 1.01f * rp.rr + rp.sy));

        const int k = k_wave + lane;
        if (k >= n_chunks) continue;
        const int s = head + 16 * k;        // the chunk's first byte: channel c0 of pixel p0
        const int p0 = s / 3, c0 = s - 3 * p0;
        int r = p0 / W, c = p0 - r * W;
        float x[6], y[6];
        uint32_t col[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {       // bytes s .. s + 15 lie in pixels p0 .. p0 + 5
            pixel_centre(rp, r, c, x[j], y[j]);
            col[j] = kBackground;
            if (++c == W) {
                c = 0;
                ++r;
            }
        }
        for (unsigned long long m = zones_near; m; m &= m - 1) {
            const int z = __builtin_ctzll(m);
            const float cx = sc.zx[z], cy = sc.zy[z];
            const uint32_t zc = sc.zc[z];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const float dx = x[j] - cx, dy = y[j] - cy;
                const float d2 = dx * dx + dy * dy;
                if (d2 <= rd.z2) col[j] = zc;
            }
        }
        if (mark_near) {
#pragma unroll
            for (int j = 0; j < 6; ++j) col[j] = over_mark(sc, rd, x[j], y[j], col[j]);
        }
        if (robot_near) {
#pragma unroll
            for (int j = 0; j < 6; ++j) col[j] = over_robot(sc, rd, x[j], y[j], col[j]);
        }
        // 18 bytes of pixels p0 .. p0 + 5, of which bytes c0 .. c0 + 15 are the chunk
        uint64_t w0 = (uint64_t)col[0] | (uint64_t)col[1] << 24 | (uint64_t)col[2] << 48;
        uint64_t w1 = (uint64_t)col[2] >> 16 | (uint64_t)col[3] << 8 | (uint64_t)col[4] << 32 | (uint64_t)col[5] << 56;
        const uint64_t w2 = (uint64_t)col[5] >> 8;
        if (c0) {
            const int sh = 8 * c0;
            w0 = w0 >> sh | w1 << (64 - sh);
            w1 = w1 >> sh | w2 << (64 - sh);
        }
        *reinterpret_cast<uint4 *>(out + s) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    }
}

}  // namespace

hipError_t launch_render(const RenderParams &rp, hipStream_t s)
{
    const int64_t chunks = (int64_t)rp.H * rp.W * 3 / 16;
    const unsigned segments = (unsigned)((chunks + kChunksPerBlock - 1) / kChunksPerBlock);
    hipLaunchKernelGGL(k_render, dim3((unsigned)rp.count, segments ? segments : 1u), dim3(kBlock), 0, s, rp);
    return hipGetLastError();
}

}  // namespace zenvk
