// layout_sampler.hpp -- Engine.reset()'s random half, written ONCE for the host and for gfx950.
//
// numpy's RandomState(seed) (MT19937 seeding, twist, tempering, random_sample, uniform, the masked-rejection randint)
// and the Safety-Gym layout rejection sampler, as host_sampler.cpp has them (its sample_layout stays the yardstick,
// pinned to numpy by tests/golden/reset_vectors.npz); here every function is ZENV_HD and takes a *policy* that says
// where the generator's 624 words and the placed objects live and how many lanes work together:
//
//   HostLanes   one thread, plain arrays (zenv_sample_layout_shared; usable without a GPU)
//   WaveLanes   one wave64 per seed (layout_sample.hip): the words in LDS, object j in lane j's registers
//
// A policy P provides
//   P::kLanes, int lane()            cooperating lanes and this one's index (1 / 0 on the host)
//   void sync()                      every store of the group before it is visible to every load after it
//   bool any(bool)                   true on every lane iff the argument is true on one of them
//   uint32_t word(i), set_word(i,v)  the generator's state word i
//   double px(j), py(j)              centre of placed object j, asked for by lane j mod kLanes only
//   void place(j, x, y)              record object j (0 = the robot, 1.. = the zones)
//   void set_aux(z, v)               the task's aux column (ColourMatch: colour 0..2; TimedTSP: the deadline in steps)
// All arithmetic is integer or IEEE float64 add / mul / compare (the build has -ffp-contract=off): same bits on x86
// and on CDNA4.  The TimedTSP deadlines add det_log.hpp's det_log / det_div / det_sqrt, the same bits on both as well.  Every lane of a group follows the same control flow: draws, accept / reject decisions and restart
// counts are group-uniform by construction (decisions go through any()).
#pragma once
#include <cstdint>

#include "../../include/zenv.h"
#include "det_log.hpp"
#include "det_math.hpp"

namespace zenvk {

constexpr int kSamplerHostAttempts = 10000;                       // [not vendored] Engine.build_layout: 10000 tries
constexpr int kSamplerDeviceAttempts = ZENV_DEVICE_RESTARTS + 1;  // a device wave gives up after that many restarts
enum { SAMPLE_OK = 0, SAMPLE_UNFINISHED = 1, SAMPLE_SEED_RANGE = 2 };   // == ZENV_SAMPLE_*

// What the sampler reads of a zenv_config, with the keepout test's two thresholds (make_sampler_cfg, host only).
struct SamplerCfg {
    int32_t task, Z;
    int32_t n_zones_locations, n_robot_locations, robot_rot_fixed;
    int32_t num_steps;                                   // TimedTSP: a deadline is int(beta(beta_a, beta_b) * num_steps)
    double extent, robot_keepout, zones_keepout, robot_rot;
    double beta_a, beta_b;
    // sqrt(s) < A  <=>  s < T for the two right-hand sides A the placement loop ever has (see keepout_threshold):
    double t_robot_zone;   // A = (robot_keepout + placements_margin) + zones_keepout: a zone against the robot
    double t_zone_zone;    // A = (zones_keepout + placements_margin) + zones_keepout: a zone against a zone
    double robot_location[2];
    // [n_zones_locations][2], in the memory of whoever runs the sampler (the caller's zenv_config on the host, a device
    // copy for the kernel): indexed by the object, and a kernel argument indexed at run time is copied to scratch
    const double *zones_locations;
};

// ------------------------------------------------------------------ MT19937 / RandomState
template <class P>
struct RandomStateT {
    P &st;
    int idx;
    bool has_gauss;      // legacy_gauss draws two normals at a time and keeps the second
    double gauss_next;
    ZENV_HD explicit RandomStateT(P &s) : st(s), idx(624), has_gauss(false), gauss_next(0.0) {}

    // init_genrand: a serial chain; every lane runs it (the values are group-uniform), lane i mod kLanes keeps word i
    ZENV_HD void seed(uint32_t seed)
    {
        uint32_t s = seed;
        for (uint32_t i = 0; i < 624; ++i) {
            if (P::kLanes == 1 || (int)(i % P::kLanes) == st.lane()) st.set_word((int)i, s);
            s = 1812433253u * (s ^ (s >> 30)) + i + 1u;
        }
        st.sync();
        idx = 624;
        has_gauss = false;
        gauss_next = 0.0;
    }

    static ZENV_HD uint32_t mix(uint32_t hi, uint32_t lo)
    {
        const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
        return (y >> 1) ^ ((lo & 1u) ? 0x9908b0dfu : 0u);
    }

    // The serial twist, word i <- word[(i + 397) % 624] ^ mix(word[i], word[(i + 1) % 624]) for i = 0 .. 623 in order,
    // done kLanes words at a time.  Word i reads (a) itself and word i + 1 as they were BEFORE this twist -- except
    // i = 623, whose successor word 0 is already new -- and (b) word (i + 397) % 624, old for i < 227 and NEW (= word
    // i - 227) beyond.  A block [b, b + kLanes) loads everything, syncs, then stores: (a) holds because i + 1 is
    // stored by this block or a later one (word 0 by the first block, which is what i = 623 wants); (b) holds because
    // kLanes <= 227: word i - 227 was stored by an earlier block, word i + 397 belongs to a later one.  kLanes = 1 is
    // the textbook loop.
    ZENV_HD void twist()
    {
        static_assert(P::kLanes <= 227, "a block must not reach its own (i + 397) % 624 words");
        for (int base = 0; base < 624; base += P::kLanes) {
            const int i = base + st.lane();
            uint32_t v = 0;
            if (i < 624) {
                const int nx = i + 1 < 624 ? i + 1 : 0;
                const int far = i + 397 < 624 ? i + 397 : i - 227;
                v = st.word(far) ^ mix(st.word(i), st.word(nx));
            }
            st.sync();
            if (i < 624) st.set_word(i, v);
            st.sync();
        }
        idx = 0;
    }

    ZENV_HD uint32_t next_u32()
    {
        if (idx >= 624) twist();
        uint32_t y = st.word(idx++);
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }

    // random_sample: (a * 2^26 + b) / 2^53 with a 27-bit a and a 26-bit b.  The sum is an integer below 2^53 and the
    // division a power of two, so the product with 2^-53 is the same exact value.
    ZENV_HD double next_double()
    {
        const uint32_t hi = next_u32() >> 5;
        const uint32_t lo = next_u32() >> 6;
        return (static_cast<double>(hi) * 67108864.0 + static_cast<double>(lo)) * (1.0 / 9007199254740992.0);
    }

    ZENV_HD double uniform(double low, double high)
    {
        const double scale = high - low;
        return low + scale * next_double();
    }

    // legacy randint(0, n), n <= 2^32: masked rejection on 32-bit draws
    ZENV_HD uint32_t randint_below(uint32_t n)
    {
        const uint32_t top = n - 1u;
        if (top == 0) return 0;
        uint32_t mask = top;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        for (;;) {
            const uint32_t v = next_u32() & mask;
            if (v <= top) return v;
        }
    }

    // legacy_gauss, standard_gamma (shape > 1: Marsaglia-Tsang) and beta (a, b > 1) as LegacyRandomState has them in
    // host_sampler.cpp, expression for expression, with det_log / det_div / det_sqrt where that one calls libm.  Every
    // lane draws the same values: the loops are group-uniform.
    ZENV_HD double gauss()
    {
        if (has_gauss) {
            has_gauss = false;
            const double g = gauss_next;
            gauss_next = 0.0;
            return g;
        }
        double x1, x2, r2;
        do {
            x1 = 2.0 * next_double() - 1.0;
            x2 = 2.0 * next_double() - 1.0;
            r2 = x1 * x1 + x2 * x2;
        } while (r2 >= 1.0 || r2 == 0.0);
        const double f = det_sqrt(det_div(-2.0 * det_log(r2), r2));
        gauss_next = f * x1;
        has_gauss = true;
        return f * x2;
    }

    ZENV_HD double standard_gamma(double shape)
    {
        const double b = shape - det_div(1., 3.);
        const double c = det_div(1., det_sqrt(9 * b));
        for (;;) {
            double x, v;
            do {
                x = gauss();
                v = 1.0 + c * x;
            } while (v <= 0.0);
            v = v * v * v;
            const double u = next_double();
            if (u < 1.0 - 0.0331 * (x * x) * (x * x)) return b * v;
            // u == 0 has log(u) = -inf on the host: always below the finite right-hand side
            if (u == 0.0 || det_log(u) < 0.5 * x * x + b * (1. - v + det_log(v))) return b * v;
        }
    }

    ZENV_HD double beta(double a, double b)
    {
        const double ga = standard_gamma(a);
        const double gb = standard_gamma(b);
        return det_div(ga, ga + gb);
    }
};

// ------------------------------------------------------------------ the keepout test without a square root
// host_sampler.cpp rejects a candidate when  sqrt(s) < A,  s = ddx*ddx + ddy*ddy  (s >= 0, never NaN: the extents are
// finite).  IEEE sqrt is correctly rounded, hence monotone: s1 <= s2  =>  sqrt(s1) <= sqrt(s2).  Let T be the SMALLEST
// double with sqrt(T) >= A (it exists for 0 < A < sqrt(DBL_MAX): sqrt(A*A) is within an ulp of A and the walk below
// finds the boundary).  Then
//     s <  T  =>  sqrt(s) < A      (else s would be a smaller double with sqrt(s) >= A)
//     s >= T  =>  sqrt(s) >= sqrt(T) >= A      (monotone)
// so  sqrt(s) < A  <=>  s < T,  and the device compares s against T: no device sqrt in the decision.  A <= 0 never
// rejects (sqrt(s) >= 0), which s < 0 reproduces.  Host only (it calls the host's sqrt); sqrt_threshold() in
// host_sampler.cpp is the same idea for the visit radius' `<=`.
double keepout_threshold(double A);
SamplerCfg make_sampler_cfg(const zenv_config &cfg);

// One candidate against one placed object.
ZENV_HD bool keepout_hit(double x, double y, double px, double py, double T)
{
    const double ddx = x - px, ddy = y - py;
    return ddx * ddx + ddy * ddy < T;
}

// ------------------------------------------------------------------ the placement loop
// sample_layout of host_sampler.cpp.  With draw_deadlines (TimedTSP) the deadlines are drawn through det_log, which is
// within an ulp of any faithful libm's log: the same deadline as the host sampler's unless beta * num_steps lands within
// a few ulps of an integer.  Returns SAMPLE_OK with the objects in P (place()), the colours in P (set_aux()) and the rotation in `rot`, or
// SAMPLE_UNFINISHED after max_attempts failed attempts (restarts == max_attempts then).  The caller checks the seed's
// range (0 <= seed, seed + 1 <= 2^32 - 1) first.
template <class P>
ZENV_HD int sample_layout_shared(const SamplerCfg &c, bool draw_colours, bool draw_deadlines, uint32_t seed,
                                 int max_attempts, P &st, double &rot, int32_t &restarts)
{
    const int Z = c.Z;
    RandomStateT<P> rs(st);
    if (draw_colours) {      // c.task == ZENV_TASK_COLOUR_MATCH, a compile-time constant in the kernel
        // colour_match_env.py:57-68 draws from RandomState(seed), before Engine.reset bumps the seed
        rs.seed(seed);
        for (int z = 0; z < Z; ++z) st.set_aux(z, (int32_t)rs.randint_below(3));
        st.sync();          // the last loads of this generator before the next one's stores
    }
    if (draw_deadlines) {    // c.task == ZENV_TASK_TIMED_TSP, a compile-time constant in the kernel
        // TTSP_env.py:19-21 draws from RandomState(seed) as well; the cached second normal carries over between zones
        rs.seed(seed);
        for (int z = 0; z < Z; ++z) st.set_aux(z, (int32_t)(rs.beta(c.beta_a, c.beta_b) * c.num_steps));
        st.sync();
    }
    rs.seed(seed + 1u);
    restarts = 0;
    for (int attempt = 0; attempt < max_attempts; ++attempt) {
        bool failed = false;
        for (int obj = 0; obj <= Z && !failed; ++obj) {
            const double keepout = (obj == 0) ? c.robot_keepout : c.zones_keepout;
            // draw_placement: the extents shrunk by the keepout, or the 2e-9-wide box of a fixed location
            double xlo = -c.extent + keepout, xhi = c.extent - keepout, ylo = xlo, yhi = xhi;
            bool fixed = false;
            double fx = 0.0, fy = 0.0;
            if (obj == 0 && c.n_robot_locations > 0) {
                fixed = true;
                fx = c.robot_location[0]; fy = c.robot_location[1];
            }
            if (obj > 0 && obj - 1 < c.n_zones_locations) {
                fixed = true;
                fx = c.zones_locations[2 * (obj - 1)]; fy = c.zones_locations[2 * (obj - 1) + 1];
            }
            if (fixed) {
                const double k = keepout + 1e-9;
                xlo = (fx - k) + keepout; xhi = (fx + k) - keepout;
                ylo = (fy - k) + keepout; yhi = (fy + k) - keepout;
            }
            bool found = false;
            for (int t = 0; t < 100 && !found; ++t) {
                const double x = rs.uniform(xlo, xhi);
                const double y = rs.uniform(ylo, yhi);
                // objects 0 .. obj-1 are placed; object 0 is the robot, and only zones are tested against anything
                bool hit = false;
                for (int j0 = 0; j0 < obj && !hit; j0 += P::kLanes) {
                    const int j = j0 + st.lane();
                    const bool h = j < obj && keepout_hit(x, y, st.px(j), st.py(j), j == 0 ? c.t_robot_zone : c.t_zone_zone);
                    hit = st.any(h);
                }
                if (!hit) {
                    st.place(obj, x, y);
                    found = true;
                }
            }
            if (!found) failed = true;
        }
        if (!failed) {
            // build_world_config: robot_rot = random_rot() unless the config fixes it -- the last draw
            rot = c.robot_rot_fixed ? c.robot_rot : rs.uniform(0.0, 2 * 3.141592653589793);
            return SAMPLE_OK;
        }
        restarts++;
    }
    return SAMPLE_UNFINISHED;
}

// The host instantiation: one lane, plain arrays.
struct HostLanes {
    static constexpr int kLanes = 1;
    uint32_t mt[624];
    double x[ZENV_MAX_ZONES + 1], y[ZENV_MAX_ZONES + 1];
    int32_t aux[ZENV_MAX_ZONES];
    int lane() const { return 0; }
    void sync() {}
    bool any(bool b) const { return b; }
    uint32_t word(int i) const { return mt[i]; }
    void set_word(int i, uint32_t v) { mt[i] = v; }
    double px(int j) const { return x[j]; }
    double py(int j) const { return y[j]; }
    void place(int j, double xx, double yy) { x[j] = xx; y[j] = yy; }
    void set_aux(int z, int32_t v) { aux[z] = v; }
};

}  // namespace zenvk
