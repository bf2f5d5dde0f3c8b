// route_solver.hpp -- the solver-ordered handles' built-in tour, written ONCE for the host and for gfx950.
//
// route_ranks of host_sampler.cpp (it stays the yardstick, as sample_layout is for layout_sampler.hpp), restated over a
// *lanes policy* the way the shared sampler is: the problem TSP_Solver.get_optim_route (main/src/utils/TSP_Solver.py:
// 24-62) hands to OR-tools for TSPOrderEnv.generate_route (main/envs/TSP_order_env.py:49-50) -- a closed tour over
// node 0 = the robot and nodes 1..Z = the zones, arc cost int64(10 x distance), first solution PATH_CHEAPEST_ARC, then
// first-improvement local search (or-opt of chains 1..3, exchange, 2-opt) to a local optimum.
//
//   HostRouteLanes   one thread, plain arrays (zenv_route_ranks_shared; usable without a GPU)
//   WaveRouteLanes   one wave64 per layout (layout_sample.hip, K21): matrix, coordinates and tour in LDS
//
// A policy R provides
//   R::kLanes, int lane()              cooperating lanes and this one's index (1 / 0 on the host)
//   void sync()                        every store of the group before it is visible to every load after it
//   uint64_t ballot(bool)              bit l = lane l's argument, the same word on every lane
//   double x(a), y(a)                  centre of node a (any lane may ask for any node)
//   int64_t d(a, b), set_d(a, b, v)    the cost matrix
//   int tour(i), set_tour(i, v)        the node at tour position i, 0 <= i < n
//   void stage(k, v, live), commit(n)  a permutation in two halves: remember position k's new node (live: k < n),
//                                      then store what was remembered (kLanes >= n, or room for n staged values)
//   void set_rank(z, v)                the result: position of zone z in the tour
//
// Why a scan in parallel takes the host's move: the host walks the candidates of an operator in a fixed order and
// takes the FIRST that improves.  A group evaluates the next kLanes candidates of that order at once -- evaluating
// changes nothing -- and the lowest set bit of the ballot is the first improving one of them; blocks before it had
// none.  Every lane derives the move from the winning index, so the control flow is group-uniform throughout.
//
// Bits: the costs are IEEE float64 subtract / multiply / add (the build has -ffp-contract=off), det_sqrt (correctly
// rounded on x86 and gfx950), one more multiply and a truncation -- defined for |coordinate| <= 1e9 (cost < 2.9e10),
// which the callers check.  Everything after the matrix is int64 addition and comparison.
//
// Termination: every accepted move lowers the tour's int64 length by at least 1 and the length is bounded below by 0,
// so the search ends without an iteration cap (the maximum seen over the tests' layouts is 39 moves at 32 zones).
#pragma once
#include <cstdint>

#include "../../include/zenv.h"
#include "det_log.hpp"
#include "det_math.hpp"

namespace zenvk {

constexpr int kRouteMaxNodes = ZENV_MAX_ZONES + 1;
enum { ROUTE_OROPT1 = 0, ROUTE_OROPT2 = 1, ROUTE_OROPT3 = 2, ROUTE_EXCHANGE = 3, ROUTE_TWO_OPT = 4, ROUTE_N_OPS = 5 };

// Row stride of the int64 matrix, in elements: odd, so that a column -- lanes with the same b and consecutive a -- falls
// on 32 different banks (8-byte reads: bank (2 (a stride + b)) mod 64 = 2 (a + b) mod 64 for stride = 1 mod 32; any odd
// stride gives 32 distinct even banks over 32 consecutive a).  Rows are contiguous anyway.
ZENV_HD int route_stride(int n) { return n | 1; }

// the lowest set bit's index (w != 0)
ZENV_HD int route_first_bit(uint64_t w) { return __builtin_ctzll(w); }

template <class R>
ZENV_HD int route_at(const R &rt, int i, int n) { return rt.tour(i < n ? i : i - n); }    // closed: position n is the depot

// One scan step's verdict: the group-wide index of the first improving candidate of [c0, c0 + kLanes), or -1.
template <class R>
ZENV_HD int route_pick(R &rt, int c0, bool improves)
{
    const uint64_t w = rt.ballot(improves);
    return w ? c0 + route_first_bit(w) : -1;
}

// The lanes rewrite the tour together: position k takes the node at old position src(k).  Every new value is staged
// (loaded) before any is committed (stored): a wave keeps position lane's in a register, the host in a second array.
template <class R, class F>
ZENV_HD void route_permute(R &rt, int n, F src)
{
    for (int k0 = 0; k0 < n; k0 += R::kLanes) {
        const int k = k0 + rt.lane();
        rt.stage(k, k < n ? rt.tour(src(k)) : 0, k < n);
    }
    rt.sync();
    rt.commit(n);
    rt.sync();
}

// rank[Z] <- the tour of (robot, zones) held by the policy (x / y of nodes 0 .. Z); moves[ROUTE_N_OPS] <- accepted
// moves per operator.  1 <= Z <= ZENV_MAX_ZONES.
template <class R>
ZENV_HD void route_solve_shared(int Z, R &rt, int32_t *moves)
{
    const int n = Z + 1;
    for (int k = 0; k < ROUTE_N_OPS; ++k) moves[k] = 0;
    // the int64 cost matrix, kLanes entries at a time
    for (int e0 = 0; e0 < n * n; e0 += R::kLanes) {
        const int e = e0 + rt.lane();
        if (e < n * n) {
            const int a = e / n, b = e - a * n;
            const double dx = rt.x(a) - rt.x(b), dy = rt.y(a) - rt.y(b);
            rt.set_d(a, b, (int64_t)(det_sqrt(dx * dx + dy * dy) * 10.0));
        }
    }
    rt.sync();
    // PATH_CHEAPEST_ARC: extend the path from the depot by the cheapest arc to a free node, lowest index on ties.  A
    // serial chain of n - 1 choices; every lane walks it (the reads are broadcasts, the values group-uniform) and lane
    // step mod kLanes keeps the choice.
    {
        uint64_t used = 1ull;
        int last = 0;
        if (rt.lane() == 0) rt.set_tour(0, 0);
        for (int step = 1; step < n; ++step) {
            int best = -1;
            int64_t best_d = 0;
            for (int c = 1; c < n; ++c) {
                if ((used >> c) & 1ull) continue;
                const int64_t dc = rt.d(last, c);
                if (best < 0 || dc < best_d) { best = c; best_d = dc; }
            }
            used |= 1ull << best;
            if (R::kLanes == 1 || step % R::kLanes == rt.lane()) rt.set_tour(step, best);
            last = best;
        }
        rt.sync();
    }
    bool improved = n > 3;
    while (improved) {
        improved = false;
        // or-opt / relocate: the chain tour[i .. i + len - 1] moves between tour[j] and tour[j + 1], orientation kept.
        // Candidate c of a chain length is (i, j) = (1 + c / n, c mod n): the host's i-major, j-minor order.
        for (int len = 1; len <= 3 && !improved; ++len) {
            const int count = (n - len) * n;                 // i = 1 .. n - len
            for (int c0 = 0; c0 < count && !improved; c0 += R::kLanes) {
                const int c = c0 + rt.lane();
                bool better = false;
                if (c < count) {
                    const int i = 1 + c / n, j = c - (i - 1) * n;
                    if (!(j >= i - 1 && j < i + len)) {      // not the chain itself or its own predecessor
                        const int p = rt.tour(i - 1), f = rt.tour(i), l = rt.tour(i + len - 1), q = route_at(rt, i + len, n);
                        const int a = rt.tour(j), b = route_at(rt, j + 1, n);
                        const int64_t gain = rt.d(p, f) + rt.d(l, q) + rt.d(a, b) - rt.d(p, q) - rt.d(a, f) - rt.d(l, b);
                        better = gain > 0;
                    }
                }
                const int win = route_pick(rt, c0, better);
                if (win >= 0) {
                    const int i = 1 + win / n, j = win - (i - 1) * n;
                    // the rest with the chain put in behind tour[j]
                    if (j < i)                               // j <= i - 2: [0..j] chain [j+1..i-1] [i+len..]
                        route_permute(rt, n, [=](int k) { return k <= j ? k : k <= j + len ? i + (k - j - 1) : k < i + len ? k - len : k; });
                    else                                     // j >= i + len: [0..i-1] [i+len..j] chain [j+1..]
                        route_permute(rt, n, [=](int k) { return k < i ? k : k <= j - len ? k + len : k <= j ? i + (k - (j - len + 1)) : k; });
                    moves[ROUTE_OROPT1 + len - 1]++;
                    improved = true;
                }
            }
        }
        // exchange: the zones at positions i < j swap places.  The host compares the whole tour's length before and
        // after; only the arcs at the two positions change and every cost is an integer, so the exact difference of
        // those arcs decides alike -- three arcs when the positions are neighbours, four otherwise.  Candidates run
        // over the square (i, j) in [1, n)^2, the pairs with j <= i idle: i-major, j-minor like the host's loops.
        const int m = n - 1;
        for (int c0 = 0; c0 < m * m && !improved; c0 += R::kLanes) {
            const int c = c0 + rt.lane();
            bool better = false;
            if (c < m * m) {
                const int i = 1 + c / m, j = 1 + (c - (i - 1) * m);
                if (j > i) {
                    const int p = rt.tour(i - 1), u = rt.tour(i), v = rt.tour(j), q = route_at(rt, j + 1, n);
                    int64_t before, after;
                    if (j == i + 1) {
                        before = rt.d(p, u) + rt.d(u, v) + rt.d(v, q);
                        after = rt.d(p, v) + rt.d(v, u) + rt.d(u, q);
                    } else {
                        const int un = rt.tour(i + 1), vp = rt.tour(j - 1);
                        before = rt.d(p, u) + rt.d(u, un) + rt.d(vp, v) + rt.d(v, q);
                        after = rt.d(p, v) + rt.d(v, un) + rt.d(vp, u) + rt.d(u, q);
                    }
                    better = after < before;
                }
            }
            const int win = route_pick(rt, c0, better);
            if (win >= 0) {
                const int i = 1 + win / m, j = 1 + (win - (i - 1) * m);
                route_permute(rt, n, [=](int k) { return k == i ? j : k == j ? i : k; });
                moves[ROUTE_EXCHANGE]++;
                improved = true;
            }
        }
        // 2-opt: reverse tour[i .. j], 1 <= i < j < n (the host's i stops at n - 2: row n - 1 of the square has no j > i)
        for (int c0 = 0; c0 < m * m && !improved; c0 += R::kLanes) {
            const int c = c0 + rt.lane();
            bool better = false;
            if (c < m * m) {
                const int i = 1 + c / m, j = 1 + (c - (i - 1) * m);
                if (j > i) {
                    const int a = rt.tour(i - 1), b = rt.tour(i), cc = rt.tour(j), e = route_at(rt, j + 1, n);
                    better = rt.d(a, cc) + rt.d(b, e) < rt.d(a, b) + rt.d(cc, e);
                }
            }
            const int win = route_pick(rt, c0, better);
            if (win >= 0) {
                const int i = 1 + win / m, j = 1 + (win - (i - 1) * m);
                route_permute(rt, n, [=](int k) { return k >= i && k <= j ? i + j - k : k; });
                moves[ROUTE_TWO_OPT]++;
                improved = true;
            }
        }
    }
    for (int k0 = 1; k0 < n; k0 += R::kLanes) {
        const int k = k0 + rt.lane();
        if (k < n) rt.set_rank(rt.tour(k) - 1, k - 1);
    }
}

// The host instantiation: one lane, plain arrays.  A permutation is staged into `next` and committed by a copy.
struct HostRouteLanes {
    static constexpr int kLanes = 1;
    double xs[kRouteMaxNodes], ys[kRouteMaxNodes];
    int64_t cost[kRouteMaxNodes * kRouteMaxNodes];
    int32_t tr[kRouteMaxNodes], next[kRouteMaxNodes];
    int32_t *rank;
    int n;
    int lane() const { return 0; }
    void sync() {}
    uint64_t ballot(bool b) const { return b ? 1ull : 0ull; }
    double x(int a) const { return xs[a]; }
    double y(int a) const { return ys[a]; }
    int64_t d(int a, int b) const { return cost[a * n + b]; }
    void set_d(int a, int b, int64_t v) { cost[a * n + b] = v; }
    int tour(int i) const { return tr[i]; }
    void set_tour(int i, int v) { tr[i] = v; }
    void stage(int k, int v, bool live) { if (live) next[k] = v; }
    void commit(int nn) { for (int k = 0; k < nn; ++k) tr[k] = next[k]; }
    void set_rank(int z, int v) { rank[z] = v; }
};

// |coordinate| <= 1e9 and finite: inside that box the cast of 10 x distance to int64 is defined
ZENV_HD bool route_coord_ok(double v) { return v >= -1e9 && v <= 1e9; }

}  // namespace zenvk
