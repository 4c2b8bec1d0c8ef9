// bh_query_host.hpp -- the host arithmetic of the analysis queries (moment maps, radial profiles and Lagrangian radii, modes,
// rotation curve, field at points, neighbours, pair counts, groups): the fixed-point exponent rule, the squared bin edges and how
// a fault of theirs is worded, the query points' check, the decisions of the Lagrangian select, the catalogue's order and the
// layout of a device block.  Standard C++ only -- nothing of HIP, nothing of the context -- so tests/query_host_replay.cpp runs
// it with the host compiler; bh_queries_host.hpp is its one user in the library.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

namespace bh {

// ---- fixed-point planes: a plane of maximum m < 2^E summed over n <= 2^L bodies stays in int64 scaled by 2^e, e = 62 - E - L
// ceil(log2(max(n, 1)))
inline int log2_ceil(int64_t n) { int L = 0; while (((int64_t)1 << L) < n) ++L; return L; }

// E of a maximum: m < 2^E (0 for m == 0)
inline int binary_exponent(double m) { int E = 0; if (m != 0.0) (void)std::frexp(m, &E); return E; }

// the exponent of one plane from its maximum; 0 where the maximum is 0
inline int32_t plane_exponent(double maxabs, int L) { return maxabs == 0.0 ? 0 : 62 - binary_exponent(maxabs) - L; }

// whether a caller's exponent e covers the maximum (any does where the maximum is 0); *at_most: the largest that does
inline bool exponent_fits(int32_t e, double maxabs, int L, int32_t *at_most)
{
    *at_most = 62 - binary_exponent(maxabs) - L;
    return maxabs == 0.0 || e <= *at_most;
}

// ---- squared bin edges.  e2[k] = edges[k]^2 for k = 0 .. nb; 0, or what is wrong with the first edge that is not in order
// (every condition that holds there: each caller words and ranks them its own way)
enum : unsigned {
    kEdgesCount = 1,                // nb outside 1 .. max_bins (nothing else is looked at)
    kEdgeNotFinite = 2, kEdgeSquareNotFinite = 4, kEdgeNegative = 8,
    kEdgeNotAscending = 16, kEdgeSquareNotAscending = 32        // against the edge before
};

inline unsigned squared_edges(const double *edges, int32_t nb, int32_t max_bins, std::vector<double> &e2)
{
    if (nb < 1 || nb > max_bins) return kEdgesCount;
    e2.resize((size_t)nb + 1);
    for (int32_t k = 0; k <= nb; ++k) {
        const double e = edges[k], s = e2[(size_t)k] = e * e;
        unsigned why = 0;
        if (!std::isfinite(e)) why |= kEdgeNotFinite;
        if (!std::isfinite(s)) why |= kEdgeSquareNotFinite;
        if (e < 0.0) why |= kEdgeNegative;
        if (k > 0 && !(edges[k - 1] < e)) why |= kEdgeNotAscending;
        if (k > 0 && !(e2[(size_t)k - 1] < s)) why |= kEdgeSquareNotAscending;
        if (why) return why;
    }
    return 0;
}

// how the radial profiles, the azimuthal modes and the rotation curve word a reason: null for 0, else the one text, the count
// before not finite before negative before not ascending.  The count's text is kEdgesCountFault, which ends where the caller
// names its own limit: "BH_..._MAX_BINS = <value>".  (The pair counts word theirs differently.)
constexpr const char *kEdgesCountFault = "nb must be 1 .. ";

inline const char *edges_fault(unsigned why)
{
    if (!why) return nullptr;
    if (why & kEdgesCount) return kEdgesCountFault;
    if (why & (kEdgeNotFinite | kEdgeSquareNotFinite)) return "an edge or its square is not finite";
    if (why & kEdgeNegative) return "the edges must be >= 0";
    return "the edges and their squares must be strictly ascending";
}

// ---- azimuthal modes (bh_modes.hpp): P planes of nb + 2 slots in the 64 KiB of dynamic LDS a launch may ask for without opting
// in.  The whole histogram and the nb + 1 squared edges when they fit (tile 0: private); else a tile of floor(65,536 / (8 P))
// slots for the range a workgroup's bodies touch.  bytes: the dynamic LDS of the launch.
constexpr int kModesLdsBytes = 65536;

inline int modes_planes(int M, bool rates) { return (rates ? 2 : 1) * (1 + 2 * M) + 1; }

struct ModesPlan { int tile; size_t bytes; };

inline ModesPlan modes_plan(int P, int nb)
{
    const size_t whole = 8 * (size_t)P * ((size_t)nb + 2) + 8 * ((size_t)nb + 1);
    if (whole <= (size_t)kModesLdsBytes) return ModesPlan{0, whole};
    const int tile = kModesLdsBytes / (8 * P);
    return ModesPlan{tile, 8 * (size_t)P * (size_t)tile};
}

// ---- query points {x, y}: the first with a coordinate that is not finite, or -1 (no points: -1)
inline int64_t first_nonfinite_point(const double *points, int64_t n_points)
{
    for (int64_t i = 0; points && i < 2 * n_points; ++i)
        if (!std::isfinite(points[i])) return i / 2;
    return -1;
}

// ---- the radix select of the Lagrangian radii, eight bits of the squared radius's pattern a round (engine.py's
// LagrangianSelect is the same in Python integers): prefixes() are the distinct digit strings the next round counts below,
// advance() takes every fraction's next digit from that round's histograms {sum w, count}[np][256], result() after the last
struct LagrangianSelect {
    static constexpr int kDigitBits = 8, kDigits = 1 << kDigitBits, kRounds = 64 / kDigitBits, kMaxFractions = 32;

    int32_t nf = 0, round = 0, np = 0;
    int64_t total = -1;                                           // round 0's sum of weights (0: no mass, done at once)
    double fraction[kMaxFractions] = {};
    uint64_t prefix[kMaxFractions] = {}, distinct[kMaxFractions] = {};       // the digits decided so far, per fraction
    int32_t which[kMaxFractions] = {};                            // fraction -> its row of the round's histograms
    int64_t below_w[kMaxFractions] = {}, below_n[kMaxFractions] = {}, last_w[kMaxFractions] = {}, last_n[kMaxFractions] = {};
    int64_t target[kMaxFractions] = {};

    LagrangianSelect(const double *fractions, int32_t n) : nf(n) { std::copy(fractions, fractions + n, fraction); }

    bool done() const { return round >= kRounds || total == 0; }

    // the distinct prefixes in the order of their first appearance; returns how many
    int32_t prefixes(const uint64_t **out)
    {
        np = 0;
        for (int32_t f = 0; f < nf; ++f) {
            int32_t k = 0;
            while (k < np && distinct[k] != prefix[f]) ++k;
            if (k == np) distinct[np++] = prefix[f];
            which[f] = k;
        }
        *out = distinct;
        return np;
    }

    void advance(const int64_t *hist)
    {
        if (round == 0) {
            int64_t W = 0;
            for (int d = 0; d < kDigits; ++d) W += hist[(size_t)d * 2];
            total = W;
            if (W == 0) return;
            for (int32_t f = 0; f < nf; ++f)
                target[f] = std::min<int64_t>(W, std::max<int64_t>(1, (int64_t)std::ceil(fraction[f] * (double)W)));
        }
        for (int32_t f = 0; f < nf; ++f) {
            const int64_t *h = hist + (size_t)which[f] * kDigits * 2;
            int d = 0;
            while (d < kDigits - 1 && below_w[f] + h[2 * d] < target[f]) { below_w[f] += h[2 * d]; below_n[f] += h[2 * d + 1]; ++d; }
            prefix[f] = (prefix[f] << kDigitBits) | (uint64_t)d;
            last_w[f] = h[2 * d]; last_n[f] = h[2 * d + 1];
        }
        ++round;
    }

    // per fraction: the squared radius, the bodies and the weight at or inside it; NaN, 0, 0 for a system without mass
    void result(double *r2, int64_t *count, int64_t *mass) const
    {
        for (int32_t f = 0; f < nf; ++f) {
            if (total == 0) { r2[f] = std::nan(""); count[f] = 0; mass[f] = 0; continue; }
            std::memcpy(&r2[f], &prefix[f], sizeof(double));
            count[f] = below_n[f] + last_n[f];
            mass[f] = below_w[f] + last_w[f];
        }
    }
};

// a caller's prefixes for one round: null, or the first rule they break
inline const char *select_prefix_fault(int32_t round, const uint64_t *prefixes, int32_t np)
{
    if (round < 0 || round >= LagrangianSelect::kRounds) return "round must be 0 .. 7";
    if (!prefixes) return "null prefixes";
    if (np < 1 || np > LagrangianSelect::kMaxFractions) return "np must be 1 .. BH_RADIAL_MAX_FRACTIONS";
    if (round == 0 && (np != 1 || prefixes[0] != 0)) return "round 0 has the one prefix 0";
    for (int32_t a = 0; a < np; ++a) {
        if (round > 0 && (prefixes[a] >> (LagrangianSelect::kDigitBits * round)) != 0) return "a prefix has more digits than the round";
        for (int32_t b = 0; b < a; ++b)
            if (prefixes[a] == prefixes[b]) return "the prefixes must be distinct";
    }
    return nullptr;
}

// ---- the group catalogue: the device numbers its records as its atomics fall; the caller gets them by count descending, then
// label ascending (labels are distinct), with `planes` sums a record
inline void catalogue_order(const uint32_t *rec_label, const uint32_t *rec_count, const int64_t *rec_sums, int64_t kept, int planes,
                            std::vector<int64_t> &labels, std::vector<int64_t> &counts, std::vector<int64_t> &sums)
{
    std::vector<int64_t> order((size_t)kept);
    for (int64_t g = 0; g < kept; ++g) order[(size_t)g] = g;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return rec_count[a] != rec_count[b] ? rec_count[a] > rec_count[b] : rec_label[a] < rec_label[b];
    });
    labels.resize((size_t)kept); counts.resize((size_t)kept); sums.resize((size_t)kept * planes);
    for (int64_t k = 0; k < kept; ++k) {
        const int64_t g = order[(size_t)k];
        labels[(size_t)k] = (int64_t)rec_label[g];
        counts[(size_t)k] = (int64_t)rec_count[g];
        std::copy(rec_sums + g * planes, rec_sums + (g + 1) * planes, sums.begin() + k * planes);
    }
}

// ---- one device block for many arrays: the parts in order, each at a multiple of 16 bytes
struct BlockPart {
    void *slot;                     // where the part's address goes: a T *
    size_t count, size;             // elements and sizeof(T)
};

template <typename T>
BlockPart part(T **slot, size_t count) { return BlockPart{slot, count, sizeof(T)}; }

// the bytes of the parts; with a base (16-byte aligned) every slot gets its address as well
inline size_t lay_out(std::initializer_list<BlockPart> parts, char *base = nullptr)
{
    size_t at = 0;
    for (const BlockPart &p : parts) {
        if (base) { char *a = base + at; std::memcpy(p.slot, &a, sizeof(a)); }
        at += (p.count * p.size + 15) / 16 * 16;
    }
    return at;
}

// the capacity that holds `want`: the power-of-two multiple of `from` (so regrowing stays rare)
inline int64_t grown_capacity(int64_t want, int64_t from = 1024) { int64_t cap = from; while (cap < want) cap <<= 1; return cap; }

}  // namespace bh
