// bh_queries_host.hpp -- the host side of the analysis queries: moment maps, radial profiles and Lagrangian radii, azimuthal modes,
// the rotation curve, the field at points, neighbour queries and lists, pair counts, friends-of-friends groups, spanning trees and
// bound pairs, with their entry points of include/bhgpu.h.  Part of the bh_engine.hip translation unit: included there once, after
// the context and the engine's helpers (fail, BH_HIP, dev_alloc, with_state, dispatch, quietly, split_check, need_forces,
// enqueue_lsd_passes ...).  The kernels are in bh_moments.hpp, bh_radial.hpp, bh_modes.hpp, bh_disc.hpp (with bh_binned.hpp under
// all four), bh_field.hpp, bh_neighbours.hpp, bh_neighbour_lists.hpp, bh_pairs.hpp, bh_groups.hpp, bh_mst.hpp and bh_binaries.hpp,
// the state in bh_queries_state.hpp, the arithmetic that needs no device in bh_query_host.hpp.  What every family shares comes
// first, with the two passes of the binned sums: first_pass, plane_exponents, radial_edges, deposit_pass.
#pragma once

#include "bh_query_host.hpp"

static_assert(LagrangianSelect::kDigitBits == kRadDigitBits && LagrangianSelect::kMaxFractions == kRadMaxFractions,
              "the host's select and the select kernel cut the same digits");

namespace {

template <typename P>
using Pointee = std::remove_cv_t<std::remove_pointer_t<P>>;

// f(pos, vel, mass) with the state arrays as they are typed: const double2 * / double *, or const float2 * / float *
template <typename F>
void state_ptrs(const bh_ctx *c, F &&f)
{
    with_state(c, [&](auto r2) {
        using Real2 = decltype(r2);
        using Real = decltype(r2.x);
        f(static_cast<const Real2 *>(c->pos), static_cast<const Real2 *>(c->vel), static_cast<const Real *>(c->mass));
    });
}

// A timed span is two marks on the stream and, once the caller has waited for the stream, span_ms between them.
int mark(bh_ctx *c, hipEvent_t &e)
{
    if (!e) BH_HIP(c, hipEventCreate(&e));
    BH_HIP(c, hipEventRecord(e, c->stream));
    return BH_OK;
}

int span_ms(bh_ctx *c, hipEvent_t from, hipEvent_t to, double *ms, bool add = false)
{
    float f = 0.f;
    BH_HIP(c, hipEventElapsedTime(&f, from, to));
    *ms = (add ? *ms : 0.0) + (double)f;
    return BH_OK;
}

// every array of a small set or none of them: after a failure all the pointers are null again, so the next call starts over
int alloc_all(bh_ctx *c, std::initializer_list<BlockPart> parts)
{
    std::vector<char *> got(parts.size(), nullptr);
    int rc = BH_OK;
    size_t k = 0;
    for (const BlockPart &p : parts)
        if (!rc) rc = dev_alloc(c, &got[k++], p.count * p.size);
    if (rc)
        for (char *&a : got) { dev_free(c, a); a = nullptr; }
    k = 0;
    for (const BlockPart &p : parts) std::memcpy(p.slot, &got[k++], sizeof(char *));
    return rc;
}

// a block of `parts` for `cap` items in place of the one b holds (the previous call has waited for its stream); the parts'
// pointers are set.  The caller decides when: b.cap is too small.  After a failure b is empty and the next call starts over.
int block_regrow(bh_ctx *c, DevBlock &b, int64_t cap, std::initializer_list<BlockPart> parts)
{
    if (b.base) { dev_free(c, b.base); c->device_bytes -= b.bytes; b = DevBlock{}; }
    const size_t bytes = lay_out(parts);
    char *base = nullptr;
    if (int rc = dev_alloc(c, &base, bytes)) return rc;
    b.base = base; b.bytes = bytes; b.cap = cap;
    lay_out(parts, base);
    return BH_OK;
}

// a first pass's record {bits[P], flag words} on the host when this returns, with its maxima as doubles; the flags are the
// caller's to test.  also: one more download that rides on the same wait.
template <typename Rec, int P>
int read_maxima(bh_ctx *c, const Rec *dev, Rec *rec, double (&maxabs)[P], void *also = nullptr, const void *also_dev = nullptr,
                size_t also_bytes = 0)
{
    BH_HIP(c, hipMemcpyAsync(rec, dev, sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
    if (also) BH_HIP(c, hipMemcpyAsync(also, also_dev, also_bytes, hipMemcpyDeviceToHost, c->stream));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    for (int p = 0; p < P; ++p) std::memcpy(&maxabs[p], &rec->bits[p], sizeof(double));
    return BH_OK;
}

// A first pass of the binned sums (bh_binned.hpp): the record zeroed, `launch` enqueued, then as read_maxima; the record's flags
// are the caller's to test and to word.  ev: the two marks around the pass, *ms the span between them (null: not timed).
template <typename Rec, int P, typename Launch>
int first_pass(bh_ctx *c, Rec *dev, Rec *rec, double (&maxabs)[P], Launch &&launch, hipEvent_t *ev = nullptr, double *ms = nullptr)
{
    if (ev) { if (int rc = mark(c, ev[0])) return rc; }
    BH_HIP(c, hipMemsetAsync(dev, 0, sizeof(Rec), c->stream));
    launch();
    BH_HIP(c, hipGetLastError());
    if (ev) { if (int rc = mark(c, ev[1])) return rc; }
    if (int rc = read_maxima(c, dev, rec, maxabs)) return rc;
    return ev ? span_ms(c, ev[0], ev[1], ms) : BH_OK;
}

// e: the caller's exponents `given` or, without, the rule's own from this context's maxima and body count.  A caller's must cover
// those -- else a contribution or a sum could leave int64.
template <int P>
int plane_exponents(bh_ctx *c, const char *who, const int32_t *given, const double (&maxabs)[P], int32_t (&e)[P])
{
    const int L = log2_ceil(c->n);
    for (int p = 0; p < P; ++p) {
        e[p] = given ? given[p] : plane_exponent(maxabs[p], L);
        int32_t most = 0;
        if (!exponent_fits(e[p], maxabs[p], L, &most))
            return fail(c, BH_ERR_ARG, std::string(who) + ": exponent " + std::to_string(e[p]) + " of plane " + std::to_string(p) +
                                       " is too large for this context's bodies (at most " + std::to_string(most) + ")");
    }
    return BH_OK;
}

// a caller's nb + 1 bin edges, squared on the host: BH_ERR_ARG unless nb is 1 .. limit and the edges and their squares are finite,
// >= 0 and strictly ascending
int radial_edges(bh_ctx *c, const std::string &who, const double *edges, int32_t nb, const char *limit_name, int32_t limit,
                 std::vector<double> &e2)
{
    if (!edges) return fail(c, BH_ERR_ARG, who + ": null edges");
    const char *fault = edges_fault(squared_edges(edges, nb, limit, e2));
    if (!fault) return BH_OK;
    const std::string most = fault == kEdgesCountFault ? limit_name + std::string(" = ") + std::to_string(limit) : std::string();
    return fail(c, BH_ERR_ARG, who + ": " + fault + most);
}

// A deposit pass over radial slots between the marks ev[0] and ev[1], *ms the span: `words` of planes zeroed and, with bodies,
// the squared edges uploaded and `launch` enqueued.  Waits for the stream: e2 is the caller's to drop after this.
template <typename Launch>
int deposit_pass(bh_ctx *c, hipEvent_t *ev, double *ms, long long *planes, size_t words, double *e2_dev, const std::vector<double> &e2,
                 Launch &&launch)
{
    if (int rc = mark(c, ev[0])) return rc;
    BH_HIP(c, hipMemsetAsync(planes, 0, words * sizeof(long long), c->stream));
    if (c->n > 0) {
        BH_HIP(c, hipMemcpyAsync(e2_dev, e2.data(), e2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        launch();
        BH_HIP(c, hipGetLastError());
    }
    if (int rc = mark(c, ev[1])) return rc;
    BH_HIP(c, hipStreamSynchronize(c->stream));
    return span_ms(c, ev[0], ev[1], ms);
}

int points_finite(bh_ctx *c, const char *who, const double *points, int64_t n_points)
{
    const int64_t i = first_nonfinite_point(points, n_points);
    return i < 0 ? BH_OK : fail(c, BH_ERR_ARG, std::string(who) + ": point " + std::to_string(i) + " has a non-finite coordinate");
}

// one launch's query points: `rows` of them from the host into `points`, their keys in `box`, and the launch's sorted order
// (the index of a point travels in its key word: written by the last pass only, wherever it ends)
int sorted_query_chunk(bh_ctx *c, const double *host_points, int64_t rows, double2 *points, const double *box, uint64_t *const keys[2],
                       uint32_t *order, uint32_t *radix, uint32_t *rowsum)
{
    static_assert(kFieldKeyBits % kSortBits == 0 && kFieldKeyBits <= kPackShift && kFieldChunk <= ((int64_t)1 << (64 - kPackShift)),
                  "the keys and the indices of a launch share a word");
    BH_HIP(c, hipMemcpyAsync(points, host_points, (size_t)rows * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(field_keys_kernel, dim3(blocks_for(rows, kBlock)), dim3(kBlock), 0, c->stream, points, rows, box, keys[0]);
    uint32_t *const into[2] = {order, order};
    enqueue_lsd_passes<kFieldSortItems>(c->stream, keys, into, radix, rowsum, rows, kFieldKeyBits, true);
    return BH_OK;
}

// ---- moment maps (bh_moments.hpp).  They read pos / vel / mass as they lie in memory and write buffers of their own: no
// tree, no record of bh_run_state.hpp, so a step before and after runs bit for bit as it would have.
int map_check(bh_ctx *c, const char *who, const double *box, int32_t nx, int32_t ny, int32_t scheme)
{
    const std::string w(who);
    if (!box) return fail(c, BH_ERR_ARG, w + ": null box");
    if (nx < 1 || ny < 1) return fail(c, BH_ERR_ARG, w + ": nx and ny must be at least 1");
    if ((int64_t)nx * ny > kMapMaxCells)
        return fail(c, BH_ERR_ARG, w + ": nx * ny exceeds BH_MAP_MAX_CELLS = " + std::to_string(kMapMaxCells));
    if (scheme != BH_MAP_NGP && scheme != BH_MAP_CIC) return fail(c, BH_ERR_ARG, w + ": scheme must be BH_MAP_NGP or BH_MAP_CIC");
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(box[k])) return fail(c, BH_ERR_ARG, w + ": the box is not finite");
    if (!(box[0] < box[1]) || !(box[2] < box[3])) return fail(c, BH_ERR_ARG, w + ": the box is empty (needs xmin < xmax and ymin < ymax)");
    if (!std::isfinite(box[1] - box[0]) || !std::isfinite(box[3] - box[2]) || !std::isfinite((double)nx / (box[1] - box[0])) ||
        !std::isfinite((double)ny / (box[3] - box[2])))
        return fail(c, BH_ERR_ARG, w + ": the box's extent or the cells per unit length overflow fp64");
    return need_upload(c, w + " before bh_upload/bh_initialize");
}

int map_alloc(bh_ctx *c, int64_t cells)
{
    MapState &s = c->map;
    if (!s.max) { if (int rc = alloc_all(c, {part(&s.max, 1), part(&s.count, 1)})) return rc; }
    if (cells > s.cells) {
        dev_free(c, s.planes); s.planes = nullptr; s.cells = 0;
        if (int rc = dev_alloc(c, &s.planes, (size_t)kMapPlanes * cells)) return rc;
        s.cells = cells;
    }
    return BH_OK;
}

// pass 1: the four maxima on the host when this returns; BH_ERR_ARG when a body is not finite
int map_maxima(bh_ctx *c, const char *who, double (&maxabs)[kMapPlanes])
{
    for (double &v : maxabs) v = 0.0;
    if (c->n == 0) return BH_OK;
    if (int rc = map_alloc(c, 0)) return rc;
    MapMax r{};
    const int rc = first_pass(c, c->map.max, &r, maxabs, [&] {
        state_ptrs(c, [&](auto pos, auto vel, auto mass) {
            hipLaunchKernelGGL((moment_max_kernel<Pointee<decltype(pos)>, Pointee<decltype(mass)>>), dim3(blocks_for(c->n, kBlock)),
                               dim3(kBlock), 0, c->stream, pos, vel, mass, c->n, c->map.max);
        });
    });
    if (rc) return rc;
    if (r.bad)
        return fail(c, BH_ERR_ARG, std::string(who) + ": a body has a non-finite position, velocity or mass (or a moment m v, m |v|^2 that "
                                   "overflows fp64)");
    return BH_OK;
}

// both passes.  e: the caller's exponents `given` or, without, the rule's own from this context's maxima.  The grid stays on the
// device (map.planes), *n_deposited on the host.
int map_passes(bh_ctx *c, const char *who, const double *box, int32_t nx, int32_t ny, int32_t scheme, const int32_t *given,
               int32_t (&e)[kMapPlanes], int64_t *n_deposited)
{
    if (int rc = map_check(c, who, box, nx, ny, scheme)) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    double maxabs[kMapPlanes];
    if (int rc = map_maxima(c, who, maxabs)) return rc;
    if (int rc = plane_exponents(c, who, given, maxabs, e)) return rc;
    const int64_t cells = (int64_t)nx * ny;
    if (int rc = map_alloc(c, cells)) return rc;
    BH_HIP(c, hipMemsetAsync(c->map.planes, 0, (size_t)kMapPlanes * cells * sizeof(long long), c->stream));
    BH_HIP(c, hipMemsetAsync(c->map.count, 0, sizeof(unsigned long long), c->stream));
    if (c->n > 0) {
        MapGrid g{};
        g.xmin = box[0]; g.xmax = box[1]; g.ymin = box[2]; g.ymax = box[3];
        g.sx = (double)nx / (box[1] - box[0]);
        g.sy = (double)ny / (box[3] - box[2]);
        g.nx = nx; g.ny = ny;
        for (int p = 0; p < kMapPlanes; ++p) g.e[p] = e[p];
        state_ptrs(c, [&](auto pos, auto vel, auto mass) {
            dispatch([&](auto cic) {
                hipLaunchKernelGGL((moment_deposit_kernel<decltype(cic)::value, Pointee<decltype(pos)>, Pointee<decltype(mass)>>),
                                   dim3(blocks_for(c->n, kBlock)), dim3(kBlock), 0, c->stream, pos, vel, mass, c->n, g, c->map.planes,
                                   c->map.count);
            }, scheme == BH_MAP_CIC);
        });
        BH_HIP(c, hipGetLastError());
    }
    unsigned long long cnt = 0;
    BH_HIP(c, hipMemcpyAsync(&cnt, c->map.count, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    *n_deposited = (int64_t)cnt;
    return BH_OK;
}

// ---- radial profiles and Lagrangian radii (bh_radial.hpp).  As the moment maps: they read pos / vel / mass as they lie in
// memory and write buffers of their own -- no tree, no build, so there is nothing for a quiet scope (bh_run_state.hpp) to put
// back: no record of it is touched, and a step before and after runs bit for bit as it would have.
int rad_alloc(bh_ctx *c)
{
    RadState &s = c->rad;
    if (s.max) return BH_OK;
    return alloc_all(c, {part(&s.max, 1), part(&s.flags, 1), part(&s.e2, (size_t)kRadMaxBins + 1),
                         part(&s.planes, (size_t)(kRadPlanes + 1) * (kRadMaxBins + 2)),
                         part(&s.hist, (size_t)kRadMaxFractions * kRadDigits * 2)});
}

int rad_centre(bh_ctx *c, const char *who, const double *centre, const double *centre_vel, RadCentre *out)
{
    if (!centre) return fail(c, BH_ERR_ARG, std::string(who) + ": null centre");
    *out = RadCentre{centre[0], centre[1], centre_vel ? centre_vel[0] : 0.0, centre_vel ? centre_vel[1] : 0.0};
    if (!(std::isfinite(out->cx) && std::isfinite(out->cy) && std::isfinite(out->ux) && std::isfinite(out->uy)))
        return fail(c, BH_ERR_ARG, std::string(who) + ": the centre or its velocity is not finite");
    return BH_OK;
}

// persistent workgroups: at most rad.blocks of them, and none without a body
unsigned rad_grid(const bh_ctx *c) { return std::min<unsigned>((unsigned)c->rad.blocks, blocks_for(c->n, kBlock)); }

// pass 1: the five maxima on the host when this returns (with_vel = false: the mass alone, the velocities are not read);
// BH_ERR_ARG when a body is not finite, or -- no_negative -- when a mass is negative
int rad_maxima(bh_ctx *c, const char *who, const RadCentre &ctr, bool with_vel, bool no_negative, double (&maxabs)[kRadPlanes])
{
    RadState &s = c->rad;
    for (double &v : maxabs) v = 0.0;
    s.max_ms = 0.0;
    if (c->n == 0) return BH_OK;
    if (int rc = rad_alloc(c)) return rc;
    RadMax r{};
    const int rc = first_pass(c, s.max, &r, maxabs, [&] {
        state_ptrs(c, [&](auto pos, auto vel, auto mass) {
            dispatch([&](auto v) {
                hipLaunchKernelGGL((radial_max_kernel<decltype(v)::value, Pointee<decltype(pos)>, Pointee<decltype(mass)>>),
                                   dim3(rad_grid(c)), dim3(kBlock), 0, c->stream, pos, vel, mass, c->n, ctr, s.max);
            }, with_vel);
        });
    }, s.ev, &s.max_ms);
    if (rc) return rc;
    if (r.bad)
        return fail(c, BH_ERR_ARG, std::string(who) + ": a body has a non-finite position, velocity or mass (or a squared radius or a "
                                   "moment m vr, m vt, m vr^2, m vt^2 that overflows fp64)");
    if (no_negative && r.negative) return fail(c, BH_ERR_ARG, std::string(who) + ": a body has a negative mass");
    return BH_OK;
}

// both passes.  e: the caller's exponents `given` or, without, the rule's own from this context's maxima.  The planes stay on the
// device (rad.planes, 6 x (nb + 2)).
int rad_passes(bh_ctx *c, const char *who, const double *centre, const double *centre_vel, const double *edges, int32_t nb,
               const int32_t *given, int32_t (&e)[kRadPlanes])
{
    RadState &s = c->rad;
    const std::string w(who);
    RadCentre ctr{};
    std::vector<double> e2;
    if (int rc = rad_centre(c, who, centre, centre_vel, &ctr)) return rc;
    if (int rc = radial_edges(c, w, edges, nb, "BH_RADIAL_MAX_BINS", kRadMaxBins, e2)) return rc;
    if (int rc = need_upload(c, w + " before bh_upload/bh_initialize")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    double maxabs[kRadPlanes];
    if (int rc = rad_maxima(c, who, ctr, true, false, maxabs)) return rc;
    if (int rc = plane_exponents(c, who, given, maxabs, e)) return rc;
    if (int rc = rad_alloc(c)) return rc;
    const int S = nb + 2;
    s.main_ms = 0.0;
    for (double &v : s.round_ms) v = 0.0;
    return deposit_pass(c, s.ev + 2, &s.main_ms, s.planes, (size_t)(kRadPlanes + 1) * S, s.e2, e2, [&] {
        RadExp ex{};
        for (int p = 0; p < kRadPlanes; ++p) ex.e[p] = e[p];
        const bool priv = S <= kRadLdsSlots;
        const size_t lds = priv ? ((size_t)(kRadPlanes + 1) * S + (size_t)nb + 1) * 8 : (size_t)(kRadPlanes + 1) * kRadLdsSlots * 8;
        state_ptrs(c, [&](auto pos, auto vel, auto mass) {
            dispatch([&](auto p) {
                hipLaunchKernelGGL((radial_deposit_kernel<decltype(p)::value, Pointee<decltype(pos)>, Pointee<decltype(mass)>>),
                                   dim3(rad_grid(c)), dim3(kBlock), lds, c->stream, pos, vel, mass, c->n, ctr, s.e2, (int)nb, ex, s.planes);
            }, priv);
        });
    });
}

// one round: rad.hist[np][256][2] on the device and complete when this returns; timed between rad.ev[4 + 2 round] and the next
int rad_select_round(bh_ctx *c, const char *who, const RadCentre &ctr, int32_t e0, int32_t round, const uint64_t *prefixes, int32_t np)
{
    RadState &s = c->rad;
    if (int rc = rad_alloc(c)) return rc;
    const int L = log2_ceil(c->n);
    if (int rc = mark(c, s.ev[4 + 2 * round])) return rc;
    BH_HIP(c, hipMemsetAsync(s.hist, 0, (size_t)np * kRadDigits * 2 * sizeof(long long), c->stream));
    BH_HIP(c, hipMemsetAsync(s.flags, 0, sizeof(unsigned long long), c->stream));
    for (int32_t p0 = 0; p0 < np && c->n > 0; p0 += kRadSelChunk) {
        RadSelect sel{};
        sel.cx = ctr.cx; sel.cy = ctr.cy;
        sel.m_limit = std::ldexp(1.0, 62 - L - e0);
        sel.e0 = e0;
        sel.hi_shift = 64 - kRadDigitBits * round;
        sel.lo_shift = 64 - kRadDigitBits * (round + 1);
        sel.np = std::min<int32_t>(kRadSelChunk, np - p0);
        for (int k = 0; k < sel.np; ++k) sel.prefix[k] = prefixes[p0 + k];
        state_ptrs(c, [&](auto pos, auto, auto mass) {
            hipLaunchKernelGGL((radial_select_kernel<Pointee<decltype(pos)>, Pointee<decltype(mass)>>), dim3(rad_grid(c)), dim3(kBlock), 0,
                               c->stream, pos, mass, c->n, sel, s.hist + (size_t)p0 * kRadDigits * 2, s.flags);
        });
        BH_HIP(c, hipGetLastError());
    }
    if (int rc = mark(c, s.ev[5 + 2 * round])) return rc;
    unsigned long long flags = 0;
    BH_HIP(c, hipMemcpyAsync(&flags, s.flags, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    BH_HIP(c, hipStreamSynchronize(c->stream));
    if (int rc = span_ms(c, s.ev[4 + 2 * round], s.ev[5 + 2 * round], &s.round_ms[round])) return rc;
    if (flags & kRadFlagBad) return fail(c, BH_ERR_ARG, std::string(who) + ": a body has a non-finite position or mass (or a squared radius that overflows fp64)");
    if (flags & kRadFlagNegative) return fail(c, BH_ERR_ARG, std::string(who) + ": a body has a negative mass");
    if (flags & kRadFlagLarge)
        return fail(c, BH_ERR_ARG, std::string(who) + ": exponent " + std::to_string(e0) + " is too large for this context's masses and body count");
    return BH_OK;
}

// ---- azimuthal modes (bh_modes.hpp).  As the radial profiles: they read pos / vel / mass as they lie in memory and write
// buffers of their own -- no tree, no build, no record of bh_run_state.hpp.
int mod_alloc(bh_ctx *c)
{
    ModState &s = c->mod;
    if (s.max) return BH_OK;
    return alloc_all(c, {part(&s.max, 1), part(&s.e2, (size_t)kModMaxBins + 1),
                         part(&s.planes, (size_t)kModMaxPlanes * (kModMaxBins + 2))});
}

// pass 1: maxA and maxD on the host when this returns (without rates the velocities are not read and maxD is 0);
// BH_ERR_ARG when a body is not finite
int mod_maxima(bh_ctx *c, const char *who, const RadCentre &ctr, int M, bool rates, double (&maxabs)[2])
{
    ModState &s = c->mod;
    maxabs[0] = maxabs[1] = 0.0;
    s.max_ms = 0.0;
    if (c->n == 0) return BH_OK;
    if (int rc = mod_alloc(c)) return rc;
    ModMax r{};
    const int rc = first_pass(c, s.max, &r, maxabs, [&] {
        state_ptrs(c, [&](auto pos, auto vel, auto mass) {
            dispatch([&](auto rt) {
                hipLaunchKernelGGL((modes_max_kernel<decltype(rt)::value, Pointee<decltype(pos)>, Pointee<decltype(mass)>>),
                                   dim3(rad_grid(c)), dim3(kBlock), 0, c->stream, pos, vel, mass, c->n, ctr, M, s.max);
            }, rates);
        });
    }, s.ev, &s.max_ms);
    if (rc) return rc;
    if (r.bad)
        return fail(c, BH_ERR_ARG, std::string(who) + ": the first pass found a body with a non-finite position, " +
                                   (rates ? "velocity, " : "") + "mass or squared radius, or a contribution m c_k, m s_k" +
                                   (rates ? ", m w c_k, m w s_k (w = b / r2)" : "") + " that overflows fp64");
    return BH_OK;
}

int mod_args(bh_ctx *c, const char *who, const double *centre, const double *centre_vel, int32_t M, RadCentre *ctr)
{
    if (int rc = rad_centre(c, who, centre, centre_vel, ctr)) return rc;
    if (M < 0 || M > kModMaxM) return fail(c, BH_ERR_ARG, std::string(who) + ": M must be 0 .. BH_MODES_MAX_M = " + std::to_string(kModMaxM));
    return BH_OK;
}

// both passes.  e: the caller's two exponents `given` or, without, the rule's own from this context's maxima.  The planes stay
// on the device (mod.planes, P x (nb + 2)).
int mod_passes(bh_ctx *c, const char *who, const double *centre, const double *centre_vel, const double *edges, int32_t nb, int32_t M,
               bool rates, const int32_t *given, int32_t (&e)[2])
{
    ModState &s = c->mod;
    const std::string w(who);
    RadCentre ctr{};
    std::vector<double> e2;
    if (int rc = mod_args(c, who, centre, centre_vel, M, &ctr)) return rc;
    if (int rc = radial_edges(c, w, edges, nb, "BH_MODES_MAX_BINS", kModMaxBins, e2)) return rc;
    if (int rc = need_upload(c, w + " before bh_upload/bh_initialize")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    double maxabs[2];
    if (int rc = mod_maxima(c, who, ctr, M, rates, maxabs)) return rc;
    if (int rc = plane_exponents(c, who, given, maxabs, e)) return rc;
    if (int rc = mod_alloc(c)) return rc;
    const int S = nb + 2, P = modes_planes(M, rates);
    s.deposit_ms = 0.0;
    return deposit_pass(c, s.ev + 2, &s.deposit_ms, s.planes, (size_t)P * S, s.e2, e2, [&] {
        const ModesPlan plan = modes_plan(P, nb);
        state_ptrs(c, [&](auto pos, auto vel, auto mass) {
            dispatch([&](auto r) {
                hipLaunchKernelGGL((modes_deposit_kernel<decltype(r)::value, Pointee<decltype(pos)>, Pointee<decltype(mass)>>),
                                   dim3(rad_grid(c)), dim3(kBlock), plan.bytes, c->stream, pos, vel, mass, c->n, ctr, s.e2, (int)nb, (int)M,
                                   plan.tile, (int)e[0], (int)e[1], s.planes);
            }, rates);
        });
    });
}

// ---- the rotation curve (bh_disc.hpp).  It reads pos, mass and the force buffer as they lie in memory (slot for slot) and
// writes buffers of its own: no record of bh_run_state.hpp changes.  disc_alloc serves bh_set_disc_velocities (bh_engine.hip) too.
int disc_alloc(bh_ctx *c)
{
    DiscState &s = c->disc;
    if (s.max) return BH_OK;
    return alloc_all(c, {part(&s.max, 1), part(&s.e2, (size_t)kDiscMaxBins + 1), part(&s.tables, (size_t)kDiscTables * kDiscMaxTable),
                         part(&s.planes, (size_t)(kDiscPlanes + 1) * (kDiscMaxBins + 2))});
}

// f(pos, mass, force) as the precision types them: the force buffer holds fp32 accelerations unless the tree is fp64
template <typename F>
void curve_ptrs(const bh_ctx *c, F &&f)
{
    switch (c->mode) {
    case Mode::F32: f((const float2 *)c->pos, (const float *)c->mass, (const float2 *)c->force); break;
    case Mode::Mixed: f((const double2 *)c->pos, (const double *)c->mass, (const float2 *)c->force); break;
    case Mode::F64:
    case Mode::Exact: f((const double2 *)c->pos, (const double *)c->mass, (const double2 *)c->force); break;
    }
}

// ---- the field at arbitrary points (bh_field.hpp)
// The tree comes from a quiet build (quietly), with the walk counters of bh_stats copied aside and put back as in
// check_walk (keys_kernel clears them).  The kernels read the tree and the call's own buffers and write the call's own buffers
// only: force, body_counts, group_cost, phi, the event timings and walk_launches are not touched.
int field_alloc(bh_ctx *c, int64_t want)
{
    FieldState &s = c->field;
    if (want <= s.block.cap) return BH_OK;
    const int64_t cap = grown_capacity(want);                  // (want <= kFieldChunk, a power of two)
    const size_t n = (size_t)cap, nbl = blocks_for(cap, kBlock * kFieldSortItems);
    return block_regrow(c, s.block, cap, {part(&s.points, n), part(&s.accel, n), part(&s.keys[0], n), part(&s.keys[1], n),
                                          part(&s.phi, n), part(&s.order, n), part(&s.counts, n),
                                          part(&s.radix, (size_t)kRadix * nbl), part(&s.rows, (size_t)kRadix)});
}

// one launch of k <= field.block.cap points: upload, keys, sort, walk; results at the points' places
int enqueue_field(bh_ctx *c, const double *points, int64_t k)
{
    FieldState &s = c->field;
    hipStream_t st = c->stream;
    const unsigned grid = blocks_for(k, kBlock);
    if (int rc = sorted_query_chunk(c, points, k, s.points, c->box, s.keys, s.order, s.radix, s.rows)) return rc;
    if (c->tree64()) {
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, c->gd, c->ld, s.order, s.points, k, c->cfg.theta, c->cfg.G, c->eps2,
                               c->ctr, s.accel, s.phi, s.counts);
        };
        if (c->mode == Mode::F64) go(field_f64_kernel<kAcceptThr>);
        else if (c->exact_thresholds) go(field_f64_kernel<kAcceptExactThr>);
        else go(field_f64_kernel<kAcceptSize>);
    } else {
        hipLaunchKernelGGL(field_f32_kernel, dim3(grid), dim3(kBlock), 0, st, c->qf, c->aux, c->spos, c->smass, s.order, s.points, k,
                           c->cfg.G, c->eps2f, c->ctr, s.accel, s.phi, s.counts);
    }
    BH_HIP(c, hipGetLastError());
    return BH_OK;
}

// ---- neighbour queries (bh_neighbours.hpp).  They read pos (and orig) as they lie in memory and write buffers of their own: no
// force tree, no record of bh_run_state.hpp, no counter and no timing of the run, so a step before and after runs bit for bit as
// it would have.
constexpr int64_t kNbChunk = kFieldChunk;       // queries per launch: a point's index travels in its key word

// the structure's block for n bodies and the launch block for `rows` queries of `entries` list entries in all
int nb_alloc(bh_ctx *c, int64_t n, int64_t rows, int64_t entries)
{
    NbState &s = c->nb;
    if (n > s.block.cap) {
        const int64_t cap = grown_capacity(n);
        int32_t off[kNbMaxLevels + 1];
        nb_levels(cap, off);
        const size_t nodes = (size_t)off[kNbMaxLevels] + kNbMaxLevels;            // (n <= cap has at most a node more per level)
        const size_t b = (size_t)cap, nbl = blocks_for(std::max(cap, kNbChunk), kBlock * kFieldSortItems);
        if (int rc = block_regrow(c, s.block, cap, {part(&s.spos, b), part(&s.boxes, nodes), part(&s.keys[0], b), part(&s.keys[1], b),
                                                    part(&s.bounds, 1), part(&s.box, 4), part(&s.slot, b), part(&s.sidx, b),
                                                    part(&s.radix, (size_t)kRadix * nbl), part(&s.rowsum, (size_t)kRadix),
                                                    part(&s.off, (size_t)kNbMaxLevels + 1)}))
            return rc;
    }
    if (rows > s.qblock.cap || entries > s.entries) {
        const int64_t cap = grown_capacity(rows, std::max<int64_t>(s.qblock.cap, 1024)), ent = std::max(entries, s.entries);
        const size_t q = (size_t)cap;
        s.entries = 0;
        if (int rc = block_regrow(c, s.qblock, cap, {part(&s.points, q), part(&s.pkeys[0], q), part(&s.pkeys[1], q),
                                                     part(&s.idx, (size_t)ent), part(&s.d2, (size_t)ent), part(&s.order, q),
                                                     part(&s.evals, q)}))
            return rc;
        s.entries = ent;
    }
    return BH_OK;
}

// bounds, keys, sort, sorted copies and boxes of the current state (n > 0), between the marks nb.ev[0] and nb.ev[1]; BH_ERR_ARG
// when a position is not finite.  *levels: the levels of the hierarchy.
int nb_build(bh_ctx *c, const char *who, int *levels)
{
    NbState &s = c->nb;
    hipStream_t st = c->stream;
    const int64_t n = c->n;
    const unsigned grid = blocks_for(n, kBlock);
    const NbBounds empty{~0ull, 0ull, ~0ull, 0ull, 0ull};
    if (int rc = mark(c, s.ev[0])) return rc;
    BH_HIP(c, hipMemcpyAsync(s.bounds, &empty, sizeof(empty), hipMemcpyHostToDevice, st));
    BH_HIP(c, hipStreamSynchronize(st));                        // (`empty` lives on this stack)
    with_state(c, [&](auto r2) {
        using Real2 = decltype(r2);
        hipLaunchKernelGGL((nb_bounds_kernel<Real2>), dim3(grid), dim3(kBlock), 0, st, static_cast<const Real2 *>(c->pos), n, s.bounds);
    });
    BH_HIP(c, hipGetLastError());
    NbBounds got{};
    BH_HIP(c, hipMemcpyAsync(&got, s.bounds, sizeof(got), hipMemcpyDeviceToHost, st));
    BH_HIP(c, hipStreamSynchronize(st));
    if (got.bad)
        return fail(c, BH_ERR_ARG, std::string(who) + ": a body of the state has a non-finite position (found by the bounds pass)");
    hipLaunchKernelGGL(nb_setup_kernel, dim3(1), dim3(1), 0, st, s.bounds, n, s.box, s.off);
    const uint32_t *orig = (c->tree64() || c->is.orig_identity) ? nullptr : c->orig;
    static_assert(kFieldKeyBits % kSortBits == 0 && ((kFieldKeyBits / kSortBits) & 1) == 0, "the sorted keys end in the first array");
    with_state(c, [&](auto r2) {
        using Real2 = decltype(r2);
        const Real2 *pos = static_cast<const Real2 *>(c->pos);
        hipLaunchKernelGGL((nb_keys_kernel<Real2>), dim3(grid), dim3(kBlock), 0, st, pos, n, s.box, s.keys[0]);
        uint32_t *const slot[2] = {s.slot, s.slot};            // (packed: written by the last pass only)
        enqueue_lsd_passes<kFieldSortItems>(st, s.keys, slot, s.radix, s.rowsum, n, kFieldKeyBits, true);
        hipLaunchKernelGGL((nb_gather_kernel<Real2>), dim3(grid), dim3(kBlock), 0, st, pos, s.slot, orig, n, s.spos, s.sidx);
    });
    int32_t off[kNbMaxLevels + 1];
    *levels = nb_levels(n, off);
    hipLaunchKernelGGL(nb_leaf_kernel, dim3(blocks_for(off[1], kBlock)), dim3(kBlock), 0, st, s.spos, n, off[1], s.boxes);
    for (int l = 1; l < *levels; ++l) {
        const int32_t count = off[l + 1] - off[l], below = off[l] - off[l - 1];
        hipLaunchKernelGGL(nb_level_kernel, dim3(blocks_for(count, kBlock)), dim3(kBlock), 0, st, s.boxes + off[l - 1], below,
                           s.boxes + off[l], count);
    }
    BH_HIP(c, hipGetLastError());
    return mark(c, s.ev[1]);
}

// a launch's queries, between the marks nb.ev[2] and nb.ev[3]: `rows` of the caller's points from `points` on, sorted, or
// (points == nullptr) the bodies themselves; then search() enqueues the family's kernel
template <typename Search>
int nb_launch(bh_ctx *c, const double *points, int64_t rows, Search &&search)
{
    NbState &s = c->nb;
    if (int rc = mark(c, s.ev[2])) return rc;
    if (points) { if (int rc = sorted_query_chunk(c, points, rows, s.points, s.box, s.pkeys, s.order, s.radix, s.rowsum)) return rc; }
    search();
    BH_HIP(c, hipGetLastError());
    return mark(c, s.ev[3]);
}

// Both queries.  k > 0: bh_neighbours; k == 0: bh_count_within at r2.  Rows come back in the launch's sorted order and are put
// at their caller places here.
int nb_query(bh_ctx *c, const char *who, const double *points, int64_t n_points, int32_t k, double r2, int64_t *idx, double *d2,
             uint32_t *evals)
{
    NbState &s = c->nb;
    const std::string w(who);
    if (int rc = diag_check(c, who)) return rc;
    if (!points && n_points != c->n) return fail(c, BH_ERR_ARG, w + ": without points, n_points must be the number of bodies");
    if (int rc = points_finite(c, who, points, n_points)) return rc;
    if (n_points == 0) return BH_OK;
    const int64_t n = c->n;
    if (n > kNbMaxBodies) return fail(c, BH_ERR_CAPACITY, w + ": more than 2^24 bodies (their indices share a key word)");
    const int64_t kk = std::max<int32_t>(k, 1);               // entries per row on the host side (counts: one)
    if (n == 0) {                                              // no bodies: nobody is near
        if (idx) std::fill(idx, idx + n_points * kk, (int64_t)-1);
        if (d2) std::fill(d2, d2 + n_points * kk, (double)INFINITY);
        if (evals) std::fill(evals, evals + n_points, 0u);
        return BH_OK;
    }
    BH_HIP(c, hipSetDevice(c->device));
    const int64_t rows_max = std::min(n_points, kNbChunk);
    if (int rc = nb_alloc(c, n, rows_max, rows_max * k)) return rc;
    int levels = 0;
    if (int rc = nb_build(c, who, &levels)) return rc;
    hipStream_t st = c->stream;
    std::vector<uint32_t> dest((size_t)rows_max), hev((size_t)rows_max);
    std::vector<int64_t> hidx(idx ? (size_t)(rows_max * k) : 0);
    std::vector<double> hd2(d2 ? (size_t)(rows_max * k) : 0);
    std::vector<uint32_t> sidx;
    if (!points) {
        sidx.resize((size_t)n);
        BH_HIP(c, hipMemcpyAsync(sidx.data(), s.sidx, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    s.query_ms = 0.0;
    for (int64_t t0 = 0; t0 < n_points; t0 += kNbChunk) {
        const int64_t rows = std::min(kNbChunk, n_points - t0);
        auto search = [&](auto pts) {
            constexpr bool PTS = decltype(pts)::value;
            if (k > 0)
                hipLaunchKernelGGL((nb_knn_kernel<PTS>), dim3(blocks_for(rows, kWave)), dim3(kWave), (size_t)k * kWave * 12, st, s.spos,
                                   s.sidx, s.keys[0], s.boxes, s.off, levels, (int32_t)n, k, s.points, s.order, s.pkeys[0], t0, rows, s.idx,
                                   s.d2, s.evals);
            else
                hipLaunchKernelGGL((nb_count_kernel<PTS>), dim3(blocks_for(rows, kBlock)), dim3(kBlock), 0, st, s.spos, s.boxes, s.off,
                                   levels, (int32_t)n, s.points, s.order, t0, rows, r2, s.evals);
        };
        if (int rc = nb_launch(c, points ? points + 2 * t0 : nullptr, rows, [&] { dispatch(search, points != nullptr); })) return rc;
        if (points) BH_HIP(c, hipMemcpyAsync(dest.data(), s.order, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (idx) BH_HIP(c, hipMemcpyAsync(hidx.data(), s.idx, (size_t)(rows * k) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (d2) BH_HIP(c, hipMemcpyAsync(hd2.data(), s.d2, (size_t)(rows * k) * sizeof(double), hipMemcpyDeviceToHost, st));
        if (evals) BH_HIP(c, hipMemcpyAsync(hev.data(), s.evals, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipStreamSynchronize(st));
        if (int rc = span_ms(c, s.ev[2], s.ev[3], &s.query_ms, true)) return rc;
        for (int64_t r = 0; r < rows; ++r) {
            const int64_t at = points ? t0 + (int64_t)dest[(size_t)r] : (int64_t)sidx[(size_t)(t0 + r)];
            if (idx) std::copy(hidx.begin() + r * k, hidx.begin() + (r + 1) * k, idx + at * k);
            if (d2) std::copy(hd2.begin() + r * k, hd2.begin() + (r + 1) * k, d2 + at * k);
            if (evals) evals[at] = hev[(size_t)r];
        }
    }
    return span_ms(c, s.ev[0], s.ev[1], &s.build_ms);
}

// ---- friends-of-friends groups (bh_groups.hpp) on the structure of the neighbour queries.  They read pos, vel, mass and orig as
// they lie in memory and write buffers of their own: a step before and after runs bit for bit as it would have.
int fof_alloc(bh_ctx *c, int64_t n)
{
    FofState &s = c->fof;
    if (n <= s.block.cap) return BH_OK;
    const size_t b = (size_t)grown_capacity(n);
    return block_regrow(c, s.block, (int64_t)b, {part(&s.sums, b * kGrpPlanes), part(&s.label, b), part(&s.ctr, 1), part(&s.max, 1),
                                                 part(&s.parent, b), part(&s.root, b), part(&s.minidx, b), part(&s.count, b),
                                                 part(&s.rec_label, b), part(&s.rec_count, b)});
}

// ---- spanning trees (bh_mst.hpp) on the structure of the neighbour queries, and of subsets on the state itself.  They read pos
// and orig as they lie in memory and write buffers of their own: a step before and after runs bit for bit as it would have.
int mst_alloc(bh_ctx *c, int64_t n)
{
    MstState &s = c->mst;
    if (n <= s.block.cap) return BH_OK;
    const int64_t cap = grown_capacity(n);
    int32_t off[kNbMaxLevels + 1];
    nb_levels(cap, off);
    const size_t nodes = (size_t)off[kNbMaxLevels] + kNbMaxLevels, b = (size_t)cap;       // (as nb_alloc)
    return block_regrow(c, s.block, cap, {part(&s.seedmin, b), part(&s.mind2, b), part(&s.minpair, b), part(&s.cand_d2, b), part(&s.cand_pair, b),
                                          part(&s.edge_pair, b), part(&s.edge_d2, b), part(&s.ctr, 1), part(&s.parent, b),
                                          part(&s.comp, b), part(&s.inv, b), part(&s.nodecomp, nodes)});
}

// an edge as the device leaves it, and the edge order
struct MstEdge {
    uint64_t d2, pair;
    bool operator<(const MstEdge &o) const { return d2 < o.d2 || (d2 == o.d2 && pair < o.pair); }
};

// `count` edges in ascending edge order into lo / hi / d2
void mst_sorted_out(MstEdge *e, int64_t count, int64_t *lo, int64_t *hi, double *d2)
{
    std::sort(e, e + count);
    for (int64_t k = 0; k < count; ++k) {
        lo[k] = (int64_t)(e[k].pair >> 24);
        hi[k] = (int64_t)(e[k].pair & 0xffffffull);
        std::memcpy(&d2[k], &e[k].d2, sizeof(double));
    }
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- bound pairs (bh_binaries.hpp) on the structure of the neighbour queries.  They read pos, vel, mass and orig as they lie in
// memory and write buffers of their own -- no force tree, no build, so there is nothing for a quiet scope to put back: a step
// before and after runs bit for bit as it would have.
int bin_alloc(bh_ctx *c, int64_t n)
{
    BinState &s = c->bin;
    if (n <= s.block.cap) return BH_OK;
    const int64_t cap = grown_capacity(n);
    int32_t off[kNbMaxLevels + 1];
    nb_levels(cap, off);
    const size_t nodes = (size_t)off[kNbMaxLevels] + kNbMaxLevels, b = (size_t)cap, room = b / 2 + 1;       // (nodes: as nb_alloc)
    return block_regrow(c, s.block, cap, {part(&s.svel, b), part(&s.smass, b), part(&s.nodemass, nodes), part(&s.eps, b),
                                          part(&s.rec, room * kBinRecord), part(&s.partner, b), part(&s.ctr, 1), part(&s.psort, b),
                                          part(&s.rec_lo, room), part(&s.rec_hi, room)});
}

// ---- neighbour lists (bh_neighbour_lists.hpp) on the structure of the neighbour queries.  As those: they read pos (and orig) as
// they lie in memory and write buffers of their own, so a step before and after runs bit for bit as it would have.
int nbl_alloc(bh_ctx *c, int64_t rows, int64_t entries, bool merge)
{
    NblState &s = c->nbl;
    if (rows > s.block.cap) {
        const int64_t cap = grown_capacity(rows);
        const size_t q = (size_t)cap;
        if (int rc = block_regrow(c, s.block, cap, {part(&s.counts, q), part(&s.evals, q), part(&s.rows_lds, q), part(&s.rows_merge, q),
                                                    part(&s.cursors, q), part(&s.rad2, q),
                                                    part(&s.tiles, (size_t)blocks_for(cap, kNblScanTile) + 1), part(&s.ctr, 1)}))
            return rc;
    }
    if (entries > s.eblock.cap) {
        if (int rc = block_regrow(c, s.eblock, entries, {part(&s.ent_d2, (size_t)entries), part(&s.ent_idx, (size_t)entries)})) return rc;
    }
    if (merge && s.eblock.cap > s.ablock.cap) {
        const size_t e = (size_t)s.eblock.cap;
        if (int rc = block_regrow(c, s.ablock, s.eblock.cap, {part(&s.alt_d2, e), part(&s.alt_idx, e)})) return rc;
    }
    return BH_OK;
}

int32_t pow2_at_least(int64_t v) { int32_t t = 2; while (t < v) t <<= 1; return t; }

}  // namespace

extern "C" {

int bh_moment_map_max(bh_ctx *c, double *maxabs)
{
    if (!c) return BH_ERR_ARG;
    if (!maxabs) return fail(c, BH_ERR_ARG, "bh_moment_map_max: null output");
    if (int rc = need_upload(c, "bh_moment_map_max before bh_upload/bh_initialize")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    double m[kMapPlanes];
    if (int rc = map_maxima(c, "bh_moment_map_max", m)) return rc;
    std::copy(m, m + kMapPlanes, maxabs);
    return BH_OK;
}

int bh_moment_map_deposit(bh_ctx *c, const double *box, int32_t nx, int32_t ny, int32_t scheme, const int32_t *exponents,
                          void **planes_dev, int64_t *n_deposited)
{
    if (!c) return BH_ERR_ARG;
    if (!exponents || !planes_dev || !n_deposited) return fail(c, BH_ERR_ARG, "bh_moment_map_deposit: null argument");
    int32_t e[kMapPlanes];
    if (int rc = map_passes(c, "bh_moment_map_deposit", box, nx, ny, scheme, exponents, e, n_deposited)) return rc;
    *planes_dev = c->map.planes;
    return BH_OK;
}

int bh_moment_map(bh_ctx *c, const double *box, int32_t nx, int32_t ny, int32_t scheme, int64_t *planes, int32_t *exponents,
                  int64_t *n_deposited)
{
    if (!c) return BH_ERR_ARG;
    if (!planes || !exponents || !n_deposited) return fail(c, BH_ERR_ARG, "bh_moment_map: null argument");
    int32_t e[kMapPlanes];
    if (int rc = map_passes(c, "bh_moment_map", box, nx, ny, scheme, nullptr, e, n_deposited)) return rc;
    BH_HIP(c, hipMemcpy(planes, c->map.planes, (size_t)kMapPlanes * nx * ny * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::copy(e, e + kMapPlanes, exponents);
    return BH_OK;
}

int bh_radial_max(bh_ctx *c, const double *centre, const double *centre_vel, double *maxabs)
{
    if (!c) return BH_ERR_ARG;
    if (!maxabs) return fail(c, BH_ERR_ARG, "bh_radial_max: null output");
    RadCentre ctr{};
    if (int rc = rad_centre(c, "bh_radial_max", centre, centre_vel, &ctr)) return rc;
    if (int rc = need_upload(c, "bh_radial_max before bh_upload/bh_initialize")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    double m[kRadPlanes];
    if (int rc = rad_maxima(c, "bh_radial_max", ctr, true, false, m)) return rc;
    std::copy(m, m + kRadPlanes, maxabs);
    return BH_OK;
}

int bh_radial_deposit(bh_ctx *c, const double *centre, const double *centre_vel, const double *edges, int32_t nb,
                      const int32_t *exponents, void **planes_dev)
{
    if (!c) return BH_ERR_ARG;
    if (!exponents || !planes_dev) return fail(c, BH_ERR_ARG, "bh_radial_deposit: null argument");
    int32_t e[kRadPlanes];
    if (int rc = rad_passes(c, "bh_radial_deposit", centre, centre_vel, edges, nb, exponents, e)) return rc;
    *planes_dev = c->rad.planes;
    return BH_OK;
}

int bh_radial_profile(bh_ctx *c, const double *centre, const double *centre_vel, const double *edges, int32_t nb, int64_t *planes,
                      int32_t *exponents)
{
    if (!c) return BH_ERR_ARG;
    if (!planes || !exponents) return fail(c, BH_ERR_ARG, "bh_radial_profile: null argument");
    int32_t e[kRadPlanes];
    if (int rc = rad_passes(c, "bh_radial_profile", centre, centre_vel, edges, nb, nullptr, e)) return rc;
    BH_HIP(c, hipMemcpy(planes, c->rad.planes, (size_t)(kRadPlanes + 1) * (nb + 2) * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::copy(e, e + kRadPlanes, exponents);
    return BH_OK;
}

int bh_radial_select(bh_ctx *c, const double *centre, int32_t exponent, int32_t round, const uint64_t *prefixes, int32_t np,
                     void **hist_dev)
{
    if (!c) return BH_ERR_ARG;
    if (!hist_dev) return fail(c, BH_ERR_ARG, "bh_radial_select: null output");
    RadCentre ctr{};
    if (int rc = rad_centre(c, "bh_radial_select", centre, nullptr, &ctr)) return rc;
    if (const char *why = select_prefix_fault(round, prefixes, np)) return fail(c, BH_ERR_ARG, std::string("bh_radial_select: ") + why);
    if (int rc = need_upload(c, "bh_radial_select before bh_upload/bh_initialize")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    c->rad.max_ms = 0.0; c->rad.main_ms = 0.0;
    for (double &v : c->rad.round_ms) v = 0.0;
    if (int rc = rad_select_round(c, "bh_radial_select", ctr, exponent, round, prefixes, np)) return rc;
    c->rad.main_ms = c->rad.round_ms[round];
    *hist_dev = c->rad.hist;
    return BH_OK;
}

int bh_lagrangian_radii(bh_ctx *c, const double *centre, const double *fractions, int32_t nf, double *r2, int64_t *count, int64_t *mass,
                        int32_t *exponent)
{
    if (!c) return BH_ERR_ARG;
    if (!fractions || !r2 || !count || !mass || !exponent) return fail(c, BH_ERR_ARG, "bh_lagrangian_radii: null argument");
    RadCentre ctr{};
    if (int rc = rad_centre(c, "bh_lagrangian_radii", centre, nullptr, &ctr)) return rc;
    if (nf < 1 || nf > kRadMaxFractions) return fail(c, BH_ERR_ARG, "bh_lagrangian_radii: nf must be 1 .. BH_RADIAL_MAX_FRACTIONS = 32");
    for (int32_t f = 0; f < nf; ++f)
        if (!(std::isfinite(fractions[f]) && fractions[f] > 0.0 && fractions[f] <= 1.0))
            return fail(c, BH_ERR_ARG, "bh_lagrangian_radii: a fraction must be finite, > 0 and <= 1");
    if (int rc = need_upload(c, "bh_lagrangian_radii before bh_upload/bh_initialize")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    double m[kRadPlanes];
    if (int rc = rad_maxima(c, "bh_lagrangian_radii", ctr, false, true, m)) return rc;
    const int32_t e0 = plane_exponent(m[0], log2_ceil(c->n));
    *exponent = e0;
    c->rad.main_ms = 0.0;
    for (double &v : c->rad.round_ms) v = 0.0;
    // the decisions between the rounds are made here, on the host, from the downloaded histograms
    LagrangianSelect sel(fractions, nf);
    std::vector<int64_t> hist((size_t)kRadMaxFractions * kRadDigits * 2);
    while (!sel.done()) {
        const int32_t round = sel.round;
        const uint64_t *distinct = nullptr;
        const int32_t np = sel.prefixes(&distinct);
        if (int rc = rad_select_round(c, "bh_lagrangian_radii", ctr, e0, round, distinct, np)) return rc;
        c->rad.main_ms += c->rad.round_ms[round];
        BH_HIP(c, hipMemcpy(hist.data(), c->rad.hist, (size_t)np * kRadDigits * 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
        sel.advance(hist.data());
    }
    sel.result(r2, count, mass);
    return BH_OK;
}

int bh_radial_times(bh_ctx *c, double *max_ms, double *main_ms, double *rounds_ms)
{
    if (!c || !max_ms || !main_ms) return fail(c, BH_ERR_ARG, "bh_radial_times: null argument");
    *max_ms = c->rad.max_ms;
    *main_ms = c->rad.main_ms;
    if (rounds_ms) std::copy(c->rad.round_ms, c->rad.round_ms + kRadRounds, rounds_ms);
    return BH_OK;
}

int bh_modes_max(bh_ctx *c, const double *centre, const double *centre_vel, int32_t M, int32_t rates, double *maxabs)
{
    if (!c) return BH_ERR_ARG;
    if (!maxabs) return fail(c, BH_ERR_ARG, "bh_modes_max: null output");
    RadCentre ctr{};
    if (int rc = mod_args(c, "bh_modes_max", centre, centre_vel, M, &ctr)) return rc;
    if (int rc = need_upload(c, "bh_modes_max before bh_upload/bh_initialize")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    double m[2];
    if (int rc = mod_maxima(c, "bh_modes_max", ctr, M, rates != 0, m)) return rc;
    std::copy(m, m + 2, maxabs);
    return BH_OK;
}

int bh_modes_deposit(bh_ctx *c, const double *centre, const double *centre_vel, const double *edges, int32_t nb, int32_t M,
                     int32_t rates, const int32_t *exponents, void **planes_dev)
{
    if (!c) return BH_ERR_ARG;
    if (!exponents || !planes_dev) return fail(c, BH_ERR_ARG, "bh_modes_deposit: null argument");
    int32_t e[2];
    if (int rc = mod_passes(c, "bh_modes_deposit", centre, centre_vel, edges, nb, M, rates != 0, exponents, e)) return rc;
    *planes_dev = c->mod.planes;
    return BH_OK;
}

int bh_azimuthal_modes(bh_ctx *c, const double *centre, const double *centre_vel, const double *edges, int32_t nb, int32_t M,
                       int32_t rates, int64_t *planes, int32_t *exponents)
{
    if (!c) return BH_ERR_ARG;
    if (!planes || !exponents) return fail(c, BH_ERR_ARG, "bh_azimuthal_modes: null argument");
    int32_t e[2];
    if (int rc = mod_passes(c, "bh_azimuthal_modes", centre, centre_vel, edges, nb, M, rates != 0, nullptr, e)) return rc;
    BH_HIP(c, hipMemcpy(planes, c->mod.planes, (size_t)modes_planes(M, rates != 0) * (nb + 2) * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::copy(e, e + 2, exponents);
    return BH_OK;
}

int bh_modes_times(bh_ctx *c, double *max_ms, double *deposit_ms)
{
    if (!c || !max_ms || !deposit_ms) return fail(c, BH_ERR_ARG, "bh_modes_times: null argument");
    *max_ms = c->mod.max_ms;
    *deposit_ms = c->mod.deposit_ms;
    return BH_OK;
}

int bh_rotation_curve(bh_ctx *c, const double *centre, const double *edges, int32_t nb, int64_t *planes, int32_t *exponents)
{
    if (!c) return BH_ERR_ARG;
    if (!planes || !exponents) return fail(c, BH_ERR_ARG, "bh_rotation_curve: null argument");
    DiscState &s = c->disc;
    RadCentre ctr{};
    std::vector<double> e2;
    if (int rc = rad_centre(c, "bh_rotation_curve", centre, nullptr, &ctr)) return rc;
    if (int rc = radial_edges(c, "bh_rotation_curve", edges, nb, "BH_DISC_MAX_BINS", kDiscMaxBins, e2)) return rc;
    if (int rc = split_check(c, "bh_rotation_curve")) return rc;
    if (int rc = need_forces(c, "bh_rotation_curve")) return rc;
    BH_HIP(c, hipSetDevice(c->device));
    if (int rc = disc_alloc(c)) return rc;
    const int S = nb + 2;
    s.max_ms = s.deposit_ms = 0.0;
    double maxabs[kDiscPlanes] = {0.0, 0.0, 0.0, 0.0};
    if (c->n > 0) {
        DiscMax r{};
        const int rc = first_pass(c, s.max, &r, maxabs, [&] {
            curve_ptrs(c, [&](auto pos, auto mass, auto force) {
                hipLaunchKernelGGL((curve_max_kernel<Pointee<decltype(pos)>, Pointee<decltype(mass)>, Pointee<decltype(force)>>),
                                   dim3(rad_grid(c)), dim3(kBlock), 0, c->stream, pos, mass, force, c->n, ctr, s.max);
            });
        }, s.ev + 2, &s.max_ms);
        if (rc) return rc;
        if (r.bad)
            return fail(c, BH_ERR_ARG, "bh_rotation_curve: a body has a non-finite position, mass or acceleration (a massless body of an "
                                       "fp64 tree: 0 / 0), or a squared radius or a contribution m r, m (x . a), m (x x a) that overflows fp64");
    }
    int32_t e[kDiscPlanes];
    if (int rc = plane_exponents(c, "bh_rotation_curve", nullptr, maxabs, e)) return rc;
    const int rc = deposit_pass(c, s.ev + 4, &s.deposit_ms, s.planes, (size_t)(kDiscPlanes + 1) * S, s.e2, e2, [&] {
        DiscExp ex{};
        for (int p = 0; p < kDiscPlanes; ++p) ex.e[p] = e[p];
        const size_t lds = ((size_t)(kDiscPlanes + 1) * S + (size_t)nb + 1) * 8;
        curve_ptrs(c, [&](auto pos, auto mass, auto force) {
            hipLaunchKernelGGL((curve_deposit_kernel<Pointee<decltype(pos)>, Pointee<decltype(mass)>, Pointee<decltype(force)>>),
                               dim3(rad_grid(c)), dim3(kBlock), lds, c->stream, pos, mass, force, c->n, ctr, s.e2, (int)nb, ex, s.planes);
        });
    });
    if (rc) return rc;
    BH_HIP(c, hipMemcpy(planes, s.planes, (size_t)(kDiscPlanes + 1) * S * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::copy(e, e + kDiscPlanes, exponents);
    return BH_OK;
}

int bh_field_at(bh_ctx *c, const double *points, int64_t n_points, double *accel, double *phi, uint32_t *counts)
{
    if (!c) return BH_ERR_ARG;
    if (n_points < 0 || (n_points > 0 && !points) || (!accel && !phi && !counts))
        return fail(c, BH_ERR_ARG, "bh_field_at: n_points < 0, null points or no output array");
    if (int rc = diag_check(c, "bh_field_at")) return rc;
    if (int rc = points_finite(c, "bh_field_at", points, n_points)) return rc;
    if (n_points == 0) return BH_OK;
    if (c->n == 0) {                                           // no bodies: no field, no terms
        if (accel) std::fill(accel, accel + 2 * n_points, 0.0);
        if (phi) std::fill(phi, phi + n_points, 0.0);
        if (counts) std::fill(counts, counts + n_points, 0u);
        return BH_OK;
    }
    BH_HIP(c, hipSetDevice(c->device));
    if (int rc = field_alloc(c, std::min(n_points, kFieldChunk))) return rc;
    int rc = quietly(c, kQuietCounters, [&] { return enqueue_build(c, false); });
    if (!rc) rc = check_overflow(c);
    if (rc) return rc;
    const FieldState &s = c->field;
    for (int64_t t0 = 0; t0 < n_points; t0 += kFieldChunk) {
        const int64_t k = std::min(kFieldChunk, n_points - t0);
        if ((rc = enqueue_field(c, points + 2 * t0, k))) return rc;
        if (accel) BH_HIP(c, hipMemcpyAsync(accel + 2 * t0, s.accel, (size_t)k * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
        if (phi) BH_HIP(c, hipMemcpyAsync(phi + t0, s.phi, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (counts) BH_HIP(c, hipMemcpyAsync(counts + t0, s.counts, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        BH_HIP(c, hipStreamSynchronize(c->stream));
    }
    return BH_OK;
}

int bh_neighbours(bh_ctx *c, const double *points, int64_t n_points, int32_t k, int64_t *idx, double *d2, uint32_t *evals)
{
    if (!c) return BH_ERR_ARG;
    if (k < 1 || k > kNbMaxK) return fail(c, BH_ERR_ARG, "bh_neighbours: k must be 1 .. BH_NEIGHBOURS_MAX_K = 32");
    if (n_points < 0) return fail(c, BH_ERR_ARG, "bh_neighbours: n_points < 0");
    if (!idx && !d2) return fail(c, BH_ERR_ARG, "bh_neighbours: no output array (idx and d2 are both null)");
    return nb_query(c, "bh_neighbours", points, n_points, k, 0.0, idx, d2, evals);
}

int bh_count_within(bh_ctx *c, const double *points, int64_t n_points, double radius, uint32_t *counts)
{
    if (!c) return BH_ERR_ARG;
    if (!(radius >= 0.0) || !std::isfinite(radius)) return fail(c, BH_ERR_ARG, "bh_count_within: the radius must be finite and >= 0");
    if (n_points < 0) return fail(c, BH_ERR_ARG, "bh_count_within: n_points < 0");
    if (!counts) return fail(c, BH_ERR_ARG, "bh_count_within: null counts");
    return nb_query(c, "bh_count_within", points, n_points, 0, radius * radius, nullptr, nullptr, counts);
}

int bh_neighbours_times(bh_ctx *c, double *build_ms, double *query_ms)
{
    if (!c || !build_ms || !query_ms) return fail(c, BH_ERR_ARG, "bh_neighbours_times: null argument");
    *build_ms = c->nb.build_ms;
    *query_ms = c->nb.query_ms;
    return BH_OK;
}

// ---- pair counts (bh_pairs.hpp) on the structure of the neighbour queries.  They read pos as it lies in memory and write buffers
// of their own: a step before and after runs bit for bit as it would have.  Allowed in LET mode and with world > 1: the
// bodies are this context's own.
int bh_pair_counts(bh_ctx *c, const double *points, int64_t n_points, const double *edges, int32_t nb, int64_t *counts, int64_t *evals)
{
    if (!c) return BH_ERR_ARG;
    if (nb < 1 || nb > kPairMaxBins) return fail(c, BH_ERR_ARG, "bh_pair_counts: 1 .. BH_PAIR_MAX_BINS = 1024 bins");
    if (!edges || !counts) return fail(c, BH_ERR_ARG, "bh_pair_counts: null edges or counts");
    if (n_points < 0) return fail(c, BH_ERR_ARG, "bh_pair_counts: n_points < 0");
    std::vector<double> e2;
    if (const unsigned why = squared_edges(edges, nb, kPairMaxBins, e2)) {
        if (why & (kEdgeNotFinite | kEdgeNegative | kEdgeNotAscending))
            return fail(c, BH_ERR_ARG, "bh_pair_counts: the edges must be finite, >= 0 and strictly ascending");
        return fail(c, BH_ERR_ARG, "bh_pair_counts: the squared edges must be finite and strictly ascending");
    }
    if (int rc = need_upload(c, "bh_pair_counts before bh_upload/bh_initialize")) return rc;
    const int64_t n = c->n;
    if (!points && n_points != n) return fail(c, BH_ERR_ARG, "bh_pair_counts: without points, n_points must be the number of bodies");
    if (int rc = points_finite(c, "bh_pair_counts", points, n_points)) return rc;
    if (n > kNbMaxBodies) return fail(c, BH_ERR_CAPACITY, "bh_pair_counts: more than 2^24 bodies (their indices share a key word)");
    std::fill(counts, counts + nb + 2, (int64_t)0);
    if (evals) *evals = 0;
    NbState &s = c->nb;
    PairState &pr = c->pair;
    pr.build_ms = pr.query_ms = 0.0;
    if (n == 0 || n_points == 0) return BH_OK;
    BH_HIP(c, hipSetDevice(c->device));
    if (int rc = nb_alloc(c, n, points ? std::min(n_points, kNbChunk) : 0, 0)) return rc;
    if (!pr.e2) { if (int rc = alloc_all(c, {part(&pr.e2, (size_t)kPairMaxBins + 1), part(&pr.hist, (size_t)kPairMaxBins + 3)})) return rc; }
    int levels = 0;
    if (int rc = nb_build(c, "bh_pair_counts", &levels)) return rc;
    hipStream_t st = c->stream;
    const size_t words = (size_t)nb + 3;                       // the bins, then the evals word
    BH_HIP(c, hipMemcpyAsync(pr.e2, e2.data(), e2.size() * sizeof(double), hipMemcpyHostToDevice, st));
    BH_HIP(c, hipMemsetAsync(pr.hist, 0, words * sizeof(unsigned long long), st));
    const size_t lds = (2 * (size_t)nb + 4) * sizeof(unsigned long long);
    for (int64_t t0 = 0; t0 < n_points; t0 += kNbChunk) {
        const int64_t rows = std::min(kNbChunk, n_points - t0);
        auto search = [&](auto pts) {
            hipLaunchKernelGGL((pair_count_kernel<decltype(pts)::value>), dim3(blocks_for(rows, kBlock)), dim3(kBlock), lds, st, s.spos,
                               s.boxes, s.off, levels, (int32_t)n, s.points, s.order, t0, rows, pr.e2, nb, pr.hist, pr.hist + nb + 2);
        };
        if (int rc = nb_launch(c, points ? points + 2 * t0 : nullptr, rows, [&] { dispatch(search, points != nullptr); })) return rc;
        BH_HIP(c, hipStreamSynchronize(st));                    // (the next chunk overwrites the points; the events are read here)
        if (int rc = span_ms(c, s.ev[2], s.ev[3], &pr.query_ms, true)) return rc;
    }
    std::vector<unsigned long long> got(words);
    BH_HIP(c, hipMemcpyAsync(got.data(), pr.hist, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    BH_HIP(c, hipStreamSynchronize(st));
    for (int32_t k = 0; k < nb + 2; ++k) counts[k] = (int64_t)got[(size_t)k];
    if (evals) *evals = (int64_t)got[(size_t)nb + 2];
    return span_ms(c, s.ev[0], s.ev[1], &pr.build_ms);
}

int bh_pair_counts_times(bh_ctx *c, double *build_ms, double *query_ms)
{
    if (!c || !build_ms || !query_ms) return fail(c, BH_ERR_ARG, "bh_pair_counts_times: null argument");
    *build_ms = c->pair.build_ms;
    *query_ms = c->pair.query_ms;
    return BH_OK;
}

int bh_groups(bh_ctx *c, double linking_length, int64_t min_members, int64_t *label, int64_t *n_groups, int64_t *n_catalogue,
              uint64_t *stats)
{
    if (!c) return BH_ERR_ARG;
    if (!(linking_length >= 0.0) || !std::isfinite(linking_length))
        return fail(c, BH_ERR_ARG, "bh_groups: the linking length must be finite and >= 0");
    if (min_members < 1) return fail(c, BH_ERR_ARG, "bh_groups: min_members must be at least 1");
    if (!n_groups) return fail(c, BH_ERR_ARG, "bh_groups: null n_groups");
    if (int rc = diag_check(c, "bh_groups")) return rc;
    const int64_t n = c->n;
    if (n > kNbMaxBodies) return fail(c, BH_ERR_CAPACITY, "bh_groups: more than 2^24 bodies (their indices share a key word)");
    NbState &nb = c->nb;
    FofState &s = c->fof;
    s.cat_labels.clear(); s.cat_counts.clear(); s.cat_sums.clear();
    std::fill(s.cat_exp, s.cat_exp + kGrpPlanes, 0);
    s.build_ms = s.link_ms = s.cat_ms = 0.0;
    *n_groups = 0;
    if (n_catalogue) *n_catalogue = 0;
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (n == 0) return BH_OK;
    const double b2 = linking_length * linking_length;
    BH_HIP(c, hipSetDevice(c->device));
    if (int rc = nb_alloc(c, n, 0, 0)) return rc;
    if (int rc = fof_alloc(c, n)) return rc;
    int levels = 0;
    if (int rc = nb_build(c, "bh_groups", &levels)) return rc;
    hipStream_t st = c->stream;
    const unsigned grid = blocks_for(n, kBlock);
    const int32_t n32 = (int32_t)n;
    const uint32_t least = (uint32_t)std::min<int64_t>(min_members, (int64_t)UINT32_MAX);
    BH_HIP(c, hipMemsetAsync(s.ctr, 0, sizeof(GrpCounters), st));
    BH_HIP(c, hipMemsetAsync(s.minidx, 0xff, (size_t)n * sizeof(uint32_t), st));
    BH_HIP(c, hipMemsetAsync(s.count, 0, (size_t)n * sizeof(uint32_t), st));
    hipLaunchKernelGGL(grp_init_kernel, dim3(grid), dim3(kBlock), 0, st, nb.boxes, nb.off, levels, n32, b2, s.parent, s.ctr);
    hipLaunchKernelGGL(grp_link_kernel, dim3(grid), dim3(kBlock), 0, st, nb.spos, nb.boxes, nb.off, levels, n32, b2, s.parent, s.ctr);
    hipLaunchKernelGGL(grp_flatten_kernel, dim3(grid), dim3(kBlock), 0, st, s.parent, nb.sidx, n32, s.root, s.minidx, s.count, s.ctr);
    hipLaunchKernelGGL(grp_label_kernel, dim3(grid), dim3(kBlock), 0, st, s.root, s.minidx, nb.sidx, n32, s.label);
    BH_HIP(c, hipGetLastError());
    if (int rc = mark(c, s.ev[0])) return rc;
    GrpExp ex{};
    GrpCounters ctr{};
    if (n_catalogue) {
        BH_HIP(c, hipMemsetAsync(s.max, 0, sizeof(GrpMax), st));
        state_ptrs(c, [&](auto pos, auto vel, auto mass) {
            hipLaunchKernelGGL((grp_max_kernel<Pointee<decltype(pos)>, Pointee<decltype(mass)>>), dim3(grid), dim3(kBlock), 0, st, pos, vel,
                               mass, n, s.max);
        });
        // (gid: the parents are not read any more)
        hipLaunchKernelGGL(grp_compact_kernel, dim3(grid), dim3(kBlock), 0, st, s.root, s.minidx, s.count, n32, least, s.parent,
                           s.rec_label, s.rec_count, s.ctr);
        BH_HIP(c, hipGetLastError());
        GrpMax mx{};
        double m[kGrpPlanes];
        if (int rc = read_maxima(c, s.max, &mx, m, &ctr, s.ctr, sizeof(ctr))) return rc;
        if (mx.bad)
            return fail(c, BH_ERR_ARG, "bh_groups: a body has a non-finite velocity or mass (or a moment m x, m v that overflows fp64)");
        const int L = log2_ceil(n);
        for (int p = 0; p < kGrpPlanes; ++p) ex.e[p] = plane_exponent(m[p], L);
    } else {
        BH_HIP(c, hipMemcpyAsync(&ctr, s.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipStreamSynchronize(st));
    }
    const int64_t kept = (int64_t)ctr.kept;
    if (n_catalogue && kept > 0) {
        BH_HIP(c, hipMemsetAsync(s.sums, 0, (size_t)kept * kGrpPlanes * sizeof(unsigned long long), st));
        state_ptrs(c, [&](auto pos, auto vel, auto mass) {
            hipLaunchKernelGGL((grp_sum_kernel<Pointee<decltype(pos)>, Pointee<decltype(mass)>>), dim3(grid), dim3(kBlock), 0, st, pos, vel,
                               mass, nb.slot, s.root, s.count, s.parent, n32, least, ex, s.sums);
        });
        BH_HIP(c, hipGetLastError());
    }
    if (int rc = mark(c, s.ev[1])) return rc;
    std::vector<uint32_t> rl((size_t)kept), rc_((size_t)kept);
    std::vector<int64_t> sums((size_t)kept * kGrpPlanes);
    if (kept > 0) {
        BH_HIP(c, hipMemcpyAsync(rl.data(), s.rec_label, (size_t)kept * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipMemcpyAsync(rc_.data(), s.rec_count, (size_t)kept * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipMemcpyAsync(sums.data(), s.sums, sums.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    if (label) BH_HIP(c, hipMemcpyAsync(label, s.label, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    BH_HIP(c, hipStreamSynchronize(st));
    if (int rc = span_ms(c, nb.ev[0], nb.ev[1], &s.build_ms)) return rc;
    if (int rc = span_ms(c, nb.ev[1], s.ev[0], &s.link_ms)) return rc;
    if (int rc = span_ms(c, s.ev[0], s.ev[1], &s.cat_ms)) return rc;
    catalogue_order(rl.data(), rc_.data(), sums.data(), kept, kGrpPlanes, s.cat_labels, s.cat_counts, s.cat_sums);
    std::copy(ex.e, ex.e + kGrpPlanes, s.cat_exp);
    *n_groups = (int64_t)ctr.roots;
    if (n_catalogue) *n_catalogue = kept;
    if (stats) { stats[0] = ctr.evals; stats[1] = ctr.pairs; stats[2] = ctr.hooks; }
    return BH_OK;
}

int bh_groups_catalogue(bh_ctx *c, int64_t max_records, int64_t *labels, int64_t *counts, int64_t *sums, int32_t *exponents,
                        int64_t *n_out)
{
    if (!c) return BH_ERR_ARG;
    if (!n_out || max_records < 0) return fail(c, BH_ERR_ARG, "bh_groups_catalogue: null n_out or max_records < 0");
    const FofState &s = c->fof;
    const int64_t g = (int64_t)s.cat_labels.size();
    *n_out = g;
    if (exponents) std::copy(s.cat_exp, s.cat_exp + kGrpPlanes, exponents);
    if (g > max_records) return fail(c, BH_ERR_CAPACITY, "bh_groups_catalogue: the catalogue has " + std::to_string(g) + " records");
    if (labels) std::copy(s.cat_labels.begin(), s.cat_labels.end(), labels);
    if (counts) std::copy(s.cat_counts.begin(), s.cat_counts.end(), counts);
    if (sums) std::copy(s.cat_sums.begin(), s.cat_sums.end(), sums);
    return BH_OK;
}

int bh_groups_times(bh_ctx *c, double *build_ms, double *link_ms, double *catalogue_ms)
{
    if (!c || !build_ms || !link_ms || !catalogue_ms) return fail(c, BH_ERR_ARG, "bh_groups_times: null argument");
    *build_ms = c->fof.build_ms;
    *link_ms = c->fof.link_ms;
    *catalogue_ms = c->fof.cat_ms;
    return BH_OK;
}

int bh_spanning_tree(bh_ctx *c, int64_t *lo, int64_t *hi, double *d2, uint64_t *stats)
{
    if (!c) return BH_ERR_ARG;
    if (!lo || !hi || !d2) return fail(c, BH_ERR_ARG, "bh_spanning_tree: null output");
    if (int rc = diag_check(c, "bh_spanning_tree")) return rc;
    const int64_t n = c->n;
    if (n > kNbMaxBodies) return fail(c, BH_ERR_CAPACITY, "bh_spanning_tree: more than 2^24 bodies (their indices share a key word)");
    NbState &nb = c->nb;
    MstState &s = c->mst;
    s.build_ms = s.rounds_ms = s.sort_ms = 0.0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return BH_OK;
    BH_HIP(c, hipSetDevice(c->device));
    if (int rc = nb_alloc(c, n, 0, 0)) return rc;
    if (int rc = mst_alloc(c, n)) return rc;
    int levels = 0;
    if (int rc = nb_build(c, "bh_spanning_tree", &levels)) return rc;
    hipStream_t st = c->stream;
    const unsigned grid = blocks_for(n, kBlock);
    const int32_t n32 = (int32_t)n;
    int32_t off[kNbMaxLevels + 1];
    nb_levels(n, off);
    BH_HIP(c, hipMemsetAsync(s.ctr, 0, sizeof(MstCounters), st));
    hipLaunchKernelGGL(mst_init_kernel, dim3(grid), dim3(kBlock), 0, st, nb.sidx, n32, s.parent, s.comp, s.inv, s.seedmin, s.mind2,
                       s.minpair);
    // The rounds: the components at least halve in each, so kMstMaxRounds are never reached; a round that joins nothing ends the
    // call as well.  One word comes back per round.
    unsigned long long left = (unsigned long long)n;
    int rounds = 0;
    while (left > 1) {
        if (rounds == kMstMaxRounds)
            return fail(c, BH_ERR_DEVICE, "bh_spanning_tree: " + std::to_string(left) + " components left after " +
                                          std::to_string(rounds) + " rounds");
        for (int l = 0; l < levels; ++l) {
            const int32_t count = off[l + 1] - off[l], below = l ? off[l] - off[l - 1] : 0;
            hipLaunchKernelGGL(mst_nodecomp_kernel, dim3(blocks_for(count, kBlock)), dim3(kBlock), 0, st, s.comp,
                               s.nodecomp + (l ? off[l - 1] : 0), l, below, n32, count, s.nodecomp + off[l]);
        }
        hipLaunchKernelGGL(mst_seed_kernel, dim3(grid), dim3(kBlock), 0, st, nb.spos, nb.sidx, s.comp, n32, s.seedmin, s.cand_d2,
                           s.cand_pair, s.ctr);
        hipLaunchKernelGGL(mst_nearest_kernel, dim3(grid), dim3(kBlock), 0, st, nb.spos, nb.sidx, s.comp, s.nodecomp, nb.boxes, nb.off,
                           levels, n32, s.seedmin, s.mind2, s.cand_d2, s.cand_pair, s.ctr);
        hipLaunchKernelGGL(mst_pick_kernel, dim3(grid), dim3(kBlock), 0, st, s.comp, s.mind2, s.cand_d2, s.cand_pair, n32, s.minpair);
        hipLaunchKernelGGL(mst_hook_kernel, dim3(grid), dim3(kBlock), 0, st, s.comp, s.inv, s.mind2, s.minpair, n32, s.parent,
                           s.edge_pair, s.edge_d2, s.ctr);
        hipLaunchKernelGGL(mst_flatten_kernel, dim3(grid), dim3(kBlock), 0, st, s.parent, n32, s.comp, s.seedmin, s.mind2,
                           s.minpair,
                           &s.ctr->roots[rounds]);
        BH_HIP(c, hipGetLastError());
        unsigned long long got = 0;
        BH_HIP(c, hipMemcpyAsync(&got, &s.ctr->roots[rounds], sizeof(got), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipStreamSynchronize(st));
        ++rounds;
        if (got < 1 || got >= left)
            return fail(c, BH_ERR_DEVICE, "bh_spanning_tree: round " + std::to_string(rounds) + " left " + std::to_string(got) +
                                          " of " + std::to_string(left) + " components");
        left = got;
    }
    BH_HIP(c, hipGetLastError());
    if (int rc = mark(c, s.ev[0])) return rc;
    // The final order, timed on its own: the records by the bits of d2 on the device -- the stable LSD passes over all 64 bits,
    // an edge's place in the append order as the payload; the union-find and the candidates are not read any more and lend
    // their arrays, the index its count matrix --, the pairs gathered into that order, then the host sorts the runs of equal d2.
    const size_t edges = (size_t)(n - 1);
    uint64_t *const keys[2] = {reinterpret_cast<uint64_t *>(s.edge_d2), reinterpret_cast<uint64_t *>(s.cand_d2)};
    uint32_t *const vals[2] = {s.parent, s.comp};
    int cur = 0;
    if (edges) {
        static_assert(kSortItems >= kFieldSortItems, "the index's count matrix holds this sort's tiles");
        hipLaunchKernelGGL(mst_iota_kernel, dim3(blocks_for((int64_t)edges, kBlock)), dim3(kBlock), 0, st, (int32_t)edges, vals[0]);
        cur = enqueue_lsd_passes<kSortItems>(st, keys, vals, nb.radix, nb.rowsum, (int64_t)edges, 64, false);
        hipLaunchKernelGGL(mst_gather_kernel, dim3(blocks_for((int64_t)edges, kBlock)), dim3(kBlock), 0, st, vals[cur], s.edge_pair,
                           (int32_t)edges, s.minpair);
        BH_HIP(c, hipGetLastError());
    }
    if (int rc = mark(c, s.ev[1])) return rc;
    MstCounters ctr{};
    std::vector<uint64_t> pr(edges);
    BH_HIP(c, hipMemcpyAsync(&ctr, s.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    if (edges) {
        BH_HIP(c, hipMemcpyAsync(pr.data(), s.minpair, edges * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipMemcpyAsync(d2, keys[cur], edges * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    BH_HIP(c, hipStreamSynchronize(st));
    if (int rc = span_ms(c, nb.ev[0], nb.ev[1], &s.build_ms)) return rc;
    if (int rc = span_ms(c, nb.ev[1], s.ev[0], &s.rounds_ms)) return rc;
    if (int rc = span_ms(c, s.ev[0], s.ev[1], &s.sort_ms)) return rc;
    if (ctr.edges != (unsigned long long)edges)
        return fail(c, BH_ERR_DEVICE, "bh_spanning_tree: " + std::to_string(ctr.edges) + " edges for " + std::to_string(n) + " bodies");
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < edges;) {
        size_t end = k + 1;
        while (end < edges && d2[end] == d2[k]) ++end;                 // (d2 >= +0 and never NaN: equal values, equal bits)
        if (end - k > 1) std::sort(pr.begin() + (std::ptrdiff_t)k, pr.begin() + (std::ptrdiff_t)end);
        k = end;
    }
    for (size_t k = 0; k < edges; ++k) {
        lo[k] = (int64_t)(pr[k] >> 24);
        hi[k] = (int64_t)(pr[k] & 0xffffffull);
    }
    s.sort_ms += ms_since(t0);
    if (stats) { stats[0] = (uint64_t)rounds; stats[1] = ctr.evals; stats[2] = ctr.skips; stats[3] = ctr.edges; }
    return BH_OK;
}

int bh_spanning_tree_subsets(bh_ctx *c, const int64_t *members, int64_t n_sets, int32_t k, int64_t *lo, int64_t *hi, double *d2)
{
    if (!c) return BH_ERR_ARG;
    if (k < 2 || k > kMstSubsetMax) return fail(c, BH_ERR_ARG, "bh_spanning_tree_subsets: k must be 2 .. BH_MST_SUBSET_MAX = 512");
    if (n_sets < 0) return fail(c, BH_ERR_ARG, "bh_spanning_tree_subsets: n_sets < 0");
    if (n_sets > 0 && (!members || !lo || !hi || !d2)) return fail(c, BH_ERR_ARG, "bh_spanning_tree_subsets: null argument");
    if (int rc = diag_check(c, "bh_spanning_tree_subsets")) return rc;
    const int64_t n = c->n;
    if (n > kNbMaxBodies)
        return fail(c, BH_ERR_CAPACITY, "bh_spanning_tree_subsets: more than 2^24 bodies (the two indices of an edge share a word)");
    MstState &s = c->mst;
    s.build_ms = s.rounds_ms = s.sort_ms = 0.0;
    // every index inside [0, n) and no index twice in a row, before anything is enqueued
    std::vector<int64_t> seen((size_t)n, (int64_t)-1);
    for (int64_t r = 0; r < n_sets; ++r)
        for (int32_t t = 0; t < k; ++t) {
            const int64_t m = members[r * k + t];
            if (m < 0 || m >= n)
                return fail(c, BH_ERR_ARG, "bh_spanning_tree_subsets: set " + std::to_string(r) + " has index " + std::to_string(m) + " outside [0, n)");
            if (seen[(size_t)m] == r)
                return fail(c, BH_ERR_ARG, "bh_spanning_tree_subsets: set " + std::to_string(r) + " has index " + std::to_string(m) + " twice");
            seen[(size_t)m] = r;
        }
    if (n_sets == 0) return BH_OK;
    BH_HIP(c, hipSetDevice(c->device));
    const int64_t per = std::max<int64_t>(1, ((int64_t)1 << 22) / k);             // sets per launch
    const int64_t want = std::min(n_sets, per) * k;
    if (want > s.sblock.cap) {
        const size_t b = (size_t)grown_capacity(want);
        if (int rc = block_regrow(c, s.sblock, (int64_t)b, {part(&s.members, b), part(&s.set_pair, b), part(&s.set_d2, b), part(&s.bad, 1)}))
            return rc;
    }
    hipStream_t st = c->stream;
    const uint32_t *slot_of = nullptr;
    if (!c->tree64() && !c->is.orig_identity) {            // (fp32 / mixed after a physical re-order: slots are not caller indices)
        if (!c->slot_of) { if (int rc = dev_alloc(c, &c->slot_of, (size_t)std::max<int64_t>(c->cfg.capacity, 1))) return rc; }
        hipLaunchKernelGGL(direct_slot_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, st, c->orig, n, c->slot_of);
        slot_of = c->slot_of;
    }
    BH_HIP(c, hipMemsetAsync(s.bad, 0, sizeof(uint32_t), st));
    const int64_t row = k - 1;
    std::vector<MstEdge> e((size_t)(n_sets * row));
    std::vector<uint64_t> pr((size_t)(std::min(n_sets, per) * row)), dd(pr.size());
    for (int64_t r0 = 0; r0 < n_sets; r0 += per) {
        const int64_t sets = std::min(per, n_sets - r0);
        BH_HIP(c, hipMemcpyAsync(s.members, members + r0 * k, (size_t)(sets * k) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (int rc = mark(c, s.ev[0])) return rc;
        state_ptrs(c, [&](auto pos, auto, auto) {
            hipLaunchKernelGGL((mst_subset_kernel<Pointee<decltype(pos)>>), dim3((unsigned)sets), dim3(kWave), (size_t)k * 36, st, pos,
                               slot_of, s.members, k, s.set_pair, s.set_d2, s.bad);
        });
        BH_HIP(c, hipGetLastError());
        if (int rc = mark(c, s.ev[1])) return rc;
        BH_HIP(c, hipMemcpyAsync(pr.data(), s.set_pair, (size_t)(sets * row) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipMemcpyAsync(dd.data(), s.set_d2, (size_t)(sets * row) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipStreamSynchronize(st));                    // (the next launch overwrites the members)
        if (int rc = span_ms(c, s.ev[0], s.ev[1], &s.rounds_ms, true)) return rc;
        for (int64_t i = 0; i < sets * row; ++i) e[(size_t)(r0 * row + i)] = MstEdge{dd[(size_t)i], pr[(size_t)i]};
    }
    uint32_t bad = 0;
    BH_HIP(c, hipMemcpy(&bad, s.bad, sizeof(bad), hipMemcpyDeviceToHost));
    if (bad) return fail(c, BH_ERR_ARG, "bh_spanning_tree_subsets: a member has a non-finite position");
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t r = 0; r < n_sets; ++r) mst_sorted_out(e.data() + r * row, row, lo + r * row, hi + r * row, d2 + r * row);
    s.sort_ms = ms_since(t0);
    return BH_OK;
}

int bh_spanning_tree_times(bh_ctx *c, double *build_ms, double *rounds_ms, double *sort_ms)
{
    if (!c || !build_ms || !rounds_ms || !sort_ms) return fail(c, BH_ERR_ARG, "bh_spanning_tree_times: null argument");
    *build_ms = c->mst.build_ms;
    *rounds_ms = c->mst.rounds_ms;
    *sort_ms = c->mst.sort_ms;
    return BH_OK;
}

int bh_binaries(bh_ctx *c, double max_separation, int64_t *partner, double *eps, int64_t *n_pairs, uint64_t *stats)
{
    if (!c) return BH_ERR_ARG;
    if (!(max_separation > 0.0)) return fail(c, BH_ERR_ARG, "bh_binaries: max_separation must be > 0 (+inf: no cut) and not NaN");
    if (!n_pairs) return fail(c, BH_ERR_ARG, "bh_binaries: null n_pairs");
    if (int rc = diag_check(c, "bh_binaries")) return rc;
    if (!(c->cfg.G > 0.0)) return fail(c, BH_ERR_ARG, "bh_binaries: G must be > 0 (the energy bound of the search rests on it)");
    const int64_t n = c->n;
    if (n > kNbMaxBodies) return fail(c, BH_ERR_CAPACITY, "bh_binaries: more than 2^24 bodies (their indices share a key word)");
    NbState &nb = c->nb;
    BinState &s = c->bin;
    s.cat_lo.clear(); s.cat_hi.clear(); s.cat_rec.clear();
    s.build_ms = s.search_ms = s.cat_ms = 0.0;
    *n_pairs = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return BH_OK;
    const double R2 = max_separation * max_separation;
    BH_HIP(c, hipSetDevice(c->device));
    if (int rc = nb_alloc(c, n, 0, 0)) return rc;
    if (int rc = bin_alloc(c, n)) return rc;
    int levels = 0;
    if (int rc = nb_build(c, "bh_binaries", &levels)) return rc;
    hipStream_t st = c->stream;
    const unsigned grid = blocks_for(n, kBlock);
    const int32_t n32 = (int32_t)n;
    const int64_t room = s.block.cap / 2 + 1;
    int32_t off[kNbMaxLevels + 1];
    nb_levels(n, off);
    BH_HIP(c, hipMemsetAsync(s.ctr, 0, sizeof(BinCounters), st));
    state_ptrs(c, [&](auto, auto vel, auto mass) {
        hipLaunchKernelGGL((bin_gather_kernel<Pointee<decltype(vel)>, Pointee<decltype(mass)>>), dim3(grid), dim3(kBlock), 0, st, vel, mass,
                           nb.slot, n, s.svel, s.smass);
    });
    for (int l = 0; l < levels; ++l) {
        const int32_t count = off[l + 1] - off[l], below = l ? off[l] - off[l - 1] : 0;
        hipLaunchKernelGGL(bin_nodemass_kernel, dim3(blocks_for(count, kBlock)), dim3(kBlock), 0, st, s.smass,
                           s.nodemass + (l ? off[l - 1] : 0), l, below, n32, count, s.nodemass + off[l]);
    }
    BH_HIP(c, hipGetLastError());
    if (int rc = mark(c, s.ev[0])) return rc;
    hipLaunchKernelGGL(bin_search_kernel, dim3(grid), dim3(kBlock), 0, st, nb.spos, s.svel, s.smass, nb.sidx, s.nodemass, nb.boxes, nb.off,
                       levels, n32, R2, c->cfg.G, s.partner, s.eps, s.psort, s.ctr);
    BH_HIP(c, hipGetLastError());
    if (int rc = mark(c, s.ev[1])) return rc;
    hipLaunchKernelGGL(bin_pairs_kernel, dim3(grid), dim3(kBlock), 0, st, nb.spos, s.svel, s.smass, nb.sidx, s.psort, n32, c->cfg.G, room,
                       s.rec_lo, s.rec_hi, s.rec, s.ctr);
    BH_HIP(c, hipGetLastError());
    if (int rc = mark(c, s.ev[2])) return rc;
    BinCounters ctr{};
    BH_HIP(c, hipMemcpyAsync(&ctr, s.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    if (partner) BH_HIP(c, hipMemcpyAsync(partner, s.partner, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (eps) BH_HIP(c, hipMemcpyAsync(eps, s.eps, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    BH_HIP(c, hipStreamSynchronize(st));
    if (int rc = span_ms(c, nb.ev[0], s.ev[0], &s.build_ms)) return rc;
    if (int rc = span_ms(c, s.ev[0], s.ev[1], &s.search_ms)) return rc;
    if (int rc = span_ms(c, s.ev[1], s.ev[2], &s.cat_ms)) return rc;
    const int64_t pairs = (int64_t)ctr.pairs;
    if (pairs > room || 2 * pairs > n)
        return fail(c, BH_ERR_DEVICE, "bh_binaries: " + std::to_string(pairs) + " mutual pairs for " + std::to_string(n) + " bodies");
    // the records as the atomics placed them; the catalogue is ascending in lo (a body is in one pair at most: no ties)
    std::vector<uint32_t> lo((size_t)pairs), hi((size_t)pairs);
    std::vector<double> rec((size_t)pairs * kBinRecord);
    if (pairs > 0) {
        BH_HIP(c, hipMemcpyAsync(lo.data(), s.rec_lo, (size_t)pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipMemcpyAsync(hi.data(), s.rec_hi, (size_t)pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipMemcpyAsync(rec.data(), s.rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipStreamSynchronize(st));
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> place((size_t)n, -1);                 // body -> its record where it is a lo: one pass over the bodies orders them
    for (int64_t k = 0; k < pairs; ++k) {
        if (lo[(size_t)k] >= (uint32_t)n || place[lo[(size_t)k]] >= 0)
            return fail(c, BH_ERR_DEVICE, "bh_binaries: record " + std::to_string(k) + " names body " + std::to_string(lo[(size_t)k]) +
                                          " a second time, or outside the state");
        place[lo[(size_t)k]] = (int32_t)k;
    }
    std::vector<int64_t> order;
    order.reserve((size_t)pairs);
    for (int64_t i = 0; i < n; ++i)
        if (place[(size_t)i] >= 0) order.push_back(place[(size_t)i]);
    s.cat_lo.resize((size_t)pairs); s.cat_hi.resize((size_t)pairs); s.cat_rec.resize(rec.size());
    for (int64_t k = 0; k < pairs; ++k) {
        const size_t g = (size_t)order[(size_t)k];
        s.cat_lo[(size_t)k] = (int64_t)lo[g];
        s.cat_hi[(size_t)k] = (int64_t)hi[g];
        std::copy(rec.begin() + (std::ptrdiff_t)(g * kBinRecord), rec.begin() + (std::ptrdiff_t)((g + 1) * kBinRecord),
                  s.cat_rec.begin() + (std::ptrdiff_t)((size_t)k * kBinRecord));
    }
    s.cat_ms += ms_since(t0);
    *n_pairs = pairs;
    if (stats) { stats[0] = ctr.evals; stats[1] = ctr.max_evals; stats[2] = ctr.opened; stats[3] = ctr.pairs; }
    return BH_OK;
}

int bh_binaries_catalogue(bh_ctx *c, int64_t max_records, int64_t *lo, int64_t *hi, double *records)
{
    if (!c) return BH_ERR_ARG;
    if (max_records < 0) return fail(c, BH_ERR_ARG, "bh_binaries_catalogue: max_records < 0");
    const BinState &s = c->bin;
    const int64_t g = (int64_t)s.cat_lo.size();
    if (g > max_records) return fail(c, BH_ERR_CAPACITY, "bh_binaries_catalogue: the catalogue has " + std::to_string(g) + " records");
    if (lo) std::copy(s.cat_lo.begin(), s.cat_lo.end(), lo);
    if (hi) std::copy(s.cat_hi.begin(), s.cat_hi.end(), hi);
    if (records) std::copy(s.cat_rec.begin(), s.cat_rec.end(), records);
    return BH_OK;
}

int bh_binaries_times(bh_ctx *c, double *build_ms, double *search_ms, double *catalogue_ms)
{
    if (!c || !build_ms || !search_ms || !catalogue_ms) return fail(c, BH_ERR_ARG, "bh_binaries_times: null argument");
    *build_ms = c->bin.build_ms;
    *search_ms = c->bin.search_ms;
    *catalogue_ms = c->bin.cat_ms;
    return BH_OK;
}

int bh_neighbour_lists(bh_ctx *c, const double *points, int64_t n_points, const double *radii, int64_t n_radii, int64_t max_entries,
                       int64_t *offsets, int64_t *idx, double *d2, int64_t *n_entries, uint64_t *stats)
{
    if (!c) return BH_ERR_ARG;
    const std::string w("bh_neighbour_lists");
    if (!offsets || !n_entries || !radii) return fail(c, BH_ERR_ARG, w + ": null offsets, n_entries or radii");
    if (n_points < 0) return fail(c, BH_ERR_ARG, w + ": n_points < 0");
    if (n_radii != 1 && n_radii != n_points) return fail(c, BH_ERR_ARG, w + ": n_radii must be 1 or n_points");
    if ((idx == nullptr) != (d2 == nullptr)) return fail(c, BH_ERR_ARG, w + ": idx and d2 come together or not at all");
    if (max_entries < 0) return fail(c, BH_ERR_ARG, w + ": max_entries < 0");
    for (int64_t i = 0; i < n_radii; ++i)
        if (!(radii[i] >= 0.0) || !std::isfinite(radii[i]))
            return fail(c, BH_ERR_ARG, w + ": radius " + std::to_string(i) + " must be finite and >= 0");
    if (int rc = diag_check(c, "bh_neighbour_lists")) return rc;
    const int64_t n = c->n;
    if (!points && n_points != n) return fail(c, BH_ERR_ARG, w + ": without points, n_points must be the number of bodies");
    if (int rc = points_finite(c, "bh_neighbour_lists", points, n_points)) return rc;
    NbState &nb = c->nb;
    NblState &s = c->nbl;
    std::fill(offsets, offsets + n_points + 1, (int64_t)0);
    *n_entries = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    s.build_ms = s.count_ms = s.fill_ms = s.sort_ms = 0.0;
    s.evals_host.assign((size_t)n_points, 0u);
    if (n_points == 0) return BH_OK;
    if (n > kNbMaxBodies) return fail(c, BH_ERR_CAPACITY, w + ": more than 2^24 bodies (their indices share a key word)");
    if (n == 0) return BH_OK;                                  // no bodies: every row is empty

    // the squared radii, each product formed once in fp64
    const bool each = n_radii != 1;                            // (one query with its one radius: the same thing)
    const double r2_all = radii[0] * radii[0];
    std::vector<double> r2host(each ? (size_t)n_points : 0);
    for (size_t i = 0; i < r2host.size(); ++i) r2host[i] = radii[i] * radii[i];

    BH_HIP(c, hipSetDevice(c->device));
    const int64_t rows_max = std::min(n_points, kNbChunk);
    if (int rc = nb_alloc(c, n, points ? rows_max : 0, 0)) return rc;
    if (int rc = nbl_alloc(c, (each && !points) ? std::max(rows_max, n) : rows_max, 0, false)) return rc;
    int levels = 0;
    if (int rc = nb_build(c, "bh_neighbour_lists", &levels)) return rc;
    hipStream_t st = c->stream;
    const int32_t n32 = (int32_t)n;
    const bool many = n_points > kNbChunk;                     // more than one chunk: a chunk's order and counts are made again to fill it

    // ---- the count pass: row lengths in launch order, and where every launch row belongs
    std::vector<uint32_t> hcount((size_t)n_points), hdest((size_t)n_points);
    if (!points) BH_HIP(c, hipMemcpyAsync(hdest.data(), nb.sidx, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (each && !points) BH_HIP(c, hipMemcpyAsync(s.rad2, r2host.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    const double *rad2 = each ? s.rad2 : nullptr;
    auto chunk_radii = [&](int64_t t0, int64_t rows) -> int {
        if (!each || !points) return BH_OK;
        BH_HIP(c, hipMemcpyAsync(s.rad2, r2host.data() + t0, (size_t)rows * sizeof(double), hipMemcpyHostToDevice, st));
        return BH_OK;
    };
    for (int64_t t0 = 0; t0 < n_points; t0 += kNbChunk) {
        const int64_t rows = std::min(kNbChunk, n_points - t0);
        if (int rc = chunk_radii(t0, rows)) return rc;
        auto search = [&](auto pts) {
            hipLaunchKernelGGL((nbl_count_kernel<decltype(pts)::value>), dim3(blocks_for(rows, kBlock)), dim3(kBlock), 0, st, nb.spos, nb.sidx,
                               nb.boxes, nb.off, levels, n32, nb.points, nb.order, t0, rows, rad2, r2_all, s.counts);
        };
        if (int rc = nb_launch(c, points ? points + 2 * t0 : nullptr, rows, [&] { dispatch(search, points != nullptr); })) return rc;
        BH_HIP(c, hipMemcpyAsync(hcount.data() + t0, s.counts, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (points) BH_HIP(c, hipMemcpyAsync(hdest.data() + t0, nb.order, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        BH_HIP(c, hipStreamSynchronize(st));
        if (int rc = span_ms(c, nb.ev[2], nb.ev[3], &s.count_ms, true)) return rc;
        if (points) for (int64_t r = 0; r < rows; ++r) hdest[(size_t)(t0 + r)] += (uint32_t)t0;
    }
    if (int rc = span_ms(c, nb.ev[0], nb.ev[1], &s.build_ms)) return rc;
    int64_t longest = 0;
    for (int64_t g = 0; g < n_points; ++g) {
        offsets[(int64_t)hdest[(size_t)g] + 1] = (int64_t)hcount[(size_t)g];
        longest = std::max<int64_t>(longest, hcount[(size_t)g]);
    }
    for (int64_t r = 0; r < n_points; ++r) offsets[r + 1] += offsets[r];
    const int64_t total = offsets[n_points];
    *n_entries = total;
    if (stats) { stats[2] = (uint64_t)total; stats[3] = (uint64_t)longest; }
    if (!idx) return BH_OK;
    if (total > max_entries)
        return fail(c, BH_ERR_CAPACITY, w + ": the lists hold " + std::to_string(total) + " entries, max_entries is " + std::to_string(max_entries));

    // ---- the fill pass, launch by launch: consecutive rows whose lengths sum to at most the budget (at least the longest row)
    const int64_t budget = std::max(s.budget, longest), room = std::max<int64_t>(std::min(budget, total), 1);
    const int64_t lds_most = std::max<int64_t>(s.sort_lds, kNblSmall);
    if (int rc = nbl_alloc(c, 0, room, longest > lds_most)) return rc;
    std::vector<unsigned long long> hd2((size_t)room);
    std::vector<uint32_t> hidx((size_t)room), hev((size_t)rows_max), rows_lds[3], rows_merge;
    // (rows_lds: the in-LDS tier by length, up to 128, up to 256, longer: a network of T entries keeps T / 2 threads busy, so short
    // rows get workgroups of one or two waves)
    BH_HIP(c, hipMemsetAsync(s.ctr, 0, sizeof(NblCounters), st));
    for (int64_t t0 = 0; t0 < n_points; t0 += kNbChunk) {
        const int64_t rows = std::min(kNbChunk, n_points - t0);
        if (many) {
            if (int rc = chunk_radii(t0, rows)) return rc;
            if (points) { if (int rc = sorted_query_chunk(c, points + 2 * t0, rows, nb.points, nb.box, nb.pkeys, nb.order, nb.radix, nb.rowsum)) return rc; }
            BH_HIP(c, hipMemcpyAsync(s.counts, hcount.data() + t0, (size_t)rows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        for (int64_t a = 0, b = 0; a < rows; a = b) {
            int64_t sum = 0, small_most = 1, lds_len[3] = {0, 0, 0};
            for (auto &v : rows_lds) v.clear();
            rows_merge.clear();
            for (b = a; b < rows && sum + (int64_t)hcount[(size_t)(t0 + b)] <= budget; ++b) {
                const int64_t len = (int64_t)hcount[(size_t)(t0 + b)];
                sum += len;
                if (len <= kNblSmall) small_most = std::max(small_most, len);
                else if (len <= lds_most) {
                    const int g = len <= 2 * kWave ? 0 : len <= 4 * kWave ? 1 : 2;
                    rows_lds[g].push_back((uint32_t)(b - a));
                    lds_len[g] = std::max(lds_len[g], len);
                }
                else rows_merge.push_back((uint32_t)(b - a));
            }
            const int64_t nq = b - a;
            const unsigned nt = blocks_for(nq, kNblScanTile);
            if (int rc = mark(c, s.ev[0])) return rc;
            hipLaunchKernelGGL(nbl_scan_totals_kernel, dim3(nt), dim3(kBlock), 0, st, s.counts + a, nq, s.tiles);
            hipLaunchKernelGGL(nbl_scan_bases_kernel, dim3(1), dim3(kBlock), 0, st, s.tiles, (int32_t)nt);
            hipLaunchKernelGGL(nbl_scan_apply_kernel, dim3(nt), dim3(kBlock), 0, st, s.counts + a, nq, s.tiles, s.cursors);
            dispatch([&](auto pts) {
                hipLaunchKernelGGL((nbl_fill_kernel<decltype(pts)::value>), dim3(blocks_for(nq, kWave)), dim3(kWave),
                                   (size_t)small_most * kWave * 12, st, nb.spos, nb.sidx, nb.boxes, nb.off, levels, n32, (int32_t)small_most,
                                   nb.points, nb.order + (points ? a : 0), t0 + a, nq, rad2, r2_all, s.counts + a, s.cursors, s.ent_d2, s.ent_idx,
                                   s.evals, s.ctr);
            }, points != nullptr);
            BH_HIP(c, hipGetLastError());
            if (int rc = mark(c, s.ev[1])) return rc;
            size_t at = 0;
            for (int g = 0; g < 3; ++g) {
                if (rows_lds[g].empty()) continue;
                const int32_t T = pow2_at_least(lds_len[g]);
                BH_HIP(c, hipMemcpyAsync(s.rows_lds + at, rows_lds[g].data(), rows_lds[g].size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL((nbl_sort_kernel<false>), dim3((unsigned)rows_lds[g].size()), dim3(std::min(kBlock, std::max(kWave, T / 2))),
                                   (size_t)T * 12, st, s.rows_lds + at, s.counts + a, s.cursors, T, s.ent_d2, s.ent_idx, s.alt_d2, s.alt_idx);
                at += rows_lds[g].size();
            }
            if (!rows_merge.empty()) {
                const int32_t T = pow2_at_least(s.sort_lds);
                BH_HIP(c, hipMemcpyAsync(s.rows_merge, rows_merge.data(), rows_merge.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL((nbl_sort_kernel<true>), dim3((unsigned)rows_merge.size()), dim3(kBlock), (size_t)T * 12, st, s.rows_merge,
                                   s.counts + a, s.cursors, T, s.ent_d2, s.ent_idx, s.alt_d2, s.alt_idx);
            }
            BH_HIP(c, hipGetLastError());
            if (int rc = mark(c, s.ev[2])) return rc;
            if (sum > 0) {
                BH_HIP(c, hipMemcpyAsync(hd2.data(), s.ent_d2, (size_t)sum * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                BH_HIP(c, hipMemcpyAsync(hidx.data(), s.ent_idx, (size_t)sum * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            }
            BH_HIP(c, hipMemcpyAsync(hev.data(), s.evals, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            BH_HIP(c, hipStreamSynchronize(st));                // (the row lists live in this scope; the next launch reuses the entries)
            if (int rc = span_ms(c, s.ev[0], s.ev[1], &s.fill_ms, true)) return rc;
            if (int rc = span_ms(c, s.ev[1], s.ev[2], &s.sort_ms, true)) return rc;
            int64_t from = 0;                                  // (the device's cursors are this prefix)
            for (int64_t r = a; r < b; ++r) {
                const int64_t at = (int64_t)hdest[(size_t)(t0 + r)], len = (int64_t)hcount[(size_t)(t0 + r)];
                std::memcpy(d2 + offsets[at], hd2.data() + from, (size_t)len * sizeof(double));
                for (int64_t e = 0; e < len; ++e) idx[offsets[at] + e] = (int64_t)hidx[(size_t)(from + e)];
                s.evals_host[(size_t)at] = hev[(size_t)(r - a)];
                from += len;
            }
        }
    }
    NblCounters ctr{};
    BH_HIP(c, hipMemcpyAsync(&ctr, s.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    BH_HIP(c, hipStreamSynchronize(st));
    if (ctr.refused || ctr.cut)
        return fail(c, BH_ERR_DEVICE, w + ": the fill pass disagrees with the count pass: " + std::to_string(ctr.refused) +
                                      " stores past a row's end were refused, " + std::to_string(ctr.cut) + " rows ended short");
    if (stats) { stats[0] = ctr.evals; stats[1] = ctr.opened; }
    return BH_OK;
}

int bh_neighbour_lists_times(bh_ctx *c, double *build_ms, double *count_ms, double *fill_ms, double *sort_ms)
{
    if (!c || !build_ms || !count_ms || !fill_ms || !sort_ms) return fail(c, BH_ERR_ARG, "bh_neighbour_lists_times: null argument");
    *build_ms = c->nbl.build_ms;
    *count_ms = c->nbl.count_ms;
    *fill_ms = c->nbl.fill_ms;
    *sort_ms = c->nbl.sort_ms;
    return BH_OK;
}

int bh_neighbour_lists_evals(bh_ctx *c, int64_t n_points, uint32_t *evals)
{
    if (!c || !evals) return fail(c, BH_ERR_ARG, "bh_neighbour_lists_evals: null argument");
    if (n_points != (int64_t)c->nbl.evals_host.size())
        return fail(c, BH_ERR_ARG, "bh_neighbour_lists_evals: the last bh_neighbour_lists call had " + std::to_string(c->nbl.evals_host.size()) + " queries");
    std::copy(c->nbl.evals_host.begin(), c->nbl.evals_host.end(), evals);
    return BH_OK;
}

}  // extern "C"
