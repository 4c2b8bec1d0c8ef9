// The body of walk_f64_kernel and walk_f64_soft_kernel (bh_walk_f64.hpp), included once in each with SOFT set: the two
// kernels are the same text, and the unsoftened one compiles to the code it had before there was a softened one (a shared
// __device__ function does not).  Not a header of its own: it needs the including kernel's template parameters, `a` and SOFT.
    static_assert(!ASM || !STATS, "the assembly loop carries no counters");
#if defined(BH64_LDS_PAD) && BH64_LDS_PAD
    __shared__ int s_pad[BH64_LDS_PAD / 4];
    if (a.dt == -12345.0) s_pad[threadIdx.x] = 1;                // (never true: keeps the array alive)
    asm volatile("" ::"v"(s_pad[0]));
#endif
    if (a.ctr->overflow) return;
    const int lane = lane_id();
    const int64_t s = a.lo + ((int64_t)blockIdx.x * (kF64Block / kWave) + wave_id()) * a.bpw + lane;
    const bool valid = lane < a.bpw && s < a.hi;
    const int64_t body = valid ? (int64_t)a.perm[s] : -1;
    const double2 p = valid ? a.pos[body] : double2{0.0, 0.0};
    const double mi = valid ? a.mass[body] : 0.0;
    const NodeD *gd = a.gd;
    const LinkD *ld = a.ld;
    double sx = 0.0, sy = 0.0;                       // sum of M * d_vec / (d2 * d)
    double eps2 = SOFT ? a.eps2 : 0.0;
    if (SOFT) asm volatile("" : "+v"(eps2));         // in VGPRs: this kernel has no SGPR to spare (80 = 8 resident waves)
    unsigned long long n_vis = 0, n_int = 0, n_wave = 0, n_quad = 0, n_acc = 0;
    uint32_t my_int = 0;

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    const char BH64_CONSTANT *cg = (const char BH64_CONSTANT *)gd;
    const char BH64_CONSTANT *cl = (const char BH64_CONSTANT *)ld;
#pragma clang diagnostic pop
    // (all three requests of a quad are issued together and waited for once: left to itself the compiler issues the second
    // half and the links only after the first half has arrived and its first node has passed the empty test -- two round
    // trips per quad)
    auto load_quad = [&](int32_t first) {
        Quad64 q;
        const char BH64_CONSTANT *pn = cg + (int64_t)first * 32;
        const char BH64_CONSTANT *pl = cl + (int64_t)first * 8;
        asm volatile("s_load_dwordx16 %0, %3, 0x0\n\t"
                     "s_load_dwordx16 %1, %3, 0x40\n\t"
                     "s_load_dwordx8 %2, %4, 0x0\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&s"(q.a), "=&s"(q.b), "=&s"(q.l)
                     : "s"(pn), "s"(pl)
                     : "memory");
        return q;
    };

    int32_t v_base = 0, v_lo = 0, v_hi = 0, v_base2 = 0, v_lo2 = 0, v_hi2 = 0;   // register-lane stack, 128 entries
    int sp = 0;
    int32_t h_idx = 0;                                // hand-off slot of the quad being evaluated: < 0 = free (a child index is > 0)
    uint64_t h_mask = 0;

    auto push = [&](int32_t child, uint64_t open) {
        if (!DEEP || sp < kWave) {
            v_base = bh64_writelane_i32(child, sp, v_base);
            v_lo = bh64_writelane_i32((int32_t)(uint32_t)open, sp, v_lo);
            v_hi = bh64_writelane_i32((int32_t)(uint32_t)(open >> 32), sp, v_hi);
        } else if (sp < 2 * kWave) {
            v_base2 = bh64_writelane_i32(child, sp - kWave, v_base2);
            v_lo2 = bh64_writelane_i32((int32_t)(uint32_t)open, sp - kWave, v_lo2);
            v_hi2 = bh64_writelane_i32((int32_t)(uint32_t)(open >> 32), sp - kWave, v_hi2);
        }
        ++sp;                                         // (beyond 128 cannot happen: 3 * 31 + 1 entries at max_depth 32)
    };
    auto pop = [&](int32_t &base, uint64_t &mask) {
        --sp;
        if (!DEEP || sp < kWave) {
            base = __builtin_amdgcn_readlane(v_base, sp);
            mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(v_hi, sp) << 32) | (uint32_t)__builtin_amdgcn_readlane(v_lo, sp);
        } else {
            base = __builtin_amdgcn_readlane(v_base2, sp - kWave);
            mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(v_hi2, sp - kWave) << 32) |
                   (uint32_t)__builtin_amdgcn_readlane(v_lo2, sp - kWave);
        }
    };

    // one node for the lanes in `mask` (all arguments but the position wave-uniform): the statement of BH64_CHILD
    const int32_t body32 = (int32_t)body;                         // (perm is 32-bit; -1 on padding lanes)
    const int32_t compat32 = -2 - body32;                         // occ + 2 == -body, project.cu:646
    auto eval = [&](double cx, double cy, double m, double thr, int32_t child, int32_t occ, uint64_t mask) {
        // m <= 1e-15 (project.cu:617) on the bit pattern, with scalar integer compares
        {
            const int32_t mh = __double2hiint(m);
            if (__builtin_expect(mh <= 0x3CD203AF, 0)) {
                if (mh < 0x3CD203AF) return;
                if ((uint32_t)__double2loint(m) <= 0x9EE75616u) return;
            }
        }
        const double dx = cx - p.x, dy = cy - p.y;
        const double d2 = fma(dx, dx, dy * dy);
        uint64_t takem, open;
        if (child < 0) {                                          // a leaf: everybody but its occupant (project.cu:623-626, 646)
            uint64_t self = __builtin_amdgcn_ballot_w64(occ == body32);
            if (COMPAT) self |= __builtin_amdgcn_ballot_w64(occ == compat32);
            takem = mask & ~self;
            open = 0;
        } else {                                                  // size / d < theta (project.cu:643) as thr < d2, see the header
            const uint64_t acc = __builtin_amdgcn_ballot_w64(thr < d2);
            takem = mask & acc;
            open = mask & ~acc;
        }
        if (open != 0) {
            if (h_idx < 0) { h_idx = child; h_mask = open; }
            else push(child, open);
        }
        if (takem != 0) {
            // M / (d2 * d):  1 / d2 = y * y,  1 / d = 1 / (sqrt(d2) + 1e-15) = y - 1e-15 y^2 to second order; added for the
            // accepting lanes only (the others may hold inf / NaN here: a body's own leaf has d2 = 0)
            const double s2 = SOFT ? d2 + eps2 : d2;
            const double y0 = __builtin_amdgcn_rsq(s2);
            const double t = s2 * y0;
            const double e = fma(-t, y0, 1.0);
            const double h = y0 * e;
            const double y = fma(h, 0.5, y0);
            const double a = y * y;
            const double b = fma(a, -1e-15, y);
            const double w = (a * m) * b;
            if ((takem >> lane) & 1ull) { sx = fma(w, dx, sx); sy = fma(w, dy, sy); }
        }
        if (STATS) { n_vis += __popcll(mask); ++n_wave; n_int += __popcll(takem); n_acc += takem != 0; my_int += (uint32_t)((takem >> lane) & 1ull); }
    };
    auto node_of = [&](const Quad64 &q, int k, double &cx, double &cy, double &m, double &thr) {
        const w64_v16i &t = (k < 2) ? q.a : q.b;
        const int o = (k & 1) * 8;
        cx = w64_f64(t[o + 0], t[o + 1]); cy = w64_f64(t[o + 2], t[o + 3]);
        m = w64_f64(t[o + 4], t[o + 5]); thr = w64_f64(t[o + 6], t[o + 7]);
    };

    // the root (node 0) alone, then quads of four siblings
    {
        const NodeD r = gd[0];
        const LinkD k = ld[0];
        h_idx = -1;
        eval(r.cx, r.cy, r.m, r.size, k.child, k.occ, __ballot(valid));
    }
    int32_t na = h_idx;
    uint64_t nam = h_mask;
    if (ASM) {
        if (na >= 0) walk64_asm<COMPAT, DEEP, SOFT>(cg, cl, na, nam, p.x, p.y, body32, eps2, sx, sy);
    } else {
        for (;;) {
            int32_t base;
            uint64_t mask;
            if (na >= 0) { base = na; mask = nam; }
            else if (sp > 0) pop(base, mask);
            else break;
            const Quad64 q = load_quad(base);
            if (STATS) ++n_quad;
            h_idx = -1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double cx, cy, m, thr;
                node_of(q, k, cx, cy, m, thr);
                eval(cx, cy, m, thr, q.l[2 * k], q.l[2 * k + 1], mask);
            }
            na = h_idx; nam = h_mask;
        }
    }

    // Epilogue.  Its arguments are read AGAIN from the kernarg segment through a laundered pointer: the compiler otherwise
    // keeps the ones used here alive in SGPRs across the traversal loop -- 82 SGPRs, 7 resident waves per SIMD; at most 80
    // is 8, and this walk answers to residency (measured, profiles/r04_f64/walk_ab.txt: 8 / 7 / 5 / 4 / 3 waves).
    const WalkF64Args BH64_CONSTANT *ka;
    {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        ka = (const WalkF64Args BH64_CONSTANT *)__builtin_amdgcn_kernarg_segment_ptr();
#pragma clang diagnostic pop
    }
    asm volatile("" : "+s"(ka));
    const WalkF64Args BH64_CONSTANT &e = *ka;
    double2 np = p;
    if (valid) {
        const double gm = e.G * mi;                               // (G * masses[i]) * nodeMass / d2 * d_vec / d, project.cu:651-658
        const double fx = gm * sx, fy = gm * sy;
        e.force_out[body] = double2{fx, fy};
        if (e.integrate) {
            const double ax = e.G * sx, ay = e.G * sy;            // F / m_i (updateAccVelPos, project.cu:827-834)
            double2 v = e.vel[body];
            v.x = fma(ax, e.dt, v.x);  v.y = fma(ay, e.dt, v.y);
            e.vel[body] = v;
            np.x = fma(v.x, e.dt, np.x);  np.y = fma(v.y, e.dt, np.y);
            e.pos[body] = np;
        }
        if (STATS && e.body_counts) e.body_counts[body] = my_int;
    }
    if (e.slots) {                                                // min/max of the new positions per workgroup (next root box)
        if (kF64Block == kWave) {
            const double xlo = wave_min(valid ? np.x : (double)INFINITY), xhi = wave_max(valid ? np.x : -(double)INFINITY);
            const double ylo = wave_min(valid ? np.y : (double)INFINITY), yhi = wave_max(valid ? np.y : -(double)INFINITY);
            if (lane == 0) bounds_to_slot(xlo, xhi, ylo, yhi, e.slots, blockIdx.x);
        } else {
            block_bounds(valid, np.x, np.y, e.slots);
        }
    }
    if (STATS && lane == 0) {
        atomicAdd(&e.ctr->visits, n_vis);
        atomicAdd(&e.ctr->interactions, n_int);
        atomicAdd(&e.ctr->wave_nodes, n_wave);
        atomicAdd(&e.ctr->wave_quads, n_quad);
        atomicAdd(&e.ctr->wave_accepts, n_acc);
    }
