// The body of walk_fast_kernel and walk_fast_soft_kernel (bh_walk_fast.hip), included once in each with SOFT set: the
// two kernels are the same text, and the unsoftened one compiles to the code it had before there was a softened one (a
// shared __device__ function does not: its __shared__ arrays are laid out in another order, and its argument loads are
// scheduled differently).  Not a header of its own: it needs the including kernel's template parameters, `a` and SOFT.
    static_assert(SPLIT == 1 || !LDS_STACK, "the split walk uses the register-lane stack");
    static_assert(!ASM || (!LDS_STACK && !STATS), "the assembly loops serve the default configuration");
    __shared__ int32_t s_base[LDS_STACK ? kWavesPerBlock : 1][LDS_STACK ? kLdsStackDepth : 1];
    __shared__ uint64_t s_mask[LDS_STACK ? kWavesPerBlock : 1][LDS_STACK ? kLdsStackDepth : 1];
    // split walk: two frontiers (current / next level), the waves' push counts, the partial sums
    constexpr int FCAP = SPLIT > 1 ? kSplitFrontier : 1;
    __shared__ int32_t fr_base[2][FCAP], fr_lo[2][FCAP], fr_hi[2][FCAP];
    __shared__ int32_t f_cnt[SPLIT > 1 ? SPLIT : 1];
    __shared__ float2 f_red[SPLIT > 1 ? SPLIT : 1][SPLIT > 1 ? kWave : 1];

    if (a.ctr->overflow) return;
#ifdef BHGPU_EXPERIMENTS
    const uint64_t dbg_t0 = a.timeline ? __builtin_amdgcn_s_memrealtime() : 0;     // 100 MHz wall clock
    const uint64_t dbg_c0 = a.timeline ? __builtin_amdgcn_s_memtime() : 0;         // shader clock cycles
#endif
    // Workgroup -> group of bodies: dispatch order.  (Measured and rejected, rounds 1-3: an XCD-contiguous placement --
    // XCD x takes the x-th contiguous eighth of the sorted order -- halves the L2 misses of the launch, 1.61 M -> 0.81 M,
    // and changes nothing: the waves that wait less for memory wait for an issue slot instead; reversed, strided and
    // heaviest-first orders: nothing either.  DESIGN.md section 4.)
    const uint32_t lb = blockIdx.x;
    if (lb >= a.nblocks) return;
    const int lane = lane_id(), w = wave_id();
    // SPLIT > 1: every wave of the workgroup holds the SAME 64 bodies
    const int64_t s = SPLIT > 1 ? a.lo + (int64_t)lb * kWave + lane : a.lo + (int64_t)lb * kBlock + threadIdx.x;
    bool valid = s < a.hi;
    const float2 p = valid ? a.spos[s] : float2{0.f, 0.f};
    asm volatile("" ::"v"(p.x), "v"(p.y));                // take the one-time vmcnt wait here, not per child
    float eps2 = SOFT ? a.eps2 : 0.f;
    if (SOFT) asm volatile("" : "+v"(eps2));              // in a VGPR: the SGPRs are the scarce file here (the operand of v_add_f32)
    float ax = 0.f, ay = 0.f;
    if (a.part == 2 && valid && (SPLIT == 1 || w == 0)) { const float2 t = a.acc_part[s]; ax = t.x; ay = t.y; }
    asm volatile("" : "+v"(ax), "+v"(ay));                // (same for this load: no s_waitcnt vmcnt in the loop)
    unsigned long long n_vis = 0, n_int = 0, n_wave = 0, n_quad = 0;
    uint32_t my_int = 0;                                     // counting variant: this lane's accepted force evaluations
    uint32_t cost = 0;                                       // loop iterations of this group's walk (re-balancing weight)

    const QuadF BH_CONSTANT *quads = as_constant(a.quads);
    const NodeAux BH_CONSTANT *aux = as_constant(a.aux);
    const float2 BH_CONSTANT *cpos = as_constant(a.spos);
    const float BH_CONSTANT *cmass = as_constant(a.smass);

    int32_t v_base = 0, v_lo = 0, v_hi = 0;      // register-lane stack: entry k lives in lane k & 63 of the
    int32_t v_base2 = 0, v_lo2 = 0, v_hi2 = 0;   // first (k < 64) or second triple: 128 entries (walk_tree_asm)
    int sp = 0;                                   // wave-uniform

    // hand-off slot of the quad being evaluated (walk_tree_asm): the first opened child that is a quad lands here
    // instead of on the stack; h_free == false: everything is pushed
    bool h_free = false;
    int32_t h_idx = -1;
    uint64_t h_mask = 0;

    auto eval = [&](const float cx, const float cy, const int32_t mbits, const float thr, const int32_t child,
                    const uint64_t mask) {
        if (mbits == 0) return;                             // empty cell (project.cu:617): scalar int test
        const float m = __int_as_float(mbits);
        const float dx = cx - p.x, dy = cy - p.y;
        const float d2 = fmaf(dx, dx, dy * dy);
        // One compare decides everything (a v_cmp result IS its ballot, so the rest is SALU):
        //   subdivided cell: thr = (size/theta)^2  -> the reference's MAC, per body (project.cu:643)
        //   leaf:            thr = 0               -> accepted unless d2 == 0, i.e. unless it is the
        //                                             body itself (the self skip, project.cu:646) or an
        //                                             exactly coincident body, where the reference divides
        //                                             by zero (inf*0 -> NaN, project.cu:651-658); fp32
        //                                             positions are quantised, that case is reachable, and
        //                                             one NaN would poison the root box of every later step
        //   bucket:          thr = +inf            -> accepted by nobody, opened by everybody
        const uint64_t farm = __ballot(d2 > thr);
        const uint64_t accm = mask & farm;
        // (measured: a uniform `if (accm != 0)` around the force math -- skipping it for cells that
        // every lane opens -- costs more in branches than it saves: 0.482 vs 0.466 ms)
        const float ri = __builtin_amdgcn_rsqf(SOFT ? d2 + eps2 : d2);
        const float wgt = __builtin_amdgcn_inverse_ballot_w64(accm) ? m * ri * ri * ri : 0.f;
        ax = fmaf(wgt, dx, ax);
        ay = fmaf(wgt, dy, ay);
        if (STATS) { n_vis += __popcll(mask); ++n_wave; n_int += __popcll(accm); my_int += (uint32_t)((accm >> lane) & 1ull); }
        if (child != -1) {                                  // subdivided cell or bucket reference
            const uint64_t open = mask & ~farm;
            if (open != 0 && h_free && child > 0) {         // handed over in registers
                h_idx = child; h_mask = open; h_free = false;
            } else if (open != 0) {                         // ~30 % of the evaluated nodes
                if (LDS_STACK) {
                    if (lane == 0) { s_base[w][sp] = child; s_mask[w][sp] = open; }
                } else if (sp < kWave) {
                    v_base = bh_writelane_i32(child, sp, v_base);
                    v_lo = bh_writelane_i32((int32_t)(uint32_t)open, sp, v_lo);
                    v_hi = bh_writelane_i32((int32_t)(uint32_t)(open >> 32), sp, v_hi);
                } else {
                    v_base2 = bh_writelane_i32(child, sp - kWave, v_base2);
                    v_lo2 = bh_writelane_i32((int32_t)(uint32_t)open, sp - kWave, v_lo2);
                    v_hi2 = bh_writelane_i32((int32_t)(uint32_t)(open >> 32), sp - kWave, v_hi2);
                }
                ++sp;
            }
        }
    };

    auto eval_quad = [&](const QuadRegs &q, const uint64_t mask) {
        if (STATS) ++n_quad;
        eval(__int_as_float(q.g[0]), __int_as_float(q.g[1]), q.g[8], __int_as_float(q.g[12]), q.c[0], mask);
        eval(__int_as_float(q.g[2]), __int_as_float(q.g[3]), q.g[9], __int_as_float(q.g[13]), q.c[1], mask);
        eval(__int_as_float(q.g[4]), __int_as_float(q.g[5]), q.g[10], __int_as_float(q.g[14]), q.c[2], mask);
        eval(__int_as_float(q.g[6]), __int_as_float(q.g[7]), q.g[11], __int_as_float(q.g[15]), q.c[3], mask);
    };

    // depth-cap cell holding several bodies (compat off): summed body by body for the lanes that
    // reached it; self and exactly coincident bodies contribute nothing (d2 == 0)
    auto bucket = [&](const int32_t node, const uint64_t mask) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        const v2i rng = *(const v2i BH_CONSTANT *)(aux + node);
        for (int32_t j = rng[0]; j < rng[0] + rng[1]; ++j) {
            const v2i ob = *(const v2i BH_CONSTANT *)(cpos + j);      // scalar loads: j is uniform
            const float om = *(const float BH_CONSTANT *)(cmass + j);
#pragma clang diagnostic pop
            const float dx = __int_as_float(ob[0]) - p.x, dy = __int_as_float(ob[1]) - p.y;
            const float d2 = fmaf(dx, dx, dy * dy);
            const float ri = __builtin_amdgcn_rsqf(SOFT ? d2 + eps2 : d2);
            const uint64_t okm = mask & __ballot(d2 > 0.f);
            const float wgt = __builtin_amdgcn_inverse_ballot_w64(okm) ? om * ri * ri * ri : 0.f;
            ax = fmaf(wgt, dx, ax);
            ay = fmaf(wgt, dy, ay);
            if (STATS) { n_int += __popcll(okm); my_int += (uint32_t)((okm >> lane) & 1ull); }
        }
    };

    auto pop_raw = [&](int32_t &base, uint64_t &mask) {         // sp > 0
        --sp;
        if (LDS_STACK) {
            base = __builtin_amdgcn_readfirstlane(s_base[w][sp]);
            const uint64_t m = s_mask[w][sp];
            mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(m >> 32)) << 32) |
                   (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)m);
        } else if (sp < kWave) {
            base = __builtin_amdgcn_readlane(v_base, sp);
            mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(v_hi, sp) << 32) |
                   (uint32_t)__builtin_amdgcn_readlane(v_lo, sp);
        } else {
            base = __builtin_amdgcn_readlane(v_base2, sp - kWave);
            mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(v_hi2, sp - kWave) << 32) |
                   (uint32_t)__builtin_amdgcn_readlane(v_lo2, sp - kWave);
        }
    };
    // take the next quad entry off the stack; bucket references (-(node id) - 2) are served on the
    // way; returns false when the stack is empty
    auto pop_quad = [&](int32_t &base, uint64_t &mask) -> bool {
        while (sp > 0) {
            --sp;
            if (LDS_STACK) {
                base = __builtin_amdgcn_readfirstlane(s_base[w][sp]);
                const uint64_t m = s_mask[w][sp];
                mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(m >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)m);
            } else {
                base = __builtin_amdgcn_readlane(v_base, sp);
                mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(v_hi, sp) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane(v_lo, sp);
            }
            if (base >= 0) return true;
            if (base <= -2) bucket(-base - 2, mask);       // base == -1 (a leaf opened by a NaN) is dropped
        }
        return false;
    };

    if (SPLIT > 1) {
        const uint64_t everyone = __ballot(valid);
        // level 0: the root quad of the local tree and of every received LET (at most 57 entries)
        const int n_remote = (a.n_trees > 0 && a.part != 1) ? a.n_trees - 1 : 0;
        const int n_local = (a.part != 2) ? 1 : 0;
        int F = n_local + n_remote;
        if (w == 0 && lane < F) {
            int32_t base = 0;
            if (lane >= n_local) {
                int32_t t = lane - n_local;
                if (t >= a.self_rank) ++t;                      // the peers in rank order, self skipped
                base = (int32_t)(a.forest_base + (int64_t)t * a.let_cap);
            }
            fr_base[0][lane] = base;
            fr_lo[0][lane] = (int32_t)(uint32_t)everyone;
            fr_hi[0][lane] = (int32_t)(uint32_t)(everyone >> 32);
        }
        __syncthreads();
        auto lane_entry = [&](int32_t vb, int32_t vl, int32_t vh, int j, int32_t &base, uint64_t &mask) {
            base = __builtin_amdgcn_readlane(vb, j);
            mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(vh, j) << 32) |
                   (uint32_t)__builtin_amdgcn_readlane(vl, j);
        };
        int cur = 0;
        while (F > 0) {                                         // one iteration per tree level
            cost += (uint32_t)F;
            int produced = 0;
            for (int r0 = 0; r0 < F; r0 += SPLIT * kSplitRound) {
                const int rem = (F - r0 < SPLIT * kSplitRound) ? F - r0 : SPLIT * kSplitRound;
                const int chunk = (rem + SPLIT - 1) / SPLIT;    // equal contiguous chunks, <= kSplitRound
                const int first = r0 + w * chunk;
                int mine = r0 + rem - first;
                mine = (mine < 0) ? 0 : (mine > chunk ? chunk : mine);
                int32_t in_base = 0, in_lo = 0, in_hi = 0;      // lane j holds this wave's j-th entry
                if (lane < mine) {
                    in_base = fr_base[cur][first + lane]; in_lo = fr_lo[cur][first + lane]; in_hi = fr_hi[cur][first + lane];
                }
                sp = 0;
                // All of this wave's quads are known before the first is evaluated, so the scalar loads
                // of entry j+1 are issued before entry j is evaluated (~1000 cycles for a lone wave against
                // a ~370-cycle load): the depth-first loop cannot do this, its next address is the
                // result of the evaluation.  (Bucket references and lanes past `mine` read quad 0.)
                auto quad_of = [&](int j) {
                    const int32_t b = __builtin_amdgcn_readlane(in_base, j & (kWave - 1));
                    return load_quad(quads + (b < 0 ? 0 : b));
                };
                if (ASM) {
                    sp = walk_list_asm<SOFT>(quads, as_constant(a.bucket_consts), in_base, in_lo, in_hi, __builtin_amdgcn_readfirstlane(mine), p.x, p.y, eps2, ax, ay,
                                       v_base, v_lo, v_hi);
                } else {
                    QuadRegs qn = quad_of(0);
                    for (int j = 0; j < mine; ++j) {
                        int32_t base; uint64_t mask;
                        lane_entry(in_base, in_lo, in_hi, j, base, mask);
                        const QuadRegs q = qn;
                        qn = quad_of(j + 1);
                        if (base <= -2) { bucket(-base - 2, mask); continue; }
                        if (base < 0) continue;
                        eval_quad(q, mask);                     // opened children -> private stack, sp <= 64
                    }
                }
                if (lane == 0) f_cnt[w] = sp;
                __syncthreads();
                int off = produced, total = 0;
#pragma unroll
                for (int k = 0; k < SPLIT; ++k) {
                    const int ck = __builtin_amdgcn_readfirstlane(f_cnt[k]);
                    off += (k < w) ? ck : 0;
                    total += ck;
                }
                if (produced + total <= FCAP) {                 // uniform over the workgroup
                    if (lane < sp) {
                        fr_base[cur ^ 1][off + lane] = v_base; fr_lo[cur ^ 1][off + lane] = v_lo; fr_hi[cur ^ 1][off + lane] = v_hi;
                    }
                    produced += total;
                } else {
                    // next frontier full (never seen in practice): every wave finishes the subtrees it
                    // has just opened depth-first, one at a time so the 64-entry stack bound holds
                    in_base = v_base; in_lo = v_lo; in_hi = v_hi;
                    const int todo = sp;
                    for (int j = 0; j < todo; ++j) {
                        int32_t base; uint64_t mask;
                        lane_entry(in_base, in_lo, in_hi, j, base, mask);
                        sp = 0;
                        if (base <= -2) { bucket(-base - 2, mask); continue; }
                        if (base < 0) continue;
                        do {
                            const QuadRegs q = load_quad(quads + base);
                            eval_quad(q, mask);
                        } while (pop_quad(base, mask));
                    }
                }
                __syncthreads();
            }
            cur ^= 1;
            F = produced;
        }
        // ---- partial sums back to wave 0, added in wave order
        f_red[w][lane] = float2{ax, ay};
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int k = 1; k < SPLIT; ++k) { ax += f_red[k][lane].x; ay += f_red[k][lane].y; }
        }
        valid = valid && (w == 0);
    } else {
        // the local tree, then (distributed step) the locally-essential tree of every peer: one
        // traversal per tree, so the stack never holds more than one tree's entries
        const uint64_t everyone = __ballot(valid);
        const int32_t t_first = (a.part == 2) ? 0 : -1, t_end = (a.part == 1) ? 0 : a.n_trees;
        for (int32_t t = t_first; t < t_end; ++t) {
            if (t >= 0 && t == a.self_rank) continue;
            int32_t base = (t < 0) ? 0 : (int32_t)(a.forest_base + (int64_t)t * a.let_cap);
            if (ASM) {
                cost += walk_tree_asm<SOFT>(quads, as_constant(a.bucket_consts), base, everyone, a.pair_limit, p.x, p.y, eps2, ax, ay);
                continue;
            }
            {
                // the C++ statement of walk_tree_asm's abstract machine: same order, same operations
                int32_t na = -1, nb = -1;                       // handed-over children (quad index, -1: none) ...
                uint64_t nam = 0, nbm = 0;                      // ... and the lanes that opened them
                bool first = true;
                for (;;) {
                    int32_t bA, bB = -1;
                    uint64_t mA, mB = 0;
                    ++cost;
                    if (first) { bA = base; mA = everyone; first = false; }
                    else {
                        if (na >= 0) { bA = na; mA = nam; }
                        else if (sp > 0) {
                            pop_raw(bA, mA);
                            if (bA < 0) {
                                if (bA <= -2) bucket(-bA - 2, mA);  // -1 (a leaf opened by a NaN) is dropped
                                continue;
                            }
                        } else if (nb >= 0) { bA = nb; mA = nbm; nb = -1; }
                        else break;
                        if (nb >= 0) { bB = nb; mB = nbm; }
                        else if (sp > 0 && sp <= a.pair_limit) {
                            pop_raw(bB, mB);
                            if (bB < 0) { ++sp; bB = -1; }          // a bucket reference: leave it on the stack
                        }
                    }
                    const QuadRegs A = load_quad(quads + bA);
                    QuadRegs B = A;
                    if (bB >= 0) B = load_quad(quads + bB);         // (both in flight before A is evaluated)
                    h_free = true; h_idx = -1;
                    eval_quad(A, mA);
                    na = h_idx; nam = h_mask;
                    nb = -1;
                    if (bB >= 0) {
                        h_free = sp <= a.pair_limit; h_idx = -1;    // too deep for another pair: push everything
                        eval_quad(B, mB);
                        nb = h_idx; nbm = h_mask;
                    }
                    h_free = false;
                }
            }
        }
    }

    // Epilogue.  Its arguments are read AGAIN from the kernarg segment through a laundered pointer: the
    // compiler otherwise loads all ~50 argument dwords up front and keeps the ones used here alive across
    // the traversal loop, which pushed the kernel to 106 SGPRs = 6 resident waves per SIMD instead of 8
    // (measured: 6,144 resident waves; the walk is latency-bound, waves are what hides the latency).
    const WalkFastArgs BH_CONSTANT *ka;
    {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        ka = (const WalkFastArgs BH_CONSTANT *)__builtin_amdgcn_kernarg_segment_ptr();
#pragma clang diagnostic pop
    }
    asm volatile("" : "+s"(ka));
    const WalkFastArgs BH_CONSTANT &e = *ka;
    float2 np = p;
    double2 np64{0.0, 0.0};
    if (e.part == 1) {
        if (valid) e.acc_part[s] = float2{ax, ay};              // raw sums; part 2 carries on from here
    } else if (valid) {
        const float gx = e.G * ax, gy = e.G * ay;
        const uint32_t body = e.perm[s];
        if (e.acc_out) e.acc_out[body] = float2{gx, gy};
        if (e.integrate && e.state64) {
            // mixed precision: the fp32 acceleration advances the fp64 state (updateAccVelPos,
            // project.cu:819-836, in the state's precision) with the fp64 time step
            double2 *pos64 = reinterpret_cast<double2 *>(e.pos), *vel64 = reinterpret_cast<double2 *>(e.vel);
            double2 v = vel64[body];
            const double2 q = pos64[body];
            v.x = fma((double)gx, e.dt64, v.x);
            v.y = fma((double)gy, e.dt64, v.y);
            np64 = double2{fma(v.x, e.dt64, q.x), fma(v.y, e.dt64, q.y)};
            vel64[body] = v;
            pos64[body] = np64;
        } else if (e.integrate) {
            float2 v = e.vel[body];
            v.x = fmaf(gx, e.dt, v.x);
            v.y = fmaf(gy, e.dt, v.y);
            np = float2{fmaf(v.x, e.dt, p.x), fmaf(v.y, e.dt, p.y)};
            if (e.to_sorted) {
                e.sstate[s] = float4{np.x, np.y, v.x, v.y};
            } else {
                e.vel[body] = v;
                e.pos[body] = np;
            }
        }
    }
    // min/max of the new positions per workgroup: the next step's root box needs no body pass
    const double bx = e.state64 ? np64.x : (double)np.x, by = e.state64 ? np64.y : (double)np.y;
    if (SPLIT > 1) {
        if ((e.slots || e.partial) && w == 0) {             // one record per 64-body group
            const double xlo = wave_min(valid ? bx : (double)INFINITY), xhi = wave_max(valid ? bx : -(double)INFINITY);
            const double ylo = wave_min(valid ? by : (double)INFINITY), yhi = wave_max(valid ? by : -(double)INFINITY);
            if (lane == 0) {
                if (e.partial) {
                    double *o = e.partial + 4 * (size_t)lb;
                    o[0] = xlo; o[1] = xhi; o[2] = ylo; o[3] = yhi;
                }
                if (e.slots) bounds_to_slot(xlo, xhi, ylo, yhi, e.slots, (uint32_t)lb);
            }
        }
    } else if (e.slots || e.partial) block_bounds(valid, bx, by, e.slots, e.partial ? e.partial + 4 * (size_t)lb : nullptr);
#ifdef BHGPU_EXPERIMENTS
    if (e.timeline && lane == 0) {                              // per wave: start, end (10 ns ticks), hardware id, cost, clock stamps
        const int64_t wv = (int64_t)blockIdx.x * (blockDim.x >> 6) + w;
        const uint64_t c1 = __builtin_amdgcn_s_memtime(), t1 = __builtin_amdgcn_s_memrealtime();
        e.timeline[6 * wv + 0] = dbg_t0;
        e.timeline[6 * wv + 1] = t1;
        e.timeline[6 * wv + 2] = (uint64_t)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_REG_HW_ID
        e.timeline[6 * wv + 3] = cost;
        e.timeline[6 * wv + 4] = dbg_c0;
        e.timeline[6 * wv + 5] = c1;
    }
#endif
    if (e.group_cost && lane == 0 && (SPLIT == 1 || w == 0)) {
        const int64_t g = (SPLIT > 1 ? e.lo + (int64_t)lb * kWave : e.lo + (int64_t)lb * kBlock + (int64_t)w * kWave) >> 6;
        if (e.part == 2) e.group_cost[g] += cost;               // the second launch of a split forest walk adds its share
        else e.group_cost[g] = cost;
    }
    if (STATS && e.body_counts && s < e.hi && my_int) atomicAdd(&e.body_counts[e.perm[s]], my_int);   // (every wave of a split group adds its share)
    if (STATS && lane == 0) {
        atomicAdd(&e.ctr->visits, n_vis);
        atomicAdd(&e.ctr->interactions, n_int);
        atomicAdd(&e.ctr->wave_nodes, n_wave);
        atomicAdd(&e.ctr->wave_quads, n_quad);
    }
