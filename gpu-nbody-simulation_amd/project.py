"""The reference program's entry points under their own names, driving the HIP engine.

`runSimulationGpu` mirrors project.cu:918-1024 (same arguments plus the former compile-time
constants as keywords; same files written: quadtree_init_gpu.txt at step 0 and
quadtree_final_gpu.txt at the last step, each BEFORE that step's update, project.cu:962-965);
`main` mirrors project.cu:1049-1105 and prints exactly the two timing lines the scaling scripts
and plot_first_scale.py:55-59 parse:

    GPU total computation took <int> milliseconds.
    GPU parallel computation took <int> microseconds.

    python -m gpu_nbody_simulation_amd.project -DN_BODIES=1024 -DN_THREADS=1024 -DN_SIMULATIONS=100

(-D options are accepted in the reference's own spelling, so `nvcc -DN_BODIES=... project.cu`
lines of the scaling scripts translate one to one.)
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np

from .engine import BarnesHutEngine, BhConfig, Precision, radial_edges, sample_targets, toomre_q_from
from .textio import loadSimulationDataFromText

# project.cu:27-35, 60-61
G = 6.67e-11
DELTA_T = 1.0
THETA = 5e-1
QUADTREE_MAX_DEPTH = 10
LOWER_M, HIGHER_M = 1e-1, 5e-1
LOWER_P, HIGHER_P = -1e-1, 1e-1
LOWER_V, HIGHER_V = -1e-4, 1e-4


def initializeCpu(n_bodies: int, seed: int = 0, save_to_file: bool = False):
    """initializeCpu (project.cu:298-302): log-uniform masses, uniform positions/velocities.
    numpy's PCG64 replaces rand(); the reference seeds from time() and is not reproducible."""
    rng = np.random.default_rng(seed)
    masses = 10.0 ** (np.log10(LOWER_M) + rng.random(n_bodies) * (np.log10(HIGHER_M) - np.log10(LOWER_M)))
    positions = LOWER_P + rng.random((n_bodies, 2)) * (HIGHER_P - LOWER_P)
    velocities = LOWER_V + rng.random((n_bodies, 2)) * (HIGHER_V - LOWER_V)
    if save_to_file:
        from .textio import save_init_files
        save_init_files(masses, positions, velocities)
        print("Masses saved to masses_init.txt")
        print("Vectors saved to positions_init.txt")
        print("Vectors saved to velocities_init.txt")
    return masses, positions, velocities


def initializeGpu(n_bodies: int, seed: int = 0, precision: Precision = Precision.F64_EXACT,
                  save_to_file: bool = False, device: int = 0):
    """initializeGpu (project.cu:304-341): bodies generated on the device with the reference's
    ranges (project.cu:30-35), reproducible for a given seed (the reference seeds cuRAND from
    time(NULL), project.cu:323).  save_to_file writes the three init files as initializeCpu's
    save_to_file branch does (project.cu:298-302)."""
    with BarnesHutEngine(BhConfig(capacity=max(n_bodies, 1), precision=precision, device=device)) as eng:
        eng.initialize(n_bodies, seed, "box", LOWER_M, HIGHER_M, LOWER_P, HIGHER_P, LOWER_V, HIGHER_V)
        positions, velocities = eng.download()
        masses = eng.masses()
    if save_to_file:
        from .textio import save_init_files
        save_init_files(masses, positions, velocities)
    return masses, positions, velocities


def initializeDisc(n_bodies: int, seed: int = 0, mass: float = 1.0, scale: float = 0.02, r_max: float = 0.2, q: float = 1.5,
                   precision: Precision = Precision.F64_EXACT, theta: float = THETA, g: float = G,
                   max_depth: int = QUADTREE_MAX_DEPTH, reference_compat: bool = True, softening: float = 0.0,
                   save_to_file: bool = False, device: int = 0):
    """A Kuzmin-Toomre disc in equilibrium: BarnesHutEngine.initialize_disc, then equilibrate_disc(q) under the force law the
    run will use (theta, g, softening).  Reproducible for a given seed."""
    with BarnesHutEngine(BhConfig(capacity=max(n_bodies, 1), theta=theta, G=g, max_depth=max_depth, precision=precision,
                                  reference_compat=reference_compat, device=device, softening=softening)) as eng:
        eng.initialize_disc(n_bodies, seed, mass, scale, r_max)
        eng.equilibrate_disc(q, seed=seed)
        positions, velocities = eng.download()
        masses = eng.masses()
    if save_to_file:
        from .textio import save_init_files
        save_init_files(masses, positions, velocities)
    return masses, positions, velocities


def runSimulationGpu(masses, positions, velocities, n_simulations: int, *, n_threads: int = 0,
                     theta: float = THETA, g: float = G, delta_t: float = DELTA_T,
                     max_depth: int = QUADTREE_MAX_DEPTH, precision: Precision = Precision.F64_EXACT,
                     reference_compat: bool = True, out_dir: str = ".", device: int = 0,
                     positions_file: str | None = None, energy_file: str | None = None, energy_every: int = 0,
                     force_error_file: str | None = None, force_error_every: int = 0, force_error_sample: int = 65536,
                     field_file: str | None = None, field_grid=None, field_box=None, softening: float = 0.0,
                     integrator: str = "euler", density_file: str | None = None, density_grid=None, density_box=None,
                     density_scheme: str = "cic", neighbours_file: str | None = None, neighbours_k: int = 6,
                     groups_file: str | None = None, linking_length: float | None = None, groups_min: int = 2,
                     profile_file: str | None = None, profile_bins: int | None = None, profile_range=None,
                     profile_spacing: str = "log", profile_centre="density", lagrange_file: str | None = None,
                     lagrange_fractions=(0.01, 0.1, 0.5, 0.9), lagrange_every: int = 0, lagrange_centre="density",
                     pairs_file: str | None = None, pairs_bins: int | None = None, pairs_range=None, pairs_spacing: str = "log",
                     pairs_randoms: int | None = None, pairs_seed: int = 0, mst_file: str | None = None,
                     segregation_file: str | None = None, segregation_massive: int | None = None, segregation_random: int = 500,
                     segregation_seed: int = 0, binaries_file: str | None = None, binaries_separation: float | None = None,
                     encounters_file: str | None = None, encounters_radius: float | None = None,
                     modes_file: str | None = None, modes_bins: int | None = None, modes_max: int = 4, modes_range=None,
                     modes_spacing: str = "log", modes_centre="density", bar_file: str | None = None, bar_mode: int = 2,
                     bar_every: int = 0, bar_range=None, bar_centre="density", curve_file: str | None = None,
                     curve_bins: int | None = None, curve_range=None, curve_spacing: str = "log", curve_centre="density"):
    """Returns (final_positions, final_velocities, gpu_parallel_duration_us).

    positions is NOT modified in place (the reference updates its by-reference argument,
    project.cu:918, 1010; the caller gets the same values as the first return value).
    positions_file: also write the trajectory as runSimulationCpu does into positions_cpu.txt
    (savePositions, project.cu:855-863, 876, 909: `t i x y ` per body, before the first step and
    after every step); this downloads the positions every step.
    energy_file: also write the diagnostics of the state (BarnesHutEngine.energy) before the first step, after every
    energy_every-th step and after the last one, one line each: `step,t,kinetic,potential,total,px,py,Lz` (%.17g).
    The steps in between still run batched, and the diagnostics are not part of gpu_parallel_duration_us.
    force_error_file: likewise, with the same cadence rules (force_error_every), the Barnes-Hut force error of the state
    against the direct sum (BarnesHutEngine.force_error) on min(n, force_error_sample) bodies drawn once, the same on
    every line: `step,t,n,median,p90,p99,p999,max,worst`.
    field_file: after the last step, also write the Barnes-Hut field of the final state (BarnesHutEngine.field) on the
    cell-centred field_grid = (NX, NY) grid over field_box = (xmin, xmax, ymin, ymax) (None: the bounding box of the final
    positions): the line `# x,y,ax,ay,phi`, then one row per point (%.17g), y the outer axis.  Not part of
    gpu_parallel_duration_us.
    density_file: after the last step, also write the moment maps of the final state (BarnesHutEngine.moment_map, scheme
    density_scheme) on the density_grid = (NX, NY) cells over density_box (None: the bounding box of the final positions):
    the line `# x,y,sigma,vx,vy,dispersion`, then one row per cell centre (%.17g; nan in a cell without mass), y the outer
    axis -- the points of field_file for the same grid and box.  Not part of gpu_parallel_duration_us.
    neighbours_file: after the last step, also write the k-th-neighbour density of the final state
    (BarnesHutEngine.local_density(neighbours_k)): the line `# i,x,y,r_k,sigma`, then one row per body in caller order (%.17g):
    its index, its position, the distance of its k-th neighbour and Casertano and Hut's surface density.  Not part of
    gpu_parallel_duration_us.
    groups_file: after the last step, also write the friends-of-friends catalogue of the final state
    (BarnesHutEngine.groups(linking_length, groups_min)): the line `# id,count,mass,x,y,vx,vy`, then one row per group with at
    least groups_min bodies (%.17g), the largest first: its label (the smallest body index in it), its member count, its mass,
    its centre of mass and its bulk velocity.  Not part of gpu_parallel_duration_us.
    profile_file: after the last step, also write the radial profile of the final state (BarnesHutEngine.radial_profile) in
    profile_bins bins, profile_spacing "log" or "linear", over profile_range = (rmin, rmax) about profile_centre ("density",
    "com" or a pair); range None: out to just beyond the farthest body, from 0 (linear) or a thousandth of that (log): the line
    `# r_lo,r_hi,count,sigma,vr,vt,sigma_r,sigma_t`, then one row per bin (%.17g; nan in a bin without mass).  Not part of
    gpu_parallel_duration_us.
    lagrange_file: also write the Lagrangian radii of the state (BarnesHutEngine.lagrangian_radii(lagrange_fractions,
    lagrange_centre)) with the cadence rules of energy_file (lagrange_every), one line each: `step,t,cx,cy,r_f1,...` (%.17g).
    Not part of gpu_parallel_duration_us.
    pairs_file: after the last step, also write the pair-separation counts of the final state (BarnesHutEngine.pair_counts) in
    pairs_bins bins, pairs_spacing "log" or "linear", over pairs_range = (rmin, rmax): the line `# r_lo,r_hi,dd`, then one row
    per bin.  With pairs_randoms = NR points drawn uniformly in the bounding box of the final positions from
    np.random.default_rng(pairs_seed), also their cross counts and the Davis-Peebles correlation
    (BarnesHutEngine.correlation): `# r_lo,r_hi,dd,dr,xi` (%.17g; nan where dr = 0).  Not part of gpu_parallel_duration_us.
    mst_file: after the last step, also write the minimum spanning tree of the final state (BarnesHutEngine.spanning_tree): the
    line `# i,j,length`, then one row per edge (%.17g), ascending in the edge order (d2, i, j).  Not part of
    gpu_parallel_duration_us.
    segregation_file: after the last step, also write the mass segregation ratio of the final state
    (BarnesHutEngine.mass_segregation(segregation_massive, segregation_random, segregation_seed)): the line
    `# k,ratio,sigma,l_massive,l_random_mean` and one row (%.17g).  Not part of gpu_parallel_duration_us.
    binaries_file: after the last step, also write the bound pairs of the final state
    (BarnesHutEngine.binaries(binaries_separation)): the line `# i,j,r,a,e,period,binding_energy`, then one row per mutual pair
    (%.17g), ascending in i: the two body indices, their separation, the semi-major axis, the eccentricity, the period and the
    binding energy -- Keplerian, whatever the softening, of the state as it is (with integrator "kdk" velocities and positions
    are at the same time).  Not part of gpu_parallel_duration_us.
    encounters_file: after the last step, also write the close pairs of the final state
    (BarnesHutEngine.neighbours_within(encounters_radius).pairs()): the line `# i,j,r`, then one row per pair of bodies no
    farther apart than encounters_radius (%.17g), i < j, ascending in (i, j): the two body indices and their separation
    sqrt(d2).  Not part of gpu_parallel_duration_us.
    modes_file: after the last step, also write the azimuthal Fourier modes of the final state
    (BarnesHutEngine.azimuthal_modes(edges, modes_max, modes_centre)) in modes_bins bins, modes_spacing "log" or "linear", over
    modes_range (None: as profile_range): the line `# r_lo,r_hi,count,mass,amp_1,phase_1,...,amp_M,phase_M`, then one row per
    bin (%.17g; nan in a bin without mass).  Not part of gpu_parallel_duration_us.
    bar_file: also write the strength of harmonic bar_mode of the state with the cadence rules of energy_file (bar_every), one
    line each: `step,t,cx,cy,amplitude,phase,pattern_speed` (%.17g) -- BarnesHutEngine.azimuthal_modes(..., rates=True)
    .total(bar_mode) of the one bin over bar_range = (rmin, rmax) about bar_centre (range None: from 0 out to just beyond the
    farthest body); velocities relative to a centre at rest.  Not part of gpu_parallel_duration_us.
    curve_file: after the last step and every other output, one BarnesHutEngine.compute_forces() of the final state and its
    rotation curve (BarnesHutEngine.rotation_curve, radial_profile and toomre_q_from about curve_centre) in curve_bins bins
    (at most 1,022), curve_spacing "log" or "linear", over curve_range (None: as profile_range): the line
    `# r_lo,r_hi,count,r,vc,omega,kappa,sigma_r,q,torque`, then one row per bin (%.17g; nan where a number is not defined).
    Not part of gpu_parallel_duration_us.
    softening: Plummer softening length (BarnesHutEngine.set_softening) of the forces and of every diagnostic above; 0 is
    the reference's unsoftened law, the only one Precision.F64_EXACT takes.
    integrator: "euler" is the reference's fused kick-drift (BarnesHutEngine.step); "kdk" runs every batch between two
    outputs as one BarnesHutEngine.step_kdk, so every line of the energy, force-error and positions files, and the state
    returned, has velocities and positions at the same time."""
    if groups_file is not None and linking_length is None:
        raise ValueError("groups_file needs a linking_length")
    if (segregation_file is None) != (segregation_massive is None):
        raise ValueError("segregation_file and segregation_massive go together")
    if (binaries_file is None) != (binaries_separation is None):
        raise ValueError("binaries_file and binaries_separation go together")
    if (encounters_file is None) != (encounters_radius is None):
        raise ValueError("encounters_file and encounters_radius go together")
    if integrator not in ("euler", "kdk"):
        raise ValueError("integrator must be 'euler' or 'kdk'")
    if (profile_file is None) != (profile_bins is None):
        raise ValueError("profile_file and profile_bins go together")
    if pairs_file is not None and (pairs_bins is None or pairs_range is None):
        raise ValueError("pairs_file needs pairs_bins and pairs_range")
    if (modes_file is None) != (modes_bins is None):
        raise ValueError("modes_file and modes_bins go together")
    if (curve_file is None) != (curve_bins is None):
        raise ValueError("curve_file and curve_bins go together")
    n = len(masses)
    # both files are opened (truncated) up front, as the reference's ofstreams are (project.cu:928-929)
    init_path = os.path.join(out_dir, "quadtree_init_gpu.txt")
    final_path = os.path.join(out_dir, "quadtree_final_gpu.txt")
    open(init_path, "w").close()
    open(final_path, "w").close()

    gpu_parallel_us = 0.0
    with BarnesHutEngine(BhConfig(capacity=max(n, 1), theta=theta, G=g, dt=delta_t, max_depth=max_depth,
                                  precision=precision, reference_compat=reference_compat,
                                  device=device, n_threads=n_threads, softening=softening)) as eng:
        eng.upload(positions, velocities, masses)
        traj = None
        absolute_t = 0.0
        if positions_file is not None:
            traj = open(os.path.join(out_dir, positions_file) if not os.path.isabs(positions_file) else positions_file, "w")
            _write_frame(traj, absolute_t, np.asarray(positions, dtype=np.float64))
        energy = None
        if energy_file is not None:
            energy = open(os.path.join(out_dir, energy_file) if not os.path.isabs(energy_file) else energy_file, "w")
        ferr = None
        if force_error_file is not None:
            ferr = open(os.path.join(out_dir, force_error_file) if not os.path.isabs(force_error_file) else force_error_file, "w")
            ferr_targets = sample_targets(n, force_error_sample)
        lagrange = None
        if lagrange_file is not None:
            lagrange = open(os.path.join(out_dir, lagrange_file) if not os.path.isabs(lagrange_file) else lagrange_file, "w")
        bar = None
        if bar_file is not None:
            bar = open(os.path.join(out_dir, bar_file) if not os.path.isabs(bar_file) else bar_file, "w")
        done = 0
        # (file, steps between its lines, what writes a line)
        samplers = []

        def sample_energy():
            e = eng.energy()
            energy.write(",".join([str(done)] + ["%.17g" % v for v in (done * delta_t, e.kinetic, e.potential, e.total,
                                                                       e.momentum[0], e.momentum[1], e.angular_momentum)]) + "\n")

        def sample_force_error():
            r = eng.force_error(targets=ferr_targets)
            ferr.write(",".join([str(done), "%.17g" % (done * delta_t), str(r.n)]
                                + ["%.17g" % v for v in (r.median, r.p90, r.p99, r.p999, r.max)] + [str(r.worst)]) + "\n")

        def sample_lagrange():
            lr = eng.lagrangian_radii(lagrange_fractions, lagrange_centre)
            lagrange.write(",".join([str(done)] + ["%.17g" % v for v in (done * delta_t, *lr.centre, *lr.r)]) + "\n")

        def sample_bar():
            centre = eng.centre_of(bar_centre)
            edges = profile_edges(1, bar_range, "linear", eng.download()[0] if bar_range is None else None, centre)
            t = eng.azimuthal_modes(edges, bar_mode, centre, rates=True).total(bar_mode)
            bar.write(",".join([str(done)] + ["%.17g" % v for v in (done * delta_t, *centre, t.amplitude, t.phase, t.pattern_speed)]) + "\n")

        if energy is not None:
            samplers.append((energy_every, sample_energy))
        if ferr is not None:
            samplers.append((force_error_every, sample_force_error))
        if lagrange is not None:
            samplers.append((lagrange_every, sample_lagrange))
        if bar is not None:
            samplers.append((bar_every, sample_bar))

        advance_engine = eng.step if integrator == "euler" else eng.step_kdk

        def steps(k):
            nonlocal gpu_parallel_us, absolute_t
            if k <= 0:
                return
            if traj is None:
                advance_engine(k)
                gpu_parallel_us += eng.stats().last_step_ms * k * 1e3
                return
            for _ in range(k):
                advance_engine(1)
                gpu_parallel_us += eng.stats().last_step_ms * 1e3
                absolute_t += delta_t
                _write_frame(traj, absolute_t, eng.download()[0])

        def advance(k):
            # (with an energy or force-error file: batches that end at the sampled steps)
            nonlocal done
            while k > 0:
                j = k
                for every, _ in samplers:
                    if every > 0:
                        j = min(j, every - done % every)
                steps(j)
                done += j
                k -= j
                for every, write in samplers:
                    if done == n_simulations or (every > 0 and done % every == 0):
                        write()

        for _, write in samplers:
            write()

        step = 0
        while step < n_simulations:
            if step == 0:
                eng.build_tree()
                eng.write_quadtree_file(init_path)
                advance(1)
                step += 1
            elif step == n_simulations - 1:
                eng.build_tree()
                eng.write_quadtree_file(final_path)
                advance(1)
                step += 1
            else:
                k = n_simulations - 1 - step
                advance(k)
                step += k
        pos, vel = eng.download()
        if field_file is not None:
            pts = field_grid_points(field_grid, field_box, pos)
            acc, phi = eng.field(pts)
            with open(os.path.join(out_dir, field_file) if not os.path.isabs(field_file) else field_file, "w") as f:
                f.write("# x,y,ax,ay,phi\n")
                f.write("".join("%.17g,%.17g,%.17g,%.17g,%.17g\n" % (x, y, a[0], a[1], q) for (x, y), a, q in zip(pts, acc, phi)))
        if density_file is not None:
            pts = field_grid_points(density_grid, density_box, pos)
            box = density_box if density_box is not None else (pos[:, 0].min(), pos[:, 0].max(), pos[:, 1].min(), pos[:, 1].max())
            mm = eng.moment_map(box, int(density_grid[0]), int(density_grid[1]), density_scheme)
            cols = [a.reshape(-1) for a in (mm.sigma, mm.vx, mm.vy, mm.dispersion)]
            with open(os.path.join(out_dir, density_file) if not os.path.isabs(density_file) else density_file, "w") as f:
                f.write("# x,y,sigma,vx,vy,dispersion\n")
                f.write("".join("%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n" % (x, y, *r) for (x, y), r in zip(pts, zip(*cols))))
        if neighbours_file is not None:
            sigma, r_k = eng.local_density(neighbours_k)
            with open(os.path.join(out_dir, neighbours_file) if not os.path.isabs(neighbours_file) else neighbours_file, "w") as f:
                f.write("# i,x,y,r_k,sigma\n")
                f.write("".join("%d,%.17g,%.17g,%.17g,%.17g\n" % (i, x, y, r, sg) for i, ((x, y), r, sg) in enumerate(zip(pos, r_k, sigma))))
        if groups_file is not None:
            g = eng.groups(linking_length, groups_min)
            with open(os.path.join(out_dir, groups_file) if not os.path.isabs(groups_file) else groups_file, "w") as f:
                f.write("# id,count,mass,x,y,vx,vy\n")
                f.write("".join("%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n" % (i, k, m, x, y, vx, vy)
                                for i, k, m, (x, y), (vx, vy) in zip(g.id, g.count, g.mass, g.com, g.velocity)))
        if profile_file is not None:
            centre = eng.centre_of(profile_centre)
            prof = eng.radial_profile(profile_edges(profile_bins, profile_range, profile_spacing, pos, centre), centre)
            cols = (prof.edges[:-1], prof.edges[1:], prof.count, prof.sigma, prof.vr, prof.vt, prof.sigma_r, prof.sigma_t)
            with open(os.path.join(out_dir, profile_file) if not os.path.isabs(profile_file) else profile_file, "w") as f:
                f.write("# r_lo,r_hi,count,sigma,vr,vt,sigma_r,sigma_t\n")
                f.write("".join("%.17g,%.17g,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n" % r for r in zip(*cols)))
        if modes_file is not None:
            centre = eng.centre_of(modes_centre)
            md = eng.azimuthal_modes(profile_edges(modes_bins, modes_range, modes_spacing, pos, centre), modes_max, centre)
            cols = [md.edges[:-1], md.edges[1:], md.count, md.mass]
            for k in range(1, md.m_max + 1):
                cols += [md.amplitude[k], md.phase[k]]
            with open(os.path.join(out_dir, modes_file) if not os.path.isabs(modes_file) else modes_file, "w") as f:
                f.write("# r_lo,r_hi,count,mass" + "".join(",amp_%d,phase_%d" % (k, k) for k in range(1, md.m_max + 1)) + "\n")
                f.write("".join(("%.17g,%.17g,%d" + ",%.17g" * (1 + 2 * md.m_max) + "\n") % r for r in zip(*cols)))
        if pairs_file is not None:
            edges = radial_edges(float(pairs_range[0]), float(pairs_range[1]), int(pairs_bins), pairs_spacing)
            with open(os.path.join(out_dir, pairs_file) if not os.path.isabs(pairs_file) else pairs_file, "w") as f:
                if pairs_randoms is None:
                    dd = eng.pair_counts(edges)
                    f.write("# r_lo,r_hi,dd\n")
                    f.write("".join("%.17g,%.17g,%d\n" % r for r in zip(dd.edges[:-1], dd.edges[1:], dd.counts)))
                else:
                    xi, dd, dr = eng.correlation(edges, pairs_random_points(pos, pairs_randoms, pairs_seed))
                    f.write("# r_lo,r_hi,dd,dr,xi\n")
                    f.write("".join("%.17g,%.17g,%d,%d,%.17g\n" % r for r in zip(dd.edges[:-1], dd.edges[1:], dd.counts, dr.counts, xi)))
        if mst_file is not None:
            t = eng.spanning_tree()
            with open(os.path.join(out_dir, mst_file) if not os.path.isabs(mst_file) else mst_file, "w") as f:
                f.write("# i,j,length\n")
                f.write("".join("%d,%d,%.17g\n" % r for r in zip(t.lo, t.hi, t.length)))
        if segregation_file is not None:
            ms = eng.mass_segregation(segregation_massive, segregation_random, segregation_seed)
            with open(os.path.join(out_dir, segregation_file) if not os.path.isabs(segregation_file) else segregation_file, "w") as f:
                f.write("# k,ratio,sigma,l_massive,l_random_mean\n")
                f.write("%d,%.17g,%.17g,%.17g,%.17g\n" % (ms.n_massive, ms.ratio, ms.sigma, ms.l_massive,
                                                          math.fsum(ms.l_random.tolist()) / len(ms.l_random)))
        if binaries_file is not None:
            b = eng.binaries(binaries_separation)
            with open(os.path.join(out_dir, binaries_file) if not os.path.isabs(binaries_file) else binaries_file, "w") as f:
                f.write("# i,j,r,a,e,period,binding_energy\n")
                f.write("".join("%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n" % r for r in zip(b.lo, b.hi, b.separation, b.semi_major_axis,
                                                                                    b.eccentricity, b.period, b.binding_energy)))
        if encounters_file is not None:
            lo, hi, d2 = eng.neighbours_within(encounters_radius).pairs()
            with open(os.path.join(out_dir, encounters_file) if not os.path.isabs(encounters_file) else encounters_file, "w") as f:
                f.write("# i,j,r\n")
                f.write("".join("%d,%d,%.17g\n" % r for r in zip(lo, hi, np.sqrt(d2))))
        if curve_file is not None:                                  # (last: its force walk may re-order the state in memory)
            centre = eng.centre_of(curve_centre)
            edges = profile_edges(curve_bins, curve_range, curve_spacing, pos, centre)
            eng.compute_forces()
            rc, prof = eng.rotation_curve(edges, centre), eng.radial_profile(edges, centre)
            cols = (rc.edges[:-1], rc.edges[1:], rc.count, rc.radius, rc.vc, rc.omega, rc.kappa, prof.sigma_r, toomre_q_from(rc, prof, g),
                    rc.torque)
            with open(os.path.join(out_dir, curve_file) if not os.path.isabs(curve_file) else curve_file, "w") as f:
                f.write("# r_lo,r_hi,count,r,vc,omega,kappa,sigma_r,q,torque\n")
                f.write("".join("%.17g,%.17g,%d,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n" % r for r in zip(*cols)))
        if traj is not None:
            traj.close()
        for f in (energy, ferr, lagrange, bar):
            if f is not None:
                f.close()
    return pos, vel, gpu_parallel_us


def field_grid_points(grid, box, positions) -> np.ndarray:
    """The (NX * NY, 2) cell centres of the NX x NY grid over box = (xmin, xmax, ymin, ymax) in row-major order, y the
    outer axis; box None: the bounding box of `positions`."""
    nx, ny = (int(g) for g in grid)
    if nx < 1 or ny < 1:
        raise ValueError("the field grid needs at least one cell per axis")
    if box is None:
        p = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
        if len(p) == 0:
            raise ValueError("no bodies: give the field box")
        box = (p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max())
    x0, x1, y0, y1 = (float(b) for b in box)
    xs = x0 + (np.arange(nx) + 0.5) * ((x1 - x0) / nx)
    ys = y0 + (np.arange(ny) + 0.5) * ((y1 - y0) / ny)
    return np.stack([np.tile(xs, ny), np.repeat(ys, nx)], axis=1)


def pairs_random_points(positions, n_random: int, seed: int = 0) -> np.ndarray:
    """The (n_random, 2) points of --pairs-randoms: uniform in the bounding box of `positions` from np.random.default_rng(seed)."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
    if len(p) == 0 or n_random < 1:
        raise ValueError("random points need bodies to bound them and n_random >= 1")
    lo, hi = p.min(axis=0), p.max(axis=0)
    return lo + (hi - lo) * np.random.default_rng(seed).random((int(n_random), 2))


def profile_edges(bins: int, rng, spacing: str, positions, centre) -> np.ndarray:
    """The bins + 1 edges of --profile-file over rng = (rmin, rmax); None: out to just beyond the farthest body from `centre`,
    from 0 ("linear") or a thousandth of that ("log")."""
    if rng is None:
        p = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
        if len(p) == 0:
            raise ValueError("no bodies: give the profile range")
        r_max = float(np.nextafter(np.sqrt(((p - np.asarray(centre, dtype=np.float64)) ** 2).sum(axis=1).max()), np.inf))
        rng = (0.0 if spacing == "linear" else 1e-3 * r_max, r_max)
    return radial_edges(float(rng[0]), float(rng[1]), int(bins), spacing)


def _centre_arg(ap, flag: str, words):
    """"density", "com" or two numbers."""
    if words is None:
        return "density"
    if len(words) == 1 and words[0] in ("density", "com"):
        return words[0]
    try:
        if len(words) == 2:
            return (float(words[0]), float(words[1]))
    except ValueError:
        pass
    ap.error(f"{flag}: density, com, or X Y")


def _write_frame(f, t: float, pos) -> None:
    """One savePositions call (project.cu:855-863): std::to_string formatting is "%f"."""
    f.write("".join("%f %d %f %f \n" % (t, i, x, y) for i, (x, y) in enumerate(pos)))


def _parse(argv):
    ap = argparse.ArgumentParser(prog="project", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-D", action="append", default=[], metavar="NAME=VALUE",
                    help="N_BODIES / N_THREADS / N_SIMULATIONS, as on the reference's nvcc line")
    ap.add_argument("--n-bodies", type=int)
    ap.add_argument("--n-threads", type=int)
    ap.add_argument("--n-simulations", type=int)
    ap.add_argument("--init", choices=["auto", "files", "random", "gpu", "disc"], default="auto",
                    help="files: loadSimulationDataFromText from the CWD; random: initializeCpu; "
                         "gpu: initializeGpu (on-device generator); auto: files when masses_init.txt "
                         "exists, else gpu -- the reference as shipped calls initializeGpu; disc: an on-device "
                         "Kuzmin-Toomre disc in equilibrium (--disc-mass, --disc-scale, --disc-rmax, --disc-q)")
    ap.add_argument("--disc-mass", type=float, default=None, metavar="M", help="total mass of --init disc (default 1)")
    ap.add_argument("--disc-scale", type=float, default=None, metavar="A", help="scale length of --init disc (default 0.02)")
    ap.add_argument("--disc-rmax", type=float, default=None, metavar="R", help="truncation radius of --init disc (default 0.2; inf: none)")
    ap.add_argument("--disc-q", type=float, default=None, metavar="Q", help="Toomre's Q of --init disc (default 1.5)")
    ap.add_argument("--curve-file", default=None, metavar="PATH",
                    help="also write r_lo,r_hi,count,r,vc,omega,kappa,sigma_r,q,torque (the rotation curve of the final state's own "
                         "forces, with Toomre's Q and the gravitational torque) of the --curve-bins radial bins about --curve-centre")
    ap.add_argument("--curve-bins", type=int, default=None, metavar="NB", help="bins of --curve-file (1 .. 1022)")
    ap.add_argument("--curve-range", type=float, nargs=2, default=None, metavar=("RMIN", "RMAX"),
                    help="range of --curve-file (default: out to just beyond the farthest body)")
    ap.add_argument("--curve-spacing", choices=["log", "linear"], default="log", help="spacing of the bin edges")
    ap.add_argument("--curve-centre", nargs="+", default=None, metavar="C", help="density (default), com or X Y")
    ap.add_argument("--positions-file", default=None, help="also write the trajectory (savePositions format)")
    ap.add_argument("--energy-file", default=None, metavar="PATH",
                    help="also write step,t,kinetic,potential,total,px,py,Lz before the first step, every "
                         "--energy-every steps and after the last")
    ap.add_argument("--energy-every", type=int, default=0, metavar="K",
                    help="steps between two lines of --energy-file (0: first and last state only)")
    ap.add_argument("--force-error-file", default=None, metavar="PATH",
                    help="also write step,t,n,median,p90,p99,p999,max,worst (Barnes-Hut force error against the direct "
                         "sum) before the first step, every --force-error-every steps and after the last")
    ap.add_argument("--force-error-every", type=int, default=0, metavar="K",
                    help="steps between two lines of --force-error-file (0: first and last state only)")
    ap.add_argument("--force-error-sample", type=int, default=65536, metavar="S",
                    help="bodies in the force-error sample (drawn once; all bodies when S >= N_BODIES)")
    ap.add_argument("--field-file", default=None, metavar="PATH",
                    help="after the last step, also write x,y,ax,ay,phi of the Barnes-Hut field on the --field-grid")
    ap.add_argument("--field-grid", type=int, nargs=2, default=None, metavar=("NX", "NY"),
                    help="cells of the cell-centred grid of --field-file (row-major rows, y the outer axis)")
    ap.add_argument("--field-box", type=float, nargs=4, default=None, metavar=("XMIN", "XMAX", "YMIN", "YMAX"),
                    help="what the grid covers (default: the bounding box of the final positions)")
    ap.add_argument("--density-file", default=None, metavar="PATH",
                    help="after the last step, also write x,y,sigma,vx,vy,dispersion (surface density, mean velocity, velocity "
                         "dispersion) of the cells of the --density-grid")
    ap.add_argument("--density-grid", type=int, nargs=2, default=None, metavar=("NX", "NY"),
                    help="cells of --density-file (rows of cell centres, y the outer axis: the points of --field-grid)")
    ap.add_argument("--density-box", type=float, nargs=4, default=None, metavar=("XMIN", "XMAX", "YMIN", "YMAX"),
                    help="what the cells cover (default: the bounding box of the final positions, as --field-box)")
    ap.add_argument("--density-scheme", choices=["ngp", "cic"], default="cic",
                    help="ngp: a body goes to the cell it is in; cic: to the four nearest cell centres, bilinearly")
    ap.add_argument("--neighbours-file", default=None, metavar="PATH",
                    help="after the last step, also write i,x,y,r_k,sigma of every body: the distance of its k-th neighbour and "
                         "the k-th-neighbour surface density (Casertano and Hut)")
    ap.add_argument("--neighbours-k", type=int, default=None, metavar="K", help="the k of --neighbours-file (default 6; 2 .. 32)")
    ap.add_argument("--groups-file", default=None, metavar="PATH",
                    help="after the last step, also write id,count,mass,x,y,vx,vy of every friends-of-friends group of the final "
                         "state (needs --linking-length)")
    ap.add_argument("--linking-length", type=float, default=None, metavar="B",
                    help="bodies at most B apart are friends; a group is a connected component of that relation")
    ap.add_argument("--groups-min", type=int, default=None, metavar="M", help="smallest group of --groups-file (default 2)")
    ap.add_argument("--profile-file", default=None, metavar="PATH",
                    help="after the last step, also write r_lo,r_hi,count,sigma,vr,vt,sigma_r,sigma_t (surface density, mean radial "
                         "and tangential velocity and their dispersions) of the --profile-bins radial bins about --profile-centre")
    ap.add_argument("--profile-bins", type=int, default=None, metavar="NB", help="bins of --profile-file (1 .. 4096)")
    ap.add_argument("--profile-range", type=float, nargs=2, default=None, metavar=("RMIN", "RMAX"),
                    help="what the bins cover (default: out to the farthest body, from 0 (linear) or a thousandth of that (log))")
    ap.add_argument("--profile-spacing", choices=["log", "linear"], default="log", help="spacing of the bin edges")
    ap.add_argument("--profile-centre", nargs="+", default=None, metavar="C",
                    help="density (the density centre, default), com (the centre of mass) or X Y")
    ap.add_argument("--modes-file", default=None, metavar="PATH",
                    help="also write r_lo,r_hi,count,mass,amp_1,phase_1,...,amp_M,phase_M (the azimuthal Fourier modes of the final "
                         "state: relative amplitude and phase per harmonic) of the --modes-bins radial bins about --modes-centre")
    ap.add_argument("--modes-bins", type=int, default=None, metavar="NB", help="bins of --modes-file (1 .. 4096)")
    ap.add_argument("--modes-max", type=int, default=None, metavar="M", help="highest harmonic of --modes-file (0 .. 16, default 4)")
    ap.add_argument("--modes-range", type=float, nargs=2, default=None, metavar=("RMIN", "RMAX"),
                    help="radii of the first and the last edge (default: as --profile-range)")
    ap.add_argument("--modes-spacing", choices=["log", "linear"], default="log", help="spacing of the bin edges")
    ap.add_argument("--modes-centre", nargs="+", default=None, metavar="C", help="density (default), com or X Y")
    ap.add_argument("--bar-file", default=None, metavar="PATH",
                    help="also write step,t,cx,cy,amplitude,phase,pattern_speed (harmonic --bar-mode of the whole --bar-range: the "
                         "bar strength) before the first step, every --bar-every steps and after the last")
    ap.add_argument("--bar-mode", type=int, default=None, metavar="K", help="harmonic of --bar-file (1 .. 16, default 2)")
    ap.add_argument("--bar-every", type=int, default=0, metavar="N",
                    help="steps between two lines of --bar-file (0: first and last state only)")
    ap.add_argument("--bar-range", type=float, nargs=2, default=None, metavar=("RMIN", "RMAX"),
                    help="radii between which the bodies count (default: from 0 to just beyond the farthest body)")
    ap.add_argument("--bar-centre", nargs="+", default=None, metavar="C", help="density (default), com or X Y")
    ap.add_argument("--lagrange-file", default=None, metavar="PATH",
                    help="also write step,t,cx,cy,r_f1,... (the centre and the radii that enclose the --lagrange-fractions of the "
                         "mass) before the first step, every --lagrange-every steps and after the last")
    ap.add_argument("--lagrange-fractions", type=float, nargs="+", default=None, metavar="F",
                    help="mass fractions in (0, 1] (default 0.01 0.1 0.5 0.9; at most 32)")
    ap.add_argument("--lagrange-every", type=int, default=0, metavar="K",
                    help="steps between two lines of --lagrange-file (0: first and last state only)")
    ap.add_argument("--lagrange-centre", nargs="+", default=None, metavar="C", help="density (default), com or X Y")
    ap.add_argument("--pairs-file", default=None, metavar="PATH",
                    help="after the last step, also write r_lo,r_hi,dd (the pairs of bodies per separation bin) of the final state; "
                         "with --pairs-randoms also dr and the Davis-Peebles correlation xi (needs --pairs-bins and --pairs-range)")
    ap.add_argument("--pairs-bins", type=int, default=None, metavar="NB", help="bins of --pairs-file (1 .. 1024)")
    ap.add_argument("--pairs-range", type=float, nargs=2, default=None, metavar=("RMIN", "RMAX"), help="the separations the bins cover")
    ap.add_argument("--pairs-spacing", choices=["log", "linear"], default=None, help="spacing of the bin edges (default log)")
    ap.add_argument("--pairs-randoms", type=int, default=None, metavar="NR",
                    help="random points, uniform in the bounding box of the final positions, for dr and xi")
    ap.add_argument("--pairs-seed", type=int, default=None, metavar="S", help="seed of --pairs-randoms (default 0)")
    ap.add_argument("--mst-file", default=None, metavar="PATH",
                    help="after the last step, also write i,j,length of every edge of the minimum spanning tree of the final state")
    ap.add_argument("--segregation-file", default=None, metavar="PATH",
                    help="after the last step, also write k,ratio,sigma,l_massive,l_random_mean: the mass segregation ratio of the "
                         "final state (needs --segregation-massive)")
    ap.add_argument("--segregation-massive", type=int, default=None, metavar="K", help="the K most massive bodies (2 .. 512)")
    ap.add_argument("--segregation-random", type=int, default=None, metavar="R", help="random sets of K bodies (default 500)")
    ap.add_argument("--segregation-seed", type=int, default=None, metavar="S", help="seed of the random sets (default 0)")
    ap.add_argument("--binaries-file", default=None, metavar="PATH",
                    help="after the last step, also write i,j,r,a,e,period,binding_energy of every bound pair of the final state "
                         "(needs --binaries-separation)")
    ap.add_argument("--binaries-separation", type=float, default=None, metavar="R",
                    help="largest separation of a pair's two bodies (> 0; inf: no cut)")
    ap.add_argument("--encounters-file", default=None, metavar="PATH",
                    help="after the last step, also write i,j,r of every pair of bodies of the final state no farther apart than "
                         "--encounters-radius")
    ap.add_argument("--encounters-radius", type=float, default=None, metavar="R", help="largest separation of a close pair (>= 0)")
    ap.add_argument("--save-init", action="store_true", help="write the three init files after initialisation")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", choices=["f64", "f32"], default="f64")
    ap.add_argument("--max-depth", type=int, default=QUADTREE_MAX_DEPTH)
    ap.add_argument("--theta", type=float, default=THETA)
    ap.add_argument("--no-compat", action="store_true", help="bucket leaves instead of the depth-cap artefact")
    ap.add_argument("--softening", type=float, default=None, metavar="EPS",
                    help="Plummer softening length of the forces and diagnostics (needs --precision f32: the default "
                         "precision reproduces the reference bit for bit, and the reference has no softening)")
    ap.add_argument("--integrator", choices=["euler", "kdk"], default="euler",
                    help="euler: the reference's fused kick-drift; kdk: synchronised kick-drift-kick leapfrog, one "
                         "step_kdk per batch between two outputs")
    ap.add_argument("-o", dest="ignored_output", help="accepted and ignored (nvcc line compatibility)")
    ap.add_argument("source", nargs="?", help="accepted and ignored (nvcc line compatibility)")
    a = ap.parse_args(argv)
    if (a.field_file is None) != (a.field_grid is None):
        ap.error("--field-file and --field-grid go together")
    if a.field_box is not None and a.field_file is None:
        ap.error("--field-box needs --field-file")
    if (a.density_file is None) != (a.density_grid is None):
        ap.error("--density-file and --density-grid go together")
    if a.density_box is not None and a.density_file is None:
        ap.error("--density-box needs --density-file")
    if a.neighbours_k is not None and a.neighbours_file is None:
        ap.error("--neighbours-k needs --neighbours-file")
    if a.neighbours_k is not None and not 2 <= a.neighbours_k <= 32:
        ap.error("--neighbours-k: 2 .. 32")
    if (a.groups_file is None) != (a.linking_length is None):
        ap.error("--groups-file and --linking-length go together")
    if a.groups_min is not None and a.groups_file is None:
        ap.error("--groups-min needs --groups-file")
    if (a.profile_file is None) != (a.profile_bins is None):
        ap.error("--profile-file and --profile-bins go together")
    if a.profile_file is None and (a.profile_range is not None or a.profile_centre is not None):
        ap.error("--profile-range and --profile-centre need --profile-file")
    if a.profile_bins is not None and not 1 <= a.profile_bins <= 4096:
        ap.error("--profile-bins: 1 .. 4096")
    if a.profile_range is not None and not (0.0 <= a.profile_range[0] < a.profile_range[1] < float("inf")):
        ap.error("--profile-range: 0 <= RMIN < RMAX, finite")
    if a.profile_range is not None and a.profile_spacing == "log" and a.profile_range[0] <= 0.0:
        ap.error("--profile-range: log spacing needs RMIN > 0")
    if (a.modes_file is None) != (a.modes_bins is None):
        ap.error("--modes-file and --modes-bins go together")
    if a.modes_file is None and (a.modes_range is not None or a.modes_centre is not None or a.modes_max is not None):
        ap.error("--modes-max, --modes-range and --modes-centre need --modes-file")
    if a.modes_bins is not None and not 1 <= a.modes_bins <= 4096:
        ap.error("--modes-bins: 1 .. 4096")
    if a.modes_max is not None and not 0 <= a.modes_max <= 16:
        ap.error("--modes-max: 0 .. 16")
    for flag, rng in (("--modes-range", a.modes_range), ("--bar-range", a.bar_range)):
        if rng is not None and not (0.0 <= rng[0] < rng[1] < float("inf")):
            ap.error(flag + ": 0 <= RMIN < RMAX, finite")
    if a.modes_range is not None and a.modes_spacing == "log" and a.modes_range[0] <= 0.0:
        ap.error("--modes-range: log spacing needs RMIN > 0")
    if a.init != "disc" and any(v is not None for v in (a.disc_mass, a.disc_scale, a.disc_rmax, a.disc_q)):
        ap.error("--disc-mass, --disc-scale, --disc-rmax and --disc-q need --init disc")
    if a.disc_mass is not None and not math.isfinite(a.disc_mass):
        ap.error("--disc-mass: finite")
    if a.disc_scale is not None and not (0.0 < a.disc_scale < math.inf):
        ap.error("--disc-scale: finite and > 0")
    if a.disc_rmax is not None and not a.disc_rmax > 0.0:
        ap.error("--disc-rmax: > 0 (inf: no truncation)")
    if a.disc_q is not None and not (0.0 <= a.disc_q < math.inf):
        ap.error("--disc-q: finite and >= 0")
    if (a.curve_file is None) != (a.curve_bins is None):
        ap.error("--curve-file and --curve-bins go together")
    if a.curve_file is None and (a.curve_range is not None or a.curve_centre is not None):
        ap.error("--curve-range and --curve-centre need --curve-file")
    if a.curve_bins is not None and not 1 <= a.curve_bins <= 1022:
        ap.error("--curve-bins: 1 .. 1022")
    if a.curve_range is not None and not (0.0 <= a.curve_range[0] < a.curve_range[1] < float("inf")):
        ap.error("--curve-range: 0 <= RMIN < RMAX, finite")
    if a.curve_range is not None and a.curve_spacing == "log" and a.curve_range[0] <= 0.0:
        ap.error("--curve-range: log spacing needs RMIN > 0")
    if a.bar_file is None and (a.bar_mode is not None or a.bar_every or a.bar_range is not None or a.bar_centre is not None):
        ap.error("--bar-mode, --bar-every, --bar-range and --bar-centre need --bar-file")
    if a.bar_mode is not None and not 1 <= a.bar_mode <= 16:
        ap.error("--bar-mode: 1 .. 16")
    if a.bar_every < 0:
        ap.error("--bar-every: at least 0")
    if a.lagrange_file is None and (a.lagrange_fractions is not None or a.lagrange_centre is not None or a.lagrange_every):
        ap.error("--lagrange-fractions, --lagrange-every and --lagrange-centre need --lagrange-file")
    if a.lagrange_fractions is not None and (len(a.lagrange_fractions) > 32 or not all(0.0 < f <= 1.0 for f in a.lagrange_fractions)):
        ap.error("--lagrange-fractions: at most 32, each in (0, 1]")
    if a.pairs_file is not None and (a.pairs_bins is None or a.pairs_range is None):
        ap.error("--pairs-file needs --pairs-bins and --pairs-range")
    if a.pairs_file is None and any(v is not None for v in (a.pairs_bins, a.pairs_range, a.pairs_spacing, a.pairs_randoms, a.pairs_seed)):
        ap.error("--pairs-bins, --pairs-range, --pairs-spacing, --pairs-randoms and --pairs-seed need --pairs-file")
    if a.pairs_seed is not None and a.pairs_randoms is None:
        ap.error("--pairs-seed needs --pairs-randoms")
    if a.pairs_bins is not None and not 1 <= a.pairs_bins <= 1024:
        ap.error("--pairs-bins: 1 .. 1024")
    if a.pairs_range is not None and not (0.0 <= a.pairs_range[0] < a.pairs_range[1] < float("inf")):
        ap.error("--pairs-range: 0 <= RMIN < RMAX, finite")
    if a.pairs_range is not None and (a.pairs_spacing or "log") == "log" and a.pairs_range[0] <= 0.0:
        ap.error("--pairs-range: log spacing needs RMIN > 0")
    if a.pairs_randoms is not None and a.pairs_randoms < 1:
        ap.error("--pairs-randoms: at least 1")
    if (a.segregation_file is None) != (a.segregation_massive is None):
        ap.error("--segregation-file and --segregation-massive go together")
    if a.segregation_file is None and (a.segregation_random is not None or a.segregation_seed is not None):
        ap.error("--segregation-random and --segregation-seed need --segregation-file")
    if a.segregation_massive is not None and not 2 <= a.segregation_massive <= 512:
        ap.error("--segregation-massive: 2 .. 512")
    if a.segregation_random is not None and a.segregation_random < 1:
        ap.error("--segregation-random: at least 1")
    if (a.binaries_file is None) != (a.binaries_separation is None):
        ap.error("--binaries-file and --binaries-separation go together")
    if a.binaries_separation is not None and not a.binaries_separation > 0.0:
        ap.error("--binaries-separation: > 0")
    if (a.encounters_file is None) != (a.encounters_radius is None):
        ap.error("--encounters-file and --encounters-radius go together")
    if a.encounters_radius is not None and not (0.0 <= a.encounters_radius < math.inf):
        ap.error("--encounters-radius: finite and >= 0")
    a.profile_centre = _centre_arg(ap, "--profile-centre", a.profile_centre)
    a.lagrange_centre = _centre_arg(ap, "--lagrange-centre", a.lagrange_centre)
    a.modes_centre = _centre_arg(ap, "--modes-centre", a.modes_centre)
    a.bar_centre = _centre_arg(ap, "--bar-centre", a.bar_centre)
    a.curve_centre = _centre_arg(ap, "--curve-centre", a.curve_centre)
    if a.groups_min is not None and a.groups_min < 1:
        ap.error("--groups-min: at least 1")
    if a.linking_length is not None and not (a.linking_length >= 0.0 and a.linking_length < float("inf")):
        ap.error("--linking-length: the length must be finite and >= 0")
    if a.softening is not None:
        if not (a.softening >= 0.0 and a.softening < float("inf")):
            ap.error("--softening: the length must be finite and >= 0")
        if a.softening != 0.0 and a.precision == "f64":
            ap.error("--softening needs --precision f32: --precision f64 reproduces the reference's results bit for bit, "
                     "and the reference has no softening")
    # project.cu:1-11.  N_THREADS: the reference's default is 1,024 CUDA threads striding over the bodies; here it
    # caps the bodies walked at a time ONLY when given (-DN_THREADS=... / --n-threads, as the scaling scripts do):
    # unset, a step walks all bodies in one launch.
    macros = {"N_BODIES": 1000 * 40, "N_THREADS": 0, "N_SIMULATIONS": 10}
    for d in a.D:
        k, _, v = d.partition("=")
        if k not in macros:
            ap.error(f"unknown macro {k}")
        try:
            macros[k] = _macro_value(v)
        except ValueError:
            ap.error(f"-D{k}={v}: expected an integer or a product of integers (the reference writes `1000 * 40`)")
    if a.n_bodies is not None:
        macros["N_BODIES"] = a.n_bodies
    if a.n_threads is not None:
        macros["N_THREADS"] = a.n_threads
    if a.n_simulations is not None:
        macros["N_SIMULATIONS"] = a.n_simulations
    return a, macros


def _macro_value(text: str) -> int:
    """Value of a -D macro as the reference writes them (project.cu:1-11): an integer literal or a
    product of integer literals such as `1000 * 40`, optionally parenthesised.  Nothing is evaluated."""
    t = text.strip()
    while t.startswith("(") and t.endswith(")"):
        t = t[1:-1].strip()
    value = 1
    for factor in t.split("*"):
        value *= int(factor.strip(), 10)               # ValueError on anything but a decimal integer
    return value


def main(argv=None) -> int:
    a, mac = _parse(sys.argv[1:] if argv is None else argv)
    n = mac["N_BODIES"]
    use_files = a.init == "files" or (a.init == "auto" and os.path.exists("masses_init.txt"))
    if use_files:
        masses, positions, velocities = loadSimulationDataFromText(
            "masses_init.txt", "positions_init.txt", "velocities_init.txt", n, N_BODIES=n)
    elif a.init == "random":
        masses, positions, velocities = initializeCpu(n, seed=a.seed, save_to_file=a.save_init)
    elif a.init == "disc":
        masses, positions, velocities = initializeDisc(
            n, seed=a.seed, mass=1.0 if a.disc_mass is None else a.disc_mass, scale=0.02 if a.disc_scale is None else a.disc_scale,
            r_max=0.2 if a.disc_rmax is None else a.disc_rmax, q=1.5 if a.disc_q is None else a.disc_q,
            precision=Precision.F64_EXACT if a.precision == "f64" else Precision.F32, theta=a.theta, max_depth=a.max_depth,
            reference_compat=not a.no_compat, softening=a.softening or 0.0, save_to_file=a.save_init)
    else:
        masses, positions, velocities = initializeGpu(
            n, seed=a.seed, precision=Precision.F64_EXACT if a.precision == "f64" else Precision.F32,
            save_to_file=a.save_init)

    start = time.perf_counter()
    _, _, gpu_parallel_us = runSimulationGpu(
        masses, positions, velocities, mac["N_SIMULATIONS"], n_threads=mac["N_THREADS"],
        theta=a.theta, max_depth=a.max_depth,
        precision=Precision.F64_EXACT if a.precision == "f64" else Precision.F32,
        reference_compat=not a.no_compat, positions_file=a.positions_file, energy_file=a.energy_file,
        energy_every=a.energy_every, force_error_file=a.force_error_file, force_error_every=a.force_error_every,
        force_error_sample=a.force_error_sample, field_file=a.field_file, field_grid=a.field_grid, field_box=a.field_box,
        softening=a.softening or 0.0, integrator=a.integrator, density_file=a.density_file, density_grid=a.density_grid,
        density_box=a.density_box, density_scheme=a.density_scheme, neighbours_file=a.neighbours_file,
        neighbours_k=6 if a.neighbours_k is None else a.neighbours_k, groups_file=a.groups_file,
        linking_length=a.linking_length, groups_min=2 if a.groups_min is None else a.groups_min,
        profile_file=a.profile_file, profile_bins=a.profile_bins, profile_range=a.profile_range,
        profile_spacing=a.profile_spacing, profile_centre=a.profile_centre, lagrange_file=a.lagrange_file,
        lagrange_fractions=(0.01, 0.1, 0.5, 0.9) if a.lagrange_fractions is None else tuple(a.lagrange_fractions),
        lagrange_every=a.lagrange_every, lagrange_centre=a.lagrange_centre, pairs_file=a.pairs_file, pairs_bins=a.pairs_bins,
        pairs_range=a.pairs_range, pairs_spacing=a.pairs_spacing or "log", pairs_randoms=a.pairs_randoms,
        pairs_seed=a.pairs_seed or 0, mst_file=a.mst_file, segregation_file=a.segregation_file,
        segregation_massive=a.segregation_massive, segregation_random=500 if a.segregation_random is None else a.segregation_random,
        segregation_seed=a.segregation_seed or 0, binaries_file=a.binaries_file, binaries_separation=a.binaries_separation,
        encounters_file=a.encounters_file, encounters_radius=a.encounters_radius, modes_file=a.modes_file,
        modes_bins=a.modes_bins, modes_max=4 if a.modes_max is None else a.modes_max, modes_range=a.modes_range,
        modes_spacing=a.modes_spacing, modes_centre=a.modes_centre, bar_file=a.bar_file,
        bar_mode=2 if a.bar_mode is None else a.bar_mode, bar_every=a.bar_every, bar_range=a.bar_range, bar_centre=a.bar_centre,
        curve_file=a.curve_file, curve_bins=a.curve_bins, curve_range=a.curve_range, curve_spacing=a.curve_spacing,
        curve_centre=a.curve_centre)
    duration_ms = int((time.perf_counter() - start) * 1e3)

    # project.cu:1090-1102, blank lines included
    sys.stdout.write("\n\n")
    sys.stdout.write("\n\n")
    sys.stdout.write(f"GPU total computation took {duration_ms} milliseconds.\n")
    sys.stdout.write("\n\n")
    sys.stdout.write(f"GPU parallel computation took {int(gpu_parallel_us)} microseconds.\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
