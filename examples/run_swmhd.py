#!/usr/bin/env python3
"""The reference's two driver scripts as one command-line example of the host mirror (no plotting, no NetCDF/JLD2):

    python examples/run_swmhd.py --formulation jacobian   [--size 64] [--stop-time 30] [--dt 0.01] [--ic uniform|gaussians]
    python examples/run_swmhd.py --formulation divergence ...

Set-up as jacobian_formulation/SWMHD_example.jl:7-42 / divergence_formulation/divergence_sw_mhd.jl:7-40: [-5,5]^2 periodic grid,
g = 9.81, f = 1, RK3, A = 0.5|y| ("uniform B_x") or the two Gaussians, h = 1, the Gaussian vortex (u, v) = 5 (y, -x) exp(-r^2)
(multiplied by h for the conservative variables), dt = 0.01, stop time 30.  Every --every iterations one progress line like the
reference's (SWMHD_example.jl:47-61: time, iteration, max|u|, max|A|, min h, wall time) and one row of the energies the reference
sends to NetCDF (:74-77) into --energies (CSV).  --dump-every T writes the fields incl. halos as .npy (the JLD2 writer's role, :80-84).
--frames T collects the reference's output frames on the device (swmhd_amd.FieldTimeSeries: the fields (u, v, A, s) every T time units,
:80-84, or those of --frame-fields out of u v h A s B_x B_y and the derived vorticity divergence current potential_vorticity, as
--frame-dtype f32|f64) and writes them to <out>/frames.npz at the end.
--zonal-means T collects x-averaged profiles on the device (swmhd_amd.ZonalMeanTimeSeries: Oceananigans' Average(u, dims = 1) in an
output writer; every T time units the float64 row means of --zonal-names out of u v h A s B_x B_y uu vv uv B_xB_x B_yB_y B_xB_y vA, one
launch per sample and no frame) and writes them to <out>/zonal_means.npz at the end; in single, --amps and --channel --gradients runs.
--zonal-spectra T collects zonal wavenumber spectra on the device (swmhd_amd.ZonalSpectrumTimeSeries: every T time units the row-averaged
power spectra along x of --spectra-names out of u v h A s B_x B_y, by a double-precision row FFT in LDS; --size must be a power of two
from 4 to 4096) and writes them to <out>/zonal_spectra.npz at the end, with the wavenumbers k and kx = 2 pi k / Lx.
--isotropic-spectra T collects isotropic power spectra E(|k|) on the device (swmhd_amd.IsotropicSpectrumTimeSeries: every T time units the
shell sums of the 2-D power spectra of --spectra-names, by a row FFT, a column FFT in LDS and a shell sum; periodic runs whose --size is a
power of two from 4 to 4096) and writes them to <out>/isotropic_spectra.npz at the end, with the shell wavenumbers k and mode counts.
The step loop runs through HIP-graph replays (two RK3 steps per replay).
--dye adds one passive tracer c = tanh(y) to the run (ShallowWaterModel(tracers=("c",)): the reference's `tracers = (:A)` with a second
name): its min / max join the progress line and the field goes into the --dump-every dumps.  With --amps, --coriolis, --gravity or
--dts every member of the ensemble carries the dye (ShallowWaterEnsemble(tracers=("c",)): one more launch per RK3 stage for all of
them); the interiors of all members go to <out>/tracers.npz at the end.  Not with --channel (Bounded ensembles carry no tracers).
--beta B adds Oceananigans' coriolis = BetaPlane(f₀ = F0, β = B) with --coriolis as F0 (swmhd_amd.BetaPlane: f = F0 + B y, y = 0 in
mid-domain; the stage kernels run with f = 0 and one more launch per RK3 stage adds f(y) (v̄, -ū)): Rossby and magneto-Rossby waves.  Comma
lists give one ensemble member per entry, like --coriolis.  With --channel it runs ONE Bounded model (one --gradients entry: Bounded
ensembles take no f(y)).  Frames of potential_vorticity are not available under --beta; vorticity is.
--viscosity NU and --diffusivity ETA add Oceananigans' closure = ScalarDiffusivity(nu = NU, kappa = ETA) (swmhd_amd.ScalarDiffusivity:
NU on u and v, ETA -- the magnetic diffusivity -- on A and on the dye; one more launch per RK3 stage).  --viscosity needs
--formulation jacobian; neither goes with --channel.  In an ensemble run both take comma lists like --coriolis (a sweep of the Reynolds
or of the magnetic Prandtl number), and a list of several values starts one.  dt is not limited by the closure: the line printed at the
start gives ScalarDiffusivity.max_stable_dt.
--hyperviscosity NU4 and --hyperdiffusivity ETA4 add closure = ScalarBiharmonicDiffusivity(nu = NU4, kappa = ETA4) in the same way
(-NU4 laplace² on u and v, -ETA4 laplace² on A and on the dye; one more launch per RK3 stage), alone or next to --viscosity /
--diffusivity: the model then takes the tuple of both closures, as Oceananigans does.  The same rules and comma lists apply.
--drag R adds Oceananigans' forcing = (u = Relaxation(rate = R), v = Relaxation(rate = R)) (swmhd_amd.Relaxation; uh, vh with
--formulation divergence): linear drag on the two momentum-like fields, one more launch per RK3 stage.  In an ensemble run a comma list
gives one member per entry (a sweep of the drag), and a list of several values starts one.  --sponge RATE,WIDTH (with --channel) puts
Relaxation(rate = RATE, mask = G) on the same two fields, G(y) = exp(-((y - y_south) / WIDTH)²) + exp(-((y - y_north) / WIDTH)²): sponge
layers that absorb what reaches the walls.  With --drag R as well the two terms are one, Relaxation(rate = 1, mask = R + RATE G).  With --channel either runs ONE Bounded model (one --gradients entry: Bounded ensembles take no forcing).  dt is not
limited by the forcing: the line printed at the start gives Relaxation.max_stable_dt.
--bump HEIGHT,WIDTH runs over bathymetry = HEIGHT exp(-(x² + y²) / WIDTH²) (ShallowWaterModel(bathymetry=...)): a Gaussian hill at the
domain centre, subtracted from the initial h so that the surface h + b starts flat.  --body-force F0,K adds swmhd_amd.Source(F0 sin(K y))
to the first momentum-like field: the steady force of a Kolmogorov flow; it combines with --drag, --beta and --stir.  Either runs one
model, with one more launch per RK3 stage for both together.
--particles N [--track A,h] carries Lagrangian particles with the flow (ShallowWaterModel(particles=swmhd_amd.LagrangianParticles(...)):
Oceananigans' LagrangianParticles with tracked_fields): a lattice of ceil(sqrt(N))^2 particles seeded at cell-centred points in row-major
order, advanced on the device in one more launch per RK3 stage.  swmhd_amd.ParticleTimeSeries collects x, y and the --track fields (the
model's prognostic names and the dye) along the trajectories on the schedule of --frames (without --frames: the first and the last
state) and writes <out>/particles.npz at the end.  With A among them the run prints the drift of A along the trajectories beside A's own
range: in the ideal model A is frozen into the flow, so the drift measures the scheme's numerical resistivity.  One model.

--stir RATE,KF[,DK] [--seed N] stirs u and v with swmhd_amd.StochasticForcing(rate = RATE, k_f = KF, dk = DK): a random stream function
in the ring of wavenumbers KF - DK/2 <= |k| < KF + DK/2 (DK: the grid's lowest wavenumber unless given), white in time, exactly
non-divergent, renewed on the device every step and reproducible from the seed; RATE is the mean kinetic-energy injection per unit
mass and time.  With --drag the two fields carry both terms: the forced-dissipative run.  One periodic model, --formulation jacobian.

    python examples/run_swmhd.py --amps 0.1,0.5,1.0 [other options as above]
runs one member per A amplitude as ONE ensemble (swmhd_amd.ShallowWaterEnsemble: every member stepped by the same three launches per RK3
step): one progress line per member, and --energies gets a leading `member` column.

    python examples/run_swmhd.py --channel --gradients -0.01,-0.05,-0.1 [other options as above]
runs the reference's commented channel experiment (SWMHD_example.jl:18-22, divergence_sw_mhd.jl:17-21,34) as a sweep over the
gradient g, one member of a swmhd_amd.BoundedShallowWaterEnsemble per value: topology (Periodic, Bounded, Flat), A = g y with
GradientBoundaryCondition(g) on A north and south (an imposed uniform B_x = -g / h), h = 1 and the vortex above.  Output as for --amps.

    python examples/run_swmhd.py --coriolis 0.5,1,2 [--gravity 9.81,4,1] [--dts 0.01,0.01,0.005] [--amps ... | --channel --gradients ...]
sweeps the physical parameters: one ensemble member per entry with its own f (coriolis = FPlane(f = ...)), g
(gravitational_acceleration) and time step.  The lists are zipped with each other and with --amps / --gradients: every list has one
entry (used for all members) or the common length.  --energies gets the member's g, f and dt as columns after `member`; with --dts a
member's time is iteration x its dt, and the run ends when the member with the largest dt reaches --stop-time.

    python examples/run_swmhd.py --plot-case jacobian_formulation/128x128_two_Gaussians_low_B
re-runs one of the twelve runs behind the reference's committed energy plots (energy_plots/*/*.png; set-up from the scripts' commented
alternatives, see tests/plot_cases.py) and prints, beside every energy row, the value read off the plot at that time
(tests/golden/plot_readings.json) -- the comparison tests/test_reference_plots.py asserts."""
import argparse, csv, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--formulation", choices=["jacobian", "divergence"], default="jacobian")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--stop-time", type=float, default=30.0)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--ic", choices=["uniform", "gaussians"], default="uniform")
    ap.add_argument("--amp", type=float, default=None, help="A amplitude (default 0.5 for |y|, 0.1 / 0.5 for the Gaussians)")
    ap.add_argument("--amps", default=None, help="comma-separated A amplitudes: one ensemble member per amplitude")
    ap.add_argument("--channel", action="store_true", help="(Periodic, Bounded) channel with gradient boundary conditions on A")
    ap.add_argument("--gradients", default=None, help="with --channel: comma-separated gradients of A, one ensemble member each")
    ap.add_argument("--coriolis", default=None, help="comma-separated Coriolis parameters f: one ensemble member per entry")
    ap.add_argument("--beta", default=None, help="beta of coriolis = BetaPlane(f0, beta), with --coriolis as f0 (ensemble runs: a comma list, one member per entry)")
    ap.add_argument("--gravity", default=None, help="comma-separated gravitational accelerations g: one ensemble member per entry")
    ap.add_argument("--dts", default=None, help="comma-separated time steps: one ensemble member per entry (overrides --dt)")
    ap.add_argument("--every", type=int, default=100, help="iterations between progress lines / energy rows")
    ap.add_argument("--energies", default=None, help="CSV file for (time, KE, ME, PE, total)")
    ap.add_argument("--dump-every", type=float, default=0.0, help="model time between field dumps (0 = none)")
    ap.add_argument("--frames", type=float, default=0.0, help="model time between output frames (0 = none); written to <out>/frames.npz")
    ap.add_argument("--frame-fields", default="u,v,A,s", help="comma-separated fields of a frame: u v h A s B_x B_y vorticity divergence current potential_vorticity")
    ap.add_argument("--frame-dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--zonal-means", type=float, default=0.0, help="model time between zonal-mean samples (0 = none); written to <out>/zonal_means.npz")
    ap.add_argument("--zonal-names", default="u,v,A,uv,B_xB_y,vA", help="comma-separated profiles: u v h A s B_x B_y uu vv uv B_xB_x B_yB_y B_xB_y vA")
    ap.add_argument("--zonal-spectra", type=float, default=0.0, help="model time between zonal-spectrum samples (0 = none); written to <out>/zonal_spectra.npz")
    ap.add_argument("--isotropic-spectra", type=float, default=0.0, help="model time between isotropic-spectrum samples (0 = none); written to <out>/isotropic_spectra.npz")
    ap.add_argument("--spectra-names", default="u,v,A", help="comma-separated spectra: u v h A s B_x B_y")
    ap.add_argument("--dye", action="store_true", help="advect one passive tracer c = tanh(y) with the flow")
    ap.add_argument("--viscosity", default=None, help="nu of ScalarDiffusivity, on u and v (ensemble runs: a comma list, one member per entry)")
    ap.add_argument("--diffusivity", default=None, help="kappa of ScalarDiffusivity, on A and the dye (ensemble runs: a comma list)")
    ap.add_argument("--hyperviscosity", default=None, help="nu of ScalarBiharmonicDiffusivity, on u and v (ensemble runs: a comma list)")
    ap.add_argument("--hyperdiffusivity", default=None, help="kappa of ScalarBiharmonicDiffusivity, on A and the dye (ensemble runs: a comma list)")
    ap.add_argument("--drag", default=None, help="rate of Relaxation on the two momentum-like fields (ensemble runs: a comma list, one member per entry)")
    ap.add_argument("--sponge", default=None, help="RATE,WIDTH with --channel: Relaxation(rate=RATE, mask=Gaussians of that width at the two walls) on the momentum-like fields")
    ap.add_argument("--stir", default=None, help="RATE,KF[,DK]: StochasticForcing(rate=RATE, k_f=KF, dk=DK or the grid's lowest wavenumber) on u and v (one periodic model, --formulation jacobian)")
    ap.add_argument("--seed", type=int, default=0, help="seed of --stir")
    ap.add_argument("--bump", default=None, help="HEIGHT,WIDTH: bathymetry = a Gaussian hill of that height and width at the domain centre, subtracted from the initial h (one model)")
    ap.add_argument("--body-force", default=None, help="F0,K: Source(F0 sin(K y)) on the first momentum-like field, a Kolmogorov force (one model)")
    ap.add_argument("--particles", type=int, default=0, help="N: carry a lattice of ceil(sqrt(N))^2 Lagrangian particles; written to <out>/particles.npz (one model)")
    ap.add_argument("--track", default="A", help="with --particles: comma-separated fields sampled along the trajectories (prognostic names, c with --dye)")
    ap.add_argument("--out", default="swmhd_out")
    ap.add_argument("--plot-case", default=None, help="one of the reference's plotted runs, e.g. jacobian_formulation/64x64_low_B_low_U")
    argv = sys.argv[1:]
    k = 0
    while k < len(argv) - 1:         # "--gradients -0.01,-0.05": argparse would read the negative list as an option
        if argv[k] in ("--gradients", "--coriolis", "--beta"):
            argv[k] = argv[k] + "=" + argv.pop(k + 1)
        k += 1
    a = ap.parse_args(argv)
    if a.plot_case:
        return plot_case(a)
    if a.channel != (a.gradients is not None):
        ap.error("--channel and --gradients go together")
    if a.channel and a.amps:
        ap.error("--channel sweeps --gradients, not --amps")
    a.sweep = any(x is not None for x in (a.coriolis, a.gravity, a.dts)) or any("," in (x or "") for x in (a.viscosity, a.diffusivity, a.hyperviscosity, a.hyperdiffusivity))
    a.closure = a.viscosity is not None or a.diffusivity is not None
    a.closure4 = a.hyperviscosity is not None or a.hyperdiffusivity is not None
    if (a.closure or a.closure4) and a.channel:
        ap.error("--viscosity / --diffusivity / --hyperviscosity / --hyperdiffusivity: not with --channel (the closures run on periodic grids)")
    if (a.viscosity is not None or a.hyperviscosity is not None) and a.formulation != "jacobian":
        ap.error("--viscosity / --hyperviscosity need --formulation jacobian (the conservative viscous stress is another operator)")
    if a.dts and a.frames > 0:
        ap.error("--frames is a schedule in time units: not with a per-member time step (--dts)")
    if a.dts and a.zonal_means > 0:
        ap.error("--zonal-means is a schedule in time units: not with a per-member time step (--dts)")
    if a.dts and a.zonal_spectra > 0:
        ap.error("--zonal-spectra is a schedule in time units: not with a per-member time step (--dts)")
    if a.dts and a.isotropic_spectra > 0:
        ap.error("--isotropic-spectra is a schedule in time units: not with a per-member time step (--dts)")
    if a.dye and a.channel:
        ap.error("--dye: not with --channel (Bounded ensembles carry no tracers)")
    a.sweep = a.sweep or "," in (a.beta or "") or "," in (a.drag or "")
    if a.stir is not None and (a.channel or a.formulation != "jacobian" or len(a.stir.split(",")) not in (2, 3)):
        ap.error("--stir RATE,KF[,DK]: a periodic grid and --formulation jacobian (the stirring is a stream function's, for u and v)")
    if a.stir is not None and (a.amps or a.sweep):
        ap.error("--stir runs one model: not with an ensemble run")
    for opt, val in (("--bump HEIGHT,WIDTH", a.bump), ("--body-force F0,K", a.body_force)):
        if val is not None and len(val.split(",")) != 2:
            ap.error(f"{opt}: two numbers")
        if val is not None and (a.amps or a.sweep):
            ap.error(f"{opt} runs one model: not with an ensemble run")
    if a.sponge is not None and (not a.channel or len(a.sponge.split(",")) != 2):
        ap.error("--sponge RATE,WIDTH needs --channel: the sponge layers stand at the channel's walls")
    # --channel with --beta, --drag or --sponge: ONE Bounded model (Bounded ensembles take no f(y) and no forcing), so one gradient, one
    # f0, one beta and one drag
    one_channel = a.channel and (a.beta is not None or a.drag is not None or a.sponge is not None or a.bump is not None or a.body_force is not None)
    if one_channel and (a.gravity or a.dts or any("," in (x or "") for x in (a.gradients, a.beta, a.coriolis, a.drag))):
        ap.error("--channel with --beta, --drag or --sponge runs one model: one --gradients entry, one --coriolis, one --beta, one --drag, "
                 "no --gravity or --dts")
    if a.particles < 0 or (a.particles and (a.amps or a.sweep or (a.channel and not one_channel))):
        ap.error("--particles N runs one model: not with an ensemble run (with --channel: beside --beta, --drag, --sponge, --bump or --body-force)")
    if (a.amps or a.channel or a.sweep) and not one_channel:
        return run_ensemble(a)
    a.sweep = False

    import torch
    import swmhd_amd as S
    from swmhd_amd import configs
    N, L = a.size, 10.0
    grid = S.RectilinearGrid(size=(N, N), x=(-L / 2, L / 2), y=(-L / 2, L / 2),
                             topology=("Periodic", "Bounded" if a.channel else "Periodic", "Flat"))
    form = "VectorInvariant" if a.formulation == "jacobian" else "Conservative"
    closures = []
    if a.closure:
        closures.append(S.ScalarDiffusivity(nu=float(a.viscosity or 0.0), kappa=float(a.diffusivity or 0.0)))
    if a.closure4:
        closures.append(S.ScalarBiharmonicDiffusivity(nu=float(a.hyperviscosity or 0.0), kappa=float(a.hyperdiffusivity or 0.0)))
    for c in closures:
        print(f"closure: {c}, max_stable_dt = {c.max_stable_dt(grid):.4g} (dt = {a.dt:g})")
    closure = None if not closures else (closures[0] if len(closures) == 1 else tuple(closures))
    # --beta B [--coriolis F0]: coriolis = BetaPlane(f0 = F0, beta = B), f = F0 + B y with y = 0 in mid-domain; one more launch per stage
    coriolis = S.BetaPlane(float(a.coriolis) if a.coriolis else configs.F, float(a.beta)) if a.beta is not None else S.FPlane(configs.F)
    if a.beta is not None:
        print(f"coriolis: {coriolis}")
    gr = float(a.gradients) if a.channel else None
    bcs = {"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(gr), south=S.GradientBoundaryCondition(gr))} if a.channel else None
    # --drag R: Relaxation(rate = R) on the two momentum-like fields.  --sponge RATE,WIDTH: Relaxation(rate = RATE, mask = G) with G the
    # two Gaussians at the walls; with both, one Relaxation(rate = 1, mask = R + RATE G): a field has one Relaxation
    momentum = ("u", "v") if form == "VectorInvariant" else ("uh", "vh")
    forcing = None
    if a.sponge is not None:
        rate, width = (float(x) for x in a.sponge.split(","))
        south, north = grid.y
        gaussians = lambda x, y: np.exp(-((y - south) / width) ** 2) + np.exp(-((y - north) / width) ** 2) + 0 * x
        if a.drag is None:
            forcing = {n: S.Relaxation(rate, mask=gaussians) for n in momentum}
        else:
            drag = float(a.drag)
            forcing = {n: S.Relaxation(1.0, mask=lambda x, y: drag + rate * gaussians(x, y)) for n in momentum}
    elif a.drag is not None:
        forcing = {n: S.Relaxation(float(a.drag)) for n in momentum}
    for n, r in (forcing or {}).items():
        print(f"forcing: {n} = {r}, max_stable_dt = {r.max_stable_dt(grid, S.fields.LOCS[n]):.4g} (dt = {a.dt:g})")
    # --stir RATE,KF[,DK]: ONE StochasticForcing under both momentum names (a random stream function in the ring |k| = KF +- DK/2, white
    # in time, renewed every step on the device), beside the drag where there is one: a field carries (Relaxation, StochasticForcing)
    if a.stir is not None:
        vals = [float(x) for x in a.stir.split(",")]
        stir = S.StochasticForcing(vals[0], vals[1], vals[2] if len(vals) > 2 else 2 * np.pi / L, seed=a.seed)
        print(f"forcing: {stir} on u, v: {len(S.forcing_modes(grid, stir.k_f, stir.dk))} modes")
        forcing = {n: ((forcing[n], stir) if forcing and n in forcing else stir) for n in momentum}
    # --body-force F0,K: Source(F0 sin(K y)) under the first momentum-like field (an acceleration in both formulations), beside whatever
    # that field carries already: the steady force of a Kolmogorov flow.  One more launch per RK3 stage for it and --bump together
    if a.body_force is not None:
        f0, kk = (float(x) for x in a.body_force.split(","))
        push = S.Source(lambda x, y: f0 * np.sin(kk * y) + 0 * x)
        print(f"forcing: {momentum[0]} = Source({f0:g} sin({kk:g} y))")
        forcing = dict(forcing or {})
        held = forcing.get(momentum[0], ())
        forcing[momentum[0]] = (held if isinstance(held, tuple) else (held,)) + (push,)
    # --bump HEIGHT,WIDTH: bathymetry = a Gaussian hill at the domain centre; h stays the fluid thickness, so the initial h is 1 - b
    # and the surface h + b starts flat
    bump = None
    if a.bump is not None:
        height, width = (float(x) for x in a.bump.split(","))
        bump = lambda x, y: height * np.exp(-(x ** 2 + y ** 2) / width ** 2)
        print(f"bathymetry: a Gaussian hill, height {height:g}, width {width:g}")
    # --particles N: a lattice of ceil(sqrt(N))^2 particles at cell-centred points of the domain, row-major (neighbours in memory are
    # neighbours in space: their gathers share cache lines until the flow scrambles them)
    particles = None
    if a.particles:
        n = int(np.ceil(np.sqrt(a.particles)))
        pts = -L / 2 + (np.arange(n) + 0.5) * (L / n)
        PX, PY = np.meshgrid(pts, pts)
        particles = S.LagrangianParticles(PX.ravel(), PY.ravel(), tracked_fields=tuple(t.strip() for t in a.track.split(",") if t.strip()))
        print(f"particles: a {n} x {n} lattice, tracked fields ({', '.join(particles.tracked_fields)})")
    model = S.ShallowWaterModel(grid, configs.G, formulation=form, tracers=("c",) if a.dye else (), closure=closure, coriolis=coriolis,
                                boundary_conditions=bcs, forcing=forcing, bathymetry=bump, particles=particles)
    amp = a.amp if a.amp is not None else (0.5 if a.ic == "uniform" or form == "Conservative" else 0.1)
    A0 = (lambda X, Y: amp * np.abs(Y)) if a.ic == "uniform" else configs.two_gaussians(amp)
    if a.channel:
        A0 = lambda X, Y: gr * Y
    u0 = lambda X, Y: 5 * Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -5 * X * np.exp(-(X ** 2 + Y ** 2))
    n1, n2 = model.names[:2]
    h0 = (lambda X, Y: np.ones_like(X)) if bump is None else (lambda X, Y: 1.0 - bump(X, Y))
    model.set(**{n1: u0, n2: v0, "h": h0, "A": A0})      # h = 1: (uh, vh) = (u, v); over a hill (uh, vh) start as (u, v) all the same
    if a.dye:
        model.set(c=lambda X, Y: np.tanh(Y))
    nsteps = int(round(a.stop_time / a.dt))
    rows = []

    def report(wall):
        d = model.diagnostics()
        dye = ""
        if a.dye:
            c = model.tracers["c"].interior()
            dye = f"min(c): {c.min().item():.4f}, max(c): {c.max().item():.4f}, "
        print(f"Time: {model.clock_time:9.3f}, iteration: {model.iteration}, max(|u|): {max(d['max_abs_u'], d['max_abs_v']):.2e}, "
              f"max(|A|): {d['max_abs_A']:.2e}, min(h): {d['min_h']:.2e}, {dye}wall time: {wall * 1e3:.1f} ms "
              f"| KE {d['kinetic_energy']:.6f} ME {d['magnetic_energy']:.6f} PE {d['potential_energy']:.3e} total {d['total_energy']:.6f}", flush=True)
        rows.append((model.clock_time, d["kinetic_energy"], d["magnetic_energy"], d["potential_energy"], d["total_energy"]))

    report(0.0)
    e0 = rows[0][4]
    series, fevery = frame_writer(a, model, nsteps)
    zonal, zevery = zonal_writer(a, model, nsteps)
    spectra, severy = spectra_writer(a, model, nsteps)
    iso, ievery = isotropic_writer(a, model, nsteps)
    parts, pevery = particle_writer(a, model, nsteps)
    model.time_step(a.dt)
    if pevery == 1:
        parts.write()
    if fevery == 1:
        series.write()
    if zevery == 1:
        zonal.write()
    if severy == 1:
        spectra.write()
    if ievery == 1:
        iso.write()
    model.capture_graph(a.dt)
    next_dump = a.dump_every
    t_start = time.perf_counter()
    t0 = None
    while model.iteration < nsteps:
        t0 = time.perf_counter() if t0 is None else t0      # wall time of one progress interval
        n = min(a.every - model.iteration % a.every, nsteps - model.iteration)
        if fevery:
            n = min(n, fevery - model.iteration % fevery)
        if zevery:
            n = min(n, zevery - model.iteration % zevery)
        if severy:
            n = min(n, severy - model.iteration % severy)
        if ievery:
            n = min(n, ievery - model.iteration % ievery)
        if pevery:
            n = min(n, pevery - model.iteration % pevery)
        model.time_steps(n, a.dt)
        if pevery and model.iteration % pevery == 0:
            parts.write(time=model.iteration * a.dt)          # one sampler launch and row copies, no synchronisation
        if fevery and model.iteration % fevery == 0:
            series.write(time=model.iteration * a.dt)         # one launch, no synchronisation
        if zevery and model.iteration % zevery == 0:
            zonal.write(time=model.iteration * a.dt)          # likewise
        if severy and model.iteration % severy == 0:
            spectra.write(time=model.iteration * a.dt)        # two launches, no synchronisation
        if ievery and model.iteration % ievery == 0:
            iso.write(time=model.iteration * a.dt)            # three launches, no synchronisation
        if model.iteration % a.every != 0 and model.iteration != nsteps:
            continue
        model.synchronize()
        report(time.perf_counter() - t0)
        t0 = None
        if a.dump_every > 0 and model.clock_time + 1e-12 >= next_dump:
            os.makedirs(a.out, exist_ok=True)
            model.save_checkpoint(os.path.join(a.out, f"fields_{model.iteration:07d}"))
            next_dump += a.dump_every
    total = time.perf_counter() - t_start
    print(f"Simulation took {total:.2f} s to finish running ({nsteps} iterations, {N * N * nsteps / total / 1e6:.1f} Mcell-steps/s); "
          f"energy drift abs(E - E0) * 100 = {abs(rows[-1][4] - e0) * 100:.4f}")
    save_frames(a, series)
    save_zonal(a, zonal)
    save_spectra(a, spectra)
    save_isotropic(a, iso)
    save_particles(a, parts)
    if a.energies:
        with open(a.energies, "w", newline="") as f:
            w = csv.writer(f); w.writerow(["time", "kinetic", "magnetic", "potential", "total"]); w.writerows(rows)


def frame_writer(a, model, nsteps):
    """--frames: (FieldTimeSeries, steps between frames), or (None, 0)"""
    if a.frames <= 0:
        return None, 0
    import torch
    import swmhd_amd as S
    sched = S.TimeInterval(a.frames)
    every = sched.steps(a.dt)
    series = S.FieldTimeSeries(model, names=tuple(n.strip() for n in a.frame_fields.split(",") if n.strip()), schedule=sched,
                               capacity=nsteps // every + 1, array_type=torch.float32 if a.frame_dtype == "f32" else torch.float64)
    series.write()          # the initial state, as Oceananigans' writers do at iteration 0
    return series, every


def save_frames(a, series):
    if series is not None:
        os.makedirs(a.out, exist_ok=True)
        series.save(os.path.join(a.out, "frames.npz"))
        print(f"{len(series)} frames of ({', '.join(series.names)}) -> {os.path.join(a.out, 'frames.npz')}")


def zonal_writer(a, model, nsteps):
    """--zonal-means: (ZonalMeanTimeSeries, steps between samples), or (None, 0)"""
    if a.zonal_means <= 0:
        return None, 0
    import swmhd_amd as S
    sched = S.TimeInterval(a.zonal_means)
    every = sched.steps(a.dt)
    zonal = S.ZonalMeanTimeSeries(model, names=tuple(n.strip() for n in a.zonal_names.split(",") if n.strip()), schedule=sched,
                                  capacity=nsteps // every + 1)
    zonal.write()           # the initial state, as the frames
    return zonal, every


def save_zonal(a, zonal):
    if zonal is not None:
        os.makedirs(a.out, exist_ok=True)
        zonal.save(os.path.join(a.out, "zonal_means.npz"))
        print(f"{len(zonal)} samples of the zonal means ({', '.join(zonal.names)}) -> {os.path.join(a.out, 'zonal_means.npz')}")


def spectra_writer(a, model, nsteps):
    """--zonal-spectra: (ZonalSpectrumTimeSeries, steps between samples), or (None, 0)"""
    if a.zonal_spectra <= 0:
        return None, 0
    import swmhd_amd as S
    sched = S.TimeInterval(a.zonal_spectra)
    every = sched.steps(a.dt)
    spectra = S.ZonalSpectrumTimeSeries(model, names=tuple(n.strip() for n in a.spectra_names.split(",") if n.strip()), schedule=sched,
                                        capacity=nsteps // every + 1)
    spectra.write()         # the initial state, as the frames
    return spectra, every


def save_spectra(a, spectra):
    if spectra is not None:
        os.makedirs(a.out, exist_ok=True)
        spectra.save(os.path.join(a.out, "zonal_spectra.npz"))
        print(f"{len(spectra)} samples of the zonal spectra ({', '.join(spectra.names)}) -> {os.path.join(a.out, 'zonal_spectra.npz')}")


def isotropic_writer(a, model, nsteps):
    """--isotropic-spectra: (IsotropicSpectrumTimeSeries, steps between samples), or (None, 0)"""
    if a.isotropic_spectra <= 0:
        return None, 0
    import swmhd_amd as S
    sched = S.TimeInterval(a.isotropic_spectra)
    every = sched.steps(a.dt)
    iso = S.IsotropicSpectrumTimeSeries(model, names=tuple(n.strip() for n in a.spectra_names.split(",") if n.strip()), schedule=sched,
                                        capacity=nsteps // every + 1)
    iso.write()             # the initial state, as the frames
    return iso, every


def save_isotropic(a, iso):
    if iso is not None:
        os.makedirs(a.out, exist_ok=True)
        iso.save(os.path.join(a.out, "isotropic_spectra.npz"))
        print(f"{len(iso)} samples of the isotropic spectra ({', '.join(iso.names)}) -> {os.path.join(a.out, 'isotropic_spectra.npz')}")


def particle_writer(a, model, nsteps):
    """--particles: (ParticleTimeSeries, steps between samples), or (None, 0).  The schedule of --frames; without it the first and the
    last state."""
    if not a.particles:
        return None, 0
    import swmhd_amd as S
    sched = S.TimeInterval(a.frames) if a.frames > 0 else S.IterationInterval(max(nsteps, 1))
    every = sched.steps(a.dt)
    parts = S.ParticleTimeSeries(model, names=("x", "y") + model.particles.tracked_fields, schedule=sched, capacity=nsteps // every + 1)
    parts.write()           # the initial state, as the frames
    return parts, every


def save_particles(a, parts):
    if parts is None:
        return
    os.makedirs(a.out, exist_ok=True)
    parts.save(os.path.join(a.out, "particles.npz"))
    print(f"{len(parts)} samples of {parts.model.particles.P} particles ({', '.join(parts.names)}) -> {os.path.join(a.out, 'particles.npz')}")
    if "A" in parts.names and len(parts) > 1:
        A = parts.numpy()[:, parts.names.index("A")]
        drift = np.abs(A[-1] - A[0])
        print(f"A along the trajectories: drift max {drift.max():.3e}, rms {np.sqrt(np.mean(drift ** 2)):.3e}; "
              f"range of A over the particles {A[0].max() - A[0].min():.3e}")


def run_ensemble(a):
    """--amps: the same run for several A amplitudes, one ensemble member each.  --channel: one member per gradient of A.
    --coriolis, --gravity, --dts: one member per entry with its own f, g and time step, zipped with the former."""
    import torch
    import swmhd_amd as S
    from swmhd_amd import configs
    form = "VectorInvariant" if a.formulation == "jacobian" else "Conservative"
    floats = lambda txt: [float(x) for x in txt.split(",") if x.strip()]
    if a.channel or a.amps:
        amps = floats(a.gradients if a.channel else a.amps)
    else:
        amps = [a.amp if a.amp is not None else (0.5 if a.ic == "uniform" or form == "Conservative" else 0.1)]
    lists = {"--coriolis": floats(a.coriolis or ""), "--gravity": floats(a.gravity or ""), "--dts": floats(a.dts or ""),
             "--viscosity": floats(a.viscosity or ""), "--diffusivity": floats(a.diffusivity or ""), "--beta": floats(a.beta or ""),
             "--hyperviscosity": floats(a.hyperviscosity or ""), "--hyperdiffusivity": floats(a.hyperdiffusivity or ""),
             "--drag": floats(a.drag or "")}
    B = max([len(amps)] + [len(v) for v in lists.values()])
    for name, v in [("--gradients" if a.channel else "--amps", amps)] + [(k, v) for k, v in lists.items() if v]:
        if len(v) not in (1, B):
            sys.exit(f"{name}: {len(v)} entries; every list has 1 entry or the common length {B}")
    amps = amps * (B // len(amps))
    per = lambda v, default: default if not v else (v * (B // len(v)))      # a list of B values, or the scalar default
    gs, fs, dt = per(lists["--gravity"], configs.G), per(lists["--coriolis"], configs.F), per(lists["--dts"], a.dt)
    a.dt = max(dt) if a.dts else a.dt                                           # the step that the stop time and --every are counted in
    N, L = a.size, 10.0
    if a.channel:
        grid = S.RectilinearGrid(size=(N, N), x=(-L / 2, L / 2), y=(-L / 2, L / 2), topology=("Periodic", "Bounded", "Flat"))
        bcs = [{"A": S.FieldBoundaryConditions(north=S.GradientBoundaryCondition(gr), south=S.GradientBoundaryCondition(gr))} for gr in amps]
        ens = S.BoundedShallowWaterEnsemble(grid, len(amps), gs, fs, formulation=form, boundary_conditions=bcs)
        A0 = [lambda X, Y, gr=gr: gr * Y for gr in amps]
    else:
        grid = S.RectilinearGrid(size=(N, N), x=(-L / 2, L / 2), y=(-L / 2, L / 2))
        closures = []
        if a.closure:
            closures.append(S.ScalarDiffusivity(nu=per(lists["--viscosity"], 0.0), kappa=per(lists["--diffusivity"], 0.0)))
        if a.closure4:
            closures.append(S.ScalarBiharmonicDiffusivity(nu=per(lists["--hyperviscosity"], 0.0), kappa=per(lists["--hyperdiffusivity"], 0.0)))
        for c in closures:
            print(f"closure: {c}, max_stable_dt = {c.max_stable_dt(grid):.4g}")
        closure = None if not closures else (closures[0] if len(closures) == 1 else tuple(closures))
        # --beta: coriolis = BetaPlane(f0, beta) with --coriolis as f0, a scalar or one value per member each
        fkw = {"coriolis_f": fs}
        if a.beta is not None:
            fkw = {"coriolis": S.BetaPlane(fs, per(lists["--beta"], 0.0))}
            print(f"coriolis: {fkw['coriolis']}")
        # --drag: Relaxation(rate) on the two momentum-like fields, a scalar or one rate per member
        forcing = None
        if a.drag is not None:
            forcing = {n: S.Relaxation(per(lists["--drag"], 0.0)) for n in (("u", "v") if form == "VectorInvariant" else ("uh", "vh"))}
            print(f"forcing: {forcing}, max_stable_dt = {min(r.max_stable_dt() for r in forcing.values()):.4g}")
        ens = S.ShallowWaterEnsemble(grid, len(amps), gs, formulation=form, tracers=("c",) if a.dye else (), closure=closure,
                                     forcing=forcing, **fkw)
        A0 = [(lambda X, Y, amp=amp: amp * np.abs(Y)) if a.ic == "uniform" else configs.two_gaussians(amp) for amp in amps]
    label = "gradient" if a.channel else "amp"
    u0 = lambda X, Y: 5 * Y * np.exp(-(X ** 2 + Y ** 2))
    v0 = lambda X, Y: -5 * X * np.exp(-(X ** 2 + Y ** 2))
    n1, n2 = ens.names[:2]
    ens.set(**{n1: u0, n2: v0, "h": lambda X, Y: np.ones_like(X), "A": A0})
    if a.dye:
        ens.set(c=lambda X, Y: np.tanh(Y))
    nsteps = int(round(a.stop_time / a.dt))
    rows = []

    def report(wall):
        c = ens.tracers["c"][(slice(None),) + grid.interior] if a.dye else None
        for m, d in enumerate(ens.diagnostics()):
            t = float(ens.clock_times[m])
            dye = f"min(c): {c[m].min().item():.4f}, max(c): {c[m].max().item():.4f}, " if a.dye else ""
            print(f"member {m} ({label} {amps[m]:g}{sweep(m)}) Time: {t:9.3f}, iteration: {ens.iteration}, "
                  f"max(|u|): {max(d['max_abs_u'], d['max_abs_v']):.2e}, max(|A|): {d['max_abs_A']:.2e}, min(h): {d['min_h']:.2e}, "
                  f"{dye}wall time: {wall * 1e3:.1f} ms | KE {d['kinetic_energy']:.6f} ME {d['magnetic_energy']:.6f} "
                  f"PE {d['potential_energy']:.3e} total {d['total_energy']:.6f}", flush=True)
            rows.append((m,) + (params(m) if a.sweep else ()) + (t, d["kinetic_energy"], d["magnetic_energy"], d["potential_energy"], d["total_energy"]))

    f0 = np.broadcast_to(np.asarray(fs, dtype=float), (len(amps),))        # (with --beta: f0; the stage kernels then run with f = 0)
    params = lambda m: (float(ens.g_values[m]), float(f0[m]), dt[m] if a.dts else a.dt)
    sweep = lambda m: ", g {:g}, f {:g}, dt {:g}".format(*params(m)) if a.sweep else ""
    report(0.0)
    e0 = [r[-1] for r in rows]
    series, fevery = frame_writer(a, ens, nsteps)
    zonal, zevery = zonal_writer(a, ens, nsteps)
    spectra, severy = spectra_writer(a, ens, nsteps)
    iso, ievery = isotropic_writer(a, ens, nsteps)
    ens.time_step(dt)
    if fevery == 1:
        series.write()
    if zevery == 1:
        zonal.write()
    if severy == 1:
        spectra.write()
    if ievery == 1:
        iso.write()
    ens.capture_graph(dt)
    t_start = time.perf_counter()
    t0 = None
    while ens.iteration < nsteps:
        t0 = time.perf_counter() if t0 is None else t0      # wall time of one progress interval
        n = min(a.every - ens.iteration % a.every, nsteps - ens.iteration)
        if fevery:
            n = min(n, fevery - ens.iteration % fevery)
        if zevery:
            n = min(n, zevery - ens.iteration % zevery)
        if severy:
            n = min(n, severy - ens.iteration % severy)
        if ievery:
            n = min(n, ievery - ens.iteration % ievery)
        ens.time_steps(n, dt)
        if fevery and ens.iteration % fevery == 0:
            series.write(time=ens.iteration * a.dt)           # all members in one launch, no synchronisation
        if zevery and ens.iteration % zevery == 0:
            zonal.write(time=ens.iteration * a.dt)            # likewise
        if severy and ens.iteration % severy == 0:
            spectra.write(time=ens.iteration * a.dt)          # likewise
        if ievery and ens.iteration % ievery == 0:
            iso.write(time=ens.iteration * a.dt)              # likewise
        if ens.iteration % a.every != 0 and ens.iteration != nsteps:
            continue
        ens.synchronize()
        report(time.perf_counter() - t0)
        t0 = None
    total = time.perf_counter() - t_start
    drift = ", ".join(f"{abs(rows[-len(amps) + m][-1] - e0[m]) * 100:.4f}" for m in range(len(amps)))
    print(f"Simulation took {total:.2f} s to finish running ({nsteps} iterations of {len(amps)} members, "
          f"{len(amps) * N * N * nsteps / total / 1e6:.1f} Mcell-steps/s); energy drift abs(E - E0) * 100 per member = {drift}")
    save_frames(a, series)
    save_zonal(a, zonal)
    save_spectra(a, spectra)
    save_isotropic(a, iso)
    if a.dye:
        os.makedirs(a.out, exist_ok=True)
        np.savez(os.path.join(a.out, "tracers.npz"), c=ens.tracers["c"][(slice(None),) + grid.interior].cpu().numpy(),
                 time=ens.clock_times, iteration=ens.iteration)
    if a.energies:
        with open(a.energies, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["member"] + (["g", "f", "dt"] if a.sweep else []) + ["time", "kinetic", "magnetic", "potential", "total"])
            w.writerows(rows)


def plot_case(a):
    """One of the reference's twelve plotted runs through the HIP engine, the plot's own readings printed beside the run's energies."""
    import json
    import swmhd_amd as S
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "plot_readings.json")) as f:
        R = json.load(f)
    if a.plot_case not in R:
        sys.exit("--plot-case must be one of: " + ", ".join(k for k in sorted(R) if not k.startswith("_")))
    r = R[a.plot_case]
    form_dir, rest = a.plot_case.split("/")
    N, ic = int(rest.split("x")[0]), rest.split("_", 1)[1]
    form = "VectorInvariant" if form_dir.startswith("jacobian") else "Conservative"
    L, dt = 10.0, 0.01
    gauss = lambda amp: (lambda X, Y: amp * np.exp(-((X - 0.5) ** 2 + Y ** 2)) - amp * np.exp(-((X + 0.5) ** 2 + Y ** 2)))
    zero = lambda X, Y: np.zeros_like(X)
    bcs, topo, u0, v0 = None, ("Periodic", "Periodic", "Flat"), zero, zero
    if ic == "low_B_low_U":          # divergence_sw_mhd.jl:34,36-37 with the commented GradientBoundaryCondition(-0.05), (Periodic, Bounded)
        A0, topo = (lambda X, Y: -0.05 * Y), ("Periodic", "Bounded", "Flat")
        u0, v0 = (lambda X, Y: Y * np.exp(-(X ** 2 + Y ** 2))), (lambda X, Y: -X * np.exp(-(X ** 2 + Y ** 2)))
        bcs = {"A": S.FieldBoundaryConditions(south=S.GradientBoundaryCondition(-0.05), north=S.GradientBoundaryCondition(-0.05))}
    else:
        A0 = gauss(0.1 if ic.endswith("low_B") else 0.5)
    grid = S.RectilinearGrid(size=(N, N), x=(-L / 2, L / 2), y=(-L / 2, L / 2), topology=topo)
    m = S.ShallowWaterModel(grid, 9.81, 1.0, formulation=form, boundary_conditions=bcs)
    n1, n2 = m.names[:2]
    m.set(**{n1: u0, n2: v0, "h": lambda X, Y: np.ones_like(X), "A": A0})
    t_end = a.stop_time if a.stop_time != 30.0 else r["times"][-1]
    step = r["times"][1] - r["times"][0]
    e0 = None
    print(f"{a.plot_case}: {form}, {N}x{N}, dt = {dt}, to t = {t_end:g}   [run | plot reading +- tolerance]")
    t0 = time.perf_counter()
    for k, t in enumerate(r["times"]):
        if t > t_end + 1e-9:
            break
        if k:
            m.time_steps(int(round(step / dt)), dt)
        d = m.diagnostics()
        e0 = d["total_energy"] if e0 is None else e0
        vals = dict(kinetic=d["kinetic_energy"], magnetic=d["magnetic_energy"], potential=d["potential_energy"], error_x100=abs(d["total_energy"] - e0) * 100)
        cells = []
        for p in ("kinetic", "magnetic", "potential", "error_x100"):
            rd = r.get(p, [None] * len(r["times"]))[k]
            ref = "      -      " if rd is None else f"{rd[0] - (490.5 if (p == 'potential' and rd[0] > 400) else 0):9.5f}+-{rd[1]:.5f}"
            cells.append(f"{p[:3]} {vals[p]:9.5f} | {ref}")
        print(f"t = {t:5.1f}  " + "   ".join(cells), flush=True)
    print(f"{m.iteration} iterations in {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()
