/*
 * Single source of truth for every run-time option of fdtd3d-amd.
 *
 * Consumed two ways:
 *   - C++ (csrc/settings.cpp, the standalone `fdtd3d` driver): X-macro expansion.
 *   - Python (fdtd3d_amd/utils/settings.py): parsed with a regex at import time,
 *     so the Python mirror can never drift from the native parser.
 *
 * Row kinds (one per line, arguments separated by ", " and strings quoted):
 *   FDTD_ACTION (cli, help)                       flag with a side effect handled by code
 *   FDTD_ACTION_ARG (cli, help)                   option with one string argument handled by code
 *   FDTD_BOOL (field, cli, help)                  flag, sets field = true
 *   FDTD_INT (field, cli, default, help)
 *   FDTD_FLOAT (field, cli, default, help)
 *   FDTD_STRING (field, cli, default, help)
 *
 * The reference's option names and defaults are preserved (reference
 * Source/Settings/Settings.inc:28-125); extensions are grouped at the end and
 * cover the reference's TODO list (Settings.inc:127-145) plus the run-time
 * replacements for its build-time CMake switches (CMakeLists.txt:5-199).
 */

/* ---- calculation mode (reference) ---- */
FDTD_ACTION ("--2d", "Run a two-dimensional scheme (TMz by default, see --2d-mode)")
FDTD_ACTION ("--3d", "Run the three-dimensional scheme")
FDTD_INT (logLevel, "--log-level", 0, "Verbosity of log output: 0 (quiet) .. 3 (debug)")

/* ---- area sizes (reference) ---- */
FDTD_INT (sizeX, "--sizex", 100, "Number of cells along x")
FDTD_INT (sizeY, "--sizey", 100, "Number of cells along y")
FDTD_INT (sizeZ, "--sizez", 100, "Number of cells along z")
FDTD_ACTION ("--same-size", "Copy the x size to y and z")
FDTD_INT (pmlSizeX, "--pml-sizex", 10, "PML thickness (cells) at both x borders")
FDTD_INT (pmlSizeY, "--pml-sizey", 10, "PML thickness (cells) at both y borders")
FDTD_INT (pmlSizeZ, "--pml-sizez", 10, "PML thickness (cells) at both z borders")
FDTD_ACTION ("--same-size-pml", "Copy the x PML thickness to y and z")
FDTD_INT (tfsfSizeX, "--tfsf-sizex", 20, "Distance (cells) of the TF/SF box from both x borders")
FDTD_INT (tfsfSizeY, "--tfsf-sizey", 20, "Distance (cells) of the TF/SF box from both y borders")
FDTD_INT (tfsfSizeZ, "--tfsf-sizez", 20, "Distance (cells) of the TF/SF box from both z borders")
FDTD_ACTION ("--same-size-tfsf", "Copy the x TF/SF distance to y and z")
FDTD_INT (ntffSizeX, "--ntff-sizex", 15, "Distance (cells) of the NTFF surface from both x borders")
FDTD_INT (ntffSizeY, "--ntff-sizey", 15, "Distance (cells) of the NTFF surface from both y borders")
FDTD_INT (ntffSizeZ, "--ntff-sizez", 15, "Distance (cells) of the NTFF surface from both z borders")
FDTD_ACTION ("--same-size-ntff", "Copy the x NTFF distance to y and z")

/* ---- time (reference) ---- */
FDTD_INT (numTimeSteps, "--time-steps", 100, "Number of leapfrog time steps")
FDTD_INT (numAmplitudeTimeSteps, "--amplitude-time-steps", 10, "Step budget between convergence checks in amplitude mode")

/* ---- incident wave (reference, degrees) ---- */
FDTD_FLOAT (incidentWaveAngle1, "--angle-teta", 90.0, "Incident wave polar angle theta (degrees)")
FDTD_FLOAT (incidentWaveAngle2, "--angle-phi", 0.0, "Incident wave azimuth angle phi (degrees)")
FDTD_FLOAT (incidentWaveAngle3, "--angle-psi", 90.0, "Incident wave polarisation angle psi (degrees)")

/* ---- concurrency (reference) ---- */
FDTD_INT (bufferSize, "--buffer-size", 1, "Ghost-layer depth; halos are exchanged every N steps (deep halo)")
FDTD_INT (numCudaGPUs, "--num-cuda-gpus", 1, "Number of GPUs per node (rank r uses device r % N)")
FDTD_BOOL (doUseParallelGrid, "--parallel-grid", "Decompose the grid over all ranks of the job")
FDTD_BOOL (doUseOptimalVirtualTopology, "--optimal-topology", "Choose the rank grid that minimises halo surface")
FDTD_STRING (fileWithAvailableTopologies, "--available-topologies", "nofile", "File listing allowed rank grids, one 'px py pz' per line")
FDTD_INT (topologySizeX, "--topology-sizex", 1, "Ranks along x of the virtual topology")
FDTD_INT (topologySizeY, "--topology-sizey", 1, "Ranks along y of the virtual topology")
FDTD_INT (topologySizeZ, "--topology-sizez", 1, "Ranks along z of the virtual topology")
FDTD_ACTION ("--same-size-topology", "Copy the x topology size to y and z")

/* ---- physics toggles (reference) ---- */
FDTD_BOOL (doUseDoubleMaterialPrecision, "--use-double-material-precision", "Sample materials on a grid twice as fine (8-point averaging)")
FDTD_BOOL (doUseTFSF, "--use-tfsf", "Inject a plane wave through a total-field/scattered-field box")
FDTD_BOOL (doUseNTFF, "--use-ntff", "Compute the near-to-far-field scattered power diagram")
FDTD_BOOL (doUsePML, "--use-pml", "Terminate the grid with absorbing layers")
FDTD_BOOL (doUseMetamaterials, "--use-metamaterials", "Enable Drude dispersive media")
FDTD_BOOL (doUseAmplitudeMode, "--use-amp-mode", "Run until the field amplitude converges")

/* ---- physics values (reference) ---- */
FDTD_FLOAT (gridStep, "--dx", 0.0005, "Spatial step (m)")
FDTD_FLOAT (sourceWaveLength, "--wavelength", 0.02, "Free-space wavelength of the source (m)")

/* ---- output (reference) ---- */
FDTD_BOOL (doSaveRes, "--save-res", "Write the final fields")
FDTD_BOOL (doSaveMaterials, "--save-materials", "Write the material grids")
FDTD_BOOL (doSaveIntermediateRes, "--save-interm-res", "Write fields every --interm-save-step steps")
FDTD_INT (intermediateSaveStep, "--interm-save-step", 100, "Interval (steps) of intermediate writes")
FDTD_BOOL (doSaveScatteredFieldRes, "--save-scattered-field-res", "Write the scattered field at the end")
FDTD_BOOL (doSaveScatteredFieldIntermediate, "--save-scattered--field-interm", "Write the scattered field at intermediate steps")

/* ---- meta (reference) ---- */
FDTD_ACTION_ARG ("--cmd-from-file", "Read the command line from a file: one token per line, no other options allowed")
FDTD_ACTION_ARG ("--save-cmd-to-file", "Write the command line (minus this option) to a file, one token per line")

/* ---- extensions: reference TODO list (Settings.inc:127-145) ---- */
FDTD_STRING (loadFromFile, "--load-from-file", "", "Resume from a checkpoint directory written by --checkpoint-dir")
FDTD_BOOL (doUsePointSource, "--use-point-source", "Force the hard point source even with TF/SF")
FDTD_BOOL (doGatherFullGrid, "--gather-full-grid", "Gather decomposed fields on rank 0 before writing")
FDTD_BOOL (saveExOnly, "--save-Ex-only", "Write only Ex")
FDTD_BOOL (saveEyOnly, "--save-Ey-only", "Write only Ey")
FDTD_BOOL (saveEzOnly, "--save-Ez-only", "Write only Ez")
FDTD_BOOL (saveHxOnly, "--save-Hx-only", "Write only Hx")
FDTD_BOOL (saveHyOnly, "--save-Hy-only", "Write only Hy")
FDTD_BOOL (saveHzOnly, "--save-Hz-only", "Write only Hz")
FDTD_BOOL (saveAsBMP, "--save-as-bmp", "Write fields as BMP slices (default when no format is given)")
FDTD_BOOL (saveAsDAT, "--save-as-dat", "Write fields as raw DAT files")
FDTD_BOOL (saveAsTXT, "--save-as-txt", "Write fields as text")
FDTD_STRING (dumperPalette, "--dumper-pallete", "rgb", "BMP palette: rgb or gray")
FDTD_INT (dumperOrthAxis, "--dumper-orth-axis", 2, "Axis orthogonal to BMP slices: 0=x 1=y 2=z")

/* ---- extensions: run-time replacements of build-time switches ---- */
FDTD_ACTION ("--1d", "Run the one-dimensional scheme (Ez/Hy line)")
FDTD_STRING (mode2D, "--2d-mode", "tmz", "Two-dimensional polarisation: tmz or tez")
FDTD_STRING (valueType, "--dtype", "f64", "Field precision: f32 or f64")
FDTD_BOOL (doUseComplexFieldValues, "--complex-field-values", "Complex fields (real and imaginary parts stepped as two real grids)")
FDTD_STRING (parallelBufferDimension, "--topology", "xyz", "Axes split across ranks: x, y, z, xy, yz, xz or xyz")
FDTD_STRING (backend, "--backend", "auto", "Compute backend: hip (MI355X kernels), torch (reference ops) or auto")
FDTD_STRING (device, "--device", "auto", "Torch device for the torch backend: cpu, cuda or auto")

/* ---- extensions: physics beyond the reference ---- */
FDTD_STRING (pmlType, "--pml-type", "upml", "Absorbing layer formulation: upml (reference D/B form) or cpml")
FDTD_FLOAT (cpmlKappaMax, "--cpml-kappa-max", 1.0, "CPML maximum kappa")
FDTD_FLOAT (cpmlAlphaMax, "--cpml-alpha-max", 0.0, "CPML maximum alpha (complex frequency shift)")
FDTD_STRING (sourceType, "--source", "sine", "Point source waveform: sine or gaussian")
FDTD_FLOAT (gaussianWidth, "--gaussian-width", 30.0, "Gaussian pulse width (steps)")
FDTD_FLOAT (gaussianDelay, "--gaussian-delay", 120.0, "Gaussian pulse delay (steps)")
FDTD_FLOAT (courantNum, "--courant", 0.5, "Courant number c*dt/dx")
FDTD_STRING (scene, "--scene", "reference", "Material scene: reference (hardcoded sphere setup), vacuum, sphere (dielectric) or drude-sphere (dispersive sphere in vacuum, needs --use-metamaterials); file (boxes, spheres and cylinders from --scene-file; Python driver)")
FDTD_STRING (sceneFile, "--scene-file", "", "With --scene file: the JSON scene file -- box (lo, hi), sphere (center, radius), cylinder (axis, center, radius, span) and mesh (file = a closed STL surface, or vertices + triangles; scale, translate; 3D) objects painted first to last over vacuum, each with eps and omega_p (in units of 2 pi f of the source; used with --use-metamaterials), coordinates in cells; smoothing linear or none")
FDTD_FLOAT (sphereEps, "--sphere-eps", 2.0, "Relative permittivity of the dielectric sphere")
FDTD_FLOAT (sphereRadius, "--sphere-radius", 20.0, "Radius (cells) of the dielectric sphere")
FDTD_FLOAT (sphereCenterX, "--sphere-center-x", 40.5, "Sphere centre x (cells)")
FDTD_FLOAT (sphereCenterY, "--sphere-center-y", 40.5, "Sphere centre y (cells)")
FDTD_FLOAT (sphereCenterZ, "--sphere-center-z", 40.5, "Sphere centre z (cells)")
FDTD_STRING (dispersion, "--dispersion", "drude", "Dispersive model of metamaterial regions: drude or lorentz")
FDTD_FLOAT (lorentzOmega0Ratio, "--lorentz-omega0", 0.5, "Lorentz resonance frequency as a fraction of the source frequency")
FDTD_INT (ntffStep, "--ntff-step", 100, "Interval (steps) of NTFF evaluations")
FDTD_STRING (checkpointDir, "--checkpoint-dir", "", "Directory for checkpoints (DAT files + JSON sidecar)")
FDTD_INT (checkpointStep, "--checkpoint-step", 0, "Interval (steps) of checkpoints; 0 = only at the end")
FDTD_STRING (outputDir, "--output-dir", ".", "Directory for field dumps")
FDTD_BOOL (doCheckFinite, "--check-finite", "Abort when a field becomes non-finite")
FDTD_INT (finiteCheckStep, "--finite-check-step", 100, "Interval (steps) of the non-finite check")
FDTD_BOOL (doUseHipGraph, "--use-hip-graph", "Capture the inner step loop into a HIP graph")
FDTD_BOOL (doProfilePhases, "--profile-phases", "Time every phase of the step loop with HIP events and print a breakdown")
FDTD_BOOL (doUseSplitKernels, "--split-kernels", "Disable the fused E+H kernel (used by default for plain 3D runs)")
FDTD_INT (amplitudeCheckSteps, "--amplitude-check-steps", 8, "Amplitude mode: steps whose changed-cell counts accumulate on the device between host reads (1 = check after every step)")
FDTD_INT (timeBlock, "--time-block", 0, "Leapfrog steps per HBM pass of the temporally blocked kernels: 3D 1..6 (fp64 1..4), 2D 1..8; 0 = automatic (3D fp32 5, fp64 4; 2D 7)")
FDTD_INT (hybridBlock, "--hybrid-block", 0, "3D runs with PML / TF-SF / dispersive media: steps per pass of the blocked core (stepped shell around it); 0 = automatic (5 on the fp32 HIP path), 1 = off")
FDTD_INT (shellStreams, "--shell-streams", 0, "Hybrid passes: HIP streams the independent stepped-shell window launches of a half step are spread over (0 = automatic: 2 on the HIP path -- the native driver uses 3 --, 1 = in order)")
FDTD_STRING (hybridGraph, "--hybrid-graph", "auto", "2D hybrid passes re-issued from a launch record once recorded (auto; graph = replayed from HIP graphs; off = planned every pass)")
FDTD_STRING (hybridTfsf, "--hybrid-tfsf", "auto", "Hybrid passes with TF/SF: where the TF/SF faces are corrected (auto / core = inside the blocked core pass when the incidence is along x or y, the stepped shell then only covers the absorbing layers; shell = the faces lie in the stepped shell; split = the x faces in the shell, the y / z faces in the core, which runs the TF/SF variant only on its y / z border slabs)")
FDTD_STRING (blockedDrude, "--blocked-drude", "auto", "Drude media (electric, uniform eps / gamma, 3D; fp32 and fp64, the native driver fp32): advance the dispersive box inside the blocked passes, its D / E history in registers (auto / on = also the torch oracle; off = the stepped dispersive box of the hybrid plan)")

/* ---- extensions: running-DFT field monitors (models/dft.py; Python driver) ---- */
FDTD_BOOL (doUseDft, "--use-dft", "Accumulate a running discrete Fourier transform of the fields on a box (amplitude and phase at every monitored wavelength from one real-valued run)")
FDTD_STRING (dftWavelengths, "--dft-wavelengths", "", "Monitored free-space wavelengths (m), comma separated, at most 8; empty = the source wavelength")
FDTD_INT (dftStep, "--dft-step", 0, "Steps between DFT samples; 0 = automatic (the largest multiple of the blocked pass length with at least 8 samples per shortest monitored period)")
FDTD_INT (dftStart, "--dft-start", 0, "First step at which the DFT monitor samples")
FDTD_INT (dftSizeX, "--dft-sizex", 0, "Distance (cells) of the DFT monitor box from both x borders (0 = the whole grid)")
FDTD_INT (dftSizeY, "--dft-sizey", 0, "Distance (cells) of the DFT monitor box from both y borders")
FDTD_INT (dftSizeZ, "--dft-sizez", 0, "Distance (cells) of the DFT monitor box from both z borders")
FDTD_ACTION ("--same-size-dft", "Copy the x DFT monitor distance to y and z")
FDTD_STRING (dftHTime, "--dft-h-time", "half", "Sample time of the H components in the DFT phase reference: half (their own time, half a step after E) or same (the E time)")
FDTD_BOOL (doUseNtffDft, "--ntff-dft", "With --use-ntff: monitor the NTFF surface slabs at the source wavelength and print the diagram of the phasors at the end of the run")
/* ---- extensions: Poynting-flux monitor on a closed box (models/flux.py; Python driver) ---- */
FDTD_BOOL (doUseFlux, "--use-flux", "Monitor the time-averaged power through the six faces of a box from running-DFT phasors (3D; wavelengths, step and start from --dft-wavelengths, --dft-step, --dft-start): radiated, scattered or absorbed power and, with TF/SF, the cross-section per wavelength")
FDTD_INT (fluxSizeX, "--flux-sizex", 0, "Distance (cells) of the flux box from both x borders")
FDTD_INT (fluxSizeY, "--flux-sizey", 0, "Distance (cells) of the flux box from both y borders")
FDTD_INT (fluxSizeZ, "--flux-sizez", 0, "Distance (cells) of the flux box from both z borders")
FDTD_ACTION ("--same-size-flux", "Copy the x flux box distance to y and z")
FDTD_INT (fluxReportStep, "--flux-report-step", 0, "Steps between flux reports; 0 = only at the end of the run")
/* ---- extensions: far-field monitor on the NTFF surface (models/farfield.py; Python driver) ---- */
FDTD_BOOL (doUseFarfield, "--use-farfield", "Monitor the far field of the currents on a closed box from running-DFT phasors (3D; wavelengths, step and start from --dft-wavelengths, --dft-step, --dft-start): radiant intensity, total radiated power, directivity and, with TF/SF, the bistatic RCS per wavelength")
FDTD_INT (farfieldSizeX, "--farfield-sizex", 0, "Distance (cells) of the far-field box from both x borders (0 = the --ntff-size* value)")
FDTD_INT (farfieldSizeY, "--farfield-sizey", 0, "Distance (cells) of the far-field box from both y borders")
FDTD_INT (farfieldSizeZ, "--farfield-sizez", 0, "Distance (cells) of the far-field box from both z borders")
FDTD_ACTION ("--same-size-farfield", "Copy the x far-field box distance to y and z")
FDTD_INT (farfieldNTheta, "--farfield-ntheta", 37, "Polar angles of the far-field report grid, uniform over [0, pi] with both ends")
FDTD_INT (farfieldNPhi, "--farfield-nphi", 72, "Azimuthal angles of the far-field report grid, uniform over [0, 2 pi)")
/* ---- extensions: field-energy monitor and decay-based stop (models/energy.py; Python driver) ---- */
FDTD_BOOL (doUseEnergy, "--use-energy", "Monitor the vacuum-weighted field energy (1/2 eps0 E^2 + 1/2 mu0 H^2) in a box: a time series in the --json line, one line per sample with --log-level >= 1")
FDTD_INT (energySizeX, "--energy-sizex", 0, "Distance (cells) of the energy box from both x borders (0 = the whole grid)")
FDTD_INT (energySizeY, "--energy-sizey", 0, "Distance (cells) of the energy box from both y borders")
FDTD_INT (energySizeZ, "--energy-sizez", 0, "Distance (cells) of the energy box from both z borders")
FDTD_ACTION ("--same-size-energy", "Copy the x energy box distance to y and z")
FDTD_INT (energyStep, "--energy-step", 0, "Steps between energy samples; 0 = automatic (a multiple of the blocked pass length or of the DFT / flux sampling step, at least 50)")
FDTD_INT (energyStart, "--energy-start", 0, "First step at which the energy monitor samples")
FDTD_FLOAT (stopDecayBy, "--stop-decay-by", 0.0, "Stop the run once the source has ended and the field energy in the box has fallen to this fraction of its peak (--time-steps stays the upper bound; pulsed sources only); 0 = off; implies --use-energy")
/* ---- extensions: field probes, time series and spectra at points (models/probe.py; Python driver) ---- */
FDTD_BOOL (doUseProbes, "--use-probes", "Record the fields at the --probe-points as time series, sampled between passes: points, samples and spectrum in the --json line, one text table per point with --save-res")
FDTD_STRING (probePoints, "--probe-points", "", "Probe points as global cell indices, x,y,z;x,y,z;... (x,y in 2D, x in 1D)")
FDTD_STRING (probeFile, "--probe-file", "", "File with further probe points, one per line: indices separated by commas or blanks, # starts a comment")
FDTD_STRING (probeComponents, "--probe-components", "", "Recorded field components, comma separated; empty = every component of the scheme")
FDTD_STRING (probePosition, "--probe-position", "node", "Where a component is taken: node (its own Yee sample at the index, an exact copy) or centre (the mean of its 1, 2 or 4 samples around the cell centre)")
FDTD_INT (probeStep, "--probe-step", 0, "Steps between probe samples; 0 = automatic (the blocked pass length, or the sampling step of the DFT / flux / far-field / energy monitors: no pass is cut)")
FDTD_INT (probeStart, "--probe-start", 0, "First step at which the probes sample")
FDTD_INT (probeSpectrum, "--probe-spectrum", 0, "Report the spectrum of the probe series at this many wavelengths, evenly spaced in frequency over --probe-band (with --source gaussian divided by the source signal's spectrum); 0 = none")
FDTD_STRING (probeBand, "--probe-band", "", "Band of --probe-spectrum as free-space wavelengths lo,hi (m)")
/* ---- extensions: source files, soft and hard dipole sources at chosen cells (layout/source_file.py; Python driver) ---- */
FDTD_STRING (sourceFile, "--source-file", "", "JSON file with a list of sources that replaces the built-in point source: per entry a component, the cell of its Yee sample, soft (added) or hard (set), an amplitude and a sine, gaussian or pulse signal; 2D and 3D")
FDTD_BOOL (doPrintJson, "--json", "Print a JSON summary line after the run")
FDTD_INT (warmupSteps, "--warmup-steps", 0, "Untimed time steps run before the timed loop (benchmarking; they advance the simulation)")
