// Oracle driver: runs the reference program's serial scheme for one argument list
// and writes its grids at full precision.
//
// This file is the project's own.  It is compiled against the reference's
// headers and sources (see build_ref.py) and links nothing of ours.  It sets the
// scheme up the way a serial run of the reference does -- its settings parser,
// its layout, its scheme, initScheme / initGrids / performSteps -- and then hands
// the scheme's grids to the reference's own DAT dumper, which writes raw field
// values to "current[<steps>]_rank-0_<name>.dat" in the working directory.
//
// The grids are private members of the scheme classes.  They are reached with
// the explicit-instantiation idiom: access checks do not apply to the arguments
// of an explicit template instantiation, so `template struct Open<Tag, &S::m>`
// may name a private member, and the friend function it defines returns the
// pointer-to-member to ordinary code.
//
// Lines starting with "oracle:" on stdout carry the scalars of the run (dt,
// Courant number, relative phase velocity of the incident line, grid sizes).

#include <cstdio>
#include <string>

#include "Grid.h"
#include "DATDumper.h"
#include "PhysicsConst.h"
#include "Settings.h"

#ifdef GRID_3D
#include "Scheme3D.h"
typedef Scheme3D SchemeT;
typedef GridCoordinate3D CoordT;
#endif
#ifdef GRID_2D
#include "SchemeTMz.h"
typedef SchemeTMz SchemeT;
typedef GridCoordinate2D CoordT;
#endif

// the parser fills the reference's one global settings object
extern Settings solverSettings;

typedef Grid<CoordT> FieldT;
typedef Grid<GridCoordinate1D> LineT;

template <class Tag, typename Tag::type Member>
struct Open
{
  friend typename Tag::type reach (Tag) { return Member; }
};

#define OPEN_MEMBER(tag, type_, member) \
  struct tag { typedef type_ SchemeT::*type; friend type reach (tag); }; \
  template struct Open<tag, &SchemeT::member>

#ifdef GRID_3D
OPEN_MEMBER (TagEx, FieldT, Ex);
OPEN_MEMBER (TagEy, FieldT, Ey);
OPEN_MEMBER (TagHz, FieldT, Hz);
OPEN_MEMBER (TagRelV, FPValue, relPhaseVelocity);
#endif
OPEN_MEMBER (TagEz, FieldT, Ez);
OPEN_MEMBER (TagHx, FieldT, Hx);
OPEN_MEMBER (TagHy, FieldT, Hy);
OPEN_MEMBER (TagEps, FieldT, Eps);
OPEN_MEMBER (TagOmegaPE, FieldT, OmegaPE);
OPEN_MEMBER (TagOmegaPM, FieldT, OmegaPM);
OPEN_MEMBER (TagSigmaX, FieldT, SigmaX);
OPEN_MEMBER (TagSigmaY, FieldT, SigmaY);
OPEN_MEMBER (TagSigmaZ, FieldT, SigmaZ);
OPEN_MEMBER (TagEInc, LineT, EInc);
OPEN_MEMBER (TagHInc, LineT, HInc);
OPEN_MEMBER (TagDt, FPValue, gridTimeStep);
OPEN_MEMBER (TagCourant, FPValue, courantNum);

template <class TCoord>
static void
dump (Grid<TCoord> &grid, time_step step, const char *name)
{
  DATDumper<TCoord> dumper;
  dumper.init (step, CURRENT, 0, name);
  dumper.dumpGrid (grid, TCoord (0), grid.getSize ());
}

#ifdef GRID_3D
static void
printSize (const char *name, const GridCoordinate3D &s)
{
  printf ("oracle: size %s %d %d %d\n", name, (int) s.getX (), (int) s.getY (), (int) s.getZ ());
}
#endif
#ifdef GRID_2D
static void
printSize (const char *name, const GridCoordinate2D &s)
{
  printf ("oracle: size %s %d %d\n", name, (int) s.getX (), (int) s.getY ());
}
#endif

#define DUMP(tag, name) \
  do { printSize (name, (scheme.*reach (tag ())).getSize ()); dump (scheme.*reach (tag ()), steps, name); } while (0)

// What one run needs from the command line, read once from the reference's settings object.
struct Run
{
  grid_coord n[3], pml[3], tfsf[3];
  FPValue angle[3];   // teta, phi, psi in radians
  time_step steps, ampSteps;
  bool amp, usePml, useTfsf, meta, ntff, doubleMaterial;
  FPValue dx, lambda;

  explicit Run (Settings &o)
  {
    const FPValue rad = PhysicsConst::Pi / 180.0;
    n[0] = o.getSizeX (); n[1] = o.getSizeY (); n[2] = o.getSizeZ ();
    pml[0] = o.getPMLSizeX (); pml[1] = o.getPMLSizeY (); pml[2] = o.getPMLSizeZ ();
    tfsf[0] = o.getTFSFSizeX (); tfsf[1] = o.getTFSFSizeY (); tfsf[2] = o.getTFSFSizeZ ();
    angle[0] = o.getIncidentWaveAngle1 () * rad;
    angle[1] = o.getIncidentWaveAngle2 () * rad;
    angle[2] = o.getIncidentWaveAngle3 () * rad;
    steps = o.getNumTimeSteps (); ampSteps = o.getNumAmplitudeSteps ();
    amp = o.getDoUseAmplitudeMode (); usePml = o.getDoUsePML (); useTfsf = o.getDoUseTFSF ();
    meta = o.getDoUseMetamaterials (); ntff = o.getDoUseNTFF ();
    doubleMaterial = o.getDoUseDoubleMaterialPrecision ();
    dx = o.getGridStep (); lambda = o.getSourceWaveLength ();
  }

  // a triple as the build's coordinate type (the 2D build keeps x and y)
  CoordT coord (const grid_coord *v) const
  {
#ifdef GRID_3D
    return CoordT (v[0], v[1], v[2]);
#else
    return CoordT (v[0], v[1]);
#endif
  }
};

int
main (int argc, char **argv)
{
  solverSettings.SetupFromCmd (argc, argv);
  const Run run (solverSettings);
  const time_step steps = run.steps;
  const CoordT whole = run.coord (run.n);

  YeeGridLayout layout (whole, run.coord (run.pml), run.coord (run.tfsf), run.angle[0], run.angle[1], run.angle[2],
                        run.doubleMaterial);

  // The two scheme classes differ in one constructor argument: Scheme3D takes the NTFF switch where SchemeTMz
  // takes the incident angle.  Results are never written as bitmaps (last argument).
#ifdef GRID_3D
#define SCHEME_EXTRA run.meta, run.ntff
#else
#define SCHEME_EXTRA run.angle[1], run.meta
#endif
  SchemeT scheme (&layout, whole, steps, run.amp, run.ampSteps, run.usePml, run.useTfsf, SCHEME_EXTRA, false);

  scheme.initScheme (run.dx, PhysicsConst::SpeedOfLight / run.lambda);
  scheme.initGrids ();

  // materials as initGrids left them, before any step
  DUMP (TagEps, "Eps");
  DUMP (TagOmegaPE, "OmegaPE");
  DUMP (TagOmegaPM, "OmegaPM");
  DUMP (TagSigmaX, "SigmaX");
  DUMP (TagSigmaY, "SigmaY");
#ifdef GRID_3D
  DUMP (TagSigmaZ, "SigmaZ");
#endif

  scheme.performSteps ();

#ifdef GRID_3D
  DUMP (TagEx, "Ex");
  DUMP (TagEy, "Ey");
#endif
  DUMP (TagEz, "Ez");
  DUMP (TagHx, "Hx");
  DUMP (TagHy, "Hy");
#ifdef GRID_3D
  DUMP (TagHz, "Hz");
#endif
  if (run.useTfsf)
  {
    printf ("oracle: size EInc %d\n", (int) (scheme.*reach (TagEInc ())).getSize ().getX ());
    dump (scheme.*reach (TagEInc ()), steps, "EInc");
    dump (scheme.*reach (TagHInc ()), steps, "HInc");
  }

  printf ("oracle: steps %u\n", (unsigned) steps);
  printf ("oracle: dx %.17g\n", (double) run.dx);
  printf ("oracle: wavelength %.17g\n", (double) run.lambda);
  printf ("oracle: dt %.17g\n", (double) (scheme.*reach (TagDt ())));
  printf ("oracle: courant %.17g\n", (double) (scheme.*reach (TagCourant ())));
#ifdef GRID_3D
  printf ("oracle: rel_phase_velocity %.17g\n", (double) (scheme.*reach (TagRelV ())));
#endif
  printf ("oracle: value_bytes %d\n", (int) sizeof (FieldValue));

  return 0;
}
