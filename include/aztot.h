/* aztot.h - C ABI of the MI355X-native azTotMD per-step hot path.
 *
 * The reference (raadyn/aztotmd) has no plugin/FFI interface: its hot path is the set of free
 * functions and kernels that main.cu calls on one opaque device struct.  Each entry point below
 * names the reference interface it replaces (paths relative to the reference's src/).
 * Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * All functions return AZTOT_OK (0) on success and a negative code on failure;
 * aztot_last_error() returns a human readable message for the calling thread.
 * A handle is single-threaded (as the reference: one host thread, main.cu:239).
 *
 * Units everywhere: Angstrom, ps, eV, e; masses in amu at this boundary (the reference's input units,
 * const.h:17-49).
 */
#ifndef AZTOT_H
#define AZTOT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZTOT_OK 0
#define AZTOT_ERR_IO -1          /* cannot open / parse an input file (reference: printf("ERROR[..]") + return 0) */
#define AZTOT_ERR_INPUT -2       /* semantically invalid or out-of-scope input */
#define AZTOT_ERR_DEVICE -3      /* HIP runtime error / no device */
#define AZTOT_ERR_ARG -4
#define AZTOT_ERR_COMM -5

/* pair potential ids: vdw.h:15-21 */
enum { AZTOT_VDW_LJ = 1, AZTOT_VDW_BUCK = 2, AZTOT_VDW_746 = 3, AZTOT_VDW_BHM = 4, AZTOT_VDW_ELIN = 5, AZTOT_VDW_EINV = 6, AZTOT_VDW_SURK = 7 };
/* electrostatics: elec.h:8-12 */
enum { AZTOT_ELEC_NONE = 0, AZTOT_ELEC_DIRECT = 1, AZTOT_ELEC_EWALD = 2, AZTOT_ELEC_FENNEL = 3,
       AZTOT_ELEC_SPME = 4 };   /* ours: smooth particle-mesh Ewald, 'elec spme rReal alpha Kx Ky Kz order' (see aztot_spme_mesh below) */
/* thermostats: temperature.h:10-12 */
enum { AZTOT_TSTAT_NONE = 0, AZTOT_TSTAT_NOSE = 1, AZTOT_TSTAT_RADI = 2 };
/* init_vel: dataStruct.h:7-10 */
enum { AZTOT_VEL_ZERO = 0, AZTOT_VEL_GAUSS = 1, AZTOT_VEL_CONST = 2, AZTOT_VEL_KENG = 3 };

typedef struct aztot_model aztot_model;   /* host model: Atoms+Field+Sim+Elec+TStat+Box of dataStruct.h */
typedef struct aztot_md aztot_md;         /* device state: cudaMD + hostManagMD of cuStruct.h:81-423 */

/* one line of the 'spec' section of field.txt (sys_init.cpp:83) + its 'radii' line (sys_init.cpp:468-480) */
typedef struct
{
    char name[8];
    double mass_amu, charge;
    int32_t frozen;              /* 'frozensp' section, sys_init.cpp:241-255 */
    double radA, radB, mxEng;
} aztot_species;

/* one line of the 'vdw' section of field.txt (vdw.cpp:244): raw user parameters */
typedef struct
{
    int32_t spec_a, spec_b, type;
    double rcut;
    double p[5];
} aztot_vdw;

/* the directives of control.txt that touch the hot path (sys_init.cpp:676-989) */
typedef struct
{
    double timestep;             /* ps */
    int32_t nstep, nequil, eqfreq;
    double temperature;          /* K */
    int32_t tstat_type;          /* AZTOT_TSTAT_* */
    double tstat_tau;            /* 'nose tau' */
    int32_t elec_type;           /* AZTOT_ELEC_* */
    double r_real, alpha;        /* elec cut-off, Ewald/Fennell alpha */
    int32_t init_vel;            /* AZTOT_VEL_* */
    double init_vel_par[3];      /* const vx vy vz | keng e */
    double elecfield[3];         /* dU/dx, dU/dy, dU/dz */
    int32_t use_cell_list;       /* 'cell_list' present */
    double cell_list;            /* desired cell edge */
    int32_t stat;                /* statistics period */
    int32_t ewald_k[3];          /* 'elec pme rReal alpha kx ky kz' (read_elec elec.cpp:33-38): k-vectors per axis, 1..48 (kEwaldKMax, csrc/model.h) */
    int32_t spme_mesh[3];        /* 'elec spme rReal alpha Kx Ky Kz order' (ours): mesh points per axis, each a power of two in 8..256 */
    int32_t spme_order;          /* ... and the B-spline order: 4, 6 or 8 */
} aztot_control;

/* array form of atoms.xyz + field.txt + control.txt (used by tests / bench; same state as aztot_init_md) */
typedef struct
{
    int32_t n_atoms, n_species, n_vdw;
    double box[3];
    const int32_t *types;
    const double *x, *y, *z, *vx, *vy, *vz;   /* vx..vz may be NULL (zeros) */
    const aztot_species *species;
    const aztot_vdw *vdw;
    aztot_control control;
} aztot_system;

/* bonded terms ("next" row: constant bonds + harmonic-cosine angles) */
enum { AZTOT_BOND_HARM = 1, AZTOT_BOND_MORSE = 2, AZTOT_BOND_PEDONE = 3, AZTOT_BOND_BUCK = 4, AZTOT_BOND_E612 = 5 };   /* bonds.cpp:158-252 */
enum { AZTOT_ANGLE_HCOS = 1 };                                                                                      /* angles.cpp:111 */

/* one line of the 'bonds' section of field.txt (read_bond, bonds.cpp:125-364) with the 'con con' tail:
   harm k r0 | mors D a r0 C | pdn D a r0 C E | buck A ro C | e612 A ro C D F */
typedef struct
{
    int32_t spec_a, spec_b, type;
    double p[5];
} aztot_bond_type;

/* one line of the 'angles' section of field.txt (read_angle, angles.cpp:78-128): centralSpec hcos k cos0 */
typedef struct
{
    int32_t central, type;
    double k, cos0;
} aztot_angle_type;

/* type tables + the contents of bonds.txt (read_bondlist, bonds.cpp:25-110) and angles.txt (read_anglelist,
   angles.cpp:22-60).  Atom indices are 0-based; type ids are 1-based as in the files (id k = entry k-1 of the table). */
typedef struct
{
    int32_t n_bond_types, n_angle_types, n_bonds, n_angles;
    const aztot_bond_type *bond_types;
    const aztot_angle_type *angle_types;
    const int32_t *bond_a, *bond_b, *bond_type;
    const int32_t *angle_c, *angle_l1, *angle_l2, *angle_type;
} aztot_bonded;

/* run-time switches that replace the reference's compile-time defines.h (defines.h:5-23) and the kernel-launch file cuda.txt (cuInit.cu:701-749),
   and settle the differences between the reference's two mains.  Always start from aztot_default_options(): it fills struct_size, and a
   library that is handed a struct of another size refuses it (AZTOT_ERR_ARG) instead of reading fields that are not there.
   Measurement switches (A/B comparisons of kernel paths, phase timing) are NOT part of this struct: they are read from the environment variable
   AZTOT_DEBUG when a device handle is created (a bit mask; the bits are listed in aztotmd_amd/csrc/engine.h, enum DebugBit). */
typedef struct
{
    uint32_t struct_size;        /* sizeof(aztot_options) of the caller, set by aztot_default_options */
    int32_t device;              /* HIP device ordinal (reference: device 0 hard-coded, cuInit.cu:688) */
    int32_t initial_forces;      /* 1: forces of the initial configuration are computed at init (serial path,
                                       sys_init.cpp:1181-1184); 0: start from F = 0 (GPU path, sys_init.cpp:551-553) */
    int32_t center_box;          /* 1: apply center_box at init (serial path only, sys_init.cpp:1145) */
    uint64_t seed;               /* seed of the counter-based RNG (thermostat, tables, init_vel) */
    int32_t pair_variant;        /* 0: auto (= 2 where the geometry allows, else 1); 1: per-atom gather kernel; 2: LDS-tiled wave-per-cell kernels (+ pair lists) */
    double cell_size;            /* 0: derive from control.cell_list / cut-off (+ skin); >0: force this cell edge */
    int32_t use_graph;           /* 1: replay the step as a captured hipGraph when possible */
    int32_t profile;             /* 1: time every kernel with HIP events (aztot_kernel_times) */
    int32_t sort_every;          /* cell-list rebuild schedule.  0 (default): adaptive - the cells are rebuilt only when an atom could have used up its
                                    share of the skin (exact; the reference rebuilds every step, main.cu:300-326, and results then differ from an
                                    every-step run in summation order only); 1: every step, the reference's schedule; n > 1: adaptive, at most every n-th step */
    double skin;                 /* Verlet skin in Angstrom: the pair lists hold every pair within cut-off + skin, an atom may move skin / 2 between two rebuilds.
                                    0 (default): automatic (about 4 % of the cut-off; cells are sized cut-off + skin when control.cell_list asks for cells
                                    of about the cut-off); > 0: this value; < 0: no skin - cells exactly as control.cell_list / split_cells
                                    (cuCellList.cu:9-34) give them, the slack is whatever the cell edge happens to overhang the cut-off */
    int32_t waves_per_cell;      /* waves that share one cell in the pair kernels (list kernel: 1 / 2 / 4, they split the cell's atoms over one LDS tile;
                                    staging kernel: 1 / 2 / 4 / 8, they split the stencil's columns).  0 (default): the engine decides - several where
                                    cells are few, tiles large or stencils wide */
    int32_t energies_every_step; /* 1: pair energies are booked on every step (0, default: only on the last step of an aztot_step call, the only one whose
                                    statistics the caller can see; forces and trajectories are bit-identical either way) */
    int32_t loopback_ranks;      /* measurement aid for aztot_init_device_slab without a transport: 1 = this rank exchanges its halo with itself
                                    (one rank of N on one GPU; never a result): what it sends to one side comes back from the other, one slab width
                                    along x away, so the physics is that of a system made of N copies of this slab.
                                    2 = the same for a model that IS such a system - a box of N exact translates of one period along x, copy k of atom j
                                    having id j * N + k; n_atoms and the cell layers along x must divide by N -: an atom or ghost that arrives from the
                                    left is the left neighbour's copy (k - 1 modulo N), one from the right the right neighbour's (k + 1).
                                    The rank then holds the atoms rank r of a real N-rank run of that box would hold, under their ids: bond and angle
                                    partners across a seam are found, and aztot_md_to_host fills the atoms that moved in.  (With 1 an atom that leaves on
                                    one side comes back as itself, and a bonded term across a seam finds no partner.)  This is what the tests hold a
                                    device-side slab rank to: plain NVE with pair, Fennell / direct and bonded forces follows the one-GPU run of the box.
                                    What does NOT follow any box, with 1 or 2: all-rank sums are rank-local under loopback (the statistics of aztot_get_stats
                                    are this rank's share; the Ewald structure factor, the Nose-Hoover and equilibration kinetic energy are those of one
                                    slab alone), and randomness keyed by atom id (the radiative thermostat's draws and photon index) differs between the
                                    copies of a replicated box, which then stop being copies.  With the Ewald sum, Nose-Hoover, equilibration rescaling or
                                    the radiative thermostat a loopback rank's timing is meaningful, its physics is not. */
    int32_t reserved[5];         /* must be zero */
} aztot_options;

/* per-step scalars: the fields tracked by stat.dat (cuStat.cu:241-261) + serial calc_chars (integrators.cpp:63-73) */
typedef struct
{
    int64_t step;                /* number of completed steps */
    double time;                 /* ps */
    double engTot, engKin, engVdW, engCoul, engElecField, engTemp, engPot;
    double temperature;          /* 2 engKin / (degFree kB) */
    double posMom[3], negMom[3]; /* wall momentum accumulators (box.cpp:230-295; cuMDfunc.cu:72-106) */
    int64_t posCross[3], negCross[3];
    double pressure;             /* from wall momentum over the last 'stat' window (main.cpp:146-152) */
    int64_t pairs_dropped;       /* pairs skipped by the |f|^2 > 1e10 rule (integrators.cpp:170) */
    int64_t n_cells;
    double nose_chit, nose_conint;  /* Nose-Hoover friction and conserved-quantity integral (temperature.h:24-25) */
    double engBond, engAngle;    /* exec_bondlist bonds.cpp:1218, exec_anglelist angles.cpp:240; both are part of engTot */
    double engCoulRec, engCoulConst; /* Ewald sum: reciprocal part (engElec2, elec.cpp:333 ; cudaMD::engCoul2) and constant part
                                        (engElec1, ewald_const elec.cpp:144 ; engCoul3); engCoul above is the real-space part */
    int64_t sort_interval;       /* steps between two rebuilds of the cell list that the next aztot_step call will use (1: every step) */
    int64_t sort_violations;     /* calls so far in which an atom left its cell's slack before the scheduled rebuild (handled exactly: by a wider stencil on one GPU, by running the steps since the last look again - from a device-side snapshot, cells rebuilt every step - on slab ranks and on small systems) */
    int64_t pair_lists;          /* 1: the steps between two rebuilds walk per-atom pair lists recorded at the rebuild (k_pair_list) ; 0: they stage every cell */
    int64_t cells_without_list;  /* cells that did not fit the lists at the last rebuild (more than 64 atoms, tile or list full): staged in full every step */
    int64_t rebuilds;            /* steps so far that rebuilt the cell list (clear_clist .. sort_atoms of main.cu:300-326; the reference: every step) */
    double skin;                 /* the Verlet skin in force, Angstrom: pair lists reach cut-off + skin, an atom may move skin / 2 between two rebuilds (0: none) */
} aztot_stats;

/* host copy of the per-atom state, fp64 SoA, in ORIGINAL atom order (id order); any pointer may be NULL */
typedef struct
{
    int32_t n_atoms;
    double *x, *y, *z, *vx, *vy, *vz, *fx, *fy, *fz, *U, *radius;
    int32_t *types;
} aztot_state;

/* ---- host model: replaces init_md / free_md (sys_init.h:11,17) ------------------------------------- */
/* reads atoms.xyz, field.txt, control.txt, cuda.txt from `dir` (reference: from the cwd) */
int aztot_init_md(const char *dir, aztot_model **out);
int aztot_model_create(const aztot_system *sys, aztot_model **out);
/* attach bonded terms to a model made by aztot_model_create (aztot_init_md reads them from field.txt + bonds.txt +
   angles.txt itself); replaces sys_init.cpp:289-314,411-427,626-673.  Must precede aztot_init_device. */
int aztot_model_set_bonded(aztot_model *m, const aztot_bonded *b);
/* string-keyed read-out of parsed/derived values as doubles; returns the number of values written
   (or needed, if cap is too small), negative on unknown key.  Keys: see aztotmd_amd/csrc/capi.cpp */
int aztot_model_query(const aztot_model *m, const char *key, double *out, int cap);
/* name of species i as written in field.txt (NUL-terminated, at most cap-1 characters) */
int aztot_model_species_name(const aztot_model *m, int i, char *buf, int cap);
/* name of nucleus i (the second word of a 'spec' line of field.txt; models made by aztot_model_create: the species name).  Nuclei are numbered in order of
   first appearance among the species (read_spec, sys_init.cpp:86-103); aztot_model_query "nuclei" gives the nucleus of each species, "n_nuclei" their number */
int aztot_model_nucleus_name(const aztot_model *m, int i, char *buf, int cap);
void aztot_free_md(aztot_model *m);

/* ---- device: replaces init_cudaMD / md_to_host / free_device_md (cuInit.h:4,6,7) --------------------- */
/* number of HIP devices this process can use (0: none, never negative); the reference takes device 0 unasked (cuInit.cu:688) */
int aztot_device_count(void);
/* blocks until device `device` has finished all work queued by this process (hipDeviceSynchronize): what a launcher brackets a timed region with */
int aztot_device_synchronize(int device);
void aztot_default_options(aztot_options *opt);
int aztot_init_device(const aztot_model *m, const aztot_options *opt, aztot_md **out);
void aztot_free_device(aztot_md *md);

/* ---- the hot path ----------------------------------------------------------------------------------- */
/* n iterations of the loop body of main.cu:281-410 (reset_quantities, verlet_1stage, iter_fastCellList,
   verlet_2stage, apply_tstat, calc_quantities) with the serial path's fp64 arithmetic */
int aztot_step(aztot_md *md, int nsteps);
/* aztot_step on ONE GPU may return with the kernels of its steps queued and the end of the call - the last step's second half-kick where it is folded into
   the next step, the reduction of the statistics, the look at the cell-list rebuild schedule - still to come: every entry point that reads or writes state
   (aztot_get_stats, aztot_md_to_host, aztot_get_clock, aztot_set_state, aztot_forces, ...) completes it first, so callers see no difference, and a caller
   that steps one step at a time (the reference's loop is per step, main.cu:281-410, with a cudaThreadSynchronize behind every kernel) does not pay for a
   synchronisation per step.  aztot_sync completes everything explicitly and returns when the device has finished: what a timed region ends with.  An error
   detected only then is reported by the call that detects it.  After any error from aztot_step / aztot_sync the handle no longer steps (the first error is
   repeated); reads still work for a post-mortem.  Slab ranks and runs with bonded terms end every call synchronously. */
int aztot_sync(aztot_md *md);
/* cell-list build + sort + pair forces for the current positions: iter_fastCellList (cuPairs.h:8) alone */
int aztot_forces(aztot_md *md);
int aztot_get_stats(aztot_md *md, aztot_stats *out);
/* per-species wall crossings since init: out[6 * s + {0..5}] = species s through the walls Xn, Xp, Yn, Yp, Zn, Zp - the
   specAcBoxNeg / specAcBoxPos counters of put_periodic (cuMDfunc.cu:35-106) that the reference writes to msd.dat
   (cuStat.cu:278-288,345-350).  cap = number of int64 slots in out (>= 6 * n_species).  Collective on several ranks. */
int aztot_species_crossings(aztot_md *md, int64_t *out, int cap);
int aztot_md_to_host(aztot_md *md, aztot_state *out);
int aztot_set_state(aztot_md *md, const aztot_state *in);
/* Restart support (checkpoint row): the scalars of the device state that aztot_md_to_host / aztot_set_state do not carry.  A run restarted with
   aztot_set_state (x, v, f, U, radius of the checkpoint) + aztot_set_clock continues exactly: the step number drives the equilibration schedule
   (sys_init.cpp:700-712, nequil / eqfreq) and keys the thermostat's counter-based random numbers; the Nose-Hoover pair (temperature.h:24-25) and the
   kinetic energy the thermostats saw last (sim->engKin, integrators.cpp:305) are the thermostat's memory.  Wall-momentum and crossing counters restart
   from zero (they are running sums for the statistics, never fed back into the dynamics). */
typedef struct
{
    int64_t step;                /* completed steps (aztot_stats.step) */
    double nose_chit, nose_conint;
    double eng_kin;              /* kinetic energy after the last completed step, eV */
} aztot_clock;
int aztot_get_clock(aztot_md *md, aztot_clock *out);
int aztot_set_clock(aztot_md *md, const aztot_clock *in);
/* the cell list as the device holds it after the last sort: cudaMD::firstAtomInCell / cellIndexes (cuStruct.h:219-222;
   calc_firstAtomInCell cuSort.cu:130-143, sort_atoms cuSort.cu:145-197).  dims[3] = cells per axis of this rank's window;
   cell_start[c] = first slot of cell c = (ix * ny + iy) * nz + iz (n_cells + 1 entries, the last one = resident atoms);
   atom_id[s] = original index of the atom in slot s.  Either array may be NULL; caps are entry counts.  Returns the number of
   cells (or a negative error); never part of a step - a read-back for tests and restarts. */
int aztot_cell_table(aztot_md *md, int32_t dims[3], int32_t *cell_start, int cap_cells, int32_t *atom_id, int cap_atoms);

/* ---- radial distribution functions: brute_rdf / brute_nrdf + copy_rdf / copy_nrdf (cuStat.cu:436-760), get_rdf / out_rdf (rdf.cpp) -------
   One GPU only: a slab handle (nranks > 1, loopback included) is refused with AZTOT_ERR_INPUT.
   Bins:    n_bins = (int)(min(rmax, L_x) * (1 / dr)) (init_rdf, rdf.cpp:40-48); rmax <= 0, dr <= 0 or n_bins == 0 -> AZTOT_ERR_ARG.
   Pairs:   every unordered pair i < j whose minimum-image distance r (fp64, delta_periodic: one shift by L where |d| > L / 2) has r * r < rmax * rmax and
            bin = (int)(r * (1 / dr)) < n_bins is counted once in `bin`, whatever rmax is against the box.  Species pair (a, b), mn = min, mx = max:
            index mn * (nSpec - 1) + mn * (1 - mn) / 2 + mx (upper-triangular, row-major: the column order of rdf.dat); nuclei the same over nucleus indices.
   Counts:  uint64 totals [bin][pair] and an int64 number of samples: exact, independent of the order the pairs arrive in.  Unlike the reference (which
            clears its float histogram after 500 samples, cuStat.cu:576-583) nothing is ever cleared but by aztot_rdf_reset / aztot_rdf_setup.
   g(r):    count * V / (nA * nB) * 2 / (sphera * dr^3 * samples) / (3 i (i + 1) + 1) * C3, C3 = 1 for A-A, 0.5 for A-B, sphera = 4 pi / 3 (const.h:15);
            0 where nA * nB == 0 or before the first sample.  Bin centres r = (i + 0.5) dr.
   Timing:  aztot_rdf_sample first completes the deferred end of the last aztot_step call (as every reader does), then only READS the state: a run that
            samples gives bit-identical positions, velocities, forces and statistics to one that calls aztot_get_stats at the same points.
   Sampling or reading before aztot_rdf_setup -> AZTOT_ERR_ARG; a handle that failed earlier refuses to sample but can still be read. */
enum { AZTOT_RDF_SPECIES = 0, AZTOT_RDF_NUCLEI = 1 };
/* (re)allocate and zero; nuclei = 1 also fills the nuclei histogram (whatever the model's 'nucl' flag says).  Returns n_bins. */
int aztot_rdf_setup(aztot_md *md, double rmax, double dr, int nuclei);
/* one sample of the current configuration (the positions aztot_md_to_host would return); returns when the sample is taken and the device idle,
   as aztot_get_stats does */
int aztot_rdf_sample(aztot_md *md);
/* zero the totals and the sample count */
int aztot_rdf_reset(aztot_md *md);
/* histogram shape of `kind` (AZTOT_RDF_*): bins and pairs; AZTOT_ERR_ARG for AZTOT_RDF_NUCLEI when the setup did not ask for nuclei */
int aztot_rdf_shape(aztot_md *md, int kind, int *n_bins, int *n_pairs);
/* raw totals [bin][pair] into counts (if cap >= n_bins * n_pairs) and the number of samples; returns n_bins * n_pairs */
int aztot_rdf_counts(aztot_md *md, int kind, int64_t *samples, uint64_t *counts, int cap);
/* bin centres r[n_bins] and g[bin][pair] (if cap >= n_bins * n_pairs); returns n_bins * n_pairs */
int aztot_rdf_values(aztot_md *md, int kind, double *r, double *g, int cap);

/* ---- coordination numbers: out_cn (out_md.cpp:389-504, CN.dat) and out_ncn (out_md.cpp:196-387, nCN.dat) --------------------------------------------
   One GPU only: a slab handle (nranks > 1, loopback included) is refused with AZTOT_ERR_INPUT.  Two kinds, which can be set up side by side and
   differ in every detail:

                      AZTOT_CN_SPECIES ('outCN R nCentral names.. nLigand names..')      AZTOT_CN_NUCLEI ('ncn n' + n lines 'nucleus1 nucleus2 R')
     groups           species indices; all columns share one radius (sys_init.cpp:890-930)   nucleus indices (aztot_model_query "nuclei"); a radius per column
     columns          nCentral x nLigand, central-major, in the order the names appear      the n lines in file order, each ONE directed column
                      (out_md.cpp:465-472,481-483)                                           (central = nucleus1, ligand = nucleus2; pairInds, out_md.cpp:258)
     test             R * R >= r2, inclusive (out_md.cpp:434)                                r2 < R * R, strict (out_md.cpp:313,318)
     the atom itself  COUNTED when its species is central and ligand: the loop over j         never: pairs i < j only (out_md.cpp:301-304)
                      does not skip j == i, r2 = 0 (out_md.cpp:429)
     rows of the file CN = 0 ... largest count (mx starts at 0, out_md.cpp:392,486)          CN = min(10, smallest) ... max(0, largest) ('mn = 10; mx = 0',
                                                                                             out_md.cpp:300); no row at all when nothing lies in between
                                                                                             (no central atom and hence largest = 0 < 10)
     file             header 'CN' + '\t<central>-<ligand>' per column; rows '%d' CN + '\t%d' per column = number of central atoms of the column with that CN

   r2 is sqr_distance (box.cpp:297-305): differences of the positions aztot_md_to_host returns, delta_periodic (one shift by L where |d| > L / 2),
   (dx*dx + dy*dy) + dz*dz in fp64 without contraction.  R may exceed L / 2: each pair is still tested once, through its nearest image.
   An atom has a count in every column whose central group is its own, whatever the count; a central group without atoms gives an all-zero column.
   Where the reference is broken rather than peculiar, we do the sane thing:
     - out_ncn leaves the last atom out of its min / max (i < nAt - 1, out_md.cpp:301) and then indexes out[k][coords - mn] with it (out of bounds):
       here min / max run over all atoms;
     - a name twice in one outCN list, or the same (nucleus1, nucleus2) twice under ncn, leaves holes in the reference's tables: rejected
       (the parser with ERROR[201] / [202] / [b010], aztot_cn_setup with AZTOT_ERR_ARG);
     - an unknown nucleus name under ncn is used after the error message (out_md.cpp:246-262): rejected with ERROR[b010] / ERROR[b011].
   Counts are integers and a sample is a snapshot: aztot_cn_sample replaces the previous sample of its kind, nothing accumulates.
   Timing as aztot_rdf_sample: completes the deferred end of the last aztot_step call, only READS the state, returns with the device idle.
   Errors: null handle, unknown kind, group index out of range, radius <= 0, no columns, sampling before the set-up, reading before a sample
   -> AZTOT_ERR_ARG; a handle that failed earlier refuses to sample but can still be read. */
enum { AZTOT_CN_SPECIES = 0, AZTOT_CN_NUCLEI = 1 };
typedef struct aztot_cn_column
{
    int32_t central, ligand;     /* group indices: species (AZTOT_CN_SPECIES) or nuclei (AZTOT_CN_NUCLEI) */
    double radius;
} aztot_cn_column;
/* (re)allocate for `kind`: replaces its columns and forgets its last sample; the other kind is untouched.  AZTOT_CN_SPECIES: all radii must be equal */
int aztot_cn_setup(aztot_md *md, int kind, const aztot_cn_column *cols, int n_cols);
/* one snapshot of the current configuration (the positions aztot_md_to_host would return) */
int aztot_cn_sample(aztot_md *md, int kind);
/* the rows of the file: columns, first and last CN of the last sample (cn_max < cn_min: no row) */
int aztot_cn_shape(aztot_md *md, int kind, int *n_cols, int *cn_min, int *cn_max);
/* counts[atom id * n_cols + column] of the last sample, -1 where the atom is not of the column's central group (if cap >= n_atoms * n_cols);
   returns n_atoms * n_cols */
int aztot_cn_per_atom(aztot_md *md, int kind, int32_t *counts, int cap);
/* table[(cn - cn_min) * n_cols + column] = central atoms of the column with that CN (if cap >= rows * n_cols); returns rows * n_cols */
int aztot_cn_table(aztot_md *md, int kind, int64_t *table, int cap);

/* ---- time correlation functions: mean-square displacement (out_msd, out_md.cpp:89-124) and velocity autocorrelation (vaf_init / vaf_info,
   out_md.cpp:535-582) per species, averaged over a ring of time origins ------------------------------------------------------------------------------
   One GPU only: a slab handle (nranks > 1, loopback included) is refused with AZTOT_ERR_INPUT.

   A SAMPLE reads the state aztot_md_to_host would return at that moment: wrapped x y z, vx vy vz with the last step's second half-kick completed,
   types.  Samples are numbered c = 0, 1, 2, ... since the last set-up or reset.  Lags are counted IN SAMPLES; equal spacing in time is the caller's
   business.

   ORIGINS.  With n_origins M and origin_every E, sample c becomes an origin iff c % E == 0 and is then stored (positions and velocities of every
   atom, by atom id) in ring slot (c / E) % M, replacing the oldest.  n_lags = M * E.  Sample c is correlated with every live origin o, itself
   included (lag 0): every o with o % E == 0, o <= c and c - o < M * E.  The pair (c, o) contributes to lag c - o; within one sample all live origins
   have different lags.  The reference's single origin (x0s / vx0 taken once) is M = 1 with E >= the number of samples taken.

   PER-ATOM TERMS, fp64, every operation rounded on its own (no contraction), from atom i's current state and its state in origin o:
       d = x - x0 per axis, then delta_periodic (box.cpp:180-205): d > L / 2 -> d -= L, else d < -L / 2 -> d += L
       m_i = (dx*dx + dy*dy) + dz*dz                       (out_md.cpp:105-114)
       v_i = (vx*vx0 + vy*vy0) + vz*vz0                    (out_md.cpp:571)
   The minimum-image displacement is the reference's definition.  PRECONDITION: no atom moves farther than L / 2 along an axis within the largest lag;
   this cannot be detected (the integrator keeps no per-atom image counters), the bounded lag window is what makes it reasonable.

   PER-SPECIES SUMS IN ONE FIXED ORDER.  For species s let t[i] be the term of atom id i if types[i] == s, else +0.0, i = 0 ... N - 1.  Folding an
   array of 2^k values by halving: for h = 2^(k-1), ..., 2, 1: a[j] = a[j] + a[j + h] for every j < h; the result is a[0].  The sum is this tree:
     1. the ids, zero-padded to a multiple of 256, in runs of 64 consecutive ids: each run folded by halving (h = 32, ..., 1);
     2. the four run sums of each chunk of 256 ids folded by halving: (w0 + w2) + (w1 + w3);
     3. the chunk sums, zero-padded to the next power of two, folded by halving.
   A sample's sums are therefore a function of the state alone: they do not depend on the order the cell sort has left the atoms in, on the launch
   shape or on the run, and a few lines of numpy reproduce them bit for bit.  No floating-point atomics anywhere.

   ACCUMULATORS.  Per lag l: count[l] (pairs (c, o) seen) and per species msd_sum[l][s], vaf_sum[l][s], each updated as acc = acc + S once per
   contributing sample, in sample order.  Values: acc / (double)(count[l] * n_s), n_s = atoms of species s; 0.0 where count[l] == 0 or n_s == 0
   (the reference prints 0 / 0 for the MSD of an empty species, out_md.cpp:120).  With M = 1 these are the reference's displ / number and
   vaf / number.

   Memory: M * 48 * N bytes for the ring, 48 * N for the current state, the partial sums and 8 * n_lags * (1 + 2 * n_species) for the accumulators;
   a set-up that cannot allocate fails with AZTOT_ERR_DEVICE, leaves no sampler and a handle that still steps.
   Timing as aztot_rdf_sample: completes the deferred end of the last aztot_step call, only READS the state, returns with the device idle.
   Errors: null handle, n_origins or origin_every < 1, n_origins * origin_every > AZTOT_TCF_MAX_LAGS, sampling or reading before the set-up, a lag
   range outside [0, n_lags) -> AZTOT_ERR_ARG; a handle that failed earlier refuses to sample but can still be read. */
#define AZTOT_TCF_MAX_LAGS (1 << 24)
/* (re)allocate and zero: forgets every origin and sum of an earlier set-up; returns n_lags */
int aztot_tcf_setup(aztot_md *md, int n_origins, int origin_every);
/* one sample of the current state */
int aztot_tcf_sample(aztot_md *md);
/* zero sums and counts, forget the origins: the next sample is sample 0 */
int aztot_tcf_reset(aztot_md *md);
/* lags, species and samples since the set-up / reset (each pointer may be null) */
int aztot_tcf_shape(aztot_md *md, int *n_lags, int *n_species, int64_t *samples);
/* raw accumulators of lags [lag0, lag0 + n): count[lag - lag0], msd_sum / vaf_sum[(lag - lag0) * n_species + species] (if cap >= n * n_species; each
   pointer may be null); returns n * n_species */
int aztot_tcf_sums(aztot_md *md, int lag0, int n, int64_t *count, double *msd_sum, double *vaf_sum, int cap);
/* the normalised values in the same layout (if cap >= n * n_species); returns n * n_species */
int aztot_tcf_values(aztot_md *md, int lag0, int n, double *msd, double *vaf, int cap);

/* ---- pressure tensor: virial of the pair terms plus the kinetic part, one snapshot per sample ------------------------------------------------------
   The reference's only pressure is the momentum carried across the box walls (aztot_stats.pressure, main.cpp:143-163): zero in a crystal at rest, shot
   noise in a liquid, no off-diagonal components.  This sampler is ours.  aztot_stats.pressure is unchanged by it.
   One GPU only: a slab handle (nranks > 1, loopback included) is refused with AZTOT_ERR_INPUT; so are a model with bonded terms (the virial of bonds
   and angles is not built) and 'elec pme' (the reciprocal-space virial is not built).  A refused set-up leaves no sampler and a handle that steps on.
   Running averages are the caller's business: a sample replaces the previous one.

   A SAMPLE reads the state aztot_md_to_host would return at that moment: wrapped x y z, vx vy vz with the last step's second half-kick completed,
   types and radii.

   PAIR SEPARATION.  d = r_i - r_j per axis, then delta_periodic (box.cpp:180-205: one shift by L where |d| > L / 2);
   r2 = (dx*dx + dy*dy) + dz*dz in fp64, every operation rounded on its own: the rule of aztot_cn_sample.
   PAIR SET.  A pair takes part iff r2 <= rMax^2, rMax the largest cut-off of the model (aztot_model_query "rmax"; at most half the box).
   PAIR TERM.  The step kernels' own pair function supplies f = -(1/r) dU/dr and both energies: the per-pair VdW cut-off, the charged-species test,
   direct and Fennell Coulomb, surk with the per-atom radii, and the drop rule f^2 > 1e10 (integrators.cpp:170-174): energy booked, force and virial
   not.  The external field (elecfield) is not translation-invariant and contributes nothing.
   VIRIAL, eV, components ab in the order xx yy zz xy xz yz:   w_i[ab] = 1/2 sum_j f_ij d_a d_b,   W[ab] = sum_i w_i[ab].
   KINETIC.  K[ab] = sum_i m_i v_a v_b, m in internal units (amu * m_scale, aztot_model_query "m_scale"); atoms of a frozen species contribute nothing.
   PRESSURE, atm.  P[ab] = (K[ab] + W[ab]) / V * 1.58e6, the constant of the wall-momentum pressure (main.cpp:147); pressure_iso = (Pxx + Pyy + Pzz) / 3.
   eng_vdw, eng_coul: the pair energies of the same walk (half per visit); pairs: unordered pairs inside rMax, exact; pairs_dropped: those the drop
   rule took the force of.

   ORDER OF THE SUMS.  No floating-point atomics anywhere.  The totals W, K, eng_vdw and eng_coul are the tree of the time correlation functions
   (above, 'PER-SPECIES SUMS IN ONE FIXED ORDER') over the per-atom values in atom-id order.  The per-atom sums over partners run in an order that is a
   function of the sampled state alone (wrapped positions, ids, types, radii, N and the box): neighbour cells in a fixed order, ids ascending inside a
   cell, dealt to a number of lanes that depends on N only and folded in a fixed order.  It does not depend on the slot order the engine's sort has
   left, on arrival order or on the run: two handles holding the same state return the same bits.

   Timing as aztot_rdf_sample: completes the deferred end of the last aztot_step call, only READS the state, returns with the device idle.
   Out of scope: the virial of bonds and angles, the reciprocal Ewald part, slab ranks, running averages, any change to aztot_stats.pressure.
   Errors: null handle, sampling or reading before the set-up, reading before a sample, 0 < cap < 6 * n_atoms -> AZTOT_ERR_ARG; a handle that failed
   earlier refuses to sample but can still be read. */
typedef struct aztot_stress
{
    int64_t step; double time, volume;
    double kinetic[6], virial[6];      /* eV; xx yy zz xy xz yz */
    double pressure[6], pressure_iso;  /* atm */
    double eng_vdw, eng_coul;          /* eV, pair energies of the same walk */
    int64_t pairs, pairs_dropped;
} aztot_stress;                        /* 208 bytes */
/* (re)allocate; forgets the last sample */
int aztot_stress_setup(aztot_md *md);
/* one snapshot of the current state; replaces the previous sample */
int aztot_stress_sample(aztot_md *md);
/* the totals of the last sample */
int aztot_stress_get(aztot_md *md, aztot_stress *out);
/* w[6 * atom id + component] of the last sample; returns 6 * n_atoms (w null and cap 0: the size alone; a shorter buffer is AZTOT_ERR_ARG) */
int aztot_stress_per_atom(aztot_md *md, double *w, int cap);

/* ---- bond-angle distributions: the angle at a central atom between two of its neighbours, integer totals over the samples --------------------------
   The reference has no such output (nothing under its src/ computes an angle between neighbours): like the pressure tensor, this sampler is ours.
   One GPU only: a slab handle (nranks > 1, loopback included) is refused with AZTOT_ERR_INPUT.

   COLUMNS.  Column (c, a, b, R_a, R_b), species indices: the angle at a central atom i of species c between a neighbour j of species a and a
   neighbour k of species b; i, j and k are three different atoms.  Both shell tests are strict: 0 < r2_ij < R_a^2 and 0 < r2_ik < R_b^2 (an atom at
   distance exactly 0 has no direction: it is no neighbour).  (c, a, b) and (c, b, a) are the same column: the set-up normalises to a <= b and swaps the
   radii with them.  a == b: every unordered pair {j, k} is counted once; a != b: every (j, k) once.  A species without atoms is fine: the column stays zero.
   The set-up rejects with AZTOT_ERR_ARG: a null handle, n_bins outside [1, AZTOT_ADF_MAX_BINS], n_cols outside [1, AZTOT_ADF_MAX_COLUMNS], a species
   index out of range, a non-zero `reserved`, a radius <= 0, a == b with R_a != R_b, the same (c, {a, b}) twice.  A refused set-up leaves the earlier one.

   SEPARATION.  The rule of aztot_cn_sample on the positions aztot_md_to_host returns: u = r_j - r_i per axis, then delta_periodic (one shift by L where
   |d| > L / 2); r2 = (ux*ux + uy*uy) + uz*uz in fp64, every operation rounded on its own.  A radius may exceed L / 2: each partner is still seen once,
   through its nearest image.

   BINS, without acos, sqrt or a division.  n_bins bins of equal width in the angle: bin b is [180 b / n_bins, 180 (b + 1) / n_bins) degrees, the last
   one includes 180.  The edge table (aztot_adf_edges) is made on the host once per set-up: c_b = cos(pi b / n_bins) rounded to double (evaluated in extended
   precision, as a sine of the complementary angle towards 90 degrees: the nearest double or its neighbour), T_b = c_b * |c_b| in double (within 2 ulp
   of its exact value), with the exactly known values forced: T_0 = 1, T_n_bins = -1, and T_(n_bins / 2) = 0 when n_bins is even.  For a triplet with u = r_j - r_i, v = r_k - r_i:
       dot = (ux*vx + uy*vy) + uz*vz,   s = dot * |dot|,   p = r2_ij * r2_ik          (each operation rounded on its own)
       bin = #{ b in [1, n_bins - 1] : s <= fl(T_b * p) }
   a function of the state and the table alone: a few lines of numpy that read the table through aztot_adf_edges reproduce every count exactly.

   TOTALS.  uint64 counts[bin][column] and the number of samples, accumulated over the samples as the RDF's; exact, independent of the order of
   arrival; cleared by a reset or a set-up only.  Values: p[bin][column] = count / (column total * width in degrees), a probability density per degree
   (it sums to 1 / width; no sin(theta) weighting), 0 where the column total is 0; theta = (b + 0.5) * width.

   NEIGHBOUR CAP.  A central atom's neighbours are held on chip.  The neighbours of an atom of species c are the atoms j != i with 0 < r2 < R^2, R the
   largest radius of any column c is central to, whose species is a ligand of such a column.  A sample counts them first (aztot_adf_neighbours).  If any
   atom has more than AZTOT_ADF_MAX_NEIGHBOURS, the sample fails with AZTOT_ERR_INPUT before any total changes: totals and the sample count stay as they
   were, the message names an atom id (the largest id among those with the largest count) and its count, the handle is not marked failed and steps on.
   aztot_adf_neighbours then returns the counts of the refused sample.

   Timing as aztot_rdf_sample: completes the deferred end of the last aztot_step call, only READS the state, returns with the device idle.
   Out of scope: nuclei groups, angles over the bonded topology, slab ranks, dihedrals, sin(theta) weighting.
   Errors: sampling or reading before the set-up, aztot_adf_neighbours before a sample, a cap too small for a non-null buffer -> AZTOT_ERR_ARG; a handle
   that failed earlier refuses to sample but can still be read. */
#define AZTOT_ADF_MAX_BINS 3600
#define AZTOT_ADF_MAX_COLUMNS 64
#define AZTOT_ADF_MAX_NEIGHBOURS 256
typedef struct aztot_adf_column
{
    int32_t central, ligand_a, ligand_b, reserved;     /* species indices; reserved must be 0 */
    double radius_a, radius_b;
} aztot_adf_column;                                    /* 32 bytes */
/* (re)allocates and zeroes; returns n_bins */
int aztot_adf_setup(aztot_md *md, int n_bins, const aztot_adf_column *cols, int n_cols);
/* adds the triplets of the current configuration to the totals */
int aztot_adf_sample(aztot_md *md);
/* zero totals and sample count */
int aztot_adf_reset(aztot_md *md);
int aztot_adf_shape(aztot_md *md, int *n_bins, int *n_cols, int64_t *samples);
/* the n_bins + 1 edge values T_b; returns n_bins + 1 (T null and cap 0: the size alone) */
int aztot_adf_edges(aztot_md *md, double *T, int cap);
/* totals counts[bin * n_cols + column]; returns n_bins * n_cols (samples and counts are each optional) */
int aztot_adf_counts(aztot_md *md, int64_t *samples, uint64_t *counts, int cap);
/* bin centres in degrees (n_bins of them) and p[bin * n_cols + column]; returns n_bins * n_cols (theta and p are each optional; cap counts p's entries) */
int aztot_adf_values(aztot_md *md, double *theta, double *p, int cap);
/* neighbours of each atom (by id) at the last sample, -1: not a central atom; returns n_atoms */
int aztot_adf_neighbours(aztot_md *md, int32_t *n, int cap);

/* ---- static structure factors: per-species amplitudes over a set of k-vectors chosen by |k|, partial S_ab(k) summed over the samples ------------------
   The reference computes no structure factor: like the pressure tensor and the bond-angle distributions, this sampler is ours.
   One GPU only: a slab handle (nranks > 1, loopback included) is refused with AZTOT_ERR_INPUT.

   VECTORS.  k = (l g_x, m g_y, n g_z) with integers l, m, n and g_a = 2 pi / L_a, 2 pi being the correctly rounded double of 2 pi
   (6.283185307179586), not the model's truncated 3.14159265359: the phase has to be periodic in the box.  Only the half space, each pair +-k once:
   l > 0, or l == 0 and m > 0, or l == m == 0 and n > 0.  For every vector kk = ((l g_x)*(l g_x) + (m g_y)*(m g_y)) + (n g_z)*(n g_z) in double, each
   operation rounded on its own ((l g_x) is the rounded product of the integer and g_x).  A vector belongs to the set iff kk <= kmax*kmax and
   bin = (int)(sqrt(kk) * (1.0 / dk)) < n_bins, n_bins = (int)(kmax * (1.0 / dk)): the RDF's rule transposed.  Every step is a correctly rounded
   operation: numpy reproduces the set exactly (tests/sk_model.py).

   ORDER AND THINNING.  The vectors are in ascending lexicographic order of (l, m, n).  With max_per_bin = M > 0, a bin that holds c > M vectors,
   numbered j = 0 ... c - 1 in that order, keeps j iff (j + 1) * M / c > j * M / c in 64-bit integer division: exactly M of them.  Bins with c <= M, and
   every bin when M == 0, keep everything.  The kept vectors, still in lexicographic order, are the set; n_k is its size.

   The set-up rejects with AZTOT_ERR_ARG: a null handle, kmax <= 0, dk <= 0, n_bins outside [1, AZTOT_SK_MAX_BINS], M < 0, an empty set, and a kmax
   that needs a harmonic above AZTOT_SK_MAX_HARMONIC on any axis, i.e. (49 g_a)*(49 g_a) <= kmax*kmax (the message names the axis and the bound on kmax
   this box admits; nothing is truncated silently).  48 is the range over which the harmonic recurrence is held to its tolerance
   (tests/test_gpu_ewald.py) and what the on-chip tables are sized for.  A refused set-up leaves the earlier one.

   A SAMPLE reads the state aztot_md_to_host would return: wrapped positions and species, by atom id.  For species s and vector k the amplitude is
   rho_s(k) = sum_{j of species s} exp(i k r_j) as (re, im), the phase being 2 pi (l x / L_x + m y / L_y + n z / L_z) with the true pi.  Per atom and
   axis exp(2 pi i x / L_a) is evaluated once; higher harmonics come by complex multiplication, negative m or n by conjugation.  Against the exact
   sum, |rho_s - exact| <= 1e-13 n_s per component (tests/test_gpu_sk.py, 50 digits).

   ORDER OF THE SUM.  No floating-point atomics anywhere.  The ids are cut into tiles of 64 consecutive ids; there are nB = min(256, ceil(N / 64)) rows.
   Row r adds the atoms of tiles r, r + nB, r + 2 nB, ... in that order, ascending id inside a tile, one atom at a time from +0.0; atoms of other
   species add nothing.  The nB row sums are zero-padded to 256 and folded by halving (a[j] = a[j] + a[j + h] for h = 128 ... 1).  The order is a function
   of N alone: it does not depend on the slot order the cell sort left, on the launch shape, on how many atoms an on-chip tile holds or on how the
   vectors are batched.  Two handles holding the same state return the same bits.

   ACCUMULATION.  Species pair (a, b), a <= b, has the RDF's pair index mn * (n_species - 1) + mn * (1 - mn) / 2 + mx.  Each sample adds, once, in
   sample order, acc[k][pair] = acc[k][pair] + t with t = (re_a*re_b) + (im_a*im_b) = Re rho_a rho_b*, each operation rounded on its own; the sample
   count goes up by one.  A reset or a set-up clears the accumulators; nothing else does.

   VALUES, Ashcroft-Langreth.  Per vector S_ab(k) = acc / (samples * sqrt(n_a n_b)), 0 where n_a n_b == 0 or before the first sample.  Per bin: the
   plain mean over the bin's kept vectors, summed in set order.  The total per vector is S(k) = sum_{a <= b} w_ab sqrt(n_a n_b) S_ab(k) / N with
   w_aa = 1, w_ab = 2 for a < b (summed in pair order), binned the same way.  The bin centre is k = (b + 0.5) dk.  n_in_bin is the number of kept
   vectors of each bin; the per-bin mean is defined as 0 where it is 0, and callers mask such rows by it.

   Timing as aztot_rdf_sample: completes the deferred end of the last aztot_step call, only READS the state, returns with the device idle.  A run that
   samples is bit-identical in state and statistics to one that calls aztot_get_stats at the same points.
   Out of scope: slab ranks, nuclei groups, charge-charge or scattering-length-weighted combinations (a caller forms them from the partials), the
   imaginary part of the cross terms, the intermediate scattering function F(k, t) (a caller can build it from aztot_sk_amplitudes), vectors past 48
   harmonics, a matrix-core (MFMA) formulation.
   Errors: sampling or reading before the set-up, aztot_sk_amplitudes before a sample, a cap too small for a non-null buffer -> AZTOT_ERR_ARG; a handle
   that failed earlier refuses to sample but can still be read. */
#define AZTOT_SK_MAX_HARMONIC 48
#define AZTOT_SK_MAX_BINS 4096
/* (re)allocates and zeroes; returns n_k */
int aztot_sk_setup(aztot_md *md, double kmax, double dk, int max_per_bin);
/* the amplitudes of the current configuration; adds Re rho_a rho_b* to the sums */
int aztot_sk_sample(aztot_md *md);
/* zero sums and sample count */
int aztot_sk_reset(aztot_md *md);
int aztot_sk_shape(aztot_md *md, int *n_vectors, int *n_bins, int *n_pairs, int64_t *samples);
/* lmn[3 * vector + axis] and bin[vector]; returns n_k (both optional; cap counts vectors) */
int aztot_sk_vectors(aztot_md *md, int32_t *lmn, int32_t *bin, int cap);
/* rho[(vector * n_species + species) * 2 + (0 re, 1 im)] of the last sample; returns n_k * n_species * 2 (rho null and cap 0: the size alone) */
int aztot_sk_amplitudes(aztot_md *md, double *rho, int cap);
/* acc[vector * n_pairs + pair]; returns n_k * n_pairs (samples and acc are each optional) */
int aztot_sk_sums(aztot_md *md, int64_t *samples, double *acc, int cap);
/* bin centres, kept vectors per bin and the total (n_bins of each), s_pair[bin * n_pairs + pair]; returns n_bins * n_pairs (every output optional; cap counts
   s_pair's entries) */
int aztot_sk_values(aztot_md *md, double *k, int32_t *n_in_bin, double *s_total, double *s_pair, int cap);

/* ---- bond-orientational order: Steinhardt q_l per atom and the neighbour-averaged q-bar_l of Lechner and Dellago ---------------------------------------
   The reference has no such output: like the pressure tensor and the bond-angle distributions, this sampler is ours.
   One GPU only: a slab handle (nranks > 1, loopback included) is refused with AZTOT_ERR_INPUT.

   SET-UP.  radius R; central_mask and ligand_mask, bit s for species s; n_orders in [1, AZTOT_BOO_MAX_ORDERS] distinct orders l in [1, AZTOT_BOO_MAX_L];
   n_bins in [1, AZTOT_BOO_MAX_BINS]; reserved = 0.  Returns n_bins.  Rejected with AZTOT_ERR_ARG: a null handle or params, R <= 0 (or not finite), an
   empty mask, a mask bit at or above n_species, an order out of range or repeated, n_orders or n_bins out of range, a non-zero `reserved`.  A refused
   set-up leaves the earlier one in place.  A species without atoms is fine.

   BONDS.  Atom i is central iff its species is in central_mask.  Its neighbours N(i) are the atoms j != i whose species is in ligand_mask and whose
   separation satisfies 0 < r2 < R * R, strict on both sides.  The separation is that of aztot_cn_sample and aztot_adf_sample on the positions
   aztot_md_to_host returns: u = r_j - r_i per axis, one shift by L where |d| > L / 2, r2 = (ux*ux + uy*uy) + uz*uz in fp64 with every operation rounded
   on its own.  R may exceed L / 2: each partner is seen once, through its nearest image.  n_i = |N(i)|; there is no neighbour cap (nothing per
   neighbour is held on chip).

   VALUES.  Bond direction (x, y, z) = u * (1 / sqrt(r2)).  For m = 0 ... l
       q_lm(i) = (1 / n_i) sum_{j in N(i)} Y_lm(direction of the bond i -> j)
   with the orthonormal complex spherical harmonics and the Condon-Shortley phase; m < 0 follows by symmetry and is neither stored nor summed.
       q_l(i) = sqrt( 4 pi / (2l + 1) * ( |q_l0|^2 + 2 sum_{m > 0} |q_lm|^2 ) )
   Averaged form, C(i) the central atoms among N(i):
       qbar_lm(i) = ( q_lm(i) + sum_{k in C(i)} q_lm(k) ) / (1 + |C(i)|),      qbar_l(i) from qbar_lm(i) by the same expression.
   n_i = 0: q_lm = 0 and q_l = qbar_l = 0; a central neighbour with n_k = 0 enters with zeros and is counted in |C(i)|.  An atom that is not central
   has n = -1 and all values 0.

   ROUTE.  No sin, cos, acos or atan2: (x + i y)^m by complex multiplication, T_l^m(z) = P_l^m(z) / sin^m(theta) by the three-term recurrence in l from
   T_m^m = (-1)^m (2m - 1)!!, the normalisation sqrt((2l + 1) / (4 pi) (l - m)! / (l + m)!) from a host table made in extended precision and applied
   once per atom to the sums.  Nothing divides by sin(theta): a bond along +-z is an ordinary bond.  One correctly rounded sqrt and one division per
   bond.  No floating-point atomics.  The harmonic arithmetic may contract to fused multiply-adds: q_lm is held to a stated tolerance, not to the bit
   (tests/boo_model.py: QLM_TOL per component, four times the measured worst error of the same route in plain fp64).

   ORDER OF THE SUMS.  A sample's per-atom values are a function of the sampled state alone (wrapped positions, ids, types, N, box, set-up): neighbour
   cells in a fixed order, ids ascending inside a cell, dealt to a number of lanes that depends on N only, folded by lane exchange in a fixed order.  Two
   handles that hold the same state return the same bits, whatever slot order their engines' sorts left.

   TOTALS over the samples.  Only central atoms with n_i > 0 enter.  uint64 hist[kind][order][species][bin], kind 0 = q, 1 = qbar, with
   bin = min(n_bins - 1, (int) fl(q * n_bins)); fp64 sum[kind][order][species]: the summation tree of aztot_tcf_sample (runs of 64 ids, the four runs of
   256, the chunks padded to a power of two and halved) over the per-atom values in id order, the term of an atom of another species +0.0, added to
   the running sum once per sample in sample order; uint64 entered[species]; the number of samples.  A reset or a set-up clears them; nothing else does.
   Values: centre (b + 0.5) / n_bins; density per unit q = count / (column total * width), width = 1 / n_bins, 0 where the column total is 0 (a
   column is one (kind, order, species)); mean = sum / entered, 0 where entered is 0.

   Timing as aztot_rdf_sample: completes the deferred end of the last aztot_step call, only READS the state, returns with the device idle.
   Out of scope: the w_l invariants (a caller forms them from aztot_boo_qlm), k-nearest or Voronoi neighbourhoods, solid-like bond counts (ten Wolde),
   nuclei groups, slab ranks, several set-ups side by side.
   Errors: sampling or reading before the set-up, aztot_boo_per_atom / aztot_boo_qlm before a sample, a cap too small for a non-null buffer ->
   AZTOT_ERR_ARG; a handle that failed earlier refuses to sample but can still be read. */
#define AZTOT_BOO_MAX_ORDERS 4
#define AZTOT_BOO_MAX_L 12
#define AZTOT_BOO_MAX_BINS 4096
typedef struct aztot_boo_params
{
    double radius;
    int32_t central_mask, ligand_mask;                 /* bit s: species s */
    int32_t n_orders, orders[AZTOT_BOO_MAX_ORDERS];
    int32_t n_bins, reserved;                          /* reserved must be 0 */
} aztot_boo_params;                                    /* 48 bytes */
/* (re)allocates and zeroes; returns n_bins */
int aztot_boo_setup(aztot_md *md, const aztot_boo_params *params);
/* the per-atom values of the current configuration; adds them to the totals */
int aztot_boo_sample(aztot_md *md);
/* zero totals and sample count */
int aztot_boo_reset(aztot_md *md);
/* orders: room for AZTOT_BOO_MAX_ORDERS entries (each output optional) */
int aztot_boo_shape(aztot_md *md, int *n_orders, int32_t *orders, int *n_bins, int *n_species, int64_t *samples);
/* last sample by atom id: n[atom] (-1: not central), q[(atom * n_orders + order) * 2 + kind]; returns n_atoms (both null and cap 0: the size alone;
   cap counts atoms) */
int aztot_boo_per_atom(aztot_md *md, int32_t *n, double *q, int cap);
/* q_lm of the last sample, qlm[((atom * n_orders + order) * 13 + m) * 2 + (0 re, 1 im)], zeros past m = l; returns n_atoms * n_orders * 26 */
int aztot_boo_qlm(aztot_md *md, double *qlm, int cap);
/* hist[((kind * n_orders + order) * n_species + species) * n_bins + bin], sums[(kind * n_orders + order) * n_species + species], entered[species];
   returns the size of hist (every output optional; cap counts hist's entries, sums and entered need room for their full size) */
int aztot_boo_counts(aztot_md *md, int64_t *samples, uint64_t *hist, double *sums, uint64_t *entered, int cap);
/* bin centres (n_bins), density in hist's layout, mean in sums' layout; returns the size of density (each optional; cap counts density's entries) */
int aztot_boo_values(aztot_md *md, double *centre, double *density, double *mean, int cap);

/* ---- smooth particle-mesh Ewald: debug read-back ------------------------------------------------------ */
/* 'elec spme' (AZTOT_ELEC_SPME) replaces the k-vector loop of 'elec pme' by a mesh; real-space and constant parts, and the statistics they are booked in
   (engCoul, engCoulConst; the mesh part in engCoulRec), are those of 'elec pme'.  Orthorhombic box, mesh K = (Kx, Ky, Kz), spline order p:
     u = K x / L per axis, f = floor(u), w = u - f; theta(j) = M_p(w + j), j = 0 .. p - 1 (M_p: cardinal B-spline) lands on mesh index (f - j) mod K
     Q(g) = 2^-40 * sum over atoms of llrint(((q theta_x) theta_y) theta_z * 2^40): 64-bit integer sums, independent of the order of the atoms
     G(m) = exp(-k^2 / 4 alpha^2) / k^2 * b_x b_y b_z, k = 2 pi m' / L (m' the signed index, pi the model's), b(m) = 1 / |sum_{k=0}^{p-2} M_p(k + 1) e^{2 pi i m k / K}|^2, G(0) = 0
     engCoulRec = 1/2 scale sum_m G |FQ|^2 (FQ the forward DFT of Q; scale: aztot_model_query "spme"), phi = scale * unnormalised inverse DFT of G FQ (real part)
     F_i,a = -q_i (K_a / L_a) sum_g phi(g) theta'_a theta_b theta_c over the atom's p^3 points; the net force is NOT removed
   One GPU only: a slab handle (nranks > 1, loopback included) with such a model is refused with AZTOT_ERR_INPUT, and so is a model with
   n_atoms * max|q| >= 2^22 (the integer sums could overflow).  aztot_stress_setup refuses it as it refuses 'elec pme'.
   aztot_spme_mesh: a mesh of the last force evaluation (aztot_forces, or the last step), re-evaluated stage by stage from the positions the handle holds:
     which = AZTOT_SPME_CHARGE    the integer charge mesh, int64_t[Kx Ky Kz], in units of 2^-40 e
     which = AZTOT_SPME_SPECTRUM  its forward DFT, (re, im) pairs of doubles
     which = AZTOT_SPME_POTENTIAL phi, (re, im) pairs of doubles (the forces use the real part)
   Point (gx, gy, gz) is entry (gz * Ky + gy) * Kx + gx.  `cap` and the result count 8-byte words; out null and cap 0: the size alone; a shorter
   buffer, an unknown `which` or a handle without an SPME model -> AZTOT_ERR_ARG. */
enum { AZTOT_SPME_CHARGE = 0, AZTOT_SPME_SPECTRUM = 1, AZTOT_SPME_POTENTIAL = 2 };
int64_t aztot_spme_mesh(aztot_md *md, int which, void *out, int64_t cap);
/* the influence function G in the same layout, Kx Ky Kz doubles (built once on the host in long double, rounded to double); returns their number */
int64_t aztot_spme_influence(aztot_md *md, double *out, int64_t cap);

/* ---- measurement ------------------------------------------------------------------------------------ */
/* per-kernel HIP-event times accumulated since the last reset (options.profile = 1).
   names: NUL-separated list written into `names` (cap bytes); ms / calls: arrays of length >= returned count */
int aztot_kernel_times(aztot_md *md, char *names, int cap, double *ms, int64_t *calls, int max_kernels);
int aztot_reset_kernel_times(aztot_md *md);
/* switch per-kernel HIP-event timing on/off at run time (off: the step may be replayed as a hipGraph) */
int aztot_set_profile(aztot_md *md, int on);

/* ---- multi-GPU slab decomposition (one process per GPU) ---------------------------------------------- */
/* size of the opaque RCCL unique id; rank 0 creates it, the launcher broadcasts it (e.g. torch.distributed) */
int aztot_comm_id_bytes(void);
int aztot_comm_make_id(void *id_bytes);
/* diagnostic: brings up a ONE-rank RCCL communicator on `device` and runs the slab ring exchange with itself (both messages in
   the N-GPU call order) plus both all-reduce flavours; AZTOT_OK if RCCL is usable on this node and delivers what was sent */
int aztot_comm_selftest(int device);
/* number of ranks in the RCCL communicator that carries this handle's halo exchange (ncclCommCount); 0 when the handle does not
   use RCCL (single GPU, host-staged callbacks, loopback).  Lets a launcher prove which transport a run really used. */
int aztot_comm_ranks(aztot_md *md);
/* host-staged exchange callback for tests without RCCL (gloo): send `sbytes` to `peer`, receive into rbuf */
typedef int (*aztot_sendrecv_fn)(void *ctx, int send_peer, const void *sbuf, int64_t sbytes,
                                 int recv_peer, void *rbuf, int64_t rcap, int64_t *rbytes);
typedef int (*aztot_allreduce_fn)(void *ctx, double *buf, int n);
/* as aztot_init_device, but this rank owns slab `rank` of `nranks` along x; exactly one of id_bytes / callbacks is used */
int aztot_init_device_slab(const aztot_model *m, const aztot_options *opt, int rank, int nranks,
                           const void *rccl_id_bytes, aztot_sendrecv_fn sendrecv, aztot_allreduce_fn allreduce, void *ctx,
                           aztot_md **out);

const char *aztot_last_error(void);
const char *aztot_version(void);

#ifdef __cplusplus
}
#endif
#endif /* AZTOT_H */
