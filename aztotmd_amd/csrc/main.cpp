// aztotmd - command-line driver with the reference program's surface (main.cu:239-463): reads atoms.xyz, field.txt,
// control.txt, cuda.txt from a directory (default: the cwd, as the reference), runs `nstep` steps of the hot path on
// the GPU and writes the reference's result files for this path:
//   stat.dat        header + one row every `stat` steps          (start_stat / copy_stat, cuStat.cu:300-330, 40-71)
//   revcon.xyz      final configuration in atoms.xyz format     (out_atoms, out_md.cpp:65-87; main.cu:436)
//   velocities.dat  per-species |v|, vx, vy, vz table            (out_velocities, out_md.cpp:126-190; main.cu:445)
//   tchars.dat      thermal energies and radii (radiative thermostat only)  (out_thermalchar, main.cu:51-118)
//   rdf.dat         radial distribution functions, when control.txt has 'rdf rmax dr every out_every [nucl]' (rdf_iter / copy_rdf, cuStat.cu:514-600)
//   rdf_n.dat       the same per nucleus pair, with 'nucl' (nrdf_iter / copy_nrdf, cuStat.cu:703-790)
//   rdf<k>.dat      running RDFs at the samples with (c - 1) % out_every == 0, k = c - 1 (and rdf_n<k>.dat)
//   CN.dat          coordination numbers of species at the end of the run, with 'outCN R nCentral names.. nLigand names..' (out_cn, out_md.cpp:389-504; main.cu:446)
//   nCN.dat         the same per nucleus pair, with 'ncn n' + n lines 'nucleus1 nucleus2 R'          (out_ncn, out_md.cpp:196-387; main.cu:448)
//   displ.dat       with 'vaf n' too: mean-square displacement per species from the time origin, one row per stat row: the '<name>-msd' columns of the serial program's msd.dat
//                   (msd_header / out_msd, out_md.cpp:19-29,89-124; main.cpp:163).  msd.dat itself follows the GPU program (wall-crossing counters)
//   vaf.dat         velocity autocorrelation per species, with 'vaf n': a row every n steps after the equilibration (vaf_header / vaf_info, out_md.cpp:547-582;
//                   main.cpp:71-75,115-117)
//   stress.dat      OUR EXTENSION, with 'stress n' (a control.txt directive the reference does not know): the pressure tensor of aztot_stress_* in atm, a row at every
//                   step c > 0 with c % n == 0: Pxx Pyy Pzz Pxy Pxz Pyz and P = (Pxx + Pyy + Pzz) / 3.  Without the line: no sampler, no file
//   adf.dat         OUR EXTENSION, with an 'adf <n_bins> <every> <n>' block (n lines '<central> <ligand1> <ligand2> <R1> <R2>', species names): the bond-angle
//                   distributions of aztot_adf_*, header "theta" + "\t<ligand1>-<central>-<ligand2>" per column, a row per bin: the bin centre in degrees and the
//                   probability density per degree of each column.  Sampled after every completed step c > nequil with c % every == 0; with every == 0, or when
//                   the run ended before the first sample, once on the final configuration.  Without the block: no sampler, no file
//   adf_n.dat       the same layout with the raw counts
//   sk.dat          OUR EXTENSION, with 'strfac <kmax> <dk> <every> <max_per_bin>': the static structure factors of aztot_sk_*, header "k\tn\tS" + "\t<nameA>-<nameB>"
//                   per species pair in pair-index order, a row per bin that holds at least one k-vector: the bin centre in 1/A, the number of k-vectors averaged,
//                   the total S(k) and the Ashcroft-Langreth partials.  The schedule of adf.dat: sampled after every completed step c > nequil with
//                   c % every == 0; with every == 0, or when the run ended before the first sample, once on the final configuration.  A kmax the box cannot
//                   serve (past 48 harmonics on an axis, or no vector at all) gives a WARNING and no file.  Without the line: no sampler, no file
//   boo.dat         OUR EXTENSION, with 'boo <R> <n_bins> <every> <n_orders> <l...> <nCentral> <names...> <nLigand> <names...>': the bond-orientational order
//                   parameters of aztot_boo_*, header "q" + "\tq<l>_<species>\tqbar<l>_<species>" per order and central species, a row per bin: the bin centre
//                   and the density per unit q of each column; then a comment line per column, "# <column> mean <mean> entered <atoms>".  The schedule of
//                   adf.dat.  Without the line: no sampler, no file
//   boo_n.dat       the same layout with the raw counts
// Both displ.dat and vaf.dat are switched on by the 'vaf n' line (n > 0): a control.txt without it runs and writes exactly what it did before the sampler existed.
// MSD / VAF schedule: ONE sampler (aztot_tcf_*) with a single origin, n_origins = 1 and origin_every = the number of samples the run takes.  Sample 0 is the
// initial state (x0s, sys_init.cpp:545); a step c < nequil that writes a stat row samples and writes a displ.dat row; at c == nequil (> 0) the sampler is
// reset and the state becomes the new origin (main.cpp:126-136; a stat row of that step follows and shows 0, as in the reference, which replaces x0s
// before out_msd runs); at c > nequil a sample is taken when c writes a stat row (displ.dat) or c % vaf == 0 (vaf.dat), one sample serving both.
// Deviations from the serial program: the time column is aztot_stats.time = c * dt (the serial vaf_info prints the time of the step before, because
// calc_chars advances it afterwards, main.cpp:117,142); with 'nequil 0' the VAF origin is the initial state (the reference never calls vaf_init then and
// reads unset memory); an empty species prints 0 (the reference's MSD prints 0 / 0).
// RDF schedule: the reference counts iStep from 0 and samples at the end of the loop body (main.cu:392-395), i.e. after completed step c whenever
// (c - 1) % every == 0: after steps 1, 1 + every, ...  Call boundaries: aztot_step is called with n = the distance to the next event, an event being a
// stat row (c % stat == 0, and the last step), an RDF sample (which only reads the state: its place against the stat row of the same step does not matter),
// the end of the equilibration, a vaf.dat row, a stress.dat row, a sample of the bond-angle distributions, one of the structure factors or one of the
// bond-orientational order.
// Unlike the reference, atoms are written in their ORIGINAL order (the reference writes them cell-sorted, SURVEY C-20).
// Everything goes through the C ABI of include/aztot.h.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <string>
#include <vector>

#include "../../include/aztot.h"

static void die(const char* what)
{
    std::fprintf(stderr, "FATAL ERROR: %s: %s\n", what, aztot_last_error());
    std::exit(1);
}

// copy_rdf / copy_nrdf layout: header "r\tA-A\tA-B...", rows "%f" r then "\t%f" per pair
static void write_rdf(aztot_md* md, int kind, const std::vector<std::string>& names, const std::string& path)
{
    const int need = aztot_rdf_values(md, kind, nullptr, nullptr, 0);
    if (need < 0) die("rdf values");
    int nb = 0, np = 0;
    if (aztot_rdf_shape(md, kind, &nb, &np) != AZTOT_OK) die("rdf shape");
    std::vector<double> r(std::max(nb, 1)), g(std::max(need, 1));
    if (aztot_rdf_values(md, kind, r.data(), g.data(), need) < 0) die("rdf values");
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) { std::perror(path.c_str()); std::exit(1); }
    std::fprintf(f, "r");
    for (size_t a = 0; a < names.size(); a++)
        for (size_t b = a; b < names.size(); b++) std::fprintf(f, "\t%s-%s", names[a].c_str(), names[b].c_str());
    std::fprintf(f, "\n");
    for (int i = 0; i < nb; i++)
    {
        std::fprintf(f, "%f", r[i]);
        for (int p = 0; p < np; p++) std::fprintf(f, "\t%f", g[(size_t)i * np + p]);
        std::fprintf(f, "\n");
    }
    std::fclose(f);
}

// out_cn / out_ncn layout: header "CN\t<central>-<ligand>...", rows "%d" CN then "\t%d" per column; false (and a warning) when the columns cannot be used
static bool write_cn(aztot_md* md, int kind, const std::vector<aztot_cn_column>& cols, const std::vector<std::string>& names, const std::string& path)
{
    if (aztot_cn_setup(md, kind, cols.data(), (int)cols.size()) != AZTOT_OK)
    {
        std::fprintf(stderr, "WARNING: %s directive not usable (%s): no %s\n", kind == AZTOT_CN_SPECIES ? "outCN" : "ncn", aztot_last_error(), path.c_str());
        return false;
    }
    if (aztot_cn_sample(md, kind) != AZTOT_OK) die("cn sample");
    int nc = 0, mn = 0, mx = 0;
    if (aztot_cn_shape(md, kind, &nc, &mn, &mx) != AZTOT_OK) die("cn shape");
    const int need = aztot_cn_table(md, kind, nullptr, 0);
    if (need < 0) die("cn table");
    std::vector<int64_t> t(std::max(need, 1));
    if (aztot_cn_table(md, kind, t.data(), need) < 0) die("cn table");
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) { std::perror(path.c_str()); std::exit(1); }
    std::fprintf(f, "CN");
    for (const auto& c : cols) std::fprintf(f, "\t%s-%s", names[c.central].c_str(), names[c.ligand].c_str());
    std::fprintf(f, "\n");
    for (int r = mn; r <= mx; r++)
    {
        std::fprintf(f, "%d", r);
        for (int c = 0; c < nc; c++) std::fprintf(f, "\t%lld", (long long)t[(size_t)(r - mn) * nc + c]);
        std::fprintf(f, "\n");
    }
    std::fclose(f);
    return true;
}

// adf.dat: header "theta\t<ligand1>-<central>-<ligand2>...", rows "%f" theta then "\t%f" per column; adf_n.dat: the same with the raw counts as "%llu"
static void write_adf(aztot_md* md, const std::vector<aztot_adf_column>& cols, const std::vector<std::string>& names, const std::string& path, const std::string& pathN)
{
    int nb = 0, nc = 0;
    if (aztot_adf_shape(md, &nb, &nc, nullptr) != AZTOT_OK) die("adf shape");
    std::vector<double> theta(std::max(nb, 1)), p((size_t)std::max(nb * nc, 1));
    std::vector<uint64_t> cnt(p.size());
    if (aztot_adf_values(md, theta.data(), p.data(), nb * nc) < 0) die("adf values");
    if (aztot_adf_counts(md, nullptr, cnt.data(), nb * nc) < 0) die("adf counts");
    for (int raw = 0; raw < 2; raw++)
    {
        const std::string& file = raw ? pathN : path;
        FILE* f = std::fopen(file.c_str(), "w");
        if (!f) { std::perror(file.c_str()); std::exit(1); }
        std::fprintf(f, "theta");
        for (const auto& c : cols) std::fprintf(f, "\t%s-%s-%s", names[c.ligand_a].c_str(), names[c.central].c_str(), names[c.ligand_b].c_str());
        std::fprintf(f, "\n");
        for (int b = 0; b < nb; b++)
        {
            std::fprintf(f, "%f", theta[b]);
            for (int k = 0; k < nc; k++)
                if (raw) std::fprintf(f, "\t%llu", (unsigned long long)cnt[(size_t)b * nc + k]);
                else std::fprintf(f, "\t%f", p[(size_t)b * nc + k]);
            std::fprintf(f, "\n");
        }
        std::fclose(f);
    }
}

// sk.dat: header "k\tn\tS\t<nameA>-<nameB>...", rows "%f" k, "\t%d" vectors in the bin, "\t%f" S and "\t%f" per pair; bins without a vector have no row
static void write_sk(aztot_md* md, const std::vector<std::string>& names, const std::string& path)
{
    int nb = 0, np = 0;
    if (aztot_sk_shape(md, nullptr, &nb, &np, nullptr) != AZTOT_OK) die("sk shape");
    std::vector<double> k(std::max(nb, 1)), tot(std::max(nb, 1)), part((size_t)std::max(nb * np, 1));
    std::vector<int32_t> cnt(std::max(nb, 1));
    if (aztot_sk_values(md, k.data(), cnt.data(), tot.data(), part.data(), nb * np) < 0) die("sk values");
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) { std::perror(path.c_str()); std::exit(1); }
    std::fprintf(f, "k\tn\tS");
    for (size_t a = 0; a < names.size(); a++)
        for (size_t b = a; b < names.size(); b++) std::fprintf(f, "\t%s-%s", names[a].c_str(), names[b].c_str());
    std::fprintf(f, "\n");
    for (int b = 0; b < nb; b++)
    {
        if (cnt[b] == 0) continue;
        std::fprintf(f, "%f\t%d\t%f", k[b], (int)cnt[b], tot[b]);
        for (int p = 0; p < np; p++) std::fprintf(f, "\t%f", part[(size_t)b * np + p]);
        std::fprintf(f, "\n");
    }
    std::fclose(f);
}

// boo.dat: header "q\tq<l>_<species>\tqbar<l>_<species>...", rows "%f" centre then "\t%f" per column, then "# <column> mean %f entered %llu" per column;
// boo_n.dat: the same with the raw counts as "%llu"
static void write_boo(aztot_md* md, int centralMask, const std::vector<std::string>& names, const std::string& path, const std::string& pathN)
{
    int no = 0, nb = 0, ns = 0;
    int32_t orders[AZTOT_BOO_MAX_ORDERS];
    if (aztot_boo_shape(md, &no, orders, &nb, &ns, nullptr) != AZTOT_OK) die("boo shape");
    const int nh = 2 * no * ns * nb;
    std::vector<double> centre(std::max(nb, 1)), dens((size_t)std::max(nh, 1)), mean((size_t)std::max(2 * no * ns, 1));
    std::vector<uint64_t> cnt(dens.size()), entered((size_t)std::max(ns, 1));
    if (aztot_boo_values(md, centre.data(), dens.data(), mean.data(), nh) < 0) die("boo values");
    if (aztot_boo_counts(md, nullptr, cnt.data(), nullptr, entered.data(), nh) < 0) die("boo counts");
    struct Col { std::string name; int at, species; };       // at: (kind * n_orders + order) * n_species + species
    std::vector<Col> cols;
    for (int o = 0; o < no; o++)
        for (int s = 0; s < ns; s++)
        {
            if (!((centralMask >> s) & 1)) continue;
            for (int kind = 0; kind < 2; kind++)
                cols.push_back({std::string(kind ? "qbar" : "q") + std::to_string(orders[o]) + "_" + names[s], (kind * no + o) * ns + s, s});
        }
    for (int raw = 0; raw < 2; raw++)
    {
        const std::string& file = raw ? pathN : path;
        FILE* f = std::fopen(file.c_str(), "w");
        if (!f) { std::perror(file.c_str()); std::exit(1); }
        std::fprintf(f, "q");
        for (const auto& c : cols) std::fprintf(f, "\t%s", c.name.c_str());
        std::fprintf(f, "\n");
        for (int b = 0; b < nb; b++)
        {
            std::fprintf(f, "%f", centre[b]);
            for (const auto& c : cols)
                if (raw) std::fprintf(f, "\t%llu", (unsigned long long)cnt[(size_t)c.at * nb + b]);
                else std::fprintf(f, "\t%f", dens[(size_t)c.at * nb + b]);
            std::fprintf(f, "\n");
        }
        for (const auto& c : cols) std::fprintf(f, "# %s mean %f entered %llu\n", c.name.c_str(), mean[c.at], (unsigned long long)entered[c.species]);
        std::fclose(f);
    }
}

// "<time>\t<step>" + "\t%f" per species: the row layout of out_msd's MSD columns and of vaf_info
static void write_tcf_row(FILE* f, double time, int step, const std::vector<double>& v)
{
    std::fprintf(f, "%f\t%d", time, step);
    for (double e : v) std::fprintf(f, "\t%f", e);
    std::fprintf(f, "\n");
}

static double q1(const aztot_model* m, const char* key)
{
    double v = 0.0;
    if (aztot_model_query(m, key, &v, 1) < 1) die(key);
    return v;
}

int main(int argc, char** argv)
{
    std::string dir = ".", out = ".";
    int device = 0, nstep_override = -1;
    for (int i = 1; i < argc; i++)
    {
        std::string a = argv[i];
        if (a == "--out" && i + 1 < argc) out = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (a == "--nstep" && i + 1 < argc) nstep_override = std::atoi(argv[++i]);
        else if (a == "-h" || a == "--help") { std::printf("usage: aztotmd [input-dir] [--out dir] [--device n] [--nstep n]\n"); return 0; }
        else dir = a;
    }
    std::printf("azTotMD hot path on MI355X (%s)\n", aztot_version());
    const std::time_t t0 = std::time(nullptr);
    aztot_model* model = nullptr;
    if (aztot_init_md(dir.c_str(), &model) != AZTOT_OK) die("SYSTEM CAN'T BE INITIALIZED");
    const int N = (int)q1(model, "n_atoms"), nSpec = (int)q1(model, "n_species");
    const int nStep = nstep_override >= 0 ? nstep_override : (int)q1(model, "nstep");
    const int stat = std::max(1, (int)q1(model, "stat"));
    const bool radi = (int)q1(model, "tstat_type") == AZTOT_TSTAT_RADI;
    double box[3];
    aztot_model_query(model, "box", box, 3);
    std::vector<std::string> names(nSpec);
    for (int i = 0; i < nSpec; i++) { char b[16]; aztot_model_species_name(model, i, b, 16); names[i] = b; }

    aztot_options opt;
    aztot_default_options(&opt);
    opt.device = device;
    opt.initial_forces = 0;                         // the GPU program starts from F = 0 (sys_init.cpp:551-553)
    aztot_md* md = nullptr;
    if (aztot_init_device(model, &opt, &md) != AZTOT_OK) die("DEVICE CAN'T BE INITIALIZED");
    std::printf("MD long %d timesteps of %f ps, %d atoms\n", nStep, q1(model, "dt"), N);

    FILE* sf = std::fopen((out + "/stat.dat").c_str(), "w");
    if (!sf) { std::perror("stat.dat"); return 1; }
    // columns follow start_stat (cuStat.cu:300-330): engBnd / engAngle appear when field.txt declares bond / angle types
    double nbd[4] = {0, 0, 0, 0};
    aztot_model_query(model, "n_bonded", nbd, 4);
    const bool hasB = nbd[0] > 0, hasA = nbd[1] > 0;
    std::fprintf(sf, "time\tstep\tengTot\tengKin\tengVdW\tengCoul1\tengCoul2%s%s%s\tmomPx\tmomNx\tmomPy\tmomNy\tmomPz\tmomNz\tpress\n", radi ? "\tengTerm" : "",
                 hasB ? "\tengBnd" : "", hasA ? "\tengAngle" : "");
    std::fprintf(sf, "time, ps\tstep, n\tengTot, eV\tengKin, eV\tengVdW, eV\tengCoul1, eV\tengCoul2, eV%s%s%s"
                     "\tmomPx, eVps/A\tmomNx, eVps/A\tmomPy, eVps/A\tmomNy, eVps/A\tmomPz, eVps/A\tmomNz, eVps/A\tpress, atm\n", radi ? "\tengTerm, eV" : "",
                 hasB ? "\tengBnd, eV" : "", hasA ? "\tengAngle, eV" : "");
    // msd.dat: despite its name the reference writes the per-species wall-crossing counters there (start_stat cuStat.cu:345-350,
    // init_cuda_stat :278-288: specAcBoxPos/Neg x, y, z per species), one row per statistics step
    FILE* mf = std::fopen((out + "/msd.dat").c_str(), "w");
    if (!mf) { std::perror("msd.dat"); return 1; }
    std::fprintf(mf, "time\tstep");
    for (int j = 0; j < nSpec; j++) std::fprintf(mf, "\t%s_px\tnx\tpy\tny\tpz\tnz", names[j].c_str());
    std::fprintf(mf, "\n");
    std::vector<int64_t> crossings(6 * (size_t)nSpec);
    // radial distribution functions (read_rdf: rdf rmax dr every out_every [nucl])
    double rdfp[6] = {0, 0, 0, 0, 0, 0};
    aztot_model_query(model, "rdf", rdfp, 6);
    const int rdfEvery = (int)rdfp[3], rdfOut = (int)rdfp[4];
    const bool nucl = rdfp[5] != 0.0;
    bool rdfOn = rdfp[0] != 0.0 && rdfEvery > 0;
    std::vector<std::string> nnames;
    if (rdfOn)
    {
        if (aztot_rdf_setup(md, rdfp[1], rdfp[2], nucl ? 1 : 0) < 0)
        {
            std::fprintf(stderr, "WARNING: rdf directive not usable (%s): no RDF output\n", aztot_last_error());
            rdfOn = false;
        }
        const int nn = (int)q1(model, "n_nuclei");
        for (int i = 0; i < nn; i++) { char b[16]; aztot_model_nucleus_name(model, i, b, 16); nnames.push_back(b); }
    }
    auto rdf_due = [&](int c) { return rdfOn && c >= 1 && (c - 1) % rdfEvery == 0; };
    // mean-square displacement and velocity autocorrelation: one sampler with a single origin (see the header comment)
    const int nEq = (int)q1(model, "nequil"), vafEvery = (int)q1(model, "vaf");
    auto stat_row = [&](int c) { return c % stat == 0 || c == nStep; };
    auto vaf_row = [&](int c) { return vafEvery > 0 && c > nEq && c % vafEvery == 0; };
    auto tcf_due = [&](int c) { return c == 0 || (nEq > 0 && c == nEq) || stat_row(c) || vaf_row(c); };
    int tcfSamples = 0;
    for (int c = 0; c <= nStep; c++) tcfSamples += tcf_due(c) ? 1 : 0;
    bool tcfOn = vafEvery > 0;
    if (tcfOn && (aztot_tcf_setup(md, 1, tcfSamples) < 0 || aztot_tcf_sample(md) != AZTOT_OK))
    {
        std::fprintf(stderr, "WARNING: no room for the MSD / VAF sampler (%s): no displ.dat, no vaf.dat\n", aztot_last_error());
        tcfOn = false;
    }
    FILE *df = nullptr, *vf = nullptr;
    if (tcfOn)
    {
        df = std::fopen((out + "/displ.dat").c_str(), "w");
        if (!df) { std::perror("displ.dat"); return 1; }
        std::fprintf(df, "Time\tStep");
        for (int j = 0; j < nSpec; j++) std::fprintf(df, "\t%s-msd", names[j].c_str());
        std::fprintf(df, "\n");
        vf = std::fopen((out + "/vaf.dat").c_str(), "w");
        if (!vf) { std::perror("vaf.dat"); return 1; }
        std::fprintf(vf, "time,ps\tiStep");
        for (int j = 0; j < nSpec; j++) std::fprintf(vf, "\t%s", names[j].c_str());
        std::fprintf(vf, "\n");
    }
    std::vector<double> msdRow(std::max(nSpec, 1)), vafRow(std::max(nSpec, 1));
    // pressure tensor ('stress n', our extension): a snapshot every n steps
    const int stressEvery = (int)q1(model, "stress");
    bool stressOn = stressEvery > 0;
    if (stressOn && aztot_stress_setup(md) != AZTOT_OK)
    {
        std::fprintf(stderr, "WARNING: stress directive not usable (%s): no stress.dat\n", aztot_last_error());
        stressOn = false;
    }
    auto stress_due = [&](int c) { return stressOn && c >= 1 && c % stressEvery == 0; };
    FILE* pf = nullptr;
    if (stressOn)
    {
        pf = std::fopen((out + "/stress.dat").c_str(), "w");
        if (!pf) { std::perror("stress.dat"); return 1; }
        std::fprintf(pf, "time\tstep\tPxx\tPyy\tPzz\tPxy\tPxz\tPyz\tP\n");
    }
    // bond-angle distributions ('adf' block, our extension): columns from the model, samples on their own schedule, the files at the end
    std::vector<double> adfq(3);
    {
        const int n = aztot_model_query(model, "adf", nullptr, 0);
        if (n < 3) die("adf");
        adfq.resize(n);
        if (aztot_model_query(model, "adf", adfq.data(), n) < 0) die("adf");
    }
    const int adfEvery = (int)adfq[1];
    bool adfOn = adfq[0] > 0.0;
    std::vector<aztot_adf_column> adfCols;
    for (int i = 0; adfOn && i < (int)adfq[2]; i++)
        adfCols.push_back({(int32_t)adfq[3 + 5 * i], (int32_t)adfq[4 + 5 * i], (int32_t)adfq[5 + 5 * i], 0, adfq[6 + 5 * i], adfq[7 + 5 * i]});
    if (adfOn && aztot_adf_setup(md, (int)adfq[0], adfCols.data(), (int)adfCols.size()) < 0)
    {
        std::fprintf(stderr, "WARNING: adf directive not usable (%s): no adf.dat\n", aztot_last_error());
        adfOn = false;
    }
    auto adf_due = [&](int c) { return adfOn && adfEvery > 0 && c > nEq && c % adfEvery == 0; };
    int adfTaken = 0;
    // static structure factors ('strfac', our extension): the schedule of the bond-angle distributions, the file at the end
    double skq[4] = {0, 0, 0, 0};
    if (aztot_model_query(model, "sk", skq, 4) < 4) die("sk");
    const int skEvery = (int)skq[2];
    bool skOn = skq[0] > 0.0;
    if (skOn && aztot_sk_setup(md, skq[0], skq[1], (int)skq[3]) < 0)
    {
        std::fprintf(stderr, "WARNING: strfac directive not usable (%s): no sk.dat\n", aztot_last_error());
        skOn = false;
    }
    auto sk_due = [&](int c) { return skOn && skEvery > 0 && c > nEq && c % skEvery == 0; };
    int skTaken = 0;
    // bond-orientational order ('boo', our extension): the schedule of the bond-angle distributions, the files at the end
    double booq[6 + AZTOT_BOO_MAX_ORDERS] = {0};
    if (aztot_model_query(model, "boo", booq, 6 + AZTOT_BOO_MAX_ORDERS) < 6) die("boo");
    const int booEvery = (int)booq[2];
    bool booOn = booq[1] > 0.0;
    aztot_boo_params booPar = {};
    booPar.radius = booq[0]; booPar.n_bins = (int32_t)booq[1]; booPar.central_mask = (int32_t)booq[3]; booPar.ligand_mask = (int32_t)booq[4];
    booPar.n_orders = (int32_t)booq[5];
    for (int o = 0; o < booPar.n_orders && o < AZTOT_BOO_MAX_ORDERS; o++) booPar.orders[o] = (int32_t)booq[6 + o];
    if (booOn && aztot_boo_setup(md, &booPar) < 0)
    {
        std::fprintf(stderr, "WARNING: boo directive not usable (%s): no boo.dat\n", aztot_last_error());
        booOn = false;
    }
    auto boo_due = [&](int c) { return booOn && booEvery > 0 && c > nEq && c % booEvery == 0; };
    int booTaken = 0;
    aztot_stats st;
    for (int done = 0; done < nStep;)
    {
        int n = std::min(stat - done % stat, nStep - done);
        if (rdfOn)
        {   // next sample: the smallest c > done with (c - 1) % every == 0
            const int next = done < 1 ? 1 : done + 1 + (rdfEvery - (done % rdfEvery)) % rdfEvery;
            n = std::min(n, next - done);
        }
        if (tcfOn)
        {
            if (done < nEq) n = std::min(n, nEq - done);
            n = std::min(n, (std::max(done, nEq) / vafEvery + 1) * vafEvery - done);
        }
        if (stressOn) n = std::min(n, (done / stressEvery + 1) * stressEvery - done);
        if (adfOn && adfEvery > 0) n = std::min(n, (std::max(done, nEq) / adfEvery + 1) * adfEvery - done);
        if (skOn && skEvery > 0) n = std::min(n, (std::max(done, nEq) / skEvery + 1) * skEvery - done);
        if (booOn && booEvery > 0) n = std::min(n, (std::max(done, nEq) / booEvery + 1) * booEvery - done);
        if (aztot_step(md, n) != AZTOT_OK) die("step");
        done += n;
        if (boo_due(done))
        {
            if (aztot_boo_sample(md) != AZTOT_OK) die("boo sample");
            booTaken++;
        }
        if (sk_due(done))
        {
            if (aztot_sk_sample(md) != AZTOT_OK) die("sk sample");
            skTaken++;
        }
        if (adf_due(done))
        {
            if (aztot_adf_sample(md) != AZTOT_OK) die("adf sample");
            adfTaken++;
        }
        if (stress_due(done))
        {
            aztot_stress ps;
            if (aztot_stress_sample(md) != AZTOT_OK || aztot_stress_get(md, &ps) != AZTOT_OK) die("stress sample");
            std::fprintf(pf, "%f\t%d", ps.time, (int)ps.step);
            for (int k = 0; k < 6; k++) std::fprintf(pf, "\t%.12g", ps.pressure[k]);
            std::fprintf(pf, "\t%.12g\n", ps.pressure_iso);
        }
        if (rdf_due(done))
        {
            if (aztot_rdf_sample(md) != AZTOT_OK) die("rdf sample");
            if (rdfOut > 0 && (done - 1) % rdfOut == 0)
            {
                write_rdf(md, AZTOT_RDF_SPECIES, names, out + "/rdf" + std::to_string(done - 1) + ".dat");
                if (nucl) write_rdf(md, AZTOT_RDF_NUCLEI, nnames, out + "/rdf_n" + std::to_string(done - 1) + ".dat");
            }
        }
        const bool tcfNow = tcfOn && tcf_due(done);
        if (!stat_row(done) && !tcfNow) continue;
        if (aztot_get_stats(md, &st) != AZTOT_OK) die("stats");
        if (tcfNow)
        {
            if (nEq > 0 && done == nEq && aztot_tcf_reset(md) != AZTOT_OK) die("tcf reset");
            if (aztot_tcf_sample(md) != AZTOT_OK) die("tcf sample");
            int64_t taken = 0;
            if (aztot_tcf_shape(md, nullptr, nullptr, &taken) != AZTOT_OK) die("tcf shape");
            // one origin, sample 0: the lag of this sample is its number
            if (aztot_tcf_values(md, (int)taken - 1, 1, msdRow.data(), vafRow.data(), nSpec) < 0) die("tcf values");
            msdRow.resize(nSpec); vafRow.resize(nSpec);
            if (stat_row(done)) write_tcf_row(df, st.time, (int)st.step, msdRow);
            if (vaf_row(done)) write_tcf_row(vf, st.time, (int)st.step, vafRow);
        }
        if (!stat_row(done)) continue;
        std::fprintf(sf, "%f\t%d\t%f\t%f\t%f\t%f\t%f", st.time, (int)st.step, st.engTot, st.engKin, st.engVdW, st.engCoul, st.engCoulRec);
        if (radi) std::fprintf(sf, "\t%f", st.engTemp);
        if (hasB) std::fprintf(sf, "\t%f", st.engBond);
        if (hasA) std::fprintf(sf, "\t%f", st.engAngle);
        std::fprintf(sf, "\t%f\t%f\t%f\t%f\t%f\t%f\t%f\n", st.posMom[0], st.negMom[0], st.posMom[1], st.negMom[1], st.posMom[2], st.negMom[2], st.pressure);
        if (aztot_species_crossings(md, crossings.data(), (int)crossings.size()) != AZTOT_OK) die("species crossings");
        std::fprintf(mf, "%f\t%d", st.time, (int)st.step);
        for (int j = 0; j < nSpec; j++)        // our slots are Xn, Xp, Yn, Yp, Zn, Zp; the file wants px nx py ny pz nz
            std::fprintf(mf, "\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld", (long long)crossings[6 * j + 1], (long long)crossings[6 * j + 0],
                         (long long)crossings[6 * j + 3], (long long)crossings[6 * j + 2], (long long)crossings[6 * j + 5], (long long)crossings[6 * j + 4]);
        std::fprintf(mf, "\n");
        std::printf("time=%f(%d) Tot=%f Kin=%f VdW=%f Coul=%f T=%f P=%f\n", st.time, (int)st.step, st.engTot, st.engKin, st.engVdW, st.engCoul, st.temperature, st.pressure);
    }
    std::fclose(sf);
    std::fclose(mf);
    if (df) std::fclose(df);
    if (vf) std::fclose(vf);
    if (pf) std::fclose(pf);
    if (rdfOn)
    {
        write_rdf(md, AZTOT_RDF_SPECIES, names, out + "/rdf.dat");
        if (nucl) write_rdf(md, AZTOT_RDF_NUCLEI, nnames, out + "/rdf_n.dat");
    }
    if (adfOn)
    {
        if (adfTaken == 0 && aztot_adf_sample(md) != AZTOT_OK) die("adf sample");
        write_adf(md, adfCols, names, out + "/adf.dat", out + "/adf_n.dat");
    }
    if (booOn)
    {
        if (booTaken == 0 && aztot_boo_sample(md) != AZTOT_OK) die("boo sample");
        write_boo(md, booPar.central_mask, names, out + "/boo.dat", out + "/boo_n.dat");
    }
    if (skOn)
    {
        if (skTaken == 0 && aztot_sk_sample(md) != AZTOT_OK) die("sk sample");
        write_sk(md, names, out + "/sk.dat");
    }
    // coordination numbers: one snapshot of the final configuration (main.cu:446-448)
    auto query_all = [&](const char* key) {
        const int n = aztot_model_query(model, key, nullptr, 0);
        if (n < 0) die(key);
        std::vector<double> v(std::max(n, 1));
        if (aztot_model_query(model, key, v.data(), n) < 0) die(key);
        v.resize(n);
        return v;
    };
    const std::vector<double> ocn = query_all("outcn");
    if (ocn[0] != 0.0)
    {
        const int nC = (int)ocn[2], nL = (int)ocn[3];
        std::vector<aztot_cn_column> cols;
        for (int a = 0; a < nC; a++)
            for (int b = 0; b < nL; b++) cols.push_back({(int32_t)ocn[4 + a], (int32_t)ocn[4 + nC + b], ocn[1]});
        write_cn(md, AZTOT_CN_SPECIES, cols, names, out + "/CN.dat");
    }
    const std::vector<double> ncn = query_all("ncn");
    if (ncn[0] != 0.0)
    {
        std::vector<aztot_cn_column> cols;
        for (int i = 0; i < (int)ncn[0]; i++) cols.push_back({(int32_t)ncn[1 + 3 * i], (int32_t)ncn[2 + 3 * i], ncn[3 + 3 * i]});
        std::vector<std::string> nn;
        const int nNucl = (int)q1(model, "n_nuclei");
        for (int i = 0; i < nNucl; i++) { char b[16]; aztot_model_nucleus_name(model, i, b, 16); nn.push_back(b); }
        write_cn(md, AZTOT_CN_NUCLEI, cols, nn, out + "/nCN.dat");
    }

    std::vector<double> x(N), y(N), z(N), vx(N), vy(N), vz(N), U(N), rad(N);
    std::vector<int32_t> types(N);
    aztot_state s = {};
    s.n_atoms = N; s.x = x.data(); s.y = y.data(); s.z = z.data(); s.vx = vx.data(); s.vy = vy.data(); s.vz = vz.data();
    s.U = U.data(); s.radius = rad.data(); s.types = types.data();
    if (aztot_md_to_host(md, &s) != AZTOT_OK) die("md_to_host");

    if (FILE* f = std::fopen((out + "/revcon.xyz").c_str(), "w"))
    {
        std::fprintf(f, "%d\n%d %f %f %f\n", N, 1, box[0], box[1], box[2]);
        for (int i = 0; i < N; i++) std::fprintf(f, "%s\t%f\t%f\t%f\n", names[types[i]].c_str(), x[i], y[i], z[i]);
        std::fclose(f);
    }
    // per-species column tables (out_velocities / out_thermalchar layout)
    std::vector<std::vector<int>> bySpec(nSpec);
    size_t mx = 0;
    for (int i = 0; i < N; i++) bySpec[types[i]].push_back(i);
    for (auto& v : bySpec) mx = std::max(mx, v.size());
    if (FILE* f = std::fopen((out + "/velocities.dat").c_str(), "w"))
    {
        std::fprintf(f, "No");
        for (int j = 0; j < nSpec; j++) std::fprintf(f, "\t%s\tx\ty\tz", names[j].c_str());
        std::fprintf(f, "\n");
        for (size_t r = 0; r < mx; r++)
        {
            std::fprintf(f, "%zu", r + 1);
            for (int j = 0; j < nSpec; j++)
                if (r < bySpec[j].size())
                {
                    const int i = bySpec[j][r];
                    std::fprintf(f, "\t%f\t%f\t%f\t%f", std::sqrt(vx[i] * vx[i] + vy[i] * vy[i] + vz[i] * vz[i]), vx[i], vy[i], vz[i]);
                }
                else std::fprintf(f, "\t\t\t\t");
            std::fprintf(f, "\n");
        }
        std::fclose(f);
    }
    if (radi)
        if (FILE* f = std::fopen((out + "/tchars.dat").c_str(), "w"))
        {
            std::fprintf(f, "No");
            for (int j = 0; j < nSpec; j++) std::fprintf(f, "\t%s_eng\t%s_rad", names[j].c_str(), names[j].c_str());
            std::fprintf(f, "\n");
            for (size_t r = 0; r < mx; r++)
            {
                std::fprintf(f, "%zu", r + 1);
                for (int j = 0; j < nSpec; j++)
                    if (r < bySpec[j].size()) std::fprintf(f, "\t%f\t%f", U[bySpec[j][r]], rad[bySpec[j][r]]);
                    else std::fprintf(f, "\t\t");
                std::fprintf(f, "\n");
            }
            std::fclose(f);
        }
    aztot_free_device(md);
    aztot_free_md(model);
    const int spent = (int)(std::time(nullptr) - t0);
    std::printf("The program's just finished correctly, the running time: %d s\n", spent);
    return 0;
}
