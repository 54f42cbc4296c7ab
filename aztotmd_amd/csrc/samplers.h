// The samplers of one rank, behind the aztot_<name>_* calls of include/aztot.h:
//   rdf     radial distribution functions     rdf.hip.h
//   cn      coordination numbers              cn.hip.h
//   tcf     time correlation functions        tcf.hip.h
//   stress  pressure tensor                   stress.hip.h
//   adf     bond-angle distributions          adf.hip.h
//   sk      static structure factors          sk.hip.h
//   boo     bond-orientational order          boo.hip.h
// What several of them share - the private cell grid, its canonical order and the sliced neighbour walk - is in grid.hip.h; the tree-ordered sum over
// atom ids is next to wave_sum in kernels.hip.h.
// Each sampler owns its device buffers and its running totals; none of it is scheduling, so none of it is Engine's.  Host-only; the bodies are in
// samplers.hip.h, included by engine.hip, the one translation unit that sees the kernels.
//
// The contract.  A sample is launched on the engine's stream between two aztot_step calls, never inside a captured step.  It reads the current per-atom
// arrays - the configuration as aztot_md_to_host would return it: the deferred end of the last aztot_step call has happened - and writes only the samplers'
// own buffers.  It returns with the engine settled AND drained, as every reader does (aztot_get_stats): the next aztot_step must open on an idle stream.
// (Returning with a sample still running changed engKin in its last bit in about one run of three: sort_every = 1, seen in test_gpu_rdf.py.)  A set-up
// replaces buffers only when nothing queued or deferred can still use them, and commits only when everything has been allocated and uploaded.
#pragma once
#include <functional>
#include <vector>

#include "device_md.h"
#include "device_resources.h"
#include "model.h"

namespace aztot {

struct Counts;
struct AdfTables;

class Samplers
{
public:
    // The engine as the samplers see it, and all they see of it
    struct PairTables { StepParams P; SpecTable S; const DevPot* pots; long long step; };
    struct Host
    {
        virtual void quiesce() = 0;                         // everything queued or deferred by earlier calls has happened (before a set-up replaces buffers)
        virtual AtomArrays begin_sample() = 0;              // refuses a failed handle, completes the deferred end of the last aztot_step; the current arrays
        virtual void end_sample(const char* where) = 0;     // the launch check, then the stream drains: every sample ends here (one with a read-back passes twice)
        virtual void launch_timed(const char* name, const std::function<void()>& launch) = 0;   // under the per-kernel timer `name` when profiling is on
        virtual PairTables pair_tables() = 0;               // what pair_visit needs, and the number of the last completed step (valid after begin_sample)
    protected:
        ~Host() = default;
    };
    struct Box { double L[3], invL[3], half[3]; };

    Samplers(Host& host, const Model& model, const Box& box, hipStream_t stream, int nranks)
        : host_(host), model_(model), box_(box), stream_(stream), nranks_(nranks), nuclei_(nuclei_of(model)) {}
    Samplers(const Samplers&) = delete;

    // radial distribution functions: a private cell grid over the current positions, integer totals
    int rdf_setup(double rmax, double dr, bool nuclei);     // (re)allocates and zeroes; returns the number of bins
    void rdf_sample();
    void rdf_reset();
    // kind 0 species, 1 nuclei: bins, pairs, samples and (if counts) the totals [bin][pair]
    void rdf_counts(int kind, int& nBins, int& nPairs, long long& samples, std::vector<unsigned long long>* counts);
    void rdf_values(int kind, std::vector<double>& r, std::vector<double>& g);     // bin centres and normalised g(r), same layout

    // coordination numbers (include/aztot.h states the rules of the two kinds): each kind keeps a snapshot of its last sample
    void cn_setup(int kind, const aztot_cn_column* cols, int nCols);   // (re)allocates; replaces the columns and forgets the last sample of `kind`
    void cn_sample(int kind);
    void cn_shape(int kind, int& nCols, int& cnMin, int& cnMax);
    void cn_per_atom(int kind, std::vector<int32_t>& out);             // [atom id][column], -1 where the atom is not the column's central
    void cn_table(int kind, std::vector<long long>& out);              // [cn - cnMin][column]

    // time correlation functions (include/aztot.h states the terms, the summation tree and the ring of origins)
    int tcf_setup(int nOrigins, int originEvery);                      // (re)allocates and zeroes; returns the number of lags
    void tcf_sample();
    void tcf_reset();                                                  // zero sums and counts, forget the origins
    void tcf_shape(int& nLags, int& nSpec, long long& samples);
    // lags [lag0, lag0 + n): pairs seen and the raw sums [lag - lag0][species] (each output optional)
    void tcf_sums(int lag0, int n, std::vector<long long>* count, std::vector<double>* msd, std::vector<double>* vaf);
    void tcf_values(int lag0, int n, std::vector<double>& msd, std::vector<double>& vaf);     // sum / (count * atoms of the species), 0 where that is 0

    // pressure tensor of the pair terms (include/aztot.h states the pair set, the terms and the order of the sums): a snapshot of the last sample
    void stress_setup();
    void stress_sample();
    void stress_get(aztot_stress& out);
    void stress_per_atom(std::vector<double>& w);                      // [atom id][xx yy zz xy xz yz]

    // bond-angle distributions (include/aztot.h states the columns, the separation and the bin rule): integer totals over the samples
    int adf_setup(int nBins, const aztot_adf_column* cols, int nCols); // (re)allocates and zeroes; returns the number of bins
    void adf_sample();                                                 // refuses (before any total changes) when an atom has more than AZTOT_ADF_MAX_NEIGHBOURS
    void adf_reset();
    void adf_shape(int& nBins, int& nCols, long long& samples);
    void adf_edges(std::vector<double>& T);                            // the n_bins + 1 edge values
    void adf_counts(std::vector<unsigned long long>& counts);          // [bin][column]
    void adf_values(std::vector<double>& theta, std::vector<double>& p);   // bin centres in degrees, density per degree [bin][column]
    void adf_neighbours(std::vector<int32_t>& n);                      // [atom id] at the last sample (a refused one included), -1: not a central atom

    // static structure factors (include/aztot.h states the vector set, the order of the sums and the values): fp64 sums over the samples
    int sk_setup(double kmax, double dk, int maxPerBin);               // (re)allocates and zeroes; returns the number of k-vectors
    void sk_sample();
    void sk_reset();
    void sk_shape(int& nVectors, int& nBins, int& nPairs, long long& samples);
    void sk_vectors(std::vector<int32_t>& lmn, std::vector<int32_t>& bin);     // [vector][l, m, n] and the bin of each
    void sk_amplitudes(std::vector<double>& rho);                      // [vector][species][re, im] of the last sample
    void sk_sums(std::vector<double>& acc);                            // [vector][pair]
    void sk_values(std::vector<double>& k, std::vector<int32_t>& nInBin, std::vector<double>& sTotal, std::vector<double>& sPair);   // [bin], [bin], [bin], [bin][pair]

    // bond-orientational order (include/aztot.h states the bonds, the values, the order of the sums and the totals)
    int boo_setup(const aztot_boo_params& p);                          // (re)allocates and zeroes; returns the number of bins
    void boo_sample();
    void boo_reset();
    void boo_shape(int& nOrders, int& nBins, int& nSpec, long long& samples, int* orders = nullptr);
    void boo_per_atom(std::vector<int32_t>& n, std::vector<double>& q);    // by atom id: n[atom], q[(atom * n_orders + order) * 2 + kind]
    void boo_qlm(std::vector<double>& qlm);                            // [atom id][order][m 0 ... 12][re, im] of kind 0
    // hist [kind][order][species][bin], sums [kind][order][species], entered [species]
    void boo_counts(std::vector<unsigned long long>& hist, std::vector<double>& sums, std::vector<unsigned long long>& entered);
    void boo_values(std::vector<double>& centre, std::vector<double>& density, std::vector<double>& mean);     // [bin], hist's layout, sums' layout

private:
    // a private cell grid over the current positions and the buffers of its counting sort (k_grid_bin / k_scan_* / k_grid_place): every sampler that looks
    // at pairs has its own, each coordination-number set-up has one (different cell edges)
    struct GridSort
    {
        DeviceArena mem;
        int32_t *cellOf = nullptr, *rankOf = nullptr, *cellCount = nullptr, *cellStart = nullptr, *chunkTot = nullptr, *kind = nullptr;
        double *x = nullptr, *y = nullptr, *z = nullptr;
        Counts* scanCounts = nullptr;   // what k_scan_apply / k_scan_single write besides the offsets goes here, not into the engine's Counts / DevStats
        DevStats* scanStats = nullptr;
        RdfGrid grid{};
    };
    // ... filled in the canonical order (cells by position, ids ascending inside a cell): the slot order is a function of the sampled state alone
    struct CanonGrid : GridSort
    {
        int32_t *arrivalId = nullptr, *canonRank = nullptr;     // slot -> id map of the arrival order, rank of every atom's id among its cell-mates
        int32_t* slotId = nullptr;                              // slot -> id map of the canonical order, -1 until a sample writes it
    };
    // the sizes of the tree-ordered sum over the atom ids (kernels.hip.h): chunks of kTreeChunk ids, their number padded to a power of two, the ids padded
    // to whole chunks
    struct IdTree
    {
        int nChunk = 0, nChunkPad = 0;
        size_t nPad = 0;
        IdTree() = default;
        explicit IdTree(int N);
    };
    struct RdfState : GridSort
    {
        double rmax = 0, dr = 0;
        int nBins = 0;                  // 0: not set up
        bool nuclei = false;
        long long samples = 0;
        int copies = 0;                 // LDS sub-histograms per workgroup of k_rdf_pairs (0: straight into the totals)
        int blocks = 0;
        unsigned long long *histS = nullptr, *histN = nullptr;
    };
    struct CnState : GridSort
    {
        std::vector<aztot_cn_column> cols;          // empty: not set up
        CnParams par{};
        int sliceShift = 0;                         // lanes per atom in k_cn_pairs = 1 << sliceShift
        int nLive[kSpecCap] = {};                   // per central group: its columns ...
        int colOf[kSpecCap * kCnLive] = {};         // ... and which column each of its counters is
        bool sampled = false;
        int cnMin = 0, cnMax = 0, rowsCap = 0;
        int32_t *slotId = nullptr, *counts = nullptr, *range = nullptr, *dSlotOf = nullptr, *dNLive = nullptr, *dColOf = nullptr;
        double *dR2Of = nullptr, *dRowMax = nullptr;
        DeviceArena tableMem;                       // the table alone: it grows when a sample has more rows than any before
        unsigned long long* table = nullptr;
    };
    // the current state and a ring of origins in atom-id order, accumulators per lag
    struct TcfState
    {
        int M = 0, E = 0;               // origins in the ring and samples between two of them; M == 0: not set up
        long long samples = 0;          // since the set-up or the last reset
        int nSpec = 0;
        IdTree tree;
        DeviceArena mem;
        double *cur = nullptr, *ring = nullptr, *partials = nullptr, *msdSum = nullptr, *vafSum = nullptr;
        int32_t* type = nullptr;        // species by atom id, -1 in the padding
        long long* count = nullptr;
        int n_lags() const { return M * E; }
    };

    // per-atom columns by atom id (StressCol), their chunk sums and totals; the grid carries the canonical in-cell order
    struct StressState : CanonGrid
    {
        bool isSetUp = false, sampled = false;
        int sliceShift = 0;
        IdTree tree;
        int32_t *visits = nullptr, *drops = nullptr;
        double *rad = nullptr, *cols = nullptr, *partials = nullptr, *totals = nullptr;
        unsigned long long* counters = nullptr;
        long long step = 0;             // of the last sample
    };

    // columns normalised to ligand_a <= ligand_b, the edge table, uint64 totals [bin][column]
    struct AdfState : GridSort
    {
        int nBins = 0;                  // 0: not set up
        std::vector<aztot_adf_column> cols;
        std::vector<double> edges;
        long long samples = 0;
        bool counted = false;           // the neighbour counts of a sample are there
        int sliceShift = 0, useLds = 0;
        int32_t *slotId = nullptr, *neigh = nullptr;
        unsigned long long *summary = nullptr, *totals = nullptr;   // summary: the largest neighbour count << 32 | the id of an atom that has it
        AdfTables* tables = nullptr;
        int8_t* colOf = nullptr;
        double* dEdges = nullptr;
    };

    // the kept k-vectors in lexicographic order with their bins, positions and species by atom id, row sums of a batch of vectors, amplitudes of the last
    // sample, sums over the samples
    struct SkState
    {
        double kmax = 0, dk = 0;
        int maxPerBin = 0, nBins = 0;   // nBins == 0: not set up
        int nK = 0, nSpec = 0, nPairs = 0;
        long long samples = 0;
        bool sampled = false;           // the amplitudes of a sample are there
        std::vector<int32_t> lmn, bin, nInBin;
        int h[3] = {1, 1, 1};           // entries of the per-axis harmonic tables: the largest |harmonic| of the set + 1
        int tile = 0, nRows = 0, nIdTiles = 0, batch = 0;      // atoms per LDS tile, rows and 64-id tiles of the summation order, vectors per launch
        DeviceArena mem;
        double *x = nullptr, *y = nullptr, *z = nullptr, *partial = nullptr, *rho = nullptr, *acc = nullptr;
        int32_t *type = nullptr, *dLmn = nullptr;
    };

    // the set-up with its host-made tables, q_lm and n in canonical slot order, per-atom values by atom id, their chunk sums, totals over the samples
    struct BooState : CanonGrid
    {
        int nBins = 0;                  // 0: not set up
        aztot_boo_params par{};
        long long samples = 0;
        bool sampled = false;           // the per-atom values of a sample are there
        int nSpec = 0, stride = 0, sliceShift = 0, useLds = 0;
        IdTree tree;
        size_t nHist = 0;               // histogram cells (the entered counts follow them)
        int32_t *nSlot = nullptr, *nById = nullptr, *typeById = nullptr;
        double *qlm = nullptr, *qCols = nullptr, *partials = nullptr, *sums = nullptr;
        unsigned long long* totals = nullptr;
    };

    // the protocol every sampler follows, once (samplers.hip.h)
    void need_one_gpu(const char* what) const;
    static void need_setup(bool isSetUp, const char* name, const char* tail = "");
    template <typename State, typename F> void set_up(State& slot, State& fresh, F&& allocate);
    template <typename F> void sample(const char* where, F&& launch);
    template <typename F> void timed(const char* name, F&& launch) { host_.launch_timed(name, launch); }

    void grid_setup(GridSort& S, double edge);                                              // cells with an edge >= `edge`, at most about N of them; allocates the sort's buffers
    void grid_fill(GridSort& S, const AtomArrays& A, const char* const timerNames[3]);      // bin, scan, place the positions of A (timer names of the three stages)
    void grid_count(GridSort& S, const AtomArrays& A, const char* const timerNames[2]);     // ... the first two: cell, arrival rank and cell offsets
    void canon_setup(CanonGrid& S, double edge);                                            // grid_setup and the buffers of the canonical order
    // bin, scan, ids, rank, place: grid_fill in the canonical order (timer names of the five stages); slotIds: the place stage also writes S.slotId
    void grid_fill_canonical(CanonGrid& S, const AtomArrays& A, const char* const timerNames[5], bool slotIds);
    int lanes_shift() const;                                                                // log2 of the lanes per atom of a sliced walk (SliceLane)
    int lane_blocks(int shift) const;                                                       // workgroups of a launch with that many lanes per atom
    RdfState& rdf_state();
    CnState& cn_state(int kind, bool needSetup, bool needSample);
    TcfState& tcf_state();
    StressState& stress_state(bool needSample);
    AdfState& adf_state();
    SkState& sk_state();
    BooState& boo_state(bool needSample);

    Host& host_;
    const Model& model_;            // the engine's (outlives the samplers)
    const Box box_;
    const hipStream_t stream_;
    const int nranks_;
    const Nuclei nuclei_;
    RdfState rdf_;
    CnState cn_[2];                 // AZTOT_CN_SPECIES, AZTOT_CN_NUCLEI
    TcfState tcf_;
    StressState stress_;
    AdfState adf_;
    SkState sk_;
    BooState boo_;
};

}  // namespace aztot
