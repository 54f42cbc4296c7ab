// Samplers: the bodies (see samplers.h for the contract).  Included by engine.hip behind the kernel headers and its own helpers (HIP_CHECK, div_up).
#pragma once
#include "samplers.h"
#include "stress.hip.h"
#include "boo.hip.h"

namespace aztot {

// ---------------------------------------------------------------------------------------------------
// The protocol, once
// ---------------------------------------------------------------------------------------------------
void Samplers::need_one_gpu(const char* what) const
{
    if (nranks_ > 1) throw std::runtime_error(std::string("out of scope: ") + what + " of a slab-decomposed (multi-GPU) run are not supported");
}

void Samplers::need_setup(bool isSetUp, const char* name, const char* tail)
{
    if (!isSetUp) throw ArgError(std::string(name) + ": aztot_" + name + "_setup has not been called" + tail);
}

// A set-up, all or nothing.  The caller has validated its arguments (a bad call leaves the earlier set-up in place) and filled the host side of `fresh`;
// `allocate` allocates and uploads the device side of it.  The earlier set-up is freed first - never two generations in memory - and `fresh` is committed only when
// everything is in place.  No room: no sampler ("not set up"), and the handle steps on - the refused allocation must not surface at the next launch check.
template <typename State, typename F> void Samplers::set_up(State& slot, State& fresh, F&& allocate)
{
    host_.quiesce();
    slot = State();                 // (nothing can still use its buffers: the stream has just drained)
    try
    {
        allocate();
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    catch (...)
    {
        (void)hipStreamSynchronize(stream_);
        (void)hipGetLastError();
        throw;
    }
    slot = std::move(fresh);
}

// A sample: the engine settles, `launch` queues the kernels on the arrays as they then stand, and the engine is left settled and drained
template <typename F> void Samplers::sample(const char* where, F&& launch)
{
    const AtomArrays A = host_.begin_sample();
    launch(A);
    host_.end_sample(where);
}

Samplers::RdfState& Samplers::rdf_state() { need_setup(rdf_.nBins != 0, "rdf"); return rdf_; }
Samplers::TcfState& Samplers::tcf_state() { need_setup(tcf_.M != 0, "tcf"); return tcf_; }
Samplers::StressState& Samplers::stress_state(bool needSample)
{
    need_setup(stress_.isSetUp, "stress");
    if (needSample && !stress_.sampled) throw ArgError("stress: aztot_stress_sample has not been called since the set-up");
    return stress_;
}
Samplers::CnState& Samplers::cn_state(int kind, bool needSetup, bool needSample)
{
    if (kind != AZTOT_CN_SPECIES && kind != AZTOT_CN_NUCLEI) throw ArgError("cn: kind must be AZTOT_CN_SPECIES or AZTOT_CN_NUCLEI");
    CnState& S = cn_[kind];
    if (needSetup) need_setup(!S.cols.empty(), "cn", " for this kind");
    if (needSample && !S.sampled) throw ArgError("cn: aztot_cn_sample has not been called since the set-up of this kind");
    return S;
}

// ---------------------------------------------------------------------------------------------------
// The private cell grid of the samplers that look at pairs (grid.hip.h), their lanes, and the sizes of the sum tree
// ---------------------------------------------------------------------------------------------------
// cells with an edge >= `edge` (a hair more: the cell of a coordinate is floor(x * nc / L) in fp64), at most about N of them (a dilute gas in a large box
// would otherwise get mostly empty cells); the buffers of the counting sort.  Histogram fields of the grid are the caller's.
void Samplers::grid_setup(GridSort& S, double edge)
{
    RdfGrid& G = S.grid;
    const int N = model_.nAt;
    long long nc[3];
    for (int k = 0; k < 3; k++) nc[k] = std::max(1LL, (long long)std::floor(box_.L[k] / (edge * (1.0 + 1e-9))));
    const long long cellCap = std::max(27, N);
    while (nc[0] * nc[1] * nc[2] > cellCap)
    {
        const int k = (nc[0] >= nc[1] && nc[0] >= nc[2]) ? 0 : (nc[1] >= nc[2] ? 1 : 2);
        nc[k] = std::max(1LL, nc[k] * 3 / 4);
    }
    for (int k = 0; k < 3; k++)
    {
        G.nc[k] = (int)nc[k];
        G.L[k] = box_.L[k]; G.invL[k] = box_.invL[k]; G.half[k] = box_.half[k];
        G.icsz[k] = (double)nc[k] / box_.L[k];
    }
    G.nCell = G.nc[0] * G.nc[1] * G.nc[2];
    G.halfShell = (G.nc[0] >= 3 && G.nc[1] >= 3 && G.nc[2] >= 3) ? 1 : 0;
    for (int t = 0; t < kSpecCap; t++) G.nucl[t] = t < model_.nSpec() ? nuclei_.of[t] : 0;
    const size_t n = (size_t)std::max(N, 1);
    S.cellOf = S.mem.alloc<int32_t>(n, false, stream_); S.rankOf = S.mem.alloc<int32_t>(n, false, stream_); S.kind = S.mem.alloc<int32_t>(n, false, stream_);
    S.x = S.mem.alloc<double>(n, false, stream_); S.y = S.mem.alloc<double>(n, false, stream_); S.z = S.mem.alloc<double>(n, false, stream_);
    S.cellCount = S.mem.alloc<int32_t>((size_t)G.nCell, true, stream_); S.cellStart = S.mem.alloc<int32_t>((size_t)(G.nCell + 1), false, stream_);
    S.chunkTot = S.mem.alloc<int32_t>((size_t)div_up(G.nCell, kScanChunk), false, stream_);
    S.scanCounts = S.mem.alloc<Counts>(1, true, stream_); S.scanStats = S.mem.alloc<DevStats>(1, true, stream_);
}

// the first two stages of the counting sort: cell and arrival rank of every atom, exclusive scan of the cell counts (which it leaves cleared for the next sample)
void Samplers::grid_count(GridSort& S, const AtomArrays& A, const char* const timerNames[2])
{
    const RdfGrid& G = S.grid;
    const int N = model_.nAt;
    const int nb = div_up(N, kBlock);
    timed(timerNames[0], [&] { hipLaunchKernelGGL(k_grid_bin, dim3(nb), dim3(kBlock), 0, stream_, G, A, N, S.cellOf, S.rankOf, S.cellCount); });
    if (G.nCell <= kScanSingleMax)
        timed(timerNames[1], [&] { hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, stream_, G.nCell, S.cellCount, S.cellStart, S.scanCounts, S.scanStats, 0); });
    else
        timed(timerNames[1], [&] {
            const int nChunk = div_up(G.nCell, kScanChunk);
            hipLaunchKernelGGL(k_scan_totals, dim3(nChunk), dim3(kBlock), 0, stream_, G.nCell, S.cellCount, S.chunkTot);
            hipLaunchKernelGGL(k_scan_apply, dim3(nChunk), dim3(kBlock), 0, stream_, G.nCell, S.cellCount, S.chunkTot, S.cellStart, S.scanCounts, S.scanStats, 0);
        });
}

// counting sort of the positions of A into the grid: wrapped coordinates and species | nucleus << 8 in slot order
void Samplers::grid_fill(GridSort& S, const AtomArrays& A, const char* const timerNames[3])
{
    const int N = model_.nAt;
    grid_count(S, A, timerNames);
    timed(timerNames[2], [&] {
        hipLaunchKernelGGL(k_grid_place, dim3(div_up(N, kBlock)), dim3(kBlock), 0, stream_, S.grid, A, N, S.cellOf, S.rankOf, S.cellStart, S.x, S.y, S.z, S.kind);
    });
}

void Samplers::canon_setup(CanonGrid& S, double edge)
{
    grid_setup(S, edge);
    const size_t n = (size_t)std::max(model_.nAt, 1);
    S.arrivalId = S.mem.alloc<int32_t>(n, false, stream_); S.canonRank = S.mem.alloc<int32_t>(n, false, stream_);
    S.slotId = S.mem.alloc<int32_t>(n, false, stream_);
    HIP_CHECK(hipMemsetAsync(S.slotId, 0xff, sizeof(int32_t) * n, stream_));
}

// the counting sort with the arrival rank k_grid_bin hands out replaced by the rank of the atom's id among its cell-mates
void Samplers::grid_fill_canonical(CanonGrid& S, const AtomArrays& A, const char* const timerNames[5], bool slotIds)
{
    const int N = model_.nAt, nb = div_up(N, kBlock);
    grid_count(S, A, timerNames);
    timed(timerNames[2], [&] { hipLaunchKernelGGL(k_grid_slot_ids, dim3(nb), dim3(kBlock), 0, stream_, A, N, S.cellOf, S.rankOf, S.cellStart, S.arrivalId); });
    timed(timerNames[3], [&] { hipLaunchKernelGGL(k_grid_canon_rank, dim3(nb), dim3(kBlock), 0, stream_, A, N, S.cellOf, S.cellStart, S.arrivalId, S.canonRank); });
    timed(timerNames[4], [&] {
        hipLaunchKernelGGL(k_grid_place, dim3(nb), dim3(kBlock), 0, stream_, S.grid, A, N, S.cellOf, S.canonRank, S.cellStart, S.x, S.y, S.z, S.kind);
        if (slotIds) hipLaunchKernelGGL(k_grid_slot_ids, dim3(nb), dim3(kBlock), 0, stream_, A, N, S.cellOf, S.canonRank, S.cellStart, S.slotId);
    });
}

// Lanes per atom of a sliced walk: enough of them that a small system still fills the chip (256 CUs x 4 waves of 64 at the least), never more than one wave.
// A function of N alone, so that the order of every per-atom sum is one too.
int Samplers::lanes_shift() const
{
    int shift = 0;
    while (shift < 6 && ((long long)std::max(model_.nAt, 1) << shift) < 65536) shift++;
    return shift;
}

int Samplers::lane_blocks(int shift) const { return (int)((((long long)model_.nAt << shift) + kBlock - 1) / kBlock); }

Samplers::IdTree::IdTree(int N) : nChunk(std::max(1, div_up(N, kTreeChunk))), nChunkPad(1), nPad((size_t)nChunk * kTreeChunk)
{
    while (nChunkPad < nChunk) nChunkPad <<= 1;
}

// ---------------------------------------------------------------------------------------------------
// Radial distribution functions (rdf.hip.h)
// ---------------------------------------------------------------------------------------------------
int Samplers::rdf_setup(double rmax, double dr, bool nuclei)
{
    need_one_gpu("radial distribution functions");
    if (!(rmax > 0.0) || !(dr > 0.0)) throw ArgError("rdf: rmax and dr must be positive");
    // bins as init_rdf (rdf.cpp:40-48, what sizes the GPU path's buffer): min(rmax, L_x) / dr
    const double nb = std::min(rmax, box_.L[0]) * (1.0 / dr);
    if (!(nb >= 1.0)) throw ArgError("rdf: no bin (dr > min(rmax, box x edge))");
    const int nSpec = model_.nSpec(), nNucl = (int)nuclei_.names.size();
    const long long nPairS = (long long)nSpec * (nSpec + 1) / 2, nPairN = nuclei ? (long long)nNucl * (nNucl + 1) / 2 : 0;
    if (nb * (double)(nPairS + nPairN) > (double)(1 << 28)) throw ArgError("rdf: too many bins (min(rmax, box x edge) / dr x pairs > 2^28)");
    RdfState R;
    R.rmax = rmax; R.dr = dr; R.nuclei = nuclei; R.nBins = (int)nb;
    const size_t nEnt = (size_t)R.nBins * (size_t)(nPairS + nPairN);
    R.copies = (4 * nEnt * sizeof(uint32_t) <= (size_t)kRdfLdsBudget) ? 4 : (nEnt * sizeof(uint32_t) <= (size_t)kRdfLdsBudget ? 1 : 0);
    R.blocks = std::max(1, std::min(kRdfMaxBlocks, div_up(model_.nAt, kBlock)));
    set_up(rdf_, R, [&] {
        grid_setup(R, rmax);
        RdfGrid& G = R.grid;
        G.r2max = rmax * rmax; G.idr = 1.0 / dr; G.nBins = R.nBins;
        G.nSpec = nSpec; G.nPairS = (int)nPairS;
        G.nNucl = nNucl; G.nPairN = (int)nPairN;
        R.histS = R.mem.alloc<unsigned long long>((size_t)R.nBins * nPairS, true, stream_);
        R.histN = R.mem.alloc<unsigned long long>((size_t)R.nBins * std::max(nPairN, 1LL), true, stream_);
    });
    return rdf_.nBins;
}

void Samplers::rdf_reset()
{
    RdfState& R = rdf_state();
    HIP_CHECK(hipMemsetAsync(R.histS, 0, (size_t)R.nBins * R.grid.nPairS * 8, stream_));
    if (R.grid.nPairN) HIP_CHECK(hipMemsetAsync(R.histN, 0, (size_t)R.nBins * R.grid.nPairN * 8, stream_));
    R.samples = 0;
    HIP_CHECK(hipStreamSynchronize(stream_));
}

void Samplers::rdf_sample()
{
    RdfState& R = rdf_state();
    sample("rdf kernels", [&](const AtomArrays& A) {
        const RdfGrid& G = R.grid;
        const int N = model_.nAt;
        if (N < 2) return;
        static const char* const names[3] = {"k_rdf_bin", "k_rdf_scan", "k_rdf_place"};
        grid_fill(R, A, names);
        const size_t lds = (size_t)R.copies * (size_t)R.nBins * (size_t)(G.nPairS + G.nPairN) * sizeof(uint32_t);
        timed("k_rdf_pairs", [&] {
            hipLaunchKernelGGL(k_rdf_pairs, dim3(R.blocks), dim3(kBlock), lds, stream_, G, N, R.cellStart, R.x, R.y, R.z, R.kind, R.copies, R.histS, R.histN);
        });
    });
    R.samples++;
}

void Samplers::rdf_counts(int kind, int& nBins, int& nPairs, long long& samples, std::vector<unsigned long long>* counts)
{
    const RdfState& R = rdf_state();
    if (kind != 0 && kind != 1) throw ArgError("rdf: kind must be AZTOT_RDF_SPECIES or AZTOT_RDF_NUCLEI");
    if (kind == 1 && !R.nuclei) throw ArgError("rdf: nuclei histograms were not requested at aztot_rdf_setup");
    nBins = R.nBins;
    nPairs = kind ? R.grid.nPairN : R.grid.nPairS;
    samples = R.samples;
    if (!counts) return;
    counts->resize((size_t)nBins * nPairs);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(counts->data(), kind ? R.histN : R.histS, counts->size() * 8, hipMemcpyDeviceToHost));
}

// g(r) as copy_rdf / copy_nrdf / out_rdf (cuStat.cu:514-560,719-760; rdf.cpp:128-175):
//   g = count * V / (nA nB) * 2 / (sphera dr^3 samples) / (3 i (i + 1) + 1) * C3,   C3 = 1 for A-A, 0.5 for A-B;  0 where nA nB = 0 or no sample
void Samplers::rdf_values(int kind, std::vector<double>& r, std::vector<double>& g)
{
    int nBins = 0, nPairs = 0;
    long long samples = 0;
    std::vector<unsigned long long> c;
    rdf_counts(kind, nBins, nPairs, samples, &c);
    std::vector<double> num;
    if (kind == 0) for (const auto& s : model_.species) num.push_back((double)s.number);
    else for (int v : nuclei_.number) num.push_back((double)v);
    const int n = (int)num.size();
    const double sphera = 4.0 * units::pi / 3.0;                        // const.h:15
    const double dr = rdf_.dr, V = box_.L[0] * box_.L[1] * box_.L[2];
    const double C1 = samples > 0 ? 2.0 / (sphera * dr * dr * dr * (double)samples) : 0.0;
    r.resize(nBins);
    g.assign((size_t)nBins * nPairs, 0.0);
    for (int i = 0; i < nBins; i++)
    {
        r[i] = (i + 0.5) * dr;
        const double C2 = 1.0 / (3.0 * i * (i + 1.0) + 1.0);
        int p = 0;
        for (int a = 0; a < n; a++)
            for (int b = a; b < n; b++, p++)
            {
                const double nAnB = num[a] * num[b];
                if (nAnB == 0.0) continue;
                const double C3 = a == b ? 1.0 : 0.5;
                g[(size_t)i * nPairs + p] = (double)c[(size_t)i * nPairs + p] * V / nAnB * C1 * C2 * C3;
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// Coordination numbers (cn.hip.h; the rules of the two kinds are stated in include/aztot.h)
// ---------------------------------------------------------------------------------------------------
void Samplers::cn_setup(int kind, const aztot_cn_column* cols, int nCols)
{
    need_one_gpu("coordination numbers");
    cn_state(kind, false, false);
    if (!cols || nCols <= 0) throw ArgError("cn: no columns");
    const int nGroups = kind == AZTOT_CN_SPECIES ? model_.nSpec() : (int)nuclei_.names.size();
    CnState T;
    std::vector<int32_t> slotOf(kSpecCap * kSpecCap, -1);
    std::vector<double> r2Of(kSpecCap * kSpecCap, 0.0), rowMax(kSpecCap, -1.0);
    double rBig = 0.0;
    for (int c = 0; c < nCols; c++)
    {
        const aztot_cn_column& col = cols[c];
        if (col.central < 0 || col.central >= nGroups || col.ligand < 0 || col.ligand >= nGroups) throw ArgError("cn: group index of a column out of range");
        if (!(col.radius > 0.0) || !std::isfinite(col.radius)) throw ArgError("cn: the radius of a column must be positive");
        if (kind == AZTOT_CN_SPECIES && col.radius != cols[0].radius) throw ArgError("cn: AZTOT_CN_SPECIES columns share one radius (outCN has one)");
        const int e = col.central * kSpecCap + col.ligand;
        if (slotOf[e] >= 0) throw ArgError("cn: the same (central, ligand) pair names two columns");
        const int q = T.nLive[col.central]++;           // (<= nGroups <= kCnLive: every ligand of a central group is distinct)
        slotOf[e] = q;
        r2Of[e] = col.radius * col.radius;
        rowMax[col.central] = std::max(rowMax[col.central], r2Of[e]);
        T.colOf[col.central * kCnLive + q] = c;
        T.par.maxLive = std::max(T.par.maxLive, q + 1);
        rBig = std::max(rBig, col.radius);
    }
    T.cols.assign(cols, cols + nCols);
    T.par.shift = kind == AZTOT_CN_SPECIES ? 0 : 8;
    T.par.inclusive = kind == AZTOT_CN_SPECIES ? 1 : 0;
    T.par.countSelf = kind == AZTOT_CN_SPECIES ? 1 : 0;
    T.par.nCols = nCols;
    const int N = model_.nAt;
    T.sliceShift = lanes_shift();
    T.rowsCap = 64;
    set_up(cn_[kind], T, [&] {
        CnState& S = T;
        grid_setup(S, rBig);
        const size_t n = (size_t)std::max(N, 1);
        S.slotId = S.mem.alloc<int32_t>(n, false, stream_);
        S.counts = S.mem.alloc<int32_t>(n * (size_t)S.par.maxLive, false, stream_);
        S.range = S.mem.alloc<int32_t>(2, false, stream_);
        S.dSlotOf = S.mem.alloc<int32_t>(slotOf.size(), false, stream_); S.dR2Of = S.mem.alloc<double>(r2Of.size(), false, stream_);
        S.dRowMax = S.mem.alloc<double>(rowMax.size(), false, stream_);
        S.dNLive = S.mem.alloc<int32_t>(kSpecCap, false, stream_); S.dColOf = S.mem.alloc<int32_t>(kSpecCap * kCnLive, false, stream_);
        HIP_CHECK(hipMemcpy(S.dSlotOf, slotOf.data(), slotOf.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(S.dR2Of, r2Of.data(), r2Of.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(S.dRowMax, rowMax.data(), rowMax.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(S.dNLive, S.nLive, sizeof(S.nLive), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(S.dColOf, S.colOf, sizeof(S.colOf), hipMemcpyHostToDevice));
        S.table = S.tableMem.alloc<unsigned long long>((size_t)S.rowsCap * nCols, false, stream_);
    });
}

template <int NL>
static void launch_cn_pairs(hipStream_t stream, int blocks, const RdfGrid& G, const CnParams& C, int N, int sliceShift, const int32_t* cellStart, const double* x,
                            const double* y, const double* z, const int32_t* kind, const int32_t* slotOf, const double* r2Of, const double* rowMax, int32_t* counts)
{
    hipLaunchKernelGGL(k_cn_pairs<NL>, dim3(blocks), dim3(kBlock), 0, stream, G, C, N, sliceShift, cellStart, x, y, z, kind, slotOf, r2Of, rowMax, counts);
}

void Samplers::cn_sample(int kind)
{
    CnState& S = cn_state(kind, true, false);
    sample("cn table", [&](const AtomArrays& A) {
        const int N = model_.nAt;
        const CnParams& C = S.par;
        // rows of the file: out_cn starts its maximum at 0 and writes from CN = 0 (out_md.cpp:392,486); out_ncn starts from mn = 10, mx = 0 (out_md.cpp:300)
        int range[2] = {kind == AZTOT_CN_SPECIES ? 0 : 10, 0};
        S.sampled = false;
        S.cnMin = range[0]; S.cnMax = range[1];
        if (N == 0) return;
        static const char* const names[3] = {"k_cn_bin", "k_cn_scan", "k_cn_place"};
        grid_fill(S, A, names);
        const int nb = div_up(N, kBlock);
        timed("k_cn_ids", [&] { hipLaunchKernelGGL(k_grid_slot_ids, dim3(nb), dim3(kBlock), 0, stream_, A, N, S.cellOf, S.rankOf, S.cellStart, S.slotId); });
        const int blocks = lane_blocks(S.sliceShift);
        timed("k_cn_pairs", [&] {
            auto go = [&](auto nl) {
                launch_cn_pairs<decltype(nl)::value>(stream_, blocks, S.grid, C, N, S.sliceShift, S.cellStart, S.x, S.y, S.z, S.kind, S.dSlotOf, S.dR2Of, S.dRowMax, S.counts);
            };
            if (C.maxLive <= 1) go(std::integral_constant<int, 1>());
            else if (C.maxLive <= 2) go(std::integral_constant<int, 2>());
            else if (C.maxLive <= 4) go(std::integral_constant<int, 4>());
            else if (C.maxLive <= 8) go(std::integral_constant<int, 8>());
            else go(std::integral_constant<int, kCnLive>());
        });
        HIP_CHECK(hipMemcpyAsync(S.range, range, sizeof(range), hipMemcpyHostToDevice, stream_));
        const int gs = std::max(1, std::min(kCnMaxBlocks, nb));
        timed("k_cn_range", [&] { hipLaunchKernelGGL(k_cn_range, dim3(gs), dim3(kBlock), 0, stream_, C, N, S.kind, S.dNLive, S.counts, S.range); });
        HIP_CHECK(hipMemcpyAsync(range, S.range, sizeof(range), hipMemcpyDeviceToHost, stream_));
        host_.end_sample("cn kernels");     // the table's rows are sized on the host from the range just read back
        S.cnMin = range[0]; S.cnMax = range[1];
        const int rows = S.cnMax - S.cnMin + 1;
        if (rows <= 0) return;
        if ((double)rows * C.nCols > (double)(1 << 28)) throw ArgError("cn: table too large (rows x columns > 2^28)");
        if (rows > S.rowsCap)
        {
            S.rowsCap = rows + rows / 2;
            S.tableMem = DeviceArena();
            S.table = S.tableMem.alloc<unsigned long long>((size_t)S.rowsCap * C.nCols, false, stream_);
        }
        const size_t ent = (size_t)rows * C.nCols;
        HIP_CHECK(hipMemsetAsync(S.table, 0, ent * 8, stream_));
        const int useLds = ent * sizeof(uint32_t) <= (size_t)kCnLdsBudget ? 1 : 0;
        timed("k_cn_table", [&] {
            hipLaunchKernelGGL(k_cn_table, dim3(gs), dim3(kBlock), useLds ? ent * sizeof(uint32_t) : 0, stream_, C, N, S.kind, S.dNLive, S.dColOf, S.counts, S.cnMin,
                               rows, useLds, S.table);
        });
    });
    S.sampled = true;
}

void Samplers::cn_shape(int kind, int& nCols, int& cnMin, int& cnMax)
{
    const CnState& S = cn_state(kind, true, true);
    nCols = S.par.nCols; cnMin = S.cnMin; cnMax = S.cnMax;
}

void Samplers::cn_per_atom(int kind, std::vector<int32_t>& out)
{
    const CnState& S = cn_state(kind, true, true);
    const int N = model_.nAt, nCols = S.par.nCols, ml = S.par.maxLive;
    out.assign((size_t)N * nCols, -1);
    if (N == 0) return;
    std::vector<int32_t> ids(N), kinds(N), cnt((size_t)N * ml);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(ids.data(), S.slotId, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(kinds.data(), S.kind, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(cnt.data(), S.counts, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost));
    for (int s = 0; s < N; s++)
    {
        const int g = (kinds[s] >> S.par.shift) & 255;
        for (int q = 0; q < S.nLive[g]; q++) out[(size_t)ids[s] * nCols + S.colOf[g * kCnLive + q]] = cnt[(size_t)s * ml + q];
    }
}

void Samplers::cn_table(int kind, std::vector<long long>& out)
{
    const CnState& S = cn_state(kind, true, true);
    const int rows = std::max(0, S.cnMax - S.cnMin + 1);
    out.assign((size_t)rows * S.par.nCols, 0);
    if (out.empty() || model_.nAt == 0) return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(out.data(), S.table, out.size() * 8, hipMemcpyDeviceToHost));
}

// ---------------------------------------------------------------------------------------------------
// Time correlation functions (tcf.hip.h; terms, summation tree and ring of origins are stated in include/aztot.h)
// ---------------------------------------------------------------------------------------------------
int Samplers::tcf_setup(int nOrigins, int originEvery)
{
    need_one_gpu("time correlation functions");
    if (nOrigins < 1 || originEvery < 1) throw ArgError("tcf: n_origins and origin_every must be at least 1");
    if ((long long)nOrigins * originEvery > AZTOT_TCF_MAX_LAGS) throw ArgError("tcf: too many lags (n_origins x origin_every > 2^24)");
    TcfState T;
    T.M = nOrigins; T.E = originEvery; T.nSpec = model_.nSpec();
    T.tree = IdTree(model_.nAt);
    set_up(tcf_, T, [&] {
        const size_t nAcc = (size_t)T.n_lags() * T.nSpec, nPad = T.tree.nPad;
        T.cur = T.mem.alloc<double>(6 * nPad, true, stream_);
        T.ring = T.mem.alloc<double>((size_t)T.M * 6 * nPad, true, stream_);
        T.type = T.mem.alloc<int32_t>(nPad, false, stream_);
        HIP_CHECK(hipMemsetAsync(T.type, 0xff, sizeof(int32_t) * nPad, stream_));
        T.partials = T.mem.alloc<double>((size_t)T.M * 2 * T.nSpec * T.tree.nChunkPad, true, stream_);
        T.msdSum = T.mem.alloc<double>(nAcc, true, stream_); T.vafSum = T.mem.alloc<double>(nAcc, true, stream_);
        T.count = T.mem.alloc<long long>((size_t)T.n_lags(), true, stream_);
    });
    return tcf_.n_lags();
}

void Samplers::tcf_reset()
{
    TcfState& T = tcf_state();
    const size_t nAcc = (size_t)T.n_lags() * T.nSpec;
    HIP_CHECK(hipMemsetAsync(T.msdSum, 0, nAcc * 8, stream_));
    HIP_CHECK(hipMemsetAsync(T.vafSum, 0, nAcc * 8, stream_));
    HIP_CHECK(hipMemsetAsync(T.count, 0, (size_t)T.n_lags() * 8, stream_));
    T.samples = 0;
    HIP_CHECK(hipStreamSynchronize(stream_));
}

void Samplers::tcf_sample()
{
    TcfState& T = tcf_state();
    sample("tcf kernels", [&](const AtomArrays& A) {
        const int N = model_.nAt;
        const long long c = T.samples;
        const IdTree& tree = T.tree;
        TcfBox B;
        for (int k = 0; k < 3; k++) { B.L[k] = box_.L[k]; B.invL[k] = box_.invL[k]; B.half[k] = box_.half[k]; }
        const bool isOrigin = c % T.E == 0;
        double* org = isOrigin ? T.ring + (size_t)((c / T.E) % T.M) * 6 * tree.nPad : nullptr;
        if (N > 0)
            timed("k_tcf_gather", [&] { hipLaunchKernelGGL(k_tcf_gather, dim3(div_up(N, kBlock)), dim3(kBlock), 0, stream_, B, A, N, tree.nPad, T.cur, org, T.type); });
        const int nLive = (int)std::min<long long>(c / T.E + 1, T.M);
        timed("k_tcf_correlate", [&] {
            hipLaunchKernelGGL(k_tcf_correlate, dim3(tree.nChunk), dim3(kBlock), 0, stream_, B, T.nSpec, tree.nPad, tree.nChunkPad, nLive, T.cur, T.type, T.ring, T.partials);
        });
        timed("k_tcf_fold", [&] {
            hipLaunchKernelGGL(k_tcf_fold, dim3(nLive * 2 * T.nSpec), dim3(kBlock), 0, stream_, T.nSpec, tree.nChunkPad, c, T.E, T.M, T.partials, T.count, T.msdSum, T.vafSum);
        });
    });
    T.samples++;
}

void Samplers::tcf_shape(int& nLags, int& nSpec, long long& samples)
{
    const TcfState& T = tcf_state();
    nLags = T.n_lags(); nSpec = T.nSpec; samples = T.samples;
}

void Samplers::tcf_sums(int lag0, int n, std::vector<long long>* count, std::vector<double>* msd, std::vector<double>* vaf)
{
    const TcfState& T = tcf_state();
    if (lag0 < 0 || n < 0 || (long long)lag0 + n > T.n_lags()) throw ArgError("tcf: lag range outside [0, n_lags)");
    const size_t nv = (size_t)n * T.nSpec, at = (size_t)lag0 * T.nSpec;
    if (count) count->assign((size_t)n, 0);
    if (msd) msd->assign(nv, 0.0);
    if (vaf) vaf->assign(nv, 0.0);
    if (n == 0) return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    if (count) HIP_CHECK(hipMemcpy(count->data(), T.count + lag0, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (msd && nv) HIP_CHECK(hipMemcpy(msd->data(), T.msdSum + at, nv * 8, hipMemcpyDeviceToHost));
    if (vaf && nv) HIP_CHECK(hipMemcpy(vaf->data(), T.vafSum + at, nv * 8, hipMemcpyDeviceToHost));
}

// displ / number and vaf / number of the reference (out_md.cpp:120,577-579), over all pairs of a lag: sum / (count * n_s); 0 where count * n_s == 0
void Samplers::tcf_values(int lag0, int n, std::vector<double>& msd, std::vector<double>& vaf)
{
    std::vector<long long> count;
    tcf_sums(lag0, n, &count, &msd, &vaf);
    const int nSpec = tcf_.nSpec;
    for (int l = 0; l < n; l++)
        for (int s = 0; s < nSpec; s++)
        {
            const long long w = count[l] * (long long)model_.species[s].number;
            const size_t e = (size_t)l * nSpec + s;
            msd[e] = w ? msd[e] / (double)w : 0.0;
            vaf[e] = w ? vaf[e] / (double)w : 0.0;
        }
}

// ---------------------------------------------------------------------------------------------------
// Pressure tensor of the pair terms (stress.hip.h; pair set, terms and the order of the sums are stated in include/aztot.h)
// ---------------------------------------------------------------------------------------------------
void Samplers::stress_setup()
{
    // what the sampler cannot see makes the tensor wrong rather than incomplete: refused ("out of scope" -> AZTOT_ERR_INPUT), no sampler, the handle steps on
    need_one_gpu("pressure tensors");
    if (!model_.bondA.empty() || !model_.angC.empty()) throw std::runtime_error("out of scope: stress: the virial of bonds and angles is not built (the model has bonded terms)");
    if (model_.elec_type == AZTOT_ELEC_EWALD) throw std::runtime_error("out of scope: stress: the reciprocal-space virial of 'elec pme' is not built");
    if (model_.elec_type == AZTOT_ELEC_SPME) throw std::runtime_error("out of scope: stress: the reciprocal-space virial of 'elec spme' is not built");
    StressState T;
    const int N = model_.nAt;
    T.isSetUp = true;
    T.sliceShift = lanes_shift();
    T.tree = IdTree(N);
    set_up(stress_, T, [&] {
        const double biggest = std::max(box_.L[0], std::max(box_.L[1], box_.L[2]));
        canon_setup(T, model_.rMax > 0.0 ? model_.rMax : biggest);
        const size_t n = (size_t)std::max(N, 1), nPad = T.tree.nPad;
        T.rad = T.mem.alloc<double>(n, true, stream_);
        T.cols = T.mem.alloc<double>((size_t)SC_COUNT * nPad, true, stream_);
        T.visits = T.mem.alloc<int32_t>(nPad, true, stream_); T.drops = T.mem.alloc<int32_t>(nPad, true, stream_);
        T.partials = T.mem.alloc<double>((size_t)SC_COUNT * T.tree.nChunkPad, true, stream_);
        T.totals = T.mem.alloc<double>(SC_COUNT, true, stream_);
        T.counters = T.mem.alloc<unsigned long long>(2, true, stream_);
    });
}

void Samplers::stress_sample()
{
    StressState& T = stress_state(false);
    sample("stress kernels", [&](const AtomArrays& A) {
        const PairTables E = host_.pair_tables();
        const int N = model_.nAt;
        const IdTree& tree = T.tree;
        T.sampled = false;
        T.step = E.step;
        HIP_CHECK(hipMemsetAsync(T.counters, 0, 2 * sizeof(unsigned long long), stream_));
        if (N > 0)
        {
            static const char* const names[5] = {"k_stress_bin", "k_stress_scan", "k_stress_ids", "k_stress_rank", "k_stress_place"};
            grid_fill_canonical(T, A, names, false);     // (the slot -> id map is k_stress_gather's)
            timed("k_stress_gather", [&] {
                hipLaunchKernelGGL(k_stress_gather, dim3(div_up(N, kBlock)), dim3(kBlock), 0, stream_, E.S, A, N, (int)E.P.use_radii, tree.nPad, T.cellOf, T.canonRank,
                                   T.cellStart, T.slotId, T.rad, T.cols);
            });
            timed("k_stress_pairs", [&] {
                hipLaunchKernelGGL(k_stress_pairs, dim3(lane_blocks(T.sliceShift)), dim3(kBlock), 0, stream_, T.grid, E.P, E.S, E.pots, N, T.sliceShift, tree.nPad,
                                   T.cellStart, T.x, T.y, T.z, T.kind, T.rad, T.slotId, T.cols, T.visits, T.drops);
            });
        }
        timed("k_stress_chunks", [&] {
            hipLaunchKernelGGL(k_stress_chunks, dim3(tree.nChunk), dim3(kBlock), 0, stream_, tree.nPad, tree.nChunkPad, T.cols, T.visits, T.drops, T.partials, T.counters);
        });
        timed("k_stress_fold", [&] { hipLaunchKernelGGL(k_tree_fold, dim3(SC_COUNT), dim3(kBlock), 0, stream_, tree.nChunkPad, 0, T.partials, T.totals); });
    });
    T.sampled = true;
}

void Samplers::stress_get(aztot_stress& out)
{
    const StressState& T = stress_state(true);
    double tot[SC_COUNT];
    unsigned long long cnt[2];
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(tot, T.totals, sizeof(tot), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(cnt, T.counters, sizeof(cnt), hipMemcpyDeviceToHost));
    std::memset(&out, 0, sizeof(out));
    out.step = T.step;
    out.time = (double)T.step * model_.tSt;
    out.volume = box_.L[0] * box_.L[1] * box_.L[2];
    for (int c = 0; c < 6; c++)
    {
        out.virial[c] = tot[SC_WXX + c];
        out.kinetic[c] = tot[SC_KXX + c];
        out.pressure[c] = (out.kinetic[c] + out.virial[c]) / out.volume * units::pressure_factor;
    }
    out.pressure_iso = (out.pressure[0] + out.pressure[1] + out.pressure[2]) / 3.0;
    out.eng_vdw = tot[SC_EVDW]; out.eng_coul = tot[SC_ECOUL];
    out.pairs = (long long)(cnt[0] / 2); out.pairs_dropped = (long long)(cnt[1] / 2);      // every unordered pair is visited from both ends
}

void Samplers::stress_per_atom(std::vector<double>& w)
{
    const StressState& T = stress_state(true);
    const int N = model_.nAt;
    w.assign((size_t)N * 6, 0.0);
    if (N == 0) return;
    std::vector<double> col((size_t)N);
    HIP_CHECK(hipStreamSynchronize(stream_));
    for (int c = 0; c < 6; c++)
    {
        HIP_CHECK(hipMemcpy(col.data(), T.cols + (size_t)(SC_WXX + c) * T.tree.nPad, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
        for (int i = 0; i < N; i++) w[(size_t)i * 6 + c] = col[i];
    }
}

// ---------------------------------------------------------------------------------------------------
// Bond-angle distributions (adf.hip.h; columns, separation and the bin rule are stated in include/aztot.h)
// ---------------------------------------------------------------------------------------------------
Samplers::AdfState& Samplers::adf_state() { need_setup(adf_.nBins != 0, "adf"); return adf_; }

int Samplers::adf_setup(int nBins, const aztot_adf_column* cols, int nCols)
{
    need_one_gpu("bond-angle distributions");
    if (nBins < 1 || nBins > AZTOT_ADF_MAX_BINS) throw ArgError("adf: n_bins must be in [1, AZTOT_ADF_MAX_BINS]");
    if (!cols || nCols < 1 || nCols > AZTOT_ADF_MAX_COLUMNS) throw ArgError("adf: the number of columns must be in [1, AZTOT_ADF_MAX_COLUMNS]");
    const int nSpec = model_.nSpec();
    AdfState T;
    AdfTables tab;
    std::vector<int8_t> colOf(kSpecCap * kSpecCap * kSpecCap, (int8_t)-1);
    for (int g = 0; g < kSpecCap; g++) { tab.rowMax2[g] = -1.0; tab.ligMask[g] = 0; }
    for (int c = 0; c < kAdfMaxCols; c++) tab.ra2[c] = tab.rb2[c] = 0.0;
    double rBig = 0.0;
    for (int c = 0; c < nCols; c++)
    {
        aztot_adf_column col = cols[c];
        if (col.central < 0 || col.central >= nSpec || col.ligand_a < 0 || col.ligand_a >= nSpec || col.ligand_b < 0 || col.ligand_b >= nSpec)
            throw ArgError("adf: species index of a column out of range");
        if (col.reserved != 0) throw ArgError("adf: the reserved field of a column must be 0");
        if (!(col.radius_a > 0.0) || !(col.radius_b > 0.0) || !std::isfinite(col.radius_a) || !std::isfinite(col.radius_b))
            throw ArgError("adf: the radii of a column must be positive");
        if (col.ligand_a == col.ligand_b && col.radius_a != col.radius_b) throw ArgError("adf: equal ligand species need equal radii");
        if (col.ligand_a > col.ligand_b) { std::swap(col.ligand_a, col.ligand_b); std::swap(col.radius_a, col.radius_b); }
        int8_t& e = colOf[(col.central * kSpecCap + col.ligand_a) * kSpecCap + col.ligand_b];
        if (e >= 0) throw ArgError("adf: the same (central, {ligand_a, ligand_b}) names two columns");
        e = (int8_t)c;
        colOf[(col.central * kSpecCap + col.ligand_b) * kSpecCap + col.ligand_a] = (int8_t)c;
        tab.ra2[c] = col.radius_a * col.radius_a; tab.rb2[c] = col.radius_b * col.radius_b;
        tab.rowMax2[col.central] = std::max(tab.rowMax2[col.central], std::max(tab.ra2[c], tab.rb2[c]));
        tab.ligMask[col.central] |= (1 << col.ligand_a) | (1 << col.ligand_b);
        rBig = std::max(rBig, std::max(col.radius_a, col.radius_b));
        T.cols.push_back(col);
    }
    T.nBins = nBins;
    // T_b = c_b |c_b|, c_b = cos(pi b / n_bins) rounded to double; the exactly known values are forced.  cos(pi b / n) evaluated in double loses its
    // relative accuracy towards 90 degrees (the argument's rounding error is absolute); here it is the sine of the complementary angle in the middle half
    // and a cosine of the angle counted from the nearer end elsewhere, in long double: c_b is the nearest double or its neighbour, T_b within 2 ulp
    T.edges.resize((size_t)nBins + 1);
    for (int b = 0; b <= nBins; b++)
    {
        const long double pi = 3.141592653589793238462643383279502884L, n = (long double)nBins;
        const int k = nBins - 2 * b;
        const double cb = 2 * std::abs(k) <= nBins ? (double)sinl(pi * (long double)k / (2.0L * n))
                                                   : (k > 0 ? (double)cosl(pi * (long double)b / n) : (double)-cosl(pi * (long double)(nBins - b) / n));
        T.edges[b] = cb * std::fabs(cb);
    }
    T.edges[0] = 1.0; T.edges[nBins] = -1.0;
    if (nBins % 2 == 0) T.edges[nBins / 2] = 0.0;
    const int N = model_.nAt;
    T.sliceShift = lanes_shift();
    const size_t nEnt = (size_t)nBins * nCols;
    T.useLds = nEnt * sizeof(uint32_t) <= (size_t)kAdfHistBudget ? 1 : 0;
    set_up(adf_, T, [&] {
        grid_setup(T, rBig);
        const size_t n = (size_t)std::max(N, 1);
        T.slotId = T.mem.alloc<int32_t>(n, false, stream_); T.neigh = T.mem.alloc<int32_t>(n, false, stream_);
        T.summary = T.mem.alloc<unsigned long long>(1, true, stream_);
        T.totals = T.mem.alloc<unsigned long long>(nEnt, true, stream_);
        T.tables = T.mem.alloc<AdfTables>(1, false, stream_);
        T.colOf = T.mem.alloc<int8_t>(colOf.size(), false, stream_);
        T.dEdges = T.mem.alloc<double>(T.edges.size(), false, stream_);
        HIP_CHECK(hipMemcpy(T.tables, &tab, sizeof(tab), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(T.colOf, colOf.data(), colOf.size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(T.dEdges, T.edges.data(), T.edges.size() * sizeof(double), hipMemcpyHostToDevice));
    });
    return adf_.nBins;
}

void Samplers::adf_reset()
{
    AdfState& S = adf_state();
    HIP_CHECK(hipMemsetAsync(S.totals, 0, (size_t)S.nBins * S.cols.size() * 8, stream_));
    S.samples = 0;
    HIP_CHECK(hipStreamSynchronize(stream_));
}

void Samplers::adf_sample()
{
    AdfState& S = adf_state();
    sample("adf kernels", [&](const AtomArrays& A) {
        const int N = model_.nAt, nCols = (int)S.cols.size();
        if (N == 0) return;
        static const char* const names[3] = {"adf_bin", "adf_scan", "adf_place"};
        grid_fill(S, A, names);
        const int nb = div_up(N, kBlock);
        unsigned long long summary = 0;
        HIP_CHECK(hipMemsetAsync(S.summary, 0, sizeof(summary), stream_));
        S.counted = false;
        timed("adf_neigh", [&] {
            hipLaunchKernelGGL(k_grid_slot_ids, dim3(nb), dim3(kBlock), 0, stream_, A, N, S.cellOf, S.rankOf, S.cellStart, S.slotId);
            hipLaunchKernelGGL(k_adf_neigh, dim3(lane_blocks(S.sliceShift)), dim3(kBlock), 0, stream_, S.grid, S.tables, N, S.sliceShift, S.cellStart, S.x, S.y, S.z, S.kind,
                               S.slotId, S.neigh, S.summary);
        });
        HIP_CHECK(hipMemcpyAsync(&summary, S.summary, sizeof(summary), hipMemcpyDeviceToHost, stream_));
        host_.end_sample("adf neighbours");     // the tile and the lanes per atom are sized on the host from the counts just read back
        S.counted = true;
        const long long most = (long long)(summary >> 32);
        if (most > AZTOT_ADF_MAX_NEIGHBOURS)     // nothing has been added yet: totals and the sample count stay as they were, the engine is settled and drained
            throw std::runtime_error("adf: atom " + std::to_string((unsigned)(summary & 0xffffffffull)) + " has " + std::to_string(most) +
                                     " neighbours inside the largest radius of its columns, more than AZTOT_ADF_MAX_NEIGHBOURS = " +
                                     std::to_string(AZTOT_ADF_MAX_NEIGHBOURS) + ": nothing was added");
        if (most < 2) return;                    // no atom has a pair of neighbours
        // lanes per central atom (fitted to the sweep of tools/adf_cost.py): the fewest, from 4, with which the launch has 65536 lanes (lanes_shift(), kept in S.sliceShift) and the
        // histogram and the tiles of a workgroup (256 / lanes of them, each `cap` neighbours) stay inside kAdfLdsComfort, so that four workgroups share a CU;
        // more while they do not fit at all.  Every lane of an atom walks all 27 cells, so the gather's cost per atom grows with the lanes; the pairs do not care
        const int cap = (int)most;
        const size_t histBytes = S.useLds ? (size_t)S.nBins * nCols * sizeof(uint32_t) : 0;
        int laneShift = 2;
        // AZTOT_ADF_LANES = 4 / 8 / 16 / 32 / 64: a measurement switch (tools/adf_cost.py, tests) that replaces the rule (but for the room in LDS); the results do not depend on it
        int forced = 0;
        if (const char* e = std::getenv("AZTOT_ADF_LANES")) forced = std::atoi(e);
        if (forced == 4 || forced == 8 || forced == 16 || forced == 32 || forced == 64)
        {
            while ((1 << laneShift) < forced) laneShift++;
            while (laneShift < 6 && histBytes + (size_t)(kBlock >> laneShift) * cap * kAdfTileBytes > (size_t)kAdfLdsBudget) laneShift++;
        }
        else while (laneShift < 6 && (laneShift < S.sliceShift || histBytes + (size_t)(kBlock >> laneShift) * cap * kAdfTileBytes > (size_t)kAdfLdsComfort))
            laneShift++;
        const int groups = kBlock >> laneShift;
        const size_t lds = histBytes + (size_t)groups * cap * kAdfTileBytes;
        // a workgroup serves at most N / blocks + groups atoms between two flushes: the overflow bound stated at k_adf_triplets
        const int blocks = std::max(div_up(N, kAdfAtomsPerFlush), std::min(kAdfMaxBlocks, div_up(N, groups)));
        timed("adf_triplets", [&] {
            hipLaunchKernelGGL(k_adf_triplets, dim3(blocks), dim3(kBlock), lds, stream_, S.grid, S.tables, N, laneShift, cap, S.nBins, nCols, S.useLds, S.cellStart, S.x,
                               S.y, S.z, S.kind, S.colOf, S.dEdges, S.totals);
        });
    });
    S.samples++;
}

void Samplers::adf_shape(int& nBins, int& nCols, long long& samples)
{
    const AdfState& S = adf_state();
    nBins = S.nBins; nCols = (int)S.cols.size(); samples = S.samples;
}

void Samplers::adf_edges(std::vector<double>& T) { T = adf_state().edges; }

void Samplers::adf_counts(std::vector<unsigned long long>& counts)
{
    const AdfState& S = adf_state();
    counts.resize((size_t)S.nBins * S.cols.size());
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(counts.data(), S.totals, counts.size() * 8, hipMemcpyDeviceToHost));
}

// p[bin][column] = count / (column total * width in degrees): a density per degree that sums to 1 / width; 0 where the column is empty
void Samplers::adf_values(std::vector<double>& theta, std::vector<double>& p)
{
    std::vector<unsigned long long> c;
    adf_counts(c);
    const int nBins = adf_.nBins, nCols = (int)adf_.cols.size();
    const double width = 180.0 / (double)nBins;
    theta.resize(nBins);
    p.assign((size_t)nBins * nCols, 0.0);
    for (int b = 0; b < nBins; b++) theta[b] = (b + 0.5) * width;
    for (int k = 0; k < nCols; k++)
    {
        unsigned long long tot = 0;
        for (int b = 0; b < nBins; b++) tot += c[(size_t)b * nCols + k];
        if (!tot) continue;
        for (int b = 0; b < nBins; b++) p[(size_t)b * nCols + k] = (double)c[(size_t)b * nCols + k] / ((double)tot * width);
    }
}

void Samplers::adf_neighbours(std::vector<int32_t>& out)
{
    const AdfState& S = adf_state();
    if (!S.counted) throw ArgError("adf: aztot_adf_sample has not been called since the set-up");
    const int N = model_.nAt;
    out.assign((size_t)N, -1);
    if (N == 0) return;
    std::vector<int32_t> ids(N), cnt(N);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(ids.data(), S.slotId, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(cnt.data(), S.neigh, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    for (int s = 0; s < N; s++) out[ids[s]] = cnt[s];
}

// ---------------------------------------------------------------------------------------------------
// Static structure factors (sk.hip.h; the vector set, the order of the sums and the values are stated in include/aztot.h)
// ---------------------------------------------------------------------------------------------------
Samplers::SkState& Samplers::sk_state() { need_setup(sk_.nBins != 0, "sk"); return sk_; }

int Samplers::sk_setup(double kmax, double dk, int maxPerBin)
{
    need_one_gpu("static structure factors");
    if (!(kmax > 0.0) || !(dk > 0.0) || !std::isfinite(kmax) || !std::isfinite(dk)) throw ArgError("sk: kmax and dk must be positive");
    if (maxPerBin < 0) throw ArgError("sk: max_per_bin must not be negative (0: keep every vector)");
    const double idk = 1.0 / dk, nb = kmax * idk;
    if (!(nb >= 1.0) || !(nb < (double)AZTOT_SK_MAX_BINS + 1.0)) throw ArgError("sk: n_bins = kmax / dk must be in [1, AZTOT_SK_MAX_BINS]");
    SkState T;
    T.kmax = kmax; T.dk = dk; T.maxPerBin = maxPerBin; T.nBins = (int)nb;
    T.nSpec = model_.nSpec(); T.nPairs = T.nSpec * (T.nSpec + 1) / 2;
    // g = 2 pi / L with the correctly rounded double of 2 pi; sq[a][h] = (h g_a) * (h g_a)
    const double twoPi = 6.283185307179586, kmax2 = kmax * kmax;
    std::vector<double> sq[3];
    int hmax[3];
    for (int a = 0; a < 3; a++)
    {
        const double g = twoPi / box_.L[a];
        for (int h = 0; h <= AZTOT_SK_MAX_HARMONIC + 1; h++) { const double k = (double)h * g; sq[a].push_back(k * k); }
        if (sq[a][AZTOT_SK_MAX_HARMONIC + 1] <= kmax2)
            throw ArgError(std::string("sk: kmax needs harmonic ") + std::to_string(AZTOT_SK_MAX_HARMONIC + 1) + " on axis " + "xyz"[a] + ", more than AZTOT_SK_MAX_HARMONIC = " +
                           std::to_string(AZTOT_SK_MAX_HARMONIC) + ": this box admits kmax < " + std::to_string((double)(AZTOT_SK_MAX_HARMONIC + 1) * twoPi /
                           std::max(box_.L[0], std::max(box_.L[1], box_.L[2]))) + " (49 * 2 pi / its longest edge); nothing is truncated");
        hmax[a] = 0;
        while (hmax[a] < AZTOT_SK_MAX_HARMONIC && sq[a][hmax[a] + 1] <= kmax2) hmax[a]++;
    }
    // the half space in ascending lexicographic order of (l, m, n): l > 0, or l == 0 and m > 0, or l == m == 0 and n > 0
    std::vector<int32_t> lmn, bin;
    std::vector<int64_t> inBin((size_t)T.nBins, 0);
    for (int l = 0; l <= hmax[0]; l++)
        for (int m = (l > 0 ? -hmax[1] : 0); m <= hmax[1]; m++)
            for (int n = ((l > 0 || m > 0) ? -hmax[2] : 1); n <= hmax[2]; n++)
            {
                const double kk = (sq[0][l] + sq[1][std::abs(m)]) + sq[2][std::abs(n)];
                if (!(kk <= kmax2)) continue;
                const int b = (int)(std::sqrt(kk) * idk);
                if (b >= T.nBins) continue;
                lmn.push_back(l); lmn.push_back(m); lmn.push_back(n);
                bin.push_back(b);
                inBin[b]++;
            }
    // thinning: a bin with c > M vectors keeps j of 0 ... c - 1 iff (j + 1) M / c > j M / c (exactly M of them)
    std::vector<int64_t> seen((size_t)T.nBins, 0);
    T.nInBin.assign((size_t)T.nBins, 0);
    for (size_t v = 0; v < bin.size(); v++)
    {
        const int b = bin[v];
        const int64_t c = inBin[b], j = seen[b]++, M = maxPerBin;
        if (M > 0 && c > M && !((j + 1) * M / c > j * M / c)) continue;
        T.lmn.push_back(lmn[3 * v]); T.lmn.push_back(lmn[3 * v + 1]); T.lmn.push_back(lmn[3 * v + 2]);
        T.bin.push_back(b);
        T.nInBin[b]++;
        for (int a = 0; a < 3; a++) T.h[a] = std::max(T.h[a], std::abs(lmn[3 * v + a]) + 1);
    }
    T.nK = (int)T.bin.size();
    if (T.nK == 0) throw ArgError("sk: no k-vector (kmax is below the smallest 2 pi / L of the box, or its bin is past the last one)");
    const int N = model_.nAt, nH = T.h[0] + T.h[1] + T.h[2];
    T.tile = kSkIdTile;
    while (T.tile > 16 && (size_t)T.tile * nH * sizeof(cplx) > (size_t)kSkLdsBudget) T.tile >>= 1;
    T.nIdTiles = std::max(1, div_up(N, kSkIdTile));
    T.nRows = std::min(kSkRows, T.nIdTiles);
    // vectors per launch: `partial` stays inside its budget however large the set is
    const size_t perVector = (size_t)T.nRows * T.nSpec * 2 * sizeof(double);
    const size_t cap = std::max<size_t>(1, kSkPartialBudget / perVector / kSkChunk) * kSkChunk;
    T.batch = (int)std::min<size_t>(cap, (size_t)T.nK);
    set_up(sk_, T, [&] {
        const size_t nPad = (size_t)T.nIdTiles * kSkIdTile;
        T.x = T.mem.alloc<double>(nPad, true, stream_); T.y = T.mem.alloc<double>(nPad, true, stream_); T.z = T.mem.alloc<double>(nPad, true, stream_);
        T.type = T.mem.alloc<int32_t>(nPad, false, stream_);
        HIP_CHECK(hipMemsetAsync(T.type, 0xff, sizeof(int32_t) * nPad, stream_));
        T.dLmn = T.mem.alloc<int32_t>(T.lmn.size(), false, stream_);
        HIP_CHECK(hipMemcpy(T.dLmn, T.lmn.data(), T.lmn.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        T.partial = T.mem.alloc<double>((size_t)T.nRows * T.batch * T.nSpec * 2, false, stream_);
        T.rho = T.mem.alloc<double>((size_t)T.nK * T.nSpec * 2, true, stream_);
        T.acc = T.mem.alloc<double>((size_t)T.nK * T.nPairs, true, stream_);
    });
    return sk_.nK;
}

void Samplers::sk_reset()
{
    SkState& S = sk_state();
    HIP_CHECK(hipMemsetAsync(S.acc, 0, (size_t)S.nK * S.nPairs * sizeof(double), stream_));
    S.samples = 0;
    HIP_CHECK(hipStreamSynchronize(stream_));
}

void Samplers::sk_sample()
{
    SkState& S = sk_state();
    sample("sk kernels", [&](const AtomArrays& A) {
        const int N = model_.nAt;
        S.sampled = false;
        TcfBox B;
        SkGeom G;
        for (int k = 0; k < 3; k++) { B.L[k] = box_.L[k]; B.invL[k] = box_.invL[k]; B.half[k] = box_.half[k]; G.L[k] = box_.L[k]; G.h[k] = S.h[k]; }
        const int nH = S.h[0] + S.h[1] + S.h[2];
        // AZTOT_SK_TILE = 16 / 32 / 64 and AZTOT_SK_BATCH = vectors per launch: measurement switches (tools/sk_cost.py, tests) that replace the two rules
        // (within the room in LDS and in `partial`); the results do not depend on them
        int tile = S.tile, batch = S.batch;
        if (const char* e = std::getenv("AZTOT_SK_TILE"))
        {
            const int t = std::atoi(e);
            if ((t == 16 || t == 32 || t == 64) && (size_t)t * nH * sizeof(cplx) <= (size_t)kSkLdsBudget) tile = t;
        }
        if (const char* e = std::getenv("AZTOT_SK_BATCH"))
        {
            const int b = std::atoi(e);
            if (b >= 1 && b <= S.batch) batch = b;
        }
        if (N > 0)
            timed("k_sk_gather", [&] { hipLaunchKernelGGL(k_sk_gather, dim3(div_up(N, kBlock)), dim3(kBlock), 0, stream_, B, A, N, S.x, S.y, S.z, S.type); });
        const size_t rowStride = (size_t)S.batch * S.nSpec * 2, lds = (size_t)tile * nH * sizeof(cplx);
        for (int v0 = 0; v0 < S.nK; v0 += batch)
        {
            const int nvb = std::min(batch, S.nK - v0);
            timed("k_sk_amplitudes", [&] {
                hipLaunchKernelGGL(k_sk_amplitudes, dim3(div_up(nvb, kSkChunk), S.nRows), dim3(kBlock), lds, stream_, G, S.nSpec, tile, S.nIdTiles, nvb, rowStride,
                                   S.dLmn + 3 * (size_t)v0, S.x, S.y, S.z, S.type, S.partial);
            });
            const size_t nEnt = (size_t)nvb * S.nSpec * 2;
            timed("k_sk_fold", [&] {
                hipLaunchKernelGGL(k_sk_fold, dim3((unsigned)((nEnt + kWave - 1) / kWave)), dim3(kWave * kSkFoldWaves), 0, stream_, S.nRows, nEnt, rowStride, S.partial,
                                   S.rho + (size_t)v0 * S.nSpec * 2);
            });
        }
        const size_t nAcc = (size_t)S.nK * S.nPairs;
        timed("k_sk_accumulate", [&] {
            hipLaunchKernelGGL(k_sk_accumulate, dim3((unsigned)((nAcc + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream_, S.nK, S.nSpec, S.nPairs, S.rho, S.acc);
        });
    });
    S.samples++;
    S.sampled = true;
}

void Samplers::sk_shape(int& nVectors, int& nBins, int& nPairs, long long& samples)
{
    const SkState& S = sk_state();
    nVectors = S.nK; nBins = S.nBins; nPairs = S.nPairs; samples = S.samples;
}

void Samplers::sk_vectors(std::vector<int32_t>& lmn, std::vector<int32_t>& bin)
{
    const SkState& S = sk_state();
    lmn = S.lmn; bin = S.bin;
}

void Samplers::sk_amplitudes(std::vector<double>& rho)
{
    const SkState& S = sk_state();
    if (!S.sampled) throw ArgError("sk: aztot_sk_sample has not been called since the set-up");
    rho.resize((size_t)S.nK * S.nSpec * 2);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(rho.data(), S.rho, rho.size() * sizeof(double), hipMemcpyDeviceToHost));
}

void Samplers::sk_sums(std::vector<double>& acc)
{
    const SkState& S = sk_state();
    acc.resize((size_t)S.nK * S.nPairs);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(acc.data(), S.acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost));
}

// Ashcroft-Langreth partials per vector, S_ab = acc / (samples * sqrt(n_a n_b)), and the total S = sum_{a <= b} w_ab sqrt(n_a n_b) S_ab / N (pair order, from
// 0.0), each averaged over the kept vectors of its bin (summed in set order, from 0.0).  Every operation is rounded on its own: tests/sk_model.py values()
void Samplers::sk_values(std::vector<double>& k, std::vector<int32_t>& nInBin, std::vector<double>& sTotal, std::vector<double>& sPair)
{
#pragma clang fp contract(off)
    std::vector<double> acc;
    sk_sums(acc);
    const SkState& S = sk_;
    const int nP = S.nPairs, nS = S.nSpec;
    k.resize(S.nBins);
    for (int b = 0; b < S.nBins; b++) k[b] = (b + 0.5) * S.dk;
    nInBin = S.nInBin;
    sTotal.assign((size_t)S.nBins, 0.0);
    sPair.assign((size_t)S.nBins * nP, 0.0);
    std::vector<double> root(nP), weight(nP);
    {
        int p = 0;
        for (int a = 0; a < nS; a++)
            for (int b = a; b < nS; b++, p++)
            {
                root[p] = std::sqrt((double)model_.species[a].number * (double)model_.species[b].number);
                weight[p] = (a == b ? 1.0 : 2.0) * root[p];
            }
    }
    const double nAt = (double)model_.nAt;
    for (int v = 0; v < S.nK; v++)
    {
        const int b = S.bin[v];
        double tot = 0.0;
        for (int p = 0; p < nP; p++)
        {
            const double d = (double)S.samples * root[p];
            const double sab = d != 0.0 ? acc[(size_t)v * nP + p] / d : 0.0;
            sPair[(size_t)b * nP + p] = sPair[(size_t)b * nP + p] + sab;
            const double term = weight[p] * sab;
            tot = tot + term;
        }
        const double sv = nAt > 0.0 ? tot / nAt : 0.0;
        sTotal[b] = sTotal[b] + sv;
    }
    for (int b = 0; b < S.nBins; b++)
    {
        if (!S.nInBin[b]) continue;
        const double c = (double)S.nInBin[b];
        sTotal[b] = sTotal[b] / c;
        for (int p = 0; p < nP; p++) sPair[(size_t)b * nP + p] = sPair[(size_t)b * nP + p] / c;
    }
}

// ---------------------------------------------------------------------------------------------------
// Bond-orientational order (boo.hip.h; bonds, values, the order of the sums and the totals are stated in include/aztot.h)
// ---------------------------------------------------------------------------------------------------
Samplers::BooState& Samplers::boo_state(bool needSample)
{
    need_setup(boo_.nBins != 0, "boo");
    if (needSample && !boo_.sampled) throw ArgError("boo: aztot_boo_sample has not been called since the set-up");
    return boo_;
}

// N_lm = sqrt((2l + 1) / (4 pi) * (l - m)! / (l + m)!) and 4 pi / (2l + 1), made in long double and rounded once
static BooOrder boo_order_table(int l, int at, int stride)
{
    const long double pi = 3.141592653589793238462643383279502884L;
    BooOrder O{};
    for (int m = 0; m <= l; m++)
    {
        long double ratio = 1.0L;                       // (l - m)! / (l + m)!
        for (int k = l - m + 1; k <= l + m; k++) ratio /= (long double)k;
        O.norm[m] = (double)sqrtl((long double)(2 * l + 1) / (4.0L * pi) * ratio);
    }
    O.scale = (double)(4.0L * pi / (long double)(2 * l + 1));
    O.at = at; O.stride = stride;
    return O;
}

int Samplers::boo_setup(const aztot_boo_params& p)
{
    need_one_gpu("bond-orientational order parameters");
    const int nSpec = model_.nSpec();
    if (!(p.radius > 0.0) || !std::isfinite(p.radius)) throw ArgError("boo: the radius must be positive");
    if (p.reserved != 0) throw ArgError("boo: the reserved field must be 0");
    const unsigned all = nSpec >= 32 ? 0xffffffffu : ((1u << nSpec) - 1u);
    if (p.central_mask == 0 || p.ligand_mask == 0) throw ArgError("boo: central_mask and ligand_mask must not be empty");
    if (((unsigned)p.central_mask & ~all) || ((unsigned)p.ligand_mask & ~all)) throw ArgError("boo: a mask names a species at or above n_species");
    if (p.n_orders < 1 || p.n_orders > AZTOT_BOO_MAX_ORDERS) throw ArgError("boo: n_orders must be in [1, AZTOT_BOO_MAX_ORDERS]");
    for (int o = 0; o < p.n_orders; o++)
    {
        if (p.orders[o] < 1 || p.orders[o] > AZTOT_BOO_MAX_L) throw ArgError("boo: an order must be in [1, AZTOT_BOO_MAX_L]");
        for (int k = 0; k < o; k++)
            if (p.orders[k] == p.orders[o]) throw ArgError("boo: the same order is given twice");
    }
    if (p.n_bins < 1 || p.n_bins > AZTOT_BOO_MAX_BINS) throw ArgError("boo: n_bins must be in [1, AZTOT_BOO_MAX_BINS]");
    BooState T;
    T.par = p;
    for (int o = p.n_orders; o < AZTOT_BOO_MAX_ORDERS; o++) T.par.orders[o] = 0;
    T.nBins = p.n_bins; T.nSpec = nSpec;
    for (int o = 0; o < p.n_orders; o++) T.stride += 2 * (p.orders[o] + 1);
    const int N = model_.nAt;
    T.sliceShift = lanes_shift();
    T.tree = IdTree(N);
    T.nHist = (size_t)2 * p.n_orders * nSpec * p.n_bins;
    T.useLds = (T.nHist + nSpec) * sizeof(uint32_t) <= (size_t)kBooHistBudget ? 1 : 0;
    set_up(boo_, T, [&] {
        canon_setup(T, p.radius);
        const size_t n = (size_t)std::max(N, 1), nCols = (size_t)2 * p.n_orders, nPad = T.tree.nPad;
        T.nSlot = T.mem.alloc<int32_t>(n, true, stream_);
        T.qlm = T.mem.alloc<double>(n * (size_t)T.stride, true, stream_);
        T.nById = T.mem.alloc<int32_t>(nPad, true, stream_); T.typeById = T.mem.alloc<int32_t>(nPad, false, stream_);
        HIP_CHECK(hipMemsetAsync(T.typeById, 0xff, sizeof(int32_t) * nPad, stream_));
        T.qCols = T.mem.alloc<double>(nCols * nPad, true, stream_);
        T.partials = T.mem.alloc<double>(nCols * nSpec * (size_t)T.tree.nChunkPad, true, stream_);
        T.sums = T.mem.alloc<double>(nCols * nSpec, true, stream_);
        T.totals = T.mem.alloc<unsigned long long>(T.nHist + nSpec, true, stream_);
    });
    return boo_.nBins;
}

void Samplers::boo_reset()
{
    BooState& S = boo_state(false);
    HIP_CHECK(hipMemsetAsync(S.totals, 0, (S.nHist + S.nSpec) * 8, stream_));
    HIP_CHECK(hipMemsetAsync(S.sums, 0, (size_t)2 * S.par.n_orders * S.nSpec * 8, stream_));
    S.samples = 0;
    HIP_CHECK(hipStreamSynchronize(stream_));
}

// one kernel per order L = 1 ... 12: the accumulators are indexed at compile time only
template <typename F> static void boo_dispatch(int l, F&& go)
{
    switch (l)
    {
    case 1: go(std::integral_constant<int, 1>()); break;
    case 2: go(std::integral_constant<int, 2>()); break;
    case 3: go(std::integral_constant<int, 3>()); break;
    case 4: go(std::integral_constant<int, 4>()); break;
    case 5: go(std::integral_constant<int, 5>()); break;
    case 6: go(std::integral_constant<int, 6>()); break;
    case 7: go(std::integral_constant<int, 7>()); break;
    case 8: go(std::integral_constant<int, 8>()); break;
    case 9: go(std::integral_constant<int, 9>()); break;
    case 10: go(std::integral_constant<int, 10>()); break;
    case 11: go(std::integral_constant<int, 11>()); break;
    case 12: go(std::integral_constant<int, 12>()); break;
    default: throw std::logic_error("boo: order outside [1, 12]");
    }
}

void Samplers::boo_sample()
{
    BooState& S = boo_state(false);
    sample("boo kernels", [&](const AtomArrays& A) {
        const int N = model_.nAt, nO = S.par.n_orders, nCols = 2 * nO;
        S.sampled = false;
        if (N == 0) return;
        const IdTree& tree = S.tree;
        static const char* const names[5] = {"k_boo_bin", "k_boo_scan", "k_boo_ids", "k_boo_rank", "k_boo_place"};
        grid_fill_canonical(S, A, names, true);
        BooParams P;
        P.r2 = S.par.radius * S.par.radius; P.centralMask = S.par.central_mask; P.ligandMask = S.par.ligand_mask;
        const int blocks = lane_blocks(S.sliceShift);
        BooOrder tab[AZTOT_BOO_MAX_ORDERS];
        for (int o = 0, at = 0; o < nO; at += 2 * (S.par.orders[o] + 1), o++) tab[o] = boo_order_table(S.par.orders[o], at, S.stride);
        timed("k_boo_qlm", [&] {
            for (int o = 0; o < nO; o++)
                boo_dispatch(S.par.orders[o], [&](auto l) {
                    hipLaunchKernelGGL(k_boo_qlm<decltype(l)::value>, dim3(blocks), dim3(kBlock), 0, stream_, S.grid, P, tab[o], N, S.sliceShift, S.cellStart, S.x, S.y,
                                       S.z, S.kind, S.nSlot, S.qlm);
                });
        });
        timed("k_boo_average", [&] {
            for (int o = 0; o < nO; o++)
                boo_dispatch(S.par.orders[o], [&](auto l) {
                    hipLaunchKernelGGL(k_boo_average<decltype(l)::value>, dim3(blocks), dim3(kBlock), 0, stream_, S.grid, P, tab[o], N, S.sliceShift, o, nO, tree.nPad,
                                       S.cellStart, S.x, S.y, S.z, S.kind, S.slotId, S.nSlot, S.qlm, S.qCols, S.nById, S.typeById);
                });
        });
        const int gs = std::max(1, std::min(kBooMaxBlocks, div_up(N, kBlock)));
        timed("k_boo_hist", [&] {
            hipLaunchKernelGGL(k_boo_hist, dim3(gs), dim3(kBlock), S.useLds ? (S.nHist + S.nSpec) * sizeof(uint32_t) : 0, stream_, N, nO, S.nSpec, S.nBins, tree.nPad,
                               S.useLds, S.qCols, S.nById, S.typeById, S.totals);
        });
        timed("k_boo_chunks", [&] {
            hipLaunchKernelGGL(k_boo_chunks, dim3(tree.nChunk), dim3(kBlock), 0, stream_, nCols, S.nSpec, tree.nPad, tree.nChunkPad, S.qCols, S.typeById, S.partials);
        });
        timed("k_boo_fold", [&] { hipLaunchKernelGGL(k_tree_fold, dim3(nCols * S.nSpec), dim3(kBlock), 0, stream_, tree.nChunkPad, 1, S.partials, S.sums); });
    });
    S.sampled = true;
    S.samples++;
}

void Samplers::boo_shape(int& nOrders, int& nBins, int& nSpec, long long& samples, int* orders)
{
    const BooState& S = boo_state(false);
    nOrders = S.par.n_orders; nBins = S.nBins; nSpec = S.nSpec; samples = S.samples;
    if (orders) for (int o = 0; o < AZTOT_BOO_MAX_ORDERS; o++) orders[o] = S.par.orders[o];
}

void Samplers::boo_per_atom(std::vector<int32_t>& n, std::vector<double>& q)
{
    const BooState& S = boo_state(true);
    const int N = model_.nAt, nO = S.par.n_orders;
    n.assign((size_t)N, -1);
    q.assign((size_t)N * nO * 2, 0.0);
    if (N == 0) return;
    std::vector<double> col((size_t)N);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(n.data(), S.nById, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    for (int kind = 0; kind < 2; kind++)
        for (int o = 0; o < nO; o++)
        {
            HIP_CHECK(hipMemcpy(col.data(), S.qCols + (size_t)(kind * nO + o) * S.tree.nPad, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
            for (int i = 0; i < N; i++) q[((size_t)i * nO + o) * 2 + kind] = col[i];
        }
}

void Samplers::boo_qlm(std::vector<double>& out)
{
    const BooState& S = boo_state(true);
    const int N = model_.nAt, nO = S.par.n_orders, M = 2 * (AZTOT_BOO_MAX_L + 1);
    out.assign((size_t)N * nO * M, 0.0);
    if (N == 0) return;
    std::vector<int32_t> ids(N);
    std::vector<double> q((size_t)N * S.stride);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(ids.data(), S.slotId, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(q.data(), S.qlm, sizeof(double) * q.size(), hipMemcpyDeviceToHost));
    for (int s = 0; s < N; s++)
    {
        if ((unsigned)ids[s] >= (unsigned)N) continue;
        for (int o = 0, at = 0; o < nO; at += 2 * (S.par.orders[o] + 1), o++)
            for (int k = 0; k < 2 * (S.par.orders[o] + 1); k++) out[((size_t)ids[s] * nO + o) * M + k] = q[(size_t)s * S.stride + at + k];
    }
}

void Samplers::boo_counts(std::vector<unsigned long long>& hist, std::vector<double>& sums, std::vector<unsigned long long>& entered)
{
    const BooState& S = boo_state(false);
    std::vector<unsigned long long> all(S.nHist + S.nSpec);
    sums.resize((size_t)2 * S.par.n_orders * S.nSpec);
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(all.data(), S.totals, all.size() * 8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(sums.data(), S.sums, sums.size() * 8, hipMemcpyDeviceToHost));
    hist.assign(all.begin(), all.begin() + S.nHist);
    entered.assign(all.begin() + S.nHist, all.end());
}

// density[column][bin] = count / (column total * width), width = 1 / n_bins, 0 where the column is empty; mean = sum / entered, 0 where nothing entered
void Samplers::boo_values(std::vector<double>& centre, std::vector<double>& density, std::vector<double>& mean)
{
    std::vector<unsigned long long> hist, entered;
    std::vector<double> sums;
    boo_counts(hist, sums, entered);
    const int nBins = boo_.nBins, nSpec = boo_.nSpec, nCols = 2 * boo_.par.n_orders * nSpec;
    const double width = 1.0 / (double)nBins;
    centre.resize(nBins);
    for (int b = 0; b < nBins; b++) centre[b] = (b + 0.5) / (double)nBins;
    density.assign(hist.size(), 0.0);
    mean.assign(sums.size(), 0.0);
    for (int c = 0; c < nCols; c++)
    {
        unsigned long long tot = 0;
        for (int b = 0; b < nBins; b++) tot += hist[(size_t)c * nBins + b];
        if (tot)
            for (int b = 0; b < nBins; b++) density[(size_t)c * nBins + b] = (double)hist[(size_t)c * nBins + b] / ((double)tot * width);
        const unsigned long long e = entered[c % nSpec];
        if (e) mean[c] = sums[c] / (double)e;
    }
}

}  // namespace aztot
