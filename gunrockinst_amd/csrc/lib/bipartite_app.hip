// lib/bipartite_app.hip -- maximum-bipartite-matching entry points of libgunrock.so.
//  * grx_bipartite_*: BipartiteProblem / BipartiteEnactor phases as separate C calls (the reference snapshot has no bipartite
//    matching; the calls are shaped like grx_spgemm_* for the operand and like grx_wl_* for the run).
#include <gunrock/gunrock_mi355x.h>

#include <gunrock/app/bipartite/bipartite_enactor.hpp>
#include <gunrock/app/bipartite/bipartite_problem.hpp>
#include <gunrock/app/handle_runner.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::bipartite;

static_assert(GRX_BIPARTITE_AUTO == BIPARTITE_AUTO && GRX_BIPARTITE_LANE == BIPARTITE_LANE && GRX_BIPARTITE_WAVE == BIPARTITE_WAVE &&
                  GRX_BIPARTITE_BLOCK == BIPARTITE_BLOCK,
              "the header's strategies are the kernels' strategies");
static_assert(GRX_BIPARTITE_HORIZONTAL == BIPARTITE_HORIZONTAL && GRX_BIPARTITE_SQUARE == BIPARTITE_SQUARE && GRX_BIPARTITE_VERTICAL == BIPARTITE_VERTICAL,
              "the header's parts are the kernels' parts");
static_assert(GRX_BIPARTITE_MAXIMUM == BIPARTITE_MAXIMUM && GRX_BIPARTITE_CAPPED == BIPARTITE_CAPPED, "the header's states are the enactor's");
static_assert(GRX_BIPARTITE_NOT_CERTIFIED == kNotCertified && GRX_BIPARTITE_BAD_MATCHING == kBadMatching && GRX_BIPARTITE_NOT_MAXIMUM == kNotMaximum,
              "the header's codes are the enactor's");

namespace {

struct BipartiteStats {
    long long ints[7] = {0, 0, 0, 0, 0, 0, 0};  // size, phases, levels, vertical levels, augmentations, greedy pairs, state
    long long certificate[3] = {0, 0, 0}, regime[3] = {0, 0, 0}, loop_levels = 0, launches = 0, readbacks = 0;
    double kernel_ms[1 + MS_COUNT] = {0, 0, 0, 0, 0, 0}, build_ms = 0;
};

struct BipartiteRunner {
    InitState state;
    virtual ~BipartiteRunner() {}
    virtual int Init(int rows, int cols, int nnz, const int *ro, const int *ci, bool on_device) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual int Reset(const int *mate_row) = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(BipartiteStats &s) = 0;
    virtual int PhaseTrace(int max_phases, int *levels, long long *augmentations, double *ms) = 0;
    virtual int ExtractMatching(int *mate_row, int *mate_col, long long *size) = 0;
    virtual int ExtractParts(int *row_part, int *col_part, long long *part_sizes) = 0;
    virtual int ExtractCover(unsigned char *row_cover, unsigned char *col_cover) = 0;
    virtual int SquareGraph(int *k, int *arcs, int **d_ro, int **d_ci, int **d_rows) = 0;
    virtual void DeviceResults(void **out) = 0;
};

template <bool INSTR>
struct BipartiteRunnerT : BipartiteRunner {
    BipartiteProblem problem;
    BipartiteEnactor<INSTR> enactor;
    EventPair timer;
    explicit BipartiteRunnerT(int device)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(int rows, int cols, int nnz, const int *ro, const int *ci, bool on_device) override
    {
        const hipError_t rc = on_device ? problem.InitFromDevice(rows, cols, nnz, const_cast<int *>(ro), const_cast<int *>(ci)) : problem.Init(rows, cols, nnz, ro, ci);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int SetOption(const char *name, double value) override { return enactor.options.Set(name, value); }
    // a result of either end state / of BIPARTITE_MAXIMUM: 0, or the code that refuses
    int Done() const { return state.ready && problem.state >= 0 ? 0 : static_cast<int>(hipErrorNotReady); }
    int Maximum() const { return Done() ? Done() : (problem.state == BIPARTITE_MAXIMUM ? 0 : kNotMaximum); }
    int Reset(const int *mate_row) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        const hipError_t rc = problem.Reset(mate_row);
        if (rc) return static_cast<int>(rc);
        return problem.bad_matching ? kBadMatching : 0;
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        const hipError_t rc = timer.Timed(problem.stream, ms, [&]() { return enactor.Enact(&problem, max_grid_size); });
        return rc ? static_cast<int>(rc) : enactor.code;
    }
    void Stats(BipartiteStats &s) override
    {
        const long long ints[7] = {enactor.size, enactor.phases, enactor.levels, enactor.vertical_levels, enactor.augmentations, enactor.greedy_pairs, enactor.state};
        for (int i = 0; i < 7; ++i) s.ints[i] = ints[i];
        for (int i = 0; i < 3; ++i) {
            s.certificate[i] = enactor.certificate[i];
            s.regime[i] = enactor.regime[i];
        }
        s.loop_levels = enactor.loop_levels;
        s.launches = enactor.step.launches;
        s.readbacks = enactor.step.readbacks;
        s.kernel_ms[0] = enactor.step.kernel_ms;
        for (int i = 0; i < MS_COUNT; ++i) s.kernel_ms[1 + i] = enactor.kind_ms[i];
        s.build_ms = problem.build_ms;
    }
    int PhaseTrace(int max_phases, int *levels, long long *augmentations, double *ms) override
    {
        return CopyTrace(enactor.trace_levels.size(), max_phases, Column(levels, [&](int i) { return enactor.trace_levels[i]; }),
                         Column(augmentations, [&](int i) { return enactor.trace_aug[i]; }), Column(ms, [&](int i) { return enactor.trace_ms[i]; }));
    }
    int ExtractMatching(int *mate_row, int *mate_col, long long *size) override
    {
        if (int refused = Done()) return refused;
        if (size) *size = problem.size;
        if (hipError_t rc = problem.Read(mate_row, problem.d_mate_row.p, static_cast<size_t>(problem.rows))) return static_cast<int>(rc);
        return static_cast<int>(problem.Read(mate_col, problem.d_mate_col.p, static_cast<size_t>(problem.cols)));
    }
    int ExtractParts(int *row_part, int *col_part, long long *part_sizes) override
    {
        if (int refused = Maximum()) return refused;
        if (part_sizes)
            for (int i = 0; i < 6; ++i) part_sizes[i] = problem.part_size[i];
        if (hipError_t rc = problem.Read(row_part, problem.d_row_part.p, static_cast<size_t>(problem.rows))) return static_cast<int>(rc);
        return static_cast<int>(problem.Read(col_part, problem.d_col_part.p, static_cast<size_t>(problem.cols)));
    }
    int ExtractCover(unsigned char *row_cover, unsigned char *col_cover) override
    {
        if (int refused = Maximum()) return refused;
        if (hipError_t rc = problem.Read(row_cover, problem.d_row_cover.p, static_cast<size_t>(problem.rows))) return static_cast<int>(rc);
        return static_cast<int>(problem.Read(col_cover, problem.d_col_cover.p, static_cast<size_t>(problem.cols)));
    }
    int SquareGraph(int *k, int *arcs, int **d_ro, int **d_ci, int **d_rows) override
    {
        if (int refused = Maximum()) return refused;
        if (hipError_t rc = problem.SquareGraph()) return static_cast<int>(rc);
        if (k) *k = problem.square_k;
        if (arcs) *arcs = problem.square_arcs;
        if (d_ro) *d_ro = problem.sq_ro.p;
        if (d_ci) *d_ci = problem.square_arcs > 0 ? problem.sq_ci.p : nullptr;
        if (d_rows) *d_rows = problem.square_k > 0 ? problem.sq_map.p : nullptr;
        return 0;
    }
    void DeviceResults(void **out) override
    {
        const bool done = Done() == 0, maximum = Maximum() == 0;
        out[0] = done ? problem.d_mate_row.p : nullptr;
        out[1] = done ? problem.d_mate_col.p : nullptr;
        out[2] = maximum ? problem.d_row_part.p : nullptr;
        out[3] = maximum ? problem.d_col_part.p : nullptr;
        out[4] = maximum ? problem.d_row_cover.p : nullptr;
        out[5] = maximum ? problem.d_col_cover.p : nullptr;
    }
};

bool BadShape(int rows, int cols, int nnz, const int *ro, const int *ci) { return rows < 0 || cols < 0 || nnz < 0 || !ro || (nnz > 0 && !ci); }

}  // namespace

struct grx_bipartite {
    std::unique_ptr<BipartiteRunner> runner;
};

extern "C" {

int grx_bipartite_create(grx_bipartite **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_bipartite{MakeRunner<BipartiteRunner, BipartiteRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_bipartite_init(grx_bipartite *p, int rows, int cols, int entries, const int *row_offsets, const int *col_indices)
{
    if (!p || BadShape(rows, cols, entries, row_offsets, col_indices)) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->Init(rows, cols, entries, row_offsets, col_indices, false);
}

int grx_bipartite_init_device(grx_bipartite *p, int rows, int cols, int entries, int *d_row_offsets, int *d_col_indices)
{
    if (!p || BadShape(rows, cols, entries, d_row_offsets, d_col_indices)) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->Init(rows, cols, entries, d_row_offsets, d_col_indices, true);
}

int grx_bipartite_set_option(grx_bipartite *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_bipartite_reset(grx_bipartite *p, const int *mate_row) { return p ? p->runner->Reset(mate_row) : -1; }

int grx_bipartite_enact(grx_bipartite *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_bipartite_stats(grx_bipartite *p, long long *size, long long *phases, long long *levels, long long *vertical_levels, long long *augmentations,
                        long long *greedy_pairs, long long *state, long long *certificate, long long *regime_columns, long long *loop_levels,
                        long long *kernel_launches, long long *readbacks, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    BipartiteStats s;
    p->runner->Stats(s);
    long long *ints[7] = {size, phases, levels, vertical_levels, augmentations, greedy_pairs, state};
    for (int i = 0; i < 7; ++i)
        if (ints[i]) *ints[i] = s.ints[i];
    for (int i = 0; i < 3; ++i) {
        if (certificate) certificate[i] = s.certificate[i];
        if (regime_columns) regime_columns[i] = s.regime[i];
    }
    if (loop_levels) *loop_levels = s.loop_levels;
    if (kernel_launches) *kernel_launches = s.launches;
    if (readbacks) *readbacks = s.readbacks;
    if (kernel_ms)
        for (int i = 0; i < 1 + MS_COUNT; ++i) kernel_ms[i] = s.kernel_ms[i];
    if (build_ms) *build_ms = s.build_ms;
    return 0;
}

int grx_bipartite_phase_trace(grx_bipartite *p, int max_phases, int *levels, long long *augmentations, double *ms)
{
    if (!p) return -1;
    return p->runner->PhaseTrace(max_phases, levels, augmentations, ms);
}

int grx_bipartite_extract_matching(grx_bipartite *p, int *h_mate_row, int *h_mate_col, long long *size)
{
    if (!p) return -1;
    return p->runner->ExtractMatching(h_mate_row, h_mate_col, size);
}

int grx_bipartite_extract_parts(grx_bipartite *p, int *h_row_part, int *h_col_part, long long *part_sizes)
{
    if (!p) return -1;
    return p->runner->ExtractParts(h_row_part, h_col_part, part_sizes);
}

int grx_bipartite_extract_cover(grx_bipartite *p, unsigned char *h_row_cover, unsigned char *h_col_cover)
{
    if (!p) return -1;
    return p->runner->ExtractCover(h_row_cover, h_col_cover);
}

int grx_bipartite_square_graph(grx_bipartite *p, int *k, int *arcs, int **d_row_offsets, int **d_col_indices, int **d_rows)
{
    if (!p) return -1;
    return p->runner->SquareGraph(k, arcs, d_row_offsets, d_col_indices, d_rows);
}

int grx_bipartite_device_results(grx_bipartite *p, int **d_mate_row, int **d_mate_col, int **d_row_part, int **d_col_part, unsigned char **d_row_cover,
                                 unsigned char **d_col_cover)
{
    if (!p) return -1;
    void *out[6];
    p->runner->DeviceResults(out);
    if (d_mate_row) *d_mate_row = static_cast<int *>(out[0]);
    if (d_mate_col) *d_mate_col = static_cast<int *>(out[1]);
    if (d_row_part) *d_row_part = static_cast<int *>(out[2]);
    if (d_col_part) *d_col_part = static_cast<int *>(out[3]);
    if (d_row_cover) *d_row_cover = static_cast<unsigned char *>(out[4]);
    if (d_col_cover) *d_col_cover = static_cast<unsigned char *>(out[5]);
    return 0;
}

void grx_bipartite_destroy(grx_bipartite *p) { delete p; }

}  // extern "C"
