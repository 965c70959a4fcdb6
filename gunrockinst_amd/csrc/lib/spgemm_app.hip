// lib/spgemm_app.hip -- sparse-product entry points of libgunrock.so.
//  * grx_spgemm_*: SpgemmProblem / SpgemmEnactor phases as separate C calls (the reference snapshot has no SpGEMM; the calls are shaped
//    like grx_sim_*).  One Enact per result; set_right / set_right_device hand over a right operand of its own.
#include <gunrock/gunrock_mi355x.h>

#include <gunrock/app/spgemm/spgemm_enactor.hpp>
#include <gunrock/app/spgemm/spgemm_problem.hpp>
#include <gunrock/app/handle_runner.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::spgemm;

static_assert(GRX_SPGEMM_AUTO == SPGEMM_AUTO && GRX_SPGEMM_LANE == SPGEMM_LANE && GRX_SPGEMM_WAVE == SPGEMM_WAVE && GRX_SPGEMM_BLOCK == SPGEMM_BLOCK &&
                  GRX_SPGEMM_GLOBAL == SPGEMM_GLOBAL,
              "the header's strategies are the kernels' strategies");
static_assert(GRX_SPGEMM_SELF == SPGEMM_SELF && GRX_SPGEMM_TRANSPOSE == SPGEMM_TRANSPOSE && GRX_SPGEMM_GIVEN == SPGEMM_GIVEN,
              "the header's right operands are the enactor's");
static_assert(GRX_SPGEMM_TOO_LARGE == kSpgemmTooLarge && GRX_SPGEMM_OVERFLOW == kSpgemmOverflow, "the header's refusals are the enactor's");

namespace {

struct SpgemmStats {
    long long rows[4] = {0, 0, 0, 0}, regime_products[4] = {0, 0, 0, 0}, products = 0, nnz = 0, probes = 0, launches = 0, readbacks = 0;
    double bound = 0, kernel_ms = 0, regime_ms[4] = {0, 0, 0, 0};
};

struct SpgemmRunner {
    InitState state;
    virtual ~SpgemmRunner() {}
    virtual int Init(int rows, int inner, int nnz, const int *ro, const int *ci, const int *val, bool on_device) = 0;
    virtual int SetRight(int rows, int cols, int nnz, const int *ro, const int *ci, const int *val, bool on_device) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(SpgemmStats &s) = 0;
    virtual int Sizes(int *rows, int *cols, long long *nnz) = 0;
    virtual int Extract(int *offsets, int *cols, long long *vals) = 0;
    virtual void DeviceResults(int **offsets, int **cols, long long **vals) = 0;
};

template <bool INSTR>
struct SpgemmRunnerT : SpgemmRunner {
    SpgemmProblem problem;
    SpgemmEnactor<INSTR> enactor;
    EventPair timer;
    explicit SpgemmRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(int rows, int inner, int nnz, const int *ro, const int *ci, const int *val, bool on_device) override
    {
        const hipError_t rc = on_device ? problem.InitFromDevice(rows, inner, nnz, const_cast<int *>(ro), const_cast<int *>(ci), const_cast<int *>(val))
                                        : problem.Init(rows, inner, nnz, ro, ci, val);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int SetRight(int rows, int cols, int nnz, const int *ro, const int *ci, const int *val, bool on_device) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        if (rows != problem.a.cols) return -1;
        const hipError_t rc = problem.SetRight(rows, cols, nnz, ro, ci, val, on_device);
        if (rc) return problem.malformed ? kMalformedGraph : static_cast<int>(rc);
        enactor.options.right = SPGEMM_GIVEN;
        return 0;
    }
    int SetOption(const char *name, double value) override { return enactor.options.Set(name, value); }
    hipError_t Reset() override
    {
        if (!state.ready) return hipErrorNotReady;
        return problem.Reset();
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        const hipError_t rc = timer.Timed(problem.stream, ms, [&]() { return enactor.template Enact<SpgemmProblem>(&problem, max_grid_size); });
        if (rc) return static_cast<int>(rc);
        if (enactor.bad_shape) return -1;
        if (enactor.too_large) return kSpgemmTooLarge;
        return enactor.overflow ? kSpgemmOverflow : 0;
    }
    void Stats(SpgemmStats &s) override
    {
        for (int i = 0; i < 4; ++i) {
            s.rows[i] = enactor.regime_rows[i];
            s.regime_products[i] = enactor.regime_products[i];
            s.regime_ms[i] = enactor.regime_ms[i];
        }
        s.products = enactor.products;
        s.nnz = enactor.nnz;
        s.probes = enactor.probes;
        s.launches = enactor.host.launches;
        s.readbacks = enactor.host.readbacks;
        s.bound = enactor.bound;
        s.kernel_ms = enactor.host.kernel_ms;
    }
    int Sizes(int *rows, int *cols, long long *nnz) override
    {
        if (!state.ready || problem.nnz < 0) return static_cast<int>(hipErrorNotReady);
        if (rows) *rows = problem.a.rows;
        if (cols) *cols = problem.result_cols;
        if (nnz) *nnz = problem.nnz;
        return 0;
    }
    int Extract(int *offsets, int *cols, long long *vals) override
    {
        if (!state.ready || problem.nnz < 0) return static_cast<int>(hipErrorNotReady);
        if (vals && !problem.with_values) return -1;
        return static_cast<int>(problem.Extract(offsets, cols, vals));
    }
    void DeviceResults(int **offsets, int **cols, long long **vals) override
    {
        const bool there = state.ready && problem.nnz >= 0;
        if (offsets) *offsets = there ? problem.offsets.p : nullptr;
        if (cols) *cols = there && problem.nnz > 0 ? problem.cols.p : nullptr;
        if (vals) *vals = there && problem.nnz > 0 && problem.with_values ? problem.vals.p : nullptr;
    }
};

bool BadShape(int rows, int cols, int nnz, const int *ro, const int *ci) { return rows < 0 || cols < 0 || nnz < 0 || !ro || (nnz > 0 && !ci); }

}  // namespace

struct grx_spgemm {
    std::unique_ptr<SpgemmRunner> runner;
};

extern "C" {

int grx_spgemm_create(grx_spgemm **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_spgemm{MakeRunner<SpgemmRunner, SpgemmRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_spgemm_init(grx_spgemm *p, int rows, int inner, int nnz, const int *offsets, const int *cols, const int *vals)
{
    if (!p || BadShape(rows, inner, nnz, offsets, cols)) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->Init(rows, inner, nnz, offsets, cols, vals, false);
}

int grx_spgemm_init_device(grx_spgemm *p, int rows, int inner, int nnz, int *d_offsets, int *d_cols, int *d_vals)
{
    if (!p || BadShape(rows, inner, nnz, d_offsets, d_cols)) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->Init(rows, inner, nnz, d_offsets, d_cols, d_vals, true);
}

int grx_spgemm_set_right(grx_spgemm *p, int rows, int cols, int nnz, const int *offsets, const int *col_indices, const int *vals)
{
    if (!p || BadShape(rows, cols, nnz, offsets, col_indices)) return -1;
    return p->runner->SetRight(rows, cols, nnz, offsets, col_indices, vals, false);
}

int grx_spgemm_set_right_device(grx_spgemm *p, int rows, int cols, int nnz, int *d_offsets, int *d_col_indices, int *d_vals)
{
    if (!p || BadShape(rows, cols, nnz, d_offsets, d_col_indices)) return -1;
    return p->runner->SetRight(rows, cols, nnz, d_offsets, d_col_indices, d_vals, true);
}

int grx_spgemm_set_option(grx_spgemm *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_spgemm_reset(grx_spgemm *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_spgemm_enact(grx_spgemm *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_spgemm_stats(grx_spgemm *p, long long *regime_rows, long long *regime_products, long long *products, long long *nnz, long long *table_probes,
                     long long *kernel_launches, long long *readbacks, double *bound, double *kernel_ms, double *regime_ms)
{
    if (!p) return -1;
    SpgemmStats s;
    p->runner->Stats(s);
    for (int i = 0; i < 4; ++i) {
        if (regime_rows) regime_rows[i] = s.rows[i];
        if (regime_products) regime_products[i] = s.regime_products[i];
        if (regime_ms) regime_ms[i] = s.regime_ms[i];
    }
    if (products) *products = s.products;
    if (nnz) *nnz = s.nnz;
    if (table_probes) *table_probes = s.probes;
    if (kernel_launches) *kernel_launches = s.launches;
    if (readbacks) *readbacks = s.readbacks;
    if (bound) *bound = s.bound;
    if (kernel_ms) *kernel_ms = s.kernel_ms;
    return 0;
}

int grx_spgemm_sizes(grx_spgemm *p, int *rows, int *cols, long long *nnz)
{
    if (!p) return -1;
    return p->runner->Sizes(rows, cols, nnz);
}

int grx_spgemm_extract(grx_spgemm *p, int *h_offsets, int *h_cols, long long *h_vals)
{
    if (!p) return -1;
    return p->runner->Extract(h_offsets, h_cols, h_vals);
}

int grx_spgemm_device_results(grx_spgemm *p, int **d_offsets, int **d_cols, long long **d_vals)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_offsets, d_cols, d_vals);
    return 0;
}

void grx_spgemm_destroy(grx_spgemm *p) { delete p; }

}  // extern "C"
