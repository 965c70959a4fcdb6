// app/msbfs/msbfs_problem.hpp -- device data for the multi-source BFS.
//
// The reference snapshot has no app/msbfs; the shape is this tree's Problem (compare app/scc/scc_problem.hpp).  The input CSR is
// read as a directed multigraph: duplicates and self-loops allowed (and without effect), rows unsorted, nothing symmetrised.  Init
// validates it as the other families do.  The in-neighbour lists a pull level needs are settled by Reset from the "inverse"
// option: the caller's, the graph itself when graphio::DeviceIsSymmetric says so, a transpose built on the device
// (graphio::DeviceTransposeCsr), or none.  State per vertex: three 64-bit words (msbfs_functor.hpp), two queue entries and the two
// per-vertex sums, 44 bytes; per source 20 bytes, and 4 * nodes more when the depths are stored.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/app/msbfs/msbfs_functor.hpp>
#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/pair_graph.hpp>
#include <gunrock/graphio/symmetry.hpp>

namespace gunrock {
namespace app {
namespace msbfs {

constexpr int kDepthsNotStored = -4;      // the depths were asked for after a Reset with store_depths off
constexpr int kInverseNotSymmetric = -5;  // "inverse" was forced to the graph itself and the symmetry check says it is directed

template <bool _USE_DOUBLE_BUFFER>
struct MsbfsProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        int *d_lent_iro = nullptr, *d_lent_ici = nullptr;    // the caller's in-neighbour lists
        DeviceArray<int> d_built_iro, d_built_ici;  // the transpose built here
        const int *d_iro = nullptr, *d_ici = nullptr;        // what the pull levels read (nullptr: none)
        DeviceArray<Word> d_seen, d_frontier, d_next;
        DeviceArray<int> d_queue[2];
        DeviceArray<Word> d_words;
        DeviceArray<int> d_sources;
        DeviceArray<unsigned long long> d_reached, d_dist_sum;
        DeviceArray<int> d_ecc;
        DeviceArray<int> d_sources_reaching;
        DeviceArray<unsigned long long> d_in_dist_sum;
        DeviceArray<int> d_depth;
        size_t source_capacity = 0, depth_capacity = 0;
    };

    SliceHolder<DataSlice> data_slices;
    bool fresh = false;   // Reset has run and Enact has not
    double build_ms = 0;  // HIP-event time of the transpose (0 when none was built)
    int inverse = INVERSE_AUTO;  // option "inverse", settled by the next Reset
    int settled = -1;            // the value d_iro / d_ici were settled for
    int symmetric = -1;          // the symmetry check's answer once asked
    std::vector<int> sources;    // of the last Reset
    bool store_depths = false;

    long long Batches() const { return (static_cast<long long>(sources.size()) + kBatch - 1) / kBatch; }

    // the kernels' view of batch `batch`
    Ctx DeviceCtx(long long batch, int wave_min_row) const
    {
        const DataSlice *ds = data_slices[0];
        const GraphSlice<int, int, int> *gs = this->graph_slices[0];
        const long long first = batch * kBatch;
        const long long count = static_cast<long long>(sources.size()) - first;
        Ctx c;
        c.ro = gs->d_row_offsets;
        c.ci = gs->d_column_indices;
        c.iro = ds->d_iro;
        c.ici = ds->d_ici;
        c.seen = ds->d_seen;
        c.frontier = ds->d_frontier;
        c.next = ds->d_next;
        c.queue_in = ds->d_queue[0];
        c.queue_out = ds->d_queue[1];
        c.words = ds->d_words;
        c.reached = ds->d_reached + first;
        c.dist_sum = ds->d_dist_sum + first;
        c.ecc = ds->d_ecc + first;
        c.sources_reaching = ds->d_sources_reaching;
        c.in_dist_sum = ds->d_in_dist_sum;
        c.depth = store_depths ? ds->d_depth + static_cast<size_t>(first) * static_cast<size_t>(this->nodes) : nullptr;
        c.mask = count >= kBatch ? ~0ull : (1ull << count) - 1ull;
        c.nodes = this->nodes;
        c.level = 0;
        c.wave_min_row = wave_min_row;
        return c;
    }

    hipError_t Build(int *d_inv_row_offsets, int *d_inv_col_indices)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t n1 = static_cast<size_t>(this->nodes > 0 ? this->nodes : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        // CSRs of `nodes` vertices?  (the kernels index with what they read)
        if ((retval = this->ValidateCsr())) return retval;
        if (d_inv_row_offsets && (retval = this->ValidateCsr(d_inv_row_offsets, d_inv_col_indices))) return retval;
        ds->d_lent_iro = d_inv_row_offsets;
        ds->d_lent_ici = d_inv_col_indices;
        DeviceArray<Word> *words[] = {&ds->d_seen, &ds->d_frontier, &ds->d_next};
        for (DeviceArray<Word> *a : words) if ((retval = a->Alloc(n1))) return retval;
        if ((retval = ds->d_queue[0].Alloc(n1))) return retval;
        if ((retval = ds->d_queue[1].Alloc(n1))) return retval;
        if ((retval = ds->d_sources_reaching.Alloc(n1))) return retval;
        if ((retval = ds->d_in_dist_sum.Alloc(n1))) return retval;
        return retval;
    }

    // One Init per object (grx_msbfs_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, false))) return retval;
        data_slices.Make();
        return Build(nullptr, nullptr);
    }

    // the inverse arrays: both or neither
    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_inv_row_offsets = nullptr,
                              int *d_inv_col_indices = nullptr)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        data_slices.Make();
        return Build(d_inv_row_offsets, d_inv_col_indices);
    }

    // d_iro / d_ci for the option's value.  *refused: INVERSE_SELF on a graph the check calls directed (nothing is changed then).
    hipError_t SettleInverse(bool *refused)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        *refused = false;
        if (settled == inverse) return retval;
        const long long n = this->nodes, m = this->edges;
        auto check = [&]() -> hipError_t {
            hipError_t retval = hipSuccess;
            if (symmetric >= 0) return retval;
            bool yes = false;
            GR_CHECK(graphio::DeviceIsSymmetric(static_cast<int>(n), m, gs->d_row_offsets, gs->d_column_indices, stream, yes), "MsbfsProblem symmetry check failed");
            symmetric = yes || m == 0 ? 1 : 0;  // (no entries: its own inverse)
            return retval;
        };
        const int *iro = nullptr, *ici = nullptr;
        bool build = false;
        switch (inverse) {
            case INVERSE_NONE:
                break;
            case INVERSE_SELF:
                if ((retval = check())) return retval;
                if (!symmetric) {
                    *refused = true;
                    return retval;
                }
                iro = gs->d_row_offsets;
                ici = gs->d_column_indices;
                break;
            case INVERSE_BUILD:
                build = !ds->d_lent_iro;
                break;
            default:  // INVERSE_AUTO: the caller's, the graph itself, a built one
                if (!ds->d_lent_iro) {
                    if ((retval = check())) return retval;
                    if (symmetric) {
                        iro = gs->d_row_offsets;
                        ici = gs->d_column_indices;
                    } else {
                        build = true;
                    }
                }
                break;
        }
        if (!iro && inverse != INVERSE_NONE && !build) {
            iro = ds->d_lent_iro;
            ici = ds->d_lent_ici;
        }
        if (build) {
            if (!ds->d_built_iro) {
                hipEvent_t ev[2] = {nullptr, nullptr};
                GR_CHECK(hipEventCreate(&ev[0]), "MsbfsProblem hipEventCreate failed");
                GR_CHECK(hipEventCreate(&ev[1]), "MsbfsProblem hipEventCreate failed");
                GR_CHECK(hipEventRecord(ev[0], stream), "MsbfsProblem hipEventRecord failed");
                if ((retval = ds->d_built_iro.Alloc(static_cast<size_t>(n) + 1))) return retval;
                if ((retval = ds->d_built_ici.Alloc(static_cast<size_t>(m > 0 ? m : 1)))) return retval;
                GR_CHECK(graphio::DeviceTransposeCsr(static_cast<int>(n), m, gs->d_row_offsets, gs->d_column_indices, ds->d_built_iro, ds->d_built_ici, stream),
                         "MsbfsProblem transpose failed");
                GR_CHECK(hipEventRecord(ev[1], stream), "MsbfsProblem hipEventRecord failed");
                GR_CHECK(hipStreamSynchronize(stream), "MsbfsProblem build sync failed");
                float ms = 0;
                GR_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]), "MsbfsProblem hipEventElapsedTime failed");
                build_ms = ms;
                hipEventDestroy(ev[0]);
                hipEventDestroy(ev[1]);
            }
            iro = ds->d_built_iro;
            ici = ds->d_built_ici;
        }
        ds->d_iro = iro;
        ds->d_ici = ici;
        settled = inverse;
        return retval;
    }

    // The sources (each in [0, nodes): the caller has checked) and every result as it stands before the first level: a source has
    // reached itself at depth 0 and nothing else.  *refused as SettleInverse's: then nothing has been reset.
    hipError_t Reset(const int *h_sources, long long count, bool with_depths, bool *refused)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if ((retval = SettleInverse(refused)) || *refused) return retval;
        const size_t n = static_cast<size_t>(this->nodes);
        const size_t rounded = static_cast<size_t>((count + kBatch - 1) / kBatch * kBatch);
        if (h_sources != sources.data()) sources.assign(h_sources, h_sources + count);
        store_depths = with_depths;
        fresh = false;
        if (rounded > ds->source_capacity) {
            ds->source_capacity = 0;
            if ((retval = ds->d_sources.Alloc(rounded))) return retval;
            if ((retval = ds->d_reached.Alloc(rounded))) return retval;
            if ((retval = ds->d_dist_sum.Alloc(rounded))) return retval;
            if ((retval = ds->d_ecc.Alloc(rounded))) return retval;
            ds->source_capacity = rounded;
        }
        const size_t cells = static_cast<size_t>(count) * n;
        if (with_depths && cells > ds->depth_capacity) {
            ds->depth_capacity = 0;
            if ((retval = ds->d_depth.Alloc(cells))) return retval;
            ds->depth_capacity = cells;
        }
        GR_CHECK(hipMemcpyAsync(ds->d_sources, sources.data(), sizeof(int) * static_cast<size_t>(count), hipMemcpyHostToDevice, stream),
                 "MsbfsProblem copy sources failed");
        GR_CHECK(hipMemsetAsync(ds->d_reached, 0, sizeof(unsigned long long) * rounded, stream), "MsbfsProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_dist_sum, 0, sizeof(unsigned long long) * rounded, stream), "MsbfsProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_ecc, 0, sizeof(int) * rounded, stream), "MsbfsProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_sources_reaching, 0, sizeof(int) * n, stream), "MsbfsProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_in_dist_sum, 0, sizeof(unsigned long long) * n, stream), "MsbfsProblem memset failed");
        if (with_depths) GR_CHECK(hipMemsetAsync(ds->d_depth, 0xFF, sizeof(int) * cells, stream), "MsbfsProblem memset failed");
        hipLaunchKernelGGL(ResetKernel, dim3(graphio::PairGrid(count)), dim3(kThreads), 0, stream, ds->d_sources, count, static_cast<int>(this->nodes), ds->d_reached,
                           ds->d_dist_sum, ds->d_ecc, ds->d_sources_reaching, with_depths ? ds->d_depth.p : nullptr);
        GR_CHECK(hipGetLastError(), "ResetKernel launch failed");
        GR_CHECK(hipStreamSynchronize(stream), "MsbfsProblem Reset sync failed");
        fresh = true;
        return retval;
    }

    // the last Reset's again (an Enact that does not follow one)
    hipError_t ResetAgain(bool *refused) { return Reset(sources.data(), static_cast<long long>(sources.size()), store_depths, refused); }

    // rows [first, first + count) of depth[source][vertex]; the caller has checked the range and that the depths are stored
    hipError_t ExtractDepths(long long first, long long count, int *h_depth)
    {
        const size_t n = static_cast<size_t>(this->nodes);
        return this->template Read<int>(h_depth, data_slices[0]->d_depth + static_cast<size_t>(first) * n, static_cast<size_t>(count) * n);
    }

    hipError_t SourceSummary(long long *h_reached, long long *h_dist_sum, int *h_ecc)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t k = sources.size();
        if ((retval = this->Read(reinterpret_cast<unsigned long long *>(h_reached), ds->d_reached.p, k))) return retval;
        if ((retval = this->Read(reinterpret_cast<unsigned long long *>(h_dist_sum), ds->d_dist_sum.p, k))) return retval;
        return this->Read(h_ecc, ds->d_ecc.p, k);
    }

    hipError_t VertexSummary(int *h_sources_reaching, long long *h_in_dist_sum)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t n = static_cast<size_t>(this->nodes);
        if ((retval = this->Read(h_sources_reaching, ds->d_sources_reaching.p, n))) return retval;
        return this->Read(reinterpret_cast<unsigned long long *>(h_in_dist_sum), ds->d_in_dist_sum.p, n);
    }
};

}  // namespace msbfs
}  // namespace app
}  // namespace gunrock
