// app/mst/mst_problem.hpp -- device data for the minimum spanning forest (Borůvka with edge filtering).
//
// Stands for the reference's MSTProblem (gunrock/app/mst/mst_problem.cuh:44-520):
//   DataSlice { d_mst_output, d_successors, d_represent, d_keys_array, ... }              (:58-95)
//   Init(stream_from_host, graph, num_gpus): uploads the CSR with its edge values          (:252-495)
//   Reset(frontier_type)                                                                    (:501-520)
//   Extract(h_mst_output): the 0/1 flag of every CSR entry in the forest                   (:218-245)
// Differences: the input is read as an undirected multigraph of any shape (unsorted rows, duplicates, asymmetric weights,
// self-loops, several components -- the reference needs a connected, mirrored graph, test_mst.cu:79, 410); the result is the
// unique forest under the order (weight, CSR index), so it is bit-exact and equals Kruskal over the entries sorted that way.
// No per-round renumbering: component ids stay vertex ids, and a compacted list of the entries that still cross components
// (cu, cv, key) shrinks round by round.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>

#include <gunrock/app/cc/cc_problem.hpp>
#include <gunrock/app/mst/mst_functor.hpp>
#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/device_csr.hpp>
#include <gunrock/graphio/symmetry.hpp>
#include <gunrock/util/memset_kernel.hpp>

namespace gunrock {
namespace app {
namespace mst {

template <bool _USE_DOUBLE_BUFFER>
struct MSTProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;
    typedef int VertexId;
    typedef int SizeT;
    typedef int Value;

    struct DataSlice {
        DeviceArray<int> d_selected;  // per CSR entry: 1 = in the forest (reference d_mst_output)
        DeviceArray<int> d_parent[2];  // component of every vertex; the hook writes the other buffer
        int cur = 0;                             // which d_parent is current
        DeviceArray<unsigned long long> d_best;  // per component: smallest key of an entry leaving it
        DeviceArray<int> d_froms;  // per CSR entry: its row
        DeviceArray<int> d_cu[2];  // the list of inter-component entries, double-buffered
        DeviceArray<int> d_cv[2];
        DeviceArray<unsigned long long> d_key[2];
        DeviceArray<unsigned> d_flags;  // filter: keep flags (list length + 1) ...
        DeviceArray<unsigned> d_pos;  // ... and their exclusive scan
        DeviceArray<unsigned long long> d_scan_sums;
        DeviceArray<unsigned long long> d_totals;  // [0] forest weight (two's complement), [1] forest edges
        DeviceArray<int> d_flag;  // convergence / mirror-weight word
    };

    SliceHolder<DataSlice> data_slices;
    int mirrored = 0;       // exact symmetry with equal mirror weights: round 1 by rows, only the f < t copies are listed
    long long list_capacity = 0;
    long long forest_edges = 0;
    long long total_weight = 0;
    util::PinnedArray<int> h_word;  // pinned read-back words

    // one device word read back (pinned)
    hipError_t ReadWord(const int *d_word, int &value, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(hipMemcpyAsync(h_word, d_word, sizeof(int), hipMemcpyDeviceToHost, stream), "MSTProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "MSTProblem read-back sync failed");
        value = h_word[0];
        return retval;
    }

    hipError_t AllocData()
    {
        hipError_t retval = hipSuccess;
        data_slices.Make();
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1), m1 = static_cast<size_t>(m > 0 ? m : 1);
        if ((retval = h_word.Alloc(2))) return retval;
        if ((retval = ds->d_flag.Alloc(1))) return retval;
        if ((retval = ds->d_totals.Alloc(2))) return retval;

        // 1. the CSR must be one: nothing below indexes with an unchecked value
        if ((retval = this->ValidateCsr())) return retval;

        if ((retval = ds->d_selected.Alloc(m1))) return retval;
        if ((retval = ds->d_parent[0].Alloc(n1))) return retval;
        if ((retval = ds->d_parent[1].Alloc(n1))) return retval;
        if ((retval = ds->d_best.Alloc(n1))) return retval;
        if ((retval = ds->d_froms.Alloc(m1))) return retval;
        if (n > 0) {
            hipLaunchKernelGGL((cc::ExpandRowsKernel<int, int>), dim3(2048), dim3(256), 0, stream, gs->d_row_offsets, static_cast<int>(n),
                               ds->d_froms);
            GR_CHECK(hipGetLastError(), "ExpandRowsKernel launch failed");
        }

        // 2. mirrored with equal weights?  (exact test: sorted duplicate-free rows, every edge with its mirror -- graphio/symmetry.hpp)
        mirrored = 0;
        const char *env = std::getenv("GUNROCK_MST_MIRRORED");  // (tests: "0" forces the general path on a mirrored input)
        if (m > 0 && !(env && env[0] == '0')) {
            bool symmetric = false;
            GR_CHECK(graphio::DeviceIsSymmetric(static_cast<int>(n), m, gs->d_row_offsets, gs->d_column_indices, stream, symmetric),
                     "MSTProblem symmetry test failed");
            if (symmetric) {
                GR_CHECK(hipMemsetAsync(ds->d_flag, 0, sizeof(int), stream), "MSTProblem memset failed");
                hipLaunchKernelGGL(MirrorWeightKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices,
                                   gs->d_edge_values, ds->d_froms, m, ds->d_flag);
                GR_CHECK(hipGetLastError(), "MirrorWeightKernel launch failed");
                int bad = 0;
                if ((retval = ReadWord(ds->d_flag, bad, stream))) return retval;
                mirrored = bad ? 0 : 1;
            }
        }

        // 3. the entry list: every non-loop entry at most (mirrored: the f < t half)
        list_capacity = mirrored ? m / 2 + 1 : m;  // (every f < t entry of a mirrored input has its f > t twin)
        const size_t lc = static_cast<size_t>(list_capacity > 0 ? list_capacity : 1);
        for (int b = 0; b < 2; ++b) {
            if ((retval = ds->d_cu[b].Alloc(lc))) return retval;
            if ((retval = ds->d_cv[b].Alloc(lc))) return retval;
            if ((retval = ds->d_key[b].Alloc(lc))) return retval;
        }
        if ((retval = ds->d_flags.Alloc(m1 + 1))) return retval;
        if ((retval = ds->d_pos.Alloc(m1 + 1))) return retval;
        if ((retval = ds->d_scan_sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(static_cast<long long>(m1) + 1))))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "MSTProblem AllocData failed");
        return retval;
    }

    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, true))) return retval;
        return AllocData();
    }

    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_edge_values)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices, d_edge_values))) return retval;
        return AllocData();
    }

    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        ds->cur = 0;
        util::MemsetIdx(ds->d_parent[0].p, this->nodes, stream);
        util::Memset(ds->d_selected.p, 0, this->edges, stream);
        GR_CHECK(hipMemsetAsync(ds->d_totals, 0, sizeof(unsigned long long) * 2, stream), "MSTProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "MSTProblem Reset sync failed");
        forest_edges = total_weight = 0;
        return retval;
    }

    // h_selected may be NULL: then only the totals are read
    hipError_t Extract(int *h_selected)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        unsigned long long totals[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(totals, ds->d_totals, sizeof(totals), hipMemcpyDeviceToHost, stream), "MSTProblem read totals failed");
        if (h_selected && this->edges > 0)
            GR_CHECK(hipMemcpyAsync(h_selected, ds->d_selected, sizeof(int) * static_cast<size_t>(this->edges), hipMemcpyDeviceToHost, stream),
                     "MSTProblem read d_selected failed");
        GR_CHECK(hipStreamSynchronize(stream), "MSTProblem Extract sync failed");
        total_weight = static_cast<long long>(totals[0]);
        forest_edges = static_cast<long long>(totals[1]);
        return retval;
    }
};

}  // namespace mst
}  // namespace app
}  // namespace gunrock
