// app/maxflow/maxflow_problem.hpp -- device data for the maximum flow and the minimum cut.
//
// The reference snapshot has no app/mf; the shape is this tree's Problem (compare app/bcc/bcc_problem.hpp).  The input CSR is read
// as a directed multigraph with int capacities in edge_values (NULL: 1 each).  Init validates it and builds, with
// graphio::PairGraph (graphio/pair_graph.hpp), the M canonical pairs a[p] < b[p] in (a, b) order and the residual CSR: the
// symmetric neighbour CSR over the pairs, rows ascending, with the capacity and the reverse entry on every entry.  The input CSR
// stays on the device (borrowed after InitFromDevice: the caller keeps it alive) because arc_flow[] is per input entry.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/maxflow/maxflow_functor.hpp>
#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace maxflow {

struct Summary {
    long long value = 0, side0 = 0, side1 = 0, side2 = 0, cut0 = 0, cut1 = 0;
    long long cap0 = 0, cap1 = 0;  // the capacity under each cut bit (both equal value: the enactor's second look at the certificate)
};

template <bool _USE_DOUBLE_BUFFER>
struct MaxflowProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_a, d_b, d_cap_ab, d_cap_ba, d_pent;  // per pair (pent: the entry a -> b)
        DeviceArray<int> d_nro, d_nci, d_neid;  // the residual CSR and the pair of every entry
        DeviceArray<int> d_mate, d_cap, d_res;  // per entry
        // per vertex
        DeviceArray<long long> d_excess;
        DeviceArray<int> d_height, d_queue, d_mark, d_list[2], d_fwd, d_bwd;
        DeviceArray<unsigned char> d_side;
        // per pair
        DeviceArray<int> d_flow;
        DeviceArray<unsigned char> d_cut;
        DeviceArray<int> d_arc_flow;  // per input entry, built at the first request behind an Enact
        DeviceArray<unsigned> d_words;
        DeviceArray<unsigned long long> d_counters;
        DeviceArray<unsigned long long> d_clock;  // PHASE_COUNT + 1 stamps
        DeviceArray<Front> d_front;
        DeviceArray<Active> d_active;
    };

    SliceHolder<DataSlice> data_slices;
    long long pairs = 0;   // M
    int src = -1, sink = -1;
    bool fresh = false;    // Reset has run and Enact has not
    bool enacted = false;  // the arrays hold a result
    bool have_arc_flow = false;
    double build_ms = 0;   // HIP-event time of the build of the pairs and the residual CSR
    Summary summary;       // of the last Enact

    Ctx DeviceCtx(int wave_min_row, int discharge_steps) const
    {
        const DataSlice *ds = data_slices[0];
        Ctx c;
        c.ro = ds->d_nro;
        c.ci = ds->d_nci;
        c.mate = ds->d_mate;
        c.res = ds->d_res;
        c.excess = ds->d_excess;
        c.height = ds->d_height;
        c.queue = ds->d_queue;
        c.mark = ds->d_mark;
        c.words = ds->d_words;
        c.counters = ds->d_counters;
        c.nodes = this->nodes;
        c.src = src;
        c.sink = sink;
        c.wave_min_row = wave_min_row;
        c.discharge_steps = discharge_steps;
        return c;
    }

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        if ((retval = ds->d_counters.Alloc(C_COUNT))) return retval;
        if ((retval = ds->d_clock.Alloc(PHASE_COUNT + 1))) return retval;
        if ((retval = ds->d_front.Alloc(1))) return retval;
        if ((retval = ds->d_active.Alloc(1))) return retval;

        // the CSR must be one: the build indexes with what it reads
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * W_COUNT, stream), "MaxflowProblem memset failed");  // (W_BAD, for the build)
        if ((retval = this->ValidateCsr())) return retval;

        long long M = 0;
        {  // (the build's scratch goes with this scope)
            graphio::BuildEvents ev;
            if ((retval = ev.Create(2))) return retval;
            if ((retval = ev.Record(0, stream))) return retval;
            graphio::PairGraph pg(n);
            graphio::DeviceScratch<unsigned long long> cap64;
            if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
            if ((retval = pg.Pairs(stream))) return retval;
            if ((retval = pg.Rows(stream))) return retval;
            ds->d_a.Adopt(graphio::Take(pg.d_src));
            ds->d_b.Adopt(graphio::Take(pg.d_dst));
            ds->d_nro.Adopt(graphio::Take(pg.d_ro));
            ds->d_nci.Adopt(graphio::Take(pg.d_ci));
            ds->d_neid.Adopt(graphio::Take(pg.d_eid));
            M = pg.pairs;
            if (m > 0) {
                if (M > 0) {
                    // the capacities: every arc finds its entry by bisecting the sorted row (the key sort carries no payload) and adds
                    // in 64 bits; then a pair's two sums must fit one int together
                    const size_t ms = static_cast<size_t>(M);
                    if ((retval = cap64.Alloc(2 * ms))) return retval;
                    GR_CHECK(hipMemsetAsync(cap64.p, 0, sizeof(unsigned long long) * 2 * ms, stream), "MaxflowProblem memset failed");
                    if ((retval = ds->d_mate.Alloc(2 * ms))) return retval;
                    if ((retval = ds->d_cap.Alloc(2 * ms))) return retval;
                    if ((retval = ds->d_res.Alloc(2 * ms))) return retval;
                    if ((retval = ds->d_cap_ab.Alloc(ms))) return retval;
                    if ((retval = ds->d_cap_ba.Alloc(ms))) return retval;
                    if ((retval = ds->d_pent.Alloc(ms))) return retval;
                }
                // (self-loops only, M = 0: their capacities are still looked at)
                hipLaunchKernelGGL(AccumulateKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices, gs->d_edge_values,
                                   static_cast<int>(n), m, ds->d_nro, ds->d_nci, cap64.p, ds->d_words + W_BAD);
                GR_CHECK(hipGetLastError(), "AccumulateKernel launch failed");
                if (M > 0) {
                    hipLaunchKernelGGL(PairEntriesKernel, dim3(graphio::PairGrid(M)), dim3(256), 0, stream, ds->d_a, ds->d_b, M, ds->d_nro, ds->d_nci, cap64.p, ds->d_pent,
                                       ds->d_mate, ds->d_cap, ds->d_cap_ab, ds->d_cap_ba, ds->d_words + W_BAD);
                    GR_CHECK(hipGetLastError(), "PairEntriesKernel launch failed");
                }
                unsigned bad_cap = 0;
                GR_CHECK(hipMemcpyAsync(&bad_cap, ds->d_words + W_BAD, sizeof(bad_cap), hipMemcpyDeviceToHost, stream), "MaxflowProblem read-back failed");
                GR_CHECK(hipStreamSynchronize(stream), "MaxflowProblem read-back sync failed");
                if (bad_cap) return this->Malformed();
            }
            pairs = M;
            if ((retval = ev.Record(1, stream))) return retval;
            GR_CHECK(hipStreamSynchronize(stream), "MaxflowProblem build sync failed");
            if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        }

        const size_t m1 = static_cast<size_t>(M > 0 ? M : 1);
        DeviceArray<int> *vertex_arrays[] = {&ds->d_height, &ds->d_queue, &ds->d_mark, &ds->d_list[0], &ds->d_list[1], &ds->d_fwd, &ds->d_bwd};
        for (DeviceArray<int> *a : vertex_arrays) if ((retval = a->Alloc(n1))) return retval;
        if ((retval = ds->d_excess.Alloc(n1))) return retval;
        if ((retval = ds->d_side.Alloc(n1))) return retval;
        if ((retval = ds->d_flow.Alloc(m1))) return retval;
        if ((retval = ds->d_cut.Alloc(m1))) return retval;
        if ((retval = ds->d_arc_flow.Alloc(static_cast<size_t>(m > 0 ? m : 1)))) return retval;
        return retval;
    }

    // One Init per object (grx_maxflow_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, true))) return retval;
        data_slices.Make();
        return Build();
    }

    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_capacities)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices, d_capacities))) return retval;
        data_slices.Make();
        return Build();
    }

    // the residuals back at the capacities; excess, heights, marks, words and counters at 0.  The caller has checked the pair.
    hipError_t Reset(int new_src, int new_sink)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t n = static_cast<size_t>(this->nodes), M = static_cast<size_t>(pairs);
        src = new_src;
        sink = new_sink;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * W_COUNT, stream), "MaxflowProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(unsigned long long) * C_COUNT, stream), "MaxflowProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_clock, 0, sizeof(unsigned long long) * (PHASE_COUNT + 1), stream), "MaxflowProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_excess, 0, sizeof(long long) * n, stream), "MaxflowProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_height, 0, sizeof(int) * n, stream), "MaxflowProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_mark, 0, sizeof(int) * n, stream), "MaxflowProblem memset failed");
        if (M) GR_CHECK(hipMemcpyAsync(ds->d_res, ds->d_cap, sizeof(int) * 2 * M, hipMemcpyDeviceToDevice, stream), "MaxflowProblem copy failed");
        GR_CHECK(hipStreamSynchronize(stream), "MaxflowProblem Reset sync failed");
        fresh = true;
        enacted = false;
        have_arc_flow = false;
        summary = Summary();
        return retval;
    }

    // every pointer may be NULL
    hipError_t Pairs(int *h_a, int *h_b, int *h_cap_ab, int *h_cap_ba)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t M = static_cast<size_t>(pairs);
        if ((retval = this->Read(h_a, ds->d_a.p, M))) return retval;
        if ((retval = this->Read(h_b, ds->d_b.p, M))) return retval;
        if ((retval = this->Read(h_cap_ab, ds->d_cap_ab.p, M))) return retval;
        return this->Read(h_cap_ba, ds->d_cap_ba.p, M);
    }

    hipError_t Extract(int *h_flow, unsigned char *h_side, unsigned char *h_cut)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t n = static_cast<size_t>(this->nodes), M = static_cast<size_t>(pairs);
        if ((retval = this->Read(h_flow, ds->d_flow.p, M))) return retval;
        if ((retval = this->Read(h_side, ds->d_side.p, n))) return retval;
        return this->Read(h_cut, ds->d_cut.p, M);
    }

    // arc_flow[] per input entry: a function of the residuals and the input, computed once per Enact
    hipError_t ArcFlow(int *h_arc_flow)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        const long long m = this->edges;
        if (m < 1) return retval;
        if (!have_arc_flow) {
            if (pairs > 0) {
                hipLaunchKernelGGL(ArcFlowKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, gs->stream, gs->d_row_offsets, gs->d_column_indices, gs->d_edge_values,
                                   static_cast<int>(this->nodes), m, ds->d_nro, ds->d_nci, ds->d_cap, ds->d_res, ds->d_arc_flow);
                GR_CHECK(hipGetLastError(), "ArcFlowKernel launch failed");
            } else {
                GR_CHECK(hipMemsetAsync(ds->d_arc_flow, 0, sizeof(int) * static_cast<size_t>(m), gs->stream), "MaxflowProblem memset failed");
            }
            have_arc_flow = true;
        }
        return this->Read(h_arc_flow, ds->d_arc_flow.p, static_cast<size_t>(m));
    }
};

}  // namespace maxflow
}  // namespace app
}  // namespace gunrock
