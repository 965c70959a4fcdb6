// app/sample/sample_enactor.hpp -- host side of neighbourhood sampling.
//
// One Enact is a host loop over the hops.  A hop is: the sampler (LaneKernel or GroupKernel, and LongRowKernel behind a fanout of -1
// that can have met a long row), the renumbering (the bitmap's bits counted per word, scanned, filled in as the new vertices, and
// the new rows' offsets), the relabelling of the hop's columns, the count and the scan of the NEXT hop over the frontier the
// renumbering left on the device, and one read-back through StepHost::Read: the new vertices, the next hop's edges and the counters.
// So the edges of a hop are known before its sampler runs (a hop that would pass "edge_limit" is refused in front of it), and an
// Enact of H hops waits for the device H + 1 times: once for the seeds' own count, once per hop.  The host-side rules -- option
// ranges, fanouts, the strategy AUTO takes -- are SampleOptions, plain C++ that a host-only program can call.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/sample/sample_functor.hpp>
#include <gunrock/app/sample/sample_problem.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace sample {

// the phases the kernel time of an instrumented Enact is split into
enum { PHASE_COUNT = 0, PHASE_SAMPLE = 1, PHASE_RENUMBER = 2, PHASE_RELABEL = 3, PHASES = 4 };

// with replacement, AUTO takes LANE from this many seeds on
constexpr long long kLaneMinSeeds = 65536;

// options (grx_sample_set_option, grx_sample_set_fanouts) and what the host derives from them
struct SampleOptions {
    int strategy = SAMPLE_AUTO;
    unsigned long long seed = 0;
    int replace = 0;
    int weighted = 0;
    long long edge_limit = kMaxEdgeLimit;
    int long_row = kDefaultLongRow;
    int eids = 1;
    std::vector<int> fanouts;

    // 0: set, 1: unknown name, -1: a value out of range.  `weights`: Init had weights
    int Set(const char *name, double value, bool weights)
    {
        if (!(value == value)) return -1;
        const long long v = Whole(value);
        const bool whole = static_cast<double>(v) == value;
        if (!std::strcmp(name, "strategy")) {
            if (v < SAMPLE_AUTO || v > SAMPLE_GROUP) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "seed")) {
            if (!whole || v < 0 || v >= (1ll << 53)) return -1;
            seed = static_cast<unsigned long long>(v);
        } else if (!std::strcmp(name, "replace")) {
            if (v < 0 || v > 1 || (v == 0 && weighted)) return -1;  // weighted sampling without replacement is out
            replace = static_cast<int>(v);
        } else if (!std::strcmp(name, "weighted")) {
            if (v < 0 || v > 1 || (v == 1 && (!weights || !replace))) return -1;
            weighted = static_cast<int>(v);
        } else if (!std::strcmp(name, "edge_limit")) {
            if (v < 1 || v > kMaxEdgeLimit) return -1;
            edge_limit = v;
        } else if (!std::strcmp(name, "long_row")) {
            if (v < kMinLongRow) return -1;
            long_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else if (!std::strcmp(name, "eids")) {
            if (v < 0 || v > 1) return -1;
            eids = static_cast<int>(v);
        } else {
            return 1;
        }
        return 0;
    }

    // 0: taken; -1: hops outside 1 .. 16, a null list or a fanout outside {-1, 1 .. 64} (the list before stays)
    int SetFanouts(int hops, const int *list)
    {
        if (hops < 1 || hops > kMaxHops || !list) return -1;
        for (int h = 0; h < hops; ++h)
            if (!ValidFanout(list[h])) return -1;
        fanouts.assign(list, list + hops);
        return 0;
    }

    // the kernel that samples a batch of `seeds` seeds.  AUTO is GROUP, which won every measured cell without replacement and every
    // one of 1024 seeds; with replacement LANE won the two cells of 65 536 seeds at scale 20 by 7 and 13 % of the kernel time, so
    // AUTO takes it from there on (between 1024 and 65 536 seeds nothing was measured)
    int Strategy(long long seeds) const
    {
        if (strategy != SAMPLE_AUTO) return strategy;
        return replace && seeds >= kLaneMinSeeds ? SAMPLE_LANE : SAMPLE_GROUP;
    }
};

// `count` distinct vertices of 0 .. nodes - 1
inline bool DistinctVertices(const int *list, long long count, long long nodes)
{
    std::vector<int> sorted(list, list + count);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= nodes) return false;
    return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
}

template <bool INSTRUMENT>
class SampleEnactor : public EnactorBase {
   public:
    explicit SampleEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG), host("SampleEnactor") {}

    SampleOptions options;
    StepHost<INSTRUMENT> host;

    // of the last Enact
    bool refused = false;  // a hop would have passed "edge_limit": no result
    bool with_eids = true;
    int hops = 0;
    int taken = SAMPLE_GROUP;  // the strategy that ran
    std::vector<long long> vertex_ptr, edge_ptr;
    long long rows_expanded[kMaxHops], rows_sampled[kMaxHops], rows_copied[kMaxHops];
    long long long_rows = 0;
    double phase_ms[PHASES];

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long seeds = problem->num_seeds, nodes = problem->nodes;
        hops = static_cast<int>(options.fanouts.size());
        refused = false;
        with_eids = options.eids != 0;
        taken = options.Strategy(seeds);
        long_rows = 0;
        for (int h = 0; h < kMaxHops; ++h) rows_expanded[h] = rows_sampled[h] = rows_copied[h] = 0;
        for (double &ms : phase_ms) ms = 0;
        vertex_ptr.assign(static_cast<size_t>(hops) + 2, seeds);
        vertex_ptr[0] = 0;
        edge_ptr.assign(static_cast<size_t>(hops) + 1, 0);

        // the pinned words: the kernels' counters, the new vertices of the hop, the edges of the next
        if ((retval = host.Begin(sizeof(unsigned long long) * (W_COUNT + 2)))) return retval;
        unsigned long long *pin = reinterpret_cast<unsigned long long *>(host.pinned);
        unsigned long long *pin_new = pin + W_COUNT, *pin_edges = pin + W_COUNT + 1;

        auto phase = [&](int which, int launches, auto &&run) -> hipError_t {
            hipError_t rc = host.Start(stream);
            if (rc) return rc;
            if ((rc = run())) return rc;
            host.launches += launches;
            float ms = 0;
            rc = host.Stop(stream, &ms);
            phase_ms[which] += ms;
            return rc;
        };
        // the picks of the frontier [first, first + *d_count or count) of hop h, scanned: the edges of the hop behind the tile offsets
        auto count_hop = [&](int h, long long first, long long cap, const unsigned long long *d_count, long long count,
                             unsigned long long **d_total) -> hipError_t {
            hipError_t rc = problem->NeedFrontier(cap);
            if (rc) return rc;
            *d_total = ds->d_count_sums + (cap + 1 + graphio::kScanTile - 1) / graphio::kScanTile;
            return phase(PHASE_COUNT, 4, [&]() -> hipError_t {
                hipLaunchKernelGGL(CountKernel, GridFor(cap + 1, max_grid_size), dim3(256), 0, stream, ds->d_ro, options.weighted ? ds->d_prefix : nullptr,
                                   ds->d_vertices, first, cap, d_count, count, h, options.fanouts[h], options.replace, ds->d_counts, ds->d_words);
                const hipError_t launched = hipGetLastError();
                if (launched) return util::GRError(launched, "CountKernel launch failed", __FILE__, __LINE__);
                return graphio::DeviceExclusiveScan<unsigned long long>(ds->d_counts, ds->d_row_base, cap + 1, ds->d_count_sums, stream);
            });
        };
        auto read = [&](const unsigned long long *d_new, const unsigned long long *d_edges) -> hipError_t {
            hipError_t rc = hipSuccess;
            if (d_new && (rc = host.Copy(pin_new, d_new, sizeof(unsigned long long), stream))) return rc;
            if (d_edges && (rc = host.Copy(pin_edges, d_edges, sizeof(unsigned long long), stream))) return rc;
            return host.Read(pin, ds->d_words, sizeof(unsigned long long) * W_COUNT, stream);
        };

        // back to the seeds: the local ids of the sample before go, the seeds' rows are empty
        if ((retval = problem->ClearLocal(seeds))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "SampleEnactor memset failed");
        hipLaunchKernelGGL(EmptyRowsKernel, GridFor(seeds + 1, max_grid_size), dim3(256), 0, stream, ds->d_offsets, 0ll, nullptr, seeds, 0ll);
        GR_CHECK(hipGetLastError(), "EmptyRowsKernel launch failed");

        long long first = 0, count = seeds, vertices = seeds, edges = 0;
        unsigned long long *d_total = nullptr;
        if ((retval = count_hop(0, 0, seeds, nullptr, seeds, &d_total))) return retval;
        *pin_new = *pin_edges = 0;
        if ((retval = read(nullptr, d_total))) return retval;
        long long hop_edges = static_cast<long long>(*pin_edges);

        const long long bit_tiles = (problem->words32 + graphio::kScanTile - 1) / graphio::kScanTile;
        unsigned long long *d_new = ds->d_bit_sums + bit_tiles;
        for (int h = 0; h < hops && count > 0; ++h) {
            rows_expanded[h] = count;
            if (edges + hop_edges > options.edge_limit) {
                refused = true;
                return retval;
            }
            if (hop_edges == 0) break;  // nothing to pick: no new vertex, an empty frontier behind it
            const int f = options.fanouts[h];
            const long long room = std::min(hop_edges, nodes - vertices);  // the new vertices at the most
            if ((retval = problem->NeedEdges(edges + hop_edges, edges, with_eids))) return retval;
            if ((retval = problem->NeedVertices(vertices + room, vertices))) return retval;

            Ctx c;
            c.ro = ds->d_ro;
            c.ci = ds->d_ci;
            c.ent = ds->d_ent;
            c.prefix = options.weighted ? ds->d_prefix : nullptr;
            c.vertices = ds->d_vertices;
            c.row_base = ds->d_row_base;
            c.offsets = ds->d_offsets;
            c.cols = ds->d_cols;
            c.eids = with_eids ? ds->d_eids : nullptr;
            c.local = ds->d_local;
            c.bitmap = ds->d_bitmap;
            c.long_rows = ds->d_long_rows;
            c.words = ds->d_words;
            c.first = first;
            c.count = count;
            c.edge_base = edges;
            c.seed = options.seed;
            c.hop = h;
            c.f = f;
            c.replace = options.replace;
            c.long_row = options.long_row;
            const bool maybe_long = f == kAllNeighbours && hop_edges > options.long_row;
            if ((retval = phase(PHASE_SAMPLE, maybe_long ? 2 : 1, [&]() -> hipError_t {
                    if (taken == SAMPLE_LANE) {
                        hipLaunchKernelGGL(LaneKernel, GridFor(count, max_grid_size), dim3(kSampleThreads), LaneStripBytes(f, options.replace), stream, c);
                    } else {
                        const int g = GroupWidth(f);
                        hipLaunchKernelGGL(GroupKernel, StepGrid(count, 64 / g, kSampleWaves, max_grid_size), dim3(kSampleThreads), 0, stream, c, g);
                    }
                    hipError_t launched = hipGetLastError();
                    if (launched) return util::GRError(launched, "sample kernel launch failed", __FILE__, __LINE__);
                    if (maybe_long) {
                        hipLaunchKernelGGL(LongRowKernel, GridFor((2 * hop_edges / options.long_row + 1) * 256, max_grid_size), dim3(kSampleThreads), 0,
                                           stream, c);
                        if ((launched = hipGetLastError())) return util::GRError(launched, "LongRowKernel launch failed", __FILE__, __LINE__);
                    }
                    return hipSuccess;
                })))
                return retval;

            if ((retval = phase(PHASE_RENUMBER, 6, [&]() -> hipError_t {
                    hipLaunchKernelGGL(BitCountKernel, GridFor(problem->words32, max_grid_size), dim3(256), 0, stream, ds->d_bitmap, problem->words32,
                                       ds->d_bit_counts);
                    hipError_t launched = hipGetLastError();
                    if (launched) return util::GRError(launched, "BitCountKernel launch failed", __FILE__, __LINE__);
                    if ((launched = graphio::DeviceExclusiveScan<unsigned long long>(ds->d_bit_counts, ds->d_bit_base, problem->words32, ds->d_bit_sums, stream)))
                        return launched;
                    hipLaunchKernelGGL(FillKernel, GridFor(problem->words32, max_grid_size), dim3(256), 0, stream, ds->d_bitmap, problem->words32,
                                       ds->d_bit_base, vertices, ds->d_vertices, ds->d_local);
                    if ((launched = hipGetLastError())) return util::GRError(launched, "FillKernel launch failed", __FILE__, __LINE__);
                    hipLaunchKernelGGL(EmptyRowsKernel, GridFor(room + 1, max_grid_size), dim3(256), 0, stream, ds->d_offsets, vertices, d_new, 0ll,
                                       edges + hop_edges);
                    if ((launched = hipGetLastError())) return util::GRError(launched, "EmptyRowsKernel launch failed", __FILE__, __LINE__);
                    return hipSuccess;
                })))
                return retval;

            if ((retval = phase(PHASE_RELABEL, 1, [&]() -> hipError_t {
                    hipLaunchKernelGGL(RelabelKernel, GridFor(hop_edges, max_grid_size), dim3(256), 0, stream, ds->d_cols, edges, edges + hop_edges,
                                       ds->d_local);
                    const hipError_t launched = hipGetLastError();
                    return launched ? util::GRError(launched, "RelabelKernel launch failed", __FILE__, __LINE__) : hipSuccess;
                })))
                return retval;

            // the next hop's count over the frontier whose size is still on the device
            const bool more = h + 1 < hops && room > 0;
            if (more && (retval = count_hop(h + 1, vertices, room, d_new, 0, &d_total))) return retval;
            *pin_edges = 0;
            if ((retval = read(d_new, more ? d_total : nullptr))) return retval;

            edges += hop_edges;
            first = vertices;
            count = static_cast<long long>(*pin_new);
            vertices += count;
            hop_edges = static_cast<long long>(*pin_edges);
            for (int later = h; later < hops; ++later) {
                vertex_ptr[later + 2] = vertices;
                edge_ptr[later + 1] = edges;
            }
            problem->num_vertices = vertices;
            problem->num_edges = edges;
        }
        for (int h = 0; h < hops; ++h) {
            rows_sampled[h] = static_cast<long long>(pin[W_SAMPLED + h]);
            rows_copied[h] = static_cast<long long>(pin[W_COPIED + h]);
            long_rows += static_cast<long long>(pin[W_LONG + h]);
        }
        return retval;
    }
};

}  // namespace sample
}  // namespace app
}  // namespace gunrock
