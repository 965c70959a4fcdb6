// app/bfs/bfs_problem.hpp -- device data for breadth-first search.
//
// Same contract as the reference's BFSProblem (gunrock/app/bfs/bfs_problem.cuh:41-364):
//   DataSlice { d_labels, d_preds, d_visited_mask }          (:57-63)
//   Init(stream_from_host, graph, num_gpus)                  (:188-261)
//   Reset(src, frontier_type, queue_sizing): labels = -1, preds = -2, mask = 0; then the source gets
//        label 0, pred -1 and is queued                      (:272-360)
//   Extract(h_labels, h_preds)                               (:144-177)
// MI355X-first differences:
//   * d_visited_mask is a bitmap of 32-bit words (n/32 words: 2 MiB at scale-24, resident in every
//     XCD's 4 MiB L2) updated with agent-scope atomicOr, so each vertex is discovered exactly once in
//     every mode -- the reference's byte mask with non-atomic RMW (filter/cta.cuh:166-207) tolerates
//     duplicate discovery, which costs redundant edge expansion on the next level;
//   * it is allocated in all four (mark_pred, idempotence) modes, and d_preds whenever MARK_PREDECESSORS
//     (the reference drops preds in idempotent+pred mode and stores garbage in labels, SURVEY appendix C;
//     here that mode yields depth labels AND valid parents);
//   * the current BSP iteration travels inside the by-value DataSlice kernel argument.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/device_csr.hpp>
#include <gunrock/graphio/relabel.hpp>
#include <gunrock/oprtr/advance/binned.hpp>
#include <gunrock/oprtr/advance/bottom_up.hpp>
#include <gunrock/util/frontier.hpp>
#include <gunrock/util/memset_kernel.hpp>

namespace gunrock {
namespace app {
namespace bfs {

// bit v = (v has no in-edge); one wave per 64 vertices, the word is written whole
template <typename SizeT>
__global__ void NoInEdgeMaskKernel(const SizeT *d_inv_row_offsets, long long nodes, long long words64, unsigned long long *d_mask)
{
    const unsigned lane = threadIdx.x & 63;
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / 64;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / 64;
    for (long long w = wave0; w < words64; w += nwaves) {
        const long long v = w * 64 + lane;
        const bool none = v < nodes && d_inv_row_offsets[v + 1] == d_inv_row_offsets[v];
        const unsigned long long m = __ballot(none);
        if (lane == 0) d_mask[w] = m;
    }
}

// vertices WITH in-edges per 64-vertex word (bits past the vertex count do not count)
static __global__ void WithInEdgesCountKernel(const unsigned long long *d_never, long long nodes, long long words64, unsigned *d_counts)
{
    const long long w = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (w >= words64) return;
    unsigned long long with_edges = ~d_never[w];
    const long long first = w * 64;
    if (first >= nodes) with_edges = 0;
    else if (first + 64 > nodes) with_edges &= (1ull << (nodes - first)) - 1ull;
    d_counts[w] = static_cast<unsigned>(__popcll(with_edges));
}

// Reset in one launch: 16-byte stores for labels / preds, the source patched in flight, queue entry 0 seeded.
// fill_labels = 0: labels are deferred (BFSProblem::labels_deferred) -- only the source's label is written here and
// EmitLabelsKernel writes every label once, at the end of Enact.
template <typename VertexId, typename SizeT, bool PRED>
__global__ void BfsResetKernel(VertexId *d_labels, VertexId *d_preds, unsigned *d_visited, const unsigned *d_never,
                               unsigned *d_snapshot, int fill_labels, long long nodes,
                               long long mask_words, VertexId src, const SizeT *d_row_offsets,
                               util::Frontier<VertexId, SizeT> queue0, SizeT *h_src_row, unsigned long long *h_src_seq,
                               unsigned long long seq, unsigned long long *d_arm_tail, int *d_arm_overflow, unsigned long long *d_arm_wide,
                               int *d_arm_log)
{
    // d_arm_*: the device words of the enactor that ran the last search on this problem (util::WorkProgress): zeroing them and
    // seeding ring slot 0 with the source's (1, degree) HERE saves that enactor its own arming kernel and the host wait for the
    // source's degree in front of it (~8 us at the start of every Enact)
    typedef __attribute__((ext_vector_type(4))) int V4;
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long tid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const long long nvec = nodes / 4;
    V4 *labels4 = reinterpret_cast<V4 *>(d_labels);
    V4 *preds4 = reinterpret_cast<V4 *>(d_preds);
    if (fill_labels || PRED) {
        for (long long k = tid; k < nvec; k += stride) {
            V4 l = {-1, -1, -1, -1};
            V4 p = {-2, -2, -2, -2};
            if (src >= 0 && k == src / 4) {
                l[src & 3] = 0;
                p[src & 3] = -1;
            }
            if (fill_labels) labels4[k] = l;
            if (PRED) preds4[k] = p;
        }
        for (long long i = nvec * 4 + tid; i < nodes; i += stride) {
            if (fill_labels) d_labels[i] = (i == src) ? 0 : -1;
            if (PRED) d_preds[i] = (i == src) ? -1 : -2;
        }
    }
    if (!fill_labels && tid == 0 && src >= 0) d_labels[src] = 0;
    for (long long w = tid; w < mask_words; w += stride)
    {
        const unsigned never = d_never ? d_never[w] : 0u;
        const unsigned src_bit = (src >= 0 && w == (src >> 5)) ? (1u << (src & 31)) : 0u;
        d_visited[w] = never | src_bit;
        // "visited before the search": what a direction switch at level 0 diffs against; the source must survive the diff
        if (d_snapshot) d_snapshot[w] = never & ~src_bit;
    }
    if (d_arm_tail && blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t >= 1 && t < util::WorkProgress::kSlots) d_arm_tail[t] = 0ull;  // (slot 0 below)
        if (t < util::WorkProgress::kWideLines)
            for (int k = 0; k < util::WorkProgress::kWideSets; ++k) d_arm_wide[(k * util::WorkProgress::kWideLines + t) * util::WorkProgress::kWideStride] = 0ull;
        if (t < 8) d_arm_log[t] = 0;
        if (t == 0) {
            *d_arm_overflow = 0;
            unsigned long long seed = 0ull;
            if (src >= 0) {
                const SizeT b = d_row_offsets[src], e = d_row_offsets[src + 1];
                if (e > b) seed = util::PackTail(1u, static_cast<unsigned>(e - b));
            }
            d_arm_tail[0] = seed;
        }
    }
    if (tid == 0 && src >= 0) {
        const SizeT begin = d_row_offsets[src], end = d_row_offsets[src + 1];
        queue0.v[0] = src;
        queue0.row_start[0] = begin;
        queue0.scan[0] = 0;
        // straight into pinned host memory, sequence word last: the host learns the source's degree while this kernel is
        // still filling labels, and queues the first level behind it without a stream synchronisation
        h_src_row[0] = begin;
        h_src_row[1] = end;
        __threadfence_system();
        __hip_atomic_store(h_src_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- deferred labels (direction-optimizing searches) ----
// A bottom-up sweep or the closing pass of a count-only level finds its vertices in VERTEX order but only some of every 16:
// writing their labels there is one partial 64-byte sector after the other (PMC, round 2: 2.3x write amplification, 34 us of
// a 350 us scale-24 search), on top of the 64 MB fill of -1 at Reset.  BFS depth = the level whose frontier bitmap holds the
// vertex, so those levels only KEEP their output bitmap (n/8 bytes each, a pool of kLevelMasks) and this kernel writes every
// label of the search once, 16 bytes per lane, at the end of Enact:
//   bit set in the bitmap of level L              -> L
//   visited, in no kept bitmap, has in-edges       -> what a top-down kernel wrote (they label at discovery: few vertices)
//   the source                                     -> 0 (Reset wrote it)
//   otherwise                                      -> -1
// FULL = false is the flush used when the pool runs out of bitmaps in the middle of a search: only the set bits are stored.
constexpr int kLevelMasks = 12;

template <typename VertexId>
struct LevelMaskList {
    const unsigned long long *mask[kLevelMasks];
    VertexId label[kLevelMasks];
    int count = 0;
    // a pass queued behind a chain of sweeps before the host knows how the chain ended: entries [chain_first, count) are the
    // chain's bitmaps in order, of which only the first d_gate[1] were filled; d_gate[0] == 0: do not run at all
    int chain_first = 0;
    const int *d_gate = nullptr;
};

// KMAX = bitmaps the kernel reads (entries past levels.count repeat entry 0: the same bit gives the same label).  All KMAX + 2
// word loads of a lane are issued before the first is looked at -- with a run-time loop over the list every bitmap was its own
// dependent round trip (33 us for the 64 MB of a scale-24 graph; the store stream alone is ~14 us).
template <typename VertexId, bool FULL, int KMAX>
__global__ __launch_bounds__(256) void EmitLabelsKernel(LevelMaskList<VertexId> levels, const unsigned long long *d_visited,
                                                        const unsigned long long *d_never, long long nodes, VertexId src, VertexId *d_labels)
{
    typedef __attribute__((ext_vector_type(4))) int V4;
    int valid = KMAX;  // entries that count (the padding repeats entry 0: harmless)
    if (levels.d_gate) {  // (uniform)
        if (levels.d_gate[0] == 0) return;
        valid = levels.chain_first + levels.d_gate[1];
    }
    const long long quads = (nodes + 3) / 4;  // four consecutive vertices per lane: one 16-byte store
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long q = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; q < quads; q += stride) {
        const long long v0 = q * 4;
        const long long w = v0 >> 6;
        const int sh = static_cast<int>(v0 & 63);
        unsigned long long mw[KMAX > 0 ? KMAX : 1];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) mw[k] = levels.mask[k][w];  // (the sixteen lanes of a word read the same address)
        unsigned long long vis = 0, nev = 0;
        if (FULL) {
            vis = d_visited[w];
            nev = d_never ? d_never[w] : 0ull;  // pre-marked "visited": never discovered
        }
        V4 out = {-1, -1, -1, -1};
        unsigned covered = 0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const unsigned m = (k < valid) ? static_cast<unsigned>(mw[k] >> sh) & 0xFu : 0u;
            covered |= m;
            const VertexId l = levels.label[k];
            if (m & 1u) out[0] = l;
            if (m & 2u) out[1] = l;
            if (m & 4u) out[2] = l;
            if (m & 8u) out[3] = l;
        }
        if (FULL) {
            unsigned keep = static_cast<unsigned>((vis & ~nev) >> sh) & 0xFu & ~covered;
            if (src >= v0 && src < v0 + 4) keep |= 1u << (src - v0);
            if (keep) {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (((keep >> b) & 1u) && v0 + b < nodes) out[b] = d_labels[v0 + b];
            }
            if (v0 + 3 < nodes) *reinterpret_cast<V4 *>(d_labels + v0) = out;
            else
                for (int b = 0; b < 4 && v0 + b < nodes; ++b) d_labels[v0 + b] = out[b];
        } else if (covered) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (((covered >> b) & 1u) && v0 + b < nodes) d_labels[v0 + b] = out[b];
        }
    }
}

// The closing label pass of a search on the relabelled copy (graphio/relabel.hpp): the level bitmaps, the visited bitmap and
// the work labels / predecessors are in the copy's numbering, the output is in the caller's, four vertices (16 bytes) per lane.
// The tier-0 (hub) vertices of a quad are consecutive new ids, and so are its tier-1 vertices: one window of each bitmap per tier
// covers them, and every word of a window is loaded before the first is looked at (one round trip, as in EmitLabelsKernel).  A
// vertex without edges is -1 without a lookup (the source: 0, predecessor -1).  Same gate and padding rules as
// EmitLabelsKernel<FULL = true>.
template <typename VertexId, int KMAX, bool PRED>
__device__ __forceinline__ void TranslateTier(const LevelMaskList<VertexId> &levels, int valid, const unsigned long long *d_visited,
                                              unsigned t4, long long x1, const VertexId *d_work_labels, const VertexId *d_work_preds,
                                              const VertexId *d_old_of_new, int (&out)[4], int (&pout)[4])
{
    const long long xw = x1 >> 6;
    const int xs = static_cast<int>(x1 & 63);
    const bool cross = xs > 60;  // (the window of up to four bits reaches into the next word)
    unsigned long long lo[KMAX > 0 ? KMAX : 1], hi[KMAX > 0 ? KMAX : 1];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) lo[k] = levels.mask[k][xw];
    const unsigned long long vlo = d_visited[xw];
    unsigned long long vhi = 0ull;
    if (cross) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) hi[k] = levels.mask[k][xw + 1];
        vhi = d_visited[xw + 1];
    }
    int lab[4] = {-1, -1, -1, -1};
    unsigned covered = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const unsigned long long win = (lo[k] >> xs) | (cross ? hi[k] << (64 - xs) : 0ull);
        const unsigned m = (k < valid) ? static_cast<unsigned>(win) & 0xFu : 0u;
        covered |= m;
        const VertexId l = levels.label[k];
        if (m & 1u) lab[0] = l;
        if (m & 2u) lab[1] = l;
        if (m & 4u) lab[2] = l;
        if (m & 8u) lab[3] = l;
    }
    const unsigned cnt = static_cast<unsigned>(__popc(t4));
    const unsigned vis = static_cast<unsigned>((vlo >> xs) | (cross ? vhi << (64 - xs) : 0ull)) & ((1u << cnt) - 1u);
    const unsigned keep = vis & ~covered;  // visited, in no kept bitmap: what a top-down kernel wrote at discovery
    int j = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if (!((t4 >> b) & 1u)) continue;
        int l = lab[0];
        if (j == 1) l = lab[1];
        if (j == 2) l = lab[2];
        if (j == 3) l = lab[3];
        if ((keep >> j) & 1u) l = d_work_labels[x1 + j];
        out[b] = l;
        if (PRED) {
            const VertexId p = d_work_preds[x1 + j];
            pout[b] = p >= 0 ? d_old_of_new[p] : p;
        }
        ++j;
    }
}

template <typename VertexId, int KMAX, bool PRED>
__global__ __launch_bounds__(256) void TranslateLabelsKernel(LevelMaskList<VertexId> levels, const unsigned long long *d_visited,
                                                             graphio::RelabelView map, long long nodes, VertexId caller_src,
                                                             const VertexId *d_work_labels, const VertexId *d_work_preds,
                                                             const VertexId *d_old_of_new, VertexId *d_labels, VertexId *d_preds)
{
    typedef __attribute__((ext_vector_type(4))) int V4;
    int valid = KMAX;
    if (levels.d_gate) {  // (uniform)
        if (levels.d_gate[0] == 0) return;
        valid = levels.chain_first + levels.d_gate[1];
    }
    const bool hubs = map.hubs > 0;  // (uniform)
    const long long quads = (nodes + 3) / 4;
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long q = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; q < quads; q += stride) {
        const long long v0 = q * 4;
        const long long w = v0 >> 6;
        const int sh = static_cast<int>(v0 & 63);
        const unsigned long long edge = map.d_edge[w];
        const unsigned long long hub = hubs ? map.d_hub[w] : 0ull;
        const long long b1 = map.d_base1[w];
        const long long b0 = hubs ? map.d_base0[w] : 0ll;
        const unsigned long long low = (1ull << sh) - 1ull;
        const unsigned h4 = static_cast<unsigned>(hub >> sh) & 0xFu, e4 = static_cast<unsigned>(edge >> sh) & 0xFu;
        int out[4] = {-1, -1, -1, -1};
        int pout[4] = {-2, -2, -2, -2};
        if (e4)
            TranslateTier<VertexId, KMAX, PRED>(levels, valid, d_visited, e4, map.hubs + b1 + __popcll(edge & low), d_work_labels, d_work_preds,
                                                d_old_of_new, out, pout);
        if (h4)
            TranslateTier<VertexId, KMAX, PRED>(levels, valid, d_visited, h4, b0 + __popcll(hub & low), d_work_labels, d_work_preds,
                                                d_old_of_new, out, pout);
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (caller_src == v0 + b && !(((h4 | e4) >> b) & 1u)) {  // a source without edges
                out[b] = 0;
                pout[b] = -1;
            }
        if (v0 + 3 < nodes) {
            *reinterpret_cast<V4 *>(d_labels + v0) = V4{out[0], out[1], out[2], out[3]};
            if (PRED) *reinterpret_cast<V4 *>(d_preds + v0) = V4{pout[0], pout[1], pout[2], pout[3]};
        } else {
            for (int b = 0; b < 4 && v0 + b < nodes; ++b) {
                d_labels[v0 + b] = out[b];
                if (PRED) d_preds[v0 + b] = pout[b];
            }
        }
    }
}

// ---- the tiled closing label pass (label_pass = 1; both numberings) ----
// The two kernels above derive the four labels of a quad per lane: the sixteen lanes of a 64-vertex word load and decode the same
// words of every kept bitmap (EmitLabelsKernel), or a window of every bitmap at their own bit offset and, as soon as one
// lane's window crosses a word, a second one (TranslateLabelsKernel: 14 wave-level loads per 1 KiB wave store at scale-24).
// Here a workgroup owns a tile of kLabelTileWords consecutive 64-vertex words of the caller's numbering and loads every bitmap
// word the tile needs ONCE, coalesced:
//   phase 1: one lane per word of the search numbering folds that word of all kept bitmaps and of the visited bitmap into
//            four code bit-planes in LDS.  The code of a vertex is 0 "no label" (-1), k + 1 "in kept bitmap k", or 13
//            "visited, in no kept bitmap, not pre-marked" (the label a top-down kernel wrote at discovery: a gather).
//            On the relabelled copy the tile's tier-1 vertices are one run of consecutive new ids (the renumbering is a
//            stable partition), at most kLabelTileWords + 1 words, and so are its tier-0 vertices: one plane set per tier.
//            The tier masks and bases of the tile go through LDS as well.
//   phase 2: every lane takes the four code bits of its quads out of the planes, maps code -> label through a 16-entry
//            table, gathers the rare code-13 label and stores 16 bytes.  The pass is bound by instruction issue once the
//            loads are shared, so this phase works on 32-bit halves: the four planes of a half sit in one 16-byte LDS
//            entry, an unaligned window is two such reads and one v_alignbit per plane, a 256-byte table spreads the window's
//            bits over the quad's positions of the tier (so both tiers OR into one set of nibbles), and one 24-bit multiply
//            per vertex gathers its four plane bits into the table offset.
// All global loads of phase 1 are issued before the first is used; phase 2 has none but the gathers.  Gate, source and
// edgeless-vertex rules are those of the kernels above.  List entries at or past `valid` do not count (the host pads
// them with a loadable pointer).  Kept bitmaps are frontiers of different levels and never overlap; if two ever did, the
// last listed one wins, as above.
constexpr int kLabelTileWords = 64;                // 4096 vertices, 16 KiB of labels per 256-thread workgroup
constexpr int kLabelSpan = kLabelTileWords + 2;    // plane words per tier: the run's kLabelTileWords + 1 and a window's upper word
static_assert(kLabelSpan <= 128 && kLabelTileWords % 16 == 0, "phase 1 maps one tier to each half of the workgroup");
constexpr unsigned kCodeWorkLabel = 13u;
static_assert(kLevelMasks < kCodeWorkLabel && kCodeWorkLabel < 16u, "four code planes");

typedef __attribute__((ext_vector_type(4))) unsigned LabelPlanes;  // the four code planes of one 32-bit half word

// ORs into e[p] the window of plane p that starts at search-numbering id x, spread over the positions t4 of the quad
__device__ __forceinline__ void TiledWindow(const LabelPlanes *planes, const unsigned char *spread, unsigned t4, unsigned x, unsigned first_half,
                                            unsigned (&e)[4])
{
    const unsigned j = (x >> 5) - first_half;
    const LabelPlanes lo = planes[j], hi = planes[j + 1];
    const unsigned row = t4 << 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)  // (v_alignbit shifts by x & 31; window bits past the tier's vertices of the quad are not looked at)
        e[p] |= spread[row | (__builtin_amdgcn_alignbit(hi[p], lo[p], x) & 0xFu)];
}

// RELABEL: the search ran on the relabelled copy (bitmaps, d_work_* in its numbering; output in the caller's).  Otherwise
// d_work_labels == d_labels, in place, and predecessors are not touched (they were written at discovery).
template <typename VertexId, bool RELABEL, bool PRED>
__global__ __launch_bounds__(256) void TiledLabelsKernel(LevelMaskList<VertexId> levels, const unsigned long long *d_visited,
                                                         const unsigned long long *d_never, graphio::RelabelView map, long long nodes,
                                                         VertexId src, const VertexId *d_work_labels, const VertexId *d_work_preds,
                                                         const VertexId *d_old_of_new, VertexId *d_labels, VertexId *d_preds,
                                                         util::PublishArgs publish)
{
    typedef __attribute__((ext_vector_type(4))) int V4;
    // The enactor's closing read-back rides on this pass (frontier.hpp PublishBody): every word it mirrors was final before
    // the pass started and the pass reads none of the words it re-arms, so the host learns how the search ended while the
    // tiles are still being written.  First of all, before the gate: a pass that does not run must still publish.
    if (publish.box && blockIdx.x == 0 && threadIdx.x < 64) util::PublishBody(publish);  // (uniform per wave; only read)
    __shared__ LabelPlanes planes[2][2 * kLabelSpan];  // [0]: tier 1 (or the caller's numbering), [1]: tier 0; per 32-bit half
    __shared__ uint2 s_tier[2][2 * kLabelTileWords];   // per half of a caller word: (tier mask, new id of its first tier vertex)
    __shared__ int table[16];
    __shared__ unsigned char spread[256];              // [t4 << 4 | c]: the low bits of c dealt to the set positions of t4
    const int t = threadIdx.x;
    const long long words = (nodes + 63) / 64;
    const long long w0 = static_cast<long long>(blockIdx.x) * kLabelTileWords;
    const bool hubs = RELABEL && map.hubs > 0;  // (uniform)
    // first search-numbering word of the tile's tier-1 / tier-0 run (asked for before the gate words: one round trip)
    long long xw1 = w0, xwh = 0;
    if (RELABEL) {
        xw1 = (map.hubs + map.d_base1[w0]) >> 6;
        if (hubs) xwh = map.d_base0[w0] >> 6;
    }
    int valid = levels.count;
    if (levels.d_gate) {  // (uniform)
        const int go = levels.d_gate[0], filled = levels.d_gate[1];
        if (go == 0) return;
        valid = levels.chain_first + filled;
    }
    // phase 1
    if (t < 16) table[t] = (t >= 1 && t <= kLevelMasks) ? levels.label[t - 1] : -1;
    if (RELABEL) {
        unsigned dealt = 0u;
        for (int b = 0, r = 0; b < 4; ++b)
            if ((t >> (4 + b)) & 1) {
                dealt |= ((static_cast<unsigned>(t) >> r) & 1u) << b;
                ++r;
            }
        spread[t] = static_cast<unsigned char>(dealt);
    }
    unsigned long long tile_edge = 0ull, tile_hub = 0ull;
    unsigned tile_base1 = 0u, tile_base0 = 0u;
    if (RELABEL && t < kLabelTileWords && w0 + t < words) {
        tile_edge = map.d_edge[w0 + t];
        tile_base1 = map.d_base1[w0 + t];
        if (hubs) {
            tile_hub = map.d_hub[w0 + t];
            tile_base0 = map.d_base0[w0 + t];
        }
    }
    const int tier = t >> 7, col = t & 127;
    if (col < kLabelSpan && (tier == 0 || hubs)) {
        const long long word = (tier ? xwh : xw1) + col;
        const bool live = col < (RELABEL ? kLabelTileWords + 1 : kLabelTileWords) && word < words;
        const long long at = live ? word : 0;
        unsigned long long m[kLevelMasks];
#pragma unroll
        for (int k = 0; k < kLevelMasks; ++k) m[k] = levels.mask[k][at];
        const unsigned long long vis = d_visited[at];
        const unsigned long long nev = (!RELABEL && d_never) ? d_never[at] : 0ull;  // pre-marked "visited": never discovered
        unsigned long long pl[4] = {0ull, 0ull, 0ull, 0ull}, later = 0ull;
#pragma unroll
        for (int k = kLevelMasks - 1; k >= 0; --k) {  // (last listed bitmap wins)
            const unsigned long long own = (k < valid ? m[k] : 0ull) & ~later;
            later |= own;
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (((k + 1) >> p) & 1) pl[p] |= own;
        }
        const unsigned long long kept = vis & ~nev & ~later;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if ((kCodeWorkLabel >> p) & 1u) pl[p] |= kept;
            if (!live) pl[p] = 0ull;
        }
        planes[tier][2 * col] = LabelPlanes{static_cast<unsigned>(pl[0]), static_cast<unsigned>(pl[1]), static_cast<unsigned>(pl[2]), static_cast<unsigned>(pl[3])};
        planes[tier][2 * col + 1] = LabelPlanes{static_cast<unsigned>(pl[0] >> 32), static_cast<unsigned>(pl[1] >> 32), static_cast<unsigned>(pl[2] >> 32),
                                                static_cast<unsigned>(pl[3] >> 32)};
    }
    if (RELABEL && t < kLabelTileWords) {
        const unsigned e_lo = static_cast<unsigned>(tile_edge), h_lo = static_cast<unsigned>(tile_hub);
        const unsigned x1 = static_cast<unsigned>(map.hubs) + tile_base1;
        s_tier[0][2 * t] = make_uint2(e_lo, x1);
        s_tier[0][2 * t + 1] = make_uint2(static_cast<unsigned>(tile_edge >> 32), x1 + __popc(e_lo));
        s_tier[1][2 * t] = make_uint2(h_lo, tile_base0);
        s_tier[1][2 * t + 1] = make_uint2(static_cast<unsigned>(tile_hub >> 32), tile_base0 + __popc(h_lo));
    }
    __syncthreads();
    // phase 2: one quad (16-byte store) per lane and step, 1 KiB per wave store; the stores of a lane go out together at
    // the end (a store between two steps makes the next step wait for it: its data registers are reused)
    const int sh = (t & 15) * 4;
    const int half = sh >> 5, s5 = sh & 31;
    const unsigned below = (1u << s5) - 1u;
    const unsigned first1 = static_cast<unsigned>(xw1) * 2u, firsth = static_cast<unsigned>(xwh) * 2u;
    constexpr int kSteps = kLabelTileWords / 16;
    int outs[kSteps][4], pouts[PRED ? kSteps : 1][4];
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
        const int wi = i * 16 + (t >> 4);
        const long long w = w0 + wi;
        if (w >= words) continue;
        const long long v0 = w * 64 + sh;
        int(&out)[4] = outs[i];
        unsigned e[4] = {0u, 0u, 0u, 0u};  // the quad's bits of the four planes, at the quad's positions
        unsigned e4 = 0u, h4 = 0u, x1 = 0u, xh = 0u;
        if (RELABEL) {
            const uint2 m1 = s_tier[0][2 * wi + half];
            e4 = (m1.x >> s5) & 0xFu;
            x1 = m1.y + __popc(m1.x & below);
            TiledWindow(planes[0], spread, e4, x1, first1, e);
            if (hubs) {
                const uint2 mh = s_tier[1][2 * wi + half];
                h4 = (mh.x >> s5) & 0xFu;
                xh = mh.y + __popc(mh.x & below);
                TiledWindow(planes[1], spread, h4, xh, firsth, e);
            }
        } else {
            const LabelPlanes c = planes[0][2 * wi + half];
#pragma unroll
            for (int p = 0; p < 4; ++p) e[p] = (c[p] >> s5) & 0xFu;
        }
        // plane p of vertex b at bit 6 p + b; times 0x8421 its four bits meet at bits 15 + b .. 18 + b (no two partial
        // products share a bit, bits 13 + b and 14 + b stay clear): the byte offset into the label table
        const unsigned packed = e[0] | (e[1] << 6) | (e[2] << 12) | (e[3] << 18);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned at = (__umul24(packed & (0x041041u << b), 0x8421u) >> (13 + b)) & 0x3Cu;
            out[b] = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(table) + at);
        }
        int pout[4] = {-2, -2, -2, -2};
        const unsigned work = e[0] & ~e[1] & e[2] & e[3];  // code 13
        const bool src_here = static_cast<unsigned long long>(static_cast<long long>(src) - v0) < 4ull;
        if (work || src_here || PRED) {  // (rare without predecessors)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (RELABEL) {
                    const unsigned lower = (1u << b) - 1u;
                    const bool in1 = (e4 >> b) & 1u, in0 = (h4 >> b) & 1u;
                    const unsigned x = in1 ? x1 + __popc(e4 & lower) : xh + __popc(h4 & lower);
                    if ((work >> b) & 1u) out[b] = d_work_labels[x];
                    if (PRED && (in1 || in0)) {
                        const VertexId p = d_work_preds[x];
                        pout[b] = p >= 0 ? d_old_of_new[p] : p;
                    }
                    if (src == v0 + b && !in1 && !in0) {  // a source without edges
                        out[b] = 0;
                        pout[b] = -1;
                    }
                } else if ((((work >> b) & 1u) || src == v0 + b) && v0 + b < nodes) {
                    out[b] = d_work_labels[v0 + b];  // (the source: Reset wrote its 0)
                }
            }
        }
        if (PRED)
#pragma unroll
            for (int b = 0; b < 4; ++b) pouts[PRED ? i : 0][b] = pout[b];
    }
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
        const long long w = w0 + i * 16 + (t >> 4);
        if (w >= words) continue;
        const long long v0 = w * 64 + sh;
        const int(&out)[4] = outs[i];
        const int(&pout)[4] = pouts[PRED ? i : 0];
        if (v0 + 3 < nodes) {
            __builtin_nontemporal_store(V4{out[0], out[1], out[2], out[3]}, reinterpret_cast<V4 *>(d_labels + v0));
            if (PRED) __builtin_nontemporal_store(V4{pout[0], pout[1], pout[2], pout[3]}, reinterpret_cast<V4 *>(d_preds + v0));
        } else {
            for (int b = 0; b < 4 && v0 + b < nodes; ++b) {
                d_labels[v0 + b] = out[b];
                if (PRED) d_preds[v0 + b] = pout[b];
            }
        }
    }
}

// Static per graph and numbering, what a direction-optimizing search reads besides the CSR: the never-discovered mask, the
// compact heads index and the heads (bottom_up.hpp).  BFSProblem holds one for the caller's numbering and, when it has built
// the relabelled copy, one for the copy; Reset points graph_slices[0] and the DataSlice at the active one.
template <typename VertexId, typename SizeT>
struct SearchGraph {
    SizeT *d_row_offsets = nullptr;  // forward CSR (borrowed)
    VertexId *d_column_indices = nullptr;
    const SizeT *d_inv_row_offsets = nullptr;  // in-neighbour CSR (borrowed)
    const VertexId *d_inv_column_indices = nullptr;
    DeviceArray<unsigned> d_never_mask;  // bit v = v has no in-edge
    DeviceArray<unsigned> d_head_base;   // vertices with in-edges before each 64-vertex word
    DeviceArray<int2> d_inv_heads;       // first two in-neighbours of every vertex with in-edges
    long long with_in_edges = 0;

    void Release()
    {
        d_never_mask.Free();
        d_head_base.Free();
        d_inv_heads.Free();
    }

    // fill the static state from the in-neighbour CSR (synchronous); mask_words: 32-bit words of a vertex bitmap
    hipError_t Build(long long nodes, long long mask_words, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        // Bit v set when v has no in-edge.  Reset preloads the visited bitmap with it, so the bottom-up sweep skips those
        // vertices (half of an R-MAT graph) without touching their row offsets, 64 at a time.
        if (!d_never_mask) GR_CHECK(d_never_mask.Alloc(static_cast<size_t>(mask_words + 2)), "SearchGraph d_never_mask failed");
        if (!d_inv_heads) GR_CHECK(d_inv_heads.Alloc(static_cast<size_t>(nodes)), "SearchGraph d_inv_heads failed");
        const long long words64 = mask_words / 2 + 1;
        long long grid = (words64 + 3) / 4;
        if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL((NoInEdgeMaskKernel<SizeT>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, stream, d_inv_row_offsets, nodes, words64,
                           reinterpret_cast<unsigned long long *>(d_never_mask.p));
        GR_CHECK(hipGetLastError(), "NoInEdgeMaskKernel launch failed");
        // heads are stored only for vertices that have in-edges: d_head_base[w] = such vertices before word w
        if (!d_head_base) GR_CHECK(d_head_base.Alloc(static_cast<size_t>(words64 + 1)), "SearchGraph d_head_base failed");
        DeviceArray<unsigned> d_counts;
        DeviceArray<unsigned long long> d_scan_sums;
        GR_CHECK(d_counts.Alloc(static_cast<size_t>(words64 + 1)), "SearchGraph scratch failed");
        GR_CHECK(d_scan_sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(words64))), "SearchGraph scratch failed");
        hipLaunchKernelGGL(WithInEdgesCountKernel, dim3(static_cast<unsigned>((words64 + 255) / 256)), dim3(256), 0, stream,
                           reinterpret_cast<const unsigned long long *>(d_never_mask.p), nodes, words64, d_counts);
        GR_CHECK(hipGetLastError(), "WithInEdgesCountKernel launch failed");
        GR_CHECK(graphio::DeviceExclusiveScan<unsigned>(d_counts, d_head_base, words64, d_scan_sums, stream), "SearchGraph head-base scan failed");
        GR_CHECK(hipStreamSynchronize(stream), "NoInEdgeMaskKernel failed");
        {   // vertices that have in-edges = last base + last count (sizes the "nearly finished" test of the enactor)
            unsigned last_base = 0, last_count = 0;
            GR_CHECK(hipMemcpy(&last_base, d_head_base + (words64 - 1), sizeof(unsigned), hipMemcpyDeviceToHost), "SearchGraph read failed");
            GR_CHECK(hipMemcpy(&last_count, d_counts + (words64 - 1), sizeof(unsigned), hipMemcpyDeviceToHost), "SearchGraph read failed");
            with_in_edges = static_cast<long long>(last_base) + last_count;
        }
        d_counts.Free();
        d_scan_sums.Free();
        if (nodes > 0) {
            long long hgrid = (nodes + 3) / 4;  // one wave per vertex
            if (hgrid > 8192) hgrid = 8192;
            hipLaunchKernelGGL((oprtr::advance::BuildHeadsKernel<VertexId, SizeT>), dim3(static_cast<unsigned>(hgrid)), dim3(256), 0, stream,
                               d_inv_row_offsets, d_inv_column_indices, nodes, d_inv_heads, d_inv_row_offsets,
                               reinterpret_cast<const unsigned long long *>(d_never_mask.p), d_head_base);
            GR_CHECK(hipGetLastError(), "BuildHeadsKernel launch failed");
            GR_CHECK(hipStreamSynchronize(stream), "BuildHeadsKernel failed");
        }
        return retval;
    }
};

template <typename _VertexId, typename _SizeT, typename _Value, bool _MARK_PREDECESSORS,
          bool _ENABLE_IDEMPOTENCE, bool _USE_DOUBLE_BUFFER>
struct BFSProblem : ProblemBase<_VertexId, _SizeT, _Value, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<_VertexId, _SizeT, _Value, _USE_DOUBLE_BUFFER> Base;
    typedef _VertexId VertexId;
    typedef _SizeT SizeT;
    typedef _Value Value;
    static constexpr bool MARK_PREDECESSORS = _MARK_PREDECESSORS;
    static constexpr bool ENABLE_IDEMPOTENCE = _ENABLE_IDEMPOTENCE;

    struct DataSlice {
        VertexId *d_labels = nullptr;         // depth per vertex, -1 = unreached
        VertexId *d_preds = nullptr;          // parent per vertex (-2 unset, -1 source)
        unsigned *d_visited_mask = nullptr;   // 1 bit per vertex
        VertexId iteration = 0;               // current BSP level (labels written = iteration + 1)
        int lite = 0;                         // 1: count-only level: mark d_fresh[d] with a plain byte store, no claim, no label
        int defer_labels = 0;                 // 1: sweeps in vertex order leave the labels to EmitLabelsKernel (their bitmaps are kept)
        unsigned char *d_fresh = nullptr;     // one byte per vertex, all zero between levels (direction-optimizing only)
        // direction-optimizing traversal (reference app/dobfs: d_frontier_map_in/out, dobfs_problem.cuh):
        unsigned *d_frontier_mask[kLevelMasks] = {};        // 1 bit per vertex: pool of frontier bitmaps (current / next / kept levels)
        unsigned *d_snapshot = nullptr;                     // the visited bitmap as it was before the last top-down level
        unsigned *d_never_mask = nullptr;                   // vertices without in-edges: nothing can ever discover them
        unsigned *d_head_base = nullptr;                    // compacted heads: first entry of every 64-vertex word (bottom_up.hpp)
        int2 *d_inv_heads = nullptr;                        // first two in-neighbours per vertex (bottom_up.hpp)
        const SizeT *d_inv_row_offsets = nullptr;           // in-neighbour CSR (CSC of the graph)
        const VertexId *d_inv_column_indices = nullptr;
    };
    static_assert(std::is_trivially_copyable<DataSlice>::value,
                  "the DataSlice is a kernel argument and is repointed between numberings: views only, the owners sit in the problem");

    // direction-optimizing switches, names from the reference's DOBFS driver (tests/dobfs/test_dobfs.cu:530-534)
    bool direction_optimizing = false;
    float alpha = 10.0f;  // top-down -> bottom-up when frontier_edges * alpha > unexplored_edges (measured optimum 8..14 on R-MAT)
    float beta = 4000.0f; // bottom-up -> top-down when frontier_vertices * beta < nodes (measured at scale-24: 24..200 equal, 1000..4000 a little better;
                          // the reference's vertex rule, dobfs_enactor.cuh:569, with a later switch: sweeps of a nearly finished search are cheap)
    // traversal_mode 1 / low-degree graphs: a frontier of at most kTwcCapacity vertices and this many edges runs in the TWC
    // workgroup (oprtr/advance/twc.hpp); 0 = never
    int twc_edge_limit = 8192;
    // A top-down level runs "count only" (byte stores instead of claims, then bottom-up) when frontier_edges * alpha * lite_factor >
    // unexplored_edges.  700 = practically every level of a direction-optimizing search beyond ~40 K frontier edges at scale-24:
    // a claimed level of 0.3-0.5 M edges costs ~50 us (memory-side atomics at 27 G/s, queue entries, scattered labels, then a read-back,
    // a snapshot copy and a bitmap diff before the sweep), the same level counted costs ~15 us and the sweeps follow without a round
    // trip.  Measured (ms per scale-24 search): 12 -> 0.327, 100 -> 0.319, 500 -> 0.312, 700 -> 0.311, 2000 -> 0.323, 5000 -> 0.346 (then
    // an 11 K-edge level turns bottom-up with a frontier of a few thousand vertices: too early).
    float lite_factor = 700.0f;
    // direction-optimizing: a level that would run count-only or bottom-up and has between min and max frontier edges starts
    // with a heads-only bottom-up pass.  -1 = automatic: edges/30 .. edges/7.8 (measured on R-MAT scale-24: below, the plain
    // count-only level is cheaper; above, the frontier is dense enough for the full bottom-up sweep to win); min 0 = never,
    // max 0 = no upper bound.
    int head_pass_min_edges = -1;
    int head_pass_max_edges = -1;
    long long with_in_edges = 0;  // vertices that have in-edges (only they can ever be discovered bottom-up)
    // a bottom-up level runs the compacting sweep (BottomUpSparseKernel) when at most nodes / sparse_sweep_div such vertices
    // can still be unvisited (0 = never)
    int sparse_sweep_div = 6;  // (measured at scale-24 with 64-word chunks: 16 -> 0.348, 8 -> 0.324, 6 -> 0.321, 4 -> 0.326, 2 -> 0.45 ms per search)
    // ... and that sweep also writes its finds as the next top-down queue when its input frontier is within this factor of the
    // switch-back threshold (frontier * beta < factor * nodes): the switch then needs no bitmap -> queue pass
    float emit_queue_factor = 128.0f;
    bool chain_closing = true;     // the closing top-down levels (and the label pass) are queued behind a chain of sweeps, gated on the device
    bool speculative_emit = true;  // deferred labels: the emit pass is queued right behind the closing top-down launch
    int chain_sweeps = 4;          // bottom-up sweeps queued per host round trip (BottomUpAutoKernel decides on the device what each
                                   // of them does); 0 = one sweep per round trip, chosen by the host
    long long HeadPassMin() const { return head_pass_min_edges >= 0 ? head_pass_min_edges : static_cast<long long>(this->edges) / 30 + 1; }
    long long HeadPassMax() const
    {
        if (head_pass_max_edges > 0) return head_pass_max_edges;
        if (head_pass_max_edges == 0) return 1ll << 40;
        return static_cast<long long>(static_cast<double>(this->edges) / 7.8);
    }
    // Top-down levels with at least this many frontier edges run as a destination-binned advance (oprtr/advance/binned.hpp):
    // expand + screen, claims on the destination's owner XCD without atomics, then a vertex-ordered closing sweep
    // (FreshToBitmapKernel + BitmapToQueueKernel) that labels, dedupes and enqueues.  0 = never.
    long long binned_min_edges = 1ll << 23;
    oprtr::advance::BinPoolStorage<VertexId> bin_pool;
    bool cooperative_launch = false;  // persistent levels kernel through hipLaunchCooperativeKernel (launch-time residency check)
    int persistent_edge_limit = 1 << 20;  // ... and up to this many inside the persistent multi-workgroup kernel (0 = off)
    int tail_edge_limit = 8192;  // levels with at most this many edge slots run inside the single-workgroup tail kernel

    SliceHolder<DataSlice> data_slices;   // host copy (a by-value kernel argument)
    DataSlice **d_data_slices = nullptr;  // kept for source compatibility; unused (no device-side struct)
    // what the slice views, under the slice's names (d_labels and d_preds view d_out_* or d_work_* below)
    DeviceArray<unsigned> d_visited_mask, d_frontier_mask[kLevelMasks], d_snapshot;
    DeviceArray<unsigned char> d_fresh;

    // bitmaps are sized in whole 64-bit words: one wave owns one word in the bottom-up sweep
    SizeT MaskWords() const { return ((this->nodes + 63) / 64) * 2; }

    // ---- two numberings of one graph (graphio/relabel.hpp, DESIGN §3.3 k) ----
    // numbering[0]: the caller's; numbering[1]: the hub-first, edgeless-last copy a symmetric problem builds in InverseIsSelf.
    // Kernels only ever see the active one: from Reset on, graph_slices[0] and the DataSlice point at it, labels and
    // predecessors are worked in d_work_* in its numbering, and the closing label pass (TranslateLabelsKernel) writes the
    // caller-order results into d_out_*, the arrays device_results() hands out.
    SearchGraph<VertexId, SizeT> numbering[2];
    graphio::RelabelledCsr relabelled;
    int relabel = -1;                 // policy (effective at the next Reset): 1 search the relabelled copy, 0 the caller's numbering,
                                      // -1 the copy on graphs of at least relabel_min_nodes vertices
    long long relabel_min_nodes = 1ll << 23;  // (scale-22 R-MAT: the label pass costs more than the sweeps save, DESIGN §3.3 k)
    long long relabel_hubs = 65536;   // size limit of the hub tier (0: two tiers, with edges / without).  65536 = the ids an 8 KiB hub slice of the
                                      // frontier bitmap answers from LDS (hub_slice below, DESIGN §3.3 n)
    // ids the dense bottom-up sweeps answer from an LDS copy of the frontier bitmap's first words (bottom_up.hpp HubSliceLookup,
    // DESIGN §3.3 n); read at every launch.  -1: the copy's hub tier while a search runs on the copy, nothing in the caller's
    // numbering; 0: off.  Whatever is asked for, HubSlice() caps it by the LDS array and by the bitmap.
    long long hub_slice = -1;
    unsigned HubSlice() const
    {
        long long ids = hub_slice >= 0 ? hub_slice : (active == 1 ? relabelled.hubs : 0);
        const long long cap = static_cast<long long>(oprtr::advance::kHubSliceWords) * 32;
        const long long bitmap = static_cast<long long>(MaskWords()) * 32;
        if (ids > cap) ids = cap;
        if (ids > bitmap) ids = bitmap;
        return static_cast<unsigned>(ids < 0 ? 0 : ids);
    }
    bool build_relabelled = false;    // policy: InverseIsSelf builds the copy (the one-shot entry point leaves it off)
    int active = 0;                   // state: numbering of the running search
    bool translate_pending = false;   // state: a non-deferred search on the copy still owes its caller-order pass
    VertexId caller_source = -1;      // the source in the caller's numbering (`source` is in the active one)
    DeviceArray<VertexId> d_out_labels, d_out_preds;    // results, caller order
    DeviceArray<VertexId> d_work_labels, d_work_preds;  // the copy's numbering (allocated with the copy)

    // (re)build the relabelled copy of a symmetric problem with at most `hubs` vertices in the hub tier
    hipError_t BuildRelabelled(long long hubs)
    {
        hipError_t retval = hipSuccess;
        hipStream_t stream = this->graph_slices[0]->stream;
        if (!direction_optimizing || numbering[0].d_inv_row_offsets != numbering[0].d_row_offsets)
            return util::GRError(hipErrorInvalidValue, "BFSProblem: the relabelled copy needs a symmetric graph (InverseIsSelf)", __FILE__, __LINE__);
        GR_CHECK(hipStreamSynchronize(stream), "BFSProblem sync failed");
        if (active == 1) UseNumbering(0);  // (the next Reset picks the new copy up)
        numbering[1].Release();
        GR_CHECK(relabelled.Build(this->nodes, this->edges, numbering[0].d_row_offsets, numbering[0].d_column_indices, hubs < 0 ? 0 : hubs,
                                  MARK_PREDECESSORS, stream),
                 "BFSProblem relabel build failed");
        numbering[1].d_row_offsets = relabelled.d_row_offsets;
        numbering[1].d_column_indices = relabelled.d_cols;
        numbering[1].d_inv_row_offsets = relabelled.d_row_offsets;
        numbering[1].d_inv_column_indices = relabelled.d_cols;
        GR_CHECK(numbering[1].Build(this->nodes, MaskWords(), stream), "BFSProblem relabelled static state failed");
        const size_t n = static_cast<size_t>(this->nodes);
        if (!d_work_labels) GR_CHECK(d_work_labels.Alloc(n), "BFSProblem work labels failed");
        if (MARK_PREDECESSORS && !d_work_preds) GR_CHECK(d_work_preds.Alloc(n), "BFSProblem work preds failed");
        relabel_hubs = hubs;
        return retval;
    }
    bool HasRelabelled() const { return relabelled.Ready() && numbering[1].d_never_mask != nullptr; }
    bool RelabelActive() const
    {
        return HasRelabelled() && (relabel > 0 || (relabel < 0 && static_cast<long long>(this->nodes) >= relabel_min_nodes));
    }
    // id of caller vertex v in the numbering the kernels see
    VertexId SearchId(VertexId v) const { return (active == 1 && v >= 0 && v < this->nodes) ? static_cast<VertexId>(relabelled.NewId(v)) : v; }

    // point the kernels' view (graph slice, DataSlice, with_in_edges) at numbering k
    void UseNumbering(int k)
    {
        DataSlice *ds = data_slices[0];
        GraphSlice<VertexId, SizeT, Value> *gs = this->graph_slices[0];
        active = k;
        const SearchGraph<VertexId, SizeT> &g = numbering[k];
        gs->d_row_offsets = g.d_row_offsets;
        gs->d_column_indices = g.d_column_indices;
        ds->d_inv_row_offsets = g.d_inv_row_offsets;
        ds->d_inv_column_indices = g.d_inv_column_indices;
        ds->d_never_mask = g.d_never_mask;
        ds->d_head_base = g.d_head_base;
        ds->d_inv_heads = g.d_inv_heads;
        with_in_edges = g.with_in_edges;
        ds->d_labels = k == 1 ? d_work_labels : d_out_labels;
        ds->d_preds = k == 1 ? d_work_preds : d_out_preds;
    }

    // Enable direction-optimizing traversal.  The in-neighbour CSR must stay valid while the problem lives;
    // for an undirected (symmetric) graph pass the problem's own device arrays (InverseIsSelf()).
    hipError_t SetInverseGraph(const SizeT *d_inv_row_offsets, const VertexId *d_inv_column_indices,
                               float alpha_ = 0.0f, float beta_ = 0.0f)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if (active != 0) UseNumbering(0);  // (a new inverse: the caller's numbering again, the copy is dropped below)
        relabelled.Release();
        numbering[1].Release();
        numbering[0].d_row_offsets = this->graph_slices[0]->d_row_offsets;
        numbering[0].d_column_indices = this->graph_slices[0]->d_column_indices;
        numbering[0].d_inv_row_offsets = d_inv_row_offsets;
        numbering[0].d_inv_column_indices = d_inv_column_indices;
        for (int i = 0; i < kLevelMasks; ++i) GR_CHECK(EnsureMask(i), "BFSProblem d_frontier_mask failed");
        if (!ds->d_snapshot) {
            GR_CHECK(d_snapshot.Alloc(static_cast<size_t>(MaskWords() + 2)), "BFSProblem d_snapshot failed");
            ds->d_snapshot = d_snapshot;
        }
        GR_CHECK(EnsureFresh(), "BFSProblem d_fresh failed");
        GR_CHECK(numbering[0].Build(static_cast<long long>(this->nodes), MaskWords(), this->graph_slices[0]->stream),
                 "BFSProblem static search state failed");
        UseNumbering(0);

        if (alpha_ > 0) alpha = alpha_;
        if (beta_ > 0) beta = beta_;
        direction_optimizing = true;
        return retval;
    }
    // bitmap i of the pool, allocated at the first request
    hipError_t EnsureMask(int i)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if (ds->d_frontier_mask[i]) return retval;
        if ((retval = d_frontier_mask[i].Alloc(static_cast<size_t>(MaskWords() + 2)))) return retval;
        ds->d_frontier_mask[i] = d_frontier_mask[i];
        return retval;
    }
    // ... and the flag bytes of the count-only and binned levels, all zero from here on
    hipError_t EnsureFresh()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if (ds->d_fresh) return retval;
        const size_t bytes = (static_cast<size_t>(this->nodes) + 1023) / 1024 * 1024 + 1024;  // FreshToBitmapKernel reads 1 KiB steps
        if ((retval = d_fresh.Alloc(bytes))) return retval;
        GR_CHECK(hipMemset(d_fresh, 0, bytes), "BFSProblem hipMemset d_fresh failed");  // levels leave it zero again
        GR_CHECK(hipDeviceSynchronize(), "BFSProblem sync failed");  // (null-stream memset: the problem's stream is not ordered behind it)
        ds->d_fresh = d_fresh;
        return retval;
    }
    // Scratch of the binned advance: the chunk pool (sized for a level that hands over every edge of the graph from
    // `workgroups` workgroups), the flag bytes and the bitmap its closing sweep writes.  Allocated on first use.
    hipError_t EnsureBinned(int workgroups, int *d_overflow)
    {
        hipError_t retval = hipSuccess;
        if (!bin_pool.Ready() || bin_pool.workgroups < workgroups)
            GR_CHECK(bin_pool.Allocate(static_cast<long long>(this->edges), workgroups, MARK_PREDECESSORS, d_overflow),
                     "BFSProblem bin pool allocation failed");
        GR_CHECK(EnsureFresh(), "BFSProblem d_fresh failed");
        GR_CHECK(EnsureMask(0), "BFSProblem d_frontier_mask failed");
        return retval;
    }

    // The graph is its own inverse (symmetric).  With build_relabelled set, this also builds the relabelled copy that Reset
    // searches while `relabel` is on.
    hipError_t InverseIsSelf(float alpha_ = 0.0f, float beta_ = 0.0f)
    {
        hipError_t retval = hipSuccess;
        if (active != 0) UseNumbering(0);
        GR_CHECK(SetInverseGraph(this->graph_slices[0]->d_row_offsets, this->graph_slices[0]->d_column_indices, alpha_, beta_),
                 "BFSProblem SetInverseGraph failed");
        // the copy is optional: when it cannot be built (device memory for the sort scratch), the searches keep the caller's numbering
        if (build_relabelled && this->nodes > 0 && BuildRelabelled(relabel_hubs) != hipSuccess) {
            hipGetLastError();  // (clear the report of the failed allocation)
            relabelled.Release();
            numbering[1].Release();
            if (active != 0) UseNumbering(0);
        }
        return retval;
    }

    hipError_t AllocData()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices.Make();
        // (a second Init: the new slice views nothing yet, so what the first one viewed goes)
        for (int i = 0; i < kLevelMasks; ++i) d_frontier_mask[i].Free();
        d_snapshot.Free();
        d_fresh.Free();
        const size_t n = static_cast<size_t>(this->nodes);
        GR_CHECK(d_out_labels.Alloc(n), "BFSProblem d_labels failed");
        if (MARK_PREDECESSORS) GR_CHECK(d_out_preds.Alloc(n), "BFSProblem d_preds failed");
        ds->d_labels = d_out_labels;
        ds->d_preds = d_out_preds;
        GR_CHECK(d_visited_mask.Alloc(static_cast<size_t>(MaskWords() + 2)), "BFSProblem d_visited_mask failed");
        ds->d_visited_mask = d_visited_mask;
        return retval;
    }

    hipError_t Init(bool stream_from_host, const Csr<VertexId, Value, SizeT> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus))) return retval;
        return AllocData();
    }

    hipError_t InitFromDevice(SizeT nodes, SizeT edges, SizeT *d_row_offsets, VertexId *d_column_indices)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        return AllocData();
    }

    // One fused kernel (labels = -1, preds = -2, visited = 0, source seeded, queue seeded) and one 8-byte read-back of
    // the source's row extent -- the reference issues 3 <<<128,128>>> memsets and 3-4 tiny H2D copies (:298-357).
    hipError_t Reset(VertexId src, FrontierType frontier_type, double queue_sizing)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Reset(frontier_type, queue_sizing))) return retval;
        GraphSlice<VertexId, SizeT, Value> *gs = this->graph_slices[0];
        DataSlice *ds = data_slices[0];
        hipStream_t stream = gs->stream;
        if (!h_src_box) {
            GR_CHECK(h_src_box.Alloc(1), "BFSProblem source box failed");
            h_src_box->seq = 0;
        }
        // the numbering of this search: the relabelled copy while `relabel` is on and the copy exists
        if (direction_optimizing) UseNumbering(RelabelActive() ? 1 : 0);
        caller_source = src;
        if (active == 1 && src >= 0 && src < this->nodes) src = static_cast<VertexId>(relabelled.NewId(src));  // (host copies of the masks)
        ds->iteration = 0;
        ds->defer_labels = 0;
        // direction-optimizing problems defer the labels of their vertex-ordered sweeps: no fill here, one pass at the end of Enact
        labels_deferred = direction_optimizing && defer_labels;
        level_masks.count = 0;
        mask_ring = 0;
        emit_current = false;
        const bool valid = src >= 0 && src < this->nodes;
        const long long work = (static_cast<long long>(this->nodes) + 3) / 4;
        long long grid = (work + 255) / 256;
        if (grid > 2048) grid = 2048;
        if (grid < 1) grid = 1;
        ++reset_seq;
        if (!util::WorkProgress::IsLive(arm_progress)) arm_progress = nullptr;  // (that enactor is gone)
        hipLaunchKernelGGL((BfsResetKernel<VertexId, SizeT, MARK_PREDECESSORS>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, stream,
                           ds->d_labels, ds->d_preds, ds->d_visited_mask, direction_optimizing ? ds->d_never_mask : nullptr,
                           direction_optimizing ? ds->d_snapshot : nullptr, labels_deferred ? 0 : 1, static_cast<long long>(this->nodes),
                           static_cast<long long>(MaskWords() + 2), valid ? src : static_cast<VertexId>(-1), gs->d_row_offsets,
                           gs->frontier_queues[0], h_src_box->row, &h_src_box->seq, reset_seq,
                           arm_progress ? arm_progress->d_tail : nullptr, arm_progress ? arm_progress->d_overflow : nullptr,
                           arm_progress ? arm_progress->d_wide : nullptr, arm_progress ? arm_progress->d_chain_log : nullptr);
        GR_CHECK(hipGetLastError(), "BfsResetKernel launch failed");
        armed_progress = arm_progress;  // (the enactor that finds its own words armed skips its arming kernel)
        // No synchronisation here: everything that follows runs on the same stream, and SourceDegree() waits for the one
        // host-visible result (the source's row, which the kernel writes first).
        src_row[0] = src_row[1] = 0;
        src_row_pending = valid;
        source = src;
        translate_pending = active == 1 && !labels_deferred;
        return retval;
    }

    // Degree of the source, known after Reset (seeds the first packed tail).
    SizeT SourceDegree()
    {
        if (src_row_pending) {
            volatile unsigned long long *flag = &h_src_box->seq;
            unsigned spins = 0, idle_checks = 0;
            while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != reset_seq) {
                if ((++spins & 0x3FFu) == 0) {
                    const hipError_t rc = hipStreamQuery(this->graph_slices[0]->stream);
                    if (rc != hipSuccess && rc != hipErrorNotReady) {  // the reset kernel failed: report a zero-degree source
                        util::GRError(rc, "BFSProblem Reset kernel failed", __FILE__, __LINE__);
                        break;
                    }
                    if (rc == hipSuccess && ++idle_checks > 1000) break;  // stream drained and still no word: give up (degree 0)
                }
            }
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == reset_seq) {
                src_row[0] = h_src_box->row[0];
                src_row[1] = h_src_box->row[1];
            }
            src_row_pending = false;
        }
        return src_row[1] - src_row[0];
    }

    hipError_t Extract(VertexId *h_labels, VertexId *h_preds)
    {
        hipError_t retval = hipSuccess;
        hipStream_t stream = this->graph_slices[0]->stream;
        GR_CHECK(FinishSearch(stream), "BFSProblem Extract: label pass failed");  // (no-op after an Enact: it ends with this pass)
        GR_CHECK(hipStreamSynchronize(stream), "BFSProblem Extract sync failed");
        if (this->nodes > 0)
            GR_CHECK(hipMemcpy(h_labels, d_out_labels, sizeof(VertexId) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost),
                     "BFSProblem hipMemcpy d_labels failed");
        if (MARK_PREDECESSORS && h_preds && this->nodes > 0)
            GR_CHECK(hipMemcpy(h_preds, d_out_preds, sizeof(VertexId) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost),
                     "BFSProblem hipMemcpy d_preds failed");
        return retval;
    }

    // ---- deferred labels: the kept level bitmaps of the running search ----
    bool defer_labels = true;       // policy (off: every kernel labels at discovery, Reset fills -1)
    bool emit_current = false;      // state: a speculative emit pass has run and no vertex has been discovered since
    bool labels_deferred = false;   // state: d_labels is incomplete until EmitLabels has run (set by Reset, cleared by EmitLabels)
    int label_pass = 1;             // policy, read at every launch: 1 the tiled closing pass (TiledLabelsKernel), 0 the per-lane kernels
    int walk_queue = 1;             // policy, read at every launch: 1 the dense bottom-up sweep queues its row walks per wave (bottom_up.hpp
                                    // DenseSweepQueued), 0 it walks them step by step (DenseSweep)
    int fused_publish = 1;          // policy, read at every Enact: 1 the read-back behind a queued tiled label pass is published by that pass
                                    // (workgroup 0, frontier.hpp PublishBody), 0 by a PublishKernel behind it
    int level_mask_limit = kLevelMasks;  // bitmaps of the pool a search may use (tests shrink it to force mid-search flushes)
    LevelMaskList<VertexId> level_masks; // (bitmap, label) of every kept level
    int mask_ring = 0;

    bool MaskKept(int idx) const
    {
        for (int k = 0; k < level_masks.count; ++k)
            if (level_masks.mask[k] == reinterpret_cast<const unsigned long long *>(data_slices[0]->d_frontier_mask[idx])) return true;
        return false;
    }
    // A bitmap of the pool that is neither kept nor one of the (up to two) the caller is still reading.  When every other one
    // is kept, the kept levels are flushed into d_labels first (partial stores -- the price the deferral normally avoids).
    hipError_t AcquireMask(hipStream_t stream, int &idx, int hold_a = -1, int hold_b = -1)
    {
        const int holds[2] = {hold_a, hold_b};
        bool got = false;
        const hipError_t rc = TryAcquireMask(stream, idx, holds, 2, got);
        if (rc) return rc;
        return got ? hipSuccess : util::GRError(hipErrorInvalidValue, "BFSProblem: no free frontier bitmap", __FILE__, __LINE__);
    }
    // the same with any number of bitmaps held; got = false when even a flush of the kept levels frees none
    hipError_t TryAcquireMask(hipStream_t stream, int &idx, const int *holds, int n_holds, bool &got)
    {
        hipError_t retval = hipSuccess;
        got = true;
        if (!data_slices[0]->d_frontier_mask[1]) {  // no pool (no inverse graph): the binned level's single bitmap
            idx = 0;
            return retval;
        }
        const int limit = level_mask_limit < 4 ? 4 : (level_mask_limit > kLevelMasks ? kLevelMasks : level_mask_limit);
        for (int round = 0; round < 2; ++round) {
            for (int t = 0; t < limit; ++t) {
                const int cand = (mask_ring + t) % limit;
                bool held = false;
                for (int h = 0; h < n_holds; ++h) held = held || holds[h] == cand;
                if (held || MaskKept(cand)) continue;
                idx = cand;
                mask_ring = (cand + 1) % limit;
                return retval;
            }
            if (level_masks.count == 0) break;  // nothing to flush: the holds alone fill the pool
            GR_CHECK(FlushLevelMasks(stream), "BFSProblem FlushLevelMasks failed");
        }
        got = false;
        return retval;
    }
    void KeepMask(int idx, VertexId label)
    {
        level_masks.mask[level_masks.count] = reinterpret_cast<const unsigned long long *>(data_slices[0]->d_frontier_mask[idx]);
        level_masks.label[level_masks.count] = label;
        ++level_masks.count;
    }
    // publish: the enactor's pending read-back, carried by the tiled pass (TiledPassReady says beforehand whether the launch
    // will be one); every other kernel here ignores it
    template <bool FULL>
    hipError_t LaunchEmit(hipStream_t stream, VertexId src, const util::PublishArgs *publish = nullptr)
    {
        DataSlice *ds = data_slices[0];
        const util::PublishArgs carried = (FULL && publish) ? *publish : util::PublishArgs();
        long long grid = ((static_cast<long long>(this->nodes) + 3) / 4 + 255) / 256;  // one quad of vertices per thread
        if (grid > (1 << 20)) grid = 1 << 20;
        if (grid < 1) grid = 1;
        LevelMaskList<VertexId> list = level_masks;
        // (one instantiation per list length up to 8: every extra bitmap is one more load per lane of a pass that is all loads and stores)
        const int kmax = list.count <= 8 ? list.count : kLevelMasks;
        for (int k = list.count; k < kmax; ++k) {  // padding: entry 0 again
            list.mask[k] = list.mask[0];
            list.label[k] = list.label[0];
        }
        const unsigned long long *vis = reinterpret_cast<const unsigned long long *>(ds->d_visited_mask);
        const unsigned long long *nev = reinterpret_cast<const unsigned long long *>(ds->d_never_mask);
        const long long n = static_cast<long long>(this->nodes);
        const dim3 g(static_cast<unsigned>(grid)), b(256);
        if (FULL && label_pass != 0) {  // the tiled pass: one kernel for every list length, either numbering
            const bool copy = active == 1;
            for (int k = list.count; k < kLevelMasks; ++k) {  // (entries past the count are loaded and not looked at)
                list.mask[k] = list.count > 0 ? list.mask[0] : vis;
                list.label[k] = -1;
            }
            const long long tiles = ((n + 63) / 64 + kLabelTileWords - 1) / kLabelTileWords;
            const dim3 tg(static_cast<unsigned>(tiles > 0 ? tiles : 1));
            if (copy) {
                const VertexId csrc = (caller_source >= 0 && caller_source < this->nodes) ? caller_source : static_cast<VertexId>(-1);
                hipLaunchKernelGGL((TiledLabelsKernel<VertexId, true, MARK_PREDECESSORS>), tg, b, 0, stream, list, vis, nev, relabelled.View(), n, csrc,
                                   d_work_labels, d_work_preds, relabelled.d_old_of_new, d_out_labels, d_out_preds, carried);
                translate_pending = false;
            } else {
                hipLaunchKernelGGL((TiledLabelsKernel<VertexId, false, false>), tg, b, 0, stream, list, vis, nev, graphio::RelabelView(), n, src,
                                   ds->d_labels, nullptr, nullptr, ds->d_labels, nullptr, carried);
            }
            level_masks.count = 0;
            return util::GRError(hipGetLastError(), "TiledLabelsKernel launch failed", __FILE__, __LINE__);
        }
        if (FULL && active == 1) {  // the search ran on the relabelled copy: the pass writes the caller's order
            const graphio::RelabelView map = relabelled.View();
            const VertexId csrc = (caller_source >= 0 && caller_source < this->nodes) ? caller_source : static_cast<VertexId>(-1);
            const VertexId *o2n = relabelled.d_old_of_new;
#define GRX_TRANSLATE_CASE(K) case K: hipLaunchKernelGGL((TranslateLabelsKernel<VertexId, K, MARK_PREDECESSORS>), g, b, 0, stream, list, vis, map, n, csrc, \
                                                          d_work_labels, d_work_preds, o2n, d_out_labels, d_out_preds); break;
            switch (kmax) {
                GRX_TRANSLATE_CASE(0) GRX_TRANSLATE_CASE(1) GRX_TRANSLATE_CASE(2) GRX_TRANSLATE_CASE(3) GRX_TRANSLATE_CASE(4) GRX_TRANSLATE_CASE(5)
                GRX_TRANSLATE_CASE(6) GRX_TRANSLATE_CASE(7) GRX_TRANSLATE_CASE(8)
                default: hipLaunchKernelGGL((TranslateLabelsKernel<VertexId, kLevelMasks, MARK_PREDECESSORS>), g, b, 0, stream, list, vis, map, n, csrc,
                                            d_work_labels, d_work_preds, o2n, d_out_labels, d_out_preds);
            }
#undef GRX_TRANSLATE_CASE
            level_masks.count = 0;
            translate_pending = false;
            return util::GRError(hipGetLastError(), "TranslateLabelsKernel launch failed", __FILE__, __LINE__);
        }
#define GRX_EMIT_CASE(K) case K: hipLaunchKernelGGL((EmitLabelsKernel<VertexId, FULL, K>), g, b, 0, stream, list, vis, nev, n, src, ds->d_labels); break;
        switch (kmax) {
            GRX_EMIT_CASE(0) GRX_EMIT_CASE(1) GRX_EMIT_CASE(2) GRX_EMIT_CASE(3) GRX_EMIT_CASE(4) GRX_EMIT_CASE(5) GRX_EMIT_CASE(6) GRX_EMIT_CASE(7)
            GRX_EMIT_CASE(8)
            default: hipLaunchKernelGGL((EmitLabelsKernel<VertexId, FULL, kLevelMasks>), g, b, 0, stream, list, vis, nev, n, src, ds->d_labels);
        }
#undef GRX_EMIT_CASE
        level_masks.count = 0;
        return util::GRError(hipGetLastError(), "EmitLabelsKernel launch failed", __FILE__, __LINE__);
    }
    // Would EmitLabelsGated (with `extra` chain bitmaps) or EmitLabelsSpeculative (extra = 0) queue the tiled pass now?
    bool TiledPassReady(int extra) const
    {
        return labels_deferred && speculative_emit && label_pass != 0 && level_masks.count + extra <= kLevelMasks;
    }
    long long mask_flushes = 0;  // kept bitmaps flushed in the middle of a search (counted over the problem's life)
    hipError_t FlushLevelMasks(hipStream_t stream)
    {
        if (level_masks.count == 0) return hipSuccess;
        ++mask_flushes;
        return LaunchEmit<false>(stream, static_cast<VertexId>(-1));
    }
    // What every Enact ends with (and Extract, for a search that was reset but not run): the deferred label pass, or, for a
    // search on the relabelled copy that labelled at discovery, the pass that brings its results into the caller's order.
    // launched (when given): did it queue a kernel?
    hipError_t FinishSearch(hipStream_t stream, bool *launched = nullptr)
    {
        if (launched) *launched = (labels_deferred && !emit_current) || (!labels_deferred && translate_pending);
        if (labels_deferred) return EmitLabels(stream);
        if (!translate_pending) return hipSuccess;
        level_masks.count = 0;
        return LaunchEmit<true>(stream, source);
    }
    // The closing pass of a search whose Reset left the labels unfilled.
    hipError_t EmitLabels(hipStream_t stream)
    {
        if (!labels_deferred) return hipSuccess;
        labels_deferred = false;
        if (emit_current) {  // a speculative pass already wrote them and nothing was discovered since
            emit_current = false;
            level_masks.count = 0;
            return hipSuccess;
        }
        return LaunchEmit<true>(stream, (source >= 0 && source < this->nodes) ? source : static_cast<VertexId>(-1));
    }
    // The same pass queued BEFORE the host knows that the search is over (behind the launch that usually ends it): the kept
    // bitmaps and the deferral stay as they are, so that a search that does go on simply ends with another pass -- the first
    // one wrote nothing wrong (labels of levels that existed), the second one covers the rest.  The caller clears emit_current
    // when anything is discovered after this.
    // ... and the same pass queued behind a CHAIN of sweeps and the closing levels that follow it on the device
    // (kernel.hpp ChainedPersistentLevelsKernel): the chain's bitmaps go in as candidates, the gate words say how many were filled
    hipError_t EmitLabelsGated(hipStream_t stream, const int *chain_masks, const VertexId *chain_labels, int chain_count, const int *d_gate,
                               const util::PublishArgs *publish = nullptr)
    {
        if (!labels_deferred || !speculative_emit) return hipSuccess;
        if (level_masks.count + chain_count > kLevelMasks) return hipSuccess;  // (no room in the list: the ordinary pass will do)
        const LevelMaskList<VertexId> keep = level_masks;
        level_masks.chain_first = level_masks.count;
        for (int k = 0; k < chain_count; ++k) KeepMask(chain_masks[k], chain_labels[k]);
        level_masks.d_gate = d_gate;
        const hipError_t rc = LaunchEmit<true>(stream, (source >= 0 && source < this->nodes) ? source : static_cast<VertexId>(-1), publish);
        level_masks = keep;
        return rc;
    }
    hipError_t EmitLabelsSpeculative(hipStream_t stream, const util::PublishArgs *publish = nullptr)
    {
        if (!labels_deferred || !speculative_emit) return hipSuccess;
        const LevelMaskList<VertexId> keep = level_masks;
        const hipError_t rc = LaunchEmit<true>(stream, (source >= 0 && source < this->nodes) ? source : static_cast<VertexId>(-1), publish);
        level_masks = keep;
        emit_current = true;
        return rc;
    }

    // the enactor words Reset arms (set by the enactor at its first Enact on this problem; must outlive the problem's searches)
    util::WorkProgress *arm_progress = nullptr;
    util::WorkProgress *armed_progress = nullptr;  // whose words the last Reset armed (nullptr: nobody's)

    VertexId source = -1;
    SizeT src_row[2] = {0, 0};
    struct SourceBox {
        unsigned long long seq;
        SizeT row[2];
    };
    util::PinnedArray<SourceBox, hipHostMallocMapped> h_src_box;  // pinned + mapped: written by BfsResetKernel
    unsigned long long reset_seq = 0;
    bool src_row_pending = false;
};

}  // namespace bfs
}  // namespace app
}  // namespace gunrock
