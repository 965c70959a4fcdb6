// app/bcc/bcc_functor.hpp -- device kernels of the biconnected components, articulation points, bridges and 2-edge-connected
// components (Tarjan-Vishkin on a BFS forest).
//
// The reference snapshot has no app/bcc (later Gunrock releases do); the shape follows this tree's primitives: truss's neighbour
// CSR with the canonical edge id on every entry, k-core's one queue with the levels as ranges of it, SCC's one-workgroup device
// loop and its canonical-id pair MergeKernel / GatherKernel (scc_functor.hpp is included, not changed).
//
// The run, on the simple undirected graph G:
//   forest     comp[] by hook-and-jump over the canonical edges (the smaller id wins, so a root is its component's minimum); every
//              vertex with comp[v] == v and a neighbour is a root, and one level-synchronous search from all of them claims
//              parent[] by CAS.  One queue holds every reached vertex once; bounds[L] .. bounds[L + 1] is level L.
//   sizes      bottom-up by level, pull form: size[v] = 1 + the sizes of the row entries whose parent is v.  No atomics.
//   numbering  top-down: a tree takes size[root] numbers from a cursor; v gives its children, in row order, pre[v] + 1 + the
//              exclusive prefix of their sizes.
//   low/high   bottom-up: the smallest and the largest pre[] that the subtree of v or a non-tree edge out of it reaches.
//   link       tree edge (parent[v], v) is a bridge iff low[v] >= pre[v] and high[v] < pre[v] + size[v]; a union-find over the non-root
//              vertices (v stands for its tree edge) joins the ends of a non-tree edge when neither is in the other's subtree, and
//              v with its child w when low[w] < pre[v] or high[w] >= pre[v] + size[v].
//   label      an edge's set is its child end's (tree edge) or the end with the larger pre (non-tree edge); the smallest edge id per
//              set names the block.  Articulation points come from the labels only (a local low/high test is wrong on a forest
//              with cross edges); the 2-edge-connected components are the forest with its bridges cut, pointer-jumped.
// A level is a STEP: a wide launch (StepKernel), or one of a stretch of steps inside a one-workgroup loop on the device, which puts
// a fence and a barrier between steps and uses agent-scope accesses on everything one step leaves for the next (its CU's L1 is not
// refreshed by what lands in L2).
#pragma once

#include <hip/hip_runtime.h>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // (only SCC's canonical-id kernels are used here)
#include <gunrock/app/scc/scc_functor.hpp>
#pragma clang diagnostic pop
#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace bcc {

enum { BCC_AUTO = 0, BCC_ROUNDS = 1, BCC_DEVICE_LOOP = 2 };
enum { PHASE_FOREST = 0, PHASE_SIZES, PHASE_NUMBER, PHASE_LOWHIGH, PHASE_LINK, PHASE_LABEL, PHASE_COUNT };

constexpr int kBccThreads = 256;
constexpr int kUnseen = -2;                  // parent[]: not reached (-1: a root, or a vertex without a neighbour)

using oprtr::kLoopMaxSteps;
using oprtr::kLoopThreads;
using oprtr::Ld;
using oprtr::Limits;
using oprtr::Narrow;
using oprtr::St;
using oprtr::TileFor;

// the words the forest's kernels and the host share: none is reset during a run
enum {
    W_TAIL = 0,  // queue tickets handed out
    W_ENTRIES,   // row entries of the vertices queued so far, modulo 2^32
    W_CURSOR,    // preorder numbers handed to trees
    W_COUNT = 4
};

enum { K_FOREST = 0, K_SIZES, K_NUMBER, K_LOWHIGH };

struct Ctx {
    const int *ro, *ci, *eid;  // the neighbour CSR of G, rows ascending, and the edge of every entry
    int *parent, *level, *pedge, *size, *pre, *low, *high;
    int *queue;                // every vertex with a neighbour once, level by level
    int *bounds;               // level L is queue[bounds[L] .. bounds[L + 1])
    unsigned *ents;            // ents[L + 1] - ents[L]: the row entries of level L
    unsigned *words;
    unsigned long long *reads;  // row entries walked
    int nodes;
    int wave_min_row;
};

// the forest's next level; the host and ForestLoopKernel carry the same
struct Front {
    int level;
    unsigned head, tail;
    unsigned entries_seen;  // W_ENTRIES when the level was complete
    unsigned step_entries;  // row entries of [head, tail)
};

struct Tally {
    unsigned entries = 0;  // row entries of the vertices this lane queued
    unsigned reads = 0;    // row entries this lane walked
};

__device__ __forceinline__ void Flush(Tally &t, const Ctx &c)
{
    const unsigned entries = util::WaveSum(t.entries);
    const unsigned long long reads = util::WaveSum(static_cast<unsigned long long>(t.reads));
    if (util::LaneId() == 0) {
        if (entries) atomicAdd(c.words + W_ENTRIES, entries);
        if (reads) atomicAdd(c.reads, reads);
    }
    t = Tally();
}

// All lanes of the wave call; the lanes with `hit` append w: one atomic on the ticket word per wave.  A vertex is claimed once, so a
// position stays under `nodes`; the test keeps a mistake elsewhere from turning into a store outside the queue.
template <bool FRESH>
__device__ __forceinline__ void Append(const Ctx &c, bool hit, int w, Tally &t)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned pos = oprtr::WaveTicket(c.words + W_TAIL, mask);
    if (hit) {
        if (pos < static_cast<unsigned>(c.nodes)) St<FRESH>(c.queue + pos, w);
        t.entries += static_cast<unsigned>(c.ro[w + 1] - c.ro[w]);
    }
}

// v of level L reaches w over edge e: the CAS decides who the parent is (a stale plain read can only say "not reached")
template <bool FRESH>
__device__ __forceinline__ bool Claim(const Ctx &c, int v, int w, int e, int L)
{
    if (Ld<FRESH>(c.parent + w) != kUnseen) return false;
    if (atomicCAS(c.parent + w, kUnseen, v) != kUnseen) return false;
    St<FRESH>(c.level + w, L + 1);
    St<FRESH>(c.pedge + w, e);
    return true;
}

// 64 queue entries by one wave: lane `lane` holds v (or -1) of level L.  Rows shorter than wave_min_row by their lane, the others by
// the whole wave, one after the other (DESIGN.md 3.11's row balance).  Every loop that holds a wave operation is wave-uniform, so with
// a wave_min_row above a hub's degree the other 63 lanes wait through that row: slow, never wrong.
template <bool FRESH, int KIND>
__device__ __forceinline__ void Tile(const Ctx &c, int v, int L, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    int b = 0, e = 0;
    if (v >= 0) {
        b = c.ro[v];
        e = c.ro[v + 1];
    }
    const bool wide = e - b >= c.wave_min_row && e > b;
    unsigned long long todo = __ballot(wide);

    if (KIND == K_FOREST) {
        int longest = wide ? 0 : e - b;
        for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
            const int other = __shfl_xor(longest, o, util::kWaveSize);
            longest = other > longest ? other : longest;
        }
        for (int j = 0; j < longest; ++j) {  // (wave-uniform)
            int w = 0;
            bool hit = false;
            if (!wide && b + j < e) {
                w = c.ci[b + j];
                ++t.reads;
                hit = Claim<FRESH>(c, v, w, c.eid[b + j], L);
            }
            Append<FRESH>(c, hit, w, t);
        }
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize), lv = __shfl(v, leader, util::kWaveSize);
            for (int from = lb; from < le; from += util::kWaveSize) {  // (wave-uniform)
                const int i = from + lane;
                int w = 0;
                bool hit = false;
                if (i < le) {
                    w = c.ci[i];
                    ++t.reads;
                    hit = Claim<FRESH>(c, lv, w, c.eid[i], L);
                }
                Append<FRESH>(c, hit, w, t);
            }
            todo &= todo - 1;
        }
    } else if (KIND == K_SIZES) {
        int sum = 1;
        if (!wide)
            for (int i = b; i < e; ++i) {
                const int w = c.ci[i];
                ++t.reads;
                if (Ld<FRESH>(c.parent + w) == v) sum += Ld<FRESH>(c.size + w);
            }
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize), lv = __shfl(v, leader, util::kWaveSize);
            int part = 0;
            for (int i = lb + lane; i < le; i += util::kWaveSize) {
                const int w = c.ci[i];
                ++t.reads;
                if (Ld<FRESH>(c.parent + w) == lv) part += Ld<FRESH>(c.size + w);
            }
            part = util::WaveSum(part);
            if (lane == leader) sum = 1 + part;
            todo &= todo - 1;
        }
        if (v >= 0) St<FRESH>(c.size + v, sum);
    } else if (KIND == K_NUMBER) {
        int pv = 0;
        if (L == 0) {  // roots: every tree a range of its own from the cursor, one atomic per wave
            const int s = v >= 0 ? Ld<FRESH>(c.size + v) : 0;
            const int incl = util::WaveInclusiveSum(s);
            const int total = __shfl(incl, util::kWaveSize - 1, util::kWaveSize);
            unsigned base = 0;
            if (lane == 0 && total) base = atomicAdd(c.words + W_CURSOR, static_cast<unsigned>(total));
            base = __shfl(base, 0, util::kWaveSize);
            pv = static_cast<int>(base) + incl - s;
            if (v >= 0) St<FRESH>(c.pre + v, pv);
        } else if (v >= 0) {
            pv = Ld<FRESH>(c.pre + v);
        }
        if (!wide) {
            int next = pv + 1;
            for (int i = b; i < e; ++i) {
                const int w = c.ci[i];
                ++t.reads;
                if (Ld<FRESH>(c.parent + w) == v) {
                    St<FRESH>(c.pre + w, next);
                    next += Ld<FRESH>(c.size + w);
                }
            }
        }
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize), lv = __shfl(v, leader, util::kWaveSize);
            int carry = __shfl(pv, leader, util::kWaveSize) + 1;
            for (int from = lb; from < le; from += util::kWaveSize) {  // (wave-uniform)
                const int i = from + lane;
                int w = 0, s = 0;
                bool child = false;
                if (i < le) {
                    w = c.ci[i];
                    ++t.reads;
                    child = Ld<FRESH>(c.parent + w) == lv;
                    if (child) s = Ld<FRESH>(c.size + w);
                }
                const int incl = util::WaveInclusiveSum(s);
                if (child) St<FRESH>(c.pre + w, carry + incl - s);
                carry += __shfl(incl, util::kWaveSize - 1, util::kWaveSize);
            }
            todo &= todo - 1;
        }
    } else {  // K_LOWHIGH
        int pv = 0, pa = -1;
        if (v >= 0) {
            pv = Ld<FRESH>(c.pre + v);
            pa = Ld<FRESH>(c.parent + v);
        }
        int lo = pv, hi = pv;
        if (!wide)
            for (int i = b; i < e; ++i) {
                const int w = c.ci[i];
                ++t.reads;
                if (w == pa) continue;
                const bool child = Ld<FRESH>(c.parent + w) == v;
                const int wl = child ? Ld<FRESH>(c.low + w) : Ld<FRESH>(c.pre + w);
                const int wh = child ? Ld<FRESH>(c.high + w) : wl;
                lo = wl < lo ? wl : lo;
                hi = wh > hi ? wh : hi;
            }
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize), lv = __shfl(v, leader, util::kWaveSize);
            const int lpa = __shfl(pa, leader, util::kWaveSize), lpv = __shfl(pv, leader, util::kWaveSize);
            int plo = lpv, phi = lpv;
            for (int i = lb + lane; i < le; i += util::kWaveSize) {
                const int w = c.ci[i];
                ++t.reads;
                if (w == lpa) continue;
                const bool child = Ld<FRESH>(c.parent + w) == lv;
                const int wl = child ? Ld<FRESH>(c.low + w) : Ld<FRESH>(c.pre + w);
                const int wh = child ? Ld<FRESH>(c.high + w) : wl;
                plo = wl < plo ? wl : plo;
                phi = wh > phi ? wh : phi;
            }
            for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
                const int olo = __shfl_xor(plo, o, util::kWaveSize), ohi = __shfl_xor(phi, o, util::kWaveSize);
                plo = olo < plo ? olo : plo;
                phi = ohi > phi ? ohi : phi;
            }
            if (lane == leader) {
                lo = plo;
                hi = phi;
            }
            todo &= todo - 1;
        }
        if (v >= 0) {
            St<FRESH>(c.low + v, lo);
            St<FRESH>(c.high + v, hi);
        }
    }
}

// level L = queue[head, tail), `tile` entries per wave at a time
template <bool FRESH, int KIND>
__device__ __forceinline__ void RunLevel(const Ctx &c, int L, long long head, long long tail, int tile, long long wave0, long long nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    if (tail > c.nodes) tail = c.nodes;
    for (long long from = head + wave0 * tile; from < tail; from += nwaves * tile) {  // (wave-uniform)
        const long long i = from + lane;
        int v = -1;
        if (lane < tile && i < tail) v = Ld<FRESH>(c.queue + i);
        Tile<FRESH, KIND>(c, v, L, t);
    }
}

// ---------------- the wide form and the device loops ----------------

template <int KIND>
static __global__ __launch_bounds__(kBccThreads) void StepKernel(Ctx c, int L, unsigned head, unsigned tail, unsigned ents, int tile)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    if (KIND == K_FOREST && blockIdx.x == 0 && threadIdx.x == 0) {  // (the end of level L: the host has read it)
        c.bounds[L + 1] = static_cast<int>(tail);
        c.ents[L + 1] = ents;
    }
    Tally t;
    RunLevel<false, KIND>(c, L, head, tail, tile, wave0, nwaves, t);
    Flush(t, c);
}

// One workgroup searches level after level while each is narrow.  Every step ends in a barrier behind a fence, the two words are read
// with agent-scope loads by every thread, and a second barrier keeps the next step's atomics behind those reads.  Uniform control
// flow: every thread carries the same Front.
static __global__ __launch_bounds__(kLoopThreads) void ForestLoopKernel(Ctx c, Front s, Limits lim, Front *d_front)
{
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    Tally t;
    if (threadIdx.x == 0) {
        c.bounds[s.level + 1] = static_cast<int>(s.tail);
        c.ents[s.level + 1] = s.entries_seen;
    }
    for (int step = 0; step < lim.max_steps && s.head < s.tail && Narrow(s.tail - s.head, s.step_entries, lim); ++step) {
        const int tile = TileFor(static_cast<long long>(s.tail - s.head), nwaves, s.step_entries);
        RunLevel<true, K_FOREST>(c, s.level, s.head, s.tail, tile, wave0, nwaves, t);
        Flush(t, c);
        __threadfence();
        __syncthreads();
        const unsigned tail = static_cast<unsigned>(Ld<true>(reinterpret_cast<const int *>(c.words) + W_TAIL));
        const unsigned entries = static_cast<unsigned>(Ld<true>(reinterpret_cast<const int *>(c.words) + W_ENTRIES));
        ++s.level;
        s.head = s.tail;
        s.tail = tail;
        s.step_entries = entries - s.entries_seen;
        s.entries_seen = entries;
        if (threadIdx.x == 0 && s.level + 1 <= c.nodes + 1) {
            c.bounds[s.level + 1] = static_cast<int>(tail);
            c.ents[s.level + 1] = entries;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *d_front = s;
}

// `count` levels from `first` on, upwards (dir = 1) or downwards (dir = -1): the host has seen that each is narrow.  A step reads
// what the step before it wrote and writes what no earlier step reads, so one barrier behind a fence separates two steps.
template <int KIND>
static __global__ __launch_bounds__(kLoopThreads) void ChainLoopKernel(Ctx c, int first, int count, int dir)
{
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    Tally t;
    for (int k = 0; k < count; ++k) {
        const int L = first + k * dir;
        const long long head = c.bounds[L], tail = c.bounds[L + 1];
        const int tile = TileFor(tail - head, nwaves, static_cast<long long>(c.ents[L + 1] - c.ents[L]));
        RunLevel<true, KIND>(c, L, head, tail, tile, wave0, nwaves, t);
        __threadfence();
        __syncthreads();
    }
    Flush(t, c);
}

// ---------------- union-find: the smaller id wins a hook, so a set's root is its minimum ----------------

__device__ __forceinline__ int Find(int *uf, int x)
{
    for (;;) {
        const int p = util::LoadAgent(uf + x);
        if (p == x) return x;
        const int g = util::LoadAgent(uf + p);
        if (g == p) return p;
        __hip_atomic_store(uf + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (path halving: g is an ancestor of x for good)
        x = g;
    }
}

__device__ __forceinline__ void Unite(int *uf, int a, int b)
{
    for (;;) {
        a = Find(uf, a);
        b = Find(uf, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        if (atomicCAS(uf + a, a, b) == a) return;  // (only a root is hooked)
    }
}

static __global__ void UniteEdgesKernel(const int *d_src, const int *d_dst, long long edges, int *d_uf)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) Unite(d_uf, d_src[e], d_dst[e]);
}

// d_out[v] = the root of v (the roots do not move any more).  Out of place: a store into d_uf[v] could be overtaken by another
// thread's path halving at v, which would leave an ancestor there that is not the root.
static __global__ void CompressKernel(int *d_uf, long long nodes, int *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) d_out[v] = Find(d_uf, static_cast<int>(v));
}

// ---------------- the forest's first step ----------------

// comp[v] == v: a root at level 0, queued when it has a neighbour; the rest unseen
static __global__ void RootsKernel(Ctx c, const int *d_comp)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (c.nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    Tally t;
    for (long long r = 0; r < rounds; ++r, v += stride) {  // (wave-uniform)
        bool hit = false;
        if (v < c.nodes) {
            const bool root = d_comp[v] == v;
            c.parent[v] = root ? -1 : kUnseen;
            c.level[v] = root ? 0 : -1;
            c.pedge[v] = -1;
            hit = root && c.ro[v + 1] > c.ro[v];
        }
        Append<false>(c, hit, static_cast<int>(v), t);
    }
    Flush(t, c);
}

// ---------------- the wide passes behind the chains ----------------

struct Tree {
    const int *parent, *pedge, *size, *pre, *low, *high;
};

// the tree edge of every non-root v; d_bridge is clear
static __global__ void BridgeKernel(Tree tr, long long nodes, unsigned char *d_bridge)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        if (tr.parent[v] < 0) continue;
        const int pv = tr.pre[v];
        if (tr.low[v] >= pv && tr.high[v] < pv + tr.size[v]) d_bridge[tr.pedge[v]] = 1;
    }
}

// b in the subtree of a?
__device__ __forceinline__ bool Under(const Tree &tr, int a, int b)
{
    const int pa = tr.pre[a], pb = tr.pre[b];
    return pb >= pa && pb < pa + tr.size[a];
}

// the two joining rules, one canonical edge per thread
static __global__ void LinkKernel(Tree tr, const int *d_src, const int *d_dst, long long edges, int *d_uf)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        const int a = d_src[e], b = d_dst[e];
        const bool down = tr.parent[b] == a, up = tr.parent[a] == b;
        if (down || up) {
            const int v = down ? a : b, w = down ? b : a;
            if (tr.parent[v] < 0) continue;  // (a root has no tree edge of its own)
            const int pv = tr.pre[v];
            if (tr.low[w] < pv || tr.high[w] >= pv + tr.size[v]) Unite(d_uf, v, w);
        } else if (!Under(tr, a, b) && !Under(tr, b, a)) {
            Unite(d_uf, a, b);
        }
    }
}

// the set of every edge (d_set: the root per vertex): its child end's, or that of the end with the larger pre
static __global__ void EdgeSetKernel(Tree tr, const int *d_src, const int *d_dst, long long edges, const int *d_uf, int *d_set)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        const int a = d_src[e], b = d_dst[e];
        int end;
        if (tr.parent[b] == a) end = b;
        else if (tr.parent[a] == b) end = a;
        else end = tr.pre[a] > tr.pre[b] ? a : b;
        d_set[e] = d_uf[end];
    }
}

// d_first[r] of a root r: the set of its first child in row order (the one numbered pre[r] + 1)
static __global__ void FirstChildKernel(Tree tr, long long nodes, const int *d_uf, int *d_first)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long w = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; w < nodes; w += stride) {
        const int p = tr.parent[w];
        if (p >= 0 && tr.parent[p] < 0 && tr.pre[w] == tr.pre[p] + 1) d_first[p] = d_uf[w];
    }
}

// a non-root with a child in another set than its own tree edge; a root whose children are in two sets (d_art is clear; every
// writer stores the same byte)
static __global__ void ArticulationKernel(Tree tr, long long nodes, const int *d_uf, const int *d_first, unsigned char *d_art)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long w = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; w < nodes; w += stride) {
        const int p = tr.parent[w];
        if (p < 0) continue;
        const int mine = d_uf[w], other = tr.parent[p] < 0 ? d_first[p] : d_uf[p];
        if (mine != other) d_art[p] = 1;
    }
}

// d_up[v]: the parent, or v itself at a root and below a bridge
static __global__ void CutForestKernel(Tree tr, long long nodes, const unsigned char *d_bridge, int *d_up)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int p = tr.parent[v];
        d_up[v] = p < 0 || d_bridge[tr.pedge[v]] ? static_cast<int>(v) : p;
    }
}

static __global__ void CountBytesKernel(const unsigned char *d_flag, long long count, unsigned long long *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned long long mine = 0;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) mine += d_flag[i] ? 1 : 0;
    mine = util::WaveSum(mine);
    if (util::LaneId() == 0 && mine) atomicAdd(d_out, mine);
}

// the block-cut tree: one key per (edge end, block), v << edge_bits | block at an articulation point v, else the sentinel
static __global__ void BlockCutKeysKernel(const int *d_src, const int *d_dst, const int *d_bcc, const unsigned char *d_art, long long edges,
                                          int edge_bits, unsigned long long sentinel, unsigned long long *d_keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        const unsigned a = static_cast<unsigned>(d_src[e]), b = static_cast<unsigned>(d_dst[e]);
        const unsigned long long id = static_cast<unsigned>(d_bcc[e]);
        d_keys[2 * e] = d_art[a] ? (static_cast<unsigned long long>(a) << edge_bits) | id : sentinel;
        d_keys[2 * e + 1] = d_art[b] ? (static_cast<unsigned long long>(b) << edge_bits) | id : sentinel;
    }
}

}  // namespace bcc
}  // namespace app
}  // namespace gunrock
