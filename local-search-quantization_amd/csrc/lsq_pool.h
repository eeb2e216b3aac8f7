// lsq_pool.h -- the selection that lives in a block's LDS (gfx950): the nn smallest of the 64-bit records a block of 256 threads is offered, kept in a pool of
// P records.  Said once, for the scans that select inside their walk: lsq_ivfsel.hip (one pool per block) and lsq_label.hip (QB
// pools per block).  Device code only: include it behind lsq_internal.h in a .hip unit.
//
//   RECORD  distinct per row (a key above the row's id), so the nn smallest are a SET that no arrival order changes.
//   POOL    P = 2 pow2ceil(max(nn, 256)) records of LDS.  The block holds `bound` -- all ones until the pool has been compacted to nn records, then the nn-th of
//           them -- and the fill, both as block-uniform registers.  A step: a lane whose record is < bound takes a slot; slots are handed out per wave by
//           __ballot, ONE integer LDS add by the wave's first hitting lane, and prefix popcounts.  The add goes to one of three step counters used in
//           rotation, so that ONE barrier per step is enough: after it every thread reads the step's count and adds it to its copy of the fill (a wave that
//           runs ahead adds to the next counter, never to the one a slower wave has yet to read; thread 0 clears the counter of the step after next).
//           Which slot a record gets depends on the order of the waves' adds; how many records a step adds does not, so the fill, and with it every
//           decision to compact, is a function of the data and the shapes alone.
//   COMPACT when fewer than 256 slots are free after a step (block-uniform): the slots past the fill up to the next power of two are set to all ones, a
//           bitonic sort in LDS puts the records in order, bound = the nn-th, fill = nn.
// pool_offer is the step of a block with ONE pool; a block with several runs pool_place / pool_settle around a barrier of its own (lsq_label.hip).
#pragma once

constexpr int SEL_THREADS = 256;

struct Pool {
    uint64_t *rec;               // LDS [P]
    unsigned *tick;              // LDS [3]: the records added in step s, at tick[s % 3]
    uint64_t bound;              // block-uniform: a record >= bound is not among the nn smallest
    int fill, P, nn;             // block-uniform
    unsigned step, compactions;
};

__device__ inline int pool_pow2ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// the records rec[0 .. fill) in ascending order; ends behind a barrier.  (fill <= P, a power of two: the padded length stays inside the pool)
__device__ inline void pool_sort(const Pool &p) {
    const int t = threadIdx.x, S = pool_pow2ceil(p.fill);
    for (int i = p.fill + t; i < S; i += SEL_THREADS) p.rec[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= S; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (S >> 1); i += SEL_THREADS) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;      // the i-th pair of partners j apart
                const uint64_t x = p.rec[lo], y = p.rec[hi];
                if ((x > y) == ((lo & k) == 0)) { p.rec[lo] = y; p.rec[hi] = x; }
            }
            __syncthreads();
        }
}

__device__ inline void pool_compact(Pool &p) {
    pool_sort(p);
    if (p.fill >= p.nn) {
        p.bound = p.rec[p.nn - 1];
        p.fill = p.nn;
    }
}

// the first half of a step, before its barrier: the wave's hitting records take their slots (one LDS add per wave)
__device__ inline void pool_place(const Pool &p, uint64_t rec, bool hit) {
    const int lane = threadIdx.x & 63;
    unsigned *c = p.tick + p.step % 3u;
    const unsigned long long mask = __ballot(hit);
    if (mask) {                                                          // (wave-uniform) one add for the wave's records of this step
        const int leader = __ffsll((long long)mask) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(c, (unsigned)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (hit) p.rec[p.fill + (int)base + __popcll(mask & ((1ull << lane) - 1ull))] = rec;
    }
}

// the second half, behind the barrier: the step's count joins the fill, the counter of the step after next is cleared, a full pool is compacted
__device__ inline void pool_settle(Pool &p) {
    unsigned *c = p.tick + p.step % 3u;
    p.fill += (int)*(volatile unsigned *)c;
    if (threadIdx.x == 0) p.tick[(p.step + 2u) % 3u] = 0u;               // read last in step - 1 (before this barrier), added to next in step + 2 (behind the next)
    p.step += 1u;
    if (p.P - p.fill < SEL_THREADS) {                                    // (block-uniform)
        pool_compact(p);
        p.compactions += 1u;
    }
}

// one step: every thread of the block calls it, `hit` says whether its record is offered and < bound.  At entry P - fill >= 256, so every slot handed out
// lies inside the pool
__device__ inline void pool_offer(Pool &p, uint64_t rec, bool hit) {
    pool_place(p, rec, hit);
    __syncthreads();
    pool_settle(p);
}

// the answer of query q from the pool: sorted, handed out as adc_gather_kernel hands out, (+inf, 0) past the records
__device__ inline void pool_hand_out(Pool &p, int64_t q, float *__restrict__ dists, int *__restrict__ ids, int idbits) {
    pool_sort(p);
    const int have = p.fill < p.nn ? p.fill : p.nn;
    for (int r = threadIdx.x; r < p.nn; r += SEL_THREADS) {
        const uint64_t rec = r < have ? p.rec[r] : 0ull;
        dists[q * p.nn + r] = r < have ? lsq_adc_unkey((uint32_t)(rec >> idbits)) : __builtin_inff();
        ids[q * p.nn + r] = (int)(uint32_t)(rec & ((1ull << idbits) - 1ull));
    }
}
