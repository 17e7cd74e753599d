// poly_scan.h -- the workgroup scan of the reduce-then-scan primitives over tiles of THREADS * E elements (poly_product.hip: products,
// poly_sum.hip: sums): the wave scan, the hand-off of the four wave totals through LDS, the padded load of a thread's run and the walk of
// the seed kernels over the tile totals.  Device code over poly_elem.h that knows no particular operation.
//
// An operation is a type Op with three static members for every scalar field Fr:
//   identity(Fe<Fr> &r)                                the neutral element; what a run reads beyond the end of its vector
//   combine(Fe<Fr> &r, const Fe<Fr> &a, const Fe<Fr> &b)   r <- a op b, associative (r may be a or b)
//   run<RUN>(Fe<Fr> &g, const Fe<Fr> (&x)[RUN])        g <- x[0] op ... op x[RUN - 1], which an operation may spell cheaper than RUN - 1
//                                                      combines
// and one guarantee: a loaded element, the identity and every result of combine and run are valid operands of combine and of store_elem,
// however many combines stand behind them.  Nothing here normalises a value: what crosses a lane, LDS or memory is whatever the
// operation returns, and the operation's file says why that is in bounds.
#pragma once
#include "poly_elem.h"

namespace panda_poly {

PANDA_HD unsigned tiles_of(u64 n, unsigned tile) { return (unsigned)((n + tile - 1) / tile); }

// r <- v of the lane d below (REV: above); lanes without such a neighbour get an unspecified value
template <class Fr, bool REV>
__device__ __forceinline__ void lane_shift(Fe<Fr> &r, const Fe<Fr> &v, unsigned d)
{
#pragma unroll
    for (int i = 0; i < NL; i++) r.l[i] = REV ? __shfl_down(v.l[i], d, 64) : __shfl_up(v.l[i], d, 64);
}

// inclusive scan of the wave: lane l <- op_{u <= l} v_u (REV: u >= l).  Six combines per thread.
template <class Op, class Fr, bool REV>
__device__ __forceinline__ void wave_scan(Fe<Fr> &v, unsigned lane)
{
#pragma unroll
    for (int s = 0; s < 6; s++) {
        const unsigned d = 1u << s;
        Fe<Fr> t, pr;
        lane_shift<Fr, REV>(t, v, d);
        Op::combine(pr, v, t);
        const bool in = REV ? lane + d < 64 : lane >= d;
        panda29::fe_select(v, in, pr, v);
    }
}

// g is the aggregate of the calling thread's run.  mine <- seed op the g of every thread before the caller (REV: behind it), total <-
// seed op all of them (the same in every thread).  One barrier; the caller puts another one before s_w (WAVES * NL words) is reused.
// Combines per thread: 6 (wave scan) + WAVES (across the waves) + 1.
template <class Op, class Fr, bool REV>
__device__ __forceinline__ void block_scan(Fe<Fr> &mine, Fe<Fr> &total, const Fe<Fr> &g, const Fe<Fr> &seed, u32 *s_w)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Fe<Fr> v = g;
    wave_scan<Op, Fr, REV>(v, lane);
    if (lane == (REV ? 0u : 63u)) lds_put(s_w + wave * NL, v.l);
    __syncthreads();
    Fe<Fr> y = seed, base = seed;
#pragma unroll
    for (int k = 0; k < WAVES; k++) {
        const int w = REV ? WAVES - 1 - k : k;
        Fe<Fr> t;
        lds_get(t, s_w + w * NL);
        Op::combine(y, y, t);
        if ((int)wave == (REV ? w - 1 : w + 1)) base = y;
    }
    total = y;
    Fe<Fr> ex, pr;
    lane_shift<Fr, REV>(ex, v, 1);
    Op::combine(pr, base, ex);
    panda29::fe_select(mine, lane == (REV ? 63u : 0u), base, pr);
}

// g <- the aggregate of the workgroup's 256 run aggregates, valid in thread 0.  One barrier, s_w as above.
template <class Op, class Fr>
__device__ __forceinline__ void block_reduce(Fe<Fr> &g, u32 *s_w)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_scan<Op, Fr, false>(g, lane);
    if (lane == 63) lds_put(s_w + wave * NL, g.l);
    __syncthreads();
    if (threadIdx.x == 0) {
        lds_get(g, s_w);
#pragma unroll
        for (int w = 1; w < WAVES; w++) {
            Fe<Fr> t;
            lds_get(t, s_w + w * NL);
            Op::combine(g, g, t);
        }
    }
}

// RUN consecutive elements from index j0 of a vector of n, the identity beyond n
template <class Op, class Fr, int RUN>
__device__ __forceinline__ void load_run(Fe<Fr> (&x)[RUN], const u32 *vec, u64 j0, u64 n)
{
#pragma unroll
    for (int e = 0; e < RUN; e++) {
        if (j0 + e < n)
            load_elem(x[e], vec + (j0 + e) * 8);
        else
            Op::identity(x[e]);
    }
}

// One walk of a seed kernel's workgroup over the `tiles` tile totals at `in`, from the first chunk of CHUNK = THREADS * CE totals up.
// carry <- carry op all totals, the same in every thread.  STORE: out[a] <- carry op the totals before a, the exclusive scan; every
// thread stores the indices it loaded, so out may be in.  Ends on a barrier: s_w is free again.
template <class Op, class Fr, int CE, bool STORE>
__device__ __forceinline__ void walk_totals(Fe<Fr> &carry, const u32 *in, u32 *out, unsigned tiles, u32 *s_w)
{
    constexpr unsigned CHUNK = THREADS * CE;
    for (unsigned k = 0; k < tiles_of(tiles, CHUNK); k++) {
        const u64 a0 = (u64)k * CHUNK + threadIdx.x * CE;
        Fe<Fr> x[CE], g, s, total;
        load_run<Op, Fr, CE>(x, in, a0, tiles);
        Op::run(g, x);
        block_scan<Op, Fr, false>(s, total, g, carry, s_w);
        carry = total;
        if constexpr (STORE) {
#pragma unroll
            for (int e = 0; e < CE; e++) {
                if (a0 + e < tiles) store_elem(out + (a0 + e) * 8, s);
                if (e < CE - 1) Op::combine(s, s, x[e]);
            }
        }
        __syncthreads();
    }
}

} // namespace panda_poly
