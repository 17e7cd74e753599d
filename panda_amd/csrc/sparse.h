// sparse.h -- the row search, the per-thread and per-tile routines and the fix-up of panda_sparse_matvec (sparse.hip), kept
// apart from the kernels so that a host program can run them (tests/host_check/sparse_host.cpp, under FE29_CHECK).
//
//   out[p][r] = sum_{k in row r} values[k] z[p][col[k]]        row r holds the nonzeros row_ptr[r] .. row_ptr[r + 1] - 1
//
// The work is split by nonzeros.  Tile t covers the nonzeros [t TILE, (t + 1) TILE), thread i of it the E consecutive ones from
// k0 = t TILE + i E.  A thread finds the row of k0 by a bounded search (row_of), walks its E nonzeros through the rows (walk_rows: a row
// change is one step to the next row, or one more bounded search when that row is empty -- never a loop over empty rows), multiplies
// (thread_segments: two nonzeros of one row per Montgomery reduction) and is left with at most E closed segments -- rows, or pieces of
// rows, whose last nonzero of the tile it holds -- and one open sum that the next thread continues.  The open sums are combined by a
// segmented scan over (flag, value); the first closed segment of a thread takes the scan's exclusive prefix unless its row starts at k0.
// A closed segment whose row began inside the tile goes to out[row], the tile's leading piece of a row that began earlier to head[t]
// (emit).  The last thread of a tile closes its open segment by force, so a row that runs on leaves its piece in out[row] or head[t].
// The fix-up then adds, for every row that crosses a tile end, head[t'] of the tiles t' it continues into to out[row]: the wave of the
// FIRST such tile owns the row (fixup_span), its lanes add the heads in steps of FIXUP_CHUNK (fixup_lane_sum).
//
// Arithmetic.  fe_mul(a, b) = a b / R (R = 2^261) and the wire form is x W (W = 2^256): fe_mul_add(v W, z W, v' W, z' W) is
// (v z + v' z') W c for c = W / R.  The stray c is removed per closed segment, after the sum, by one fe_mul with c^-1 in the form fe_mul
// multiplies (panda_sop::wire_factor_inverse): everything stored to out and head is a canonical wire residue, the fix-up only adds.
//
// Memory safety, whatever bytes row_ptr and col hold.  row_of reads row_ptr[mid] for lo < mid <= hi only and returns a row in [lo, hi];
// every caller passes hi <= n_rows - 1, so a row index is below n_rows by construction, and row_ptr is read at row and row + 1 alone.  A
// column index is clamped below n_cols before it addresses z.  A position addresses col / values only if it is below nnz (n_live).  A
// tile index addresses head only if it is below tiles (fixup_span clamps the last tile).  For a structure panda_sparse_check rejects
// the VALUES are unspecified, the accesses are not.
//
// Bounds (contract at the top of fe29.h; worst case every operand p - 1, BLS12-381 Fr with R / p = 70.6 the tightest):
//   loaded element    fe_unpack of a canonical residue                                    tight, < p      (canonical)
//   pair              fe_mul_add(v < p, z < p, v' < p, z' < p): 2 p^2 < 0.9 R p, 27 column terms of < 2^58 in a u64
//                                                                                         tight, < 2p;  fe_reduce_once -> canonical
//   single            fe_mul(v < p, z < p): p^2 < 0.9 R p                                 tight, < 2p;  fe_reduce_once -> canonical
//   segment sum       add_canon (poly_sum.h) of canonical values                          tight, < p      (canonical)
//   scan, prefix      add_canon of canonical values, in registers, lanes and LDS          tight, < p      (canonical)
//   closed segment    fe_mul(sum < p, c^-1 < p): p^2 < 0.9 R p -> tight, < 2p; fe_reduce_once
//                                                                                         tight, < p      (canonical)
//   fix-up            add_canon of canonical values from out and head                     tight, < p      (canonical)
// Every accumulator is canonical again after EVERY addition and only canonical values are operands of a product, so neither the row
// length, the tile count nor the batch enters a bound.  (A value or z at or above the modulus is outside the contract; as a 256-bit
// number it is below 2^256 < 2.3 p, so even then 2 (2^256)^2 < 0.9 R p and no column overflows.)
#pragma once
#include <stdint.h>

#include "fe29.h"
#include "poly_sum.h"
#include "poly_terms.h"

namespace panda_sparse {

using panda29::Fe;
using panda29::u32;
typedef uint64_t u64;

constexpr int NL = 9;                   // limbs of every supported scalar field
constexpr int TILE_THREADS = 256;       // threads of a tile's workgroup
constexpr int E = 4;                    // consecutive nonzeros per thread
constexpr u32 TILE = TILE_THREADS * E;  // nonzeros per tile
constexpr u32 FIXUP_CHUNK = 64;         // heads a fix-up wave adds per step, one per lane
constexpr u32 MAX_LOG = 28;             // n_rows, n_cols, nnz, batch x n_rows, batch x n_cols <= 2^28

#if defined(FE29_CHECK)
template <class Fr>
inline void check_canonical(const Fe<Fr> &v)
{
    for (int i = 0; i < NL - 1; i++) assert(v.l[i] < (1u << 29) && "sparse: limb not tight");
    bool below = false;
    for (int i = NL - 1; i >= 0; i--)
        if (v.l[i] != Fr::P[i]) {
            below = v.l[i] < Fr::P[i];
            break;
        }
    assert(below && "sparse: value not below p");
}
#define PANDA_SPARSE_CANON(v) check_canonical(v)
#define PANDA_SPARSE_TIGHT_2P(v) panda_sop::check_tight_2p(v)
#else
#define PANDA_SPARSE_CANON(v)
#define PANDA_SPARSE_TIGHT_2P(v)
#endif

// The last row r in [lo, hi] with row_ptr(r) <= k, lo if there is none; lo <= hi.  For a valid structure and lo = 0, hi = n_rows - 1
// this is the row that holds nonzero k: the upper bound over row_ptr, less one, clamped to the last row.  row_ptr is read at indices in
// (lo, hi] alone; the interval halves every step, so 32 steps are never reached.
template <class RowPtr>
PANDA_HD u32 row_of(RowPtr &&row_ptr, u32 k, u32 lo, u32 hi)
{
    for (int step = 0; step < 32 && lo < hi; step++) {
        const u32 mid = lo + (hi - lo + 1) / 2; // lo < mid <= hi
        if (row_ptr(mid) <= k)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The rows of the thread's n_live <= E nonzeros k0 .. k0 + n_live - 1, each in [r_lo, r_hi] and non-decreasing, and `end`, row_ptr at the
// last one's row + 1.  row_ptr is read at indices in [r_lo, r_hi + 1].
template <class RowPtr>
PANDA_HD void walk_rows(u32 (&row)[E], u32 &end, RowPtr &&row_ptr, u32 k0, u32 n_live, u32 r_lo, u32 r_hi)
{
    u32 r = row_of(row_ptr, k0, r_lo, r_hi);
    end = row_ptr(r + 1);
#pragma unroll
    for (int e = 0; e < E; e++) {
        const u32 k = k0 + e;
        if ((u32)e < n_live && e > 0 && k >= end && r < r_hi) {
            r++;
            end = row_ptr(r + 1);
            if (k >= end && r < r_hi) { // an empty row: search, do not walk
                r = row_of(row_ptr, k, r, r_hi);
                end = row_ptr(r + 1);
            }
        }
        row[e] = r;
    }
}

// What a thread holds after its nonzeros.
template <class Fr>
struct Segments {
    Fe<Fr> val[E];  // val[e]: the sum, still carrying c, of the segment that closes behind slot e (where bit e of `closed` is set)
    u32 row[E];     // the row of slot e, below n_rows
    u32 closed;     // bit e: the row's last nonzero of this tile is slot e
    u32 first;      // the lowest set bit's index, E if none: that segment continues the threads before unless `starts`
    bool starts;    // the row of slot 0 begins at k0
    Fe<Fr> open;    // the sum behind the last closed slot (zero if there is nothing): what the next thread continues
    u32 flag;       // the thread's scan element is (flag, open): 1 if a segment begins in this thread
};

// access: row_ptr(i), col(k), value(Fe &, k), z(Fe &, c) -- the caller's loads, each called with an index inside its extent only.
// force: the thread holds the tile's last nonzero and closes its open segment.
template <class Fr, class Access>
PANDA_HD void thread_segments(Segments<Fr> &S, Access &&access, u32 k0, u32 n_live, bool force, u32 r_lo, u32 r_hi, u32 n_cols)
{
    static_assert(E == 4, "two pairs per thread");
    Fe<Fr> zero;
    panda29::fe_zero(zero);
    S.closed = 0, S.first = E, S.starts = false, S.flag = 0, S.open = zero;
#pragma unroll
    for (int e = 0; e < E; e++) S.row[e] = r_lo, S.val[e] = zero;
    if (n_live == 0) return;
    auto row_ptr = [&](u32 i) { return access.row_ptr(i); };
    u32 end;
    walk_rows(S.row, end, row_ptr, k0, n_live, r_lo, r_hi);
    S.starts = access.row_ptr(S.row[0]) == k0;
#pragma unroll
    for (int e = 0; e < E; e++) {
        if ((u32)e >= n_live) continue;
        const bool last = (u32)e + 1 == n_live;
        const bool closes = last ? (force || end <= k0 + n_live) : (e + 1 < E && S.row[e + 1] != S.row[e]);
        if (closes) S.closed |= 1u << e;
    }
    Fe<Fr> v[E], z[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        v[e] = zero, z[e] = zero;
        if ((u32)e < n_live) {
            u32 c = access.col(k0 + e);
            c = c < n_cols ? c : 0u; // n_cols >= 1
            access.value(v[e], k0 + e);
            access.z(z[e], c);
        }
    }
    Fe<Fr> acc = zero, t;
#pragma unroll
    for (int e = 0; e < E; e += 2) {
        // slots e and e + 1 are one row's unless e closes; a dead slot multiplies zeros
        const bool split = (S.closed >> e) & 1u;
        Fe<Fr> v1, none = zero;
        panda29::fe_select(v1, split, none, v[e + 1]);
        panda29::fe_mul_add(t, v[e], z[e], v1, z[e + 1]);
        PANDA_SPARSE_TIGHT_2P(t);
        panda29::fe_reduce_once(t);
        panda_poly::add_canon(acc, acc, t);
        PANDA_SPARSE_CANON(acc);
        if (split) {
            S.val[e] = acc;
            panda29::fe_mul(t, v[e + 1], z[e + 1]); // the unpaired product
            PANDA_SPARSE_TIGHT_2P(t);
            panda29::fe_reduce_once(t);
            acc = t;
        }
        if ((S.closed >> (e + 1)) & 1u) {
            S.val[e + 1] = acc;
            acc = zero;
        }
    }
    S.open = acc;
    S.flag = S.closed ? 1u : (S.starts ? 1u : 0u);
#pragma unroll
    for (int e = E - 1; e >= 0; e--)
        if ((S.closed >> e) & 1u) S.first = e;
}

// the scan's operator on (flag, value), values canonical: (fa, a) then (fb, b)
template <class Fr>
PANDA_HD void seg_combine(u32 &f, Fe<Fr> &v, u32 fa, const Fe<Fr> &a, u32 fb, const Fe<Fr> &b)
{
    Fe<Fr> sum;
    panda_poly::add_canon(sum, a, b);
    panda29::fe_select(v, fb != 0, b, sum);
    f = fa | fb;
    PANDA_SPARSE_CANON(v);
}

// The thread's closed segments, with the exclusive prefix (pf, pv) of the scan over the threads before it in the tile: store(in_tile, row,
// value) receives a canonical wire residue for out[row] (in_tile) or for the tile's head.  cinv = c^-1 as fe_mul multiplies it.
template <class Fr, class Store>
PANDA_HD void emit(const Segments<Fr> &S, u32 pf, const Fe<Fr> &pv, const Fe<Fr> &cinv, Store &&store)
{
#pragma unroll
    for (int e = 0; e < E; e++) {
        if (!((S.closed >> e) & 1u)) continue;
        Fe<Fr> total = S.val[e];
        bool in_tile = true;
        if ((u32)e == S.first && !S.starts) {
            panda_poly::add_canon(total, pv, S.val[e]);
            in_tile = pf != 0;
        }
        PANDA_SPARSE_CANON(total);
        panda29::fe_mul(total, total, cinv);
        PANDA_SPARSE_TIGHT_2P(total);
        panda29::fe_reduce_once(total);
        PANDA_SPARSE_CANON(total);
        store(in_tile, S.row[e], total);
    }
}

// Tile t >= 1 of `tiles`: true if the row r of its first nonzero began in tile t - 1, so that this tile is the first the row continues
// into and its wave owns out[r]; t_last is then the last tile whose head belongs to the row, t <= t_last < tiles.  A row belongs to at
// most one t, the tile behind the one row_ptr(r) lies in, so no two waves write one row.
template <class RowPtr>
PANDA_HD bool fixup_span(u32 &r, u32 &t_last, RowPtr &&row_ptr, u32 t, u32 n_rows, u32 tiles)
{
    const u32 k = t * TILE;
    r = row_of(row_ptr, k, 0u, n_rows - 1);
    const u32 start = row_ptr(r), end = row_ptr(r + 1);
    t_last = t;
    if (!(start < k && start >= k - TILE)) return false;
    if (end > k) t_last = (end - 1) / TILE;
    if (t_last >= tiles) t_last = tiles - 1;
    return true;
}

// lane's share of head[t .. t_last]: every FIXUP_CHUNK-th tile from t + lane, canonical
template <class Fr, class Head>
PANDA_HD void fixup_lane_sum(Fe<Fr> &sum, Head &&head, u32 t, u32 t_last, u32 lane)
{
    panda29::fe_zero(sum);
    for (u64 j = (u64)t + lane; j <= t_last; j += FIXUP_CHUNK) {
        Fe<Fr> h;
        head(h, (u32)j);
        panda_poly::add_canon(sum, sum, h);
        PANDA_SPARSE_CANON(sum);
    }
}

inline u32 tiles_of_nnz(u64 nnz) { return (u32)((nnz + TILE - 1) / TILE); }

inline bool shape_valid(u64 n_rows, u64 n_cols, u64 nnz, u64 batch)
{
    const u64 cap = (u64)1 << MAX_LOG;
    return n_rows >= 1 && n_cols >= 1 && batch >= 1 && n_rows <= cap && n_cols <= cap && nnz <= cap && batch <= cap && batch * n_rows <= cap &&
           batch * n_cols <= cap;
}

// One tile on the host, thread after thread, with a serial scan in place of the kernel's parallel one: what k_sparse_tile computes.
// store(in_tile, row, value) as for emit.
template <class Fr, class Access, class Store>
inline void host_tile(Access &&access, u32 t, u32 n_rows, u32 n_cols, u32 nnz, Store &&store)
{
    const u32 first = t * TILE, last = (nnz - first < TILE ? nnz : first + TILE) - 1;
    auto row_ptr = [&](u32 i) { return access.row_ptr(i); };
    const u32 r_lo = row_of(row_ptr, first, 0u, n_rows - 1), r_hi = row_of(row_ptr, last, r_lo, n_rows - 1);
    const Fe<Fr> &cinv = panda_sop::wire_factor_inverse<Fr>();
    u32 pf = 0;
    Fe<Fr> pv;
    panda29::fe_zero(pv);
    for (u32 i = 0; i < (u32)TILE_THREADS; i++) {
        const u32 k0 = first + i * E, n_live = k0 >= nnz ? 0u : (nnz - k0 < (u32)E ? nnz - k0 : (u32)E);
        const bool force = n_live > 0 && (i == (u32)TILE_THREADS - 1 || k0 + E >= nnz);
        Segments<Fr> S;
        thread_segments(S, access, k0, n_live, force, r_lo, r_hi, n_cols);
        emit(S, pf, pv, cinv, store);
        seg_combine(pf, pv, pf, pv, S.flag, S.open);
    }
}

} // namespace panda_sparse
