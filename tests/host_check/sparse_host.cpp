// Host run of the sparse product: panda_amd/csrc/sparse.h -- the row search, the per-thread routine, the tile (with a serial scan in place of
// the kernel's parallel one), the emit and the fix-up -- built for the HOST with FE29_CHECK (128-bit shadow column accumulators in fe_mul /
// fe_mul_add; the classes of sparse.h's bounds table asserted after every step).  Every load and store goes through an accessor that
// checks its index against the buffer's extent.  Valid matrices are compared with 256-bit modular arithmetic written here (shift-and-add
// products on four 64-bit words, no Montgomery form): every value and every z equal to p - 1, rows of length 1, 2, 3 and 4 T + 1, empty
// rows and runs of them, nonzero counts around the tile size, a row over more tiles than a fix-up step takes, the three fields.
// Invalid structures (row_ptr all ones, decreasing, random; col all ones, random) are run for their accesses alone: none may leave its
// extent, and no row of `out` may be stored twice by one launch.
// Test infrastructure: compiled and run by tests/test_sparse.py with g++; prints "ok <checked values>" and exits 0.
#define FE29_CHECK 1
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../panda_amd/csrc/sparse.h"

using namespace panda29;
using panda_sparse::TILE;

namespace {

struct U256 {
    u64 w[4];
};

bool geq(const U256 &a, const U256 &b)
{
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
    return true;
}
bool same(const U256 &a, const U256 &b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }
u64 add(U256 &r, const U256 &a, const U256 &b)
{
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (u64)c;
        c >>= 64;
    }
    return (u64)c;
}
void sub(U256 &r, const U256 &a, const U256 &b)
{
    u64 borrow = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - borrow;
        r.w[i] = (u64)d;
        borrow = (u64)(d >> 64) & 1;
    }
}

const U256 ZERO = {{0, 0, 0, 0}};

struct Field {
    U256 p;
    U256 addmod(const U256 &a, const U256 &b) const // a, b < p
    {
        U256 r;
        const u64 carry = add(r, a, b);
        if (carry || geq(r, p)) sub(r, r, p);
        return r;
    }
    U256 mulmod(const U256 &a, const U256 &b) const
    {
        U256 r = ZERO;
        for (int bit = 255; bit >= 0; bit--) {
            r = addmod(r, r);
            if ((b.w[bit >> 6] >> (bit & 63)) & 1) r = addmod(r, a);
        }
        return r;
    }
    U256 powmod(U256 a, const U256 &e) const
    {
        U256 r = {{1, 0, 0, 0}};
        for (int bit = 0; bit < 256; bit++) {
            if ((e.w[bit >> 6] >> (bit & 63)) & 1) r = mulmod(r, a);
            a = mulmod(a, a);
        }
        return r;
    }
};

U256 from_words(const u32 *w)
{
    U256 r;
    for (int i = 0; i < 4; i++) r.w[i] = (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32);
    return r;
}
void to_words(u32 *w, const U256 &a)
{
    for (int i = 0; i < 4; i++) {
        w[2 * i] = (u32)a.w[i];
        w[2 * i + 1] = (u32)(a.w[i] >> 32);
    }
}

u64 rng_state = 0x9E3779B97F4A7C15ull;
u64 rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
U256 random_below(const Field &F)
{
    U256 r;
    for (int i = 0; i < 4; i++) r.w[i] = rng();
    r.w[3] &= (~0ull) >> 1;
    while (geq(r, F.p)) sub(r, r, F.p);
    return r;
}

long checked = 0;

void fail(const char *what)
{
    fprintf(stderr, "failed: %s\n", what);
    exit(1);
}
void require(bool ok, const char *what)
{
    if (!ok) fail(what);
}

// a CSR matrix and a vector on the "wire" (256-bit values below p; for the adversarial runs the structure is arbitrary)
struct Matrix {
    u32 n_rows, n_cols, nnz;
    std::vector<u32> row_ptr, col;
    std::vector<U256> values, z;
};

// the loads of sparse.h's routines, each checked against its extent
template <class Fr>
struct CheckedAccess {
    const Matrix &m;
    mutable long loads = 0;
    u32 row_ptr(u32 i) const
    {
        require(i <= m.n_rows, "row_ptr read outside its n_rows + 1 entries");
        loads++;
        return m.row_ptr[i];
    }
    u32 col(u32 k) const
    {
        require(k < m.nnz, "col read outside its nnz entries");
        loads++;
        return m.col[k];
    }
    void value(Fe<Fr> &v, u32 k) const
    {
        require(k < m.nnz, "values read outside its nnz entries");
        u32 w[8];
        to_words(w, m.values[k]);
        fe_unpack(v, w);
        loads++;
    }
    void z(Fe<Fr> &v, u32 c) const
    {
        require(c < m.n_cols, "z read outside its n_cols entries");
        u32 w[8];
        to_words(w, m.z[c]);
        fe_unpack(v, w);
        loads++;
    }
};

template <class Fr>
U256 to_u256(const Fe<Fr> &v)
{
    u32 w[8];
    fe_pack(w, v);
    return from_words(w);
}

// the product as the two launches compute it; `valid`: the structure is a legal CSR, so no row may be stored twice by one launch
template <class Fr>
std::vector<U256> run_product(const Field &F, const Matrix &m, bool valid)
{
    std::vector<U256> out(m.n_rows, ZERO);
    const u32 tiles = panda_sparse::tiles_of_nnz(m.nnz);
    std::vector<U256> head(tiles, ZERO);
    std::vector<char> stored(m.n_rows, 0), head_stored(tiles, 0);
    CheckedAccess<Fr> access{m};
    for (u32 t = 0; t < tiles; t++)
        panda_sparse::host_tile<Fr>(access, t, m.n_rows, m.n_cols, m.nnz, [&](bool in_tile, u32 row, const Fe<Fr> &total) {
            require(row < m.n_rows, "a row index at or above n_rows reached out");
            if (in_tile) {
                require(!valid || !stored[row], "a row was stored twice by the tile launch");
                stored[row] = 1;
                out[row] = to_u256(total);
            } else {
                require(!valid || !head_stored[t], "a tile's head was stored twice");
                head_stored[t] = 1;
                head[t] = to_u256(total);
            }
        });
    std::vector<char> fixed(m.n_rows, 0);
    auto rp = [&](u32 i) { return access.row_ptr(i); };
    for (u32 t = 1; t < tiles; t++) {
        u32 r, t_last;
        if (!panda_sparse::fixup_span(r, t_last, rp, t, m.n_rows, tiles)) continue;
        require(r < m.n_rows && t_last < tiles && t_last >= t, "the fix-up's span left its extents");
        require(!fixed[r], "a row was fixed up twice"); // whatever the structure
        fixed[r] = 1;
        U256 sum = ZERO;
        for (u32 lane = 0; lane < panda_sparse::FIXUP_CHUNK; lane++) {
            Fe<Fr> s;
            panda_sparse::fixup_lane_sum(
                s,
                [&](Fe<Fr> &h, u32 j) {
                    require(j < tiles, "head read outside its tiles");
                    u32 w[8];
                    to_words(w, head[j]);
                    fe_unpack(h, w);
                },
                t, t_last, lane);
            sum = F.addmod(sum, to_u256(s));
        }
        out[r] = F.addmod(out[r], sum);
    }
    checked += access.loads > 0;
    return out;
}

// from the definition: wire(v) wire(z) / W summed over the row
std::vector<U256> expected(const Field &F, const U256 &winv, const Matrix &m)
{
    std::vector<U256> out(m.n_rows, ZERO);
    for (u32 r = 0; r < m.n_rows; r++)
        for (u32 k = m.row_ptr[r]; k < m.row_ptr[r + 1]; k++) out[r] = F.addmod(out[r], F.mulmod(F.mulmod(m.values[k], m.z[m.col[k]]), winv));
    return out;
}

template <class Fr>
void compare(const Field &F, const U256 &winv, const Matrix &m, const char *what)
{
    const std::vector<U256> got = run_product<Fr>(F, m, true), want = expected(F, winv, m);
    for (u32 r = 0; r < m.n_rows; r++) {
        if (!same(got[r], want[r])) {
            fprintf(stderr, "row %u of %u, nnz %u: ", r, m.n_rows, m.nnz);
            fail(what);
        }
        checked++;
    }
}

// a valid matrix from its row lengths; pick(k) gives the value and z entries
template <class Pick>
Matrix build(const std::vector<u32> &lengths, u32 n_cols, Pick &&pick)
{
    Matrix m;
    m.n_rows = (u32)lengths.size(), m.n_cols = n_cols;
    m.row_ptr.push_back(0);
    for (u32 len : lengths) m.row_ptr.push_back(m.row_ptr.back() + len);
    m.nnz = m.row_ptr.back();
    for (u32 k = 0; k < m.nnz; k++) {
        m.col.push_back((u32)(rng() % n_cols));
        m.values.push_back(pick(k));
    }
    for (u32 c = 0; c < n_cols; c++) m.z.push_back(pick(c + 1));
    return m;
}

std::vector<u32> random_lengths(u32 nnz)
{
    std::vector<u32> lengths;
    u32 have = 0;
    while (have < nnz) {
        u32 len = (u32)(rng() % 7);
        len = len > nnz - have ? nnz - have : len;
        lengths.push_back(len);
        have += len;
    }
    lengths.push_back(0);
    return lengths;
}

template <class Fr>
void run_field(bool long_row)
{
    Field F;
    F.p = from_words(Fr::PW);
    U256 pm1, pm2, one = {{1, 0, 0, 0}}, two = {{2, 0, 0, 0}}, w = one;
    sub(pm1, F.p, one);
    sub(pm2, F.p, two);
    for (int i = 0; i < 256; i++) w = F.addmod(w, w); // W mod p
    const U256 winv = F.powmod(w, pm2);
    require(same(F.mulmod(w, winv), one), "W^-1");
    auto all_pm1 = [&](u32) { return pm1; };
    auto any = [&](u32) { return random_below(F); };
    auto edge = [&](u32 k) { return k % 5 == 0 ? ZERO : k % 5 == 1 ? one : k % 5 == 2 ? pm1 : random_below(F); };

    // every value and every z p - 1; rows of length 1, 2, 3 (one product unpaired) and 4 T + 1, empty rows between them
    compare<Fr>(F, winv, build({1, 2, 3, 0, 4 * TILE + 1, 0, 0, 3, 2, 1, 1}, 7, all_pm1), "all p - 1");
    compare<Fr>(F, winv, build({4 * TILE + 1}, 1, all_pm1), "one row of 4 T + 1, one column, all p - 1");
    // nonzero counts around the tile size, row lengths 0 .. 6
    for (u32 nnz : {1u, 2u, 3u, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 4 * TILE + 3}) compare<Fr>(F, winv, build(random_lengths(nnz), 257, edge), "random rows");
    // rows that end at T - 1, at T, and start at T; one row of 3 T + 5
    compare<Fr>(F, winv, build({TILE - 1, 1, 5, TILE - 6, 3}, 11, any), "rows on tile ends");
    compare<Fr>(F, winv, build({TILE, TILE, 1}, 11, any), "rows that are tiles");
    compare<Fr>(F, winv, build({2, 3 * TILE + 5, 2}, 11, any), "a row over four tiles");
    // runs of empty rows: first, last, 2 T + 1 in the middle, one that ends where a tile begins
    {
        std::vector<u32> lengths(2 * TILE + 1 + 8, 0);
        lengths[3] = 2, lengths[4] = TILE - 2, lengths[lengths.size() - 3] = 5, lengths[lengths.size() - 2] = 1;
        compare<Fr>(F, winv, build(lengths, 5, any), "runs of empty rows");
        std::vector<u32> sparse_rows(3 * TILE, 0);
        sparse_rows[7] = 1, sparse_rows[2 * TILE + 1] = 1;
        compare<Fr>(F, winv, build(sparse_rows, 3, any), "3 T rows, two nonzeros");
    }
    if (long_row) compare<Fr>(F, winv, build({3, (panda_sparse::FIXUP_CHUNK + 1) * TILE + 9, 0, 4}, 9, any), "a row over more tiles than a fix-up step");

    // invalid structures: only the accesses count
    for (u32 nnz : {1u, 5u, TILE - 1, TILE + 1, 3 * TILE + 2}) {
        for (u32 n_rows : {1u, 2u, 7u, 300u, 2 * TILE + 3}) {
            for (int kind = 0; kind < 6; kind++) {
                Matrix m;
                m.n_rows = n_rows, m.n_cols = 1 + (u32)(rng() % 9), m.nnz = nnz;
                m.row_ptr.resize(n_rows + 1);
                for (u32 i = 0; i <= n_rows; i++) {
                    const u32 r32 = (u32)rng();
                    m.row_ptr[i] = kind == 0   ? 0xFFFFFFFFu
                                   : kind == 1 ? (n_rows - i) * (nnz / n_rows + 1) // decreasing
                                   : kind == 2 ? r32                                // anything
                                   : kind == 3 ? r32 % (2 * nnz + 1)                // near the legal range, unordered
                                   : kind == 4 ? 0u                                 // all zero: row_ptr[n_rows] != nnz
                                               : (i * (u64)nnz / n_rows > nnz ? nnz : (u32)(i * (u64)nnz / n_rows)); // legal rows, bad columns
                }
                for (u32 k = 0; k < nnz; k++) {
                    m.col.push_back(kind % 2 ? 0xFFFFFFFFu : (u32)rng());
                    m.values.push_back(k % 3 ? pm1 : random_below(F));
                }
                for (u32 c = 0; c < m.n_cols; c++) m.z.push_back(pm1);
                run_product<Fr>(F, m, false);
            }
        }
    }
}

} // namespace

int main()
{
    // the search alone: the last row at or below k, clamped
    {
        const u32 rp[] = {0, 0, 3, 3, 3, 8, 8};
        auto f = [&](u32 i) { return rp[i]; };
        const u32 want[8] = {1, 1, 1, 4, 4, 4, 4, 4};
        for (u32 k = 0; k < 8; k++) {
            require(panda_sparse::row_of(f, k, 0u, 5u) == want[k], "row_of");
            checked++;
        }
        require(panda_sparse::row_of(f, 100u, 0u, 5u) == 5 && panda_sparse::row_of(f, 2u, 3u, 5u) == 3, "row_of clamps");
    }
    run_field<Bn254Fr>(true);
    run_field<Bls377Fr>(false);
    run_field<Bls381Fr>(false);
    printf("ok %ld\n", checked);
    return 0;
}
