// Host run of panda_poly_sum_of_products' arithmetic: panda_amd/csrc/poly_terms.h -- the program builder with the wire form's constants
// folded in and the PANDA_HD per-element routine the kernel runs -- built for the HOST with FE29_CHECK (128-bit shadow column accumulators
// in fe_mul / fe_mul_add; tight limbs and a value below 2p asserted after every product, every term and the scale).  The results are
// compared with 256-bit modular arithmetic written here (shift-and-add products on four 64-bit words, no Montgomery form), at the edges
// of the bound argument: every operand p - 1, 64 terms of degree 4, one term of degree 256, coefficients 0 and p - 1, degree-0 terms,
// rotations that wrap, the three scale modes, the three fields, one and two elements per call of the routine.
// Test infrastructure: compiled and run by tests/test_poly_sum_of_products.py with g++; prints "ok <checked elements>" and exits 0.
#define FE29_CHECK 1
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../panda_amd/csrc/poly_terms.h"

using namespace panda29;
using panda_sop::Program;

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
// a + b and a - b on 257 bits: the carry / borrow out is returned
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
        U256 r = {{0, 0, 0, 0}};
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
    r.w[3] &= (~0ull) >> 1; // every modulus here is above 2^252: at most a few subtractions
    while (geq(r, F.p)) sub(r, r, F.p);
    return r;
}

struct Case {
    unsigned n, batch, n_columns;
    std::vector<unsigned> degrees;
    std::vector<u32> factors; // {column, rotation as the bits of an int32_t} pairs
    std::vector<U256> coeffs, scales;
    unsigned scale_mode;
    int fill; // columns: 0 random, 1 every element p - 1
};

long checked = 0;

template <class Fr, int E>
void run_case(const Field &F, const U256 &winv, const Case &c)
{
    const unsigned n = c.n, batch = c.batch;
    U256 pm1;
    sub(pm1, F.p, U256{{1, 0, 0, 0}});
    std::vector<std::vector<u32>> cols(c.n_columns, std::vector<u32>((size_t)batch * n * 8));
    std::vector<std::vector<U256>> vals(c.n_columns, std::vector<U256>((size_t)batch * n));
    std::vector<const void *> ptrs(c.n_columns);
    for (unsigned k = 0; k < c.n_columns; k++) {
        for (size_t j = 0; j < (size_t)batch * n; j++) {
            vals[k][j] = c.fill ? pm1 : random_below(F);
            to_words(&cols[k][j * 8], vals[k][j]);
        }
        ptrs[k] = cols[k].data();
    }
    std::vector<u32> coeff_words(c.coeffs.size() * 8), scale_words(c.scales.size() * 8 + 8);
    for (size_t t = 0; t < c.coeffs.size(); t++) to_words(&coeff_words[t * 8], c.coeffs[t]);
    for (size_t j = 0; j < c.scales.size(); j++) to_words(&scale_words[j * 8], c.scales[j]);
    Program P;
    panda_sop::build_program<Fr>(P, ptrs.data(), c.n_columns, coeff_words.data(), c.degrees.data(), (unsigned)c.degrees.size(), c.factors.data(),
                                 c.scales.empty() ? nullptr : scale_words.data(), (unsigned)c.scales.size(), c.scale_mode, n);
    for (unsigned t = 0; t < P.n_terms; t++) // the folded constants are canonical
        for (int l = 0; l < panda_sop::NL; l++)
            if (P.coeff[t][l] >= (1u << 29)) abort();
    for (unsigned p = 0; p < batch; p++)
        for (unsigned i0 = 0; i0 < n; i0 += E) {
            u32 idx[E];
            for (int e = 0; e < E; e++) idx[e] = i0 + e < n ? i0 + e : 0;
            Fe<Fr> r[E];
            panda_sop::evaluate<Fr, E>(r, P, p, idx, n, [&](Fe<Fr> &v, u32 column, u32 j) {
                if (j >= n || column >= c.n_columns) abort();
                fe_unpack(v, reinterpret_cast<const u32 *>(P.column[column]) + ((size_t)p * n + j) * 8);
            });
            for (int e = 0; e < E; e++) {
                // what store_elem does
                fe_reduce_small(r[e]);
                u32 got[8];
                fe_pack(got, r[e]);
                // the definition, on wire residues: a term of degree d is k prod(w) / W^d, a scale one more division by W
                U256 sum = {{0, 0, 0, 0}};
                size_t f = 0;
                for (size_t t = 0; t < c.degrees.size(); t++) {
                    U256 term = c.coeffs[t];
                    for (unsigned d = 0; d < c.degrees[t]; d++, f++) {
                        const int64_t rot = (int64_t)(int32_t)c.factors[2 * f + 1];
                        const unsigned j = (unsigned)((((int64_t)idx[e] + rot) % (int64_t)n + (int64_t)n) % (int64_t)n);
                        term = F.mulmod(F.mulmod(term, vals[c.factors[2 * f]][(size_t)p * n + j]), winv);
                    }
                    sum = F.addmod(sum, term);
                }
                if (c.scale_mode == panda_sop::SCALE_PER_VECTOR) sum = F.mulmod(F.mulmod(sum, c.scales[p % c.scales.size()]), winv);
                if (c.scale_mode == panda_sop::SCALE_CYCLIC) sum = F.mulmod(F.mulmod(sum, c.scales[idx[e] % c.scales.size()]), winv);
                u32 want[8];
                to_words(want, sum);
                if (memcmp(got, want, 32) != 0) {
                    fprintf(stderr, "mismatch: n %u batch %u terms %zu vector %u index %u E %d\n", n, batch, c.degrees.size(), p, idx[e], E);
                    exit(1);
                }
                checked++;
            }
        }
}

void push_factor(Case &c, unsigned column, int32_t rotation)
{
    c.factors.push_back(column);
    c.factors.push_back((u32)rotation);
}

template <class Fr>
void run_field()
{
    Field F;
    F.p = from_words(Fr::PW);
    U256 pm1, pm2, w = {{1, 0, 0, 0}};
    sub(pm1, F.p, U256{{1, 0, 0, 0}});
    sub(pm2, F.p, U256{{2, 0, 0, 0}});
    for (int i = 0; i < 256; i++) w = F.addmod(w, w); // W mod p
    const U256 winv = F.powmod(w, pm2);
    const U256 zero = {{0, 0, 0, 0}};
    std::vector<Case> cases;
    for (int fill = 0; fill < 2; fill++)
        for (unsigned mode = 0; mode < 3; mode++) {
            const U256 k_edge = fill ? pm1 : random_below(F);
            Case c{5, 2, 3, {}, {}, {}, {}, mode, fill}; // 64 terms of degree 4, rotations on every factor
            for (unsigned t = 0; t < 64; t++) {
                c.degrees.push_back(4);
                c.coeffs.push_back(fill ? pm1 : random_below(F));
                for (unsigned d = 0; d < 4; d++) push_factor(c, (t + d) % 3, (int32_t)(t * 7 + d) - 100);
            }
            if (mode)
                for (unsigned j = 0; j < (mode == 1 ? 3u : 16u); j++) c.scales.push_back(fill ? pm1 : random_below(F));
            cases.push_back(c);
            Case one{3, 2, 2, {256}, {}, {k_edge}, c.scales, mode, fill}; // one term of degree 256
            for (unsigned d = 0; d < 256; d++) push_factor(one, d & 1, d % 5 == 0 ? INT32_MIN : (int32_t)d - 128);
            cases.push_back(one);
            Case mix{4, 3, 2, {0, 1, 2, 0, 3, 1}, {}, {k_edge, zero, pm1, zero, k_edge, w}, c.scales, mode, fill}; // degree 0, coefficients 0 and p - 1
            const int32_t rots[7] = {0, 1, -1, 4, 5, -4, INT32_MAX};
            for (unsigned f = 0; f < 7; f++) push_factor(mix, f & 1, rots[f]);
            cases.push_back(mix);
            Case fill_only{1, 2, 1, {0}, {}, {k_edge}, c.scales, mode, fill}; // n = 1, nothing but a constant
            cases.push_back(fill_only);
        }
    for (const Case &c : cases) {
        run_case<Fr, 1>(F, winv, c);
        run_case<Fr, 2>(F, winv, c);
    }
}

} // namespace

int main()
{
    run_field<Bn254Fr>();
    run_field<Bls377Fr>();
    run_field<Bls381Fr>();
    printf("ok %ld\n", checked);
    return 0;
}
