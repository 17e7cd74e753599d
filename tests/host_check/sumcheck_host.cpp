// Host run of the sumcheck arithmetic: panda_amd/csrc/sumcheck.h -- the round's program builder, the PANDA_HD per-pair routine the round
// kernel runs (plain, and fused with the fold in front), the fold and the eq table's factors -- built for the HOST with FE29_CHECK (128-bit
// shadow column accumulators in fe_mul / fe_mul_add; the limb class and value bound of sumcheck.h's table asserted after every step: the
// points and differences canonical, the products and accumulators tight and below 2p).  The results are compared with 256-bit modular
// arithmetic written here (shift-and-add products on four 64-bit words, no Montgomery form), at the edges of the bound argument: every
// operand p - 1, lo = 0 with hi = p - 1 and the reverse, 64 terms of degree 4, one term of degree 256, degree-0 terms, coefficients 0 and
// p - 1, 1 and 8 evaluation points, challenges 0, 1 and p - 1, both binding orders, the three fields.
// Test infrastructure: compiled and run by tests/test_sumcheck.py with g++; prints "ok <checked values>" and exits 0.
#define FE29_CHECK 1
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../panda_amd/csrc/sumcheck.h"

using namespace panda29;
using panda_sumcheck::EqFactors;
using panda_sumcheck::Round;

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
    U256 submod(const U256 &a, const U256 &b) const
    {
        U256 r;
        if (geq(a, b)) {
            sub(r, a, b);
            return r;
        }
        sub(r, p, b);
        return addmod(a, r);
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
    fprintf(stderr, "mismatch: %s\n", what);
    exit(1);
}

template <class Fr>
void expect(const Fe<Fr> &got, const U256 &want, const char *what)
{
    panda_sumcheck::check_canonical(got);
    u32 g[8], w[8];
    fe_pack(g, got);
    to_words(w, want);
    if (memcmp(g, w, 32) != 0) fail(what);
    checked++;
}

struct Expr {
    unsigned n_columns;
    std::vector<unsigned> degrees;
    std::vector<u32> factors; // {column, 0} pairs
    std::vector<U256> coeffs;
};

enum Fill { RANDOM, ALL_MINUS_ONE, LO_ZERO_HI_MINUS_ONE, LO_MINUS_ONE_HI_ZERO };

// the pair (lo, hi) of index i in a table of 2 * pairs elements
void pair_of(unsigned &lo, unsigned &hi, unsigned i, unsigned pairs, unsigned order)
{
    lo = order ? i : 2 * i;
    hi = order ? i + pairs : 2 * i + 1;
}

// g(t) over tables of `len` wire residues, the definition: a term of degree d is k prod(w) / W^d
template <int NE>
void reference_round(U256 (&g)[NE], const Field &F, const U256 &winv, const Expr &x, const std::vector<std::vector<U256>> &tab, unsigned len, unsigned order)
{
    for (int t = 0; t < NE; t++) g[t] = ZERO;
    for (unsigned i = 0; i < len / 2; i++) {
        unsigned il, ih;
        pair_of(il, ih, i, len / 2, order);
        for (int t = 0; t < NE; t++) {
            size_t f = 0;
            for (size_t term = 0; term < x.degrees.size(); term++) {
                U256 v = x.coeffs[term];
                for (unsigned d = 0; d < x.degrees[term]; d++, f++) {
                    const std::vector<U256> &col = tab[x.factors[2 * f]];
                    U256 pt = col[il];
                    const U256 delta = F.submod(col[ih], col[il]);
                    for (int s = 0; s < t; s++) pt = F.addmod(pt, delta);
                    v = F.mulmod(F.mulmod(v, pt), winv);
                }
                g[t] = F.addmod(g[t], v);
            }
        }
    }
}

template <class Fr, int NE>
void run_case(const Field &F, const U256 &winv, const Expr &x, unsigned log_n, unsigned order, Fill fill, const U256 &challenge)
{
    const unsigned len = 1u << log_n;
    U256 pm1;
    sub(pm1, F.p, U256{{1, 0, 0, 0}});
    std::vector<std::vector<u32>> cols(x.n_columns, std::vector<u32>((size_t)len * 8)), out(x.n_columns, std::vector<u32>((size_t)len * 4, 0xA5A5A5A5u));
    std::vector<std::vector<U256>> vals(x.n_columns, std::vector<U256>(len));
    std::vector<const void *> ptrs(x.n_columns);
    std::vector<void *> fptrs(x.n_columns);
    for (unsigned k = 0; k < x.n_columns; k++) {
        for (unsigned j = 0; j < len; j++) {
            const bool hi = order ? j >= len / 2 : (j & 1);
            vals[k][j] = fill == RANDOM ? random_below(F) : fill == ALL_MINUS_ONE ? pm1 : (fill == LO_ZERO_HI_MINUS_ONE) == hi ? pm1 : ZERO;
            to_words(&cols[k][(size_t)j * 8], vals[k][j]);
        }
        ptrs[k] = cols[k].data();
        fptrs[k] = out[k].data();
    }
    std::vector<u32> coeff_words(x.coeffs.size() * 8), r_words(8);
    for (size_t t = 0; t < x.coeffs.size(); t++) to_words(&coeff_words[t * 8], x.coeffs[t]);
    to_words(r_words.data(), challenge);

    // the plain round
    {
        Round R;
        panda_sumcheck::build_round<Fr>(R, ptrs.data(), x.n_columns, coeff_words.data(), x.degrees.data(), (unsigned)x.degrees.size(), x.factors.data(), nullptr,
                                        nullptr);
        Fe<Fr> sum[NE];
        for (int t = 0; t < NE; t++) fe_zero(sum[t]);
        for (unsigned i = 0; i < len / 2; i++) {
            unsigned il, ih;
            pair_of(il, ih, i, len / 2, order);
            Fe<Fr> acc[NE];
            panda_sumcheck::round_pair<Fr, NE>(acc, R.prog, [&](Fe<Fr> &lo, Fe<Fr> &hi, u32 f) {
                const u32 *src = reinterpret_cast<const u32 *>(R.prog.column[R.prog.factor[f][0]]);
                fe_unpack(lo, src + (size_t)il * 8);
                fe_unpack(hi, src + (size_t)ih * 8);
            });
            for (int t = 0; t < NE; t++) panda_poly::add_canon(sum[t], sum[t], acc[t]);
        }
        U256 want[NE];
        reference_round<NE>(want, F, winv, x, vals, len, order);
        for (int t = 0; t < NE; t++) expect(sum[t], want[t], "plain round");
    }
    if (log_n < 2) return;

    // the fused round: fold with the challenge, then the round over the folded tables, the folded elements stored once per column
    std::vector<std::vector<U256>> folded(x.n_columns, std::vector<U256>(len / 2));
    for (unsigned k = 0; k < x.n_columns; k++)
        for (unsigned j = 0; j < len / 2; j++) {
            unsigned il, ih;
            pair_of(il, ih, j, len / 2, order);
            folded[k][j] = F.addmod(vals[k][il], F.mulmod(F.mulmod(F.submod(vals[k][ih], vals[k][il]), challenge), winv));
        }
    Round R;
    panda_sumcheck::build_round<Fr>(R, ptrs.data(), x.n_columns, coeff_words.data(), x.degrees.data(), (unsigned)x.degrees.size(), x.factors.data(), fptrs.data(),
                                    r_words.data());
    Fe<Fr> rc, sum[NE];
    fe_const(rc, R.challenge);
    panda_sumcheck::check_canonical(rc);
    for (int t = 0; t < NE; t++) fe_zero(sum[t]);
    std::vector<unsigned> stores(x.n_columns, 0);
    for (unsigned i = 0; i < len / 4; i++) {
        unsigned jl, jh, l0, l1, h0, h1;
        pair_of(jl, jh, i, len / 4, order);
        pair_of(l0, l1, jl, len / 2, order);
        pair_of(h0, h1, jh, len / 2, order);
        auto folded_pair = [&](Fe<Fr> &lo, Fe<Fr> &hi, u32 column, bool store) {
            const u32 *src = reinterpret_cast<const u32 *>(R.prog.column[column]);
            Fe<Fr> a0, a1, b0, b1;
            fe_unpack(a0, src + (size_t)l0 * 8);
            fe_unpack(a1, src + (size_t)l1 * 8);
            fe_unpack(b0, src + (size_t)h0 * 8);
            fe_unpack(b1, src + (size_t)h1 * 8);
            panda_sumcheck::fold_canon(lo, a0, a1, rc);
            panda_sumcheck::fold_canon(hi, b0, b1, rc);
            if (store) {
                u32 *dst = reinterpret_cast<u32 *>(R.folded[column]);
                fe_pack(dst + (size_t)jl * 8, lo);
                fe_pack(dst + (size_t)jh * 8, hi);
                expect(lo, folded[column][jl], "folded lo");
                expect(hi, folded[column][jh], "folded hi");
                if (i == 0) stores[column]++;
            }
        };
        Fe<Fr> acc[NE];
        panda_sumcheck::round_pair<Fr, NE>(acc, R.prog, [&](Fe<Fr> &lo, Fe<Fr> &hi, u32 f) { folded_pair(lo, hi, R.prog.factor[f][0], R.store[f] != 0); });
        for (u32 q = 0; q < R.n_idle; q++) {
            Fe<Fr> lo, hi;
            folded_pair(lo, hi, R.idle[q], true);
        }
        for (int t = 0; t < NE; t++) panda_poly::add_canon(sum[t], sum[t], acc[t]);
    }
    for (unsigned k = 0; k < x.n_columns; k++) {
        if (stores[k] != 1) fail("a column's folded pair is stored exactly once");
        for (unsigned j = 0; j < len / 2; j++) {
            u32 w[8];
            to_words(w, folded[k][j]);
            if (memcmp(w, &out[k][(size_t)j * 8], 32) != 0) fail("folded table");
        }
    }
    U256 want[NE];
    reference_round<NE>(want, F, winv, x, folded, len / 2, order);
    for (int t = 0; t < NE; t++) expect(sum[t], want[t], "fused round");
}

template <class Fr>
void run_eq(const Field &F, const U256 &w, const U256 &winv, const std::vector<U256> &point)
{
    const unsigned log_n = (unsigned)point.size();
    std::vector<u32> words(8 * (log_n + 1));
    for (unsigned j = 0; j < log_n; j++) to_words(&words[8 * j], point[j]);
    EqFactors T;
    panda_sumcheck::build_eq_factors<Fr>(T, words.data(), log_n);
    U256 total = ZERO;
    for (u32 x = 0; x < (1u << log_n); x++) {
        U256 want = w; // the wire's one
        for (unsigned j = 0; j < log_n; j++) {
            const U256 f = (x >> j) & 1 ? point[j] : F.submod(w, point[j]);
            want = F.mulmod(F.mulmod(want, f), winv);
        }
        Fe<Fr> got;
        panda_sumcheck::eq_element(got, T, x, log_n);
        expect(got, want, "eq table");
        total = F.addmod(total, want);
    }
    if (memcmp(&total, &w, sizeof(U256)) != 0) fail("the eq table sums to one");
}

template <class Fr>
void run_field()
{
    Field F;
    F.p = from_words(Fr::PW);
    U256 pm1, pm2, w = {{1, 0, 0, 0}};
    sub(pm1, F.p, U256{{1, 0, 0, 0}});
    sub(pm2, F.p, U256{{2, 0, 0, 0}});
    for (int i = 0; i < 256; i++) w = F.addmod(w, w); // W mod p: the wire's one
    const U256 winv = F.powmod(w, pm2);
    const U256 wire_minus_one = F.submod(ZERO, w);
    const U256 challenges[4] = {ZERO, w, wire_minus_one, random_below(F)};
    const Fill fills[4] = {RANDOM, ALL_MINUS_ONE, LO_ZERO_HI_MINUS_ONE, LO_MINUS_ONE_HI_ZERO};
    for (int fi = 0; fi < 4; fi++) {
        const Fill fill = fills[fi];
        const U256 k_edge = fill == RANDOM ? random_below(F) : pm1;
        Expr many{3, {}, {}, {}}; // 64 terms of degree 4
        for (unsigned t = 0; t < 64; t++) {
            many.degrees.push_back(4);
            many.coeffs.push_back(fill == RANDOM ? random_below(F) : pm1);
            for (unsigned d = 0; d < 4; d++) {
                many.factors.push_back((t + d) % 3);
                many.factors.push_back(0);
            }
        }
        Expr deep{3, {256}, {}, {k_edge}}; // one term of degree 256; column 2 is named by no factor
        for (unsigned d = 0; d < 256; d++) {
            deep.factors.push_back(d & 1);
            deep.factors.push_back(0);
        }
        Expr mix{2, {0, 1, 2, 0, 3, 1}, {}, {k_edge, ZERO, pm1, ZERO, k_edge, w}}; // degree 0, coefficients 0 and p - 1, a column twice in a term
        const u32 mix_columns[7] = {0, 1, 1, 0, 0, 1, 1};
        for (unsigned f = 0; f < 7; f++) {
            mix.factors.push_back(mix_columns[f]);
            mix.factors.push_back(0);
        }
        Expr constant{1, {0}, {}, {k_edge}};
        for (unsigned order = 0; order < 2; order++)
            for (int c = 0; c < 4; c++) {
                const U256 &r = challenges[c];
                run_case<Fr, 8>(F, winv, mix, 3, order, fill, r);
                run_case<Fr, 1>(F, winv, many, 2, order, fill, r);
                if (c != 3 && fill != ALL_MINUS_ONE) continue; // the long expressions: every challenge at p - 1, a random one at the other fills
                run_case<Fr, 8>(F, winv, many, 2, order, fill, r);
                run_case<Fr, 8>(F, winv, deep, 2, order, fill, r);
                run_case<Fr, 1>(F, winv, deep, 2, order, fill, r);
                run_case<Fr, 1>(F, winv, mix, 1, order, fill, r);
                run_case<Fr, 8>(F, winv, constant, 2, order, fill, r);
            }
    }
    run_eq<Fr>(F, w, winv, {});
    run_eq<Fr>(F, w, winv, {ZERO});
    run_eq<Fr>(F, w, winv, {w, ZERO, w});
    run_eq<Fr>(F, w, winv, {wire_minus_one, wire_minus_one, wire_minus_one, wire_minus_one});
    run_eq<Fr>(F, w, winv, {random_below(F), w, random_below(F), wire_minus_one, random_below(F)});
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
