// Host run of Poseidon: panda_amd/csrc/poseidon.h -- the table, the round, the permutation and the sponge that the kernels run -- built for
// the HOST with FE29_CHECK (128-bit shadow column accumulators in the products, the operand ranges of fe_mul_shoup and fe_carry, and the
// classes of poseidon.h's bounds table asserted after every step).
//
// Without arguments: every bound at its edge.  The host twin is compared with 256-bit modular arithmetic written here (shift-and-add
// products on four 64-bit words, no Montgomery form, plain residues) for the three fields, t = 2 and t = 5, each alpha the field admits
// (BN254 5, 7, 11, 17; BLS12-377 11, 17; BLS12-381 5, 7, 17 -- and alpha_valid must say exactly that), with every matrix entry and round
// constant equal to p - 1, to 0, to 1 and random, on states of all p - 1, all 0 and mixed, for R_F = 2 with R_P = 0, R_F = 4 with R_P = 3
// and once the largest shape, R_F = 16 with R_P = 128; the sponge over 1, t - 1, t and 2 (t - 1) + 1 elements of p - 1.  Prints "ok N".
//
// With a file argument: reads "field t alpha R_F R_P n", then (R_F + R_P) t round constants, t t matrix entries and n t state elements as
// hexadecimal wire values, and prints the n t elements of the permuted states the same way.  tests/test_poseidon.py compares them with
// tests/poseidon_ref.py.
// Test infrastructure: compiled and run by tests/test_poseidon.py with g++.
#define FE29_CHECK 1
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../panda_amd/csrc/poseidon.h"

using namespace panda29;
typedef uint64_t u64;

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

const U256 ZERO = {{0, 0, 0, 0}}, ONE = {{1, 0, 0, 0}};

struct Field {
    U256 p, wire_one; // W mod p
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
    U256 powsmall(const U256 &a, unsigned e) const
    {
        U256 r = ONE;
        for (unsigned k = 0; k < e; k++) r = mulmod(r, a);
        return r;
    }
    U256 to_wire(const U256 &x) const { return mulmod(x, wire_one); }
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

template <class Fr>
Field field_of()
{
    Field F;
    F.p = from_words(Fr::PW);
    U256 v = ONE; // 2^256 mod p by 256 doublings
    for (int k = 0; k < 256; k++) v = F.addmod(v, v);
    F.wire_one = v;
    return F;
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

void require(bool ok, const char *what)
{
    if (!ok) {
        fprintf(stderr, "failed: %s\n", what);
        exit(1);
    }
}

// a parameter set on plain residues
struct Params {
    unsigned t, alpha, rf, rp;
    std::vector<U256> rc, mds;
};

std::vector<u32> wire_words(const Field &F, const std::vector<U256> &plain)
{
    std::vector<u32> w(plain.size() * 8);
    for (size_t k = 0; k < plain.size(); k++) to_words(&w[8 * k], F.to_wire(plain[k]));
    return w;
}

// the definition, on plain residues
void ref_permute(const Field &F, const Params &P, std::vector<U256> &s)
{
    const unsigned t = P.t;
    for (unsigned r = 0; r < P.rf + P.rp; r++) {
        const bool full = r < P.rf / 2 || r >= P.rf / 2 + P.rp;
        for (unsigned j = 0; j < t; j++) s[j] = F.addmod(s[j], P.rc[r * t + j]);
        for (unsigned j = 0; j < (full ? t : 1u); j++) s[j] = F.powsmall(s[j], P.alpha);
        std::vector<U256> n(t, ZERO);
        for (unsigned i = 0; i < t; i++)
            for (unsigned j = 0; j < t; j++) n[i] = F.addmod(n[i], F.mulmod(P.mds[i * t + j], s[j]));
        s = n;
    }
}
U256 ref_sponge(const Field &F, const Params &P, const U256 &tag, const std::vector<U256> &msg)
{
    std::vector<U256> s(P.t, ZERO);
    s[0] = tag;
    for (size_t j0 = 0; j0 < msg.size(); j0 += P.t - 1) {
        for (unsigned k = 0; k + 1 < P.t && j0 + k < msg.size(); k++) s[1 + k] = F.addmod(s[1 + k], msg[j0 + k]);
        ref_permute(F, P, s);
    }
    return s[0];
}

template <class Fr>
std::vector<u32> build(const Field &F, const Params &P)
{
    const std::vector<u32> rc = wire_words(F, P.rc), mds = wire_words(F, P.mds);
    require(panda_hash::params_valid<Fr>(P.t, P.alpha, P.rf, P.rp, rc.data(), mds.data()), "a valid parameter set was refused");
    std::vector<u32> table(panda_hash::table_words(P.t, P.rf + P.rp));
    panda_hash::build_table<Fr>(table.data(), P.t, P.alpha, P.rf, P.rp, rc.data(), mds.data());
    return table;
}

// what store_elem does: any value the routines leave -> the canonical wire value
template <class Fr>
U256 canonical(Fe<Fr> v)
{
    fe_reduce_small(v);
    u32 w[8];
    fe_pack(w, v);
    return from_words(w);
}
template <class Fr>
Fe<Fr> element(const Field &F, const U256 &plain)
{
    u32 w[8];
    to_words(w, F.to_wire(plain));
    Fe<Fr> v;
    fe_unpack(v, w);
    return v;
}

template <class Fr, int T>
void check_permute(const Field &F, const Params &P, const std::vector<u32> &table, const std::vector<U256> &state)
{
    Fe<Fr> s[T];
    for (int j = 0; j < T; j++) s[j] = element<Fr>(F, state[j]);
    panda_hash::permute<Fr, T>(s, table.data(), P.alpha, P.rf, P.rp);
    std::vector<U256> want = state;
    ref_permute(F, P, want);
    for (int j = 0; j < T; j++) {
        require(same(canonical(s[j]), F.to_wire(want[j])), "the permutation differs from the definition");
        checked++;
    }
}

template <class Fr, int T>
void check_sponge(const Field &F, const Params &P, const std::vector<u32> &table, const U256 &tag, const std::vector<U256> &msg)
{
    Fe<Fr> h;
    panda_hash::sponge<Fr, T>(h, element<Fr>(F, tag), msg.size(), [&](Fe<Fr> &m, u64 j) { m = element<Fr>(F, msg[j]); }, table.data(), P.alpha, P.rf, P.rp);
    require(same(canonical(h), F.to_wire(ref_sponge(F, P, tag, msg))), "the sponge differs from the definition");
    checked++;
}

template <class Fr, int T>
void run_width(const Field &F, unsigned alpha, bool largest)
{
    U256 pm1;
    sub(pm1, F.p, ONE);
    const unsigned shapes[3][2] = {{2, 0}, {4, 3}, {panda_hash::MAX_FULL_ROUNDS, panda_hash::MAX_PARTIAL_ROUNDS}};
    for (int shape = 0; shape < (largest ? 3 : 2); shape++)
        for (int fill = 0; fill < 4; fill++) {
            if (shape == 2 && fill != 0 && fill != 3) continue;
            Params P = {(unsigned)T, alpha, shapes[shape][0], shapes[shape][1], {}, {}};
            const size_t n_rc = (size_t)(P.rf + P.rp) * T;
            for (size_t k = 0; k < n_rc + T * T; k++) {
                const U256 v = fill == 0 ? pm1 : fill == 1 ? ZERO : fill == 2 ? ONE : random_below(F);
                (k < n_rc ? P.rc : P.mds).push_back(v);
            }
            const std::vector<u32> table = build<Fr>(F, P);
            std::vector<U256> all_max(T, pm1), all_zero(T, ZERO), mixed(T);
            for (int j = 0; j < T; j++) mixed[j] = j % 3 == 0 ? pm1 : j % 3 == 1 ? random_below(F) : ONE;
            check_permute<Fr, T>(F, P, table, all_max);
            check_permute<Fr, T>(F, P, table, all_zero);
            check_permute<Fr, T>(F, P, table, mixed);
            if (shape == 1 && (fill == 0 || fill == 3))
                for (size_t len : {(size_t)1, (size_t)T - 1, (size_t)T, (size_t)2 * (T - 1) + 1})
                    check_sponge<Fr, T>(F, P, table, pm1, std::vector<U256>(len, pm1));
        }
}

template <class Fr>
void run_field(const unsigned (&alphas)[4], unsigned n_alphas)
{
    const Field F = field_of<Fr>();
    for (unsigned alpha = 0; alpha < 20; alpha++) {
        bool listed = false;
        for (unsigned k = 0; k < n_alphas; k++) listed |= alphas[k] == alpha;
        require(panda_hash::alpha_valid<Fr>(alpha) == listed, "alpha_valid disagrees with the field's list");
        checked++;
    }
    for (unsigned k = 0; k < n_alphas; k++) {
        run_width<Fr, 2>(F, alphas[k], false);
        run_width<Fr, 5>(F, alphas[k], k == 0);
    }
    // refusals of the parameter check: a constant equal to the modulus, the shapes
    Params P = {3, alphas[0], 2, 1, std::vector<U256>(9, ONE), std::vector<U256>(9, ONE)};
    std::vector<u32> rc = wire_words(F, P.rc), mds = wire_words(F, P.mds);
    require(panda_hash::params_valid<Fr>(3, alphas[0], 2, 1, rc.data(), mds.data()), "valid");
    require(!panda_hash::params_valid<Fr>(3, alphas[0], 3, 1, rc.data(), mds.data()), "odd R_F");
    require(!panda_hash::params_valid<Fr>(3, alphas[0], 0, 1, rc.data(), mds.data()), "R_F 0");
    require(!panda_hash::params_valid<Fr>(6, alphas[0], 2, 1, rc.data(), mds.data()) && !panda_hash::params_valid<Fr>(1, alphas[0], 2, 1, rc.data(), mds.data()), "width");
    to_words(&rc[8 * 8], F.p);
    require(!panda_hash::params_valid<Fr>(3, alphas[0], 2, 1, rc.data(), mds.data()), "a round constant equal to the modulus");
    to_words(&rc[8 * 8], ONE);
    to_words(&mds[8 * 8], F.p);
    require(!panda_hash::params_valid<Fr>(3, alphas[0], 2, 1, rc.data(), mds.data()), "a matrix entry equal to the modulus");
    checked += 6;
}

// ------------------------------------------------------------------------------------------------- the file mode

bool read_hex(FILE *f, U256 &v)
{
    char text[80];
    if (fscanf(f, "%79s", text) != 1) return false;
    v = ZERO;
    for (const char *c = text; *c; c++) {
        const int d = *c >= '0' && *c <= '9' ? *c - '0' : *c >= 'a' && *c <= 'f' ? *c - 'a' + 10 : -1;
        if (d < 0) return false;
        for (int i = 3; i > 0; i--) v.w[i] = (v.w[i] << 4) | (v.w[i - 1] >> 60);
        v.w[0] = (v.w[0] << 4) | (u64)d;
    }
    return true;
}

template <class Fr, int T>
int run_file_width(FILE *f, unsigned alpha, unsigned rf, unsigned rp, unsigned n)
{
    const size_t n_rc = (size_t)(rf + rp) * T;
    std::vector<u32> rc(n_rc * 8), mds((size_t)T * T * 8);
    U256 v;
    for (size_t k = 0; k < n_rc + T * T; k++) {
        if (!read_hex(f, v)) return 2;
        to_words(k < n_rc ? &rc[8 * k] : &mds[8 * (k - n_rc)], v);
    }
    if (!panda_hash::params_valid<Fr>(T, alpha, rf, rp, rc.data(), mds.data())) return 3;
    std::vector<u32> table(panda_hash::table_words(T, rf + rp));
    panda_hash::build_table<Fr>(table.data(), T, alpha, rf, rp, rc.data(), mds.data());
    for (unsigned i = 0; i < n; i++) {
        Fe<Fr> s[T];
        for (int j = 0; j < T; j++) {
            if (!read_hex(f, v)) return 2;
            u32 w[8];
            to_words(w, v);
            fe_unpack(s[j], w);
        }
        panda_hash::permute<Fr, T>(s, table.data(), alpha, rf, rp);
        for (int j = 0; j < T; j++) {
            const U256 out = canonical(s[j]);
            printf("%016llx%016llx%016llx%016llx\n", (unsigned long long)out.w[3], (unsigned long long)out.w[2], (unsigned long long)out.w[1],
                   (unsigned long long)out.w[0]);
        }
    }
    return 0;
}

template <class Fr>
int run_file_field(FILE *f, unsigned t, unsigned alpha, unsigned rf, unsigned rp, unsigned n)
{
    switch (t) {
    case 2: return run_file_width<Fr, 2>(f, alpha, rf, rp, n);
    case 3: return run_file_width<Fr, 3>(f, alpha, rf, rp, n);
    case 4: return run_file_width<Fr, 4>(f, alpha, rf, rp, n);
    case 5: return run_file_width<Fr, 5>(f, alpha, rf, rp, n);
    default: return 3;
    }
}

int run_file(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) return 2;
    unsigned field, t, alpha, rf, rp, n;
    if (fscanf(f, "%u %u %u %u %u %u", &field, &t, &alpha, &rf, &rp, &n) != 6) return 2;
    if (!panda_hash::shape_valid(t, rf, rp)) return 3;
    const int rc = field == 0 ? run_file_field<Bn254Fr>(f, t, alpha, rf, rp, n)
                 : field == 1 ? run_file_field<Bls377Fr>(f, t, alpha, rf, rp, n)
                 : field == 2 ? run_file_field<Bls381Fr>(f, t, alpha, rf, rp, n)
                              : 3;
    fclose(f);
    return rc;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc > 1) return run_file(argv[1]);
    run_field<Bn254Fr>({5, 7, 11, 17}, 4);
    run_field<Bls377Fr>({11, 17, 0, 0}, 2);
    run_field<Bls381Fr>({5, 7, 17, 0}, 3);
    // the tree's plan
    panda_hash::TreePlan plan;
    u64 offset[28];
    require(panda_hash::tree_plan(plan, 3, 28, offset) && plan.nodes == (1ull << 28) - 1 && offset[27] == plan.nodes - 1 && plan.top_levels == 9, "plan, arity 2");
    require(!panda_hash::tree_plan(plan, 3, 29, nullptr) && !panda_hash::tree_plan(plan, 2, 4, nullptr) && !panda_hash::tree_plan(plan, 5, 15, nullptr), "plan refusals");
    checked += 2;
    printf("ok %ld\n", checked);
    return 0;
}
