// points_mul_host.cpp -- the routines of panda_amd/csrc/points_mul.h on the host under FE29_CHECK (every column accumulator and every limb
// range of fe29.h is asserted), against the affine group law in integer arithmetic of ec_ref.h, as tests/host_check/ec_ntt_host.cpp
// does for ec_ntt.h.  For the three curves:
//   scalar_bits / scalar_mul   k in {0, 1, 2, r - 1, one with the top bit of r set, the single bit 2^77, a 64-bit and a 128-bit value}: every
//                              loop length from k's own bit count up to 256 gives k P; the base in affine and in XYZZ form; P the identity
//   add_affine_wire            A the identity, A generic, A = k P (the doubling path), A = -k P (the identity)
//   scalar_from_wire           Montgomery wire residue -> the integer
//   power_table / power_scalar c s^i for i in {0, 1, 2^27 + 5, 2^28 - 1} against modular exponentiation
// Every stored point is checked against the stored-point bounds of ec_ntt.h.  Prints "ok <checks>"; any failure aborts with a message.
// Build: g++ -O2 -std=c++17 (tests/test_points_mul.py does).
#include "ec_ref.h"

#include <initializer_list>

#include "../../panda_amd/csrc/points_mul.h"

using namespace panda_pmul;

static Big random_words(int words)
{
    Big r;
    for (int i = 0; i < words; i++) r.w[i] = (uint32_t)rnd();
    r.w[words - 1] |= 0x80000000u; // exactly 32 * words bits
    return r;
}

// one copy of each routine under test per field: every call site would otherwise inline the whole group law again
template <class F>
__attribute__((noinline)) static void mul(Xyzz<F> &acc, const Xyzz<F> &b, const uint32_t (&k)[SCALAR_WORDS], unsigned len)
{
    scalar_mul(acc, b, k, len);
}
template <class F>
__attribute__((noinline)) static void add_wire(Xyzz<F> &acc, const uint32_t *wire)
{
    add_affine_wire(acc, wire);
}

template <class F, class Fr>
static void run_curve(const CurveText &text)
{
    const char *name = text.name;
    const Curve<F> c = make_curve<F, Fr>(text);
    CHECK(ec_mul(c.r, c.g, c.p).inf, "%s: order of the generator", name);
    Big seed = random_words(7);
    const Pt P = ec_mul(seed, c.g, c.p), Q = ec_mul(Big(11), c.g, c.p);
    Xyzz<F> id;
    xyzz_set_identity(id);

    Big top, single;
    top.w[(c.r_bits - 1) >> 5] = 1u << ((c.r_bits - 1) & 31);
    single.w[77 >> 5] = 1u << (77 & 31);
    const Big ks[] = {Big(), Big(1), Big(2), sub(c.r, Big(1)), add(top, Big(5)), single, random_words(2), random_words(4)};
    const int want_bits[] = {0, 1, 2, c.r_bits, c.r_bits, 78, 64, 128};
    for (int ki = 0; ki < 8; ki++) {
        const Big &k = ks[ki];
        CHECK(cmp(k, c.r) < 0, "%s: scalar range", name);
        uint32_t kw[SCALAR_WORDS];
        scalar_words(kw, k);
        const unsigned own = scalar_bits(kw);
        CHECK((int)own == want_bits[ki] && (int)own == bits(k), "%s: scalar_bits of scalar %d", name, ki);
        const Pt kP = ec_mul(k, P, c.p);
        const Xyzz<F> forms[2] = {from_ref(P, c), projective_form(P, c)};
        for (unsigned len = own; len <= 256; len++) {
            Xyzz<F> t;
            mul(t, forms[len & 1], kw, len);
            CHECK(same(to_ref(t, c), kP), "%s: scalar %d over %u bits", name, ki, len);
            check_stored(t, c, "scalar_mul");
            Xyzz<F> o;
            mul(o, id, kw, len);
            CHECK(xyzz_is_identity(o), "%s: scalar %d times the identity over %u bits", name, ki, len);
        }
        // the addend: the identity, a generic point, k P itself and -k P, after the shortest and the longest loop
        const Pt addends[] = {Pt(), Q, kP, neg(kP, c.p)};
        for (unsigned len : {own, 256u}) {
            for (int ai = 0; ai < 4; ai++) {
                for (int form = 0; form < 2; form++) {
                    Xyzz<F> t;
                    mul(t, forms[form], kw, len);
                    uint32_t aw[2 * F::L];
                    affine_wire<F>(aw, addends[ai], c);
                    if (addends[ai].inf) aw[F::L] = 7; // x == 0 alone marks the identity
                    add_wire(t, aw);
                    CHECK(same(to_ref(t, c), ec_add(addends[ai], kP, c.p)), "%s: scalar %d addend %d", name, ki, ai);
                    if (ai == 3) CHECK(xyzz_is_identity(t), "%s: A = -k P leaves the identity", name);
                    check_stored(t, c, "add_affine_wire");
                }
                Xyzz<F> o;
                mul(o, id, kw, len);
                uint32_t aw[2 * F::L];
                affine_wire<F>(aw, addends[ai], c);
                add_wire(o, aw);
                CHECK(same(to_ref(o, c), addends[ai]), "%s: the identity times scalar %d, addend %d", name, ki, ai);
                check_stored(o, c, "add_affine_wire over the identity");
            }
        }
    }
    {
        uint32_t kw[SCALAR_WORDS];
        scalar_words(kw, sub(c.r, Big(1)));
        Xyzz<F> t;
        mul(t, from_ref(Q, c), kw, scalar_bits(kw));
        CHECK(same(to_ref(t, c), neg(Q, c.p)), "%s: (r - 1) P = -P", name);
    }

    // scalars: the wire residue to the integer, and c s^i
    Big Rr(1);
    for (int i = 0; i < 256; i++) Rr = mod_add(Rr, Rr, c.r);
    auto fr_wire = [&](uint32_t (&w)[SCALAR_WORDS], const Big &v) { scalar_words(w, mod_mul(v, Rr, c.r)); };
    const Big values[] = {Big(), Big(1), sub(c.r, Big(1)), random_words(4), mod_mul(random_words(7), random_words(7), c.r)};
    for (const Big &v : values) {
        uint32_t wire[SCALAR_WORDS], out[SCALAR_WORDS], want[SCALAR_WORDS];
        fr_wire(wire, v);
        scalar_from_wire<Fr>(out, wire);
        scalar_words(want, v);
        CHECK(memcmp(out, want, sizeof out) == 0, "%s: scalar_from_wire", name);
    }
    const Big cs[][2] = {{Big(1), Big(1)}, {Big(3), Big(5)}, {values[4], mod_mul(random_words(6), random_words(7), c.r)}, {Big(), values[3]}, {values[3], Big()}};
    for (const auto &pair : cs) {
        uint32_t wire[SCALAR_WORDS];
        Fe<Fr> fc, fs;
        fr_wire(wire, pair[0]);
        fe_from_wire(fc, wire);
        fr_wire(wire, pair[1]);
        fe_from_wire(fs, wire);
        PowerTable<Fr> table;
        power_table(table, fc, fs);
        for (uint32_t i : {0u, 1u, (1u << 27) + 5u, (1u << 28) - 1u}) {
            uint32_t out[SCALAR_WORDS], want[SCALAR_WORDS];
            power_scalar(out, table, i);
            scalar_words(want, mod_mul(pair[0], mod_pow(pair[1], Big(i), c.r), c.r));
            CHECK(memcmp(out, want, sizeof out) == 0, "%s: c s^%u", name, i);
        }
    }
    CHECK(mul_blocks(1) == 1 && mul_blocks(64) == 1 && mul_blocks(65) == 2 && mul_blocks((u64)1 << 28) == (u64)1 << 22, "mul_blocks");
    CHECK(norm_blocks(1) == 1 && norm_blocks(4096) == 1 && norm_blocks(4097) == 2 && norm_blocks((u64)1 << 28) == (u64)1 << 16, "norm_blocks");
}

int main()
{
    g_rng = 0xD1B54A32D192ED03ull;
    run_curve<Bn254Fq, Bn254Fr>(BN254);
    run_curve<Bls377Fq, Bls377Fr>(BLS12_377);
    run_curve<Bls381Fq, Bls381Fr>(BLS12_381);
    printf("ok %ld\n", g_checks);
    return 0;
}
