// Host check of the signed-limb field operations (fe29.h, "Signed contract") and of the signed mixed addition (curve29.h,
// xyzz_madd_core_s) for BN254 Fq.  A program of its own: tests/test_fe29_signed_host.py builds it with the host compiler and FE29_CHECK
// (wide signed shadow of every column, limb-class asserts), feeds it operands at the edges of the contract and compares what it
// writes with Python's integers.  It is also the thing to build with -fsanitize=address,undefined: nothing here touches a GPU.
//
//   fe29_signed_host <op> <in> <out>      op = mul | sqr | muladd | sub | norm | unsign<K> | zero
//       in: records of four operands a, b, c, d of N int32 limbs each; out: N int32 limbs per record (zero: one int32)
//   fe29_signed_host chain <in> <out>
//       in: records of 2 N uint32 limbs, rows (x, y) in internal form, canonical; a row of zeros is the identity
//       out: per step the signed accumulator, the unsigned accumulator and the signed one as a reader converts it (3 x 4 N limbs)
#define FE29_CHECK 1
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../panda_amd/csrc/curve29.h"

using namespace panda29;
typedef Bn254Fq F;
constexpr int N = F::N;

static std::vector<uint32_t> read_all(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        perror(path);
        exit(2);
    }
    std::vector<uint32_t> v;
    uint32_t buf[4096];
    size_t n;
    while ((n = fread(buf, 4, 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static void write_all(const char *path, const std::vector<uint32_t> &v)
{
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(v.data(), 4, v.size(), f) != v.size()) {
        perror(path);
        exit(2);
    }
    fclose(f);
}

static Fe<F> fe_at(const std::vector<uint32_t> &v, size_t off)
{
    Fe<F> r;
    for (int i = 0; i < N; i++) r.l[i] = v[off + i];
    return r;
}

static void put(std::vector<uint32_t> &o, const Fe<F> &a)
{
    for (int i = 0; i < N; i++) o.push_back(a.l[i]);
}

static void put(std::vector<uint32_t> &o, const Xyzz<F> &p)
{
    put(o, p.X);
    put(o, p.Y);
    put(o, p.ZZ);
    put(o, p.ZZZ);
}

// the output classes of the contract
static void check_s_tight(const Fe<F> &a)
{
    for (int i = 0; i < N - 1; i++) assert(a.l[i] < (1u << 29) && "s-tight: lower limb outside [0, 2^29)");
}
static void check_s_loose(const Fe<F> &a)
{
    for (int i = 0; i < N - 1; i++) assert((int32_t)a.l[i] >= -3 && (int32_t)a.l[i] < (1 << 29) + 1 && "s-loose: lower limb outside [-3, 2^29 + 1)");
}
static void check_loose(const Fe<F> &a)
{
    for (int i = 0; i < N - 1; i++) assert(a.l[i] <= (1u << 29) + 8 && "loose: lower limb above 2^29 + 8");
    assert((int32_t)a.l[N - 1] >= 0 && "loose: negative top limb");
}

template <int K>
static void unsign(Fe<F> &r, const Fe<F> &a)
{
    fe_from_signed<F, K>(r, a);
    check_loose(r);
}

static int run_op(const char *op, const char *in, const char *out)
{
    const std::vector<uint32_t> v = read_all(in);
    const size_t recs = v.size() / (4 * N);
    std::vector<uint32_t> o;
    for (size_t k = 0; k < recs; k++) {
        const Fe<F> a = fe_at(v, k * 4 * N), b = fe_at(v, k * 4 * N + N), c = fe_at(v, k * 4 * N + 2 * N), d = fe_at(v, k * 4 * N + 3 * N);
        Fe<F> r;
        if (!strcmp(op, "mul")) {
            fe_mul_s(r, a, b);
            check_s_tight(r);
        } else if (!strcmp(op, "sqr")) {
            fe_sqr_s(r, a);
            check_s_tight(r);
        } else if (!strcmp(op, "muladd")) {
            fe_mul_add_s(r, a, b, c, d);
            check_s_tight(r);
        } else if (!strcmp(op, "sub"))
            fe_sub_s(r, a, b);
        else if (!strcmp(op, "norm")) {
            fe_norm_s(r, a);
            check_s_loose(r);
        } else if (!strcmp(op, "unsign1"))
            unsign<1>(r, a);
        else if (!strcmp(op, "unsign4"))
            unsign<4>(r, a);
        else if (!strcmp(op, "zero")) {
            o.push_back(fe_is_zero_mod_p_s(a) ? 1u : 0u);
            continue;
        } else {
            fprintf(stderr, "unknown op %s\n", op);
            return 2;
        }
        put(o, r);
    }
    write_all(out, o);
    return 0;
}

// The loop of accumulate_chunk around the addition, for one bucket: identity rows are skipped, a row that meets an identity
// accumulator becomes the accumulator, rare == 1 doubles the row (and, signed, brings X back under its bound), rare == 2 is the identity.
template <bool SIGNED>
static void step(Xyzz<F> &acc, bool &id, const Fe<F> &x, const Fe<F> &y, bool inf)
{
    if (inf) return;
    if (id) {
        xyzz_from_affine(acc, x, y);
        id = false;
        return;
    }
    const int rare = SIGNED ? xyzz_madd_core_s(acc, x, y) : xyzz_madd_core(acc, x, y);
    if (rare == 1) {
        xyzz_dbl_affine(acc, x, y);
        if (SIGNED) signed_after_doubling(acc);
        id = xyzz_is_identity(acc);
    } else if (rare == 2) {
        xyzz_set_identity(acc);
        id = true;
    }
}

static int run_chain(const char *in, const char *out)
{
    typedef SignedBounds<F> SB;
    const std::vector<uint32_t> v = read_all(in);
    const size_t rows = v.size() / (2 * N);
    std::vector<uint32_t> o;
    Xyzz<F> s, u;
    xyzz_set_identity(s);
    xyzz_set_identity(u);
    bool sid = true, uid = true;
    for (size_t k = 0; k < rows; k++) {
        const Fe<F> x = fe_at(v, k * 2 * N), y = fe_at(v, k * 2 * N + N);
        const bool inf = fe_all_zero(x) && fe_all_zero(y);
        step<true>(s, sid, x, y, inf);
        step<false>(u, uid, x, y, inf);
        assert(sid == uid && "signed and unsigned chains disagree on the identity");
        check_s_loose(s.X);
        check_s_tight(s.Y);
        check_s_tight(s.ZZZ);
        check_s_tight(s.ZZ);
        assert((int32_t)s.ZZ.l[N - 1] >= 0 && s.ZZ.l[N - 1] < (1u << 23) && "ZZ's top limb must leave bit 31 free for the stored mark");
        Xyzz<F> c = s; // what load_xyzz_stored makes of a marked point
        if (!sid) {
            fe_from_signed<F, SB::KX>(c.X, s.X);
            fe_from_signed<F, SB::KY>(c.Y, s.Y);
            fe_from_signed<F, SB::KZZZ>(c.ZZZ, s.ZZZ);
            check_loose(c.X);
            check_loose(c.Y);
            check_loose(c.ZZZ);
        }
        put(o, s);
        put(o, u);
        put(o, c);
    }
    write_all(out, o);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: %s <op> <in> <out>\n", argv[0]);
        return 2;
    }
    if (!strcmp(argv[1], "chain")) return run_chain(argv[2], argv[3]);
    return run_op(argv[1], argv[2], argv[3]);
}
