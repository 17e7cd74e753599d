// kzg_open_all.hip -- KZG proofs of one polynomial at all n points of its domain by Feist-Khovratovich (panda_kzg_open_all_setup,
// panda_kzg_open_all, panda_kzg_open_all_plan); DESIGN.md 5.10.  With f the n coefficients, s_i = [tau^i]G and w = omega2^2:
//   proof_k = commitment to (f(X) - f(w^k)) / (X - w^k) = sum_m w^(km) h_m,     h_m = sum_{i <= n - 2 - m} f_(m + 1 + i) s_i,  h_(n - 1) = O
// and h_m is entry n - 1 + m of the linear convolution of f with s'_j = s_(n - 2 - j), j <= n - 2: 2n - 2 entries, so the cyclic
// convolution of length 2n does not wrap.  The call composes the library's own entry points:
//   setup   k_reverse_pad: s' and n + 1 identities into d_table; panda_ec_ntt forward of 2n points in place (once per SRS and size)
//   open    k_pad_coeffs: f and n zeros; panda_ntt_execute_batch forward of 2n scalars (one member); panda_points_scalar_mul EACH against
//           d_table; panda_ec_ntt inverse of 2n points in place; k_take_middle: entries n - 1 .. 2n - 3 and one identity into d_proofs;
//           panda_ec_ntt forward of n points with omega2^2 in place in d_proofs
// The temporaries live in the caller's d_work: panda_ec_ntt and panda_points_scalar_mul take the calling thread's arena themselves.
//   d_work = [2n scalars | 2n points].  The scalar transform leaves its result in its source or its destination by the parity of its
// passes, and the point region is large enough to be the other buffer: the padded coefficients go to whichever of the two makes the
// result land in the scalar region.
#include <string.h>

#include "ec_ntt.h"
#include "fe29.h"
#include "panda_internal.h"
#include "point_vec.h"
#include "poly_elem.h"

using namespace panda29;
using panda_ecntt::affine_bytes;
using panda_ecntt::SCALAR_WORDS;
using panda_poly::ranges_overlap;
typedef uint64_t u64;

namespace {

constexpr unsigned MAX_LOG_N = PANDA_EC_NTT_MAX_LOG_N - 1; // 2n within the EC-NTT's cap
constexpr unsigned COPY_THREADS = 256;

// out[j] = s'_j = srs[n - 2 - j] for j <= n - 2, all-zero bytes (the identity) for n - 1 <= j < 2n; V uint4 per point
template <int V>
__global__ void __launch_bounds__(COPY_THREADS) k_reverse_pad(const uint4 *__restrict__ srs, uint4 *__restrict__ out, u64 n)
{
    const u64 j = (u64)blockIdx.x * COPY_THREADS + threadIdx.x;
    if (j >= 2 * n) return;
#pragma unroll
    for (int v = 0; v < V; v++) out[j * V + v] = j + 2 <= n ? srs[(n - 2 - j) * V + v] : make_uint4(0, 0, 0, 0);
}

// out[j] = f_j for j < n, zero for n <= j < 2n; two uint4 per scalar
__global__ void __launch_bounds__(COPY_THREADS) k_pad_coeffs(const uint4 *__restrict__ coeffs, uint4 *__restrict__ out, u64 n)
{
    const u64 j = (u64)blockIdx.x * COPY_THREADS + threadIdx.x;
    if (j >= 2 * n) return;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    out[2 * j] = j < n ? coeffs[2 * j] : zero;
    out[2 * j + 1] = j < n ? coeffs[2 * j + 1] : zero;
}

// proofs[m] = conv[n - 1 + m] for m <= n - 2, the identity for m = n - 1
template <int V>
__global__ void __launch_bounds__(COPY_THREADS) k_take_middle(const uint4 *__restrict__ conv, uint4 *__restrict__ proofs, u64 n)
{
    const u64 m = (u64)blockIdx.x * COPY_THREADS + threadIdx.x;
    if (m >= n) return;
#pragma unroll
    for (int v = 0; v < V; v++) proofs[m * V + v] = m + 1 < n ? conv[(n - 1 + m) * V + v] : make_uint4(0, 0, 0, 0);
}

size_t work_bytes_of(unsigned curve, unsigned log_n) { return panda::align256(((size_t)2 << log_n) * (32 + affine_bytes(curve))); }
unsigned copy_blocks(u64 items) { return (unsigned)((items + COPY_THREADS - 1) / COPY_THREADS); }

// omega2 below the modulus and of order exactly 2n (omega2^n == -1), as panda_ec_ntt checks its root; *omega = omega2^2 on the wire
bool roots_valid(unsigned curve, const void *omega2, unsigned log_n, u32 (&w2)[SCALAR_WORDS], u32 (&w)[SCALAR_WORDS])
{
    memcpy(w2, omega2, sizeof w2);
    return panda_poly::with_field(curve, [&](auto fr) {
        typedef decltype(fr) Fr;
        if (!panda_poly::wire_below_modulus<Fr>(w2)) return false;
        Fe<Fr> root, t;
        fe_from_wire(root, w2);
        fe_sqr(t, root);
        fe_to_wire(w, t);
        return panda_ecntt::order_is_pow2(root, log_n + 1); // omega2^n == -1
    });
}

bool shape_invalid(unsigned curve, unsigned log_n) { return curve > 2 || log_n == 0 || log_n > MAX_LOG_N; }

unsigned scalar_passes(unsigned log_n)
{
    unsigned passes = 0;
    panda_ntt_batch_plan(log_n + 1, PANDA_NTT_FORWARD, 1, &passes, nullptr);
    return passes;
}

#define KZG_TRY(expr)                                   \
    do {                                                \
        const panda_error kzg_err__ = (panda_error)(expr); \
        if (kzg_err__ != panda_success) return kzg_err__; \
    } while (0)

} // namespace

extern "C" {

// The calls: see include/panda_interface.h.  Every check comes before any runtime call.
panda_error panda_kzg_open_all_setup(unsigned curve, const void *d_srs, unsigned log_n, const void *omega2, void *d_table, panda_stream stream)
{
    if (shape_invalid(curve, log_n) || !d_srs || !omega2 || !d_table) return panda_error_invalid_value;
    const u64 n = (u64)1 << log_n;
    const size_t pb = affine_bytes(curve), srs_bytes = n * pb, table_bytes = 2 * n * pb;
    if (ranges_overlap(d_srs, srs_bytes, d_table, table_bytes)) return panda_error_invalid_value;
    if (panda::extent_too_short(d_srs, srs_bytes) || panda::extent_too_short(d_table, table_bytes)) return panda_error_invalid_value;
    u32 w2[SCALAR_WORDS], w[SCALAR_WORDS];
    if (!roots_valid(curve, omega2, log_n, w2, w)) return panda_error_invalid_value;
    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    KZG_TRY(panda::order_after_null_stream(s));
    if (curve == 0)
        hipLaunchKernelGGL((k_reverse_pad<4>), dim3(copy_blocks(2 * n)), dim3(COPY_THREADS), 0, s, (const uint4 *)d_srs, (uint4 *)d_table, n);
    else
        hipLaunchKernelGGL((k_reverse_pad<6>), dim3(copy_blocks(2 * n)), dim3(COPY_THREADS), 0, s, (const uint4 *)d_srs, (uint4 *)d_table, n);
    KZG_TRY(hipGetLastError());
    return panda_ec_ntt(curve, d_table, d_table, log_n + 1, PANDA_EC_NTT_FORWARD, w2, stream);
}

panda_error panda_kzg_open_all(unsigned curve, const void *d_coeffs, const void *d_table, unsigned log_n, const void *omega2, void *d_work, size_t work_bytes,
                               void *d_proofs, panda_stream stream)
{
    if (shape_invalid(curve, log_n) || !d_coeffs || !d_table || !omega2 || !d_work || !d_proofs) return panda_error_invalid_value;
    const u64 n = (u64)1 << log_n;
    const size_t pb = affine_bytes(curve), need = work_bytes_of(curve, log_n);
    if (work_bytes < need) return panda_error_invalid_value;
    const struct {
        const void *p;
        size_t bytes;
    } buf[4] = {{d_coeffs, (size_t)n * 32}, {d_table, (size_t)2 * n * pb}, {d_work, need}, {d_proofs, (size_t)n * pb}};
    for (int a = 0; a < 4; a++) {
        for (int b = a + 1; b < 4; b++)
            if (ranges_overlap(buf[a].p, buf[a].bytes, buf[b].p, buf[b].bytes)) return panda_error_invalid_value;
        if (panda::extent_too_short(buf[a].p, buf[a].bytes)) return panda_error_invalid_value;
    }
    u32 w2[SCALAR_WORDS], w[SCALAR_WORDS];
    if (!roots_valid(curve, omega2, log_n, w2, w)) return panda_error_invalid_value;

    hipStream_t s = static_cast<hipStream_t>(stream.handle);
    char *scalars = (char *)d_work, *points = scalars + 2 * n * 32; // 2n scalars, 2n points
    const bool via_points = (scalar_passes(log_n) & 1u) != 0;       // the transform ends in its destination: start in the point region
    KZG_TRY(panda::order_after_null_stream(s));
    hipLaunchKernelGGL(k_pad_coeffs, dim3(copy_blocks(2 * n)), dim3(COPY_THREADS), 0, s, (const uint4 *)d_coeffs, (uint4 *)(via_points ? points : scalars), n);
    KZG_TRY(hipGetLastError());
    unsigned flag = 0;
    panda_ntt_configuration_v1 cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.stream = stream;
    cfg.d_src = via_points ? points : scalars;
    cfg.d_dst = via_points ? scalars : points;
    cfg.d_omega = w2;
    cfg.log_n = log_n + 1;
    cfg.flag = &flag;
    KZG_TRY(panda_ntt_execute_batch(curve, PANDA_NTT_FORWARD, cfg, 1, nullptr));
    if (flag != (via_points ? 1u : 0u)) return panda_error_invalid_value; // the plan and the call disagree: not reachable
    KZG_TRY(panda_points_scalar_mul(curve, PANDA_POINTS_MUL_EACH, d_table, scalars, nullptr, nullptr, points, 2 * n, stream));
    KZG_TRY(panda_ec_ntt(curve, points, points, log_n + 1, PANDA_EC_NTT_INVERSE, w2, stream));
    if (curve == 0)
        hipLaunchKernelGGL((k_take_middle<4>), dim3(copy_blocks(n)), dim3(COPY_THREADS), 0, s, (const uint4 *)points, (uint4 *)d_proofs, n);
    else
        hipLaunchKernelGGL((k_take_middle<6>), dim3(copy_blocks(n)), dim3(COPY_THREADS), 0, s, (const uint4 *)points, (uint4 *)d_proofs, n);
    KZG_TRY(hipGetLastError());
    return panda_ec_ntt(curve, d_proofs, d_proofs, log_n, PANDA_EC_NTT_FORWARD, w, stream);
}

panda_error panda_kzg_open_all_plan(unsigned curve, unsigned log_n, size_t *work_bytes, unsigned *launches)
{
    if (shape_invalid(curve, log_n)) return panda_error_invalid_value;
    if (work_bytes) *work_bytes = work_bytes_of(curve, log_n);
    if (launches) {
        unsigned mul = 0, inverse = 0, forward = 0;
        panda_points_scalar_mul_plan(curve, PANDA_POINTS_MUL_EACH, (u64)2 << log_n, &mul, nullptr);
        panda_ec_ntt_plan(curve, log_n + 1, PANDA_EC_NTT_INVERSE, &inverse, nullptr, nullptr);
        panda_ec_ntt_plan(curve, log_n, PANDA_EC_NTT_FORWARD, &forward, nullptr, nullptr);
        *launches = 1 + scalar_passes(log_n) + mul + inverse + 1 + forward; // the pad and the middle copy are the composite's own
    }
    return panda_success;
}

} // extern "C"
