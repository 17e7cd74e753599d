// poly_sum.h -- the additions of panda_poly_running_sum (poly_sum.hip), kept apart from the kernels so that a host program can run them
// (tests/host_check/lookup_host.cpp, under FE29_CHECK).  DESIGN.md 5.6.
//
// Bounds (contract at the top of fe29.h; the three scalar fields have nine limbs and p < 2^255):
//   loaded element    fe_unpack of a canonical residue                          tight, < p
//   add_canon(a, b)   a, b canonical: limb-wise sum, limbs < 2^30, value < 2p;  fe_carry (carries <= 1) -> tight; fe_reduce_once
//                                                                               canonical, < p
//   sum_run<E>        E <= RUN_MAX = 7 canonical elements added limb-wise, no carries: limbs 0..7 <= 7 (2^29 - 1) < 2^32 - 8, the top
//                     limb < 7 2^24, value < 7p < 2^9 p: what fe_reduce_small takes -> canonical, < p
// Every value that crosses a lane, LDS or memory is canonical, so the number of elements, tiles and chunks does not enter.
#pragma once
#include "fe29.h"

namespace panda_poly {

using panda29::Fe;

constexpr int RUN_MAX = 7; // elements sum_run may add before it reduces

// a, b canonical -> a + b canonical
template <class Fr>
PANDA_HD void add_canon(Fe<Fr> &r, const Fe<Fr> &a, const Fe<Fr> &b)
{
    Fe<Fr> t;
    panda29::fe_add_nr(t, a, b);
    panda29::fe_carry(t);
    panda29::fe_reduce_once(t);
    r = t;
}
// the sum of E <= RUN_MAX canonical elements, canonical
template <class Fr, int E>
PANDA_HD void sum_run(Fe<Fr> &g, const Fe<Fr> (&x)[E])
{
    static_assert(E >= 1 && E <= RUN_MAX, "sum_run: limbs must stay below 2^32 - 8");
    Fe<Fr> t = x[0];
#pragma unroll
    for (int e = 1; e < E; e++) panda29::fe_add_nr(t, t, x[e]);
    panda29::fe_reduce_small(t);
    g = t;
}

} // namespace panda_poly
