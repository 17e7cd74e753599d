// xcd_remap.h -- which tile a workgroup of a tile kernel takes, so that the workgroups that share an XCD take neighbouring tiles.
//
// The dispatcher deals the workgroups of a launch round-robin over the chip's eight XCDs (linear id mod 8: tools/xcd_map.hip), and each
// XCD has an L2 of its own.  In the scatter kernels of the bucket sort tile t's run of a partition ends exactly where tile t + 1's begins,
// so with tile = workgroup id the two halves of every boundary line are dirtied in two different L2s.  With this map the workgroups
// id = x, x + 8, x + 16, ... -- one XCD's -- take a contiguous range of tiles, in the order they are dispatched.
// A bijection of [0, nwg) for every nwg >= 1 (tests/test_msm_tail_shapes.py checks the host build of this very function): the first
// nwg mod 8 classes hold one workgroup more than the others.  Plain C++: included by the HIP sources and by the host check.
#pragma once

#if defined(__HIPCC__)
#define PANDA_XCD_HD __host__ __device__ __forceinline__
#else
#define PANDA_XCD_HD inline
#endif

namespace panda {

constexpr unsigned XCDS = 8;

PANDA_XCD_HD unsigned xcd_remap(unsigned id, unsigned nwg)
{
    const unsigned cls = id % XCDS, idx = id / XCDS; // cls labels the workgroups that share an XCD, not the XCD's number
    const unsigned q = nwg / XCDS, r = nwg % XCDS;
    const unsigned first = cls < r ? cls * (q + 1) : r * (q + 1) + (cls - r) * q;
    return first + idx;
}

} // namespace panda
